// head.cuh -- kernels of the net head (dfx_head_* of include/dfx.h; gfx950): channel top-k / argmax and softmax over a
// row matrix.  HBM-bound work, no MFMA.
//
// TOP-K.  Every element becomes ONE unsigned 64-bit number, (key << 32) | (0xffffffff - channel), where `key` is the
// element mapped monotonically onto u32 (u8 as is; s8 / s32 with the sign bit flipped; f32 by IEEE totalOrder: negative
// patterns inverted, others with the sign bit set).  "Larger value first, lower channel first among equals" is then plain
// `>` on distinct numbers, so a sequential scan, a per-lane scan followed by a wave butterfly, and any other tree give the
// same k numbers in the same order.  0 is below every real element (the low half of a real one is at least 0xffff0001)
// and marks an empty slot.  val is read back from src at the winning channel: the element's bits, verbatim.
//
// SOFTMAX (1-byte src).  In key space both dtypes are 0 .. 255, and m - src[k] = key(m) - key(src[k]).  The sum of table
// entries is an exact u32 (dfx_head_set_table refuses a table that could overflow it), so its order does not matter; the
// probability is float(E) / float(S), one correctly rounded division, computed by head_prob() on every path.
//
//   head_generic_*   one thread per row, sequential, any alignment: defines the arithmetic
//   head_row_*       a wave per row, four rows per workgroup.  A lane scans the 16-byte groups lane, lane + 64, ...; the
//                    lanes meet through __shfl_xor butterflies (no LDS for top-k).  Top-k with k > 1: every lane keeps its
//                    own sorted list of 8, then k rounds of "wave maximum of the list heads, the owner pops".  Softmax keeps
//                    a lane's first group in a register over its three passes (max, sum, store), i.e. the whole row for
//                    c <= 1024, and re-reads further groups, which are in L2.
//   head_pixel_*     a lane per row (src_ld <= 160 bytes, a multiple of 16).  16-byte loads; the first four groups of a
//                    row (src_ld <= 64) stay in registers for softmax, further ones are re-read.  One-byte results of four
//                    neighbouring lanes meet in one dword through __shfl_down, so a wave stores 16 dwords, not 64 bytes.
#pragma once

#include "dfx_device.cuh"

namespace dfx {

struct HeadArgs {
  const unsigned char *src;
  unsigned char *out;          // idx (TOPK) or dst (SOFTMAX)
  unsigned char *val;          // TOPK: val or null
  const unsigned int *table;   // SOFTMAX: the handle's device copy of E
  long long rows;
  int c, src_ld, out_ld, k;
  int src_dt, out_dt;
  int out_vec;                 // SOFTMAX: every dst row starts on a 16-byte boundary (16-byte stores for whole groups)
  float out_scale;
};

__device__ __forceinline__ unsigned head_key32(unsigned bits, int dt) {  // s32 / f32
  if (dt == DFX_S32) return bits ^ 0x80000000u;
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
__device__ __forceinline__ unsigned head_key8(unsigned byte, int dt) { return dt == DFX_U8 ? byte : (byte ^ 0x80u); }
__device__ __forceinline__ unsigned long long head_pair(unsigned key, int ch) {
  return ((unsigned long long)key << 32) | (0xffffffffu - (unsigned)ch);
}
__device__ __forceinline__ int head_pair_channel(unsigned long long p) { return (int)(0xffffffffu - (unsigned)p); }

__device__ __forceinline__ float head_prob(unsigned e, float fs) { return __fdiv_rn(__uint2float_rn(e), fs); }
// the reorder's conversion to u8: rint (ties to even), NaN -> 0, clamp
__device__ __forceinline__ int head_cvt_u8(float p, float out_scale) {
  const float v = __fmul_rn(p, out_scale);
  float r = __builtin_rintf(v);
  r = (v != v) ? 0.0f : r;
  r = r < 0.0f ? 0.0f : (r > 255.0f ? 255.0f : r);
  return (int)r;
}

// ---- shared with attn.cuh (the fused attention's softmax in LDS): byte access and the wave reductions -----------------------
__device__ __forceinline__ unsigned head_byte(const v4i &raw, int e) { return ((unsigned)raw[e >> 2] >> (8 * (e & 3))) & 0xffu; }

__device__ __forceinline__ unsigned long long head_wave_max(unsigned long long x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned long long o = __shfl_xor(x, m);
    x = o > x ? o : x;
  }
  return x;
}
__device__ __forceinline__ unsigned head_wave_max(unsigned x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned o = (unsigned)__shfl_xor((int)x, m);
    x = o > x ? o : x;
  }
  return x;
}
__device__ __forceinline__ unsigned head_wave_sum(unsigned x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x += (unsigned)__shfl_xor((int)x, m);
  return x;
}

// the same over aligned groups of W consecutive lanes (W a power of two <= 64): every lane of a group gets the group's result
template <int W>
__device__ __forceinline__ unsigned head_lanes_max(unsigned x) {
#pragma unroll
  for (int m = W / 2; m >= 1; m >>= 1) {
    const unsigned o = (unsigned)__shfl_xor((int)x, m);
    x = o > x ? o : x;
  }
  return x;
}
template <int W>
__device__ __forceinline__ unsigned head_lanes_sum(unsigned x) {
#pragma unroll
  for (int m = W / 2; m >= 1; m >>= 1) x += (unsigned)__shfl_xor((int)x, m);
  return x;
}

#ifdef DFX_HEAD_KERNELS

// the K best pairs seen so far, best first
template <int K>
struct HeadList {
  unsigned long long b[K];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int j = 0; j < K; ++j) b[j] = 0;
  }
  __device__ __forceinline__ void insert(unsigned long long x) {
    if (x > b[K - 1]) {
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const unsigned long long lo = x > b[j] ? b[j] : x;
        b[j] = x > b[j] ? x : b[j];
        x = lo;
      }
    }
  }
  __device__ __forceinline__ void pop() {
#pragma unroll
    for (int j = 0; j + 1 < K; ++j) b[j] = b[j + 1];
    b[K - 1] = 0;
  }
};

// result t of `row`: the pair's channel into idx, the element at that channel into val
__device__ __forceinline__ void head_emit(const HeadArgs &a, long long row, int t, unsigned long long pair) {
  const int ch = head_pair_channel(pair);
  const size_t o = (size_t)row * a.out_ld + t;
  if (a.out_dt == DFX_U8) a.out[o] = (unsigned char)ch;
  else reinterpret_cast<int *>(a.out)[o] = ch;
  if (a.val) {
    const size_t s = (size_t)row * a.src_ld + ch;
    if (a.src_dt == DFX_U8 || a.src_dt == DFX_S8) a.val[o] = a.src[s];
    else reinterpret_cast<unsigned *>(a.val)[o] = reinterpret_cast<const unsigned *>(a.src)[s];
  }
}

// ---- generic: one thread per row --------------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(256) void head_generic_topk_kernel(HeadArgs a) {
  const long long stride = (long long)gridDim.x * 256;
  const bool wide = a.src_dt == DFX_S32 || a.src_dt == DFX_F32;
  for (long long row = (long long)blockIdx.x * 256 + threadIdx.x; row < a.rows; row += stride) {
    const size_t base = (size_t)row * a.src_ld;
    HeadList<K> l;
    l.clear();
    for (int j = 0; j < a.c; ++j) {
      const unsigned key = wide ? head_key32(reinterpret_cast<const unsigned *>(a.src)[base + j], a.src_dt) : head_key8(a.src[base + j], a.src_dt);
      l.insert(head_pair(key, j));
    }
#pragma unroll
    for (int t = 0; t < K; ++t)
      if (t < a.k) head_emit(a, row, t, l.b[t]);
  }
}

__global__ __launch_bounds__(256) void head_generic_softmax_kernel(HeadArgs a) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long row = (long long)blockIdx.x * 256 + threadIdx.x; row < a.rows; row += stride) {
    const unsigned char *p = a.src + (size_t)row * a.src_ld;
    unsigned m = 0;
    for (int j = 0; j < a.c; ++j) {
      const unsigned key = head_key8(p[j], a.src_dt);
      m = key > m ? key : m;
    }
    unsigned sum = 0;
    for (int j = 0; j < a.c; ++j) sum += a.table[m - head_key8(p[j], a.src_dt)];
    const float fs = __uint2float_rn(sum);
    const size_t o = (size_t)row * a.out_ld;
    for (int j = 0; j < a.c; ++j) {
      const float pr = head_prob(a.table[m - head_key8(p[j], a.src_dt)], fs);
      if (a.out_dt == DFX_F32) reinterpret_cast<float *>(a.out)[o + j] = pr;
      else a.out[o + j] = (unsigned char)head_cvt_u8(pr, a.out_scale);
    }
  }
}

// ---- shared by the row and the pixel kernels -----------------------------------------------------------------------------

// the probabilities of the 16-byte group `g` of a row whose maximum key is m, stored behind `dst_row` (bytes); only the
// `nvalid` leading channels of the group exist
__device__ __forceinline__ void head_store_group(const HeadArgs &a, const unsigned *tab, unsigned char *dst_row, int g, int nvalid, const v4i &raw,
                                                 unsigned m, float fs) {
  float pr[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const unsigned key = head_key8(head_byte(raw, e), a.src_dt);
    pr[e] = head_prob(tab[e < nvalid ? m - key : 0], fs);  // (a pad byte may exceed the maximum)
  }
  if (a.out_dt == DFX_F32) {
    float *q = reinterpret_cast<float *>(dst_row) + (size_t)g * 16;
    if (a.out_vec && nvalid == 16) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const v4i o = {__float_as_int(pr[4 * v]), __float_as_int(pr[4 * v + 1]), __float_as_int(pr[4 * v + 2]), __float_as_int(pr[4 * v + 3])};
        dfx_store16(reinterpret_cast<v4i *>(q) + v, o);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (e < nvalid) q[e] = pr[e];
    }
  } else {
    unsigned char *q = dst_row + (size_t)g * 16;
    int by[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) by[e] = head_cvt_u8(pr[e], a.out_scale);
    if (a.out_vec && nvalid == 16) {
      v4i o = {0, 0, 0, 0};
#pragma unroll
      for (int e = 0; e < 16; ++e) o[e >> 2] |= by[e] << (8 * (e & 3));
      dfx_store16(reinterpret_cast<v4i *>(q), o);
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (e < nvalid) q[e] = (unsigned char)by[e];
    }
  }
}

// ---- row: a wave per row ---------------------------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(256) void head_row_topk_kernel(HeadArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long stride = (long long)gridDim.x * 4;
  const bool wide = a.src_dt == DFX_S32 || a.src_dt == DFX_F32;
  const int epg = wide ? 4 : 16;                      // elements per 16-byte group
  const int groups = (a.c + epg - 1) / epg;           // (src_ld * element size is a multiple of 16: the last group lies in the row)
  for (long long row = (long long)blockIdx.x * 4 + wave; row < a.rows; row += stride) {
    const v4i *p = reinterpret_cast<const v4i *>(a.src + (size_t)row * a.src_ld * (wide ? 4 : 1));
    HeadList<K> l;
    l.clear();
    for (int g = lane; g < groups; g += 64) {
      const v4i raw = p[g];
      if (wide) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int j = g * 4 + e;
          if (j < a.c) l.insert(head_pair(head_key32((unsigned)raw[e], a.src_dt), j));
        }
      } else {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int j = g * 16 + e;
          if (j < a.c) l.insert(head_pair(head_key8(head_byte(raw, e), a.src_dt), j));
        }
      }
    }
    // k rounds: the wave's best list head is the next result; its owner (pairs are distinct) moves on
    unsigned long long mine = 0;
#pragma unroll
    for (int t = 0; t < K; ++t) {
      if (t < a.k) {
        const unsigned long long top = head_wave_max(l.b[0]);
        if (K > 1 && l.b[0] == top) l.pop();
        if (lane == t) mine = top;
      }
    }
    if (lane < a.k) head_emit(a, row, lane, mine);
  }
}

__global__ __launch_bounds__(256) void head_row_softmax_kernel(HeadArgs a) {
  __shared__ unsigned tab[256];
  tab[threadIdx.x] = a.table[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long stride = (long long)gridDim.x * 4;
  const int groups = (a.c + 15) / 16;
  const int osz = a.out_dt == DFX_F32 ? 4 : 1;
  for (long long row = (long long)blockIdx.x * 4 + wave; row < a.rows; row += stride) {
    const v4i *p = reinterpret_cast<const v4i *>(a.src + (size_t)row * a.src_ld);
    const v4i zero = {0, 0, 0, 0};
    const v4i keep = lane < groups ? p[lane] : zero;  // the lane's first group stays here over the three passes
    unsigned m = 0;
    for (int g = lane; g < groups; g += 64) {
      const v4i raw = g == lane ? keep : p[g];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const unsigned key = head_key8(head_byte(raw, e), a.src_dt);
        if (g * 16 + e < a.c) m = key > m ? key : m;
      }
    }
    m = head_wave_max(m);
    unsigned sum = 0;
    for (int g = lane; g < groups; g += 64) {
      const v4i raw = g == lane ? keep : p[g];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const unsigned key = head_key8(head_byte(raw, e), a.src_dt);
        if (g * 16 + e < a.c) sum += tab[m - key];
      }
    }
    const float fs = __uint2float_rn(head_wave_sum(sum));
    unsigned char *dst_row = a.out + (size_t)row * a.out_ld * osz;
    for (int g = lane; g < groups; g += 64) {
      const v4i raw = g == lane ? keep : p[g];
      const int left = a.c - g * 16;
      head_store_group(a, tab, dst_row, g, left < 16 ? left : 16, raw, m, fs);
    }
  }
}

// ---- pixel: a lane per row ---------------------------------------------------------------------------------------------------
// One byte per lane, rows `row` of consecutive lanes consecutive: the four bytes of an aligned quad of lanes leave as one
// dword where all four rows exist (q is 4-byte aligned and the wave's first row is a multiple of 64), else byte by byte.
// Every lane of the wave calls this, active or not.
__device__ __forceinline__ void head_store_quads(unsigned char *q, long long row, long long rows, int byte) {
  const int b1 = __shfl_down(byte, 1), b2 = __shfl_down(byte, 2), b3 = __shfl_down(byte, 3);
  const long long quad = row & ~3ll;
  if (quad + 3 < rows) {
    if ((row & 3) == 0) *reinterpret_cast<unsigned *>(q + row) = (unsigned)(byte | (b1 << 8) | (b2 << 16) | (b3 << 24));
  } else if (row < rows) {
    q[row] = (unsigned char)byte;
  }
}

__global__ __launch_bounds__(256) void head_pixel_topk_kernel(HeadArgs a) {
  const long long stride = (long long)gridDim.x * 256;
  const int groups = (a.c + 15) / 16;
  for (long long base = (long long)blockIdx.x * 256; base < a.rows; base += stride) {  // (uniform: the shuffles below need the whole wave)
    const long long row = base + threadIdx.x;
    const bool active = row < a.rows;
    int bk = -1, bi = 0;
    if (active) {
      const v4i *p = reinterpret_cast<const v4i *>(a.src + (size_t)row * a.src_ld);
      for (int g = 0; g < groups; ++g) {
        const v4i raw = p[g];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int key = (int)head_key8(head_byte(raw, e), a.src_dt), j = g * 16 + e;
          const bool better = j < a.c && key > bk;  // strictly: the first of equal maxima stays
          bk = better ? key : bk;
          bi = better ? j : bi;
        }
      }
    }
    const int vbyte = (int)head_key8((unsigned)(bk & 0xff), a.src_dt);  // (the key map is its own inverse)
    if (a.out_ld == 1) {
      if (a.out_dt == DFX_U8) head_store_quads(a.out, row, a.rows, bi);
      else if (active) reinterpret_cast<int *>(a.out)[row] = bi;
      if (a.val) head_store_quads(a.val, row, a.rows, vbyte);
    } else if (active) {
      const size_t o = (size_t)row * a.out_ld;
      if (a.out_dt == DFX_U8) a.out[o] = (unsigned char)bi;
      else reinterpret_cast<int *>(a.out)[o] = bi;
      if (a.val) a.val[o] = (unsigned char)vbyte;
    }
  }
}

__global__ __launch_bounds__(256) void head_pixel_softmax_kernel(HeadArgs a) {
  __shared__ unsigned tab[256];
  tab[threadIdx.x] = a.table[threadIdx.x];
  __syncthreads();
  const long long stride = (long long)gridDim.x * 256;
  const int groups = (a.c + 15) / 16;
  const int osz = a.out_dt == DFX_F32 ? 4 : 1;
  for (long long row = (long long)blockIdx.x * 256 + threadIdx.x; row < a.rows; row += stride) {
    const v4i *p = reinterpret_cast<const v4i *>(a.src + (size_t)row * a.src_ld);
    v4i keep[4];  // groups 0 .. 3 (src_ld <= 64: the whole row) stay in registers; further groups are re-read from L2
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const v4i zero = {0, 0, 0, 0};
      keep[g] = g < groups ? p[g] : zero;
    }
    auto each_group = [&](auto f) {
#pragma unroll
      for (int g = 0; g < 4; ++g)
        if (g < groups) f(keep[g], g);
      for (int g = 4; g < groups; ++g) f(p[g], g);
    };
    unsigned m = 0;
    each_group([&](const v4i &raw, int g) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const unsigned key = head_key8(head_byte(raw, e), a.src_dt);
        if (g * 16 + e < a.c) m = key > m ? key : m;
      }
    });
    unsigned sum = 0;
    each_group([&](const v4i &raw, int g) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const unsigned key = head_key8(head_byte(raw, e), a.src_dt);
        if (g * 16 + e < a.c) sum += tab[m - key];
      }
    });
    const float fs = __uint2float_rn(sum);
    unsigned char *dst_row = a.out + (size_t)row * a.out_ld * osz;
    each_group([&](const v4i &raw, int g) {
      const int left = a.c - g * 16;
      head_store_group(a, tab, dst_row, g, left < 16 ? left : 16, raw, m, fs);
    });
  }
}

#endif  // DFX_HEAD_KERNELS

}  // namespace dfx
