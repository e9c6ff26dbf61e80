// se.cuh -- kernels of the squeeze-and-excitation op (dfx_se_* of include/dfx.h; gfx950).  Three launches for the whole op:
//   se_squeeze_kernel   HBM-bound, reads src once.  A workgroup takes one (image, slice of pixels, chunk of channel groups);
//                       a lane owns 16 bytes of channels and walks the slice's pixels, adding the bytes as packed 16-bit
//                       halves (v & 0x00ff00ff, (v >> 8) & 0x00ff00ff: two VALU per 4 bytes plus the adds), flushed to s32
//                       after SE_FLUSH = 257 pixels at the latest.  The lanes that share a channel group meet in LDS; the
//                       workgroup's partial sums go to the handle's slab [bs][slices][c] with plain stores.  No atomics,
//                       no flags: integer sums give the same bits for every slice count.
//   se_excite_kernel    one workgroup per image: slab -> z (dfx_pool's average) -> FC1 (relu, u8) -> FC2 (s8) -> table ->
//                       the {bs,c} gate.  Activations sit in LDS as u8 ^ 0x80 (= u8 - 128 as s8) for v_dot4_i32_i8, the
//                       host's compensation 128 * sum(w) makes every sum exact, and the weight rows are zero-padded to
//                       16 bytes, so the dot products run in 16-byte steps without a tail.  Exact requant only.  In
//                       DFX_SE_SQUEEZE it stops after z.
//   se_scale_kernel     HBM-bound, reads src again and writes dst.  A lane owns a fixed 16-channel group of one image: its
//                       16 gate bytes and 16 scales are loaded once, then it walks down pixels.
// The generic kernels (se_squeeze_generic: a thread per (image, channel); se_scale_generic: a thread per byte) take any c
// and any alignment; se_excite_kernel serves both paths.
#pragma once

#include "dfx_device.cuh"
#include "se_plan.h"

namespace dfx {

struct SeArgs {
  const unsigned char *src;
  unsigned char *dst;
  int *slab;                  // handle scratch: [bs][slices][c] partial sums
  unsigned char *gate;        // handle scratch: [bs][c] (DFX_SE_SCALE)
  const signed char *w1;      // [cr][cpad], rows zero-padded to a multiple of 16
  const signed char *w2;      // [c][crpad]
  const int *comp1, *comp2;   // 128 * sum of the row's weights
  const float *bias1, *scale1, *bias2, *scale2;  // cr, cr, c, c entries
  const float *out_scale;     // c entries
  const unsigned char *lut;   // 256 entries
  int bs, c, cr, px, cpad, crpad, mode, rm;
  int slices, groups, gl, gchunks, pln, parts;  // squeeze kernel (SePlan)
  long long sq_items;         // squeeze: workgroup items (band) or bs * c (generic)
  int ex_parts;               // excite kernel: lanes per channel that add the slab's slices, 1 = one
  int cols;                   // scale kernel: pixel lanes per image; a lane walks pixels `cols` apart
  long long sc_total;         // scale: lanes (band) or bytes (generic)
};

// dfx_pool's average of u8 (pool_eltwise.hip, avg_finish<unsigned char>), word for word
__device__ __forceinline__ unsigned char se_avg_u8(int sum, int count) {
  return (unsigned char)min(255, max(0, (int)__builtin_rintf(__fdiv_rn((float)sum, (float)count))));
}

// one byte of the rescale: exact integer product (<= 65025), then the conv's requant chain without a bias
__device__ __forceinline__ unsigned se_scale_byte(unsigned s, unsigned g, float scale, int rm) {
  return sat_u8_bits(cvt_x86_rt(requant((int)(s * g), 0.0f, scale, true), rm));
}

constexpr int SE_EXCITE_MAX_THREADS = 1024;  // the excite kernel's workgroup: 256 lanes, 1024 for the wide layers
constexpr int SE_RED_PITCH = 17;  // ints per lane in the squeeze kernel's LDS image: conflict-free writes

// The kernels are plain functions, not templates: only se.hip, which launches them, may define them (se_api.hip takes
// SeArgs and the constants from this header).
#ifdef DFX_SE_KERNELS

__global__ __launch_bounds__(SE_THREADS) void se_squeeze_kernel(SeArgs a) {
  __shared__ int red[SE_THREADS * SE_RED_PITCH];
  __shared__ int part[SE_THREADS];
  const int t = threadIdx.x;
  const int gi = t % a.gl, pl = t / a.gl;  // pl >= pln: a lane without work
  const int nch = 16 * a.gl;
  for (long long item = blockIdx.x; item < a.sq_items; item += gridDim.x) {
    const int gc = (int)(item % a.gchunks);
    const long long r = item / a.gchunks;
    const int s = (int)(r % a.slices);
    const long long n = r / a.slices;
    const int g = gc * a.gl + gi;
    const int p0 = (int)((long long)s * a.px / a.slices), p1 = (int)((long long)(s + 1) * a.px / a.slices);
    int acc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0;
    if (pl < a.pln && g < a.groups) {
      const unsigned char *base = a.src + (size_t)n * a.px * a.c + (size_t)g * 16;
      const size_t step = (size_t)a.pln * a.c;
      const unsigned char *ptr = base + (size_t)(p0 + pl) * a.c;
      int left = p0 + pl >= p1 ? 0 : (p1 - p0 - pl + a.pln - 1) / a.pln;  // pixels of this lane (se_lane_pixels)
      while (left > 0) {
        const int run = min(left, SE_FLUSH);
        left -= run;
        unsigned lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0};
        int k = 0;
        for (; k + 4 <= run; k += 4, ptr += 4 * step) {  // four loads in flight
          v4i v[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const v4i *>(ptr + u * step);
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              lo[q] += (unsigned)v[u][q] & 0x00ff00ffu;
              hi[q] += ((unsigned)v[u][q] >> 8) & 0x00ff00ffu;
            }
        }
        for (; k < run; ++k, ptr += step) {
          const v4i v = *reinterpret_cast<const v4i *>(ptr);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            lo[q] += (unsigned)v[q] & 0x00ff00ffu;
            hi[q] += ((unsigned)v[q] >> 8) & 0x00ff00ffu;
          }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // dword q holds channels 4q .. 4q + 3 in its bytes 0 .. 3
          acc[4 * q + 0] += (int)(lo[q] & 0xffffu);
          acc[4 * q + 1] += (int)(hi[q] & 0xffffu);
          acc[4 * q + 2] += (int)(lo[q] >> 16);
          acc[4 * q + 3] += (int)(hi[q] >> 16);
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) red[t * SE_RED_PITCH + e] = acc[e];
    __syncthreads();
    int *out = a.slab + ((size_t)n * a.slices + s) * a.c + (size_t)gc * nch;
    const int c_left = a.c - gc * nch;  // channels of this chunk that exist
    if (a.parts > 1) {  // few channels, many pixel lanes: parts lanes per channel first (nch * parts <= 256)
      if (t < nch * a.parts) {
        const int ch = t % nch, k0 = t / nch;
        int sum = 0;
        for (int k = k0; k < a.pln; k += a.parts) sum += red[(k * a.gl + (ch >> 4)) * SE_RED_PITCH + (ch & 15)];
        part[t] = sum;
      }
      __syncthreads();
      if (t < nch && t < c_left) {
        int sum = 0;
        for (int k = 0; k < a.parts; ++k) sum += part[k * nch + t];
        out[t] = sum;
      }
    } else {
      for (int ch = t; ch < nch && ch < c_left; ch += SE_THREADS) {
        int sum = 0;
        for (int k = 0; k < a.pln; ++k) sum += red[(k * a.gl + (ch >> 4)) * SE_RED_PITCH + (ch & 15)];
        out[ch] = sum;
      }
    }
    __syncthreads();  // the next item overwrites red and part
  }
}

// one thread per (image, channel): the slab has one slice
__global__ __launch_bounds__(256) void se_squeeze_generic(SeArgs a) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < a.sq_items; id += stride) {
    const int ch = (int)(id % a.c);
    const long long n = id / a.c;
    const unsigned char *sp = a.src + (size_t)n * a.px * a.c + ch;
    int sum = 0;
    for (int p = 0; p < a.px; ++p) sum += (int)sp[(size_t)p * a.c];
    a.slab[id] = sum;
  }
}

__global__ __launch_bounds__(SE_EXCITE_MAX_THREADS) void se_excite_kernel(SeArgs a) {
  extern __shared__ v4i se_lds[];  // z ^ 0x80: cpad bytes; h ^ 0x80: crpad bytes; partial slab sums: blockDim.x ints
  unsigned char *zb = reinterpret_cast<unsigned char *>(se_lds);
  unsigned char *hb = zb + a.cpad;
  int *part = reinterpret_cast<int *>(hb + a.crpad);
  const int t = threadIdx.x, nt = blockDim.x, lane = t & 63, wave = t >> 6, waves = nt >> 6;
  unsigned char *out = a.mode == DFX_SE_SCALE ? a.gate : a.dst;
  for (long long n = blockIdx.x; n < a.bs; n += gridDim.x) {
    // squeeze: add the slab's slices (few channels, many slices: ex_parts lanes per channel first), dfx_pool's average
    const int *img = a.slab + (size_t)n * a.slices * a.c;
    if (a.ex_parts > 1) {  // c * ex_parts <= blockDim.x
      if (t < a.c * a.ex_parts) {
        const int ch = t % a.c;
        int sum = 0;
#pragma unroll 4
        for (int s = t / a.c; s < a.slices; s += a.ex_parts) sum += img[(size_t)s * a.c + ch];
        part[t] = sum;
      }
      __syncthreads();
    }
    for (int ch = t; ch < a.cpad; ch += nt) {
      unsigned char zx = 0x80;  // the padding up to cpad is the u8 0
      if (ch < a.c) {
        int sum = 0;
        if (a.ex_parts > 1) {
          for (int k = 0; k < a.ex_parts; ++k) sum += part[k * a.c + ch];
        } else {
#pragma unroll 4
          for (int s = 0; s < a.slices; ++s) sum += img[(size_t)s * a.c + ch];
        }
        const unsigned char z = se_avg_u8(sum, a.px);
        if (a.mode == DFX_SE_SQUEEZE) out[(size_t)n * a.c + ch] = z;
        zx = z ^ 0x80;
      }
      zb[ch] = zx;
    }
    for (int j = a.cr + t; j < a.crpad; j += nt) hb[j] = 0x80;
    __syncthreads();  // z is complete; `part` may be written again
    if (a.mode == DFX_SE_SQUEEZE) continue;
    // FC1: four outputs per wave at a time, lanes over 16-byte steps of the zero-padded rows
    const int cv = a.cpad >> 4;
    for (int j0 = wave * 4; j0 < a.cr; j0 += waves * 4) {
      const v4i *w[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) w[q] = reinterpret_cast<const v4i *>(a.w1 + (size_t)min(j0 + q, a.cr - 1) * a.cpad);
      int acc[4] = {0, 0, 0, 0};
      for (int k = lane; k < cv; k += 64) {
        const v4i zv = se_lds[k];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const v4i wv = w[q][k];
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[q] = __builtin_amdgcn_sdot4(zv[e], wv[e], acc[q], false);
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] += __shfl_xor(acc[q], off);
      }
      const int j = j0 + lane;
      if (lane < 4 && j < a.cr) {  // every lane holds the four sums: lane q finishes output j0 + q
        const int mine = lane == 0 ? acc[0] : lane == 1 ? acc[1] : lane == 2 ? acc[2] : acc[3];
        const float f = requant(mine + a.comp1[j], a.bias1[j], a.scale1[j], true);
        hb[j] = (unsigned char)(sat_u8_bits(cvt_x86_rt(f, a.rm)) ^ 0x80u);
      }
    }
    __syncthreads();
    // FC2: a thread per channel, 16-byte steps of its zero-padded row with h broadcast from LDS
    const int rv = a.crpad >> 4;
    const v4i *hv = se_lds + (a.cpad >> 4);
    for (int ch = t; ch < a.c; ch += nt) {
      const v4i *wr = reinterpret_cast<const v4i *>(a.w2 + (size_t)ch * a.crpad);
      int acc = a.comp2[ch];
#pragma unroll 4
      for (int k = 0; k < rv; ++k) {
        const v4i hh = hv[k], wv = wr[k];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_sdot4(hh[e], wv[e], acc, false);
      }
      const int tq = sat_s8(cvt_x86_rt(requant(acc, a.bias2[ch], a.scale2[ch], false), a.rm));
      out[(size_t)n * a.c + ch] = a.lut[tq + 128];
    }
    __syncthreads();  // the next image overwrites z and h
  }
}

union SeVec {
  v4i v;
  unsigned char e[16];
};

template <int RM>
__global__ __launch_bounds__(256) void se_scale_kernel(SeArgs a) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < a.sc_total; id += stride) {
    // consecutive lanes: consecutive channel groups, then consecutive pixels -- coalesced loads and stores
    const int g = (int)(id % a.groups);
    const long long t = id / a.groups;
    const int col = (int)(t % a.cols);
    const long long n = t / a.cols;
    SeVec gv;
    gv.v = *reinterpret_cast<const v4i *>(a.gate + (size_t)n * a.c + (size_t)g * 16);
    float sc[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const v4f f = *reinterpret_cast<const v4f *>(a.out_scale + (size_t)g * 16 + 4 * q);
      sc[4 * q + 0] = f[0]; sc[4 * q + 1] = f[1]; sc[4 * q + 2] = f[2]; sc[4 * q + 3] = f[3];
    }
    const size_t img = (size_t)n * a.px * a.c + (size_t)g * 16;
    for (int p = col; p < a.px; p += a.cols) {
      const size_t off = img + (size_t)p * a.c;
      SeVec v, r;
      v.v = *reinterpret_cast<const v4i *>(a.src + off);
#pragma unroll
      for (int e = 0; e < 16; ++e) r.e[e] = (unsigned char)se_scale_byte(v.e[e], gv.e[e], sc[e], RM);
      dfx_store16(reinterpret_cast<v4i *>(a.dst + off), r.v);
    }
  }
}

// one thread per byte
__global__ __launch_bounds__(256) void se_scale_generic(SeArgs a) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long per_image = (long long)a.px * a.c;
  for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < a.sc_total; id += stride) {
    const int ch = (int)(id % a.c);
    const long long n = id / per_image;
    a.dst[id] = (unsigned char)se_scale_byte(a.src[id], a.gate[(size_t)n * a.c + ch], a.out_scale[ch], a.rm);
  }
}

#endif  // DFX_SE_KERNELS

}  // namespace dfx
