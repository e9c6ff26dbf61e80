// select.cuh -- kernels of the image-wide top-K with peak filter (dfx_select_* of include/dfx.h; gfx950).  Memory-bound
// work, no MFMA.
//
// Every candidate becomes ONE unsigned 64-bit number, (key << 32) | (0xffffffff - e): key is the 1-byte element mapped
// monotonically onto 0 .. 255 (head.cuh's head_key8), e its index inside the image.  "Larger value first, lower index
// first among equals" is plain `>` on distinct numbers; 0 is below every real pair (e <= 2^31 - 2) and pads the sort.
// With 256 keys the K best are found exactly without sorting the image: a histogram of the candidates' keys gives the
// threshold key t (select_plan.h: select_threshold), every key above t is taken, and of the key t itself the lowest e's.
// At most K pairs are then sorted.  val is the key mapped back: for one byte that is the element verbatim.
//
//   select_generic_kernel   a workgroup per image does all of it with byte loads: histogram in LDS, threshold, an ordered
//                           pass that ranks the tie bin by a workgroup prefix sum, the sort, the stores.  Defines the bits.
//   select_hist_kernel      launch A: a workgroup per (image, chunk of consecutive pixels).  A lane takes 16 channels of a
//                           pixel with one 16-byte load; for the 3x3 test it loads the same 16 channels of the up to eight
//                           neighbours (lines its neighbours in the workgroup touch as well: they come from the cache) and
//                           compares bytewise.  Per-wave LDS histograms, merged, stored plainly into the chunk's slab row.
//   select_scan_kernel      launch B: a workgroup per image sums the slab, finds t and every chunk's offsets / quota.
//   select_compact_kernel   launch C: the grid of A re-evaluates the candidates and writes the pairs to cand.  Keys above
//                           t take the next free slot of the chunk's range (an LDS counter: their order does not matter,
//                           they are sorted later); keys equal to t are ranked in index order by a workgroup prefix sum
//                           and kept while the rank is below the chunk's quota.
//   select_sort_kernel      launch D: a workgroup per image, bitonic sort in LDS, idx / val / fill / count, the gathers.
// No cross-workgroup flag, spin or counter and no global atomic: what a launch needs from other workgroups was written by
// the launch before it.
#pragma once

#include "dfx_device.cuh"
#include "select_plan.h"

namespace dfx {

struct SelectArgs {
  const unsigned char *src;
  int *idx;
  unsigned char *val;            // or null
  int *count;
  const unsigned char *gsrc[DFX_SELECT_MAX_GATHER];
  unsigned char *gdst[DFX_SELECT_MAX_GATHER];
  int row_bytes[DFX_SELECT_MAX_GATHER], pixel_stride[DFX_SELECT_MAX_GATHER];
  int n_gather;
  unsigned *slab, *plan;         // the handle's scratch (histogram path)
  unsigned long long *cand;
  int bs, h, w, c, src_ld, k, idx_ld, peak, src_dt, min_key;
  int chunk_px, chunks;
  long long items;               // bs * chunks
};

#ifdef DFX_SELECT_KERNELS

__device__ __forceinline__ unsigned long long select_pair(unsigned key, unsigned e) {
  return ((unsigned long long)key << 32) | (0xffffffffu - e);
}
__device__ __forceinline__ unsigned select_byte(const v4i &raw, int j) { return ((unsigned)raw[j >> 2] >> (8 * (j & 3))) & 0xffu; }

// exclusive prefix sum of v over the workgroup in lane order; *total: the sum.  Every lane calls it.  wt: 16 ints of LDS.
__device__ __forceinline__ int select_block_scan(int v, int *wt, int *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d);
    inc += lane >= d ? o : 0;
  }
  if (lane == 63) wt[wave] = inc;
  __syncthreads();
  int off = 0, tot = 0;
  for (int i = 0; i < waves; ++i) {
    const int x = wt[i];
    off += i < wave ? x : 0;
    tot += x;
  }
  __syncthreads();  // (wt is written again by the next call)
  *total = tot;
  return off + inc - v;
}

// pairs[0 .. count-1] -> sorted, best first; then image r's idx / val / fill / count and gather rows.  pairs: LDS, room
// for select_sort_size(k) entries.
__device__ __forceinline__ void select_finish(const SelectArgs &a, int r, unsigned long long *pairs, unsigned count) {
  const int T = blockDim.x, tid = threadIdx.x;
  int P = 64;
  while (P < a.k) P *= 2;
  for (int i = tid; i < P; i += T)
    if ((unsigned)i >= count) pairs[i] = 0;
  __syncthreads();
  for (int kk = 2; kk <= P; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += T) {
        const int o = i ^ j;
        if (o > i) {
          const unsigned long long x = pairs[i], y = pairs[o];
          const bool swap = (i & kk) == 0 ? x < y : x > y;  // descending runs where bit kk of i is clear
          if (swap) {
            pairs[i] = y;
            pairs[o] = x;
          }
        }
      }
      __syncthreads();
    }
  }
  for (int j = tid; j < a.k; j += T) {
    const bool real = (unsigned)j < count;
    const unsigned long long p = pairs[j];
    const size_t o = (size_t)r * a.idx_ld + j;
    a.idx[o] = real ? (int)(0xffffffffu - (unsigned)p) : -1;
    if (a.val) a.val[o] = real ? (unsigned char)select_key8((unsigned)(p >> 32), a.src_dt) : (unsigned char)0;  // (the key map is its own inverse)
  }
  if (tid == 0) a.count[r] = (int)count;
  const size_t px = (size_t)a.h * a.w;
  for (int i = 0; i < a.n_gather; ++i) {
    const int rb = a.row_bytes[i];
    const size_t st = (size_t)a.pixel_stride[i];
    const unsigned char *gs = a.gsrc[i] + (size_t)r * px * st;
    unsigned char *gd = a.gdst[i] + (size_t)r * a.k * rb;
    const int total = a.k * rb;  // <= 4096 * 1024
    for (int q = tid; q < total; q += T) {
      const int j = q / rb, b = q - j * rb;
      unsigned char v = 0;
      if ((unsigned)j < count) {
        const unsigned e = 0xffffffffu - (unsigned)pairs[j];
        v = gs[(size_t)(e / (unsigned)a.c) * st + b];
      }
      gd[q] = v;
    }
  }
}

// ---- generic: a workgroup per image ------------------------------------------------------------------------------------
// the key of element e of the image at `img` when it is a candidate, else -1
__device__ __forceinline__ int select_cand_key(const SelectArgs &a, const unsigned char *img, unsigned e) {
  const unsigned p = e / (unsigned)a.c, k = e - p * (unsigned)a.c;
  const int v = (int)select_key8(img[(size_t)p * a.src_ld + k], a.src_dt);
  if (v < a.min_key) return -1;
  if (a.peak == DFX_SELECT_PEAK3) {
    const int y = (int)(p / (unsigned)a.w), x = (int)(p - (unsigned)y * (unsigned)a.w);
    for (int dy = -1; dy <= 1; ++dy) {
      const int yy = y + dy;
      if (yy < 0 || yy >= a.h) continue;
      for (int dx = -1; dx <= 1; ++dx) {
        const int xx = x + dx;
        if (xx < 0 || xx >= a.w || (dy == 0 && dx == 0)) continue;
        const int n = (int)select_key8(img[((size_t)yy * a.w + xx) * a.src_ld + k], a.src_dt);
        if (n > v) return -1;
      }
    }
  }
  return v;
}

__global__ __launch_bounds__(SELECT_SORT_THREADS) void select_generic_kernel(SelectArgs a) {
  __shared__ unsigned long long pairs[DFX_SELECT_MAX_K];
  __shared__ unsigned hist[SELECT_BINS];
  __shared__ int wt[16];
  __shared__ unsigned ctr[2];  // ([1]: padding, so that the sizes add up to the kernel's LDS)
  __shared__ SelectThreshold th;
  const int T = blockDim.x, tid = threadIdx.x;
  const size_t px = (size_t)a.h * a.w;
  const unsigned n = (unsigned)(px * a.c);  // <= 2^31 - 1
  for (int r = blockIdx.x; r < a.bs; r += gridDim.x) {
    const unsigned char *img = a.src + (size_t)r * px * a.src_ld;
    for (int i = tid; i < SELECT_BINS; i += T) hist[i] = 0;
    if (tid == 0) ctr[0] = 0;
    __syncthreads();
    for (unsigned e = tid; e < n; e += T) {
      const int key = select_cand_key(a, img, e);
      if (key >= 0) atomicAdd(&hist[key], 1u);  // (LDS; a count does not depend on the order)
    }
    __syncthreads();
    if (tid == 0) th = select_threshold(hist, a.k);
    __syncthreads();
    const int t = th.t;
    const unsigned n_gt = th.n_gt, quota = th.quota;
    unsigned running = 0;
    for (unsigned base = 0; base < n; base += T) {  // (uniform: the prefix sum needs every lane)
      const unsigned e = base + tid;
      const int key = e < n ? select_cand_key(a, img, e) : -1;
      if (key > t) {
        const unsigned slot = atomicAdd(&ctr[0], 1u);
        if (slot < n_gt) pairs[slot] = select_pair((unsigned)key, e);
      }
      const int flag = key == t;
      int tot;
      const unsigned rank = running + (unsigned)select_block_scan(flag, wt, &tot);
      if (flag && rank < quota) pairs[n_gt + rank] = select_pair((unsigned)key, e);
      running += (unsigned)tot;
    }
    __syncthreads();
    select_finish(a, r, pairs, th.count);
    __syncthreads();
  }
}

// ---- histogram path ------------------------------------------------------------------------------------------------------
// The 16 channels gi * 16 .. of pixel p of the image at `img`: their keys (kv, a byte each) and which of them are
// candidates (bit j: channel gi * 16 + j).  gpp: 16-byte groups per pixel.
__device__ __forceinline__ unsigned select_group(const SelectArgs &a, const unsigned char *img, long long p, int gi, int gpp, v4i &kv) {
  const v4i *q = reinterpret_cast<const v4i *>(img) + p * gpp + gi;
  const int flip = a.src_dt == DFX_S8 ? (int)0x80808080u : 0;
  const v4i raw = *q;
  kv = v4i{raw[0] ^ flip, raw[1] ^ flip, raw[2] ^ flip, raw[3] ^ flip};
  const int nvalid = a.c - gi * 16;
  unsigned mask = nvalid >= 16 ? 0xffffu : nvalid <= 0 ? 0u : ((1u << nvalid) - 1u);
#pragma unroll
  for (int j = 0; j < 16; ++j)
    if ((int)select_byte(kv, j) < a.min_key) mask &= ~(1u << j);
  if (a.peak == DFX_SELECT_PEAK3 && mask) {
    const int y = (int)(p / a.w), x = (int)(p - (long long)y * a.w);
    for (int dy = -1; dy <= 1; ++dy) {
      if (y + dy < 0 || y + dy >= a.h) continue;
      for (int dx = -1; dx <= 1; ++dx) {
        if (x + dx < 0 || x + dx >= a.w || (dy == 0 && dx == 0)) continue;
        const v4i nr = q[((long long)dy * a.w + dx) * gpp];
        const v4i nb = v4i{nr[0] ^ flip, nr[1] ^ flip, nr[2] ^ flip, nr[3] ^ flip};
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if (select_byte(nb, j) > select_byte(kv, j)) mask &= ~(1u << j);
      }
    }
  }
  return mask;
}

__global__ __launch_bounds__(SELECT_THREADS) void select_hist_kernel(SelectArgs a) {
  __shared__ unsigned hist[SELECT_THREADS / 64][SELECT_BINS];
  const int tid = threadIdx.x, wave = tid >> 6;
  const long long px = (long long)a.h * a.w;
  const int gpp = a.src_ld / 16;
  for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
    const int r = (int)(item / a.chunks), ch = (int)(item - (long long)r * a.chunks);
    const unsigned char *img = a.src + (size_t)r * px * a.src_ld;
    for (int i = tid; i < (SELECT_THREADS / 64) * SELECT_BINS; i += SELECT_THREADS) (&hist[0][0])[i] = 0;
    __syncthreads();
    const long long p0 = (long long)ch * a.chunk_px, p1 = p0 + a.chunk_px < px ? p0 + a.chunk_px : px;
    const long long groups = (p1 - p0) * gpp;
    for (long long g = tid; g < groups; g += SELECT_THREADS) {
      const long long p = p0 + g / gpp;
      const int gi = (int)(g % gpp);
      v4i kv;
      const unsigned mask = select_group(a, img, p, gi, gpp, kv);
      if (mask) {
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if (mask >> j & 1u) atomicAdd(&hist[wave][select_byte(kv, j)], 1u);  // (LDS)
      }
    }
    __syncthreads();
    static_assert(SELECT_THREADS == SELECT_BINS, "a lane per key");
    unsigned s = 0;
#pragma unroll
    for (int v = 0; v < SELECT_THREADS / 64; ++v) s += hist[v][tid];
    a.slab[(size_t)item * SELECT_BINS + tid] = s;
    __syncthreads();
  }
}

__global__ __launch_bounds__(SELECT_SORT_THREADS) void select_scan_kernel(SelectArgs a) {
  __shared__ unsigned part[SELECT_SORT_THREADS / SELECT_BINS][SELECT_BINS];
  __shared__ unsigned total[SELECT_BINS];
  __shared__ unsigned gt[SELECT_MAX_CHUNKS], eq[SELECT_MAX_CHUNKS], cplan[SELECT_CHUNK_WORDS * SELECT_MAX_CHUNKS];
  __shared__ SelectThreshold th;
  const int T = SELECT_SORT_THREADS, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int r = blockIdx.x; r < a.bs; r += gridDim.x) {
    const unsigned *slab = a.slab + (size_t)r * a.chunks * SELECT_BINS;
    unsigned *plan = a.plan + (size_t)r * (SELECT_HDR_WORDS + SELECT_CHUNK_WORDS * (size_t)a.chunks);
    {  // the image's histogram: a lane per key and quarter of the chunks
      const int b = tid % SELECT_BINS, q = tid / SELECT_BINS;
      unsigned s = 0;
      for (int c = q; c < a.chunks; c += T / SELECT_BINS) s += slab[(size_t)c * SELECT_BINS + b];
      part[q][b] = s;
    }
    __syncthreads();
    if (tid < SELECT_BINS) {
      unsigned s = 0;
#pragma unroll
      for (int q = 0; q < T / SELECT_BINS; ++q) s += part[q][tid];
      total[tid] = s;
    }
    __syncthreads();
    if (tid == 0) th = select_threshold(total, a.k);
    __syncthreads();
    const int t = th.t;
    for (int c = wave; c < a.chunks; c += T / 64) {  // a wave per chunk: its candidates above t and at t
      unsigned g = 0;
      for (int b = t + 1 + lane; b < SELECT_BINS; b += 64) g += slab[(size_t)c * SELECT_BINS + b];
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) g += (unsigned)__shfl_xor((int)g, m);
      if (lane == 0) {
        gt[c] = g;
        eq[c] = slab[(size_t)c * SELECT_BINS + t];
      }
    }
    __syncthreads();
    if (tid == 0) select_chunk_offsets(gt, eq, a.chunks, th.n_gt, th.quota, cplan);
    __syncthreads();
    // a word per lane (the serial loop above would otherwise leave as 16-byte stores, which this library only issues
    // through dfx_store16)
    if (tid < SELECT_HDR_WORDS) plan[tid] = tid == 0 ? (unsigned)t : tid == 1 ? th.count : tid == 2 ? th.n_gt : th.quota;
    for (int i = tid; i < SELECT_CHUNK_WORDS * a.chunks; i += T) plan[SELECT_HDR_WORDS + i] = cplan[i];
    __syncthreads();
  }
}

__global__ __launch_bounds__(SELECT_THREADS) void select_compact_kernel(SelectArgs a) {
  __shared__ int wt[16];
  __shared__ unsigned ctr;
  const int tid = threadIdx.x;
  const long long px = (long long)a.h * a.w;
  const int gpp = a.src_ld / 16;
  for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
    const int r = (int)(item / a.chunks), ch = (int)(item - (long long)r * a.chunks);
    const unsigned *plan = a.plan + (size_t)r * (SELECT_HDR_WORDS + SELECT_CHUNK_WORDS * (size_t)a.chunks);
    const unsigned *mine = plan + SELECT_HDR_WORDS + SELECT_CHUNK_WORDS * ch;
    const unsigned t = plan[0], n_gt = plan[2];
    const unsigned off_gt = mine[0], quota = mine[1], off_eq = mine[2];
    const unsigned end_gt = ch + 1 < a.chunks ? mine[SELECT_CHUNK_WORDS] : n_gt;
    if (end_gt == off_gt && quota == 0) continue;  // (uniform) nothing of this chunk is taken
    const unsigned char *img = a.src + (size_t)r * px * a.src_ld;
    unsigned long long *cand = a.cand + (size_t)r * a.k;
    if (tid == 0) ctr = 0;
    __syncthreads();
    const long long p0 = (long long)ch * a.chunk_px, p1 = p0 + a.chunk_px < px ? p0 + a.chunk_px : px;
    const long long groups = (p1 - p0) * gpp;
    unsigned running = 0;
    for (long long base = 0; base < groups; base += SELECT_THREADS) {  // (uniform: the prefix sum needs every lane)
      const long long g = base + tid;
      unsigned mask = 0, e0 = 0;
      v4i kv = {0, 0, 0, 0};
      if (g < groups) {
        const long long p = p0 + g / gpp;
        const int gi = (int)(g % gpp);
        mask = select_group(a, img, p, gi, gpp, kv);
        e0 = (unsigned)(p * a.c + gi * 16);
      }
      int neq = 0;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const unsigned key = select_byte(kv, j);
        if ((mask >> j & 1u) && key > t) {
          const unsigned slot = off_gt + atomicAdd(&ctr, 1u);  // (LDS)
          if (slot < end_gt) cand[slot] = select_pair(key, e0 + j);
        }
        neq += (mask >> j & 1u) && key == t;
      }
      int tot;
      unsigned rank = running + (unsigned)select_block_scan(neq, wt, &tot);
      if (neq) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          if ((mask >> j & 1u) && select_byte(kv, j) == t) {
            if (rank < quota) cand[off_eq + rank] = select_pair(t, e0 + j);
            ++rank;
          }
        }
      }
      running += (unsigned)tot;
      if (running >= quota && end_gt == off_gt) break;  // (uniform)
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(SELECT_SORT_THREADS) void select_sort_kernel(SelectArgs a) {
  __shared__ unsigned long long pairs[DFX_SELECT_MAX_K];
  const int T = blockDim.x, tid = threadIdx.x;
  for (int r = blockIdx.x; r < a.bs; r += gridDim.x) {
    const unsigned *plan = a.plan + (size_t)r * (SELECT_HDR_WORDS + SELECT_CHUNK_WORDS * (size_t)a.chunks);
    const unsigned count = plan[1] < (unsigned)a.k ? plan[1] : (unsigned)a.k;
    const unsigned long long *cand = a.cand + (size_t)r * a.k;
    for (unsigned i = tid; i < count; i += T) pairs[i] = cand[i];
    __syncthreads();
    select_finish(a, r, pairs, count);
    __syncthreads();
  }
}

#endif  // DFX_SELECT_KERNELS

}  // namespace dfx
