// nms.cuh -- kernels of the box decode + greedy NMS (dfx_nms_* of include/dfx.h; gfx950).  No MFMA.
//
// Every floating-point step is one __f*_rn call in the order of the definition, so the decode and the overlap test give the
// same bits wherever they are evaluated; the greedy rule then makes the result a function of the inputs alone.
//
//   nms_generic_kernel   a workgroup of 1024 lanes per image: boxes, labels and an alive byte per position in LDS, then a
//                        serial walk over j.  A j that is alive and valid is kept; the lanes test their own positions > j
//                        against it and clear their alive bytes; one barrier per kept j.  Defines the bits.
//   nms_prep_kernel      launch A: a lane per position decodes (or copies) its box into box[bs][n64 * 64] and its label into
//                        lab; invalid entries and positions >= n_valid get label -1, which matches nothing.
//   nms_mask_kernel      launch B: a wave per (image, tile of the upper triangle).  Lane t owns row box rb * 64 + t; the 64
//                        column boxes and labels are LDS broadcast reads; one u64 per lane, stored plainly.
//   nms_scan_kernel      launch C: a wave per image.  Lane l holds word l of the removed bitmap.  Per 64-row block: the
//                        diagonal words go to LDS and nms_block_scan (nms_plan.h) resolves the block; then every lane l > b
//                        ORs word l of the kept rows, sixteen independent loads at a time; the next block's diagonal words
//                        are already on their way.
// No cross-workgroup flag, spin or counter and no global atomic: what a launch needs from other workgroups was written by
// the launch before it.
#pragma once

#include "dfx_device.cuh"
#include "nms_plan.h"

namespace dfx {

struct NmsArgs {
  const float *boxes;            // BOXES
  const int *idx;                // or null
  const unsigned char *deltas;
  const float *anchors, *tab_c, *tab_s;
  const int *count_in;           // or null
  int *keep, *count;
  float *boxes_out;              // or null
  v4f *box;                      // the handle's scratch (mask path)
  int *lab;
  unsigned long long *mask;
  const unsigned short *tiles;
  int bs, n, n64, max_out, keep_ld, mode, per_class, classes, apx, row_bytes, idx_ld, n_tiles;
  long long n_entries;           // n_anchors * classes
  float iou_thr, clip_w, clip_h;
};

#ifdef DFX_NMS_KERNELS

__device__ __forceinline__ int nms_n_valid(const NmsArgs &a, int r) {
  if (!a.count_in) return a.n;
  const int c = a.count_in[r];
  return c < 0 ? 0 : c > a.n ? a.n : c;
}

__device__ __forceinline__ float nms_clip(float x, float hi) {
  x = x < 0.0f ? 0.0f : x;
  return x > hi ? hi : x;
}

// box and label of position j of image r (j < n_valid).  Label -1: invalid.  wide: anchors may be read 16 bytes at a time.
template <bool wide>
__device__ __forceinline__ v4f nms_load(const NmsArgs &a, int r, int j, int *label) {
  int e = 0;
  bool ok = true;
  if (a.idx && (a.mode == DFX_NMS_DECODE || a.per_class)) {
    e = a.idx[(size_t)r * a.idx_ld + j];
    ok = e >= 0 && (long long)e < a.n_entries;
  }
  *label = !ok ? -1 : a.per_class ? e % a.classes : 0;
  if (a.mode == DFX_NMS_BOXES) {
    const float *p = a.boxes + ((size_t)r * a.n + j) * 4;
    if (wide) return *reinterpret_cast<const v4f *>(p);
    return v4f{p[0], p[1], p[2], p[3]};
  }
  if (!ok) return v4f{0.0f, 0.0f, 0.0f, 0.0f};
  const int g = e / a.classes, an = g % a.apx;
  const unsigned char *q = a.deltas + ((size_t)r * a.n + j) * a.row_bytes + 4 * an;
  const float *ap = a.anchors + (size_t)g * 4;
  v4f A;
  if (wide) A = *reinterpret_cast<const v4f *>(ap);
  else A = v4f{ap[0], ap[1], ap[2], ap[3]};
  const float aw = __fsub_rn(A[2], A[0]), ah = __fsub_rn(A[3], A[1]);
  const float acx = __fadd_rn(A[0], __fmul_rn(0.5f, aw)), acy = __fadd_rn(A[1], __fmul_rn(0.5f, ah));
  const float cx = __fadd_rn(acx, __fmul_rn(a.tab_c[q[0]], aw)), cy = __fadd_rn(acy, __fmul_rn(a.tab_c[q[1]], ah));
  const float w = __fmul_rn(aw, a.tab_s[q[2]]), hh = __fmul_rn(ah, a.tab_s[q[3]]);
  const float hw = __fmul_rn(0.5f, w), hhh = __fmul_rn(0.5f, hh);
  v4f b = {__fsub_rn(cx, hw), __fsub_rn(cy, hhh), __fadd_rn(cx, hw), __fadd_rn(cy, hhh)};
  if (a.clip_w > 0.0f) {
    b[0] = nms_clip(b[0], a.clip_w);
    b[2] = nms_clip(b[2], a.clip_w);
    b[1] = nms_clip(b[1], a.clip_h);
    b[3] = nms_clip(b[3], a.clip_h);
  }
  return b;
}

__device__ __forceinline__ float nms_area(const v4f &x) { return __fmul_rn(__fsub_rn(x[2], x[0]), __fsub_rn(x[3], x[1])); }

// "a suppresses b", a the box of the lower position; the labels are compared by the caller
__device__ __forceinline__ bool nms_over(const v4f &a, float area_a, const v4f &b, float thr) {
  const float xx1 = a[0] > b[0] ? a[0] : b[0], yy1 = a[1] > b[1] ? a[1] : b[1];
  const float xx2 = a[2] < b[2] ? a[2] : b[2], yy2 = a[3] < b[3] ? a[3] : b[3];
  float w = __fsub_rn(xx2, xx1), h = __fsub_rn(yy2, yy1);
  w = w > 0.0f ? w : 0.0f;
  h = h > 0.0f ? h : 0.0f;
  const float inter = __fmul_rn(w, h);
  const float u = __fsub_rn(__fadd_rn(area_a, nms_area(b)), inter);
  return __fdiv_rn(inter, u) > thr;
}

// ---- generic: a workgroup per image -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(NMS_GENERIC_THREADS) void nms_generic_kernel(NmsArgs a) {
  __shared__ v4f box[DFX_NMS_MAX_N];
  __shared__ int lab[DFX_NMS_MAX_N];
  __shared__ unsigned char alive[DFX_NMS_MAX_N];
  const int T = NMS_GENERIC_THREADS, tid = threadIdx.x;
  for (int r = blockIdx.x; r < a.bs; r += gridDim.x) {
    const int nv = nms_n_valid(a, r);
    int *keep = a.keep + (size_t)r * a.keep_ld;
    float *bo = a.boxes_out ? a.boxes_out + (size_t)r * a.max_out * 4 : nullptr;
    for (int j = tid; j < nv; j += T) {
      int l;
      box[j] = nms_load<false>(a, r, j, &l);
      lab[j] = l;
      alive[j] = l >= 0;
    }
    __syncthreads();
    int cnt = 0;
    for (int j = 0; j < nv && cnt < a.max_out; ++j) {
      if (!alive[j]) continue;  // (uniform: alive[j] was last written before the previous barrier)
      const v4f bj = box[j];
      const int lj = lab[j];
      const float aj = nms_area(bj);
      if (tid == 0) keep[cnt] = j;
      // a coordinate per lane (four stores of one lane would leave as a 16-byte store, which this library only issues
      // through dfx_store16, and boxes_out need not be 16-byte aligned here)
      if (bo && tid < 4) bo[4 * cnt + tid] = tid == 0 ? bj[0] : tid == 1 ? bj[1] : tid == 2 ? bj[2] : bj[3];
      ++cnt;
      // position p = j + 1 + tid, + T, ...
      for (int p = j + 1 + tid; p < nv; p += T)
        if (alive[p] && lab[p] == lj && nms_over(bj, aj, box[p], a.iou_thr)) alive[p] = 0;
      __syncthreads();
    }
    for (int i = cnt + tid; i < a.max_out; i += T) keep[i] = -1;
    if (bo)
      for (int i = 4 * cnt + tid; i < 4 * a.max_out; i += T) bo[i] = 0.0f;
    if (tid == 0) a.count[r] = cnt;
    __syncthreads();  // (the LDS is filled again for the next image)
  }
}

// ---- mask path ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NMS_PREP_THREADS) void nms_prep_kernel(NmsArgs a) {
  const int per = a.n64 * NMS_TILE;
  const long long total = (long long)a.bs * per;
  for (long long i = (long long)blockIdx.x * NMS_PREP_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * NMS_PREP_THREADS) {
    const int r = (int)(i / per), j = (int)(i - (long long)r * per);
    v4f b = {0.0f, 0.0f, 0.0f, 0.0f};
    int l = -1;
    if (j < nms_n_valid(a, r)) b = nms_load<true>(a, r, j, &l);
    dfx_store16(a.box + i, b);
    a.lab[i] = l;
  }
}

__global__ __launch_bounds__(NMS_MASK_THREADS) void nms_mask_kernel(NmsArgs a) {
  __shared__ v4f cbox[NMS_MASK_THREADS / 64][NMS_TILE];
  __shared__ int clab[NMS_MASK_THREADS / 64][NMS_TILE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long items = (long long)a.bs * a.n_tiles;
  const int per = a.n64 * NMS_TILE;
  // (uniform trip count over the workgroup: every wave reaches both barriers)
  for (long long base = (long long)blockIdx.x * (NMS_MASK_THREADS / 64); base < items; base += (long long)gridDim.x * (NMS_MASK_THREADS / 64)) {
    const long long item = base + wave;
    bool work = item < items;
    int r = 0, rb = 0, cb = 0;
    if (work) {
      r = (int)(item / a.n_tiles);
      const unsigned t = a.tiles[item - (long long)r * a.n_tiles];
      rb = (int)(t & 0xffu);
      cb = (int)(t >> 8);
      work = cb * NMS_TILE < nms_n_valid(a, r);  // tiles wholly beyond n_valid: nothing reads their words
    }
    const size_t img = (size_t)r * per;
    if (work) {
      cbox[wave][lane] = a.box[img + cb * NMS_TILE + lane];
      clab[wave][lane] = a.lab[img + cb * NMS_TILE + lane];
    }
    __syncthreads();
    if (work) {
      const int row = rb * NMS_TILE + lane;
      const v4f b = a.box[img + row];
      const int l = a.lab[img + row];
      const float ar = nms_area(b);
      unsigned long long word = 0;
      const int first = rb == cb ? lane + 1 : 0;  // column position > row position
      if (l >= 0) {
        for (int c = first; c < NMS_TILE; ++c)
          if (clab[wave][c] == l && nms_over(b, ar, cbox[wave][c], a.iou_thr)) word |= 1ull << c;
      }
      a.mask[(img + row) * a.n64 + cb] = word;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(NMS_SCAN_THREADS) void nms_scan_kernel(NmsArgs a) {
  __shared__ uint64_t diag[NMS_TILE];
  const int lane = threadIdx.x;
  const int per = a.n64 * NMS_TILE;
  for (int r = blockIdx.x; r < a.bs; r += gridDim.x) {
    const int nv = nms_n_valid(a, r), nb = (nv + NMS_TILE - 1) / NMS_TILE;
    const size_t img = (size_t)r * per;
    const unsigned long long *mask = a.mask + img * a.n64;
    int *keep = a.keep + (size_t)r * a.keep_ld;
    v4f *bo = a.boxes_out ? reinterpret_cast<v4f *>(a.boxes_out) + (size_t)r * a.max_out : nullptr;
    unsigned long long removed = 0;  // word `lane`
    int cnt = 0;
    // the diagonal word and the label of this lane's row of the NEXT block are loaded before the current block is worked on
    unsigned long long dnext = nb > 0 ? mask[(size_t)lane * a.n64] : 0;
    int lnext = nb > 0 ? a.lab[img + lane] : -1;
    for (int b = 0; b < nb && cnt < a.max_out; ++b) {
      const int row = b * NMS_TILE + lane;
      diag[lane] = dnext;
      const unsigned long long valid = __ballot(lnext >= 0);
      if (b + 1 < nb) {  // (uniform)
        dnext = mask[(size_t)(row + NMS_TILE) * a.n64 + b + 1];
        lnext = a.lab[img + row + NMS_TILE];
      }
      const unsigned long long rem_b = __shfl(removed, b);
      __syncthreads();  // (one wave: orders the LDS writes before the reads)
      const unsigned long long kept = nms_block_scan(diag, valid & ~rem_b, a.max_out - cnt);
      __syncthreads();
      // word `lane` of every kept row, for the blocks behind this one: NMS_SCAN_BATCH unconditional, independent loads at a
      // time (a batch that runs out of kept rows loads its last row again: OR does not mind)
      if (lane > b && lane < nb) {
        unsigned long long left = kept;
        while (left) {
          unsigned long long w[NMS_SCAN_BATCH];
          int t = __builtin_ctzll(left);
#pragma unroll
          for (int u = 0; u < NMS_SCAN_BATCH; ++u) {
            w[u] = mask[(size_t)(b * NMS_TILE + t) * a.n64 + lane];
            left &= left - 1;
            t = left ? __builtin_ctzll(left) : t;
          }
#pragma unroll
          for (int u = 0; u < NMS_SCAN_BATCH; ++u) removed |= w[u];
        }
      }
      if (kept >> lane & 1ull) {
        const int o = cnt + __popcll(kept & ((1ull << lane) - 1ull));
        keep[o] = row;
        if (bo) dfx_store16(bo + o, a.box[img + row]);
      }
      cnt += __popcll(kept);
    }
    for (int i = cnt + lane; i < a.max_out; i += NMS_SCAN_THREADS) {
      keep[i] = -1;
      if (bo) dfx_store16(bo + i, v4f{0.0f, 0.0f, 0.0f, 0.0f});
    }
    if (lane == 0) a.count[r] = cnt;
  }
}

#endif  // DFX_NMS_KERNELS

}  // namespace dfx
