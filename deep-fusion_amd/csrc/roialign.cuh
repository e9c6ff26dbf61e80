// roialign.cuh -- kernels of RoIAlign (dfx_roialign_* of include/dfx.h; gfx950).  No MFMA.
//
// Every floating-point step is one __f*_rn call in the order of the definition, so both kernels give the same bits.
//
//   roialign_generic_kernel   a thread per output element: it works out its RoI's level and start / bin size, then its S * S
//                             samples, each with its own coordinates.  Any c, ld and alignment.  Defines the bits.
//   roialign_tile_kernel      a workgroup per RoI, or per run of bin rows of one RoI (roialign_plan.h).  Every lane works out
//                             the RoI's level, start and bin size itself (uniform loads); the lanes then write the run's y
//                             entries and the x entries -- low / high byte offset, the two weights, valid -- into LDS; one
//                             barrier; then a lane owns one 16-byte channel group of one bin: four 16-byte corner loads per
//                             sample, bytes converted in registers, the defined accumulation order, one 16-byte store.
// An invalid coordinate (a NaN among them) never reaches an int conversion or an address: its entry is offset 0 with the
// valid bit clear, and a sample with a clear bit adds +0.0f, which leaves the accumulator's bits as they are (the
// accumulator starts at +0.0f and a sum with +0.0f is never -0.0f), so it is skipped.
#pragma once

#include "dfx_device.cuh"
#include "roialign_plan.h"

namespace dfx {

struct RoiArgs {
  const void *src[4];
  const float *boxes;
  const int *count;              // BATCHED, or null
  const int *batch_idx;          // LIST
  void *dst;
  int h[4], w[4], ld[4];
  float scale[4], thr[3];
  int bs, n, mode, levels, c, ph, pw, S, aligned, dst_ld;
  int rows_per_group, splits;    // tile path
  unsigned long long elements;   // generic path: R * ph * pw * c
};

#ifdef DFX_ROIALIGN_KERNELS

template <typename V> __device__ __forceinline__ V roi_pick(const V (&v)[4], int l) {
  return l == 0 ? v[0] : l == 1 ? v[1] : l == 2 ? v[2] : v[3];
}

// what a RoI needs before its samples
struct RoiHead {
  bool live;                     // false: the row is zeros
  int img, level;
  float rsw, rsh, bw, bh;
};

__device__ __forceinline__ RoiHead roi_head(const RoiArgs &a, unsigned r) {
  RoiHead hd = {};
  if (a.mode == DFX_ROI_BATCHED) {
    hd.img = (int)(r / (unsigned)a.n);
    int nv = a.n;
    if (a.count) {
      const int cnt = a.count[hd.img];
      nv = cnt < 0 ? 0 : cnt > a.n ? a.n : cnt;
    }
    hd.live = (int)(r % (unsigned)a.n) < nv;
  } else {
    hd.img = a.batch_idx[r];
    hd.live = hd.img >= 0 && hd.img < a.bs;
  }
  if (!hd.live) return hd;
  const float *b = a.boxes + (size_t)r * 4;
  const float x1 = b[0], y1 = b[1], x2 = b[2], y2 = b[3];
  const float area = __fmul_rn(__fsub_rn(x2, x1), __fsub_rn(y2, y1));
  int level = 0;
  for (int i = 0; i < 3; ++i)
    if (i + 1 < a.levels && area >= a.thr[i]) ++level;
  hd.level = level;
  const float s = roi_pick(a.scale, level), o = a.aligned ? 0.5f : 0.0f;
  hd.rsw = __fsub_rn(__fmul_rn(x1, s), o);
  hd.rsh = __fsub_rn(__fmul_rn(y1, s), o);
  const float rew = __fsub_rn(__fmul_rn(x2, s), o), reh = __fsub_rn(__fmul_rn(y2, s), o);
  float rw = __fsub_rn(rew, hd.rsw), rh = __fsub_rn(reh, hd.rsh);
  if (!a.aligned) {
    rw = rw > 1.0f ? rw : 1.0f;
    rh = rh > 1.0f ? rh : 1.0f;
  }
  hd.bw = __fdiv_rn(rw, (float)a.pw);
  hd.bh = __fdiv_rn(rh, (float)a.ph);
  return hd;
}

// one sample coordinate of one axis: bin p, sample i of S, over a map of L pixels
struct RoiAxis {
  int lo, hi;
  float l, h;                    // weight of hi (ly / lx), weight of lo (hy / hx)
  bool valid;
};

__device__ __forceinline__ RoiAxis roi_axis(float start, float bin, int p, int i, int S, int L) {
  float y = __fadd_rn(__fadd_rn(start, __fmul_rn((float)p, bin)), __fdiv_rn(__fmul_rn(__fadd_rn((float)i, 0.5f), bin), (float)S));
  RoiAxis e = {0, 0, 0.0f, 0.0f, false};
  e.valid = y >= -1.0f && y <= (float)L;
  if (!e.valid) return e;        // (a NaN, an Inf or a far coordinate never reaches the int conversion)
  if (y <= 0.0f) y = 0.0f;
  int yl = (int)y, yh;
  if (yl >= L - 1) {
    yh = yl = L - 1;
    y = (float)yl;
  } else {
    yh = yl + 1;
  }
  e.lo = yl;
  e.hi = yh;
  e.l = __fsub_rn(y, (float)yl);
  e.h = __fsub_rn(1.0f, e.l);
  return e;
}

// rint (ties to even) and the clamp of the reorder's conversion; f32 stores the value as it is
template <typename T> __device__ __forceinline__ T roi_cvt(float v);
template <> __device__ __forceinline__ float roi_cvt<float>(float v) { return v; }
template <> __device__ __forceinline__ signed char roi_cvt<signed char>(float v) {
  return (signed char)min(127, max(-128, (int)__builtin_rintf(v)));
}
template <> __device__ __forceinline__ unsigned char roi_cvt<unsigned char>(float v) {
  return (unsigned char)min(255, max(0, (int)__builtin_rintf(v)));
}

__device__ __forceinline__ float roi_sample(float w1, float w2, float w3, float w4, float v1, float v2, float v3, float v4) {
  return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(w1, v1), __fmul_rn(w2, v2)), __fmul_rn(w3, v3)), __fmul_rn(w4, v4));
}

// ---- generic: a thread per output element --------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(ROI_THREADS) void roialign_generic_kernel(RoiArgs a) {
  const unsigned long long stride = (unsigned long long)gridDim.x * ROI_THREADS;
  for (unsigned long long e = (unsigned long long)blockIdx.x * ROI_THREADS + threadIdx.x; e < a.elements; e += stride) {
    const int ch = (int)(e % (unsigned)a.c);
    const unsigned long long px = e / (unsigned)a.c;           // dst pixel: < 2^32 (roialign_plan.h)
    const int pwi = (int)(px % (unsigned)a.pw), phi = (int)(px / (unsigned)a.pw % (unsigned)a.ph);
    const unsigned r = (unsigned)(px / ((unsigned)a.pw * (unsigned)a.ph));
    T *out = (T *)a.dst + (size_t)px * a.dst_ld + ch;
    const RoiHead hd = roi_head(a, r);
    if (!hd.live) {
      *out = (T)0;
      continue;
    }
    const int H = roi_pick(a.h, hd.level), W = roi_pick(a.w, hd.level), ld = roi_pick(a.ld, hd.level);
    const T *img = (const T *)roi_pick(a.src, hd.level) + (size_t)hd.img * H * W * ld + ch;
    float acc = 0.0f;
    for (int iy = 0; iy < a.S; ++iy) {
      const RoiAxis y = roi_axis(hd.rsh, hd.bh, phi, iy, a.S, H);
      for (int ix = 0; ix < a.S; ++ix) {
        const RoiAxis x = roi_axis(hd.rsw, hd.bw, pwi, ix, a.S, W);
        if (!y.valid || !x.valid) continue;
        const float v1 = (float)img[((size_t)y.lo * W + x.lo) * ld], v2 = (float)img[((size_t)y.lo * W + x.hi) * ld];
        const float v3 = (float)img[((size_t)y.hi * W + x.lo) * ld], v4 = (float)img[((size_t)y.hi * W + x.hi) * ld];
        acc = __fadd_rn(acc, roi_sample(__fmul_rn(y.h, x.h), __fmul_rn(y.h, x.l), __fmul_rn(y.l, x.h), __fmul_rn(y.l, x.l), v1, v2, v3, v4));
      }
    }
    *out = roi_cvt<T>(__fdiv_rn(acc, (float)(a.S * a.S)));
  }
}

// ---- tile: a workgroup per RoI or run of bin rows ------------------------------------------------------------------------
struct RoiEntry {
  unsigned lo, hi;               // byte offsets inside the image (y: whole pixel rows; x: pixels)
  float l, h;
  int valid;
};
static_assert(sizeof(RoiEntry) == ROI_ENTRY_BYTES, "roialign_plan.h states the entry's size");

// the N f32 values of a 16-byte group
template <typename T> struct RoiGroup;
template <> struct RoiGroup<float> {
  static constexpr int N = 4;
  static __device__ __forceinline__ void unpack(const v4i &q, float (&v)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = __int_as_float(q[k]);
  }
  static __device__ __forceinline__ v4i pack(const float (&v)[4]) {
    return v4i{__float_as_int(v[0]), __float_as_int(v[1]), __float_as_int(v[2]), __float_as_int(v[3])};
  }
};
template <> struct RoiGroup<unsigned char> {
  static constexpr int N = 16;
  static __device__ __forceinline__ void unpack(const v4i &q, float (&v)[16]) {
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = (float)(((unsigned)q[k / 4] >> (8 * (k % 4))) & 0xffu);  // v_cvt_f32_ubyte0..3
  }
  static __device__ __forceinline__ v4i pack(const float (&v)[16]) {
    v4i q;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      q[k] = (int)((unsigned)roi_cvt<unsigned char>(v[4 * k]) | (unsigned)roi_cvt<unsigned char>(v[4 * k + 1]) << 8 |
                   (unsigned)roi_cvt<unsigned char>(v[4 * k + 2]) << 16 | (unsigned)roi_cvt<unsigned char>(v[4 * k + 3]) << 24);
    return q;
  }
};
template <> struct RoiGroup<signed char> {
  static constexpr int N = 16;
  static __device__ __forceinline__ void unpack(const v4i &q, float (&v)[16]) {
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = (float)((int)((unsigned)q[k / 4] << (24 - 8 * (k % 4))) >> 24);
  }
  static __device__ __forceinline__ v4i pack(const float (&v)[16]) {
    v4i q;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      q[k] = (int)((unsigned)(unsigned char)roi_cvt<signed char>(v[4 * k]) | (unsigned)(unsigned char)roi_cvt<signed char>(v[4 * k + 1]) << 8 |
                   (unsigned)(unsigned char)roi_cvt<signed char>(v[4 * k + 2]) << 16 |
                   (unsigned)(unsigned char)roi_cvt<signed char>(v[4 * k + 3]) << 24);
    return q;
  }
};

template <typename T, int S>
__global__ __launch_bounds__(ROI_THREADS) void roialign_tile_kernel(RoiArgs a) {
  using G = RoiGroup<T>;
  constexpr int N = G::N;
  __shared__ RoiEntry ty[ROI_TABLE], tx[ROI_TABLE];
  const int tid = threadIdx.x;
  const unsigned r = blockIdx.x / (unsigned)a.splits;
  const int row0 = (int)(blockIdx.x % (unsigned)a.splits) * a.rows_per_group;
  const int rows = min(a.rows_per_group, a.ph - row0);
  const int groups = a.c / N;
  const int items = rows * a.pw * groups;
  // bytes: dst and every level stay below 2^32 (roialign_plan.h)
  unsigned char *dst = (unsigned char *)a.dst + ((size_t)r * a.ph + row0) * a.pw * a.dst_ld * sizeof(T);
  const unsigned dst_px = (unsigned)a.dst_ld * sizeof(T);
  const RoiHead hd = roi_head(a, r);  // the same in every lane
  if (!hd.live) {
    for (int it = tid; it < items; it += ROI_THREADS)
      *reinterpret_cast<v4i *>(dst + (size_t)(it / groups) * dst_px + (it % groups) * 16) = v4i{0, 0, 0, 0};
    return;
  }
  const int H = roi_pick(a.h, hd.level), W = roi_pick(a.w, hd.level);
  const unsigned px_bytes = (unsigned)roi_pick(a.ld, hd.level) * sizeof(T), row_bytes = (unsigned)W * px_bytes;
  const unsigned char *img = (const unsigned char *)roi_pick(a.src, hd.level) + (size_t)hd.img * H * row_bytes;
  const int ny = rows * S, nx = a.pw * S;  // <= ROI_TABLE each
  for (int t = tid; t < ny + nx; t += ROI_THREADS) {
    const bool isy = t < ny;
    const int k = isy ? t : t - ny;
    const RoiAxis e = isy ? roi_axis(hd.rsh, hd.bh, row0 + k / S, k % S, S, H) : roi_axis(hd.rsw, hd.bw, k / S, k % S, S, W);
    const unsigned step = isy ? row_bytes : px_bytes;
    const RoiEntry out = {(unsigned)e.lo * step, (unsigned)e.hi * step, e.l, e.h, e.valid ? 1 : 0};
    if (isy) ty[k] = out;
    else tx[k] = out;
  }
  __syncthreads();
  for (int it = tid; it < items; it += ROI_THREADS) {
    const int g = it % groups, bin = it / groups, pwi = bin % a.pw, phr = bin / a.pw;
    const unsigned char *base = img + g * 16;
    float acc[N];
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0.0f;
    for (int iy = 0; iy < S; ++iy) {
      const RoiEntry y = ty[phr * S + iy];
      if (!y.valid) continue;
#pragma unroll
      for (int ix = 0; ix < S; ++ix) {
        const RoiEntry x = tx[pwi * S + ix];
        if (!x.valid) continue;
        const v4i q1 = *reinterpret_cast<const v4i *>(base + y.lo + x.lo), q2 = *reinterpret_cast<const v4i *>(base + y.lo + x.hi);
        const v4i q3 = *reinterpret_cast<const v4i *>(base + y.hi + x.lo), q4 = *reinterpret_cast<const v4i *>(base + y.hi + x.hi);
        const float w1 = __fmul_rn(y.h, x.h), w2 = __fmul_rn(y.h, x.l), w3 = __fmul_rn(y.l, x.h), w4 = __fmul_rn(y.l, x.l);
        float v1[N], v2[N], v3[N], v4[N];
        G::unpack(q1, v1);
        G::unpack(q2, v2);
        G::unpack(q3, v3);
        G::unpack(q4, v4);
#pragma unroll
        for (int k = 0; k < N; ++k) acc[k] = __fadd_rn(acc[k], roi_sample(w1, w2, w3, w4, v1[k], v2[k], v3[k], v4[k]));
      }
    }
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = __fdiv_rn(acc[k], (float)(S * S));
    *reinterpret_cast<v4i *>(dst + (size_t)bin * dst_px + g * 16) = G::pack(acc);
  }
}

#endif  // DFX_ROIALIGN_KERNELS

}  // namespace dfx
