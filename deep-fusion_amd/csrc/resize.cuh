// resize.cuh -- kernels of the activation resize (dfx_resize_* of include/dfx.h; gfx950).  HBM-bound work, no MFMA.
// Both kernels read the per-axis tables resize_plan.h built on the host (two source indices and two weights per output
// row / column) and evaluate, for bilinear,
//   top = v[y0,x0]*wx0 + v[y0,x1]*wx1;  bot = v[y1,x0]*wx0 + v[y1,x1]*wx1;  out = top*wy0 + bot*wy1
// with every multiply and add rounded separately (the library is built with -ffp-contract=off), so one kernel serves
// all three coordinate modes and the two kernels give the same bits.
//   resize_generic_kernel  one thread per output element: any c, any alignment the op accepts
//   resize_band_kernel     one lane per 16 bytes of channels of one output column and a band of output rows: `top` and
//                          `bot` stay in registers down the band and only what the next row changes is rebuilt
#pragma once

#include <type_traits>

#include "dfx_device.cuh"

namespace dfx {

struct ResizeArgs {
  const unsigned char *src;
  const unsigned char *add;  // null without the fused add; may be dst
  unsigned char *dst;
  const int *y0, *y1, *x0, *x1;          // device tables: oh / ow entries each
  const float *wy0, *wy1, *wx0, *wx1;
  int bs, c, ih, iw, oh, ow, dt, algo, relu;
  int rows;         // band kernel: output rows per lane
  int bands;        // band kernel: bands per image, ceil(oh / rows)
  int groups;       // band kernel: 16-byte channel groups per pixel
  long long total;  // work items: output elements (generic) or bs * bands * ow * groups (band)
};

// rint (ties to even) and the clamp of the reorder's conversion; f32 stores the value as it is
template <typename T> __device__ __forceinline__ T resize_cvt(float v);
template <> __device__ __forceinline__ float resize_cvt<float>(float v) { return v; }
template <> __device__ __forceinline__ signed char resize_cvt<signed char>(float v) {
  return (signed char)min(127, max(-128, (int)__builtin_rintf(v)));
}
template <> __device__ __forceinline__ unsigned char resize_cvt<unsigned char>(float v) {
  return (unsigned char)min(255, max(0, (int)__builtin_rintf(v)));
}

// dfx_eltwise's two-input sum: the resized value first, then the added tensor's
template <typename T>
__device__ __forceinline__ T resize_sum(T r, T a, bool relu) {
  typedef typename EltAcc<T>::type A;
  return elt_finish<T>((A)r + (A)a, relu);
}

// one horizontal interpolation, the formula's `top` / `bot`
__device__ __forceinline__ float resize_lerp(float a, float b, float w0, float w1) {
  return __fadd_rn(__fmul_rn(a, w0), __fmul_rn(b, w1));
}

template <typename T>
__global__ __launch_bounds__(256) void resize_generic_kernel(ResizeArgs a) {
  const T *src = reinterpret_cast<const T *>(a.src);
  const T *add = reinterpret_cast<const T *>(a.add);
  T *dst = reinterpret_cast<T *>(a.dst);
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < a.total; id += stride) {
    const int ch = (int)(id % a.c);
    long long t = id / a.c;
    const int ox = (int)(t % a.ow);
    t /= a.ow;
    const int oy = (int)(t % a.oh), n = (int)(t / a.oh);
    const T *img = src + (size_t)n * a.ih * a.iw * a.c + ch;
    const int y0 = a.y0[oy], x0 = a.x0[ox];
    T r;
    if constexpr (std::is_same<T, int>::value) {
      r = img[((size_t)y0 * a.iw + x0) * a.c];  // (s32: nearest only)
    } else {
      if (a.algo == DFX_RESIZE_NEAREST) {
        r = img[((size_t)y0 * a.iw + x0) * a.c];
      } else {
        const int y1 = a.y1[oy], x1 = a.x1[ox];
        const float wx0 = a.wx0[ox], wx1 = a.wx1[ox];
        const float top = resize_lerp((float)img[((size_t)y0 * a.iw + x0) * a.c], (float)img[((size_t)y0 * a.iw + x1) * a.c], wx0, wx1);
        const float bot = resize_lerp((float)img[((size_t)y1 * a.iw + x0) * a.c], (float)img[((size_t)y1 * a.iw + x1) * a.c], wx0, wx1);
        r = resize_cvt<T>(resize_lerp(top, bot, a.wy0[oy], a.wy1[oy]));
      }
    }
    if (add) r = resize_sum<T>(r, add[id], a.relu != 0);
    dst[id] = r;
  }
}

// 16 bytes of T as N values
template <typename T>
union ResizeVec {
  v4i v;
  T e[16 / sizeof(T)];
};

// the horizontal interpolation of 16 bytes of channels of source row `row` (a pointer to its first pixel's group)
template <typename T>
__device__ __forceinline__ void resize_hrow(const T *row, int x0, int x1, int c, float wx0, float wx1, float (&out)[16 / sizeof(T)]) {
  constexpr int N = 16 / (int)sizeof(T);
  ResizeVec<T> p, q;
  p.v = *reinterpret_cast<const v4i *>(row + (size_t)x0 * c);
  q.v = *reinterpret_cast<const v4i *>(row + (size_t)x1 * c);
#pragma unroll
  for (int e = 0; e < N; ++e) out[e] = resize_lerp((float)p.e[e], (float)q.e[e], wx0, wx1);
}

template <typename T, int ALGO, bool ADD>
__global__ __launch_bounds__(256) void resize_band_kernel(ResizeArgs a) {
  constexpr int N = 16 / (int)sizeof(T);
  const T *src = reinterpret_cast<const T *>(a.src);
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < a.total; id += stride) {
    // consecutive lanes: consecutive channel groups, then consecutive output columns -- coalesced stores
    const int g = (int)(id % a.groups);
    long long t = id / a.groups;
    const int ox = (int)(t % a.ow);
    t /= a.ow;
    const int band = (int)(t % a.bands), n = (int)(t / a.bands);
    const int oy_begin = band * a.rows, oy_end = min(a.oh, oy_begin + a.rows);
    const T *img = src + (size_t)n * a.ih * a.iw * a.c + (size_t)g * N;
    const size_t dst_px = ((size_t)n * a.oh * a.ow + ox) * a.c + (size_t)g * N;  // + oy * ow * c
    const int x0 = a.x0[ox], x1 = a.x1[ox];
    const float wx0 = a.wx0[ox], wx1 = a.wx1[ox];
    int cy0 = -1, cy1 = -1;  // the source rows `top` and `bot` (nearest: `held`) were built from
    float top[N], bot[N];
    ResizeVec<T> held;
    for (int oy = oy_begin; oy < oy_end; ++oy) {
      const int y0 = a.y0[oy];
      ResizeVec<T> r;
      if constexpr (ALGO == DFX_RESIZE_NEAREST) {
        if (y0 != cy0) held.v = *reinterpret_cast<const v4i *>(img + ((size_t)y0 * a.iw + x0) * a.c);
        cy0 = y0;
        r.v = held.v;
      } else {
        const int y1 = a.y1[oy];
        if (y0 != cy0) {
          if (y0 == cy1) {  // the walk moved down one source row: the old `bot` is the new `top`
#pragma unroll
            for (int e = 0; e < N; ++e) top[e] = bot[e];
          } else {
            resize_hrow<T>(img + (size_t)y0 * a.iw * a.c, x0, x1, a.c, wx0, wx1, top);
          }
        }
        if (y1 != cy1 || cy0 < 0) {
          if (y1 == y0) {  // clamped at the last source row
#pragma unroll
            for (int e = 0; e < N; ++e) bot[e] = top[e];
          } else {
            resize_hrow<T>(img + (size_t)y1 * a.iw * a.c, x0, x1, a.c, wx0, wx1, bot);
          }
        }
        cy0 = y0;
        cy1 = y1;
        const float wy0 = a.wy0[oy], wy1 = a.wy1[oy];
#pragma unroll
        for (int e = 0; e < N; ++e) r.e[e] = resize_cvt<T>(resize_lerp(top[e], bot[e], wy0, wy1));
      }
      const size_t off = dst_px + (size_t)oy * a.ow * a.c;
      if constexpr (ADD) {
        ResizeVec<T> s;
        s.v = *reinterpret_cast<const v4i *>(reinterpret_cast<const T *>(a.add) + off);
#pragma unroll
        for (int e = 0; e < N; ++e) r.e[e] = resize_sum<T>(r.e[e], s.e[e], a.relu != 0);
      }
      dfx_store16(reinterpret_cast<v4i *>(reinterpret_cast<T *>(a.dst) + off), r.v);
    }
  }
}

}  // namespace dfx
