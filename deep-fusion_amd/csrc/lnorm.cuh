// lnorm.cuh -- kernels of the int8 layer norm / RMS norm (dfx_lnorm_* of include/dfx.h; gfx950).  HBM-bound work, no MFMA.
//
// Per row: t_k = x_k * 2^shift[k]; S = sum t_k and Q = sum t_k^2 are EXACT integers (lnorm_plan.h restates the bounds), so the
// order in which lanes add them does not matter.  Everything behind them -- lnorm_scale() and lnorm_value() below, called
// by both kernels -- is a fixed sequence of single-rounded f32 operations (the library is built with -ffp-contract=off), so
// both kernels give the same bits.  sqrtf() here is the correctly rounded one (v_sqrt_f32 plus its correction);
// __fsqrt_rn is NOT: it compiles to the bare instruction.
//
//   lnorm_generic_kernel   one thread per row, sequential, any alignment and leading dimension: defines the arithmetic
//   lnorm_row_kernel<W>    W in {4, 8, 16, 32, 64} consecutive lanes own a row, 256 / W rows per workgroup trip.  A lane
//                          loads the 16-byte groups lane, lane + W, ...; its first four stay in registers over both passes
//                          (statistics, store), further ones are re-read, from L2.  Without shifts the statistics are
//                          v_dot4 products; with shifts plain integer VALU.  The lanes of a row meet through __shfl_xor
//                          butterflies.  gamma / beta are staged once per workgroup in LDS where the plan has room.
//                          Every lane of a row computes the row's `a` from the same inputs; the per-element tail has no
//                          division.  Whole groups leave as 16-byte stores, the last group element by element.
#pragma once

#include "dfx_device.cuh"
#include "lnorm_plan.h"

namespace dfx {

struct LnormArgs {
  const unsigned char *src;
  unsigned char *dst;
  const float *gamma, *beta;     // the handle's device image: whole 16-channel groups, pads 0
  const unsigned char *shift;    // likewise; null: no shifts
  long long rows;
  int c, src_ld, dst_ld;
  int mode, src_dt, dst_dt;
  int stage;                     // row kernel: gamma / beta go through LDS (8 * up16(c) bytes of dynamic LDS)
  float eps;
};

__device__ __forceinline__ int lnorm_elem(unsigned byte, int src_dt) { return src_dt == DFX_U8 ? (int)byte : (int)(signed char)byte; }

// the row's factor `a` from its exact statistics
__device__ __forceinline__ float lnorm_scale(int mode, int c, int S, unsigned long long Q, float eps) {
  const float fc = __int2float_rn(c);  // exact
  if (mode == DFX_LNORM_LAYER) {
    const unsigned long long D = (unsigned long long)c * Q - (unsigned long long)((long long)S * S);
    const float v = __fdiv_rn(__ull2float_rn(D), __int2float_rn(c * c));
    return __fdiv_rn(__fdiv_rn(1.0f, sqrtf(__fadd_rn(v, eps))), fc);
  }
  const float v = __fdiv_rn(__ull2float_rn(Q), fc);
  return __fdiv_rn(1.0f, sqrtf(__fadd_rn(v, eps)));
}
// u_k from t_k
__device__ __forceinline__ int lnorm_centre(int mode, int c, int S, int t) { return mode == DFX_LNORM_LAYER ? c * t - S : t; }
__device__ __forceinline__ float lnorm_value(int u, float a, float gamma, float beta) {
  return __fadd_rn(__fmul_rn(__fmul_rn(__int2float_rn(u), a), gamma), beta);
}
// the reorder's conversion to a 1-byte integer type: rint (ties to even), NaN -> 0, clamp to the range
__device__ __forceinline__ int lnorm_cvt(float v, bool is_u8) {
  float r = __builtin_rintf(v);
  const float lo = is_u8 ? 0.0f : -128.0f, hi = is_u8 ? 255.0f : 127.0f;
  r = (v != v) ? 0.0f : r;
  r = r < lo ? lo : (r > hi ? hi : r);
  return (int)r;
}

#ifdef DFX_LNORM_KERNELS

// ---- generic: one thread per row -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lnorm_generic_kernel(LnormArgs a) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long row = (long long)blockIdx.x * 256 + threadIdx.x; row < a.rows; row += stride) {
    const unsigned char *p = a.src + (size_t)row * a.src_ld;
    int S = 0;
    unsigned long long Q = 0;
    for (int j = 0; j < a.c; ++j) {
      const int t = lnorm_elem(p[j], a.src_dt) * (1 << (a.shift ? a.shift[j] : 0));
      S += t;
      Q += (unsigned long long)(t * t);
    }
    const float f = lnorm_scale(a.mode, a.c, S, Q, a.eps);
    const size_t o = (size_t)row * a.dst_ld;
    for (int j = 0; j < a.c; ++j) {
      const int t = lnorm_elem(p[j], a.src_dt) * (1 << (a.shift ? a.shift[j] : 0));
      const float y = lnorm_value(lnorm_centre(a.mode, a.c, S, t), f, a.gamma[j], a.beta[j]);
      if (a.dst_dt == DFX_F32) reinterpret_cast<float *>(a.dst)[o + j] = y;
      else a.dst[o + j] = (unsigned char)lnorm_cvt(y, a.dst_dt == DFX_U8);
    }
  }
}

// ---- row: W lanes per row --------------------------------------------------------------------------------------------------
template <int W>
__device__ __forceinline__ int lnorm_lanes_sum(int x) {
#pragma unroll
  for (int m = W / 2; m >= 1; m >>= 1) x += __shfl_xor(x, m);
  return x;
}
template <int W>
__device__ __forceinline__ unsigned long long lnorm_lanes_sum(unsigned long long x) {
#pragma unroll
  for (int m = W / 2; m >= 1; m >>= 1) x += __shfl_xor(x, m);
  return x;
}

__device__ __forceinline__ unsigned lnorm_byte(const v4i &raw, int e) { return ((unsigned)raw[e >> 2] >> (8 * (e & 3))) & 0xffu; }

// `raw` with the bytes of channels nvalid .. 15 cleared (they add nothing to S and Q then)
__device__ __forceinline__ v4i lnorm_mask(const v4i &raw, int nvalid) {
  v4i m;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int left = nvalid - 4 * q;  // valid bytes of this dword
    const unsigned keep = left >= 4 ? 0xffffffffu : left <= 0 ? 0u : (0xffffffffu >> (8 * (4 - left)));
    m[q] = (int)((unsigned)raw[q] & keep);
  }
  return m;
}

template <int W, bool SHIFT>
__global__ __launch_bounds__(256) void lnorm_row_kernel(LnormArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lnorm_lds[];
  constexpr int ROWS = 256 / W;
  const int groups = (a.c + 15) / 16;
  const int cp = groups * 16;
  float *lg = reinterpret_cast<float *>(lnorm_lds), *lb = lg + cp;
  if (a.stage) {
    for (int i = threadIdx.x; i < cp; i += 256) {
      lg[i] = a.gamma[i];
      lb[i] = a.beta[i];
    }
    __syncthreads();
  }
  const int lane = threadIdx.x & (W - 1), sub = threadIdx.x / W;
  const bool is_u8 = a.src_dt == DFX_U8, out_u8 = a.dst_dt == DFX_U8, out_f32 = a.dst_dt == DFX_F32;
  const long long stride = (long long)gridDim.x * ROWS;
  const v4i zero = {0, 0, 0, 0};
  for (long long base = (long long)blockIdx.x * ROWS; base < a.rows; base += stride) {  // (uniform: the shuffles need every lane)
    const bool active = base + sub < a.rows;
    const long long row = active ? base + sub : a.rows - 1;  // idle lanes repeat the last row and store nothing
    const v4i *p = reinterpret_cast<const v4i *>(a.src + (size_t)row * a.src_ld);
    const v4i *ps = reinterpret_cast<const v4i *>(a.shift);
    v4i keep[LNORM_KEEP];
#pragma unroll
    for (int i = 0; i < LNORM_KEEP; ++i) keep[i] = lane + i * W < groups ? p[lane + i * W] : zero;
    // f(raw, g) over the lane's groups: the kept ones, then the re-read ones
    auto each_group = [&](auto f) {
#pragma unroll
      for (int i = 0; i < LNORM_KEEP; ++i)
        if (lane + i * W < groups) f(keep[i], lane + i * W);
      for (int g = lane + LNORM_KEEP * W; g < groups; g += W) f(p[g], g);
    };

    // pass 1: the exact statistics
    int S = 0;
    unsigned long long Q = 0;
    if (SHIFT) {
      each_group([&](const v4i &raw, int g) {
        const v4i sh = ps[g];
        const int left = a.c - g * 16;
        int s = 0;
        unsigned long long q = 0;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int t = e < left ? lnorm_elem(lnorm_byte(raw, e), a.src_dt) * (1 << lnorm_byte(sh, e)) : 0;
          s += t;
          q += (unsigned)(t * t);
        }
        S += s;
        Q += q;
      });
    } else {
      unsigned q32 = 0;  // (a whole unshifted row's Q fits u32: lnorm_plan.h)
      each_group([&](const v4i &raw, int g) {
        const int left = a.c - g * 16;
        const v4i m = left < 16 ? lnorm_mask(raw, left) : raw;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          if (is_u8) {
            S = (int)__builtin_amdgcn_udot4((unsigned)m[d], 0x01010101u, (unsigned)S, false);
            q32 = __builtin_amdgcn_udot4((unsigned)m[d], (unsigned)m[d], q32, false);
          } else {
            S = __builtin_amdgcn_sdot4(m[d], 0x01010101, S, false);
            q32 = (unsigned)__builtin_amdgcn_sdot4(m[d], m[d], (int)q32, false);
          }
        }
      });
      Q = q32;
    }
    S = lnorm_lanes_sum<W>(S);
    Q = lnorm_lanes_sum<W>(Q);
    const float f = lnorm_scale(a.mode, a.c, S, Q, a.eps);

    // pass 2: the values
    unsigned char *dst_row = a.dst + (size_t)row * a.dst_ld * (out_f32 ? 4 : 1);
    each_group([&](const v4i &raw, int g) {
      if (!active) return;
      const int left = a.c - g * 16;
      v4i sh = zero;
      if (SHIFT) sh = ps[g];
      float y[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        v4f gm, bt;
        if (a.stage) {
          gm = *reinterpret_cast<const v4f *>(lg + g * 16 + 4 * q);
          bt = *reinterpret_cast<const v4f *>(lb + g * 16 + 4 * q);
        } else {
          gm = *reinterpret_cast<const v4f *>(a.gamma + g * 16 + 4 * q);
          bt = *reinterpret_cast<const v4f *>(a.beta + g * 16 + 4 * q);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int e = 4 * q + j;
          int t = lnorm_elem(lnorm_byte(raw, e), a.src_dt);
          if (SHIFT) t *= 1 << lnorm_byte(sh, e);
          y[e] = lnorm_value(lnorm_centre(a.mode, a.c, S, t), f, gm[j], bt[j]);
        }
      }
      if (out_f32) {
        float *q = reinterpret_cast<float *>(dst_row) + (size_t)g * 16;
        if (left >= 16) {
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const v4i o = {__float_as_int(y[4 * v]), __float_as_int(y[4 * v + 1]), __float_as_int(y[4 * v + 2]), __float_as_int(y[4 * v + 3])};
            dfx_store16(reinterpret_cast<v4i *>(q) + v, o);
          }
        } else {
#pragma unroll
          for (int e = 0; e < 16; ++e)
            if (e < left) q[e] = y[e];
        }
      } else {
        unsigned char *q = dst_row + (size_t)g * 16;
        int by[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) by[e] = lnorm_cvt(y[e], out_u8) & 0xff;
        if (left >= 16) {
          v4i o = {0, 0, 0, 0};
#pragma unroll
          for (int e = 0; e < 16; ++e) o[e >> 2] |= by[e] << (8 * (e & 3));
          dfx_store16(reinterpret_cast<v4i *>(q), o);
        } else {
#pragma unroll
          for (int e = 0; e < 16; ++e)
            if (e < left) q[e] = (unsigned char)by[e];
        }
      }
    });
  }
}

#endif  // DFX_LNORM_KERNELS

}  // namespace dfx
