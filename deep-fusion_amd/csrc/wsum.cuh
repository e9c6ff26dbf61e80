// wsum.cuh -- kernels of the scaled element-wise sum (dfx_wsum_* of include/dfx.h; gfx950).  HBM-bound work, no MFMA.
// For element (n,y,x,k), every f32 operation rounded separately (the library is built with -ffp-contract=off):
//   v = float(src_0) * s_0[k];  v = v + float(src_i) * s_i[k] (i = 1 .. n-1);  v = v + bias[k];  v = vmaxps(+0, v);
//   f32 dst: v;  u8 / s8 dst: the reorder's conversion (rint or floor, NaN -> 0, clamp);  table: lut[cvt<lut_in>(v) (+ 128)]
// Both kernels evaluate it with the same functions below, so they give the same bits.
//   wsum_generic_kernel  one thread per output element: any c, any alignment the op accepts; everything a runtime switch
//   wsum_vec_kernel      one lane per 16 consecutive channels of a pixel.  Consecutive lanes take consecutive groups, so a
//                        wave reads and writes one contiguous span per tensor.  The handle's image of the per-channel
//                        constants and the table (wsum_plan.h) is copied into LDS once per workgroup; per-tensor scales
//                        are kernel arguments.  The inputs are a runtime loop with a wave-uniform switch on the dtype:
//                        there is one instance per (dst kind, ReLU, round mode), none per tuple of input dtypes or per n.
#pragma once

#include "dfx_device.cuh"

namespace dfx {

struct WsumArgs {
  const unsigned char *src[DFX_WSUM_MAX_INPUTS];
  unsigned char *dst;
  const unsigned char *image;       // device image of the per-channel constants and the table (wsum_plan.h); null: none
  float s1[DFX_WSUM_MAX_INPUTS];    // per-tensor scales (unused where slot[i] >= 0)
  float b1;                         // per-tensor bias
  int dt[DFX_WSUM_MAX_INPUTS];
  int slot[DFX_WSUM_MAX_INPUTS];    // slot of input i's per-channel scales in the image, -1: per tensor
  int bias_slot;                    // slot of the per-channel bias, -1: per tensor or none
  int has_bias;
  int n, c, groups;                 // groups: 16-channel groups per pixel (vec kernel)
  int relu, rm, dst_dt, lut_in_dt;
  int image_bytes, lut_off;         // image_bytes: a multiple of 16
  long long total;                  // work items: elements (generic) or 16-channel groups (vec)
};

enum { WSUM_OUT_F32 = 0, WSUM_OUT_U8 = 1, WSUM_OUT_S8 = 2, WSUM_OUT_LUT = 3 };

// the reorder's conversion to a 1-byte integer type: rint (ties to even) or floor, NaN -> 0, clamp to the range
__device__ __forceinline__ int wsum_cvt(float v, int rm, bool is_u8) {
  float r = rm ? __builtin_floorf(v) : __builtin_rintf(v);
  const float lo = is_u8 ? 0.0f : -128.0f, hi = is_u8 ? 255.0f : 127.0f;
  r = (v != v) ? 0.0f : r;
  r = r < lo ? lo : (r > hi ? hi : r);
  return (int)r;
}
// index into the table: dfx_se's convention
__device__ __forceinline__ int wsum_lut_index(float v, int rm, int lut_in_dt) {
  return lut_in_dt == DFX_U8 ? wsum_cvt(v, rm, true) : wsum_cvt(v, rm, false) + 128;
}
__device__ __forceinline__ float wsum_add_term(float v, float x, float s) { return __fadd_rn(v, __fmul_rn(x, s)); }

__device__ __forceinline__ float wsum_load1(const unsigned char *base, int dt, size_t idx) {
  if (dt == DFX_F32) return reinterpret_cast<const float *>(base)[idx];
  if (dt == DFX_S32) return __int2float_rn(reinterpret_cast<const int *>(base)[idx]);
  if (dt == DFX_U8) return (float)base[idx];
  return (float)(int)reinterpret_cast<const signed char *>(base)[idx];
}

#ifdef DFX_WSUM_KERNELS

__global__ __launch_bounds__(256) void wsum_generic_kernel(WsumArgs a) {
  const float *consts = reinterpret_cast<const float *>(a.image);
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < a.total; id += stride) {
    const int ch = (int)(id % a.c);
    float v = 0.0f;
    for (int i = 0; i < a.n; ++i) {
      const float x = wsum_load1(a.src[i], a.dt[i], (size_t)id);
      const float s = a.slot[i] >= 0 ? consts[(size_t)a.slot[i] * a.c + ch] : a.s1[i];
      v = i == 0 ? __fmul_rn(x, s) : wsum_add_term(v, x, s);
    }
    if (a.has_bias) v = __fadd_rn(v, a.bias_slot >= 0 ? consts[(size_t)a.bias_slot * a.c + ch] : a.b1);
    if (a.relu) v = relu_x86(v);
    if (a.lut_in_dt != DFX_UNDEF) a.dst[id] = a.image[a.lut_off + wsum_lut_index(v, a.rm, a.lut_in_dt)];
    else if (a.dst_dt == DFX_F32) reinterpret_cast<float *>(a.dst)[id] = v;
    else a.dst[id] = (unsigned char)wsum_cvt(v, a.rm, a.dst_dt == DFX_U8);
  }
}

extern __shared__ v4i wsum_lds[];

// x[e] * s[e] for the 16 channels from `ch` on of input i at element offset `off`
__device__ __forceinline__ void wsum_products(const WsumArgs &a, int i, size_t off, int ch, float (&p)[16]) {
  const int dt = a.dt[i];
  const unsigned char *base = a.src[i];
  float x[16];
  if (dt == DFX_U8 || dt == DFX_S8) {
    const v4i raw = *reinterpret_cast<const v4i *>(base + off);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int w = raw[e >> 2] >> (8 * (e & 3));
      x[e] = dt == DFX_U8 ? (float)(w & 0xff) : (float)(int)(signed char)(w & 0xff);
    }
  } else {
    const v4i *p4 = reinterpret_cast<const v4i *>(base + off * 4);
    v4i raw[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) raw[q] = p4[q];
#pragma unroll
    for (int e = 0; e < 16; ++e) x[e] = dt == DFX_F32 ? __int_as_float(raw[e >> 2][e & 3]) : __int2float_rn(raw[e >> 2][e & 3]);
  }
  const int slot = a.slot[i];
  if (slot >= 0) {
    const v4f *sc = reinterpret_cast<const v4f *>(reinterpret_cast<const float *>(wsum_lds) + (size_t)slot * a.c + ch);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const v4f f = sc[q];
#pragma unroll
      for (int r = 0; r < 4; ++r) p[4 * q + r] = __fmul_rn(x[4 * q + r], f[r]);
    }
  } else {
    const float s = a.s1[i];
#pragma unroll
    for (int e = 0; e < 16; ++e) p[e] = __fmul_rn(x[e], s);
  }
}

template <int OUT, bool RELU, int RM>
__global__ __launch_bounds__(256) void wsum_vec_kernel(WsumArgs a) {
  // the per-channel constants and the table, once per workgroup
  const v4i *image = reinterpret_cast<const v4i *>(a.image);
  for (int k = threadIdx.x; k < (a.image_bytes >> 4); k += 256) wsum_lds[k] = image[k];
  if (a.image_bytes) __syncthreads();
  const unsigned char *lut = reinterpret_cast<const unsigned char *>(wsum_lds) + a.lut_off;
  const long long stride = (long long)gridDim.x * 256;
  const int id0 = blockIdx.x * 256 + threadIdx.x;  // (at most 2048 workgroups)
  // the lane's channel group, kept up from step to step without a 64-bit remainder
  int g = id0 % a.groups;
  const int gstep = (int)(stride % a.groups);
  for (long long id = id0; id < a.total; id += stride) {
    const size_t off = (size_t)id * 16;  // in elements: consecutive lanes, consecutive 16-channel groups
    const int ch = g * 16;
    float v[16], p[16];
    wsum_products(a, 0, off, ch, v);
    for (int i = 1; i < a.n; ++i) {
      wsum_products(a, i, off, ch, p);
#pragma unroll
      for (int e = 0; e < 16; ++e) v[e] = __fadd_rn(v[e], p[e]);
    }
    if (a.has_bias) {
      if (a.bias_slot >= 0) {
        const v4f *b = reinterpret_cast<const v4f *>(reinterpret_cast<const float *>(wsum_lds) + (size_t)a.bias_slot * a.c + ch);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const v4f f = b[q];
#pragma unroll
          for (int r = 0; r < 4; ++r) v[4 * q + r] = __fadd_rn(v[4 * q + r], f[r]);
        }
      } else {
#pragma unroll
        for (int e = 0; e < 16; ++e) v[e] = __fadd_rn(v[e], a.b1);
      }
    }
    if (RELU) {
#pragma unroll
      for (int e = 0; e < 16; ++e) v[e] = relu_x86(v[e]);
    }
    if (OUT == WSUM_OUT_F32) {
      v4i *q4 = reinterpret_cast<v4i *>(a.dst + off * 4);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const v4i o = {__float_as_int(v[4 * q]), __float_as_int(v[4 * q + 1]), __float_as_int(v[4 * q + 2]), __float_as_int(v[4 * q + 3])};
        dfx_store16(q4 + q, o);
      }
    } else {
      v4i o = {0, 0, 0, 0};
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        int b;
        if (OUT == WSUM_OUT_LUT) b = lut[wsum_lut_index(v[e], RM, a.lut_in_dt)];
        else b = wsum_cvt(v[e], RM, OUT == WSUM_OUT_U8) & 0xff;
        o[e >> 2] |= b << (8 * (e & 3));
      }
      dfx_store16(reinterpret_cast<v4i *>(a.dst + off), o);
    }
    g += gstep;
    if (g >= a.groups) g -= a.groups;
  }
}

#endif  // DFX_WSUM_KERNELS

}  // namespace dfx
