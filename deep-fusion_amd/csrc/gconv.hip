// gconv.hip -- the grouped conv's kernels: the instances of the MFMA kernel (gconv.cuh) and the generic backstop (one
// thread per output element, any window / stride / channel counts / groups, the exact requant route).
#include "gconv.cuh"

namespace dfx {

__global__ __launch_bounds__(256) void gconv_generic_kernel(GcArgs a) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const int icg = a.ic / a.groups, ocg = a.oc / a.groups;
  for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < a.items; id += stride) {
    const int k = (int)(id % a.oc);
    const long long px = id / a.oc;
    const int ox = (int)(px % a.ow);
    const long long r = px / a.ow;
    const int oy = (int)(r % a.oh), n = (int)(r / a.oh);
    const int y0 = oy * a.sh - a.pt, x0 = ox * a.sw - a.pl;
    const int c0 = (k / ocg) * icg;  // first input channel of k's group
    int acc = 0;
    for (int ky = 0; ky < a.kh; ++ky) {
      const int y = y0 + ky;
      if (y < 0 || y >= a.ih) continue;
      for (int kx = 0; kx < a.kw; ++kx) {
        const int x = x0 + kx;
        if (x < 0 || x >= a.iw) continue;
        const unsigned char *sp = a.src + (((size_t)n * a.ih + y) * a.iw + x) * a.ic + c0;
        const signed char *wp = a.wraw + ((size_t)k * icg * a.kh + ky) * a.kw + kx;
        for (int i = 0; i < icg; ++i) acc += (int)sp[i] * (int)wp[(size_t)i * a.kh * a.kw];
      }
    }
    const float f = requant(acc, a.bias[k], a.scale[k], a.relu != 0);
    switch (a.dst_dt) {
      case DFX_F32: reinterpret_cast<float *>(a.dst)[id] = f; break;
      case DFX_S32: reinterpret_cast<int *>(a.dst)[id] = cvt_x86_rt(f, a.rm); break;
      case DFX_S8: reinterpret_cast<signed char *>(a.dst)[id] = (signed char)sat_s8(cvt_x86_rt(f, a.rm)); break;
      default: a.dst[id] = (unsigned char)sat_u8_bits(cvt_x86_rt(f, a.rm)); break;
    }
  }
}

// mode 0: launch; mode 1: admit `lds` bytes of dynamic LDS for the instance (once per handle, at create)
template <int S, int NIB, int DST, bool FAST>
static int gc_one(const GcArgs &a, int grid, int lds, hipStream_t s, int mode) {
  auto k = a.t_tr > 0 ? gconv_mfma_tile_kernel<S, NIB, DST, FAST> : gconv_mfma_kernel<S, NIB, DST, FAST>;
  if (mode == 1) return (int)hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  k<<<grid, GC_THREADS, lds, s>>>(a);
  return 0;
}

template <int S, int NIB>
static int gc_sn(const GcArgs &a, int grid, int lds, hipStream_t s, int mode, bool fast) {
#define GC_LAUNCH(DST) return fast ? gc_one<S, NIB, DST, true>(a, grid, lds, s, mode) : gc_one<S, NIB, DST, false>(a, grid, lds, s, mode)
  switch (a.dst_dt) {
    case DFX_F32: GC_LAUNCH(DFX_F32);
    case DFX_S32: GC_LAUNCH(DFX_S32);
    case DFX_S8: GC_LAUNCH(DFX_S8);
    case DFX_U8: GC_LAUNCH(DFX_U8);
  }
#undef GC_LAUNCH
  return -1;
}

// MFMA path: 3x3, sh == sw in {1, 2}, ic / groups in {4 .. 64} (checked by the host); -1: no such instance
int launch_gconv_mfma(const GcArgs &a, int grid, int lds, hipStream_t s, int mode, bool fast) {
  const bool two = a.ic / a.groups == 64;
  if (a.sh == 1) return two ? gc_sn<1, 2>(a, grid, lds, s, mode, fast) : gc_sn<1, 1>(a, grid, lds, s, mode, fast);
  if (a.sh == 2) return two ? gc_sn<2, 2>(a, grid, lds, s, mode, fast) : gc_sn<2, 1>(a, grid, lds, s, mode, fast);
  return -1;
}

int launch_gconv_generic(const GcArgs &a, int grid, hipStream_t s) {
  gconv_generic_kernel<<<grid, 256, 0, s>>>(a);
  return 0;
}

}  // namespace dfx
