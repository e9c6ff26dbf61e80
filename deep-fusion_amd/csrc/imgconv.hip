// imgconv.hip -- the first-layer conv's kernels: the instances of the MFMA kernel (imgconv.cuh) and the generic backstop
// (one thread per output element, any window / stride / ic <= 4 / oc, the exact requant route).
#include "imgconv.cuh"

namespace dfx {

__global__ __launch_bounds__(256) void imgconv_generic_kernel(IcArgs a) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < a.items; id += stride) {
    const int k = (int)(id % a.oc);
    const long long px = id / a.oc;
    const int ox = (int)(px % a.ow);
    const long long r = px / a.ow;
    const int oy = (int)(r % a.oh), n = (int)(r / a.oh);
    const int y0 = oy * a.sh - a.pt, x0 = ox * a.sw - a.pl;
    int acc = 0;
    for (int ky = 0; ky < a.kh; ++ky) {
      const int y = y0 + ky;
      if (y < 0 || y >= a.ih) continue;
      for (int kx = 0; kx < a.kw; ++kx) {
        const int x = x0 + kx;
        if (x < 0 || x >= a.iw) continue;
        const unsigned char *sp = a.src + (((size_t)n * a.ih + y) * a.iw + x) * a.ic;
        const signed char *wp = a.wraw + ((size_t)k * a.ic * a.kh + ky) * a.kw + kx;
        for (int i = 0; i < a.ic; ++i) acc += (int)sp[i] * (int)wp[(size_t)i * a.kh * a.kw];
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
template <int K, int S, int DST, bool FAST>
static int ic_one(const IcArgs &a, int grid, int lds, hipStream_t s, int mode) {
  auto k = imgconv_mfma_kernel<K, S, DST, FAST>;
  if (mode == 1) return (int)hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  k<<<grid, IC_THREADS, lds, s>>>(a);
  return 0;
}

template <int K, int S>
static int ic_ks(const IcArgs &a, int grid, int lds, hipStream_t s, int mode, bool fast) {
#define IC_LAUNCH(DST) return fast ? ic_one<K, S, DST, true>(a, grid, lds, s, mode) : ic_one<K, S, DST, false>(a, grid, lds, s, mode)
  switch (a.dst_dt) {
    case DFX_F32: IC_LAUNCH(DFX_F32);
    case DFX_S32: IC_LAUNCH(DFX_S32);
    case DFX_S8: IC_LAUNCH(DFX_S8);
    case DFX_U8: IC_LAUNCH(DFX_U8);
  }
#undef IC_LAUNCH
  return -1;
}

// MFMA path: (window, stride) in {7x7 / 2, 3x3 / 1, 3x3 / 2} (checked by the host); -1: no such instance
int launch_imgconv_mfma(const IcArgs &a, int grid, int lds, hipStream_t s, int mode, bool fast) {
  if (a.kh == 7 && a.sh == 2) return ic_ks<7, 2>(a, grid, lds, s, mode, fast);
  if (a.kh == 3 && a.sh == 1) return ic_ks<3, 1>(a, grid, lds, s, mode, fast);
  if (a.kh == 3 && a.sh == 2) return ic_ks<3, 2>(a, grid, lds, s, mode, fast);
  return -1;
}

int launch_imgconv_generic(const IcArgs &a, int grid, hipStream_t s) {
  imgconv_generic_kernel<<<grid, 256, 0, s>>>(a);
  return 0;
}

}  // namespace dfx
