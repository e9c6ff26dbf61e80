// dilconv.hip -- the dilated conv's kernels: the instances of the K-slabbed MFMA kernel (dilconv.cuh) and the generic
// backstop (one thread per output element, the formula of include/dfx.h, any window / stride / dilation / padding /
// channel counts, the exact requant route).
#include "dilconv.cuh"

namespace dfx {

__global__ __launch_bounds__(256) void dilconv_generic_kernel(DlArgs a) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < a.items; id += stride) {
    const int k = (int)(id % a.oc);
    const long long px = id / a.oc;
    const int ox = (int)(px % a.ow);
    const long long r = px / a.ow;
    const int oy = (int)(r % a.oh), n = (int)(r / a.oh);
    int acc = 0;
    for (int ky = 0; ky < a.kh; ++ky) {
      const int y = oy * a.sh - a.pt + ky * a.dh;  // |.| < 2^31: oy * sh - pt <= ih - 1 (validated), ky * dh <= 254 * 255
      if (y < 0) continue;
      if (y >= a.ih) break;  // larger ky only raise it
      for (int kx = 0; kx < a.kw; ++kx) {
        const int x = ox * a.sw - a.pl + kx * a.dw;
        if (x < 0) continue;
        if (x >= a.iw) break;
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
template <int R, int DST, bool FAST>
static int dl_one(const DlArgs &a, int grid, int lds, hipStream_t s, int mode) {
  auto k = dilconv_mfma_kernel<R, DST, FAST>;
  if (mode == 1) return (int)hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  k<<<grid, DL_THREADS, lds, s>>>(a);
  return 0;
}

template <int R>
static int dl_r(const DlArgs &a, int grid, int lds, hipStream_t s, int mode, bool fast) {
#define DL_LAUNCH(DST) return fast ? dl_one<R, DST, true>(a, grid, lds, s, mode) : dl_one<R, DST, false>(a, grid, lds, s, mode)
  switch (a.dst_dt) {
    case DFX_F32: DL_LAUNCH(DFX_F32);
    case DFX_S32: DL_LAUNCH(DFX_S32);
    case DFX_S8: DL_LAUNCH(DFX_S8);
    case DFX_U8: DL_LAUNCH(DFX_U8);
  }
#undef DL_LAUNCH
  return -1;
}

// MFMA path: 3x3, stride (1,1), 1 .. DL_MAX_STRIPS strips per wave (checked by the host); -1: no such instance
int launch_dilconv_mfma(const DlArgs &a, int grid, int lds, hipStream_t s, int mode, bool fast) {
  if (a.kh != 3 || a.kw != 3 || a.sh != 1 || a.sw != 1) return -1;
  if (a.rstrips == 1) return dl_r<1>(a, grid, lds, s, mode, fast);
  if constexpr (DL_MAX_STRIPS >= 2) {
    if (a.rstrips == 2) return dl_r<DL_MAX_STRIPS>(a, grid, lds, s, mode, fast);
  }
  return -1;
}

int launch_dilconv_generic(const DlArgs &a, int grid, hipStream_t s) {
  dilconv_generic_kernel<<<grid, 256, 0, s>>>(a);
  return 0;
}

}  // namespace dfx
