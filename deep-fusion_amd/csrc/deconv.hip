// deconv.hip -- the transposed conv's kernels: the instances of the sub-pixel MFMA kernel (deconv.cuh) and the generic
// backstop (one thread per output element, the gather formula of include/dfx.h, any window / stride / padding / channel
// counts, the exact requant route).
#include "deconv.cuh"

namespace dfx {

__global__ __launch_bounds__(256) void deconv_generic_kernel(DcArgs a) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < a.items; id += stride) {
    const int k = (int)(id % a.oc);
    const long long px = id / a.oc;
    const int ox = (int)(px % a.ow);
    const long long r = px / a.ow;
    const int oy = (int)(r % a.oh), n = (int)(r / a.oh);
    int acc = 0;
    for (int ky = 0; ky < a.kh; ++ky) {
      const int ty = oy + a.pt - ky;  // = iy * sh
      if (ty < 0) break;              // larger ky only lower it
      const int y = ty / a.sh;
      if (ty - y * a.sh != 0 || y >= a.ih) continue;
      for (int kx = 0; kx < a.kw; ++kx) {
        const int tx = ox + a.pl - kx;
        if (tx < 0) break;
        const int x = tx / a.sw;
        if (tx - x * a.sw != 0 || x >= a.iw) continue;
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
template <int T, int DST, bool FAST>
static int dc_one(const DcArgs &a, int grid, int lds, hipStream_t s, int mode) {
  auto k = deconv_mfma_kernel<T, DST, FAST>;
  if (mode == 1) return (int)hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  k<<<grid, DC_THREADS, lds, s>>>(a);
  return 0;
}

template <int T>
static int dc_t(const DcArgs &a, int grid, int lds, hipStream_t s, int mode, bool fast) {
#define DC_LAUNCH(DST) return fast ? dc_one<T, DST, true>(a, grid, lds, s, mode) : dc_one<T, DST, false>(a, grid, lds, s, mode)
  switch (a.dst_dt) {
    case DFX_F32: DC_LAUNCH(DFX_F32);
    case DFX_S32: DC_LAUNCH(DFX_S32);
    case DFX_S8: DC_LAUNCH(DFX_S8);
    case DFX_U8: DC_LAUNCH(DFX_U8);
  }
#undef DC_LAUNCH
  return -1;
}

// MFMA path: stride (2,2), window 2x2 (T = 1), 3x3 or 4x4 (T = 2) (checked by the host); -1: no such instance
int launch_deconv_mfma(const DcArgs &a, int grid, int lds, hipStream_t s, int mode, bool fast) {
  if (a.sh != 2 || a.sw != 2 || a.kh != a.kw) return -1;
  if (a.kh == 2) return dc_t<1>(a, grid, lds, s, mode, fast);
  if (a.kh == 3 || a.kh == 4) return dc_t<2>(a, grid, lds, s, mode, fast);
  return -1;
}

int launch_deconv_generic(const DcArgs &a, int grid, hipStream_t s) {
  deconv_generic_kernel<<<grid, 256, 0, s>>>(a);
  return 0;
}

}  // namespace dfx
