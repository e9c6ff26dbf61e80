// dwconv.hip -- the depthwise conv's kernels: the instances of the sliding-window kernel (dwconv.cuh) and the generic
// backstop (one thread per output element, any window / stride / channel count, the exact requant route).
#include "dwconv.cuh"

namespace dfx {

__global__ __launch_bounds__(256) void dwconv_generic_kernel(DwArgs a) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < a.items; id += stride) {
    const int k = (int)(id % a.c);
    const long long px = id / a.c;
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
        acc += (int)a.src[(((size_t)n * a.ih + y) * a.iw + x) * a.c + k] * (int)a.wraw[((size_t)k * a.kh + ky) * a.kw + kx];
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

template <int K, int S>
static int launch_window_ks(const DwArgs &a, int grid, int block, int lds, hipStream_t s) {
  constexpr bool WLDS = K == 5;
#define DW_LAUNCH(DST)                                                                     \
  if (a.fast) dwconv_window_kernel<K, S, DST, true, WLDS><<<grid, block, lds, s>>>(a);     \
  else dwconv_window_kernel<K, S, DST, false, WLDS><<<grid, block, lds, s>>>(a);           \
  return 0
  switch (a.dst_dt) {
    case DFX_F32: DW_LAUNCH(DFX_F32);
    case DFX_S32: DW_LAUNCH(DFX_S32);
    case DFX_S8: DW_LAUNCH(DFX_S8);
    case DFX_U8: DW_LAUNCH(DFX_U8);
  }
#undef DW_LAUNCH
  return -1;
}

// window path: kh == kw in {3, 5}, sh == sw in {1, 2} (checked by the host); -1: no such instance
int launch_dwconv_window(const DwArgs &a, int grid, int block, int lds, hipStream_t s) {
  if (a.kh == 3 && a.sh == 1) return launch_window_ks<3, 1>(a, grid, block, lds, s);
  if (a.kh == 3 && a.sh == 2) return launch_window_ks<3, 2>(a, grid, block, lds, s);
  if (a.kh == 5 && a.sh == 1) return launch_window_ks<5, 1>(a, grid, block, lds, s);
  if (a.kh == 5 && a.sh == 2) return launch_window_ks<5, 2>(a, grid, block, lds, s);
  return -1;
}

int launch_dwconv_generic(const DwArgs &a, int grid, hipStream_t s) {
  dwconv_generic_kernel<<<grid, 256, 0, s>>>(a);
  return 0;
}

}  // namespace dfx
