// resize.hip -- instances and launchers of the activation resize kernels (resize.cuh).
#include "resize.cuh"

namespace dfx {

template <typename T>
static void launch_generic_t(const ResizeArgs &a, int grid, hipStream_t s) {
  resize_generic_kernel<T><<<grid, 256, 0, s>>>(a);
}

int launch_resize_generic(const ResizeArgs &a, int grid, hipStream_t s) {
  switch (a.dt) {
    case DFX_F32: launch_generic_t<float>(a, grid, s); break;
    case DFX_S32: if (a.algo != DFX_RESIZE_NEAREST) return -1; launch_generic_t<int>(a, grid, s); break;
    case DFX_S8: launch_generic_t<signed char>(a, grid, s); break;
    case DFX_U8: launch_generic_t<unsigned char>(a, grid, s); break;
    default: return -1;
  }
  return 0;
}

template <typename T, int ALGO>
static void launch_band_t(const ResizeArgs &a, int grid, hipStream_t s) {
  if (a.add) resize_band_kernel<T, ALGO, true><<<grid, 256, 0, s>>>(a);
  else resize_band_kernel<T, ALGO, false><<<grid, 256, 0, s>>>(a);
}

int launch_resize_band(const ResizeArgs &a, int grid, hipStream_t s) {
  if (a.algo == DFX_RESIZE_NEAREST) {
    switch (a.dt) {
      case DFX_F32: launch_band_t<float, DFX_RESIZE_NEAREST>(a, grid, s); break;
      case DFX_S32: launch_band_t<int, DFX_RESIZE_NEAREST>(a, grid, s); break;
      case DFX_S8: launch_band_t<signed char, DFX_RESIZE_NEAREST>(a, grid, s); break;
      case DFX_U8: launch_band_t<unsigned char, DFX_RESIZE_NEAREST>(a, grid, s); break;
      default: return -1;
    }
  } else {
    switch (a.dt) {
      case DFX_F32: launch_band_t<float, DFX_RESIZE_BILINEAR>(a, grid, s); break;
      case DFX_S8: launch_band_t<signed char, DFX_RESIZE_BILINEAR>(a, grid, s); break;
      case DFX_U8: launch_band_t<unsigned char, DFX_RESIZE_BILINEAR>(a, grid, s); break;
      default: return -1;
    }
  }
  return 0;
}

}  // namespace dfx
