// roialign.hip -- instances and the launchers of the RoIAlign kernels (roialign.cuh).
#define DFX_ROIALIGN_KERNELS
#include "roialign.cuh"

namespace dfx {

void launch_roialign_generic(const RoiArgs &a, int dt, int grid, hipStream_t s) {
  if (dt == DFX_U8) roialign_generic_kernel<unsigned char><<<grid, ROI_THREADS, 0, s>>>(a);
  else if (dt == DFX_S8) roialign_generic_kernel<signed char><<<grid, ROI_THREADS, 0, s>>>(a);
  else roialign_generic_kernel<float><<<grid, ROI_THREADS, 0, s>>>(a);
}

template <typename T>
static void launch_tile(const RoiArgs &a, unsigned grid, hipStream_t s) {
  switch (a.S) {
    case 1: roialign_tile_kernel<T, 1><<<grid, ROI_THREADS, 0, s>>>(a); break;
    case 2: roialign_tile_kernel<T, 2><<<grid, ROI_THREADS, 0, s>>>(a); break;
    case 3: roialign_tile_kernel<T, 3><<<grid, ROI_THREADS, 0, s>>>(a); break;
    default: roialign_tile_kernel<T, 4><<<grid, ROI_THREADS, 0, s>>>(a); break;
  }
}

void launch_roialign_tile(const RoiArgs &a, int dt, unsigned grid, hipStream_t s) {
  if (dt == DFX_U8) launch_tile<unsigned char>(a, grid, s);
  else if (dt == DFX_S8) launch_tile<signed char>(a, grid, s);
  else launch_tile<float>(a, grid, s);
}

}  // namespace dfx
