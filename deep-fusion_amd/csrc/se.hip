// se.hip -- instances and launchers of the squeeze-and-excitation kernels (se.cuh).
#define DFX_SE_KERNELS
#include "se.cuh"

namespace dfx {

int launch_se_squeeze(const SeArgs &a, int grid, hipStream_t s) {
  se_squeeze_kernel<<<grid, SE_THREADS, 0, s>>>(a);
  return 0;
}

int launch_se_squeeze_generic(const SeArgs &a, int grid, hipStream_t s) {
  se_squeeze_generic<<<grid, 256, 0, s>>>(a);
  return 0;
}

int launch_se_excite(const SeArgs &a, int grid, int block, int lds, hipStream_t s) {
  se_excite_kernel<<<grid, block, lds, s>>>(a);
  return 0;
}

int launch_se_scale(const SeArgs &a, int grid, hipStream_t s) {
  if (a.rm == DFX_ROUND_DOWN) se_scale_kernel<1><<<grid, 256, 0, s>>>(a);
  else se_scale_kernel<0><<<grid, 256, 0, s>>>(a);
  return 0;
}

int launch_se_scale_generic(const SeArgs &a, int grid, hipStream_t s) {
  se_scale_generic<<<grid, 256, 0, s>>>(a);
  return 0;
}

// static LDS of the squeeze kernel (dfx_se_info.lds_bytes)
int se_squeeze_lds_bytes() { return (int)sizeof(int) * (SE_THREADS * SE_RED_PITCH + SE_THREADS); }

}  // namespace dfx
