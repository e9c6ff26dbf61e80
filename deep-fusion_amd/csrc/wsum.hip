// wsum.hip -- instances and launchers of the scaled element-wise sum's kernels (wsum.cuh).
#define DFX_WSUM_KERNELS
#include "wsum.cuh"

namespace dfx {

int launch_wsum_generic(const WsumArgs &a, int grid, hipStream_t s) {
  wsum_generic_kernel<<<grid, 256, 0, s>>>(a);
  return 0;
}

namespace {
template <int OUT, int RM>
void launch_vec(const WsumArgs &a, int grid, hipStream_t s) {
  if (a.relu) wsum_vec_kernel<OUT, true, RM><<<grid, 256, a.image_bytes, s>>>(a);
  else wsum_vec_kernel<OUT, false, RM><<<grid, 256, a.image_bytes, s>>>(a);
}
template <int OUT>
void launch_vec_rm(const WsumArgs &a, int grid, hipStream_t s) {
  if (a.rm == DFX_ROUND_DOWN) launch_vec<OUT, 1>(a, grid, s);
  else launch_vec<OUT, 0>(a, grid, s);
}
}  // namespace

int launch_wsum_vec(const WsumArgs &a, int grid, hipStream_t s) {
  if (a.lut_in_dt != DFX_UNDEF) launch_vec_rm<WSUM_OUT_LUT>(a, grid, s);
  else if (a.dst_dt == DFX_F32) launch_vec<WSUM_OUT_F32, 0>(a, grid, s);  // (no rounding: one instance for both modes)
  else if (a.dst_dt == DFX_U8) launch_vec_rm<WSUM_OUT_U8>(a, grid, s);
  else if (a.dst_dt == DFX_S8) launch_vec_rm<WSUM_OUT_S8>(a, grid, s);
  else return -1;
  return 0;
}

}  // namespace dfx
