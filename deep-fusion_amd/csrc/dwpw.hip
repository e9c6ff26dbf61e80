// dwpw.hip -- instantiations of the fused depthwise + pointwise conv kernel (dwpw.cuh) and its launcher.
#include "dwpw.cuh"

namespace dfx {

// mode 0: launch; mode 1: raise the dynamic-LDS limit; mode 2: resident workgroups per CU
template <int S, int OCB, int DST>
static int dwpw_one(const DwPwArgs &a, int grid, int lds, hipStream_t s, int mode) {
  auto k = dwpw_kernel<S, OCB, DST>;
  if (mode == 1)
    return (int)hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (mode == 2) {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k, DWPW_THREADS, lds) != hipSuccess) return -1;
    return n;
  }
  k<<<grid, DWPW_THREADS, lds, s>>>(a);
  return 0;
}

template <int S, int DST>
static int dwpw_ocb(const DwPwArgs &a, int grid, int lds, hipStream_t s, int mode) {
  switch (a.oc) {
    case 64: return dwpw_one<S, 2, DST>(a, grid, lds, s, mode);
    case 128: return dwpw_one<S, 4, DST>(a, grid, lds, s, mode);
    case 256: return dwpw_one<S, 8, DST>(a, grid, lds, s, mode);
  }
  return -1;
}

template <int S>
static int dwpw_dst(const DwPwArgs &a, int dst_dt, int grid, int lds, hipStream_t s, int mode) {
  switch (dst_dt) {
    case DFX_F32: return dwpw_ocb<S, DFX_F32>(a, grid, lds, s, mode);
    case DFX_S32: return dwpw_ocb<S, DFX_S32>(a, grid, lds, s, mode);
    case DFX_S8: return dwpw_ocb<S, DFX_S8>(a, grid, lds, s, mode);
    case DFX_U8: return dwpw_ocb<S, DFX_U8>(a, grid, lds, s, mode);
  }
  return -1;
}

// 3x3, stride (1,1) or (2,2) (checked by the host); -1: no such instance
int launch_dwpw(const DwPwArgs &a, int stride, int dst_dt, int grid, int lds, hipStream_t s, int mode) {
  if (stride == 1) return dwpw_dst<1>(a, dst_dt, grid, lds, s, mode);
  if (stride == 2) return dwpw_dst<2>(a, dst_dt, grid, lds, s, mode);
  return -1;
}

}  // namespace dfx
