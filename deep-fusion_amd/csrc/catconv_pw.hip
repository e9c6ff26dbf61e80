// catconv_pw.hip -- instantiations of the concat + pointwise conv kernel (catconv_pw.cuh) and its launcher.
#include "catconv_pw.cuh"

namespace dfx {

// mode 0: launch; mode 1: raise the dynamic-LDS limit; mode 2: resident workgroups per CU
template <int OCB, int DST>
static int cat_one(const ConvArgs &a, const PwGeom &g, const CatTab &t, int grid, int lds, hipStream_t s, int mode) {
  auto k = catconv_pw_kernel<OCB, DST>;
  if (mode == 1)
    return (int)hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (mode == 2) {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k, PW_THREADS, lds) != hipSuccess) return -1;
    return n;
  }
  k<<<grid, PW_THREADS, lds, s>>>(a, g, t);
  return 0;
}

template <int DST>
static int cat_dst(const ConvArgs &a, const PwGeom &g, const CatTab &t, int grid, int lds, hipStream_t s, int mode) {
  switch (g.ocb) {
    case 2: return cat_one<2, DST>(a, g, t, grid, lds, s, mode);
    case 4: return cat_one<4, DST>(a, g, t, grid, lds, s, mode);
    case 8: return cat_one<8, DST>(a, g, t, grid, lds, s, mode);
  }
  return -1;
}

int launch_catconv_pw(const ConvArgs &a, const PwGeom &g, const CatTab &t, int dst_dt, int grid, int lds, hipStream_t s, int mode) {
  switch (dst_dt) {
    case DFX_F32: return cat_dst<DFX_F32>(a, g, t, grid, lds, s, mode);
    case DFX_S32: return cat_dst<DFX_S32>(a, g, t, grid, lds, s, mode);
    case DFX_S8: return cat_dst<DFX_S8>(a, g, t, grid, lds, s, mode);
    case DFX_U8: return cat_dst<DFX_U8>(a, g, t, grid, lds, s, mode);
  }
  return -1;
}

}  // namespace dfx
