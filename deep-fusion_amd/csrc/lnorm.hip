// lnorm.hip -- instances and the launcher of the layer norm's kernels (lnorm.cuh).
#define DFX_LNORM_KERNELS
#include "lnorm.cuh"

namespace dfx {

namespace {
template <int W>
void launch_row(const LnormArgs &a, int grid, int lds, hipStream_t s) {
  if (a.shift) lnorm_row_kernel<W, true><<<grid, 256, lds, s>>>(a);
  else lnorm_row_kernel<W, false><<<grid, 256, lds, s>>>(a);
}
}  // namespace

// path: DFX_LNORM_ROW | DFX_LNORM_GENERIC; lanes: lnorm_lanes(c); lds: dynamic LDS of the row kernel.  -1: no such instance.
int launch_lnorm(const LnormArgs &a, int path, int lanes, int grid, int lds, hipStream_t s) {
  if (path == DFX_LNORM_GENERIC) {
    lnorm_generic_kernel<<<grid, 256, 0, s>>>(a);
    return 0;
  }
  if (path != DFX_LNORM_ROW) return -1;
  switch (lanes) {
    case 4: launch_row<4>(a, grid, lds, s); break;
    case 8: launch_row<8>(a, grid, lds, s); break;
    case 16: launch_row<16>(a, grid, lds, s); break;
    case 32: launch_row<32>(a, grid, lds, s); break;
    case 64: launch_row<64>(a, grid, lds, s); break;
    default: return -1;
  }
  return 0;
}

}  // namespace dfx
