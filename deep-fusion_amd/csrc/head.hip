// head.hip -- instances and the launcher of the net head's kernels (head.cuh).
#define DFX_HEAD_KERNELS
#include "head.cuh"

namespace dfx {

// path: DFX_HEAD_PIXEL | DFX_HEAD_ROW | DFX_HEAD_GENERIC; softmax: the mode.  -1: no such instance.
int launch_head(const HeadArgs &a, int path, bool softmax, int grid, hipStream_t s) {
  if (softmax) {
    if (path == DFX_HEAD_PIXEL) head_pixel_softmax_kernel<<<grid, 256, 0, s>>>(a);
    else if (path == DFX_HEAD_ROW) head_row_softmax_kernel<<<grid, 256, 0, s>>>(a);
    else if (path == DFX_HEAD_GENERIC) head_generic_softmax_kernel<<<grid, 256, 0, s>>>(a);
    else return -1;
    return 0;
  }
  if (a.k < 1 || a.k > DFX_HEAD_MAX_K) return -1;
  if (path == DFX_HEAD_PIXEL) {
    if (a.k != 1) return -1;
    head_pixel_topk_kernel<<<grid, 256, 0, s>>>(a);
  } else if (path == DFX_HEAD_ROW) {
    if (a.k == 1) head_row_topk_kernel<1><<<grid, 256, 0, s>>>(a);
    else head_row_topk_kernel<8><<<grid, 256, 0, s>>>(a);
  } else if (path == DFX_HEAD_GENERIC) {
    if (a.k == 1) head_generic_topk_kernel<1><<<grid, 256, 0, s>>>(a);
    else head_generic_topk_kernel<8><<<grid, 256, 0, s>>>(a);
  } else {
    return -1;
  }
  return 0;
}

}  // namespace dfx
