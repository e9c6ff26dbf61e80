// window.hip -- instances and the launcher of the window partition / reverse kernels (window.cuh).
#define DFX_WINDOW_KERNELS
#include "window.cuh"

namespace dfx {

// path: DFX_WINDOW_ROW | DFX_WINDOW_GENERIC.  -1: no such instance.
int launch_window(const WindowArgs &a, int path, int grid, hipStream_t s) {
  if (path == DFX_WINDOW_GENERIC) window_generic_kernel<<<grid, WINDOW_THREADS, 0, s>>>(a);
  else if (path == DFX_WINDOW_ROW) window_row_kernel<<<grid, WINDOW_THREADS, 0, s>>>(a);
  else return -1;
  return 0;
}

}  // namespace dfx
