// select.hip -- instances and the launchers of the image-wide top-K's kernels (select.cuh).
#define DFX_SELECT_KERNELS
#include "select.cuh"

namespace dfx {

void launch_select_generic(const SelectArgs &a, int grid, hipStream_t s) { select_generic_kernel<<<grid, SELECT_SORT_THREADS, 0, s>>>(a); }
void launch_select_hist(const SelectArgs &a, int grid, hipStream_t s) { select_hist_kernel<<<grid, SELECT_THREADS, 0, s>>>(a); }
void launch_select_scan(const SelectArgs &a, int grid, hipStream_t s) { select_scan_kernel<<<grid, SELECT_SORT_THREADS, 0, s>>>(a); }
void launch_select_compact(const SelectArgs &a, int grid, hipStream_t s) { select_compact_kernel<<<grid, SELECT_THREADS, 0, s>>>(a); }
void launch_select_sort(const SelectArgs &a, int grid, hipStream_t s) { select_sort_kernel<<<grid, SELECT_SORT_THREADS, 0, s>>>(a); }

}  // namespace dfx
