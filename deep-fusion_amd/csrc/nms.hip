// nms.hip -- instances and the launchers of the box decode + greedy NMS kernels (nms.cuh).
#define DFX_NMS_KERNELS
#include "nms.cuh"

namespace dfx {

void launch_nms_generic(const NmsArgs &a, int grid, hipStream_t s) { nms_generic_kernel<<<grid, NMS_GENERIC_THREADS, 0, s>>>(a); }
void launch_nms_prep(const NmsArgs &a, int grid, hipStream_t s) { nms_prep_kernel<<<grid, NMS_PREP_THREADS, 0, s>>>(a); }
void launch_nms_mask(const NmsArgs &a, int grid, hipStream_t s) { nms_mask_kernel<<<grid, NMS_MASK_THREADS, 0, s>>>(a); }
void launch_nms_scan(const NmsArgs &a, int grid, hipStream_t s) { nms_scan_kernel<<<grid, NMS_SCAN_THREADS, 0, s>>>(a); }

}  // namespace dfx
