// plan_common.h -- the arithmetic every device-free *_plan.h repeats: element sizes, rounding up to 16, the extent of a row
// matrix in bytes and the overlap of two byte ranges.  No HIP and nothing beyond C++11, so that the plan headers and the
// stand-alone tools/*_plan_check.cc programs can include it.  What an op knows about its own tensors (window_src_extent,
// pe_dst_extent, nms_*_extent, select_*_extent, roi_*_extent) stays in the op's plan header and is built on these.
#pragma once

#include <stdint.h>

#include "../../include/dfx.h"

namespace dfx {

inline int plan_dt_size(int dt) { return (dt == DFX_F32 || dt == DFX_S32) ? 4 : 1; }

inline long long plan_up16(long long v) { return (v + 15) / 16 * 16; }

// bytes from a buffer's first to behind its last touched byte: rows `ld` elements apart, `cols` touched per row
inline unsigned long long plan_extent(long long rows, long long ld, long long cols, long long esize) {
  return ((unsigned long long)(rows - 1) * (unsigned long long)ld + (unsigned long long)cols) * (unsigned long long)esize;
}

inline bool plan_overlap(uintptr_t a, unsigned long long abytes, uintptr_t b, unsigned long long bbytes) {
  return a < b + bbytes && b < a + abytes;
}

}  // namespace dfx
