// roialign_plan.h -- plain C++, no HIP: what RoIAlign (dfx_roialign_* of include/dfx.h) decides before a kernel runs -- the
// descriptor's validation and size limits, the tile kernel's class, the split of a RoI's bin rows over workgroups, grids, LDS
// bytes, buffer extents for the overlap check, algorithmic bytes.  tools/roialign_plan_check.cc walks it over a grid of
// descriptors on the host, under the host sanitizers.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/dfx.h"
#include "plan_common.h"

namespace dfx {

constexpr int ROI_THREADS = 256;                   // both kernels
constexpr int ROI_TABLE = DFX_ROIALIGN_MAX_BINS * DFX_ROIALIGN_MAX_SAMPLING;  // 256 entries per axis table
constexpr int ROI_ENTRY_BYTES = 20;                // low / high byte offset, two weights, valid
constexpr long long ROI_MAX_GENERIC_GRID = 1 << 20;
// The kernels address dst and every level with 32-bit byte offsets: a tensor of this many bytes or more is refused.
constexpr unsigned long long ROI_MAX_BYTES = 1ull << 32;
// workgroups the tile plan wants in flight before it stops splitting RoIs: two per CU of an MI355X
constexpr int ROI_SPLIT_TARGET = 512;

// (v == v && |v| <= FLT_MAX) without <cmath>
inline bool roi_finite(float v) { return v == v && v <= 3.402823466e+38f && v >= -3.402823466e+38f; }
inline int roi_esize(int dt) { return dt == DFX_F32 ? 4 : 1; }
inline unsigned long long roi_rows(const dfx_roialign_desc &d) {
  return d.mode == DFX_ROI_BATCHED ? (unsigned long long)d.bs * (unsigned)d.n : (unsigned long long)d.n;
}

// bytes from a buffer's first to behind its last touched byte
inline unsigned long long roi_level_extent(const dfx_roialign_desc &d, int l) {
  const unsigned long long px = (unsigned long long)d.bs * (unsigned)d.h[l] * (unsigned)d.w[l];
  return ((px - 1) * (unsigned)d.src_ld[l] + (unsigned)d.c) * roi_esize(d.dt);
}
inline unsigned long long roi_dst_extent(const dfx_roialign_desc &d) {
  const unsigned long long px = roi_rows(d) * (unsigned)d.ph * (unsigned)d.pw;
  return ((px - 1) * (unsigned)d.dst_ld + (unsigned)d.c) * roi_esize(d.dt);
}
inline unsigned long long roi_boxes_extent(const dfx_roialign_desc &d) { return roi_rows(d) * 16; }

// the tile kernel's class (the pointers' alignment is checked per submit)
inline bool roi_tile_class(const dfx_roialign_desc &d) {
  const int es = roi_esize(d.dt);
  if (d.c % (16 / es)) return false;
  if ((long long)d.dst_ld * es % 16) return false;
  for (int l = 0; l < d.levels; ++l)
    if ((long long)d.src_ld[l] * es % 16) return false;
  return true;
}

// DFX_OK, or the code dfx_roialign_create returns with *why set
inline int roi_validate(const dfx_roialign_desc &d, const char **why) {
  const char *dummy;
  if (!why) why = &dummy;
  *why = "";
  if (d.bs < 1 || d.n < 1) return *why = "bs and n must be at least 1", DFX_ERR_INVALID;
  if (d.mode != DFX_ROI_BATCHED && d.mode != DFX_ROI_LIST) return *why = "bad mode", DFX_ERR_INVALID;
  if (d.levels < 1 || d.levels > DFX_ROIALIGN_MAX_LEVELS) return *why = "levels must lie in 1 .. 4", DFX_ERR_INVALID;
  if (d.c < 1) return *why = "c must be at least 1", DFX_ERR_INVALID;
  if (d.dt != DFX_U8 && d.dt != DFX_S8 && d.dt != DFX_F32) return *why = "dt must be u8, s8 or f32", DFX_ERR_INVALID;
  if (d.dst_ld < d.c) return *why = "dst_ld below c", DFX_ERR_INVALID;
  for (int l = 0; l < d.levels; ++l) {
    if (d.h[l] < 1 || d.h[l] > 65535 || d.w[l] < 1 || d.w[l] > 65535) return *why = "h and w must lie in 1 .. 65535", DFX_ERR_INVALID;
    if (d.src_ld[l] < d.c) return *why = "src_ld below c", DFX_ERR_INVALID;
    if (!roi_finite(d.spatial_scale[l]) || !(d.spatial_scale[l] > 0.0f)) return *why = "spatial_scale must be finite and > 0", DFX_ERR_INVALID;
  }
  for (int i = 0; i + 1 < d.levels; ++i) {
    if (!roi_finite(d.level_area_thr[i])) return *why = "level_area_thr must be finite", DFX_ERR_INVALID;
    if (i && d.level_area_thr[i] < d.level_area_thr[i - 1]) return *why = "level_area_thr must not decrease", DFX_ERR_INVALID;
  }
  if (d.ph < 1 || d.ph > DFX_ROIALIGN_MAX_BINS || d.pw < 1 || d.pw > DFX_ROIALIGN_MAX_BINS) return *why = "ph and pw must lie in 1 .. 64", DFX_ERR_INVALID;
  if (d.sampling_ratio < 0 || d.sampling_ratio > DFX_ROIALIGN_MAX_SAMPLING) return *why = "sampling_ratio must lie in 1 .. 4", DFX_ERR_INVALID;
  if (d.aligned != 0 && d.aligned != 1) return *why = "aligned must be 0 or 1", DFX_ERR_INVALID;
  if (d.force_path != -1 && d.force_path != DFX_ROIALIGN_TILE && d.force_path != DFX_ROIALIGN_GENERIC) return *why = "bad force_path", DFX_ERR_INVALID;
  if (d.force_path == DFX_ROIALIGN_TILE && !roi_tile_class(d)) return *why = "force_path TILE outside the tile kernel's class", DFX_ERR_INVALID;
  if (d.sampling_ratio == 0) return *why = "adaptive sampling (sampling_ratio 0) is not built", DFX_ERR_UNSUPPORTED;
  // (every factor is below 2^31 and the products are formed in u64 step by step: (2^31)^2 * 2^12 * 2^31 would overflow, so
  //  the row count is bounded first)
  if (roi_rows(d) >= ROI_MAX_BYTES) return *why = "dst of 2^32 bytes or more", DFX_ERR_UNSUPPORTED;
  const unsigned long long dpx = roi_rows(d) * (unsigned)d.ph * (unsigned)d.pw;  // < 2^32 * 2^12
  if (dpx >= ROI_MAX_BYTES || dpx * (unsigned)d.dst_ld >= ROI_MAX_BYTES || dpx * (unsigned)d.dst_ld * roi_esize(d.dt) >= ROI_MAX_BYTES)
    return *why = "dst of 2^32 bytes or more", DFX_ERR_UNSUPPORTED;
  for (int l = 0; l < d.levels; ++l) {
    const unsigned long long px = (unsigned long long)d.bs * (unsigned)d.h[l] * (unsigned)d.w[l];  // < 2^31 * 2^32: no overflow
    if (px >= ROI_MAX_BYTES || px * (unsigned)d.src_ld[l] >= ROI_MAX_BYTES || px * (unsigned)d.src_ld[l] * roi_esize(d.dt) >= ROI_MAX_BYTES)
      return *why = "a level of 2^32 bytes or more", DFX_ERR_UNSUPPORTED;
  }
  return DFX_OK;
}

// the handle's path.  AUTO RULE (include/dfx.h DFX_ROIALIGN_AUTO_NOTE, measured in profiles/roialign/): the tile kernel in
// its class from the smallest sizes at which it was measured and won -- 256 bytes of channels per pixel, 100 RoIs, 7 x 7
// bins; the generic kernel below any of them (unmeasured) and outside the class.
constexpr int ROI_TILE_AUTO_MIN_PIXEL_BYTES = 256, ROI_TILE_AUTO_MIN_ROIS = 100, ROI_TILE_AUTO_MIN_BINS = 49;
inline int roi_path(const dfx_roialign_desc &d) {
  if (d.force_path != -1) return d.force_path;
  const bool measured = (long long)d.c * roi_esize(d.dt) >= ROI_TILE_AUTO_MIN_PIXEL_BYTES && roi_rows(d) >= (unsigned)ROI_TILE_AUTO_MIN_ROIS &&
                        d.ph * d.pw >= ROI_TILE_AUTO_MIN_BINS;
  return roi_tile_class(d) && measured ? DFX_ROIALIGN_TILE : DFX_ROIALIGN_GENERIC;
}

// tile path: bin rows a workgroup owns.  A whole RoI where R alone fills the device, else the RoI's bin rows are split
// until about ROI_SPLIT_TARGET workgroups exist (never below one row).
inline int roi_rows_per_group(const dfx_roialign_desc &d) {
  const unsigned long long R = roi_rows(d);
  if (R >= (unsigned)ROI_SPLIT_TARGET) return d.ph;
  int splits = (int)((ROI_SPLIT_TARGET + R - 1) / R);
  if (splits > d.ph) splits = d.ph;
  return (d.ph + splits - 1) / splits;
}
inline int roi_splits(const dfx_roialign_desc &d) {
  const int rows = roi_rows_per_group(d);
  return (d.ph + rows - 1) / rows;
}
// workgroup g of the tile grid owns RoI g / splits, bin rows [(g % splits) * rows, min(ph, that + rows))
inline unsigned roi_tile_grid(const dfx_roialign_desc &d) { return (unsigned)(roi_rows(d) * roi_splits(d)); }  // < 2^32 / 16
inline unsigned long long roi_elements(const dfx_roialign_desc &d) { return roi_rows(d) * (unsigned)d.ph * (unsigned)d.pw * (unsigned)d.c; }
inline int roi_generic_grid(const dfx_roialign_desc &d) {
  const unsigned long long g = (roi_elements(d) + ROI_THREADS - 1) / ROI_THREADS;
  return (int)(g < (unsigned long long)ROI_MAX_GENERIC_GRID ? g : ROI_MAX_GENERIC_GRID);
}
inline int roi_grid(const dfx_roialign_desc &d, int path) { return path == DFX_ROIALIGN_TILE ? (int)roi_tile_grid(d) : roi_generic_grid(d); }
// table entries a tile workgroup writes: its rows' y samples and the whole x axis
inline int roi_table_entries_y(const dfx_roialign_desc &d) { return roi_rows_per_group(d) * d.sampling_ratio; }
inline int roi_table_entries_x(const dfx_roialign_desc &d) { return d.pw * d.sampling_ratio; }
inline int roi_lds_bytes(int path) { return path == DFX_ROIALIGN_TILE ? 2 * ROI_TABLE * ROI_ENTRY_BYTES : 0; }

// what one submit must read and write: boxes and count / batch_idx, four corner pixels per sample, dst
inline unsigned long long roi_algorithmic_bytes(const dfx_roialign_desc &d) {
  const unsigned long long R = roi_rows(d), bins = R * (unsigned)d.ph * (unsigned)d.pw, cb = (unsigned long long)d.c * roi_esize(d.dt);
  return R * 16 + (d.mode == DFX_ROI_BATCHED ? (unsigned long long)d.bs * 4 : R * 4) +
         bins * (unsigned)(d.sampling_ratio * d.sampling_ratio) * 4 * cb + bins * cb;
}

}  // namespace dfx
