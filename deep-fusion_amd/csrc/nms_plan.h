// nms_plan.h -- plain C++, no HIP: what the box decode + greedy NMS (dfx_nms_* of include/dfx.h) decides before a kernel
// runs -- the descriptor's validation, the handle's path, the enumeration of the upper triangle of 64 x 64 tiles, the layout
// of the handle's scratch, LDS sizes, buffer extents for the overlap check -- and the scan's step over one 64-row block.
// That step is ONE definition: nms.cuh compiles the same function for the device (NMS_HD), and tools/nms_plan_check.cc runs
// it on the host against a brute-force greedy walk, under the host sanitizers.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/dfx.h"
#include "plan_common.h"

#if defined(__HIPCC__)
#define NMS_HD __host__ __device__ inline
#else
#define NMS_HD inline
#endif

namespace dfx {

constexpr int NMS_TILE = 64;                // boxes per tile side: one u64 of the mask per row box and tile
constexpr int NMS_GENERIC_THREADS = 1024;   // the generic kernel: one workgroup per image
constexpr int NMS_PREP_THREADS = 256;       // launch A: a lane per position
constexpr int NMS_MASK_THREADS = 256;       // launch B: four waves, a tile each
constexpr int NMS_SCAN_THREADS = 64;        // launch C: one wave per image
constexpr int NMS_SCAN_BATCH = 16;          // launch C: rows of the mask whose loads are in flight together
constexpr int NMS_MAX_BLOCKS = DFX_NMS_MAX_N / NMS_TILE;  // 64: the removed bitmap is one u64 per lane of a wave
constexpr long long NMS_MAX_GRID = 1 << 20;
constexpr long long NMS_MAX_ENTRY = 2147483647ll;         // n_anchors * classes

// (v == v && |v| <= FLT_MAX) without <cmath>
inline bool nms_finite(float v) { return v == v && v <= 3.402823466e+38f && v >= -3.402823466e+38f; }

// DFX_OK, or the code dfx_nms_create returns with *why set
inline int nms_validate(const dfx_nms_desc &d, const char **why) {
  const char *dummy;
  if (!why) why = &dummy;
  *why = "";
  if (d.bs < 1) return *why = "bs must be at least 1", DFX_ERR_INVALID;
  if (d.n < 1 || d.n > DFX_NMS_MAX_N) return *why = "n must lie in 1 .. 4096", DFX_ERR_INVALID;
  if (d.max_out < 1 || d.max_out > d.n) return *why = "max_out must lie in 1 .. n", DFX_ERR_INVALID;
  if (d.keep_ld < d.max_out) return *why = "keep_ld below max_out", DFX_ERR_INVALID;
  if (d.mode != DFX_NMS_BOXES && d.mode != DFX_NMS_DECODE) return *why = "bad mode", DFX_ERR_INVALID;
  if (d.per_class != 0 && d.per_class != 1) return *why = "per_class must be 0 or 1", DFX_ERR_INVALID;
  if (d.force_path != -1 && d.force_path != DFX_NMS_MASK && d.force_path != DFX_NMS_GENERIC) return *why = "bad force_path", DFX_ERR_INVALID;
  if (d.classes < 1 || d.anchors_per_pixel < 1 || d.n_anchors < 1) return *why = "classes, anchors_per_pixel and n_anchors must be at least 1", DFX_ERR_INVALID;
  if (d.n_anchors > NMS_MAX_ENTRY / d.classes) return *why = "n_anchors * classes beyond 2^31 - 1", DFX_ERR_INVALID;
  if (!nms_finite(d.iou_thr)) return *why = "iou_thr must be finite", DFX_ERR_INVALID;
  const bool reads_idx = d.mode == DFX_NMS_DECODE || d.per_class;
  if (reads_idx && d.idx_ld < d.n) return *why = "idx_ld below n", DFX_ERR_INVALID;
  if (d.mode == DFX_NMS_DECODE) {
    if (d.anchors_per_pixel > 16384 || d.row_bytes < 4 * d.anchors_per_pixel) return *why = "row_bytes below 4 * anchors_per_pixel", DFX_ERR_INVALID;
    if (d.clip_w != d.clip_w || d.clip_h != d.clip_h) return *why = "clip_w or clip_h is NaN", DFX_ERR_INVALID;
    if (d.clip_w > 0 && !(d.clip_h >= 0)) return *why = "clip_w > 0 needs clip_h >= 0", DFX_ERR_INVALID;
  }
  return DFX_OK;
}

inline bool nms_reads_idx(const dfx_nms_desc &d) { return d.mode == DFX_NMS_DECODE || d.per_class != 0; }
inline int nms_blocks(int n) { return (n + NMS_TILE - 1) / NMS_TILE; }          // n64
inline int nms_tiles(int n) { const int b = nms_blocks(n); return b * (b + 1) / 2; }

// the handle's path.  AUTO RULE (include/dfx.h DFX_NMS_AUTO_NOTE, measured in profiles/nms/): the mask path from n = 200 and
// max_out = 100 on, the smallest of each at which it was measured and won; the generic kernel below (n 1000 with max_out 20 is
// 1.6 times faster on its one launch, n 100 is a tie).
constexpr int NMS_MASK_AUTO_MIN_N = 200, NMS_MASK_AUTO_MIN_OUT = 100;  // the smallest n and max_out measured
inline int nms_path(const dfx_nms_desc &d) {
  if (d.force_path != -1) return d.force_path;
  return d.n >= NMS_MASK_AUTO_MIN_N && d.max_out >= NMS_MASK_AUTO_MIN_OUT ? DFX_NMS_MASK : DFX_NMS_GENERIC;
}

// The upper triangle of an n64 x n64 grid of tiles, row block by row block: entry t = rb | cb << 8 with cb >= rb.  Returns
// the number of entries, nms_tiles(n); `out` has room for that many.
inline int nms_enumerate_tiles(int n, uint16_t *out) {
  const int b = nms_blocks(n);
  int t = 0;
  for (int rb = 0; rb < b; ++rb)
    for (int cb = rb; cb < b; ++cb) out[t++] = (uint16_t)(rb | cb << 8);
  return t;
}

inline int nms_image_grid(int bs) { return (int)(bs < NMS_MAX_GRID ? bs : NMS_MAX_GRID); }
inline int nms_prep_grid(int bs, int n) {
  const long long g = ((long long)bs * nms_blocks(n) * NMS_TILE + NMS_PREP_THREADS - 1) / NMS_PREP_THREADS;
  return (int)(g < NMS_MAX_GRID ? g : NMS_MAX_GRID);
}
inline long long nms_mask_items(int bs, int n) { return (long long)bs * nms_tiles(n); }
inline int nms_mask_grid(int bs, int n) {
  const long long g = (nms_mask_items(bs, n) + NMS_MASK_THREADS / 64 - 1) / (NMS_MASK_THREADS / 64);
  return (int)(g < NMS_MAX_GRID ? g : NMS_MAX_GRID);
}

// scratch of a mask-path handle, in bytes from its start: box [bs][n64 * 64] float4 | lab [bs][n64 * 64] s32 |
// mask [bs][n64 * 64][n64] u64 | tile table [tiles] u16
struct NmsScratch {
  size_t off_lab, off_mask, off_tiles, bytes;
};
inline size_t nms_round16(size_t v) { return (v + 15) & ~(size_t)15; }
inline NmsScratch nms_scratch(int bs, int n) {
  const size_t b = (size_t)nms_blocks(n), rows = (size_t)bs * b * NMS_TILE;
  NmsScratch s;
  s.off_lab = rows * 16;
  s.off_mask = s.off_lab + nms_round16(rows * 4);
  s.off_tiles = s.off_mask + rows * b * 8;
  s.bytes = s.off_tiles + nms_round16((size_t)nms_tiles(n) * 2);
  return s;
}

// static LDS of the kernels (nms.cuh)
inline int nms_lds_generic() { return DFX_NMS_MAX_N * 16 + DFX_NMS_MAX_N * 4 + DFX_NMS_MAX_N; }
inline int nms_lds_mask() { return (NMS_MASK_THREADS / 64) * NMS_TILE * (16 + 4); }
inline int nms_lds_bytes(int path) { return path == DFX_NMS_MASK ? nms_lds_mask() : nms_lds_generic(); }
inline int nms_launches(int path) { return path == DFX_NMS_MASK ? 3 : 1; }

// bytes from a buffer's first to behind its last touched byte
inline unsigned long long nms_boxes_extent(const dfx_nms_desc &d) { return (unsigned long long)d.bs * d.n * 16; }
inline unsigned long long nms_idx_extent(const dfx_nms_desc &d) { return ((unsigned long long)(d.bs - 1) * (unsigned)d.idx_ld + (unsigned)d.n) * 4; }
inline unsigned long long nms_deltas_extent(const dfx_nms_desc &d) {
  return ((unsigned long long)d.bs * d.n - 1) * (unsigned)d.row_bytes + 4ull * (unsigned)d.anchors_per_pixel;
}
inline unsigned long long nms_anchors_extent(const dfx_nms_desc &d) { return (unsigned long long)d.n_anchors * 16; }
inline unsigned long long nms_keep_extent(const dfx_nms_desc &d) { return ((unsigned long long)(d.bs - 1) * (unsigned)d.keep_ld + (unsigned)d.max_out) * 4; }
inline unsigned long long nms_boxes_out_extent(const dfx_nms_desc &d) { return (unsigned long long)d.bs * d.max_out * 16; }

// what one submit must read and write (without boxes_out, which a submit may leave out)
inline unsigned long long nms_algorithmic_bytes(const dfx_nms_desc &d) {
  const unsigned long long e = (unsigned long long)d.bs * d.n;
  unsigned long long b = d.mode == DFX_NMS_DECODE ? e * (4 + 4 + 16) : e * 16 + (d.per_class ? e * 4 : 0);
  return b + (unsigned long long)d.bs * d.max_out * 4 + (unsigned long long)d.bs * 4;
}

// ---- the scan's step over one 64-row block -------------------------------------------------------------------------------
// diag[t]: the word of row t of the block's diagonal tile (bit c: "t suppresses c", c > t only).  cand: the rows of the
// block that are valid and not removed by a kept row of an earlier block.  budget >= 1: how many may still be kept.  Returns
// the rows kept, lowest first, at most `budget` of them: row t is kept iff it is in cand and no kept row below it has its bit.
NMS_HD uint64_t nms_block_scan(const uint64_t *diag, uint64_t cand, int budget) {
  uint64_t live = cand, kept = 0;
  int taken = 0;
  while (live != 0 && taken < budget) {
    const int t = __builtin_ctzll(live);
    kept |= (uint64_t)1 << t;
    ++taken;
    live &= ~diag[t];
    live &= ~((uint64_t)1 << t);
  }
  return kept;
}

}  // namespace dfx
