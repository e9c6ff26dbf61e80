// select_plan.h -- plain C++, no HIP: what the image-wide top-K (dfx_select_* of include/dfx.h) decides before a kernel
// runs -- the descriptor's validation, the class of the histogram path, the cut of an image into chunks, the layout of
// the handle's scratch, LDS sizes, buffer extents for the overlap check -- and the threshold / quota scan over a
// histogram slab.  The scan is ONE definition: select.cuh compiles the same functions for the device (SELECT_HD), and
// tools/select_plan_check.cc runs them on the host against a brute-force sort, under the host sanitizers.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/dfx.h"
#include "plan_common.h"

#if defined(__HIPCC__)
#define SELECT_HD __host__ __device__ inline
#else
#define SELECT_HD inline
#endif

namespace dfx {

constexpr int SELECT_THREADS = 256;           // histogram and compaction kernels
constexpr int SELECT_SORT_THREADS = 1024;     // scan, sort and the generic kernel: one workgroup per image
constexpr int SELECT_BINS = 256;
constexpr int SELECT_MAX_CHUNKS = 1024;       // chunks of one image (the scan keeps two counters per chunk in LDS)
constexpr int SELECT_MIN_CHUNK_BYTES = 16384; // default plan: a workgroup reads at least this much of src
constexpr int SELECT_WGS_PER_CU = 4;          // default plan: workgroups of launch A per CU
constexpr long long SELECT_MAX_GRID = 1 << 20;           // workgroups of one launch; further items by grid stride
constexpr long long SELECT_MAX_IMAGE = 2147483647ll;     // h * w * c
constexpr long long SELECT_MAX_ELEMS = 1ll << 40;        // bs * h * w * src_ld
constexpr int SELECT_MAX_PIXEL_STRIDE = 65536;
constexpr int SELECT_HIST_AUTO_MIN_BYTES = 4096;  // auto takes the histogram path from images of this many bytes on
constexpr int SELECT_HDR_WORDS = 4;           // plan per image: t, count, n_gt, quota
constexpr int SELECT_CHUNK_WORDS = 3;         // plan per chunk: off_gt, quota_eq, off_eq

inline bool select_src_dt_1byte(int dt) { return dt == DFX_U8 || dt == DFX_S8; }
inline int select_dt_min(int dt) { return dt == DFX_S8 ? -128 : 0; }
inline int select_dt_max(int dt) { return dt == DFX_S8 ? 127 : 255; }
// the element as an unsigned key that orders like the value (head.cuh's head_key8)
SELECT_HD unsigned select_key8(unsigned byte, int dt) { return dt == DFX_U8 ? (byte & 0xffu) : ((byte ^ 0x80u) & 0xffu); }

// DFX_OK, or the code dfx_select_create returns with *why set.  Everything DFX_ERR_INVALID is found before anything
// DFX_ERR_UNSUPPORTED.
inline int select_validate(const dfx_select_desc &d, const char **why) {
  const char *dummy;
  if (!why) why = &dummy;
  *why = "";
  if (d.bs < 1 || d.h < 1 || d.w < 1) return *why = "bs, h and w must be at least 1", DFX_ERR_INVALID;
  if (d.c < 1 || d.c > 65535) return *why = "c must lie in 1 .. 65535", DFX_ERR_INVALID;
  if (d.src_ld < d.c || d.src_ld > 65535) return *why = "src_ld must lie in c .. 65535", DFX_ERR_INVALID;
  if (d.src_dt != DFX_U8 && d.src_dt != DFX_S8 && d.src_dt != DFX_S32 && d.src_dt != DFX_F32) return *why = "bad src dtype", DFX_ERR_INVALID;
  if (d.k < 1 || d.k > DFX_SELECT_MAX_K) return *why = "k must lie in 1 .. 4096", DFX_ERR_INVALID;
  if (d.idx_ld < d.k) return *why = "idx_ld below k", DFX_ERR_INVALID;
  if (d.peak != DFX_SELECT_ALL && d.peak != DFX_SELECT_PEAK3) return *why = "bad peak mode", DFX_ERR_INVALID;
  if (d.force_path != -1 && d.force_path != DFX_SELECT_HIST && d.force_path != DFX_SELECT_GENERIC) return *why = "bad force_path", DFX_ERR_INVALID;
  // h * w <= 2^62, then * c and * src_ld only once the quotient shows that the product fits
  const long long px = (long long)d.h * d.w;
  if (px > SELECT_MAX_IMAGE / d.c) return *why = "h * w * c beyond 2^31 - 1", DFX_ERR_INVALID;
  if (d.bs > SELECT_MAX_ELEMS / (px * d.src_ld)) return *why = "bs * h * w * src_ld beyond 2^40", DFX_ERR_INVALID;
  if (d.n_gather < 0 || d.n_gather > DFX_SELECT_MAX_GATHER) return *why = "n_gather must lie in 0 .. 4", DFX_ERR_INVALID;
  for (int i = 0; i < d.n_gather; ++i) {
    if (d.row_bytes[i] < 1 || d.row_bytes[i] > DFX_SELECT_MAX_ROW_BYTES) return *why = "row_bytes must lie in 1 .. 1024", DFX_ERR_INVALID;
    if (d.pixel_stride_bytes[i] < d.row_bytes[i] || d.pixel_stride_bytes[i] > SELECT_MAX_PIXEL_STRIDE)
      return *why = "pixel_stride_bytes must lie in row_bytes .. 65536", DFX_ERR_INVALID;
  }
  if (select_src_dt_1byte(d.src_dt) && (d.min_val < select_dt_min(d.src_dt) || d.min_val > select_dt_max(d.src_dt)))
    return *why = "min_val outside src's dtype", DFX_ERR_INVALID;
  if (!select_src_dt_1byte(d.src_dt)) return *why = "s32 / f32 scores are not built (they need a multi-pass radix)", DFX_ERR_UNSUPPORTED;
  return DFX_OK;
}

// the class of the histogram path, as far as the descriptor decides it (pointer alignment is checked per submit)
inline bool select_hist_class(const dfx_select_desc &d) { return d.src_ld % 16 == 0; }

// the handle's path.  AUTO RULE (include/dfx.h DFX_SELECT_AUTO_NOTE, measured in profiles/select/): the histogram path in
// its class from images of 4096 bytes (h * w * src_ld) on, the smallest at which it was measured and won; the generic
// kernel below that (a 1008-byte row is 1.5 to 1.7 times faster on its one launch) and outside the class.
inline int select_path(const dfx_select_desc &d) {
  if (d.force_path != -1) return d.force_path;
  return select_hist_class(d) && (long long)d.h * d.w * d.src_ld >= SELECT_HIST_AUTO_MIN_BYTES ? DFX_SELECT_HIST : DFX_SELECT_GENERIC;
}

// The cut of an image of `px` pixels into chunks of consecutive pixels.  forced_px > 0 (DFX_SELECT_CHUNK) asks for that
// many pixels per chunk; the default gives the device SELECT_WGS_PER_CU workgroups per CU over the batch, each with at
// least SELECT_MIN_CHUNK_BYTES of src.  Either is raised until an image has at most SELECT_MAX_CHUNKS chunks.
struct SelectPlan {
  int chunk_px, chunks;
  long long items;  // bs * chunks: workgroups' worth of work in launches A and C
  int grid;
};
inline SelectPlan select_plan(int bs, long long px, int src_ld, int cus, long long forced_px) {
  long long cpx;
  if (forced_px > 0) {
    cpx = forced_px;
  } else {
    long long per_image = ((long long)cus * SELECT_WGS_PER_CU + bs - 1) / bs;
    if (per_image < 1) per_image = 1;
    cpx = (px + per_image - 1) / per_image;
    const long long min_px = (SELECT_MIN_CHUNK_BYTES + src_ld - 1) / src_ld;
    if (cpx < min_px) cpx = min_px;
  }
  const long long floor_px = (px + SELECT_MAX_CHUNKS - 1) / SELECT_MAX_CHUNKS;
  if (cpx < floor_px) cpx = floor_px;
  if (cpx > px) cpx = px;
  SelectPlan p;
  p.chunk_px = (int)cpx;
  p.chunks = (int)((px + cpx - 1) / cpx);
  p.items = (long long)bs * p.chunks;
  p.grid = (int)(p.items < SELECT_MAX_GRID ? p.items : SELECT_MAX_GRID);
  return p;
}
inline int select_image_grid(int bs) { return (int)(bs < SELECT_MAX_GRID ? bs : SELECT_MAX_GRID); }

// scratch of a histogram-path handle, in bytes from its start: slab [bs][chunks][256] u32 | plan [bs][4 + 3 * chunks] u32
// | cand [bs][k] u64
struct SelectScratch {
  size_t off_plan, off_cand, bytes;
};
inline size_t select_round16(size_t v) { return (v + 15) & ~(size_t)15; }
inline SelectScratch select_scratch(int bs, int chunks, int k) {
  SelectScratch s;
  s.off_plan = select_round16((size_t)bs * chunks * SELECT_BINS * 4);
  s.off_cand = s.off_plan + select_round16((size_t)bs * (SELECT_HDR_WORDS + SELECT_CHUNK_WORDS * (size_t)chunks) * 4);
  s.bytes = s.off_cand + select_round16((size_t)bs * k * 8);
  return s;
}

// elements the sort works on: the power of two at or above k, at least 64
inline int select_sort_size(int k) {
  int p = 64;
  while (p < k) p *= 2;
  return p;
}
// static LDS of the kernels (select.cuh): the sort's pairs, a histogram, the scan's wave totals and a few counters
inline int select_lds_hist() { return (SELECT_THREADS / 64) * SELECT_BINS * 4; }
inline int select_lds_compact() { return 16 * 4 + 4; }
inline int select_lds_scan() { return SELECT_SORT_THREADS * 4 + SELECT_BINS * 4 + (2 + SELECT_CHUNK_WORDS) * SELECT_MAX_CHUNKS * 4 + 16; }
inline int select_lds_sort() { return DFX_SELECT_MAX_K * 8; }
inline int select_lds_generic() { return DFX_SELECT_MAX_K * 8 + SELECT_BINS * 4 + 16 * 4 + 8 + 16; }
inline int select_lds_bytes(int path) { return path == DFX_SELECT_HIST ? select_lds_sort() : select_lds_generic(); }
inline int select_launches(int path) { return path == DFX_SELECT_HIST ? 4 : 1; }

// bytes from a buffer's first to behind its last touched byte
inline unsigned long long select_src_extent(const dfx_select_desc &d) {
  return ((unsigned long long)d.bs * d.h * d.w - 1) * (unsigned)d.src_ld + (unsigned)d.c;
}
inline unsigned long long select_idx_extent(const dfx_select_desc &d, int esize) {
  return ((unsigned long long)(d.bs - 1) * (unsigned)d.idx_ld + (unsigned)d.k) * (unsigned)esize;
}
inline unsigned long long select_gather_src_extent(const dfx_select_desc &d, int i) {
  return ((unsigned long long)d.bs * d.h * d.w - 1) * (unsigned)d.pixel_stride_bytes[i] + (unsigned)d.row_bytes[i];
}
inline unsigned long long select_gather_dst_extent(const dfx_select_desc &d, int i) {
  return (unsigned long long)d.bs * d.k * (unsigned)d.row_bytes[i];
}

// what one submit must read and write: the valid src elements, idx, count, and with_val / the gather rows
inline unsigned long long select_algorithmic_bytes(const dfx_select_desc &d) {
  unsigned long long n = (unsigned long long)d.bs * d.h * d.w * d.c + (unsigned long long)d.bs * d.k * 4 + (unsigned long long)d.bs * 4;
  for (int i = 0; i < d.n_gather; ++i) n += 2ull * d.bs * d.k * d.row_bytes[i];
  return n;
}

// ---- the scan ----------------------------------------------------------------------------------------------------------
// From the 256 totals of an image's candidates per key: the threshold key t -- the largest with #(key >= t) >= k, or the
// lowest candidate key when there are fewer than k candidates (0 when there are none) --, the number of candidates above
// it, how many of the key t itself are taken, and count = min(k, candidates).
struct SelectThreshold {
  int t;
  unsigned n_gt, quota, count;
};
SELECT_HD SelectThreshold select_threshold(const unsigned *total, int k) {
  SelectThreshold r;
  unsigned acc = 0;
  int lowest = 0;
  for (int b = SELECT_BINS - 1; b >= 0; --b) {
    if (total[b] == 0) continue;
    if (acc + total[b] >= (unsigned)k) {
      r.t = b; r.n_gt = acc; r.quota = (unsigned)k - acc; r.count = (unsigned)k;
      return r;
    }
    acc += total[b];
    lowest = b;
  }
  // fewer than k candidates: all of them
  r.t = lowest;
  r.quota = total[lowest];
  r.n_gt = acc - r.quota;
  r.count = acc;
  return r;
}
// Per chunk, in index order, from its number of candidates above t (gt[c]) and at t (eq[c]): where its keys above t go in
// the image's candidate list, how many of its keys at t it may keep (the lowest chunks are served first, so the lowest
// element indices win the tie bin) and where those go.  plan: SELECT_CHUNK_WORDS words per chunk.
SELECT_HD void select_chunk_offsets(const unsigned *gt, const unsigned *eq, int chunks, unsigned n_gt, unsigned quota, unsigned *plan) {
  unsigned off_gt = 0, off_eq = n_gt, left = quota;
  for (int c = 0; c < chunks; ++c) {
    const unsigned take = eq[c] < left ? eq[c] : left;
    plan[SELECT_CHUNK_WORDS * c + 0] = off_gt;
    plan[SELECT_CHUNK_WORDS * c + 1] = take;
    plan[SELECT_CHUNK_WORDS * c + 2] = off_eq;
    off_gt += gt[c];
    off_eq += take;
    left -= take;
  }
}

}  // namespace dfx
