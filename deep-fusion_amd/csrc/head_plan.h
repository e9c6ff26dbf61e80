// head_plan.h -- host-only, plain C++: what the net head (dfx_head_* of include/dfx.h: channel top-k / argmax and softmax
// over a row matrix) decides before a kernel runs: the descriptor's validation, which kernel classes a descriptor is in,
// the auto rule, whether a softmax table is admitted and the grid (buffer extents and the overlap test: plan_common.h).
// No HIP in here, so that it can be built and run on its own (tools/head_plan_check.cc, under the host sanitizers).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/dfx.h"
#include "plan_common.h"

namespace dfx {

constexpr int HEAD_THREADS = 256;
constexpr int HEAD_ROWS_PER_BLOCK = 4;              // row path: a wave owns a row
constexpr int HEAD_MAX_BLOCKS = 256 * 8;            // grid-stride kernels: 8 workgroups per CU
constexpr long long HEAD_MAX_ELEMS = 1ll << 40;     // rows * the largest leading dimension, inclusive
constexpr int HEAD_PIXEL_MAX_LD = 160;              // pixel path: ten 16-byte groups per row (ADE20K's 150 classes)
constexpr int HEAD_TABLE_BYTES = 256 * 4;
constexpr int HEAD_ROW_AUTO_MIN_BYTES = 160;        // auto takes the row path from rows of this many bytes on

inline bool head_src_dt_ok(int dt) { return dt == DFX_F32 || dt == DFX_S32 || dt == DFX_S8 || dt == DFX_U8; }
inline bool head_path_ok(int p) { return p == DFX_HEAD_PIXEL || p == DFX_HEAD_ROW || p == DFX_HEAD_GENERIC; }

// elements between rows of the first output (idx or dst) and the elements of a row that are written
inline int head_out_ld(const dfx_head_desc &d) { return d.mode == DFX_HEAD_TOPK ? d.idx_ld : d.dst_ld; }
inline int head_out_cols(const dfx_head_desc &d) { return d.mode == DFX_HEAD_TOPK ? d.k : d.c; }

// DFX_OK, or the code dfx_head_create returns with *why set to the reason.  Everything DFX_ERR_INVALID is found before
// anything DFX_ERR_UNSUPPORTED (the class of a forced path is head_create's business: head_in_class below).
inline int head_validate(const dfx_head_desc &d, const char **why) {
  const char *dummy;
  if (!why) why = &dummy;
  *why = "";
  if (d.mode != DFX_HEAD_TOPK && d.mode != DFX_HEAD_SOFTMAX) return *why = "bad mode", DFX_ERR_INVALID;
  if (d.rows < 1) return *why = "rows must be at least 1", DFX_ERR_INVALID;
  if (d.c < 1 || d.c > DFX_HEAD_MAX_C) return *why = "c must lie in 1 .. 65535", DFX_ERR_INVALID;
  if (!head_src_dt_ok(d.src_dt)) return *why = "bad src dtype", DFX_ERR_INVALID;
  if (d.src_ld < d.c) return *why = "src_ld below c", DFX_ERR_INVALID;
  if (d.mode == DFX_HEAD_TOPK) {
    if (d.k < 1 || d.k > DFX_HEAD_MAX_K) return *why = "k must lie in 1 .. 8", DFX_ERR_INVALID;
    if (d.k > d.c) return *why = "k above c", DFX_ERR_INVALID;
    if (d.dst_dt != DFX_S32 && d.dst_dt != DFX_U8) return *why = "idx must be s32 or u8", DFX_ERR_INVALID;
    if (d.dst_dt == DFX_U8 && d.c > 256) return *why = "a u8 idx needs c <= 256", DFX_ERR_INVALID;
    if (d.idx_ld < d.k) return *why = "idx_ld below k", DFX_ERR_INVALID;
  } else {
    if (d.dst_dt != DFX_F32 && d.dst_dt != DFX_U8) return *why = "a softmax dst must be f32 or u8", DFX_ERR_INVALID;
    if (d.dst_ld < d.c) return *why = "dst_ld below c", DFX_ERR_INVALID;
    // (NaN fails both comparisons)
    if (d.dst_dt == DFX_U8 && !(d.out_scale >= -3.4028234e38f && d.out_scale <= 3.4028234e38f))
      return *why = "out_scale is not finite", DFX_ERR_INVALID;
  }
  if (d.force_path != -1 && !head_path_ok(d.force_path)) return *why = "bad force_path", DFX_ERR_INVALID;
  const long long ld = d.src_ld > head_out_ld(d) ? d.src_ld : head_out_ld(d);  // < 2^31: the quotient is exact
  if (d.rows > HEAD_MAX_ELEMS / ld) return *why = "more than 2^40 elements", DFX_ERR_INVALID;
  if (d.mode == DFX_HEAD_SOFTMAX && plan_dt_size(d.src_dt) != 1)
    return *why = "softmax of a 4-byte src (reorder it to u8 / s8 first)", DFX_ERR_UNSUPPORTED;
  return DFX_OK;
}

// the class of a path, as far as the descriptor decides it (pointer alignment is checked per submit)
inline bool head_pixel_class(const dfx_head_desc &d) {
  return plan_dt_size(d.src_dt) == 1 && (d.mode == DFX_HEAD_SOFTMAX || d.k == 1) && d.src_ld % 16 == 0 && d.src_ld <= HEAD_PIXEL_MAX_LD;
}
inline bool head_row_class(const dfx_head_desc &d) { return ((long long)d.src_ld * plan_dt_size(d.src_dt)) % 16 == 0; }
inline bool head_in_class(const dfx_head_desc &d, int path) {
  return path == DFX_HEAD_PIXEL ? head_pixel_class(d) : path == DFX_HEAD_ROW ? head_row_class(d) : path == DFX_HEAD_GENERIC;
}

// the handle's path.  AUTO RULE (include/dfx.h DFX_HEAD_AUTO_NOTE, measured in profiles/head/): the pixel kernel everywhere
// in its class, but for a softmax of 160-byte rows, where the row kernel was measured faster than both others; else the row
// kernel in its class where a row has at least 160 bytes (the shortest row at which it was measured and won; at 32 bytes a
// wave per row loses 7 to 39 times); the generic kernel everywhere else.
inline int head_path(const dfx_head_desc &d) {
  if (d.force_path != -1) return d.force_path;
  const bool long_row = head_row_class(d) && (long long)d.src_ld * plan_dt_size(d.src_dt) >= HEAD_ROW_AUTO_MIN_BYTES;
  if (d.mode == DFX_HEAD_SOFTMAX && long_row) return DFX_HEAD_ROW;
  if (head_pixel_class(d)) return DFX_HEAD_PIXEL;
  return long_row ? DFX_HEAD_ROW : DFX_HEAD_GENERIC;
}

// workgroups of 256 lanes for `rows` rows; cap <= 0: none (DFX_HEAD_GRID)
inline int head_grid(long long rows, int path, long long cap) {
  const int per = path == DFX_HEAD_ROW ? HEAD_ROWS_PER_BLOCK : HEAD_THREADS;
  long long blocks = (rows + per - 1) / per;
  if (blocks > HEAD_MAX_BLOCKS) blocks = HEAD_MAX_BLOCKS;
  if (cap > 0 && blocks > cap) blocks = cap;
  return (int)(blocks < 1 ? 1 : blocks);
}
inline int head_lds_bytes(const dfx_head_desc &d, int path) {
  return d.mode == DFX_HEAD_SOFTMAX && path != DFX_HEAD_GENERIC ? HEAD_TABLE_BYTES : 0;
}

// DFX_OK or DFX_ERR_INVALID: E[0] == 0 (S could be 0) or c * max(E) beyond u32 (S could leave u32)
inline int head_table_ok(const uint32_t *e, int c, const char **why) {
  const char *dummy;
  if (!why) why = &dummy;
  *why = "";
  if (e[0] == 0) return *why = "E[0] is 0: the sum could be 0", DFX_ERR_INVALID;
  uint32_t mx = 0;
  for (int i = 0; i < 256; ++i) mx = e[i] > mx ? e[i] : mx;
  if ((uint64_t)c * mx > 0xffffffffull) return *why = "c * max(E) beyond 2^32 - 1: the sum could leave u32", DFX_ERR_INVALID;
  return DFX_OK;
}

// what one submit must read and write (without val, which submit may or may not be given)
inline unsigned long long head_algorithmic_bytes(const dfx_head_desc &d) {
  const unsigned long long in = (unsigned long long)d.rows * d.c * plan_dt_size(d.src_dt);
  return in + (unsigned long long)d.rows * head_out_cols(d) * plan_dt_size(d.dst_dt);
}

}  // namespace dfx
