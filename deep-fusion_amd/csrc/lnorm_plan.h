// lnorm_plan.h -- host-only, plain C++: what the int8 layer norm / RMS norm (dfx_lnorm_* of include/dfx.h) decides before a
// kernel runs: the descriptor's validation, the bounds that make its integer statistics exact, the class of the row kernel,
// the lanes per row, the auto rule, the grid and the LDS plan (buffer extents and the overlap test: plan_common.h).
// No HIP in here, so that it can be built and run on its own (tools/lnorm_plan_check.cc, under the host sanitizers).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/dfx.h"
#include "plan_common.h"

namespace dfx {

constexpr int LNORM_THREADS = 256;
constexpr int LNORM_MAX_BLOCKS = 256 * 8;            // grid-stride kernels: 8 workgroups per CU
constexpr long long LNORM_MAX_ELEMS = 1ll << 40;     // rows * the larger leading dimension, inclusive
constexpr int LNORM_KEEP = 4;                        // row kernel: 16-byte groups a lane keeps in registers over both passes
constexpr int LNORM_MAX_LANES = 64;                  // row kernel: at most a wave per row
constexpr int LNORM_LDS_MAX = 64 * 1024;             // gamma / beta are staged in LDS where their image fits this

// ---- the bounds of include/dfx.h, section "Per row": what makes DFX_LNORM_MAX_C = 16384 the limit
constexpr long long LNORM_MAX_T = 255ll << DFX_LNORM_MAX_SHIFT;                    // |t_k|: u8 255 * 2^7 (s8: 128 * 2^7 is below it)
constexpr long long LNORM_MAX_S = LNORM_MAX_T * DFX_LNORM_MAX_C;                   // |S|
constexpr unsigned long long LNORM_MAX_Q = (unsigned long long)(LNORM_MAX_T * LNORM_MAX_T) * DFX_LNORM_MAX_C;
static_assert(LNORM_MAX_T == 32640, "|t_k| <= 32640");
static_assert(LNORM_MAX_T * LNORM_MAX_T < (1ll << 31), "t_k^2 fits s32");
static_assert(LNORM_MAX_S < (1ll << 30), "|S| < 2^30");
static_assert(LNORM_MAX_Q < (1ull << 44), "Q < 2^44");
static_assert(LNORM_MAX_Q < (1ull << 58) / DFX_LNORM_MAX_C, "c * Q (and D = c * Q - S^2 <= c * Q) < 2^58");
static_assert(LNORM_MAX_S * LNORM_MAX_S < (1ll << 60), "S^2 fits s64");
static_assert((long long)DFX_LNORM_MAX_C * LNORM_MAX_T + LNORM_MAX_S < (1ll << 31), "|u_k| = |c * t_k - S| < 2^31");
static_assert((long long)DFX_LNORM_MAX_C * DFX_LNORM_MAX_C < (1ll << 31), "c * c fits s32");
static_assert(DFX_LNORM_MAX_C < (1 << 24), "f32(c) is exact");
// without shifts a lane of the row kernel keeps its share of Q in u32: at most 16384 / (16 * 4) groups of 16 squares of 255
static_assert((unsigned long long)DFX_LNORM_MAX_C * 255 * 255 < (1ull << 32), "a row's unshifted Q fits u32");

inline bool lnorm_src_dt_ok(int dt) { return dt == DFX_S8 || dt == DFX_U8; }
inline bool lnorm_dst_dt_ok(int dt) { return dt == DFX_S8 || dt == DFX_U8 || dt == DFX_F32; }
inline bool lnorm_path_ok(int p) { return p == DFX_LNORM_ROW || p == DFX_LNORM_GENERIC; }

// DFX_OK, or the code dfx_lnorm_create returns with *why set to the reason.  Everything DFX_ERR_INVALID is found before
// anything DFX_ERR_UNSUPPORTED (the class of a forced path is lnorm_create's business: lnorm_in_class below).
inline int lnorm_validate(const dfx_lnorm_desc &d, const char **why) {
  const char *dummy;
  if (!why) why = &dummy;
  *why = "";
  if (d.mode != DFX_LNORM_LAYER && d.mode != DFX_LNORM_RMS) return *why = "bad mode", DFX_ERR_INVALID;
  if (d.rows < 1) return *why = "rows must be at least 1", DFX_ERR_INVALID;
  if (d.c < 1 || d.c > DFX_LNORM_MAX_C) return *why = "c must lie in 1 .. 16384", DFX_ERR_INVALID;
  if (!lnorm_src_dt_ok(d.src_dt)) return *why = "src dtype must be u8 or s8", DFX_ERR_INVALID;
  if (!lnorm_dst_dt_ok(d.dst_dt)) return *why = "dst dtype must be u8, s8 or f32", DFX_ERR_INVALID;
  if (d.src_ld < d.c) return *why = "src_ld below c", DFX_ERR_INVALID;
  if (d.dst_ld < d.c) return *why = "dst_ld below c", DFX_ERR_INVALID;
  // (NaN fails both comparisons)
  if (!(d.eps > 0.0f && d.eps <= 3.4028234e38f)) return *why = "eps must be finite and above 0", DFX_ERR_INVALID;
  if (d.force_path != -1 && !lnorm_path_ok(d.force_path)) return *why = "bad force_path", DFX_ERR_INVALID;
  const long long ld = d.src_ld > d.dst_ld ? d.src_ld : d.dst_ld;  // < 2^31: the quotient is exact
  if (d.rows > LNORM_MAX_ELEMS / ld) return *why = "more than 2^40 elements", DFX_ERR_INVALID;
  return DFX_OK;
}

// the class of a path, as far as the descriptor decides it (pointer alignment is checked per submit)
inline bool lnorm_row_class(const dfx_lnorm_desc &d) {
  return d.src_ld % 16 == 0 && ((long long)d.dst_ld * plan_dt_size(d.dst_dt)) % 16 == 0;
}
inline bool lnorm_in_class(const dfx_lnorm_desc &d, int path) {
  return path == DFX_LNORM_ROW ? lnorm_row_class(d) : path == DFX_LNORM_GENERIC;
}

// row kernel: consecutive lanes that own a row: the smallest of 4, 8, 16, 32, 64 that is at least ceil(c / 16), capped at 64
inline int lnorm_lanes(int c) {
  const int groups = (c + 15) / 16;
  int w = 4;
  while (w < groups && w < LNORM_MAX_LANES) w *= 2;
  return w;
}

// the handle's path.  AUTO RULE (include/dfx.h DFX_LNORM_AUTO_NOTE): the row kernel is unmeasured, so nothing takes it on
// auto; it runs where force_path asks for it.
inline bool lnorm_row_auto(const dfx_lnorm_desc &d) {
  (void)d;
  return false;
}
inline int lnorm_path(const dfx_lnorm_desc &d) {
  if (d.force_path != -1) return d.force_path;
  return lnorm_row_class(d) && lnorm_row_auto(d) ? DFX_LNORM_ROW : DFX_LNORM_GENERIC;
}

// workgroups of 256 lanes for `rows` rows; cap <= 0: none (DFX_LNORM_GRID)
inline int lnorm_grid(long long rows, int c, int path, long long cap) {
  const int per = path == DFX_LNORM_ROW ? LNORM_THREADS / lnorm_lanes(c) : LNORM_THREADS;
  long long blocks = (rows + per - 1) / per;
  if (blocks > LNORM_MAX_BLOCKS) blocks = LNORM_MAX_BLOCKS;
  if (cap > 0 && blocks > cap) blocks = cap;
  return (int)(blocks < 1 ? 1 : blocks);
}
// row kernel: gamma and beta of whole 16-channel groups (the pad reads as 0), staged once per workgroup; 0: read from global
inline int lnorm_lds_bytes(const dfx_lnorm_desc &d, int path) {
  const int bytes = 8 * plan_up16(d.c);
  return path == DFX_LNORM_ROW && bytes <= LNORM_LDS_MAX ? bytes : 0;
}
// the device image of the parameters: gamma[up16(c)] f32, beta[up16(c)] f32, shift[up16(c)] u8; pads are 0
inline size_t lnorm_param_bytes(int c) { return (size_t)9 * plan_up16(c); }

// what one submit must read and write
inline unsigned long long lnorm_algorithmic_bytes(const dfx_lnorm_desc &d, bool has_shift) {
  const unsigned long long io = (unsigned long long)d.rows * d.c * (1 + plan_dt_size(d.dst_dt));
  return io + (unsigned long long)d.c * (has_shift ? 9 : 8);
}

}  // namespace dfx
