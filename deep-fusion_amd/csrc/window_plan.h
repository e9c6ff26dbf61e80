// window_plan.h -- host-only, plain C++: what the window partition / reverse op (dfx_window_* of include/dfx.h) decides before
// a kernel runs: the descriptor's validation, the padded geometry, THE ROW MAP (the one place where shift, padding, order and
// direction exist), the class of the row kernel, the auto rule, the grids, the extent of both buffers (for the overlap check)
// and the byte count.  No HIP in here, so that it can be built and run on its own (tools/window_plan_check.cc, under the host
// sanitizers).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/dfx.h"
#include "plan_common.h"

namespace dfx {

constexpr int WINDOW_THREADS = 256;
constexpr int WINDOW_MAX_BLOCKS = 256 * 8;           // grid-stride kernels: 8 workgroups per CU (LNORM_MAX_BLOCKS' precedent)
constexpr int WINDOW_UNROLL = 4;                     // row kernel: 16-byte groups a lane moves per trip, all loaded before the first store
constexpr long long WINDOW_MAX_ELEMS = 1ll << 40;    // window-side rows * the larger leading dimension, inclusive

inline bool window_dt_ok(int dt) { return dt == DFX_U8 || dt == DFX_S8 || dt == DFX_S32 || dt == DFX_F32; }
inline bool window_path_ok(int p) { return p == DFX_WINDOW_ROW || p == DFX_WINDOW_GENERIC; }

// the padded map (valid once h, w, wh, ww have passed window_validate)
inline int window_hp(const dfx_window_desc &d) { return (d.h + d.wh - 1) / d.wh * d.wh; }
inline int window_wp(const dfx_window_desc &d) { return (d.w + d.ww - 1) / d.ww * d.ww; }
inline int window_nwx(const dfx_window_desc &d) { return window_wp(d) / d.ww; }
inline int window_count(const dfx_window_desc &d) { return (window_hp(d) / d.wh) * window_nwx(d); }    // nW
inline long long window_win_rows(const dfx_window_desc &d) { return (long long)window_hp(d) * window_wp(d); }  // per image
inline long long window_grid_rows(const dfx_window_desc &d) { return (long long)d.h * d.w; }               // per image

// DFX_OK, or the code dfx_window_create returns with *why set to the reason.  Everything DFX_ERR_INVALID is found before
// anything DFX_ERR_UNSUPPORTED (the class of a forced path is window_create's business: window_in_class below).
inline int window_validate(const dfx_window_desc &d, const char **why) {
  const char *dummy;
  if (!why) why = &dummy;
  *why = "";
  if (d.dir != DFX_WINDOW_PARTITION && d.dir != DFX_WINDOW_REVERSE) return *why = "bad dir", DFX_ERR_INVALID;
  if (!window_dt_ok(d.dt)) return *why = "dtype must be u8, s8, s32 or f32", DFX_ERR_INVALID;
  if (d.bs < 1) return *why = "bs must be at least 1", DFX_ERR_INVALID;
  if (d.h < 1 || d.h > DFX_WINDOW_MAX_HW || d.w < 1 || d.w > DFX_WINDOW_MAX_HW) return *why = "h and w must lie in 1 .. 65535", DFX_ERR_INVALID;
  if (d.c < 1) return *why = "c must be at least 1", DFX_ERR_INVALID;
  if (d.wh < 1 || d.wh > DFX_WINDOW_MAX_WIN || d.ww < 1 || d.ww > DFX_WINDOW_MAX_WIN) return *why = "wh and ww must lie in 1 .. 255", DFX_ERR_INVALID;
  if (d.order != DFX_WINDOW_ROW_MAJOR && d.order != DFX_WINDOW_COL_MAJOR) return *why = "bad order", DFX_ERR_INVALID;
  const int hp = window_hp(d), wp = window_wp(d);  // < 65535 + 255
  if (d.shift_y < 0 || d.shift_y >= hp) return *why = "shift_y must lie in 0 .. hp-1", DFX_ERR_INVALID;
  if (d.shift_x < 0 || d.shift_x >= wp) return *why = "shift_x must lie in 0 .. wp-1", DFX_ERR_INVALID;
  if (d.grid_ld < d.c) return *why = "grid_ld below c", DFX_ERR_INVALID;
  if (d.win_ld < d.c) return *why = "win_ld below c", DFX_ERR_INVALID;
  if (d.force_path != -1 && !window_path_ok(d.force_path)) return *why = "bad force_path", DFX_ERR_INVALID;
  if ((long long)hp * wp > DFX_WINDOW_MAX_PADDED) return *why = "padded map hp * wp above 2^22", DFX_ERR_INVALID;
  const long long ld = d.grid_ld > d.win_ld ? d.grid_ld : d.win_ld;   // >= 1
  const long long rows = (long long)d.bs * hp * wp;                   // < 2^31 * 2^22
  if (rows > WINDOW_MAX_ELEMS / ld) return *why = "more than 2^40 elements", DFX_ERR_INVALID;
  return DFX_OK;
}

// ---- the two sides as the op's source and destination
inline bool window_src_is_grid(const dfx_window_desc &d) { return d.dir == DFX_WINDOW_PARTITION; }
inline long long window_src_rows(const dfx_window_desc &d) { return window_src_is_grid(d) ? window_grid_rows(d) : window_win_rows(d); }
inline long long window_dst_rows(const dfx_window_desc &d) { return window_src_is_grid(d) ? window_win_rows(d) : window_grid_rows(d); }
inline long long window_src_ld(const dfx_window_desc &d) { return window_src_is_grid(d) ? d.grid_ld : d.win_ld; }
inline long long window_dst_ld(const dfx_window_desc &d) { return window_src_is_grid(d) ? d.win_ld : d.grid_ld; }

// window-side row (within one image) of the token at padded coordinates (Y, X)
inline int window_row_of(const dfx_window_desc &d, int Y, int X) {
  const int wy = Y / d.wh, iy = Y % d.wh, wx = X / d.ww, ix = X % d.ww;
  const int in = d.order == DFX_WINDOW_COL_MAJOR ? ix * d.wh + iy : iy * d.ww + ix;
  return (wy * window_nwx(d) + wx) * (d.wh * d.ww) + in;
}

// THE MAP: one entry per row of the DESTINATION within one image, the source row within one image it is copied from.
//   PARTITION  hp * wp entries: window-side row -> grid row, or -1 for a pad token
//   REVERSE    h * w entries:   grid row -> window-side row
// Built by walking the window side in its own order, from the definition in include/dfx.h.
inline void window_build_map(const dfx_window_desc &d, std::vector<int32_t> &map) {
  const int hp = window_hp(d), wp = window_wp(d);
  map.assign((size_t)window_dst_rows(d), -1);
  for (int Y = 0; Y < hp; ++Y) {
    const int y = (Y + d.shift_y) % hp;
    for (int X = 0; X < wp; ++X) {
      const int x = (X + d.shift_x) % wp;
      const int wr = window_row_of(d, Y, X);
      const bool pad = y >= d.h || x >= d.w;
      if (d.dir == DFX_WINDOW_PARTITION) map[(size_t)wr] = pad ? -1 : y * d.w + x;
      else if (!pad) map[(size_t)y * d.w + x] = wr;
    }
  }
}
inline long long window_pad_tokens(const dfx_window_desc &d) { return (long long)d.bs * (window_win_rows(d) - window_grid_rows(d)); }

// the class of a path, as far as the descriptor decides it (pointer alignment is checked per submit)
inline bool window_row_class(const dfx_window_desc &d) {
  const long long es = plan_dt_size(d.dt);
  return ((long long)d.c * es) % 16 == 0 && (d.grid_ld * es) % 16 == 0 && (d.win_ld * es) % 16 == 0;
}
inline bool window_in_class(const dfx_window_desc &d, int path) {
  return path == DFX_WINDOW_ROW ? window_row_class(d) : path == DFX_WINDOW_GENERIC;
}
// row kernel: consecutive lanes that move one token
inline long long window_lanes(const dfx_window_desc &d) { return (long long)d.c * plan_dt_size(d.dt) / 16; }

// the handle's path.  AUTO RULE (include/dfx.h DFX_WINDOW_AUTO_NOTE): the row kernel is unmeasured, so nothing takes it on
// auto; it runs where force_path asks for it.
inline bool window_row_auto(const dfx_window_desc &d) {
  (void)d;
  return false;
}
inline int window_path(const dfx_window_desc &d) {
  if (d.force_path != -1) return d.force_path;
  return window_row_class(d) && window_row_auto(d) ? DFX_WINDOW_ROW : DFX_WINDOW_GENERIC;
}

// workgroups of 256 lanes: the row kernel moves 256 * WINDOW_UNROLL 16-byte groups per workgroup trip, the generic kernel
// 256 elements; cap <= 0: none (DFX_WINDOW_GRID)
inline int window_grid(const dfx_window_desc &d, int path, long long cap) {
  const long long rows = (long long)d.bs * window_dst_rows(d);
  const long long work = path == DFX_WINDOW_ROW ? rows * window_lanes(d) : rows * d.c;   // <= 2^40
  const long long per = path == DFX_WINDOW_ROW ? WINDOW_THREADS * WINDOW_UNROLL : WINDOW_THREADS;
  long long blocks = (work + per - 1) / per;
  if (blocks > WINDOW_MAX_BLOCKS) blocks = WINDOW_MAX_BLOCKS;
  if (cap > 0 && blocks > cap) blocks = cap;
  return (int)(blocks < 1 ? 1 : blocks);
}

inline unsigned long long window_src_extent(const dfx_window_desc &d) {
  return plan_extent((long long)d.bs * window_src_rows(d), window_src_ld(d), d.c, plan_dt_size(d.dt));
}
inline unsigned long long window_dst_extent(const dfx_window_desc &d) {
  return plan_extent((long long)d.bs * window_dst_rows(d), window_dst_ld(d), d.c, plan_dt_size(d.dt));
}

// what one submit must read and write: the valid bytes of the tokens read (pad tokens are not), of the tokens written, the map
inline unsigned long long window_algorithmic_bytes(const dfx_window_desc &d) {
  const unsigned long long token = (unsigned long long)d.c * plan_dt_size(d.dt);
  const unsigned long long grid = (unsigned long long)d.bs * window_grid_rows(d), win = (unsigned long long)d.bs * window_win_rows(d);
  return (grid + (d.dir == DFX_WINDOW_PARTITION ? win : grid)) * token + 4ull * (unsigned long long)window_dst_rows(d);
}

}  // namespace dfx
