// linear_plan.h -- host-only, plain C++: what the int8 token linear op (dfx_linear_* of include/dfx.h) decides before a
// kernel runs: the descriptor's validation in the order the header documents, the tile kernel's class, the auto rule, the
// tile height BM, the tile count and the grids, the LDS size, the sections of the device image and the algorithmic counts.
// No HIP in here, so that it can be built and run on its own (tools/linear_plan_check.cc, under the host sanitizers).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/dfx.h"
#include "plan_common.h"

namespace dfx {

constexpr int LIN_THREADS = 256;                  // four waves own a BM x LIN_BN tile of dst
constexpr int LIN_BN = 128;                       // dst columns per tile = rows of a weight block
constexpr int LIN_KS = 64;                        // k per slab
constexpr int LIN_BM_MAX = 128, LIN_BM_MIN = 64;  // the two tile heights
constexpr int LIN_KMAX = 65025;
constexpr int LIN_NMAX = 2147483647 - (LIN_BN - 1);  // n rounded up to LIN_BN fits an int
constexpr long long LIN_MAX_ELEMS = 1ll << 40;    // rows * max(src_ld, dst_ld)
constexpr int LIN_WBLOCK = LIN_BN * LIN_KS;       // bytes of one (n-block, slab) of the weight image: what LDS holds of it
constexpr int LIN_TILE_GRID_PER_CU = 2;           // workgroups per CU at most; the rest is the kernel's loop over tiles
constexpr int LIN_GEN_GRID_PER_CU = 16;

inline bool lin_dt_ok(int dt) { return dt == DFX_F32 || dt == DFX_S32 || dt == DFX_S8 || dt == DFX_U8; }
inline bool lin_has_table(const dfx_linear_desc &d) { return d.lut_in_dt != DFX_UNDEF; }
// the type the requant produces: dst's, or the table's index type
inline int lin_requant_dt(const dfx_linear_desc &d) { return lin_has_table(d) ? d.lut_in_dt : d.dst_dt; }
inline bool lin_relu(const dfx_linear_desc &d) { return d.relu != 0 || lin_requant_dt(d) == DFX_U8; }

// the class of the tile kernel as far as the descriptor decides it (the alignment of src and dst is checked per submit)
inline bool lin_tile_class(const dfx_linear_desc &d) { return d.src_ld % 16 == 0; }

// DFX_OK, or the code dfx_linear_create returns with *why set to the reason.  Everything DFX_ERR_INVALID is found before
// anything DFX_ERR_UNSUPPORTED.
inline int lin_validate(const dfx_linear_desc &d, const char **why) {
  const char *dummy;
  if (!why) why = &dummy;
  *why = "";
  if (d.rows < 1) return *why = "rows below 1", DFX_ERR_INVALID;
  if (d.k < 1 || d.k > LIN_KMAX) return *why = "k must lie in 1 .. 65025 (the accumulator could leave s32)", DFX_ERR_INVALID;
  if (d.n < 1 || d.n > LIN_NMAX) return *why = "n must lie in 1 .. 2^31 - 128", DFX_ERR_INVALID;
  if (d.src_dt != DFX_U8 && d.src_dt != DFX_S8) return *why = "bad src dtype (u8 or s8)", DFX_ERR_INVALID;
  if (!lin_dt_ok(d.dst_dt)) return *why = "bad dst dtype", DFX_ERR_INVALID;
  if (d.bia_dt != DFX_UNDEF && !lin_dt_ok(d.bia_dt)) return *why = "bad bias dtype", DFX_ERR_INVALID;
  if (d.round_mode != DFX_ROUND_NEAREST && d.round_mode != DFX_ROUND_DOWN) return *why = "bad round mode", DFX_ERR_INVALID;
  if (d.nscales != 1 && d.nscales != d.n) return *why = "scales count must be 1 or n", DFX_ERR_INVALID;
  if (d.lut_in_dt != DFX_UNDEF && d.lut_in_dt != DFX_U8 && d.lut_in_dt != DFX_S8) return *why = "bad lut_in_dt (none, u8 or s8)", DFX_ERR_INVALID;
  if (lin_has_table(d) && d.dst_dt != DFX_U8 && d.dst_dt != DFX_S8) return *why = "a table needs a 1-byte dst", DFX_ERR_INVALID;
  if (d.force_path != -1 && d.force_path != DFX_LINEAR_TILE && d.force_path != DFX_LINEAR_GENERIC) return *why = "bad force_path", DFX_ERR_INVALID;
  if (d.src_ld < d.k) return *why = "src_ld below k", DFX_ERR_INVALID;
  if (d.dst_ld < d.n) return *why = "dst_ld below n", DFX_ERR_INVALID;
  const long long ld = d.src_ld > d.dst_ld ? d.src_ld : d.dst_ld;
  if ((unsigned __int128)d.rows * (unsigned __int128)ld > (unsigned __int128)LIN_MAX_ELEMS)
    return *why = "rows * max(src_ld, dst_ld) beyond 2^40", DFX_ERR_INVALID;
  if (d.force_path == DFX_LINEAR_TILE && !lin_tile_class(d))
    return *why = "descriptor outside the tile kernel's class (src_ld a multiple of 16)", DFX_ERR_UNSUPPORTED;
  return DFX_OK;
}

// AUTO RULE (include/dfx.h DFX_LINEAR_AUTO_NOTE, DESIGN.md section 4.24, measured in profiles/linear/): the tile kernel in its
// class from the smallest of each size at which tools/bench_linear timed it and it beat both the generic kernel and dfx_bmm's
// MFMA kernel on the same operands: rows >= 1576 (ViT-B bs 8), n >= 96 and k >= 96 (the Swin stage-1 block), at least 54 tiles
// of 64 x 128 and 1700 * 256 * 256 multiply-adds (both the DETR 256 -> 256 point).  It won at all 14 measured points; nothing
// smaller was timed, so everything smaller stays generic and reaches the tile kernel with force_path.
constexpr long long LIN_AUTO_MIN_ROWS = 1576, LIN_AUTO_MIN_TILES64 = 54, LIN_AUTO_MIN_MACS = 1700ll * 256 * 256;
constexpr int LIN_AUTO_MIN_N = 96, LIN_AUTO_MIN_K = 96;
inline bool lin_tile_auto(const dfx_linear_desc &d) {
  if (d.rows < LIN_AUTO_MIN_ROWS || d.n < LIN_AUTO_MIN_N || d.k < LIN_AUTO_MIN_K) return false;
  if (((d.rows + LIN_BM_MIN - 1) / LIN_BM_MIN) * (((long long)d.n + LIN_BN - 1) / LIN_BN) < LIN_AUTO_MIN_TILES64) return false;
  return (unsigned __int128)d.rows * (unsigned __int128)((long long)d.n * d.k) >= (unsigned __int128)LIN_AUTO_MIN_MACS;
}
inline int lin_path(const dfx_linear_desc &d) {
  if (d.force_path != -1) return d.force_path;
  return lin_tile_class(d) && lin_tile_auto(d) ? DFX_LINEAR_TILE : DFX_LINEAR_GENERIC;
}

inline int lin_nblocks(int n) { return (int)(((long long)n + LIN_BN - 1) / LIN_BN); }
inline int lin_nslabs(int k) { return (k + LIN_KS - 1) / LIN_KS; }
inline long long lin_mtiles(long long rows, int bm) { return (rows + bm - 1) / bm; }
inline long long lin_tiles(const dfx_linear_desc &d, int bm) { return lin_mtiles(d.rows, bm) * lin_nblocks(d.n); }

// the tile height: 128 rows, or 64 where 128 would leave fewer tiles than CUs.  forced: 64 | 128 (DFX_LINEAR_BM), else 0
inline int lin_bm(const dfx_linear_desc &d, int cus, int forced) {
  if (forced == LIN_BM_MIN || forced == LIN_BM_MAX) return forced;
  return lin_tiles(d, LIN_BM_MAX) >= (long long)(cus < 1 ? 1 : cus) ? LIN_BM_MAX : LIN_BM_MIN;
}

inline long long lin_items(const dfx_linear_desc &d) { return d.rows * (long long)d.n; }

// workgroups of 256 lanes; cap <= 0: none (DFX_LINEAR_GRID)
inline int lin_grid(const dfx_linear_desc &d, int path, int bm, int cus, long long cap) {
  if (cus < 1) cus = 1;
  long long blocks = path == DFX_LINEAR_TILE ? lin_tiles(d, bm) : (lin_items(d) + LIN_THREADS - 1) / LIN_THREADS;
  const long long most = (long long)cus * (path == DFX_LINEAR_TILE ? LIN_TILE_GRID_PER_CU : LIN_GEN_GRID_PER_CU);
  if (blocks > most) blocks = most;
  if (cap > 0 && blocks > cap) blocks = cap;
  return (int)(blocks < 1 ? 1 : blocks);
}

// tile kernel: two slab buffers of (BM tokens + LIN_BN weight rows) x LIN_KS bytes | comp, bias, scale of the tile's
// LIN_BN columns | the table
inline int lin_lds_bytes(int path, int bm) {
  return path == DFX_LINEAR_TILE ? 2 * (bm * LIN_KS + LIN_WBLOCK) + 3 * LIN_BN * 4 + 256 : 0;
}

// The device image: packed weights | comp | bias | scale | table.  The constants have LIN_BN entries per n-block (the
// entries n .. stay 0); every section starts at a multiple of 16.
struct LinImage {
  size_t off_comp, off_bias, off_scale, off_table, bytes;
};
inline size_t lin_packed_bytes(int n, int k) { return (size_t)lin_nblocks(n) * (size_t)lin_nslabs(k) * LIN_WBLOCK; }
inline LinImage lin_image(int n, int k) {
  LinImage im;
  const size_t consts = (size_t)lin_nblocks(n) * LIN_BN * 4;
  im.off_comp = lin_packed_bytes(n, k);
  im.off_bias = im.off_comp + consts;
  im.off_scale = im.off_bias + consts;
  im.off_table = im.off_scale + consts;
  im.bytes = im.off_table + 256;
  return im;
}

inline unsigned long long lin_algorithmic_ops(const dfx_linear_desc &d) {
  return 2ull * (unsigned long long)d.rows * (unsigned long long)d.n * (unsigned long long)d.k;
}
// src's valid bytes + the weights + dst's elements + bias (as f32) and scales as given + the table
inline unsigned long long lin_algorithmic_bytes(const dfx_linear_desc &d) {
  return (unsigned long long)d.rows * d.k + (unsigned long long)d.n * d.k +
         (unsigned long long)d.rows * d.n * (unsigned)plan_dt_size(d.dst_dt) + (d.bia_dt != DFX_UNDEF ? 4ull * d.n : 0) + 4ull * d.nscales +
         (lin_has_table(d) ? 256 : 0);
}


}  // namespace dfx
