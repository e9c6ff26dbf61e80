// bmm_plan.h -- host-only, plain C++: what the batched int8 matrix product (dfx_bmm_* of include/dfx.h) decides before a
// kernel runs: the descriptor's validation in the order the header documents (the C-overlap rule and the 2^40 limit
// included), the MFMA kernel's class, the auto rule, the proof of the fast requant route from the shape alone, the extent
// of every operand (for the overlap check of a submit), the grids and the algorithmic counts.
// No HIP in here, so that it can be built and run on its own (tools/bmm_plan_check.cc, under the host sanitizers).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cmath>

#include "../../include/dfx.h"
#include "plan_common.h"

namespace dfx {

constexpr int BMM_THREADS = 256;                 // four waves; a wave owns a 32 x 32 tile of C
constexpr int BMM_WAVES = BMM_THREADS / 64;
constexpr int BMM_KMAX = 65025;
constexpr int BMM_MN_MAX = 2147483647 - 31;        // m and n rounded up to 32 fit an int (tiles, the scale buffer)
constexpr long long BMM_MAX_ELEMS = 1ll << 40;   // an operand's index range must stay below it
constexpr int BMM_GRID_PER_CU = 16;              // workgroups per CU at most; the rest is the kernels' loop
constexpr int BMM_NN_PITCH = 48;                 // bytes per transposed B row in LDS: 32 k + 16 (16-byte aligned rows)
constexpr int BMM_NN_LDS = BMM_WAVES * 2 * 32 * BMM_NN_PITCH;   // two buffers per wave

inline bool bmm_dt_ok(int dt) { return dt == DFX_F32 || dt == DFX_S32 || dt == DFX_S8 || dt == DFX_U8; }
inline long long bmm_b_rows(const dfx_bmm_desc &d) { return d.trans_b ? d.n : d.k; }
inline long long bmm_b_cols(const dfx_bmm_desc &d) { return d.trans_b ? d.k : d.n; }

// The rule for C: the (extent, stride) pairs (N,1), (M,ldc), (batch1,c_s1), (batch0,c_s0) without the extents of 1, sorted
// by stride; the first stride must be at least 1 and each further one at least the previous stride times the previous
// extent.  Then no two elements share an address.  (Strides are >= 0 and below 2^62 here; the products are taken in 128 bits.)
inline bool bmm_c_disjoint(const dfx_bmm_desc &d) {
  long long ext[4] = {d.n, d.m, d.batch1, d.batch0};
  long long str[4] = {1, d.ldc, d.c_s1, d.c_s0};
  int cnt = 0;
  for (int i = 0; i < 4; ++i)
    if (ext[i] != 1) {
      ext[cnt] = ext[i];
      str[cnt] = str[i];
      ++cnt;
    }
  for (int i = 1; i < cnt; ++i)  // insertion sort by stride (stable)
    for (int j = i; j > 0 && str[j] < str[j - 1]; --j) {
      const long long e = ext[j], s = str[j];
      ext[j] = ext[j - 1]; str[j] = str[j - 1];
      ext[j - 1] = e; str[j - 1] = s;
    }
  if (cnt > 0 && str[0] < 1) return false;  // a stride of 0 under an extent above 1 (the first pair has no predecessor)
  for (int i = 1; i < cnt; ++i)
    if ((unsigned __int128)str[i] < (unsigned __int128)str[i - 1] * (unsigned __int128)ext[i - 1]) return false;
  return true;
}

// one past the largest element index of an operand with `rows` x `cols` valid elements per matrix (128 bits: no overflow)
inline unsigned __int128 bmm_span(const dfx_bmm_desc &d, long long s0, long long s1, long long ld, long long rows, long long cols) {
  return (unsigned __int128)(d.batch0 - 1) * (unsigned __int128)s0 + (unsigned __int128)(d.batch1 - 1) * (unsigned __int128)s1 +
         (unsigned __int128)(rows - 1) * (unsigned __int128)ld + (unsigned __int128)cols;
}
inline unsigned long long bmm_a_elems(const dfx_bmm_desc &d) { return (unsigned long long)bmm_span(d, d.a_s0, d.a_s1, d.lda, d.m, d.k); }
inline unsigned long long bmm_b_elems(const dfx_bmm_desc &d) {
  return (unsigned long long)bmm_span(d, d.b_s0, d.b_s1, d.ldb, bmm_b_rows(d), bmm_b_cols(d));
}
inline unsigned long long bmm_c_elems(const dfx_bmm_desc &d) { return (unsigned long long)bmm_span(d, d.c_s0, d.c_s1, d.ldc, d.m, d.n); }

// DFX_OK, or the code dfx_bmm_create returns with *why set to the reason.  Everything DFX_ERR_INVALID is found before
// anything DFX_ERR_UNSUPPORTED.
inline bool bmm_mfma_class(const dfx_bmm_desc &d);
inline int bmm_validate(const dfx_bmm_desc &d, const char **why) {
  const char *dummy;
  if (!why) why = &dummy;
  *why = "";
  if (d.batch0 < 1 || d.batch1 < 1 || d.m < 1 || d.n < 1 || d.k < 1) return *why = "non-positive size", DFX_ERR_INVALID;
  if (d.m > BMM_MN_MAX || d.n > BMM_MN_MAX) return *why = "m or n beyond 2^31 - 32 (rounded up to 32 it must fit an int)", DFX_ERR_INVALID;
  if (d.k > BMM_KMAX) return *why = "k beyond 65025 (the accumulator could leave s32)", DFX_ERR_INVALID;
  if (d.trans_b != 0 && d.trans_b != 1) return *why = "bad trans_b", DFX_ERR_INVALID;
  if (d.a_dt != DFX_U8 && d.a_dt != DFX_S8) return *why = "bad a dtype (u8 or s8)", DFX_ERR_INVALID;
  if (d.b_dt != DFX_U8 && d.b_dt != DFX_S8) return *why = "bad b dtype (s8)", DFX_ERR_INVALID;
  if (!bmm_dt_ok(d.dst_dt)) return *why = "bad dst dtype", DFX_ERR_INVALID;
  if (d.round_mode != DFX_ROUND_NEAREST && d.round_mode != DFX_ROUND_DOWN) return *why = "bad round mode", DFX_ERR_INVALID;
  if (d.nscales != 1 && d.nscales != d.n) return *why = "scales count must be 1 or n", DFX_ERR_INVALID;
  if (d.force_path != -1 && d.force_path != DFX_BMM_MFMA && d.force_path != DFX_BMM_GENERIC) return *why = "bad force_path", DFX_ERR_INVALID;
  if (d.lda < d.k) return *why = "lda below k", DFX_ERR_INVALID;
  if (d.ldb < bmm_b_cols(d)) return *why = d.trans_b ? "ldb below k" : "ldb below n", DFX_ERR_INVALID;
  if (d.ldc < d.n) return *why = "ldc below n", DFX_ERR_INVALID;
  if (d.a_s0 < 0 || d.a_s1 < 0 || d.b_s0 < 0 || d.b_s1 < 0 || d.c_s0 < 0 || d.c_s1 < 0) return *why = "negative stride", DFX_ERR_INVALID;
  // (a stride of 2^40 or more cannot belong to an operand below the limit unless its extent is 1: the limit below finds
  //  it; it also keeps the 128-bit products far from overflow)
  if (!bmm_c_disjoint(d)) return *why = "elements of C could overlap (strides against extents)", DFX_ERR_INVALID;
  const unsigned __int128 lim = (unsigned __int128)BMM_MAX_ELEMS;
  if (bmm_span(d, d.a_s0, d.a_s1, d.lda, d.m, d.k) >= lim || bmm_span(d, d.b_s0, d.b_s1, d.ldb, bmm_b_rows(d), bmm_b_cols(d)) >= lim ||
      bmm_span(d, d.c_s0, d.c_s1, d.ldc, d.m, d.n) >= lim)
    return *why = "an operand's index range reaches 2^40 elements", DFX_ERR_INVALID;
  if (d.b_dt == DFX_U8) return *why = "u8 B is not built", DFX_ERR_UNSUPPORTED;
  if (d.force_path == DFX_BMM_MFMA && !bmm_mfma_class(d))
    return *why = "descriptor outside the MFMA kernel's class (lda, ldb and the batch strides of A and B multiples of 16)", DFX_ERR_UNSUPPORTED;
  return DFX_OK;
}

// the class of the MFMA kernel as far as the descriptor decides it (the alignment of a and b is checked per submit)
inline bool bmm_mfma_class(const dfx_bmm_desc &d) {
  return d.b_dt == DFX_S8 && d.lda % 16 == 0 && d.ldb % 16 == 0 && d.a_s0 % 16 == 0 && d.a_s1 % 16 == 0 && d.b_s0 % 16 == 0 &&
         d.b_s1 % 16 == 0;
}

// AUTO RULE (include/dfx.h DFX_BMM_AUTO_NOTE, DESIGN.md section 4.21, measured in profiles/bmm/): the MFMA kernel in its
// class from the smallest of each size at which tools/bench_bmm timed it and it won: M >= 49, N >= 32, K >= 32 (the Swin window
// point: 192 matrices of 49 x 49 x 32 and 49 x 32 x 49), G * M * N * K >= 192 * 49 * 49 * 32, and at least 384 tiles of 32 x 32
// (the fewest that were timed: Swin P.V; the deepest K loops timed, 850 and 4096, ran on 432 and 1024 tiles).  A few tiles
// under a deep K -- one workgroup walking up to 65025 k -- were never timed and stay generic, like everything smaller; the
// MFMA kernel is reachable there with force_path.
constexpr long long BMM_AUTO_MIN_MACS = 192ll * 49 * 49 * 32;
constexpr long long BMM_AUTO_MIN_TILES = 384;
constexpr int BMM_AUTO_MIN_M = 49, BMM_AUTO_MIN_N = 32, BMM_AUTO_MIN_K = 32;
inline bool bmm_auto_mfma(const dfx_bmm_desc &d) {
  if (d.m < BMM_AUTO_MIN_M || d.n < BMM_AUTO_MIN_N || d.k < BMM_AUTO_MIN_K) return false;
  const unsigned __int128 g = (unsigned __int128)((long long)d.batch0 * d.batch1);
  if (g * (unsigned __int128)((((long long)d.m + 31) / 32) * (((long long)d.n + 31) / 32)) < (unsigned __int128)BMM_AUTO_MIN_TILES) return false;
  return g * (unsigned __int128)((long long)d.m * d.n) * (unsigned)d.k >= (unsigned __int128)BMM_AUTO_MIN_MACS;
}
inline int bmm_path(const dfx_bmm_desc &d) {
  if (d.force_path != -1) return d.force_path;
  return bmm_mfma_class(d) && bmm_auto_mfma(d) ? DFX_BMM_MFMA : DFX_BMM_GENERIC;
}

// the fast requant route's proof from the shape alone: |acc| <= bound, scales finite, bound * |scale| <= 2^30
inline double bmm_acc_bound(const dfx_bmm_desc &d) { return (d.a_dt == DFX_U8 ? 255.0 : 128.0) * 128.0 * (double)d.k; }
inline bool bmm_fast_ok(const dfx_bmm_desc &d, const float *scales) {
  if (d.round_mode != DFX_ROUND_NEAREST) return false;
  const double bound = bmm_acc_bound(d);
  for (int i = 0; i < d.nscales; ++i) {
    if (!std::isfinite(scales[i])) return false;
    if (bound * std::fabs((double)scales[i]) > 1073741824.0) return false;  // 2^30
  }
  return true;
}

inline long long bmm_matrices(const dfx_bmm_desc &d) { return (long long)d.batch0 * d.batch1; }
inline long long bmm_mtiles(const dfx_bmm_desc &d) { return ((long long)d.m + 31) / 32; }
inline long long bmm_ntiles(const dfx_bmm_desc &d) { return ((long long)d.n + 31) / 32; }
inline long long bmm_tiles(const dfx_bmm_desc &d) { return bmm_matrices(d) * bmm_mtiles(d) * bmm_ntiles(d); }
// workgroup units of the MFMA kernel: BMM_WAVES consecutive tiles each
inline long long bmm_units(const dfx_bmm_desc &d) { return (bmm_tiles(d) + BMM_WAVES - 1) / BMM_WAVES; }
inline long long bmm_items(const dfx_bmm_desc &d) { return bmm_matrices(d) * d.m * d.n; }

// workgroups of 256 lanes; cap <= 0: none (DFX_BMM_GRID)
inline int bmm_grid(const dfx_bmm_desc &d, int path, int cus, long long cap) {
  long long blocks = path == DFX_BMM_MFMA ? bmm_units(d) : (bmm_items(d) + BMM_THREADS - 1) / BMM_THREADS;
  const long long most = (long long)(cus < 1 ? 1 : cus) * BMM_GRID_PER_CU;
  if (blocks > most) blocks = most;
  if (cap > 0 && blocks > cap) blocks = cap;
  return (int)(blocks < 1 ? 1 : blocks);
}
inline int bmm_lds_bytes(const dfx_bmm_desc &d, int path) { return path == DFX_BMM_MFMA && !d.trans_b ? BMM_NN_LDS : 0; }

inline unsigned long long bmm_algorithmic_ops(const dfx_bmm_desc &d) {
  return 2ull * (unsigned long long)bmm_matrices(d) * (unsigned long long)d.m * (unsigned long long)d.n * (unsigned long long)d.k;
}
// the distinct bytes of A, B and C: an operand broadcast over a batch dimension (stride 0) counts once over it
inline unsigned long long bmm_algorithmic_bytes(const dfx_bmm_desc &d) {
  const unsigned long long ga = (unsigned long long)(d.a_s0 == 0 ? 1 : d.batch0) * (unsigned long long)(d.a_s1 == 0 ? 1 : d.batch1);
  const unsigned long long gb = (unsigned long long)(d.b_s0 == 0 ? 1 : d.batch0) * (unsigned long long)(d.b_s1 == 0 ? 1 : d.batch1);
  return ga * (unsigned long long)d.m * d.k + gb * (unsigned long long)d.k * d.n +
         (unsigned long long)bmm_matrices(d) * d.m * d.n * (unsigned)plan_dt_size(d.dst_dt);
}


}  // namespace dfx
