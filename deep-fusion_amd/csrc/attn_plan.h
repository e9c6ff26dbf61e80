// attn_plan.h -- host-only, plain C++: what the fused int8 attention (dfx_attn_* of include/dfx.h) decides before a kernel
// runs: the descriptor's validation in the order the header documents, the descriptors of the three ops it is defined by
// (dfx_bmm NT, dfx_head softmax, dfx_bmm NN over the handle's scratch), the fused kernel's class and LDS plan, the auto
// rule, both requant-route proofs (bmm_plan.h's, on those descriptors), the grid and the algorithmic counts.
// No HIP in here, so that it can be built and run on its own (tools/attn_plan_check.cc, under the host sanitizers).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "bmm_plan.h"
#include "plan_common.h"
#include "head_plan.h"

namespace dfx {

constexpr int ATTN_THREADS = 256;                // four waves own a strip of 32 query rows of one g
constexpr int ATTN_WAVES = ATTN_THREADS / 64;
constexpr int ATTN_STRIP = 32;
constexpr int ATTN_D_MAX = 256;                  // the strip's Q fragments: 8 steps of 32 d, 32 VGPRs
constexpr int ATTN_TK_MAX = 4096;                // the class bound on tk (the non-local point)
constexpr int ATTN_TK_LIMIT = BMM_KMAX;          // the descriptor's bound on tk: dfx_bmm's K (below dfx_head's c of 65535)
static_assert(ATTN_TK_LIMIT <= DFX_HEAD_MAX_C, "tk is also the softmax's c");
constexpr int ATTN_GRID_PER_CU = 8;              // workgroups per CU at most; the rest is the kernel's loop
constexpr int ATTN_V_LDS = BMM_NN_LDS;           // the four waves' transposed V images (bmm.cuh's), reused for the split-key sums
constexpr int ATTN_LDS_MAX = 160 * 1024;

inline long long attn_matrices(const dfx_attn_desc &d) { return (long long)d.batch0 * d.batch1; }
// leading dimension (bytes = elements) of the chain's L and P scratch; the fused strip's rows are 16 longer
inline long long attn_ldl(const dfx_attn_desc &d) { return plan_up16(d.tk); }
inline long long attn_pitch(const dfx_attn_desc &d) { return plan_up16(d.tk) + 16; }
inline unsigned long long attn_scratch_bytes(const dfx_attn_desc &d) {  // L and P together
  return 2ull * (unsigned long long)attn_matrices(d) * (unsigned long long)d.tq * (unsigned long long)attn_ldl(d);
}

// the three ops the attention is defined by.  L and P are {G, tq, up16(tk)} in scratch.
inline dfx_bmm_desc attn_bmm_logits(const dfx_attn_desc &d) {
  dfx_bmm_desc b = {};
  b.batch0 = d.batch0; b.batch1 = d.batch1; b.m = d.tq; b.n = d.tk; b.k = d.d;
  b.trans_b = 1; b.a_dt = d.q_dt; b.b_dt = d.k_dt; b.dst_dt = DFX_S8; b.relu = 0; b.round_mode = d.round_mode;
  b.nscales = 1; b.force_path = -1;
  b.a_s0 = d.q_s0; b.a_s1 = d.q_s1; b.lda = d.ldq;
  b.b_s0 = d.k_s0; b.b_s1 = d.k_s1; b.ldb = d.ldk;
  b.ldc = attn_ldl(d); b.c_s1 = (long long)d.tq * b.ldc; b.c_s0 = (long long)d.batch1 * b.c_s1;
  return b;
}
inline dfx_head_desc attn_head_softmax(const dfx_attn_desc &d) {
  dfx_head_desc h = {};
  h.rows = attn_matrices(d) * d.tq;
  h.mode = DFX_HEAD_SOFTMAX; h.src_dt = DFX_S8; h.dst_dt = DFX_U8; h.c = d.tk;
  h.src_ld = h.dst_ld = (int)attn_ldl(d);
  h.out_scale = d.prob_scale; h.force_path = -1;
  return h;
}
inline dfx_bmm_desc attn_bmm_context(const dfx_attn_desc &d) {
  dfx_bmm_desc b = {};
  b.batch0 = d.batch0; b.batch1 = d.batch1; b.m = d.tq; b.n = d.dv; b.k = d.tk;
  b.trans_b = 0; b.a_dt = DFX_U8; b.b_dt = d.v_dt; b.dst_dt = d.dst_dt; b.relu = d.relu; b.round_mode = d.round_mode;
  b.nscales = d.nscales; b.force_path = -1;
  b.lda = attn_ldl(d); b.a_s1 = (long long)d.tq * b.lda; b.a_s0 = (long long)d.batch1 * b.a_s1;
  b.b_s0 = d.v_s0; b.b_s1 = d.v_s1; b.ldb = d.ldv;
  b.c_s0 = d.o_s0; b.c_s1 = d.o_s1; b.ldc = d.ldo;
  return b;
}

inline bool attn_fused_class(const dfx_attn_desc &d);

// DFX_OK, or the code dfx_attn_create returns with *why set to the reason.  Everything DFX_ERR_INVALID is found before
// anything DFX_ERR_UNSUPPORTED.
inline int attn_validate(const dfx_attn_desc &d, const char **why) {
  const char *dummy;
  if (!why) why = &dummy;
  *why = "";
  if (d.batch0 < 1 || d.batch1 < 1 || d.tq < 1 || d.tk < 1 || d.d < 1 || d.dv < 1) return *why = "non-positive size", DFX_ERR_INVALID;
  if (d.tq > BMM_MN_MAX || d.dv > BMM_MN_MAX) return *why = "tq or dv beyond 2^31 - 32", DFX_ERR_INVALID;
  if (d.d > BMM_KMAX) return *why = "d beyond 65025 (the accumulator could leave s32)", DFX_ERR_INVALID;
  // (tk is the softmax's c, at most 65535, AND the context product's K, at most 65025: the smaller one holds)
  if (d.tk > ATTN_TK_LIMIT) return *why = "tk beyond 65025 (the context's accumulator could leave s32)", DFX_ERR_INVALID;
  if (d.q_dt != DFX_U8 && d.q_dt != DFX_S8) return *why = "bad q dtype (u8 or s8)", DFX_ERR_INVALID;
  if (d.k_dt != DFX_U8 && d.k_dt != DFX_S8) return *why = "bad k dtype (s8)", DFX_ERR_INVALID;
  if (d.v_dt != DFX_U8 && d.v_dt != DFX_S8) return *why = "bad v dtype (s8)", DFX_ERR_INVALID;
  if (!bmm_dt_ok(d.dst_dt)) return *why = "bad dst dtype", DFX_ERR_INVALID;
  if (d.round_mode != DFX_ROUND_NEAREST && d.round_mode != DFX_ROUND_DOWN) return *why = "bad round mode", DFX_ERR_INVALID;
  if (d.nscales != 1 && d.nscales != d.dv) return *why = "out scales count must be 1 or dv", DFX_ERR_INVALID;
  if (d.force_path != -1 && d.force_path != DFX_ATTN_FUSED && d.force_path != DFX_ATTN_CHAIN) return *why = "bad force_path", DFX_ERR_INVALID;
  // (NaN fails both comparisons)
  if (!(d.prob_scale >= -3.4028234e38f && d.prob_scale <= 3.4028234e38f)) return *why = "prob_scale is not finite", DFX_ERR_INVALID;
  if (d.ldq < d.d) return *why = "ldq below d", DFX_ERR_INVALID;
  if (d.ldk < d.d) return *why = "ldk below d", DFX_ERR_INVALID;
  if (d.ldv < d.dv) return *why = "ldv below dv", DFX_ERR_INVALID;
  if (d.ldo < d.dv) return *why = "ldo below dv", DFX_ERR_INVALID;
  if (d.q_s0 < 0 || d.q_s1 < 0 || d.k_s0 < 0 || d.k_s1 < 0 || d.v_s0 < 0 || d.v_s1 < 0 || d.o_s0 < 0 || d.o_s1 < 0)
    return *why = "negative stride", DFX_ERR_INVALID;
  const dfx_bmm_desc b0 = attn_bmm_logits(d), b1 = attn_bmm_context(d);
  if (!bmm_c_disjoint(b1)) return *why = "elements of O could overlap (strides against extents)", DFX_ERR_INVALID;
  const unsigned __int128 lim = (unsigned __int128)BMM_MAX_ELEMS;
  if (bmm_span(b0, d.q_s0, d.q_s1, d.ldq, d.tq, d.d) >= lim || bmm_span(b0, d.k_s0, d.k_s1, d.ldk, d.tk, d.d) >= lim ||
      bmm_span(b1, d.v_s0, d.v_s1, d.ldv, d.tk, d.dv) >= lim || bmm_span(b1, d.o_s0, d.o_s1, d.ldo, d.tq, d.dv) >= lim)
    return *why = "an operand's index range reaches 2^40 elements", DFX_ERR_INVALID;
  if ((unsigned __int128)attn_matrices(d) * (unsigned __int128)d.tq * (unsigned __int128)attn_ldl(d) >= lim)
    return *why = "the logits' G * tq * up16(tk) reach 2^40", DFX_ERR_INVALID;
  if (d.k_dt == DFX_U8 || d.v_dt == DFX_U8) return *why = "u8 K / V is not built", DFX_ERR_UNSUPPORTED;
  if (d.force_path == DFX_ATTN_FUSED && !attn_fused_class(d))
    return *why = "descriptor outside the fused kernel's class (ldq, ldk, ldv and the batch strides of Q, K, V multiples of 16; d <= 256; "
                  "tk <= 4096)",
           DFX_ERR_UNSUPPORTED;
  return DFX_OK;
}

// bytes of dynamic LDS of the fused kernel: [table][strip L / P: 32 rows of `pitch`][V images / split-key sums]
inline long long attn_lds_bytes(const dfx_attn_desc &d) { return HEAD_TABLE_BYTES + (long long)ATTN_STRIP * attn_pitch(d) + ATTN_V_LDS; }

// the class of the fused kernel as far as the descriptor decides it (the alignment of q, k, v is checked per submit)
inline bool attn_fused_class(const dfx_attn_desc &d) {
  return d.k_dt == DFX_S8 && d.v_dt == DFX_S8 && d.ldq % 16 == 0 && d.ldk % 16 == 0 && d.ldv % 16 == 0 && d.q_s0 % 16 == 0 &&
         d.q_s1 % 16 == 0 && d.k_s0 % 16 == 0 && d.k_s1 % 16 == 0 && d.v_s0 % 16 == 0 && d.v_s1 % 16 == 0 && d.d <= ATTN_D_MAX &&
         d.tk <= ATTN_TK_MAX && attn_lds_bytes(d) <= ATTN_LDS_MAX;
}

// AUTO RULE (include/dfx.h DFX_ATTN_AUTO_NOTE, DESIGN.md section 4.22, measured in profiles/attn/): the fused kernel in its class
// inside the box of the points at which tools/bench_attn timed it against the chain and it won by more than the rounds'
// spread -- ViT-B (T 197, d 64), a Swin stage (T 49, d 32, 384 strips), a DETR encoder (T 850, d 32): from the smallest tq, tk,
// d, dv and strip count of those on, and up to the largest tk, d and dv of those, because beyond them lies the non-local point
// (tk 4096, d = dv = 256), where it LOSES 2.1x; what lies between was never timed and stays on the chain, like everything smaller.
constexpr int ATTN_AUTO_MIN_TQ = 49, ATTN_AUTO_MIN_TK = 49, ATTN_AUTO_MAX_TK = 850;
constexpr int ATTN_AUTO_MIN_D = 32, ATTN_AUTO_MAX_D = 64;   // d and dv
constexpr long long ATTN_AUTO_MIN_STRIPS = 384;
inline long long attn_strips(const dfx_attn_desc &d);
inline bool attn_auto_fused(const dfx_attn_desc &d) {
  return d.tq >= ATTN_AUTO_MIN_TQ && d.tk >= ATTN_AUTO_MIN_TK && d.tk <= ATTN_AUTO_MAX_TK && d.d >= ATTN_AUTO_MIN_D && d.d <= ATTN_AUTO_MAX_D &&
         d.dv >= ATTN_AUTO_MIN_D && d.dv <= ATTN_AUTO_MAX_D && attn_strips(d) >= ATTN_AUTO_MIN_STRIPS;
}
inline int attn_path(const dfx_attn_desc &d) {
  if (d.force_path != -1) return d.force_path;
  return attn_fused_class(d) && attn_auto_fused(d) ? DFX_ATTN_FUSED : DFX_ATTN_CHAIN;
}

// both requant routes, proved from the shape as dfx_bmm_set_scales does
inline bool attn_fast_logits(const dfx_attn_desc &d, float logit_scale) { return bmm_fast_ok(attn_bmm_logits(d), &logit_scale); }
inline bool attn_fast_context(const dfx_attn_desc &d, const float *out_scales) { return bmm_fast_ok(attn_bmm_context(d), out_scales); }

// strips of 32 query rows: the fused kernel's units
inline long long attn_strips(const dfx_attn_desc &d) { return attn_matrices(d) * (((long long)d.tq + ATTN_STRIP - 1) / ATTN_STRIP); }
// the context's column tiles and the parts the key range is split into where there are fewer tiles than waves
inline long long attn_vtiles(const dfx_attn_desc &d) { return ((long long)d.dv + 31) / 32; }
inline int attn_kparts(const dfx_attn_desc &d) {
  const long long t = attn_vtiles(d);
  return t >= ATTN_WAVES ? 1 : (int)(ATTN_WAVES / t);
}
// workgroups of the fused kernel; cap <= 0: none (DFX_ATTN_GRID)
inline int attn_grid(const dfx_attn_desc &d, int cus, long long cap) {
  long long blocks = attn_strips(d);
  const long long most = (long long)(cus < 1 ? 1 : cus) * ATTN_GRID_PER_CU;
  if (blocks > most) blocks = most;
  if (cap > 0 && blocks > cap) blocks = cap;
  return (int)(blocks < 1 ? 1 : blocks);
}

inline unsigned long long attn_algorithmic_ops(const dfx_attn_desc &d) {
  return 2ull * (unsigned long long)attn_matrices(d) * (unsigned long long)d.tq * (unsigned long long)d.tk *
         ((unsigned long long)d.d + (unsigned long long)d.dv);
}
// the distinct bytes of Q, K, V and O: an operand broadcast over a batch dimension (stride 0) counts once over it
inline unsigned long long attn_algorithmic_bytes(const dfx_attn_desc &d) {
  const unsigned long long gq = (unsigned long long)(d.q_s0 == 0 ? 1 : d.batch0) * (unsigned long long)(d.q_s1 == 0 ? 1 : d.batch1);
  const unsigned long long gk = (unsigned long long)(d.k_s0 == 0 ? 1 : d.batch0) * (unsigned long long)(d.k_s1 == 0 ? 1 : d.batch1);
  const unsigned long long gv = (unsigned long long)(d.v_s0 == 0 ? 1 : d.batch0) * (unsigned long long)(d.v_s1 == 0 ? 1 : d.batch1);
  return gq * (unsigned long long)d.tq * d.d + gk * (unsigned long long)d.tk * d.d + gv * (unsigned long long)d.tk * d.dv +
         (unsigned long long)attn_matrices(d) * d.tq * d.dv * (unsigned)plan_dt_size(d.dst_dt);
}

}  // namespace dfx
