// attn_plan_check -- host-only check of csrc/attn_plan.h, what the fused attention (dfx_attn_*) decides before a kernel runs:
// the descriptor's validation at the last admitted and the first refused value of every clause, in the header's order
// (INVALID before UNSUPPORTED), the O-overlap rule on the interleaved-heads layout, the 2^40 limits, the fused class and its
// LDS plan at the bound on tk, both requant-route proofs at their edges, the key split, the grid under the cap, the three
// descriptors of the chain and the algorithmic counts.  No HIP: it builds with SAN=1 (ASan + UBSan) and runs anywhere.
//   attn_plan_check        the self-check
//   attn_plan_check -      reads descriptors from stdin, one per line: the fields of dfx_attn_desc in its order (prob_scale as
//                          a decimal float), then cus, cap, a logit scale and ONE out scale (used for every channel); prints
//                          "rc class path lds strips kparts grid fast_logits fast_context scratch ops bytes chain_ok"
//                          (chain_ok: the three ops accept the chain's descriptors; -1 where rc is not 0)
//                          (tests/test_attn_cpu.py compares them with the Python mirror of tests/attn_ref.py)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../csrc/attn_plan.h"

using namespace dfx;

static int g_bad = 0;
#define EXPECT(cond)                                                 \
  do {                                                               \
    if (!(cond)) {                                                   \
      printf("attn_plan_check: line %d: %s\n", __LINE__, #cond);     \
      ++g_bad;                                                       \
    }                                                                \
  } while (0)

// densely packed {batch0, batch1} matrices, leading dimensions of Q, K, V rounded up to 16
static dfx_attn_desc dense(int b0, int b1, int tq, int tk, int d, int dv) {
  dfx_attn_desc a;
  memset(&a, 0, sizeof(a));
  a.batch0 = b0; a.batch1 = b1; a.tq = tq; a.tk = tk; a.d = d; a.dv = dv;
  a.q_dt = DFX_S8; a.k_dt = DFX_S8; a.v_dt = DFX_S8; a.dst_dt = DFX_S8; a.round_mode = DFX_ROUND_NEAREST; a.nscales = 1; a.force_path = -1;
  a.prob_scale = 255.0f;
  a.ldq = plan_up16(d); a.q_s1 = a.ldq * tq; a.q_s0 = a.q_s1 * b1;
  a.ldk = plan_up16(d); a.k_s1 = a.ldk * tk; a.k_s0 = a.k_s1 * b1;
  a.ldv = plan_up16(dv); a.v_s1 = a.ldv * tk; a.v_s0 = a.v_s1 * b1;
  a.ldo = dv; a.o_s1 = a.ldo * tq; a.o_s0 = a.o_s1 * b1;
  return a;
}
// the three ops the attention is defined by accept their descriptors: must hold wherever attn_validate returns DFX_OK, so that
// dfx_attn_create cannot fail in them after the attention's own validation has passed
static bool chain_ok(const dfx_attn_desc &d) {
  return bmm_validate(attn_bmm_logits(d), nullptr) == DFX_OK && head_validate(attn_head_softmax(d), nullptr) == DFX_OK &&
         bmm_validate(attn_bmm_context(d), nullptr) == DFX_OK;
}
static int rc(const dfx_attn_desc &d) {
  const char *why = nullptr;
  const int r = attn_validate(d, &why);
  if (r == DFX_OK) EXPECT(chain_ok(d));
  EXPECT(why != nullptr && (r == DFX_OK) == (why[0] == 0));
  EXPECT(attn_validate(d, nullptr) == r);
  return r;
}

static int from_stdin() {
  char line[2048];
  while (fgets(line, sizeof(line), stdin)) {
    long long v[28];
    double ps = 0, ls = 0, os = 0;
    int pos = 0, adv = 0;
    bool ok = true;
    for (int i = 0; i < 14 && ok; ++i) ok = sscanf(line + pos, "%lld%n", &v[i], &adv) == 1, pos += adv;
    if (ok) ok = sscanf(line + pos, "%lf%n", &ps, &adv) == 1, pos += adv;
    for (int i = 15; i < 28 && ok; ++i) ok = sscanf(line + pos, "%lld%n", &v[i], &adv) == 1, pos += adv;
    long long cus = 0, cap = 0;
    if (ok) ok = sscanf(line + pos, "%lld %lld %lf %lf", &cus, &cap, &ls, &os) == 4;
    if (!ok) {
      printf("bad line\n");
      return 2;
    }
    dfx_attn_desc d;
    memset(&d, 0, sizeof(d));
    d.batch0 = (int)v[0]; d.batch1 = (int)v[1]; d.tq = (int)v[2]; d.tk = (int)v[3]; d.d = (int)v[4]; d.dv = (int)v[5];
    d.q_dt = (int)v[6]; d.k_dt = (int)v[7]; d.v_dt = (int)v[8]; d.dst_dt = (int)v[9]; d.relu = (int)v[10]; d.round_mode = (int)v[11];
    d.nscales = (int)v[12]; d.force_path = (int)v[13]; d.prob_scale = (float)ps; d.reserved = (int)v[15];
    d.q_s0 = v[16]; d.q_s1 = v[17]; d.ldq = v[18]; d.k_s0 = v[19]; d.k_s1 = v[20]; d.ldk = v[21];
    d.v_s0 = v[22]; d.v_s1 = v[23]; d.ldv = v[24]; d.o_s0 = v[25]; d.o_s1 = v[26]; d.ldo = v[27];
    const int r = attn_validate(d, nullptr);
    if (r == DFX_ERR_INVALID) {
      printf("%d\n", r);
      continue;
    }
    const std::vector<float> outs((size_t)d.nscales, (float)os);
    printf("%d %d %d %lld %lld %d %d %d %d %llu %llu %llu %d\n", r, (int)attn_fused_class(d), r ? -1 : attn_path(d), attn_lds_bytes(d), attn_strips(d),
           attn_kparts(d), attn_grid(d, (int)cus, cap), (int)attn_fast_logits(d, (float)ls), (int)attn_fast_context(d, outs.data()),
           attn_scratch_bytes(d), attn_algorithmic_ops(d), attn_algorithmic_bytes(d), r ? -1 : (int)chain_ok(d));
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 1 && strcmp(argv[1], "-") == 0) return from_stdin();
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  // ---- sizes and limits: each at its last admitted and first refused value
  EXPECT(rc(dense(1, 1, 1, 1, 1, 1)) == DFX_OK);
  EXPECT(rc(dense(0, 1, 1, 1, 1, 1)) == DFX_ERR_INVALID && rc(dense(1, 0, 1, 1, 1, 1)) == DFX_ERR_INVALID && rc(dense(1, 1, 0, 1, 1, 1)) == DFX_ERR_INVALID);
  EXPECT(rc(dense(1, 1, 1, 0, 1, 1)) == DFX_ERR_INVALID && rc(dense(1, 1, 1, 1, 0, 1)) == DFX_ERR_INVALID && rc(dense(1, 1, 1, 1, 1, 0)) == DFX_ERR_INVALID);
  EXPECT(rc(dense(1, 1, 33, 33, 65025, 33)) == DFX_OK && rc(dense(1, 1, 33, 33, 65026, 33)) == DFX_ERR_INVALID);
  EXPECT(rc(dense(1, 1, 33, 65025, 16, 33)) == DFX_OK && rc(dense(1, 1, 33, 65026, 16, 33)) == DFX_ERR_INVALID);  // the context's K
  EXPECT(rc(dense(1, 1, 33, 65025, 65025, 33)) == DFX_OK);                                                        // both contractions at their limit
  {
    dfx_attn_desc d = dense(1, 1, 1, 16, 16, 16);
    d.tq = 2147483647 - 31; EXPECT(rc(d) == DFX_OK);
    d.tq = 2147483647 - 30; EXPECT(rc(d) == DFX_ERR_INVALID);
    d = dense(1, 1, 1, 16, 16, 16);
    d.dv = 2147483647 - 31; d.ldv = d.ldo = d.dv; EXPECT(rc(d) == DFX_OK);
    d.dv = 2147483647 - 30; d.ldv = d.ldo = d.dv; EXPECT(rc(d) == DFX_ERR_INVALID);
  }
  for (int v = -2; v <= 6; ++v) {
    dfx_attn_desc d = dense(2, 3, 33, 37, 40, 35);
    d.q_dt = v; EXPECT(rc(d) == ((v == DFX_U8 || v == DFX_S8) ? DFX_OK : DFX_ERR_INVALID));
    d = dense(2, 3, 33, 37, 40, 35); d.k_dt = v; EXPECT(rc(d) == (v == DFX_S8 ? DFX_OK : v == DFX_U8 ? DFX_ERR_UNSUPPORTED : DFX_ERR_INVALID));
    d = dense(2, 3, 33, 37, 40, 35); d.v_dt = v; EXPECT(rc(d) == (v == DFX_S8 ? DFX_OK : v == DFX_U8 ? DFX_ERR_UNSUPPORTED : DFX_ERR_INVALID));
    d = dense(2, 3, 33, 37, 40, 35); d.dst_dt = v; EXPECT(rc(d) == ((v >= DFX_F32 && v <= DFX_U8) ? DFX_OK : DFX_ERR_INVALID));
    d = dense(2, 3, 33, 37, 40, 35); d.round_mode = v; EXPECT(rc(d) == ((v == 0 || v == 1) ? DFX_OK : DFX_ERR_INVALID));
    d = dense(2, 3, 33, 37, 40, 35); d.force_path = v; EXPECT(rc(d) == ((v >= -1 && v <= 1) ? DFX_OK : DFX_ERR_INVALID));
  }
  {
    dfx_attn_desc d = dense(2, 3, 33, 37, 40, 35);
    d.nscales = 35; EXPECT(rc(d) == DFX_OK);
    d.nscales = 34; EXPECT(rc(d) == DFX_ERR_INVALID);
    d.nscales = 0; EXPECT(rc(d) == DFX_ERR_INVALID);
    d = dense(2, 3, 33, 37, 40, 35);
    d.prob_scale = 3.4028234e38f; EXPECT(rc(d) == DFX_OK);
    d.prob_scale = -1.0f; EXPECT(rc(d) == DFX_OK);
    d.prob_scale = inf; EXPECT(rc(d) == DFX_ERR_INVALID);
    d.prob_scale = nan; EXPECT(rc(d) == DFX_ERR_INVALID);
    // INVALID is found before UNSUPPORTED
    d = dense(2, 3, 33, 37, 40, 35); d.k_dt = DFX_U8; d.ldo = 34; EXPECT(rc(d) == DFX_ERR_INVALID);
  }
  // ---- leading dimensions and strides
  {
    dfx_attn_desc d = dense(2, 3, 33, 37, 40, 35);
    d.ldq = 40; EXPECT(rc(d) == DFX_OK); d.ldq = 39; EXPECT(rc(d) == DFX_ERR_INVALID);
    d = dense(2, 3, 33, 37, 40, 35); d.ldk = 40; EXPECT(rc(d) == DFX_OK); d.ldk = 39; EXPECT(rc(d) == DFX_ERR_INVALID);
    d = dense(2, 3, 33, 37, 40, 35); d.ldv = 35; EXPECT(rc(d) == DFX_OK); d.ldv = 34; EXPECT(rc(d) == DFX_ERR_INVALID);
    d = dense(2, 3, 33, 37, 40, 35); d.ldo = 34; EXPECT(rc(d) == DFX_ERR_INVALID);
    int64_t dfx_attn_desc::*bcast[6] = {&dfx_attn_desc::q_s0, &dfx_attn_desc::q_s1, &dfx_attn_desc::k_s0, &dfx_attn_desc::k_s1, &dfx_attn_desc::v_s0,
                                          &dfx_attn_desc::v_s1};
    for (int i = 0; i < 6; ++i) {
      d = dense(2, 3, 33, 37, 40, 35); d.*bcast[i] = 0; EXPECT(rc(d) == DFX_OK);  // a broadcast
      d.*bcast[i] = -1; EXPECT(rc(d) == DFX_ERR_INVALID);
    }
    d = dense(2, 3, 33, 37, 40, 35); d.o_s0 = 0; EXPECT(rc(d) == DFX_ERR_INVALID);  // never on O
    d = dense(2, 3, 33, 37, 40, 35); d.o_s1 = 0; EXPECT(rc(d) == DFX_ERR_INVALID);
    d = dense(2, 3, 33, 37, 40, 35); d.o_s1 -= 1; EXPECT(rc(d) == DFX_ERR_INVALID);
    d = dense(2, 3, 33, 37, 40, 35); d.o_s0 += 1; EXPECT(rc(d) == DFX_OK);
    // interleaved heads: {bs 2, T 37, heads 3 * d 32}
    d = dense(2, 3, 37, 37, 32, 32);
    d.q_s0 = d.k_s0 = d.v_s0 = d.o_s0 = 37 * 96; d.q_s1 = d.k_s1 = d.v_s1 = d.o_s1 = 32; d.ldq = d.ldk = d.ldv = d.ldo = 96;
    EXPECT(rc(d) == DFX_OK && attn_fused_class(d));
    d.o_s1 = 31; EXPECT(rc(d) == DFX_ERR_INVALID);
    d.o_s1 = 32; d.ldo = 95; EXPECT(rc(d) == DFX_ERR_INVALID);
    // the 2^40 limits
    d = dense(2, 3, 33, 37, 40, 35);
    const long long q_span = (long long)bmm_span(attn_bmm_logits(d), 0, d.q_s1, d.ldq, d.tq, d.d);
    d.q_s0 = (1ll << 40) - 1 - q_span; EXPECT(rc(d) == DFX_OK);
    d.q_s0 = (1ll << 40) - q_span; EXPECT(rc(d) == DFX_ERR_INVALID);
    d = dense(2, 3, 33, 37, 40, 35); d.v_s0 = 1ll << 62; EXPECT(rc(d) == DFX_ERR_INVALID);
    d = dense(2, 3, 33, 37, 40, 35); d.o_s0 = 1ll << 40; EXPECT(rc(d) == DFX_ERR_INVALID);
    // the logits: G * tq * up16(tk) at tk's limit (up16(65025) = 65040): the first tq that reaches 2^40 and the one before
    const int tq_edge = (int)(((1ll << 40) + 65039) / 65040);
    d = dense(1, 1, tq_edge, 65025, 1, 1);
    EXPECT(rc(d) == DFX_ERR_INVALID);
    d = dense(1, 1, tq_edge - 1, 65025, 1, 1); EXPECT(rc(d) == DFX_OK);
    d = dense(1, 1, 2147483647 - 31, 1, 1, 2147483647 - 31); d.ldv = d.ldo = d.dv; d.o_s1 = d.o_s0 = 0;
    EXPECT(rc(d) == DFX_ERR_INVALID);  // (O's index range)
    // all three strides of every operand near their limit at once: 1024 x 1024 matrices, 2^30 / 2^20 apart, rows 2^10 (Q, O) and
    // 2^16 (K, V) apart: the extents the overlap check takes, the strips and the chain's descriptors at that range
    d = dense(1024, 1024, 1024, 16, 16, 16);
    d.dst_dt = DFX_F32; d.force_path = DFX_ATTN_FUSED;
    d.q_s0 = d.k_s0 = d.v_s0 = d.o_s0 = 1ll << 30; d.q_s1 = d.k_s1 = d.v_s1 = d.o_s1 = 1ll << 20; d.ldq = d.ldo = 1ll << 10; d.ldk = d.ldv = 1ll << 16;
    EXPECT(rc(d) == DFX_OK && attn_fused_class(d) && chain_ok(d));
    {
      const dfx_bmm_desc bl = attn_bmm_logits(d), bo = attn_bmm_context(d);
      EXPECT(bmm_a_elems(bl) == (1ull << 40) - 1024 + 16 && bmm_c_elems(bo) == (1ull << 40) - 1024 + 16);
      EXPECT(bmm_b_elems(bl) == 1023ull * (1ull << 30) + 1023ull * (1ull << 20) + 15ull * (1ull << 16) + 16 && bmm_b_elems(bo) == bmm_b_elems(bl));
      const uintptr_t far = (uintptr_t)1 << 47;
      const unsigned long long ob = 4 * bmm_c_elems(bo);
      EXPECT(plan_overlap(far, ob, far + ob - 1, 1) && !plan_overlap(far, ob, far + ob, 16) && !plan_overlap(far, ob, far - 16, 16) && plan_overlap(far, ob, far - 16, 17));
    }
    EXPECT(attn_strips(d) == 1ll << 25 && attn_grid(d, 256, 0) == 2048 && attn_grid(d, 256, 1ll << 40) == 2048);
    EXPECT(attn_algorithmic_ops(d) == 2ull * (1ull << 38) * 2);
    d.ldq += 1008; EXPECT(rc(d) == DFX_ERR_INVALID);  // Q's index range beyond 2^40 (the step keeps the class)
    d.ldq -= 1008; d.o_s1 -= 1; EXPECT(rc(d) == DFX_ERR_INVALID);  // (O's matrices would meet)
  }
  // ---- the fused class, its LDS plan, the forced path outside it
  {
    dfx_attn_desc d = dense(1, 1, 33, 4096, 16, 32);
    EXPECT(attn_fused_class(d) && attn_lds_bytes(d) == 1024 + 32 * 4112 + 12288 && attn_lds_bytes(d) <= ATTN_LDS_MAX);
    d.force_path = DFX_ATTN_FUSED; EXPECT(rc(d) == DFX_OK);
    d = dense(1, 1, 33, 4097, 16, 32); EXPECT(!attn_fused_class(d) && rc(d) == DFX_OK && attn_path(d) == DFX_ATTN_CHAIN);
    d.force_path = DFX_ATTN_FUSED; EXPECT(rc(d) == DFX_ERR_UNSUPPORTED);
    d.force_path = DFX_ATTN_CHAIN; EXPECT(rc(d) == DFX_OK);
    d = dense(1, 1, 33, 64, 256, 32); EXPECT(attn_fused_class(d));
    d = dense(1, 1, 33, 64, 257, 32); EXPECT(!attn_fused_class(d));
    int64_t dfx_attn_desc::*al[9] = {&dfx_attn_desc::q_s0, &dfx_attn_desc::q_s1, &dfx_attn_desc::ldq, &dfx_attn_desc::k_s0, &dfx_attn_desc::k_s1,
                                       &dfx_attn_desc::ldk, &dfx_attn_desc::v_s0, &dfx_attn_desc::v_s1, &dfx_attn_desc::ldv};
    for (int i = 0; i < 9; ++i) {
      d = dense(2, 3, 33, 37, 40, 35); d.force_path = DFX_ATTN_FUSED; EXPECT(rc(d) == DFX_OK);
      d.*al[i] += 8; EXPECT(!attn_fused_class(d) && rc(d) == DFX_ERR_UNSUPPORTED);
      d.force_path = -1; EXPECT(rc(d) == DFX_OK && attn_path(d) == DFX_ATTN_CHAIN);
    }
    d = dense(2, 3, 33, 37, 40, 35); EXPECT(attn_path(d) == DFX_ATTN_CHAIN);
    d.force_path = DFX_ATTN_FUSED; EXPECT(attn_path(d) == DFX_ATTN_FUSED);
    // the auto rule at both sides of each bound: the Swin stage's 64 x 3 windows of 49, d 32
    d = dense(64, 3, 49, 49, 32, 32); EXPECT(attn_strips(d) == 384 && attn_path(d) == DFX_ATTN_FUSED);
    d = dense(64, 3, 48, 49, 32, 32); EXPECT(attn_path(d) == DFX_ATTN_CHAIN);
    d = dense(64, 3, 49, 48, 32, 32); EXPECT(attn_path(d) == DFX_ATTN_CHAIN);
    d = dense(64, 3, 49, 49, 31, 32); EXPECT(attn_path(d) == DFX_ATTN_CHAIN);
    d = dense(64, 3, 49, 49, 32, 31); EXPECT(attn_path(d) == DFX_ATTN_CHAIN);
    d = dense(63, 3, 49, 49, 32, 32); EXPECT(attn_strips(d) == 378 && attn_path(d) == DFX_ATTN_CHAIN);
    d = dense(64, 3, 49, 850, 64, 64); EXPECT(attn_path(d) == DFX_ATTN_FUSED);
    d = dense(64, 3, 49, 851, 64, 64); EXPECT(attn_path(d) == DFX_ATTN_CHAIN);
    d = dense(64, 3, 49, 850, 65, 64); EXPECT(attn_path(d) == DFX_ATTN_CHAIN);
    d = dense(64, 3, 49, 850, 64, 65); EXPECT(attn_path(d) == DFX_ATTN_CHAIN);
    d = dense(4, 1, 4096, 4096, 256, 256); EXPECT(attn_fused_class(d) && attn_strips(d) == 512 && attn_path(d) == DFX_ATTN_CHAIN);  // the measured loss
    d = dense(64, 3, 49, 49, 32, 32); d.ldq += 8; EXPECT(attn_path(d) == DFX_ATTN_CHAIN);  // outside the class
  }
  // ---- both route proofs at their edges: bound * |scale| <= 2^30
  {
    dfx_attn_desc d = dense(1, 1, 33, 64, 64, 32);                            // s8 Q: 128 * 128 * 64 = 2^20; context 255 * 128 * 64
    EXPECT(attn_fast_logits(d, 1024.0f) && !attn_fast_logits(d, 1024.0001f) && !attn_fast_logits(d, inf) && !attn_fast_logits(d, nan));
    d.q_dt = DFX_U8; EXPECT(!attn_fast_logits(d, 1024.0f) && attn_fast_logits(d, 512.0f));
    const float edge = 1073741824.0f / (255.0f * 128.0f * 64.0f);
    float s = (double)edge * (255.0 * 128.0 * 64.0) > 1073741824.0 ? std::nextafter(edge, 0.0f) : edge;
    EXPECT(attn_fast_context(d, &s));
    s = edge * 1.0001f; EXPECT(!attn_fast_context(d, &s));
    s = nan; EXPECT(!attn_fast_context(d, &s));
    d.round_mode = DFX_ROUND_DOWN; s = 1.0f; EXPECT(!attn_fast_context(d, &s) && !attn_fast_logits(d, 1.0f));
  }
  // ---- strips, the key split, the grid, the chain's descriptors, the counts
  {
    dfx_attn_desc d = dense(2, 2, 65, 70, 32, 33);
    EXPECT(attn_strips(d) == 12 && attn_vtiles(d) == 2 && attn_kparts(d) == 2);
    EXPECT(attn_grid(d, 256, 0) == 12 && attn_grid(d, 256, 3) == 3 && attn_grid(d, 1, 0) == 8 && attn_grid(d, 0, 0) == 8);
    d.dv = 32; EXPECT(attn_kparts(d) == 4);
    d.dv = 96; EXPECT(attn_kparts(d) == 1);
    d.dv = 128; EXPECT(attn_kparts(d) == 1);
    d = dense(2, 3, 33, 37, 40, 35);
    const dfx_bmm_desc l = attn_bmm_logits(d), c = attn_bmm_context(d);
    const dfx_head_desc h = attn_head_softmax(d);
    EXPECT(bmm_validate(l, nullptr) == DFX_OK && bmm_validate(c, nullptr) == DFX_OK && head_validate(h, nullptr) == DFX_OK);
    EXPECT(l.ldc == 48 && l.c_s1 == 33 * 48 && l.c_s0 == 3 * 33 * 48 && c.lda == 48 && c.a_s1 == l.c_s1 && c.a_s0 == l.c_s0);
    EXPECT(h.rows == 6 * 33 && h.c == 37 && h.src_ld == 48 && h.dst_ld == 48 && h.src_dt == DFX_S8 && h.dst_dt == DFX_U8);
    EXPECT(attn_scratch_bytes(d) == 2ull * 6 * 33 * 48);
    EXPECT(attn_algorithmic_ops(d) == 2ull * 6 * 33 * 37 * 75);
    EXPECT(attn_algorithmic_bytes(d) == 6ull * (33 * 40 + 37 * 40 + 37 * 35 + 33 * 35));
    d.k_s0 = d.k_s1 = 0; d.dst_dt = DFX_F32;
    EXPECT(attn_algorithmic_bytes(d) == 6ull * 33 * 40 + 37 * 40 + 6ull * 37 * 35 + 6ull * 33 * 35 * 4);
  }
  if (g_bad) {
    printf("attn_plan_check: %d checks FAILED\n", g_bad);
    return 1;
  }
  printf("attn plans: validation order, the O-overlap rule, the 2^40 limits, the fused class, both routes' edges and grids hold\n");
  return 0;
}
