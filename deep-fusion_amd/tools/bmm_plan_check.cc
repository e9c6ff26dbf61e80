// bmm_plan_check -- host-only check of csrc/bmm_plan.h, what the batched matrix product (dfx_bmm_*) decides before a kernel
// runs: the descriptor's validation at the last admitted and the first refused value of every clause, in the header's order
// (INVALID before UNSUPPORTED), the C-overlap rule on the interleaved-heads layout, the 2^40 limit, the MFMA class, the
// fast route's proof at its edge, the grids under the cap and the algorithmic counts.  No HIP: it builds with SAN=1 (ASan +
// UBSan) and runs anywhere.
//   bmm_plan_check        the self-check
//   bmm_plan_check -      reads descriptors from stdin, one per line: the 13 int32 fields and the 9 strides in dfx_bmm_desc's
//                         order, then cus and cap; prints for each
//                         "rc class path tiles grid_mfma grid_generic lds_mfma ops bytes a_elems b_elems c_elems"
//                         (tests/test_bmm_cpu.py compares them with the Python mirror of tests/bmm_ref.py)
#include <cstdio>
#include <cstring>
#include <limits>

#include "../csrc/bmm_plan.h"

using namespace dfx;

static int g_bad = 0;
#define EXPECT(cond)                                                 \
  do {                                                               \
    if (!(cond)) {                                                   \
      printf("bmm_plan_check: line %d: %s\n", __LINE__, #cond);      \
      ++g_bad;                                                       \
    }                                                                \
  } while (0)

// densely packed {batch0, batch1} matrices, leading dimensions rounded up to 16
static dfx_bmm_desc dense(int b0, int b1, int m, int n, int k, int trans_b) {
  dfx_bmm_desc d;
  memset(&d, 0, sizeof(d));
  d.batch0 = b0; d.batch1 = b1; d.m = m; d.n = n; d.k = k; d.trans_b = trans_b;
  d.a_dt = DFX_U8; d.b_dt = DFX_S8; d.dst_dt = DFX_S8; d.round_mode = DFX_ROUND_NEAREST; d.nscales = 1; d.force_path = -1;
  const long long brows = trans_b ? n : k, bcols = trans_b ? k : n;
  d.lda = (k + 15) / 16 * 16; d.a_s1 = d.lda * m; d.a_s0 = d.a_s1 * b1;
  d.ldb = (bcols + 15) / 16 * 16; d.b_s1 = d.ldb * brows; d.b_s0 = d.b_s1 * b1;
  d.ldc = n; d.c_s1 = d.ldc * m; d.c_s0 = d.c_s1 * b1;
  return d;
}
static int rc(const dfx_bmm_desc &d) {
  const char *why = nullptr;
  const int r = bmm_validate(d, &why);
  EXPECT(why != nullptr && (r == DFX_OK) == (why[0] == 0));
  EXPECT(bmm_validate(d, nullptr) == r);
  return r;
}

static int from_stdin() {
  char line[1024];
  while (fgets(line, sizeof(line), stdin)) {
    long long v[24];
    int n = 0, pos = 0, adv = 0;
    while (n < 24 && sscanf(line + pos, "%lld%n", &v[n], &adv) == 1) {
      pos += adv;
      ++n;
    }
    if (n != 24) {
      printf("bad line\n");
      return 2;
    }
    dfx_bmm_desc d;
    memset(&d, 0, sizeof(d));
    d.batch0 = (int)v[0]; d.batch1 = (int)v[1]; d.m = (int)v[2]; d.n = (int)v[3]; d.k = (int)v[4]; d.trans_b = (int)v[5];
    d.a_dt = (int)v[6]; d.b_dt = (int)v[7]; d.dst_dt = (int)v[8]; d.relu = (int)v[9]; d.round_mode = (int)v[10]; d.nscales = (int)v[11];
    d.force_path = (int)v[12];
    d.a_s0 = v[13]; d.a_s1 = v[14]; d.lda = v[15]; d.b_s0 = v[16]; d.b_s1 = v[17]; d.ldb = v[18]; d.c_s0 = v[19]; d.c_s1 = v[20]; d.ldc = v[21];
    const int cus = (int)v[22];
    const long long cap = v[23];
    const int r = bmm_validate(d, nullptr);
    if (r == DFX_ERR_INVALID) {
      printf("%d\n", r);
      continue;
    }
    printf("%d %d %d %lld %d %d %d %llu %llu %llu %llu %llu\n", r, (int)bmm_mfma_class(d), r ? -1 : bmm_path(d), bmm_tiles(d),
           bmm_grid(d, DFX_BMM_MFMA, cus, cap), bmm_grid(d, DFX_BMM_GENERIC, cus, cap), bmm_lds_bytes(d, DFX_BMM_MFMA), bmm_algorithmic_ops(d),
           bmm_algorithmic_bytes(d), bmm_a_elems(d), bmm_b_elems(d), bmm_c_elems(d));
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 1 && strcmp(argv[1], "-") == 0) return from_stdin();
  const long long big = std::numeric_limits<long long>::max();
  // ---- sizes, K, enums: each at its last admitted and first refused value
  EXPECT(rc(dense(1, 1, 1, 1, 1, 1)) == DFX_OK);
  EXPECT(rc(dense(0, 1, 1, 1, 1, 1)) == DFX_ERR_INVALID && rc(dense(1, 0, 1, 1, 1, 1)) == DFX_ERR_INVALID);
  EXPECT(rc(dense(1, 1, 0, 1, 1, 1)) == DFX_ERR_INVALID && rc(dense(1, 1, 1, 0, 1, 1)) == DFX_ERR_INVALID && rc(dense(1, 1, 1, 1, 0, 1)) == DFX_ERR_INVALID);
  EXPECT(rc(dense(1, 1, 33, 33, 65025, 1)) == DFX_OK && rc(dense(1, 1, 33, 33, 65026, 1)) == DFX_ERR_INVALID);
  EXPECT(rc(dense(1, 1, 33, 33, 65025, 0)) == DFX_OK && rc(dense(1, 1, 33, 33, 65026, 0)) == DFX_ERR_INVALID);
  {  // m and n rounded up to 32 must fit an int
    dfx_bmm_desc d = dense(1, 1, 1, 16, 16, 1);
    d.n = 2147483647 - 31; d.ldc = d.n; EXPECT(rc(d) == DFX_OK);
    d.n = 2147483647 - 30; d.ldc = d.n; EXPECT(rc(d) == DFX_ERR_INVALID);
    d = dense(1, 1, 1, 16, 16, 1);
    d.m = 2147483647 - 31; EXPECT(rc(d) == DFX_OK);
    d.m = 2147483647 - 30; EXPECT(rc(d) == DFX_ERR_INVALID);
  }
  for (int v = -1; v <= 6; ++v) {
    dfx_bmm_desc d = dense(2, 3, 33, 37, 40, 1);
    d.trans_b = v; EXPECT(rc(d) == ((v == 0 || v == 1) ? DFX_OK : DFX_ERR_INVALID));
    d = dense(2, 3, 33, 37, 40, 1); d.a_dt = v; EXPECT(rc(d) == ((v == DFX_U8 || v == DFX_S8) ? DFX_OK : DFX_ERR_INVALID));
    d = dense(2, 3, 33, 37, 40, 1); d.b_dt = v;
    EXPECT(rc(d) == (v == DFX_S8 ? DFX_OK : v == DFX_U8 ? DFX_ERR_UNSUPPORTED : DFX_ERR_INVALID));
    d = dense(2, 3, 33, 37, 40, 1); d.dst_dt = v; EXPECT(rc(d) == ((v >= DFX_F32 && v <= DFX_U8) ? DFX_OK : DFX_ERR_INVALID));
    d = dense(2, 3, 33, 37, 40, 1); d.round_mode = v; EXPECT(rc(d) == ((v == 0 || v == 1) ? DFX_OK : DFX_ERR_INVALID));
    d = dense(2, 3, 33, 37, 40, 1); d.force_path = v; EXPECT(rc(d) == ((v >= -1 && v <= 1) ? DFX_OK : DFX_ERR_INVALID));
  }
  {
    dfx_bmm_desc d = dense(2, 3, 33, 37, 40, 1);
    d.nscales = 37; EXPECT(rc(d) == DFX_OK);
    d.nscales = 36; EXPECT(rc(d) == DFX_ERR_INVALID);
    d.nscales = 0; EXPECT(rc(d) == DFX_ERR_INVALID);
  }
  // ---- leading dimensions
  for (int t = 0; t <= 1; ++t) {
    dfx_bmm_desc d = dense(1, 1, 33, 37, 40, t);
    d.lda = 40; EXPECT(rc(d) == DFX_OK);
    d.lda = 39; EXPECT(rc(d) == DFX_ERR_INVALID);
    d = dense(1, 1, 33, 37, 40, t);
    d.ldb = t ? 40 : 37; EXPECT(rc(d) == DFX_OK);
    d.ldb = t ? 39 : 36; EXPECT(rc(d) == DFX_ERR_INVALID);
    d = dense(1, 1, 33, 37, 40, t);
    d.ldc = 37; EXPECT(rc(d) == DFX_OK);
    d.ldc = 36; EXPECT(rc(d) == DFX_ERR_INVALID);
  }
  // ---- strides: 0 broadcasts A or B, never C; negative never
  {
    dfx_bmm_desc d = dense(2, 3, 33, 37, 40, 1);
    d.a_s0 = 0; d.b_s1 = 0; EXPECT(rc(d) == DFX_OK);
    d.a_s1 = -1; EXPECT(rc(d) == DFX_ERR_INVALID);
    d = dense(2, 3, 33, 37, 40, 1); d.b_s0 = -16; EXPECT(rc(d) == DFX_ERR_INVALID);
    d = dense(2, 3, 33, 37, 40, 1); d.c_s0 = -1; EXPECT(rc(d) == DFX_ERR_INVALID);
    d = dense(2, 3, 33, 37, 40, 1); d.c_s1 = 0; EXPECT(rc(d) == DFX_ERR_INVALID);
    d = dense(2, 3, 33, 37, 40, 1); d.c_s0 = 0; EXPECT(rc(d) == DFX_ERR_INVALID);
    d = dense(1, 1, 33, 37, 40, 1); d.c_s0 = 0; d.c_s1 = 0; EXPECT(rc(d) == DFX_OK);  // extents of 1 are dropped
    d = dense(2, 3, 33, 37, 40, 1); d.c_s1 -= 1; EXPECT(rc(d) == DFX_ERR_INVALID);     // matrices one element too close
    d = dense(2, 3, 33, 37, 40, 1); d.c_s0 -= 1; EXPECT(rc(d) == DFX_ERR_INVALID);
    d = dense(2, 3, 33, 37, 40, 1); d.c_s0 += 1; EXPECT(rc(d) == DFX_OK);
  }
  // ---- interleaved heads: C written into {bs, T, heads * d}: N = d, c_s1 = d, ldc = heads * d, c_s0 = T * heads * d
  {
    const int bs = 2, heads = 3, T = 37, dd = 32;
    dfx_bmm_desc d = dense(bs, heads, T, dd, T, 0);
    d.ldc = heads * dd; d.c_s1 = dd; d.c_s0 = (long long)T * heads * dd;
    EXPECT(rc(d) == DFX_OK && bmm_c_disjoint(d));
    d.c_s1 = dd - 1; EXPECT(rc(d) == DFX_ERR_INVALID && !bmm_c_disjoint(d));
    d.c_s1 = dd; d.ldc = heads * dd - 1; EXPECT(rc(d) == DFX_ERR_INVALID);
    d.ldc = heads * dd; d.c_s0 -= 1; EXPECT(rc(d) == DFX_ERR_INVALID);
    d.c_s0 += 1; EXPECT(rc(d) == DFX_OK);
    EXPECT(bmm_c_elems(d) == (unsigned long long)((bs - 1) * d.c_s0 + (heads - 1) * dd + (T - 1) * d.ldc + dd));
  }
  // ---- the 2^40 limit on every operand; huge strides neither overflow nor pass
  {
    dfx_bmm_desc d = dense(2, 1, 1, 16, 16, 1);
    d.a_s0 = (1ll << 40) - 16 - 1; EXPECT(rc(d) == DFX_OK);     // last index 2^40 - 2
    d.a_s0 = (1ll << 40) - 16; EXPECT(rc(d) == DFX_ERR_INVALID);  // one past the last index reaches 2^40
    d = dense(2, 1, 1, 16, 16, 1); d.b_s0 = (1ll << 40) - 16 * 16 - 1; EXPECT(rc(d) == DFX_OK);
    d.b_s0 += 1; EXPECT(rc(d) == DFX_ERR_INVALID);
    d = dense(2, 1, 1, 16, 16, 1); d.c_s0 = (1ll << 40) - 16 - 1; EXPECT(rc(d) == DFX_OK);
    d.c_s0 += 1; EXPECT(rc(d) == DFX_ERR_INVALID);
    d = dense(2, 2, 2, 16, 16, 1); d.a_s0 = big; d.a_s1 = big; d.lda = big; EXPECT(rc(d) == DFX_ERR_INVALID);
    d = dense(2, 2, 2, 16, 16, 1); d.c_s0 = big; d.c_s1 = big / 2; d.ldc = big / 8; EXPECT(rc(d) == DFX_ERR_INVALID);
    d = dense(1, 1, 1, 16, 16, 1); d.a_s0 = big; d.b_s1 = big; d.c_s0 = big; EXPECT(rc(d) == DFX_OK);  // extents of 1: never used
    // all three strides of every operand near their limit at once: 1024 x 1024 matrices of 1024 rows, 2^30 / 2^20 / 2^10 apart;
    // the extents, tiles, items and grids at that range, and the overlap of operands of 2^40 elements
    d = dense(1024, 1024, 1024, 16, 16, 1);
    d.dst_dt = DFX_S32; d.force_path = DFX_BMM_MFMA;
    d.a_s0 = d.c_s0 = d.b_s0 = 1ll << 30; d.a_s1 = d.c_s1 = d.b_s1 = 1ll << 20; d.lda = d.ldc = 1ll << 10; d.ldb = 1ll << 16;
    EXPECT(rc(d) == DFX_OK && bmm_mfma_class(d) && bmm_c_disjoint(d));
    EXPECT(bmm_a_elems(d) == (1ull << 40) - 1024 + 16 && bmm_c_elems(d) == (1ull << 40) - 1024 + 16);
    EXPECT(bmm_b_elems(d) == 1023ull * (1ull << 30) + 1023ull * (1ull << 20) + 15ull * (1ull << 16) + 16);
    EXPECT(bmm_matrices(d) == 1ll << 20 && bmm_tiles(d) == 1ll << 25 && bmm_units(d) == 1ll << 23 && bmm_items(d) == 1ll << 34);
    EXPECT(bmm_grid(d, DFX_BMM_MFMA, 256, 0) == 4096 && bmm_grid(d, DFX_BMM_GENERIC, 256, 0) == 4096 && bmm_grid(d, DFX_BMM_MFMA, 256, 1ll << 40) == 4096);
    EXPECT(bmm_algorithmic_ops(d) == 1ull << 39 && bmm_algorithmic_bytes(d) == (1ull << 34) + (1ull << 28) + (1ull << 36));
    d.lda += 1008; d.ldc += 1008; EXPECT(rc(d) == DFX_ERR_INVALID);  // beyond 2^40 (the step keeps the class)
    d.ldc -= 1008; EXPECT(rc(d) == DFX_ERR_INVALID);
    d.lda -= 1008; d.c_s1 -= 1; EXPECT(rc(d) == DFX_ERR_INVALID);    // (C's matrices would meet)
    const uintptr_t far = (uintptr_t)1 << 47;
    const unsigned long long cb = 4 * ((1ull << 40) - 1024 + 16);
    EXPECT(plan_overlap(far, cb, far + cb - 1, 1) && !plan_overlap(far, cb, far + cb, 16) && !plan_overlap(far, cb, far - 16, 16) && plan_overlap(far, cb, far - 16, 17));
  }
  // ---- INVALID before UNSUPPORTED; the MFMA class
  {
    dfx_bmm_desc d = dense(2, 3, 33, 37, 40, 1);
    d.b_dt = DFX_U8; EXPECT(rc(d) == DFX_ERR_UNSUPPORTED);
    d.ldc = 36; EXPECT(rc(d) == DFX_ERR_INVALID);
    d = dense(2, 3, 33, 37, 40, 1); d.force_path = DFX_BMM_MFMA; EXPECT(rc(d) == DFX_OK && bmm_mfma_class(d) && bmm_path(d) == DFX_BMM_MFMA);
    int64_t *fields[6] = {&d.lda, &d.ldb, &d.a_s0, &d.a_s1, &d.b_s0, &d.b_s1};
    for (int i = 0; i < 6; ++i) {
      d = dense(2, 3, 33, 37, 40, 1); d.force_path = DFX_BMM_MFMA;
      *fields[i] += 8;
      EXPECT(!bmm_mfma_class(d) && rc(d) == DFX_ERR_UNSUPPORTED);
      d.force_path = DFX_BMM_GENERIC; EXPECT(rc(d) == DFX_OK && bmm_path(d) == DFX_BMM_GENERIC);
      d.force_path = -1; EXPECT(rc(d) == DFX_OK && bmm_path(d) == DFX_BMM_GENERIC);
      *fields[i] += 8;
      d.force_path = DFX_BMM_MFMA; EXPECT(bmm_mfma_class(d) && rc(d) == DFX_OK);
    }
    d = dense(2, 3, 33, 37, 40, 1); d.a_s0 = 0; d.b_s1 = 0; d.force_path = DFX_BMM_MFMA; EXPECT(rc(d) == DFX_OK);  // a broadcast is in the class
    d = dense(2, 3, 33, 37, 40, 1); EXPECT(bmm_path(d) == DFX_BMM_GENERIC);  // auto: below every measured size
    // the auto rule at its edges: the Swin window point and one less of each bound
    for (int t = 0; t <= 1; ++t) {
      d = dense(64, 3, 49, t ? 49 : 32, t ? 32 : 49, t); EXPECT(bmm_path(d) == DFX_BMM_MFMA);
      d = dense(64, 3, 48, t ? 49 : 32, t ? 32 : 49, t); EXPECT(bmm_path(d) == DFX_BMM_GENERIC);
      d = dense(63, 3, 49, t ? 49 : 32, t ? 32 : 49, t); EXPECT(bmm_path(d) == DFX_BMM_GENERIC);
      d = dense(64, 3, 49, t ? 49 : 32, t ? 32 : 49, t); d.lda += 8; EXPECT(bmm_path(d) == DFX_BMM_GENERIC);  // outside the class
    }
    d = dense(8, 12, 197, 197, 31, 1); EXPECT(bmm_path(d) == DFX_BMM_GENERIC);
    // few tiles under a deep K were never timed: 2 tiles with K = 65025 pass the multiply-add bound and stay generic
    d = dense(1, 1, 49, 32, 65025, 1); EXPECT(bmm_path(d) == DFX_BMM_GENERIC);
    d = dense(1, 1, 49, 32, 65025, 0); EXPECT(bmm_path(d) == DFX_BMM_GENERIC);
    d = dense(1, 1, 32 * 12, 32 * 32, 4096, 1); EXPECT(bmm_tiles(d) == 384 && bmm_path(d) == DFX_BMM_MFMA);
    d = dense(1, 1, 32 * 12, 32 * 32 - 32, 4096, 1); EXPECT(bmm_tiles(d) == 372 && bmm_path(d) == DFX_BMM_GENERIC);
    d = dense(64, 3, 49, 32, 49, 0); EXPECT(bmm_tiles(d) == 384);  // the Swin P.V point itself
    d = dense(8, 12, 197, 31, 197, 0); EXPECT(bmm_path(d) == DFX_BMM_GENERIC);
    d = dense(8, 12, 197, 197, 64, 1); EXPECT(bmm_path(d) == DFX_BMM_MFMA);
  }
  // ---- the fast route's proof: bound * |scale| <= 2^30 at its edge
  {
    dfx_bmm_desc d = dense(1, 1, 33, 37, 64, 1);  // u8 A: bound = 255 * 128 * 64 = 2088960
    EXPECT(bmm_acc_bound(d) == 2088960.0);
    float s = 514.0f;  // 2^30 / 2088960 = 514.008...
    EXPECT(bmm_fast_ok(d, &s));
    s = 514.01f; EXPECT(!bmm_fast_ok(d, &s));
    s = -514.0f; EXPECT(bmm_fast_ok(d, &s));
    s = std::numeric_limits<float>::infinity(); EXPECT(!bmm_fast_ok(d, &s));
    s = std::numeric_limits<float>::quiet_NaN(); EXPECT(!bmm_fast_ok(d, &s));
    s = 1.0f; d.round_mode = DFX_ROUND_DOWN; EXPECT(!bmm_fast_ok(d, &s));
    d.round_mode = DFX_ROUND_NEAREST; d.a_dt = DFX_S8;  // bound = 128 * 128 * 64 = 2^20: the edge is exactly 1024
    EXPECT(bmm_acc_bound(d) == 1048576.0);
    s = 1024.0f; EXPECT(bmm_fast_ok(d, &s));
    s = 1024.0001f; EXPECT(!bmm_fast_ok(d, &s));
    d.nscales = 37;
    float sc[37];
    for (int i = 0; i < 37; ++i) sc[i] = 1.0f;
    EXPECT(bmm_fast_ok(d, sc));
    sc[36] = 1025.0f; EXPECT(!bmm_fast_ok(d, sc));
    d = dense(1, 1, 33, 33, 65025, 1); s = 1.0f;  // the largest K: 255 * 128 * 65025 > 2^30 even at scale 1
    EXPECT(!bmm_fast_ok(d, &s));
    s = 0.5f; EXPECT(bmm_fast_ok(d, &s));
  }
  // ---- tiles, grids under the cap, LDS, counts
  {
    dfx_bmm_desc d = dense(1, 2, 70, 130, 96, 1);
    EXPECT(bmm_tiles(d) == 2 * 3 * 5 && bmm_units(d) == 8);
    EXPECT(bmm_grid(d, DFX_BMM_MFMA, 256, 0) == 8 && bmm_grid(d, DFX_BMM_MFMA, 256, 3) == 3 && bmm_grid(d, DFX_BMM_MFMA, 256, 1) == 1);
    EXPECT(bmm_grid(d, DFX_BMM_GENERIC, 256, 0) == (2 * 70 * 130 + 255) / 256 && bmm_grid(d, DFX_BMM_GENERIC, 1, 0) == 16);
    EXPECT(bmm_lds_bytes(d, DFX_BMM_MFMA) == 0 && bmm_lds_bytes(d, DFX_BMM_GENERIC) == 0);
    EXPECT(bmm_algorithmic_ops(d) == 2ull * 2 * 70 * 130 * 96);
    EXPECT(bmm_algorithmic_bytes(d) == 2ull * 70 * 96 + 2ull * 130 * 96 + 2ull * 70 * 130);
    d.b_s1 = 0; EXPECT(bmm_algorithmic_bytes(d) == 2ull * 70 * 96 + 130 * 96 + 2ull * 70 * 130);
    d.dst_dt = DFX_F32; EXPECT(bmm_algorithmic_bytes(d) == 2ull * 70 * 96 + 130 * 96 + 4 * 2ull * 70 * 130);
    d = dense(1, 2, 70, 130, 96, 0);
    EXPECT(bmm_lds_bytes(d, DFX_BMM_MFMA) == BMM_NN_LDS && BMM_NN_LDS == 12288);
    d = dense(65535, 65535, 1, 1, 1, 1);
    EXPECT(rc(d) == DFX_OK && bmm_grid(d, DFX_BMM_MFMA, 256, 0) == 256 * BMM_GRID_PER_CU);
    EXPECT(plan_overlap(100, 10, 109, 1) && !plan_overlap(100, 10, 110, 1) && !plan_overlap(110, 1, 100, 10));
  }
  if (g_bad) {
    printf("bmm_plan_check: %d checks failed\n", g_bad);
    return 1;
  }
  printf("bmm plans: validation order, the C-overlap rule, the 2^40 limit, classes, the route's edge and grids hold\n");
  return 0;
}
