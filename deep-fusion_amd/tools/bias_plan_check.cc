// bias_plan_check -- host-only check of csrc/bias_plan.h, what the logit bias of dfx_bmm / dfx_attn (dfx_logit_bias_desc)
// decides before a kernel runs: the layout's validation at the last admitted and the first refused value of every clause
// (INVALID before UNSUPPORTED), the host extent, the device image and its index function against a direct gather, the zero
// pads, the scan (max |finite|, -inf found, +inf / NaN refused, gaps never read), the distinct bytes and the biased route
// proof at its edge.  No HIP: it builds with SAN=1 (ASan + UBSan) and runs anywhere.
//   bias_plan_check        the self-check
//   bias_plan_check -      reads one layout per line from stdin: batch0 batch1 m n k a_dt round_mode nscales, then period0
//                          period1 s0 s1 ld, then max_abs has_ninf scale (the scan's result and ONE scale used for every
//                          channel); prints "rc host_elems rows cols image_elems distinct_bytes fast" (only rc where it is
//                          DFX_ERR_INVALID) (tests/test_attn_bias_cpu.py compares them with the mirror of tests/attn_bias_ref.py)
//   bias_plan_check scan   reads "period0 period1 s0 s1 ld m n count" and then `count` floats (inf, -inf, nan allowed) from
//                          stdin; prints "rc max_abs has_ninf" and the image's floats, one line per image row
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../csrc/bias_plan.h"

using namespace dfx;

static int g_bad = 0;
#define EXPECT(cond)                                                 \
  do {                                                               \
    if (!(cond)) {                                                   \
      printf("bias_plan_check: line %d: %s\n", __LINE__, #cond);     \
      ++g_bad;                                                       \
    }                                                                \
  } while (0)

// densely packed {b0, b1} NT matrices, s8 x s8 -> s8
static dfx_bmm_desc dense(int b0, int b1, int m, int n, int k) {
  dfx_bmm_desc d;
  memset(&d, 0, sizeof(d));
  d.batch0 = b0; d.batch1 = b1; d.m = m; d.n = n; d.k = k; d.trans_b = 1;
  d.a_dt = DFX_S8; d.b_dt = DFX_S8; d.dst_dt = DFX_S8; d.round_mode = DFX_ROUND_NEAREST; d.nscales = 1; d.force_path = -1;
  d.lda = (k + 15) / 16 * 16; d.a_s1 = d.lda * m; d.a_s0 = d.a_s1 * b1;
  d.ldb = d.lda; d.b_s1 = d.ldb * n; d.b_s0 = d.b_s1 * b1;
  d.ldc = n; d.c_s1 = d.ldc * m; d.c_s0 = d.c_s1 * b1;
  return d;
}
static dfx_logit_bias_desc layout(int p0, int p1, long long s0, long long s1, long long ld) {
  dfx_logit_bias_desc b;
  b.period0 = p0; b.period1 = p1; b.s0 = s0; b.s1 = s1; b.ld = ld;
  return b;
}
static int rc(const dfx_bmm_desc &d, const dfx_logit_bias_desc &b) {
  const char *why = nullptr;
  const int r = bias_validate(d, b, &why);
  EXPECT(why != nullptr && (r == DFX_OK) == (why[0] == 0));
  EXPECT(bias_validate(d, b, nullptr) == r);
  return r;
}

static int from_stdin() {
  char line[1024];
  while (fgets(line, sizeof(line), stdin)) {
    long long v[13];
    double max_abs = 0, scale = 0;
    int ninf = 0, pos = 0, adv = 0;
    bool ok = true;
    for (int i = 0; i < 13 && ok; ++i) ok = sscanf(line + pos, "%lld%n", &v[i], &adv) == 1, pos += adv;
    if (ok) ok = sscanf(line + pos, "%lf %d %lf", &max_abs, &ninf, &scale) == 3;
    if (!ok) {
      printf("bad line\n");
      return 2;
    }
    dfx_bmm_desc d = dense((int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4]);
    d.a_dt = (int)v[5]; d.round_mode = (int)v[6]; d.nscales = (int)v[7];
    if (bmm_validate(d, nullptr) != DFX_OK) {
      printf("bad descriptor\n");
      return 2;
    }
    const dfx_logit_bias_desc b = layout((int)v[8], (int)v[9], v[10], v[11], v[12]);
    const int r = bias_validate(d, b, nullptr);
    if (r == DFX_ERR_INVALID) {
      printf("%d\n", r);
      continue;
    }
    BiasScan s;
    s.max_abs = max_abs;
    s.has_ninf = ninf != 0;
    const std::vector<float> scales((size_t)d.nscales, (float)scale);
    printf("%d %llu %lld %lld %llu %llu %d\n", r, bias_host_elems(d, b), bias_rows(d, b), bias_cols(d), bias_image_elems(d, b), bias_distinct_bytes(d, b),
           (int)bmm_fast_ok_biased(d, scales.data(), s));
  }
  return 0;
}

static int scan_stdin() {
  long long p0, p1, s0, s1, ld, m, n, count;
  if (scanf("%lld %lld %lld %lld %lld %lld %lld %lld", &p0, &p1, &s0, &s1, &ld, &m, &n, &count) != 8) return 2;
  const dfx_bmm_desc d = dense((int)p0, (int)p1, (int)m, (int)n, 16);
  const dfx_logit_bias_desc b = layout((int)p0, (int)p1, s0, s1, ld);
  if (bmm_validate(d, nullptr) != DFX_OK || bias_validate(d, b, nullptr) != DFX_OK || (unsigned long long)count != bias_host_elems(d, b)) return 2;
  std::vector<float> t((size_t)count);  // (exactly the extent: a read beyond it is the sanitizer's to find)
  for (long long i = 0; i < count; ++i) {
    char w[64];
    if (scanf("%63s", w) != 1) return 2;
    t[(size_t)i] = strtof(w, nullptr);
  }
  BiasScan s;
  const int r = bias_scan(d, b, t.data(), &s);
  printf("%d %.9g %d\n", r, s.max_abs, (int)s.has_ninf);
  if (r != DFX_OK) return 0;
  std::vector<float> img((size_t)bias_image_elems(d, b), -7.0f);
  bias_fill_image(d, b, t.data(), img.data());
  const long long cols = bias_cols(d);
  for (size_t i = 0; i < img.size(); ++i) printf("%.9g%c", img[i], (long long)(i + 1) % cols == 0 ? '\n' : ' ');
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 1 && strcmp(argv[1], "-") == 0) return from_stdin();
  if (argc > 1 && strcmp(argv[1], "scan") == 0) return scan_stdin();
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  // ---- validation: each clause at its last admitted and first refused value
  {
    const dfx_bmm_desc d = dense(4, 3, 33, 37, 40);
    EXPECT(rc(d, layout(1, 1, 0, 0, 37)) == DFX_OK && rc(d, layout(4, 3, 3 * 33 * 37, 33 * 37, 37)) == DFX_OK);
    EXPECT(rc(d, layout(0, 1, 0, 0, 37)) == DFX_ERR_INVALID && rc(d, layout(5, 1, 0, 0, 37)) == DFX_ERR_INVALID);
    EXPECT(rc(d, layout(1, 0, 0, 0, 37)) == DFX_ERR_INVALID && rc(d, layout(1, 4, 0, 0, 37)) == DFX_ERR_INVALID);
    EXPECT(rc(d, layout(2, 3, 0, 0, 37)) == DFX_OK);                       // a period that does not divide the batch is fine; overlapping tables too
    EXPECT(rc(d, layout(3, 2, 1, 1, 0)) == DFX_OK);
    EXPECT(rc(d, layout(1, 1, -1, 0, 37)) == DFX_ERR_INVALID && rc(d, layout(1, 1, 0, -1, 37)) == DFX_ERR_INVALID && rc(d, layout(1, 1, 0, 0, -1)) == DFX_ERR_INVALID);
    EXPECT(rc(d, layout(1, 1, 0, 0, 0)) == DFX_OK && rc(d, layout(1, 1, 0, 0, 36)) == DFX_ERR_INVALID && rc(d, layout(1, 1, 0, 0, 1)) == DFX_ERR_INVALID);
    // the host extent: below 2^40 floats
    const long long span = 32ll * 37 + 37;
    EXPECT(rc(d, layout(2, 1, (1ll << 40) - 1 - span, 0, 37)) == DFX_OK && rc(d, layout(2, 1, (1ll << 40) - span, 0, 37)) == DFX_ERR_INVALID);
    EXPECT(rc(d, layout(2, 2, 1ll << 62, 1ll << 62, 37)) == DFX_ERR_INVALID);
    EXPECT(bias_host_elems(d, layout(4, 3, 5000, 1500, 40)) == 3ull * 5000 + 2 * 1500 + 32 * 40 + 37);
    EXPECT(bias_host_elems(d, layout(4, 3, 100, 40, 0)) == 3ull * 100 + 2 * 40 + 37);
  }
  // ---- the image: {tables, m or 1, up32(n)}, at most 2^30 bytes
  {
    const dfx_bmm_desc d = dense(4, 3, 33, 37, 40);
    EXPECT(bias_cols(d) == 64 && bias_rows(d, layout(1, 1, 0, 0, 37)) == 33 && bias_rows(d, layout(1, 1, 0, 0, 0)) == 1);
    EXPECT(bias_image_elems(d, layout(4, 3, 0, 0, 37)) == 12ull * 33 * 64 && bias_image_bytes(d, layout(2, 1, 0, 0, 0)) == 2ull * 64 * 4);
    EXPECT(bias_cols(dense(1, 1, 1, 32, 16)) == 32 && bias_cols(dense(1, 1, 1, 33, 16)) == 64 && bias_cols(dense(1, 1, 1, 1, 16)) == 32);
    dfx_bmm_desc big = dense(1, 1, 8192, 32768, 16);                       // 8192 x 32768 x 4 bytes = 2^30
    EXPECT(bmm_validate(big, nullptr) == DFX_OK && rc(big, layout(1, 1, 0, 0, 32768)) == DFX_OK);
    big = dense(1, 1, 8193, 32768, 16);
    EXPECT(bmm_validate(big, nullptr) == DFX_OK && rc(big, layout(1, 1, 0, 0, 32768)) == DFX_ERR_UNSUPPORTED && rc(big, layout(1, 1, 0, 0, 0)) == DFX_OK);
    EXPECT(rc(big, layout(1, 1, 0, 0, 32767)) == DFX_ERR_INVALID);         // INVALID is found before UNSUPPORTED
    big = dense(2, 1, 8192, 32768, 16);
    EXPECT(rc(big, layout(2, 1, 0, 0, 32768)) == DFX_ERR_UNSUPPORTED && rc(big, layout(1, 1, 0, 0, 32768)) == DFX_OK);
    // distinct bytes: a period under a stride of 0 addresses one table
    EXPECT(bias_distinct_bytes(d, layout(4, 3, 5000, 1500, 40)) == 12ull * 33 * 37 * 4 && bias_distinct_bytes(d, layout(4, 3, 0, 1500, 40)) == 3ull * 33 * 37 * 4);
    EXPECT(bias_distinct_bytes(d, layout(4, 1, 37, 0, 0)) == 4ull * 37 * 4);
  }
  // ---- fill and index against a direct gather; pads zero; gaps (NaN) never read
  for (int variant = 0; variant < 4; ++variant) {
    const dfx_bmm_desc d = dense(4, 3, 5, 37, 16);
    const dfx_logit_bias_desc b = variant == 0 ? layout(2, 3, 3 * 5 * 37, 5 * 37, 37) : variant == 1 ? layout(2, 3, 1000, 300, 41)
                                  : variant == 2 ? layout(4, 1, 50, 0, 0) : layout(1, 2, 0, 37, 0);
    EXPECT(rc(d, b) == DFX_OK);
    std::vector<float> t((size_t)bias_host_elems(d, b), nan);
    const long long rows = bias_rows(d, b), cols = bias_cols(d);
    for (int p0 = 0; p0 < b.period0; ++p0)
      for (int p1 = 0; p1 < b.period1; ++p1)
        for (long long m = 0; m < rows; ++m)
          for (int n = 0; n < d.n; ++n) t[bias_host_index(b, p0, p1, m, n)] = (float)(1000 * p0 + 100 * p1 + 10 * m) + 0.25f * n;
    BiasScan s;
    EXPECT(bias_scan(d, b, t.data(), &s) == DFX_OK && !s.has_ninf);
    EXPECT(s.max_abs == 1000.0 * (b.period0 - 1) + 100.0 * (b.period1 - 1) + 10.0 * (rows - 1) + 0.25 * 36);
    std::vector<float> img((size_t)bias_image_elems(d, b), nan);
    bias_fill_image(d, b, t.data(), img.data());
    for (int b0 = 0; b0 < d.batch0; ++b0)
      for (int b1 = 0; b1 < d.batch1; ++b1)
        for (int m = 0; m < d.m; ++m)
          for (int n = 0; n < cols; ++n) {
            const size_t i = bias_image_index(b.period0, b.period1, rows, cols, b0, b1, m, n);
            EXPECT(i < img.size());
            if (i >= img.size()) continue;
            const float want = n < d.n ? (float)(1000 * (b0 % b.period0) + 100 * (b1 % b.period1) + 10 * (rows == 1 ? 0 : m)) + 0.25f * n : 0.0f;
            EXPECT(img[i] == want);
          }
  }
  // ---- the scan: -inf found, +inf and NaN refused wherever they stand
  {
    const dfx_bmm_desc d = dense(2, 2, 3, 5, 16);
    const dfx_logit_bias_desc b = layout(2, 2, 30, 15, 5);
    std::vector<float> t((size_t)bias_host_elems(d, b), 1.5f);
    BiasScan s;
    t[bias_host_index(b, 1, 1, 2, 4)] = -inf;
    t[bias_host_index(b, 0, 1, 1, 0)] = -2.5e9f;
    EXPECT(bias_scan(d, b, t.data(), &s) == DFX_OK && s.has_ninf && s.max_abs == (double)-(-2.5e9f));
    for (int where = 0; where < 2; ++where)
      for (int what = 0; what < 2; ++what) {
        std::vector<float> u = t;
        u[where ? bias_host_index(b, 1, 1, 2, 4) : 0] = what ? nan : inf;
        EXPECT(bias_scan(d, b, u.data(), nullptr) == DFX_ERR_INVALID);
      }
  }
  // ---- the biased route proof: (bound + max |bias|) * |scale| <= 2^30, no -inf, nearest rounding, finite scales
  {
    dfx_bmm_desc d = dense(1, 1, 33, 64, 64);                              // s8 A: bound 128 * 128 * 64 = 2^20
    BiasScan s;
    float sc = 512.0f;
    s.max_abs = 1048576.0; EXPECT(bmm_fast_ok_biased(d, &sc, s));          // (2^20 + 2^20) * 2^9 = 2^30
    s.max_abs = 1048577.0; EXPECT(!bmm_fast_ok_biased(d, &sc, s));
    s.max_abs = 0.0; sc = 1024.0f; EXPECT(bmm_fast_ok_biased(d, &sc, s) && bmm_fast_ok(d, &sc));
    s.max_abs = 1.0; EXPECT(!bmm_fast_ok_biased(d, &sc, s));
    sc = -512.0f; s.max_abs = 1048576.0; EXPECT(bmm_fast_ok_biased(d, &sc, s));
    s.has_ninf = true; s.max_abs = 0.0; sc = 1.0f; EXPECT(!bmm_fast_ok_biased(d, &sc, s));
    s.has_ninf = false; sc = inf; EXPECT(!bmm_fast_ok_biased(d, &sc, s));
    sc = nan; EXPECT(!bmm_fast_ok_biased(d, &sc, s));
    sc = 1.0f; d.round_mode = DFX_ROUND_DOWN; EXPECT(!bmm_fast_ok_biased(d, &sc, s));
    d.round_mode = DFX_ROUND_NEAREST; d.a_dt = DFX_U8; sc = 256.0f; s.max_abs = 2097152.0 + 8192.0;   // bound 255 * 2^13
    EXPECT(bmm_fast_ok_biased(d, &sc, s));
    s.max_abs += 1.0; EXPECT(!bmm_fast_ok_biased(d, &sc, s));
  }
  if (g_bad) {
    printf("bias_plan_check: %d checks FAILED\n", g_bad);
    return 1;
  }
  printf("bias plans: validation order, the host extent, the image and its index, the scan and the biased route's edge hold\n");
  return 0;
}
