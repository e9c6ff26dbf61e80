// lnorm_plan_check -- host-only check of csrc/lnorm_plan.h, what the int8 layer norm / RMS norm (dfx_lnorm_*) decides before
// a kernel runs: the order of the descriptor's validation (every DFX_ERR_INVALID before the one DFX_ERR_UNSUPPORTED) at the
// last admitted and the first refused value of every bound, the bounds of the integer statistics recomputed at c = 16384 with
// shift 7, the class and auto predicates, the lanes per row at every switch, the grids under the cap, the LDS plan, the
// extents the overlap check uses and the 2^40 limit.  No HIP: it builds with SAN=1 (ASan + UBSan) and runs anywhere.
//   lnorm_plan_check
#include <cstdio>
#include <cstring>
#include <vector>

#include "../csrc/lnorm_plan.h"

using namespace dfx;

static int g_bad = 0;
#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      printf("lnorm_plan_check: line %d: %s\n", __LINE__, #cond);     \
      ++g_bad;                                                        \
    }                                                                 \
  } while (0)

static dfx_lnorm_desc desc(long long rows, int c, int src_ld, int dst_ld, int src_dt = DFX_S8, int dst_dt = DFX_S8, int mode = DFX_LNORM_LAYER) {
  dfx_lnorm_desc d;
  memset(&d, 0, sizeof(d));
  d.rows = rows; d.mode = mode; d.src_dt = src_dt; d.dst_dt = dst_dt; d.c = c; d.src_ld = src_ld; d.dst_ld = dst_ld;
  d.eps = 1e-3f; d.force_path = -1;
  return d;
}
static int rc(const dfx_lnorm_desc &d, const char **why_out = nullptr) {
  const char *why = nullptr;
  const int r = lnorm_validate(d, &why);
  EXPECT(why != nullptr && (r == DFX_OK) == (why[0] == 0));
  EXPECT(lnorm_validate(d, nullptr) == r);
  if (why_out) *why_out = why;
  return r;
}
static float bits_f(unsigned b) {
  float f;
  memcpy(&f, &b, 4);
  return f;
}

int main() {
  // ---- validation, each bound at its last admitted and first refused value
  EXPECT(rc(desc(1, 1, 1, 1)) == DFX_OK);
  EXPECT(rc(desc(0, 1, 1, 1)) == DFX_ERR_INVALID && rc(desc(-1, 1, 1, 1)) == DFX_ERR_INVALID);
  EXPECT(rc(desc(4, 0, 16, 16)) == DFX_ERR_INVALID);
  EXPECT(rc(desc(4, 16384, 16384, 16384)) == DFX_OK && rc(desc(4, 16385, 16400, 16400)) == DFX_ERR_INVALID);
  EXPECT(rc(desc(4, 96, 95, 96)) == DFX_ERR_INVALID && rc(desc(4, 96, 96, 95)) == DFX_ERR_INVALID && rc(desc(4, 96, 97, 101)) == DFX_OK);
  for (int dt : {(int)DFX_UNDEF, (int)DFX_F32, (int)DFX_S32, 5, -1}) EXPECT(rc(desc(4, 96, 96, 96, dt, DFX_S8)) == DFX_ERR_INVALID);
  for (int dt : {(int)DFX_UNDEF, (int)DFX_S32, 5, -1}) EXPECT(rc(desc(4, 96, 96, 96, DFX_S8, dt)) == DFX_ERR_INVALID);
  for (int s : {(int)DFX_S8, (int)DFX_U8})
    for (int o : {(int)DFX_S8, (int)DFX_U8, (int)DFX_F32}) EXPECT(rc(desc(4, 96, 96, 96, s, o)) == DFX_OK);
  for (int m = -2; m <= 3; ++m) EXPECT(rc(desc(4, 96, 96, 96, DFX_S8, DFX_S8, m)) == ((m == 0 || m == 1) ? DFX_OK : DFX_ERR_INVALID));
  {
    dfx_lnorm_desc d = desc(4, 96, 96, 96);
    for (int p = -3; p <= 3; ++p) {
      d.force_path = p;
      EXPECT(rc(d) == ((p >= -1 && p <= 1) ? DFX_OK : DFX_ERR_INVALID));
    }
    d.force_path = -1;
    const struct { unsigned bits; bool ok; } eps[] = {{0x00000001u, true}, {0x7f7fffffu, true}, {0x00000000u, false}, {0x80000000u, false},
                                                       {0x80000001u, false}, {0xbf800000u, false}, {0x7f800000u, false}, {0xff800000u, false},
                                                       {0x7fc00000u, false}, {0xffc00001u, false}, {0x3f800000u, true}};
    for (const auto &e : eps) {
      d.eps = bits_f(e.bits);
      EXPECT((rc(d) == DFX_OK) == e.ok);
    }
  }
  // ---- the order: with faults i and j > i the reason is i's; the forced path's class comes after everything invalid
  {
    struct Fault { const char *word; void (*set)(dfx_lnorm_desc &); };
    const Fault faults[] = {
        {"mode", [](dfx_lnorm_desc &d) { d.mode = 7; }},
        {"rows", [](dfx_lnorm_desc &d) { d.rows = 0; }},
        {"c must", [](dfx_lnorm_desc &d) { d.c = 0; }},
        {"src dtype", [](dfx_lnorm_desc &d) { d.src_dt = DFX_F32; }},
        {"dst dtype", [](dfx_lnorm_desc &d) { d.dst_dt = DFX_S32; }},
        {"src_ld", [](dfx_lnorm_desc &d) { d.src_ld = d.c - 1; }},
        {"dst_ld", [](dfx_lnorm_desc &d) { d.dst_ld = d.c - 1; }},
        {"eps", [](dfx_lnorm_desc &d) { d.eps = 0.0f; }},
        {"force_path", [](dfx_lnorm_desc &d) { d.force_path = 2; }},
        {"2^40", [](dfx_lnorm_desc &d) { d.rows = 1ll << 40; }},
    };
    const int n = (int)(sizeof(faults) / sizeof(faults[0]));
    for (int i = 0; i < n; ++i)
      for (int j = i; j < n; ++j) {
        if ((i == 1 && j == 9) || (i == 2 && (j == 5 || j == 6))) continue;  // (the same field, or a bound that follows c)
        dfx_lnorm_desc d = desc(4, 100, 100, 100);
        d.force_path = DFX_LNORM_ROW;  // outside the row class as well: never reported while something is invalid
        faults[j].set(d);
        faults[i].set(d);
        if (j == 8) d.force_path = 2;
        const char *why = "";
        EXPECT(rc(d, &why) == DFX_ERR_INVALID && strstr(why, faults[i].word) != nullptr);
      }
    dfx_lnorm_desc d = desc(4, 100, 100, 100);
    d.force_path = DFX_LNORM_ROW;
    EXPECT(rc(d) == DFX_OK && !lnorm_in_class(d, d.force_path));  // lnorm_create turns this into DFX_ERR_UNSUPPORTED
  }
  // ---- the 2^40 limit: rows * max(src_ld, dst_ld), no product formed before it is known to fit
  EXPECT(rc(desc(1ll << 36, 16, 16, 16)) == DFX_OK && rc(desc((1ll << 36) + 1, 16, 16, 16)) == DFX_ERR_INVALID);
  EXPECT(rc(desc(1ll << 35, 16, 16, 32)) == DFX_OK && rc(desc((1ll << 35) + 1, 16, 16, 32)) == DFX_ERR_INVALID);
  EXPECT(rc(desc(1ll << 35, 16, 32, 16)) == DFX_OK && rc(desc((1ll << 35) + 1, 16, 32, 16)) == DFX_ERR_INVALID);
  EXPECT(rc(desc(1ll << 40, 1, 1, 1)) == DFX_OK && rc(desc((1ll << 40) + 1, 1, 1, 1)) == DFX_ERR_INVALID);
  EXPECT(rc(desc(0x7fffffffffffffffll, 1, 0x7fffffff, 1)) == DFX_ERR_INVALID);
  // ---- the bounds of include/dfx.h at c = 16384 with shift 7, recomputed here in 64-bit integers
  {
    const long long c = DFX_LNORM_MAX_C;
    long long S = 0, Sa = 0;
    unsigned long long Q = 0, Qa = 0;
    long long tmax = 0, umax = 0;
    for (long long k = 0; k < c; ++k) {
      const long long t = 255ll << DFX_LNORM_MAX_SHIFT;                     // all 255 u8: the largest |S| and Q
      const long long ta = (k % 2 ? 127ll : -128ll) * (1ll << DFX_LNORM_MAX_SHIFT);  // alternating s8 extremes: the largest u_k of s8
      S += t; Q += (unsigned long long)(t * t);
      Sa += ta; Qa += (unsigned long long)(ta * ta);
      tmax = t > tmax ? t : tmax;
    }
    EXPECT(tmax == LNORM_MAX_T && S == LNORM_MAX_S && Q == LNORM_MAX_Q);
    EXPECT(S < (1ll << 30) && Q < (1ull << 44));
    EXPECT((unsigned long long)c * Q < (1ull << 58) && (unsigned long long)c * Q - (unsigned long long)(S * S) == 0);   // a constant row: D = 0
    const unsigned long long Da = (unsigned long long)c * Qa - (unsigned long long)(Sa * Sa);
    EXPECT(Da < (1ull << 58) && Da > 0);
    for (long long t : {-128ll * 128, 127ll * 128}) {
      const long long u = c * t - Sa;
      umax = (u < 0 ? -u : u) > umax ? (u < 0 ? -u : u) : umax;
    }
    // the largest |u_k| of all: one element at 0 among 255 << 7 (S just below its maximum, c * t_k = 0), and its mirror
    const long long u0 = c * 0 - (S - LNORM_MAX_T), u1 = c * LNORM_MAX_T - LNORM_MAX_T;
    EXPECT(umax < (1ll << 31) && -u0 < (1ll << 31) && u1 < (1ll << 31) && c * LNORM_MAX_T + LNORM_MAX_S < (1ll << 31));
    EXPECT(c * c < (1ll << 31) && (long long)(float)c == c);
    EXPECT((unsigned long long)c * 255 * 255 < (1ull << 32));
  }
  // ---- class, auto, lanes
  for (int dst_dt : {(int)DFX_S8, (int)DFX_U8, (int)DFX_F32})
    for (int sld = 96; sld <= 130; ++sld)
      for (int dld = 96; dld <= 130; ++dld) {
        const dfx_lnorm_desc d = desc(7, 96, sld, dld, DFX_S8, dst_dt);
        const int es = plan_dt_size(dst_dt);
        EXPECT(lnorm_row_class(d) == (sld % 16 == 0 && (dld * es) % 16 == 0));
        EXPECT(lnorm_in_class(d, DFX_LNORM_GENERIC) && lnorm_in_class(d, DFX_LNORM_ROW) == lnorm_row_class(d) && !lnorm_in_class(d, 2));
        // the auto rule: the row kernel only in its class and only where lnorm_row_auto() admits the point
        EXPECT(lnorm_path(d) == (lnorm_row_class(d) && lnorm_row_auto(d) ? DFX_LNORM_ROW : DFX_LNORM_GENERIC));
        dfx_lnorm_desc f = d;
        for (int p = 0; p < 2; ++p) {
          f.force_path = p;
          EXPECT(lnorm_path(f) == p);
        }
      }
  EXPECT(lnorm_row_class(desc(3, 100, 112, 100, DFX_S8, DFX_F32)) && !lnorm_row_class(desc(3, 100, 112, 100, DFX_S8, DFX_S8)));
  {
    const struct { int c, w; } lanes[] = {{1, 4}, {16, 4}, {64, 4}, {65, 8}, {96, 8}, {128, 8}, {129, 16}, {144, 16}, {256, 16}, {257, 32}, {512, 32},
                                          {513, 64}, {768, 64}, {1024, 64}, {1025, 64}, {4096, 64}, {4097, 64}, {16384, 64}};
    for (const auto &l : lanes) EXPECT(lnorm_lanes(l.c) == l.w);
    for (int c = 1; c <= DFX_LNORM_MAX_C; ++c) {
      const int w = lnorm_lanes(c), groups = (c + 15) / 16;
      EXPECT((w == 4 || w == 8 || w == 16 || w == 32 || w == 64) && (w >= groups || w == 64) && (w == 4 || w / 2 < groups));
    }
  }
  // ---- grids, LDS, parameter image
  for (long long rows : {1ll, 3ll, 4ll, 5ll, 63ll, 64ll, 65ll, 255ll, 256ll, 257ll, 1ll << 20, 1ll << 40})
    for (long long cap : {0ll, 1ll, 3ll, 5000ll})
      for (int c : {1, 96, 200, 400, 768})
        for (int p = 0; p < 2; ++p) {
          const int per = p == DFX_LNORM_ROW ? 256 / lnorm_lanes(c) : 256;
          const int g = lnorm_grid(rows, c, p, cap);
          long long want = (rows + per - 1) / per;
          if (want > LNORM_MAX_BLOCKS) want = LNORM_MAX_BLOCKS;
          if (cap > 0 && want > cap) want = cap;
          EXPECT(g == want && g >= 1 && g <= LNORM_MAX_BLOCKS);
        }
  EXPECT(lnorm_lds_bytes(desc(4, 768, 768, 768), DFX_LNORM_ROW) == 6144 && lnorm_lds_bytes(desc(4, 768, 768, 768), DFX_LNORM_GENERIC) == 0);
  EXPECT(lnorm_lds_bytes(desc(4, 100, 112, 112), DFX_LNORM_ROW) == 8 * 112);
  EXPECT(lnorm_lds_bytes(desc(4, 8192, 8192, 8192), DFX_LNORM_ROW) == 65536 && lnorm_lds_bytes(desc(4, 8193, 8208, 8208), DFX_LNORM_ROW) == 0);
  EXPECT(lnorm_lds_bytes(desc(4, 16384, 16384, 16384), DFX_LNORM_ROW) == 0);
  EXPECT(lnorm_param_bytes(1) == 144 && lnorm_param_bytes(16) == 144 && lnorm_param_bytes(17) == 288 && lnorm_param_bytes(16384) == 9 * 16384);
  // ---- extents, overlap, bytes
  EXPECT(plan_extent(1, 32, 21, 1) == 21 && plan_extent(3, 32, 21, 4) == (2 * 32 + 21) * 4);
  EXPECT(plan_extent(1ll << 35, 32, 32, 4) == (1ull << 42));
  // the documented maximum rows * ld = 2^40 at both ends of the pitch's range, 4-byte elements; the pitches of tests/far_offsets.py
  EXPECT(plan_extent(1ll << 40, 1, 1, 4) == (1ull << 42) && plan_extent(1ll << 26, 16384, 16384, 4) == (1ull << 42));
  EXPECT(plan_extent(513, 2147483647, 16384, 4) == (512ull * 2147483647ull + 16384) * 4 && rc(desc(512, 16384, 2147483647, 2147483647)) == DFX_OK);
  EXPECT(plan_extent(5, (1 << 30) + 4160, 40, 1) == (1ull << 32) + 4 * 4160 + 40 && plan_extent(3, (1 << 29) + 1040, 40, 4) == (1ull << 32) + 8320 + 160);
  EXPECT(plan_extent(3, (1ll << 31) + 4160, 40, 1) == (1ull << 32) + 8320 + 40);  // (a pitch above 2^31: the shared extent takes 64-bit pitches)
  EXPECT(lnorm_algorithmic_bytes(desc(1ll << 40, 1, 1, 1, DFX_U8, DFX_F32), false) == 5 * (1ull << 40) + 8);
  {
    const uintptr_t far = (uintptr_t)1 << 47;  // an operand of 2^42 bytes against a neighbour on either side, and one between its rows
    EXPECT(plan_overlap(far, 1ull << 42, far + (1ull << 42) - 1, 1) && !plan_overlap(far, 1ull << 42, far + (1ull << 42), 16) &&
           !plan_overlap(far, 1ull << 42, far - 16, 16) && plan_overlap(far, 1ull << 42, far - 16, 17) &&
           plan_overlap(far + (1ull << 32) + 64, 240, far, (1ull << 32) + 16680));
  }
  EXPECT(plan_overlap(100, 10, 109, 5) && !plan_overlap(100, 10, 110, 5) && !plan_overlap(110, 5, 100, 10) && plan_overlap(100, 10, 90, 11));
  EXPECT(lnorm_algorithmic_bytes(desc(70, 96, 96, 96), false) == 70 * 96 * 2 + 8 * 96);
  EXPECT(lnorm_algorithmic_bytes(desc(70, 96, 112, 128, DFX_U8, DFX_F32), true) == 70 * 96 * 5 + 9 * 96);
  if (g_bad) {
    printf("lnorm_plan_check: %d checks FAILED\n", g_bad);
    return 1;
  }
  printf("lnorm plans: validation order, bounds, classes, lanes, grids and the 2^40 limit hold\n");
  return 0;
}
