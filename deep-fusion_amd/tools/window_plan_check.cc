// window_plan_check -- host-only check of csrc/window_plan.h, what the window partition / reverse op (dfx_window_*) decides
// before a kernel runs: the order of the descriptor's validation (every DFX_ERR_INVALID before the one DFX_ERR_UNSUPPORTED) at
// the last admitted and the first refused value of every limit; THE ROW MAP against a second formula (the inverse mapping, from
// the grid's side), partition map o reverse map = identity on non-pad tokens, the pad count bs * (hp * wp - h * w); the class and
// auto predicates, the grids under the cap, the extents, the overlap predicate and 64-bit offsets for rows * ld up to 2^40
// (nothing is allocated for those).  No HIP: it builds with SAN=1 (ASan + UBSan) and runs anywhere.
//   window_plan_check
#include <cstdio>
#include <cstring>
#include <vector>

#include "../csrc/window_plan.h"

using namespace dfx;

static int g_bad = 0;
#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      printf("window_plan_check: line %d: %s\n", __LINE__, #cond);    \
      ++g_bad;                                                        \
    }                                                                 \
  } while (0)

static dfx_window_desc desc(int dir, int bs, int h, int w, int c, int wh, int ww, int sy = 0, int sx = 0, int order = DFX_WINDOW_ROW_MAJOR,
                            int dt = DFX_S8, long long gld = 0, long long wld = 0) {
  dfx_window_desc d;
  memset(&d, 0, sizeof(d));
  d.dir = dir; d.dt = dt; d.bs = bs; d.h = h; d.w = w; d.c = c; d.wh = wh; d.ww = ww; d.shift_y = sy; d.shift_x = sx; d.order = order;
  d.grid_ld = gld ? gld : c; d.win_ld = wld ? wld : c;
  d.pad_value = 0; d.force_path = -1;
  return d;
}
static int rc(const dfx_window_desc &d, const char **why_out = nullptr) {
  const char *why = nullptr;
  const int r = window_validate(d, &why);
  EXPECT(why != nullptr && (r == DFX_OK) == (why[0] == 0));
  EXPECT(window_validate(d, nullptr) == r);
  if (why_out) *why_out = why;
  return r;
}
static const int P = DFX_WINDOW_PARTITION, R = DFX_WINDOW_REVERSE;

// the second formula: from the GRID's side.  Grid (y, x) sits at padded (Y, X) = ((y - shift_y) mod hp, (x - shift_x) mod wp)
// after the roll by -shift; its window and its place within it follow by division.
static int win_row_from_grid(const dfx_window_desc &d, int y, int x) {
  const int hp = window_hp(d), wp = window_wp(d);
  const int Y = ((y - d.shift_y) % hp + hp) % hp, X = ((x - d.shift_x) % wp + wp) % wp;
  const int per = d.wh * d.ww, nwx = wp / d.ww;
  const int widx = (Y / d.wh) * nwx + X / d.ww;
  const int iy = Y - Y / d.wh * d.wh, ix = X - X / d.ww * d.ww;
  return widx * per + (d.order == DFX_WINDOW_COL_MAJOR ? ix * d.wh + iy : iy * d.ww + ix);
}

static void check_maps(dfx_window_desc d) {
  d.dir = P;
  std::vector<int32_t> part, rev;
  window_build_map(d, part);
  d.dir = R;
  window_build_map(d, rev);
  const long long win = window_win_rows(d), grid = window_grid_rows(d);
  EXPECT((long long)part.size() == win && (long long)rev.size() == grid);
  long long pads = 0;
  std::vector<char> seen((size_t)grid, 0);
  for (long long r = 0; r < win; ++r) {
    const int m = part[(size_t)r];
    if (m < 0) { ++pads; EXPECT(m == -1); continue; }
    EXPECT(m < grid && !seen[(size_t)m]);
    if (m >= grid) continue;
    seen[(size_t)m] = 1;
    EXPECT(rev[(size_t)m] == r);                                        // reverse o partition = identity on non-pad tokens
    EXPECT(win_row_from_grid(d, m / d.w, m % d.w) == r);                // the second formula
  }
  for (long long g = 0; g < grid; ++g) {
    EXPECT(seen[(size_t)g]);                                            // every grid token lies in exactly one window-side row
    const int r = rev[(size_t)g];
    EXPECT(r >= 0 && r < win && part[(size_t)r] == g && r == win_row_from_grid(d, (int)(g / d.w), (int)(g % d.w)));
  }
  EXPECT(pads == win - grid && window_pad_tokens(d) == (long long)d.bs * pads);
}

int main() {
  // ---- validation, each limit at its last admitted and first refused value
  EXPECT(rc(desc(P, 1, 1, 1, 1, 1, 1)) == DFX_OK && rc(desc(R, 1, 1, 1, 1, 1, 1)) == DFX_OK);
  EXPECT(rc(desc(2, 1, 1, 1, 1, 1, 1)) == DFX_ERR_INVALID && rc(desc(-1, 1, 1, 1, 1, 1, 1)) == DFX_ERR_INVALID);
  for (int dt : {(int)DFX_UNDEF, 5, -1}) EXPECT(rc(desc(P, 1, 4, 4, 16, 2, 2, 0, 0, 0, dt)) == DFX_ERR_INVALID);
  for (int dt : {(int)DFX_F32, (int)DFX_S32, (int)DFX_S8, (int)DFX_U8}) EXPECT(rc(desc(P, 1, 4, 4, 16, 2, 2, 0, 0, 0, dt)) == DFX_OK);
  EXPECT(rc(desc(P, 0, 4, 4, 16, 2, 2)) == DFX_ERR_INVALID && rc(desc(P, -3, 4, 4, 16, 2, 2)) == DFX_ERR_INVALID);
  EXPECT(rc(desc(P, 1, 0, 4, 16, 2, 2)) == DFX_ERR_INVALID && rc(desc(P, 1, 4, 0, 16, 2, 2)) == DFX_ERR_INVALID);
  EXPECT(rc(desc(P, 1, 65535, 1, 16, 255, 1)) == DFX_OK && rc(desc(P, 1, 65536, 1, 16, 255, 1)) == DFX_ERR_INVALID);
  EXPECT(rc(desc(P, 1, 1, 65535, 16, 1, 255)) == DFX_OK && rc(desc(P, 1, 1, 65536, 16, 1, 255)) == DFX_ERR_INVALID);
  EXPECT(rc(desc(P, 1, 4, 4, 0, 2, 2)) == DFX_ERR_INVALID && rc(desc(P, 1, 4, 4, 1, 2, 2)) == DFX_OK);
  EXPECT(rc(desc(P, 1, 4, 4, 16, 0, 2)) == DFX_ERR_INVALID && rc(desc(P, 1, 4, 4, 16, 2, 0)) == DFX_ERR_INVALID);
  EXPECT(rc(desc(P, 1, 4, 4, 16, 255, 255)) == DFX_OK && rc(desc(P, 1, 4, 4, 16, 256, 2)) == DFX_ERR_INVALID && rc(desc(P, 1, 4, 4, 16, 2, 256)) == DFX_ERR_INVALID);
  EXPECT(rc(desc(P, 1, 4, 4, 16, 2, 2, 0, 0, 2)) == DFX_ERR_INVALID && rc(desc(P, 1, 4, 4, 16, 2, 2, 0, 0, -1)) == DFX_ERR_INVALID);
  // the shift lies within the PADDED map: 16 x 12 with window 7 is 21 x 14
  EXPECT(rc(desc(P, 1, 16, 12, 16, 7, 7, 20, 13)) == DFX_OK && rc(desc(P, 1, 16, 12, 16, 7, 7, 21, 0)) == DFX_ERR_INVALID &&
         rc(desc(P, 1, 16, 12, 16, 7, 7, 0, 14)) == DFX_ERR_INVALID && rc(desc(P, 1, 16, 12, 16, 7, 7, -1, 0)) == DFX_ERR_INVALID &&
         rc(desc(P, 1, 16, 12, 16, 7, 7, 0, -1)) == DFX_ERR_INVALID);
  EXPECT(rc(desc(P, 1, 5, 4, 16, 7, 7, 6, 6)) == DFX_OK && rc(desc(P, 1, 5, 4, 16, 7, 7, 7, 0)) == DFX_ERR_INVALID);  // a window larger than the image
  EXPECT(rc(desc(P, 1, 4, 4, 16, 2, 2, 0, 0, 0, DFX_S8, 15, 16)) == DFX_ERR_INVALID && rc(desc(P, 1, 4, 4, 16, 2, 2, 0, 0, 0, DFX_S8, 16, 15)) == DFX_ERR_INVALID &&
         rc(desc(P, 1, 4, 4, 16, 2, 2, 0, 0, 0, DFX_S8, 17, 1000)) == DFX_OK);
  {
    dfx_window_desc d = desc(P, 1, 4, 4, 16, 2, 2);
    for (int p = -3; p <= 3; ++p) {
      d.force_path = p;
      EXPECT(rc(d) == ((p >= -1 && p <= 1) ? DFX_OK : DFX_ERR_INVALID));
    }
  }
  // hp * wp <= 2^22: 2048 x 2048 is the limit; one more window row is beyond it
  EXPECT(rc(desc(P, 1, 2048, 2048, 16, 2, 2)) == DFX_OK && rc(desc(P, 1, 2049, 2048, 16, 2, 2)) == DFX_ERR_INVALID);
  EXPECT(rc(desc(P, 1, 2047, 2047, 16, 2, 2)) == DFX_OK && rc(desc(P, 1, 65535, 64, 16, 1, 1)) == DFX_OK && rc(desc(P, 1, 65535, 65, 16, 1, 1)) == DFX_ERR_INVALID);
  EXPECT(rc(desc(P, 1, 65535, 65535, 16, 255, 255)) == DFX_ERR_INVALID);
  // bs * hp * wp * max(grid_ld, win_ld) <= 2^40, no product formed before it is known to fit
  EXPECT(rc(desc(P, 1 << 14, 2048, 2048, 16, 2, 2)) == DFX_OK && rc(desc(P, (1 << 14) + 1, 2048, 2048, 16, 2, 2)) == DFX_ERR_INVALID);
  EXPECT(rc(desc(P, 1 << 13, 2048, 2048, 16, 2, 2, 0, 0, 0, DFX_S8, 32, 16)) == DFX_OK && rc(desc(P, (1 << 13) + 1, 2048, 2048, 16, 2, 2, 0, 0, 0, DFX_S8, 32, 16)) == DFX_ERR_INVALID);
  EXPECT(rc(desc(R, 1 << 13, 2048, 2048, 16, 2, 2, 0, 0, 0, DFX_F32, 16, 32)) == DFX_OK && rc(desc(R, (1 << 13) + 1, 2048, 2048, 16, 2, 2, 0, 0, 0, DFX_F32, 16, 32)) == DFX_ERR_INVALID);
  EXPECT(rc(desc(P, 1, 1, 3, 16, 1, 3, 0, 0, 0, DFX_S8, (1ll << 40) / 3, 16)) == DFX_OK && rc(desc(P, 1, 1, 3, 16, 1, 3, 0, 0, 0, DFX_S8, (1ll << 40) / 3 + 1, 16)) == DFX_ERR_INVALID);
  EXPECT(rc(desc(P, 0x7fffffff, 2048, 2048, 16, 2, 2, 0, 0, 0, DFX_S8, 0x7fffffffffffffffll, 16)) == DFX_ERR_INVALID);
  // the padding counts: a 1 x 3 map under a 255 x 255 window is 65025 rows per image
  EXPECT(rc(desc(P, 1, 1, 3, 16, 255, 255, 0, 0, 0, DFX_S8, (1ll << 40) / 65025, 16)) == DFX_OK &&
         rc(desc(P, 1, 1, 3, 16, 255, 255, 0, 0, 0, DFX_S8, (1ll << 40) / 65025 + 1, 16)) == DFX_ERR_INVALID);
  // ---- the order: with faults i and j > i the reason is i's; the forced path's class comes after everything invalid
  {
    struct Fault { const char *word; void (*set)(dfx_window_desc &); };
    const Fault faults[] = {
        {"dir", [](dfx_window_desc &d) { d.dir = 7; }},
        {"dtype", [](dfx_window_desc &d) { d.dt = DFX_UNDEF; }},
        {"bs", [](dfx_window_desc &d) { d.bs = 0; }},
        {"h and w", [](dfx_window_desc &d) { d.h = 0; }},
        {"c must", [](dfx_window_desc &d) { d.c = 0; }},
        {"wh and ww", [](dfx_window_desc &d) { d.ww = 256; }},
        {"order", [](dfx_window_desc &d) { d.order = 2; }},
        {"shift_y", [](dfx_window_desc &d) { d.shift_y = 1 << 20; }},
        {"shift_x", [](dfx_window_desc &d) { d.shift_x = -1; }},
        {"grid_ld", [](dfx_window_desc &d) { d.grid_ld = d.c - 1; }},
        {"win_ld", [](dfx_window_desc &d) { d.win_ld = d.c - 1; }},
        {"force_path", [](dfx_window_desc &d) { d.force_path = 2; }},
        {"2^22", [](dfx_window_desc &d) { d.h = 4096; d.w = 2048; }},
        {"2^40", [](dfx_window_desc &d) { d.bs = 1 << 30; }},
    };
    const int n = (int)(sizeof(faults) / sizeof(faults[0]));
    for (int i = 0; i < n; ++i)
      for (int j = i; j < n; ++j) {
        // (the same field, or a bound that follows another fault's field: c for the lds, h for the padded size, bs for 2^40)
        if ((i == 3 && j == 12) || (i == 4 && (j == 9 || j == 10)) || (i == 2 && j == 13)) continue;
        dfx_window_desc d = desc(P, 2, 10, 13, 21, 7, 7);
        d.force_path = DFX_WINDOW_ROW;  // outside the row class as well: never reported while something is invalid
        faults[j].set(d);
        faults[i].set(d);
        if (j == 11) d.force_path = 2;
        const char *why = "";
        EXPECT(rc(d, &why) == DFX_ERR_INVALID && strstr(why, faults[i].word) != nullptr);
      }
    dfx_window_desc d = desc(P, 2, 10, 13, 21, 7, 7);
    d.force_path = DFX_WINDOW_ROW;
    EXPECT(rc(d) == DFX_OK && !window_in_class(d, d.force_path));  // window_create turns this into DFX_ERR_UNSUPPORTED
  }
  // ---- geometry
  {
    const dfx_window_desc d = desc(P, 2, 16, 12, 64, 7, 7, 3, 3);
    EXPECT(window_hp(d) == 21 && window_wp(d) == 14 && window_count(d) == 6 && window_win_rows(d) == 294 && window_grid_rows(d) == 192);
    EXPECT(window_pad_tokens(d) == 2 * (294 - 192));
    const dfx_window_desc m = desc(P, 1, 56, 56, 96, 2, 2, 0, 0, DFX_WINDOW_COL_MAJOR);
    EXPECT(window_hp(m) == 56 && window_count(m) == 784 && window_pad_tokens(m) == 0);
    const dfx_window_desc big = desc(P, 1, 5, 4, 16, 7, 7);
    EXPECT(window_hp(big) == 7 && window_wp(big) == 7 && window_count(big) == 1 && window_pad_tokens(big) == 29);
  }
  // ---- the map: a second formula, the two directions against each other, the pad count
  {
    const int grids[][2] = {{1, 1}, {7, 7}, {10, 13}, {3, 200}, {5, 4}, {16, 12}, {56, 56}, {1, 3}, {255, 2}};
    const int wins[][2] = {{1, 1}, {2, 2}, {4, 4}, {7, 7}, {3, 5}, {5, 3}, {1, 3}, {255, 1}};
    for (const auto &g : grids)
      for (const auto &w : wins)
        for (int order = 0; order < 2; ++order) {
          dfx_window_desc d = desc(P, 3, g[0], g[1], 16, w[0], w[1], 0, 0, order);
          const int hp = window_hp(d), wp = window_wp(d);
          const int shifts[][2] = {{0, 0}, {w[0] / 2, w[1] / 2}, {w[0] / 2, 0}, {0, w[1] / 2}, {hp - 1, wp - 1}, {hp - 1, 0}, {1 % hp, (wp - 1)}};
          for (const auto &s : shifts) {
            d.shift_y = s[0]; d.shift_x = s[1];
            EXPECT(rc(d) == DFX_OK);
            check_maps(d);
          }
        }
    // hand-checked entries: 4 x 4, window 2, no shift: window 1 (wy 0, wx 1) holds grid tokens 2, 3, 6, 7 (row-major), 2, 6, 3, 7 (column-major)
    std::vector<int32_t> m;
    window_build_map(desc(P, 1, 4, 4, 16, 2, 2), m);
    EXPECT(m.size() == 16 && m[4] == 2 && m[5] == 3 && m[6] == 6 && m[7] == 7 && m[12] == 10);
    window_build_map(desc(P, 1, 4, 4, 16, 2, 2, 0, 0, DFX_WINDOW_COL_MAJOR), m);
    EXPECT(m[4] == 2 && m[5] == 6 && m[6] == 3 && m[7] == 7);
    // shift 1: torch.roll(-1) brings grid (1, 1) to padded (0, 0); the last row and column wrap to the first
    window_build_map(desc(P, 1, 4, 4, 16, 2, 2, 1, 1), m);
    EXPECT(m[0] == 5 && m[1] == 6 && m[2] == 9 && m[15] == 0);
    // 3 x 3 under window 2: padded to 4 x 4, 7 pad tokens; padded (1, 3) is a pad token, and with shift 1 grid (0, 0) lands at padded (3, 3)
    window_build_map(desc(P, 1, 3, 3, 16, 2, 2), m);
    EXPECT(m[0] == 0 && m[1] == 1 && m[2] == 3 && m[3] == 4 && m[4] == 2 && m[5] == -1 && m[7] == -1 && m[15] == -1);
    window_build_map(desc(P, 1, 3, 3, 16, 2, 2, 1, 1), m);
    EXPECT(m[0] == 4 && m[15] == 0 && m[12] == -1);
    window_build_map(desc(R, 1, 3, 3, 16, 2, 2), m);
    EXPECT(m.size() == 9 && m[0] == 0 && m[2] == 4 && m[4] == 3 && m[8] == 12);
  }
  // ---- class, auto, lanes
  for (int dt : {(int)DFX_S8, (int)DFX_U8, (int)DFX_F32, (int)DFX_S32})
    for (int c = 1; c <= 40; ++c)
      for (int gld = c; gld <= c + 17; ++gld)
        for (int wld = c; wld <= c + 17; wld += 3) {
          const dfx_window_desc d = desc(P, 2, 10, 13, c, 7, 7, 0, 0, 0, dt, gld, wld);
          const int es = plan_dt_size(dt);
          EXPECT(window_row_class(d) == ((c * es) % 16 == 0 && (gld * es) % 16 == 0 && (wld * es) % 16 == 0));
          EXPECT(window_in_class(d, DFX_WINDOW_GENERIC) && window_in_class(d, DFX_WINDOW_ROW) == window_row_class(d) && !window_in_class(d, 2));
          EXPECT(window_path(d) == (window_row_class(d) && window_row_auto(d) ? DFX_WINDOW_ROW : DFX_WINDOW_GENERIC));
          if (window_row_class(d)) EXPECT(window_lanes(d) * 16 == (long long)c * es);
          dfx_window_desc f = d;
          for (int p = 0; p < 2; ++p) {
            f.force_path = p;
            EXPECT(window_path(f) == p);
          }
        }
  EXPECT(window_lanes(desc(P, 1, 4, 4, 96, 2, 2)) == 6 && window_lanes(desc(P, 1, 4, 4, 16, 2, 2)) == 1 && window_lanes(desc(P, 1, 4, 4, 68, 2, 2, 0, 0, 0, DFX_F32)) == 17);
  // ---- grids
  for (int dir = 0; dir < 2; ++dir)
    for (int bs : {1, 3, 64, 4096})
      for (long long cap : {0ll, 1ll, 3ll, 5000ll})
        for (int c : {16, 96, 272})
          for (int p = 0; p < 2; ++p) {
            const dfx_window_desc d = desc(dir, bs, 10, 13, c, 7, 7);
            const long long rows = (long long)bs * (dir == P ? 14 * 14 : 10 * 13);
            const long long work = p == DFX_WINDOW_ROW ? rows * (c / 16) : rows * c, per = p == DFX_WINDOW_ROW ? 1024 : 256;
            long long want = (work + per - 1) / per;
            if (want > WINDOW_MAX_BLOCKS) want = WINDOW_MAX_BLOCKS;
            if (cap > 0 && want > cap) want = cap;
            EXPECT(window_grid(d, p, cap) == want && want >= 1);
          }
  EXPECT(window_grid(desc(P, 1 << 14, 2048, 2048, 16, 2, 2), DFX_WINDOW_GENERIC, 0) == WINDOW_MAX_BLOCKS);  // 2^40 elements of work
  // ---- sides, extents, overlap, bytes
  {
    const dfx_window_desc p = desc(P, 2, 16, 12, 64, 7, 7, 3, 3, 0, DFX_S8, 80, 192), r = desc(R, 2, 16, 12, 64, 7, 7, 3, 3, 0, DFX_F32, 80, 192);
    EXPECT(window_src_rows(p) == 192 && window_dst_rows(p) == 294 && window_src_ld(p) == 80 && window_dst_ld(p) == 192);
    EXPECT(window_src_rows(r) == 294 && window_dst_rows(r) == 192 && window_src_ld(r) == 192 && window_dst_ld(r) == 80);
    EXPECT(window_src_extent(p) == (383ull * 80 + 64) && window_dst_extent(p) == (587ull * 192 + 64));
    EXPECT(window_src_extent(r) == (587ull * 192 + 64) * 4 && window_dst_extent(r) == (383ull * 80 + 64) * 4);
    EXPECT(window_algorithmic_bytes(p) == (384ull + 588) * 64 + 4 * 294 && window_algorithmic_bytes(r) == 2ull * 384 * 256 + 4 * 192);
  }
  EXPECT(plan_extent(1, 32, 21, 1) == 21 && plan_extent(3, 32, 21, 4) == (2 * 32 + 21) * 4);
  // 64-bit offsets: rows * ld = 2^40 with 4-byte elements, and the pitches of tests/far_offsets.py (three rows)
  EXPECT(plan_extent(1ll << 36, 16, 16, 4) == (1ull << 42) && plan_extent(3, (1ll << 40) / 3, 16, 4) == (2 * ((1ull << 40) / 3) + 16) * 4);
  EXPECT(plan_extent(3, (1ll << 31) + 4160, 16, 1) == (1ull << 32) + 8320 + 16 && plan_extent(3, ((1ll << 31) + 4160) / 4, 4, 4) == (1ull << 32) + 8320 + 16);
  {
    const dfx_window_desc f = desc(P, 1, 1, 3, 16, 1, 3, 0, 0, 0, DFX_S8, 16, (1ll << 31) + 4160);
    EXPECT(rc(f) == DFX_OK && window_dst_extent(f) == (1ull << 32) + 8336 && window_src_extent(f) == 48);
    const dfx_window_desc big = desc(P, 1 << 14, 2048, 2048, 4, 2, 2, 0, 0, 0, DFX_F32, 16, 16);
    EXPECT(rc(big) == DFX_OK && window_dst_extent(big) == (((1ull << 36) - 1) * 16 + 4) * 4 && window_algorithmic_bytes(big) == (2ull << 36) * 16 + (4ull << 22));
    const uintptr_t far = (uintptr_t)1 << 47;  // an operand of 2^42 bytes against a neighbour on either side, and one between its rows
    EXPECT(plan_overlap(far, 1ull << 42, far + (1ull << 42) - 1, 1) && !plan_overlap(far, 1ull << 42, far + (1ull << 42), 16) &&
           !plan_overlap(far, 1ull << 42, far - 16, 16) && plan_overlap(far, 1ull << 42, far - 16, 17) &&
           plan_overlap(far + (1ull << 32) + 64, 240, far, (1ull << 32) + 8336));
  }
  EXPECT(plan_overlap(100, 10, 109, 5) && !plan_overlap(100, 10, 110, 5) && !plan_overlap(110, 5, 100, 10) && plan_overlap(100, 10, 90, 11));
  if (g_bad) {
    printf("window_plan_check: %d checks FAILED\n", g_bad);
    return 1;
  }
  printf("window plans: validation order, maps, pad counts, classes, grids, extents and the 2^40 limit hold\n");
  return 0;
}
