// head_plan_check -- host-only check of csrc/head_plan.h, what the net head (dfx_head_*) decides before a kernel runs:
// the descriptor's validation at the last admitted and the first refused value of every bound, the class predicates of the
// three paths swept over dtypes, k and src_ld, the softmax table's two refusals at c * max(E) = 2^32 - 1 and 2^32, the
// grids under the cap, the extents the overlap check uses and the 2^40 limit.  No HIP: it builds with SAN=1 (ASan + UBSan)
// and runs anywhere.
//   head_plan_check
#include <cstdio>
#include <cstring>
#include <vector>

#include "../csrc/head_plan.h"

using namespace dfx;

static int g_bad = 0;
#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      printf("head_plan_check: line %d: %s\n", __LINE__, #cond);      \
      ++g_bad;                                                        \
    }                                                                 \
  } while (0)

static dfx_head_desc topk(long long rows, int c, int ld, int dt, int k, int idx_dt) {
  dfx_head_desc d;
  memset(&d, 0, sizeof(d));
  d.rows = rows; d.mode = DFX_HEAD_TOPK; d.src_dt = dt; d.dst_dt = idx_dt; d.c = c; d.src_ld = ld; d.idx_ld = k; d.k = k;
  d.force_path = -1;
  return d;
}
static dfx_head_desc softmax(long long rows, int c, int ld, int dt, int dst_dt, int dst_ld) {
  dfx_head_desc d;
  memset(&d, 0, sizeof(d));
  d.rows = rows; d.mode = DFX_HEAD_SOFTMAX; d.src_dt = dt; d.dst_dt = dst_dt; d.c = c; d.src_ld = ld; d.dst_ld = dst_ld;
  d.out_scale = 255.0f; d.force_path = -1;
  return d;
}
static int rc(const dfx_head_desc &d) {
  const char *why = nullptr;
  const int r = head_validate(d, &why);
  EXPECT(why != nullptr && (r == DFX_OK) == (why[0] == 0));
  EXPECT(head_validate(d, nullptr) == r);
  return r;
}

int main() {
  const int dts[4] = {DFX_U8, DFX_S8, DFX_S32, DFX_F32};
  // ---- validation, each bound at its last admitted and first refused value
  EXPECT(rc(topk(1, 1, 1, DFX_U8, 1, DFX_U8)) == DFX_OK);
  EXPECT(rc(topk(0, 1, 1, DFX_U8, 1, DFX_U8)) == DFX_ERR_INVALID);
  EXPECT(rc(topk(4, 0, 16, DFX_U8, 1, DFX_U8)) == DFX_ERR_INVALID);
  EXPECT(rc(topk(4, 65535, 65535, DFX_S8, 8, DFX_S32)) == DFX_OK);
  EXPECT(rc(topk(4, 65536, 65536, DFX_S8, 8, DFX_S32)) == DFX_ERR_INVALID);
  for (int k = -1; k <= 10; ++k) EXPECT(rc(topk(4, 21, 32, DFX_U8, k, DFX_U8)) == ((k >= 1 && k <= 8) ? DFX_OK : DFX_ERR_INVALID));
  for (int c = 1; c <= 9; ++c)
    for (int k = 1; k <= 8; ++k) EXPECT(rc(topk(4, c, 16, DFX_F32, k, DFX_S32)) == (k <= c ? DFX_OK : DFX_ERR_INVALID));
  EXPECT(rc(topk(4, 256, 256, DFX_U8, 1, DFX_U8)) == DFX_OK);
  EXPECT(rc(topk(4, 257, 272, DFX_U8, 1, DFX_U8)) == DFX_ERR_INVALID);
  EXPECT(rc(topk(4, 257, 272, DFX_U8, 1, DFX_S32)) == DFX_OK);
  EXPECT(rc(topk(4, 21, 20, DFX_U8, 1, DFX_U8)) == DFX_ERR_INVALID);
  EXPECT(rc(topk(4, 21, 21, DFX_U8, 1, DFX_U8)) == DFX_OK);
  for (int bad : {(int)DFX_UNDEF, 5, -1}) {
    EXPECT(rc(topk(4, 21, 32, bad, 1, DFX_U8)) == DFX_ERR_INVALID);
    EXPECT(rc(topk(4, 21, 32, DFX_U8, 1, bad)) == DFX_ERR_INVALID);
    EXPECT(rc(softmax(4, 21, 32, DFX_U8, bad, 21)) == DFX_ERR_INVALID);
  }
  EXPECT(rc(topk(4, 21, 32, DFX_U8, 1, DFX_F32)) == DFX_ERR_INVALID && rc(topk(4, 21, 32, DFX_U8, 1, DFX_S8)) == DFX_ERR_INVALID);
  {
    dfx_head_desc d = topk(4, 21, 32, DFX_U8, 3, DFX_U8);
    d.idx_ld = 2;
    EXPECT(rc(d) == DFX_ERR_INVALID);
    d.idx_ld = 3;
    EXPECT(rc(d) == DFX_OK);
    d.mode = 2;
    EXPECT(rc(d) == DFX_ERR_INVALID);
    d.mode = DFX_HEAD_TOPK;
    for (int p = -3; p <= 4; ++p) {
      d.force_path = p;
      EXPECT(rc(d) == ((p >= -1 && p <= 2) ? DFX_OK : DFX_ERR_INVALID));
    }
  }
  EXPECT(rc(softmax(4, 21, 32, DFX_U8, DFX_F32, 21)) == DFX_OK && rc(softmax(4, 21, 32, DFX_S8, DFX_U8, 32)) == DFX_OK);
  EXPECT(rc(softmax(4, 21, 32, DFX_U8, DFX_F32, 20)) == DFX_ERR_INVALID);
  EXPECT(rc(softmax(4, 21, 32, DFX_U8, DFX_S32, 21)) == DFX_ERR_INVALID && rc(softmax(4, 21, 32, DFX_U8, DFX_S8, 21)) == DFX_ERR_INVALID);
  EXPECT(rc(softmax(4, 21, 32, DFX_S32, DFX_F32, 21)) == DFX_ERR_UNSUPPORTED && rc(softmax(4, 21, 32, DFX_F32, DFX_F32, 21)) == DFX_ERR_UNSUPPORTED);
  EXPECT(rc(softmax(4, 21, 20, DFX_S32, DFX_F32, 21)) == DFX_ERR_INVALID);  // invalid is found before unsupported
  {
    dfx_head_desc d = softmax(4, 21, 32, DFX_U8, DFX_U8, 21);
    const unsigned inf = 0x7f800000u, nan = 0x7fc00000u;
    memcpy(&d.out_scale, &inf, 4);
    EXPECT(rc(d) == DFX_ERR_INVALID);
    memcpy(&d.out_scale, &nan, 4);
    EXPECT(rc(d) == DFX_ERR_INVALID);
    d.dst_dt = DFX_F32;  // ignored there
    EXPECT(rc(d) == DFX_OK);
  }
  // ---- the 2^40 limit: rows * max(src_ld, out_ld), no product formed before it is known to fit
  EXPECT(rc(topk(1ll << 36, 16, 16, DFX_U8, 1, DFX_U8)) == DFX_OK);
  EXPECT(rc(topk((1ll << 36) + 1, 16, 16, DFX_U8, 1, DFX_U8)) == DFX_ERR_INVALID);
  EXPECT(rc(softmax(1ll << 35, 16, 16, DFX_U8, DFX_U8, 32)) == DFX_OK);
  EXPECT(rc(softmax((1ll << 35) + 1, 16, 16, DFX_U8, DFX_U8, 32)) == DFX_ERR_INVALID);
  EXPECT(rc(topk(1ll << 40, 1, 1, DFX_U8, 1, DFX_U8)) == DFX_OK);
  EXPECT(rc(topk((1ll << 40) + 1, 1, 1, DFX_U8, 1, DFX_U8)) == DFX_ERR_INVALID);
  EXPECT(rc(topk(0x7fffffffffffffffll, 1, 0x7fffffff, DFX_U8, 1, DFX_U8)) == DFX_ERR_INVALID);
  {
    dfx_head_desc d = topk(1ll << 36, 16, 16, DFX_U8, 1, DFX_U8);
    d.idx_ld = 32;  // idx rows further apart than src rows
    EXPECT(rc(d) == DFX_ERR_INVALID);
  }
  // ---- classes
  for (int dt : dts)
    for (int k = 1; k <= 8; ++k)
      for (int ld = 8; ld <= 200; ++ld) {
        const dfx_head_desc d = topk(7, 8, ld, dt, k, DFX_S32);
        const int es = plan_dt_size(dt);
        EXPECT(head_pixel_class(d) == (es == 1 && k == 1 && ld % 16 == 0 && ld <= 160));
        EXPECT(head_row_class(d) == ((ld * es) % 16 == 0));
        EXPECT(head_in_class(d, DFX_HEAD_GENERIC) && head_in_class(d, DFX_HEAD_PIXEL) == head_pixel_class(d) &&
               head_in_class(d, DFX_HEAD_ROW) == head_row_class(d));
        // the auto rule: pixel in its class, else row from 160-byte rows on, else generic
        EXPECT(head_path(d) == (head_pixel_class(d) ? DFX_HEAD_PIXEL : (head_row_class(d) && ld * es >= 160) ? DFX_HEAD_ROW : DFX_HEAD_GENERIC));
        dfx_head_desc f = d;
        for (int p = 0; p < 3; ++p) {
          f.force_path = p;
          EXPECT(head_path(f) == p);
        }
      }
  EXPECT(head_pixel_class(softmax(7, 150, 160, DFX_S8, DFX_U8, 150)) && !head_pixel_class(softmax(7, 161, 176, DFX_S8, DFX_U8, 161)));
  EXPECT(head_row_class(softmax(7, 161, 176, DFX_S8, DFX_U8, 161)) && !head_row_class(softmax(7, 21, 21, DFX_S8, DFX_U8, 21)));
  EXPECT(head_row_class(topk(3, 1000, 1000, DFX_F32, 5, DFX_S32)) && !head_row_class(topk(3, 1000, 1001, DFX_F32, 5, DFX_S32)));
  EXPECT(head_path(topk(3, 1000, 1008, DFX_S8, 5, DFX_S32)) == DFX_HEAD_ROW && head_path(topk(3, 1000, 1000, DFX_F32, 1, DFX_S32)) == DFX_HEAD_ROW);
  EXPECT(head_path(topk(70, 21, 32, DFX_S8, 5, DFX_U8)) == DFX_HEAD_GENERIC && head_path(topk(70, 21, 32, DFX_S8, 1, DFX_U8)) == DFX_HEAD_PIXEL);
  EXPECT(head_path(topk(70, 37, 40, DFX_S32, 1, DFX_U8)) == DFX_HEAD_ROW && head_path(topk(70, 21, 36, DFX_S32, 1, DFX_U8)) == DFX_HEAD_GENERIC);
  EXPECT(head_path(softmax(70, 150, 160, DFX_U8, DFX_U8, 150)) == DFX_HEAD_ROW && head_path(softmax(70, 130, 144, DFX_U8, DFX_U8, 130)) == DFX_HEAD_PIXEL &&
         head_path(topk(70, 150, 160, DFX_U8, 1, DFX_U8)) == DFX_HEAD_PIXEL && head_path(softmax(70, 161, 176, DFX_U8, DFX_U8, 161)) == DFX_HEAD_ROW);
  EXPECT(head_path(softmax(70, 21, 21, DFX_U8, DFX_U8, 21)) == DFX_HEAD_GENERIC && head_path(topk(3, 1000, 1001, DFX_S8, 5, DFX_S32)) == DFX_HEAD_GENERIC);
  // ---- the table's two refusals
  {
    std::vector<uint32_t> e(256, 0);
    const char *why = nullptr;
    EXPECT(head_table_ok(e.data(), 21, &why) == DFX_ERR_INVALID && why && why[0]);
    e[0] = 1;
    EXPECT(head_table_ok(e.data(), 65535, nullptr) == DFX_OK);
    e[0] = 65537;  // 65535 * 65537 = 2^32 - 1: the last admitted value
    EXPECT(head_table_ok(e.data(), 65535, &why) == DFX_OK && why[0] == 0);
    e[255] = 65538;  // the maximum need not be E[0]
    EXPECT(head_table_ok(e.data(), 65535, nullptr) == DFX_ERR_INVALID);
    e[255] = 0;
    e[0] = 0xffffffffu;
    EXPECT(head_table_ok(e.data(), 1, nullptr) == DFX_OK && head_table_ok(e.data(), 2, nullptr) == DFX_ERR_INVALID);
    e[0] = 1u << 31;  // 2 * 2^31 = 2^32: the first refused value
    EXPECT(head_table_ok(e.data(), 2, nullptr) == DFX_ERR_INVALID);
    e[0] = (1u << 31) - 1;
    EXPECT(head_table_ok(e.data(), 2, nullptr) == DFX_OK);
    for (int c = 1; c <= 65535; c += 131) {
      e[0] = (uint32_t)(0xffffffffull / c);
      EXPECT(head_table_ok(e.data(), c, nullptr) == DFX_OK);
      if ((uint64_t)(e[0] + 1ull) * c > 0xffffffffull && e[0] != 0xffffffffu) {
        e[0] += 1;
        EXPECT(head_table_ok(e.data(), c, nullptr) == DFX_ERR_INVALID);
      }
    }
  }
  // ---- grids
  for (long long rows : {1ll, 3ll, 4ll, 5ll, 255ll, 256ll, 257ll, 70ll, 193ll, 1ll << 20, 1ll << 40})
    for (long long cap : {0ll, 1ll, 2ll, 5000ll})
      for (int p = 0; p < 3; ++p) {
        const int per = p == DFX_HEAD_ROW ? 4 : 256;
        const int g = head_grid(rows, p, cap);
        long long want = (rows + per - 1) / per;
        if (want > HEAD_MAX_BLOCKS) want = HEAD_MAX_BLOCKS;
        if (cap > 0 && want > cap) want = cap;
        EXPECT(g == want && g >= 1 && g <= HEAD_MAX_BLOCKS);
      }
  EXPECT(head_lds_bytes(softmax(4, 21, 32, DFX_U8, DFX_U8, 21), DFX_HEAD_PIXEL) == 1024 && head_lds_bytes(softmax(4, 21, 32, DFX_U8, DFX_U8, 21), DFX_HEAD_GENERIC) == 0);
  EXPECT(head_lds_bytes(topk(4, 21, 32, DFX_U8, 1, DFX_U8), DFX_HEAD_ROW) == 0);
  // ---- extents, overlap, bytes
  EXPECT(plan_extent(1, 32, 21, 1) == 21 && plan_extent(3, 32, 21, 4) == (2 * 32 + 21) * 4);
  EXPECT(plan_extent(1ll << 35, 32, 32, 4) == (1ull << 42));
  // the documented maximum rows * ld = 2^40 at both ends of the pitch's range, 4-byte elements; the pitches of tests/far_offsets.py
  EXPECT(plan_extent(1ll << 40, 1, 1, 4) == (1ull << 42) && plan_extent(513, 2147483647, 65535, 4) == (512ull * 2147483647ull + 65535) * 4);
  EXPECT(plan_extent(5, (1 << 30) + 4160, 21, 1) == (1ull << 32) + 4 * 4160 + 21 && plan_extent(3, (1 << 29) + 1040, 5, 4) == (1ull << 32) + 8320 + 20);
  EXPECT(plan_extent(3, (1ll << 31) + 4160, 40, 1) == (1ull << 32) + 8320 + 40);  // (a pitch above 2^31: the shared extent takes 64-bit pitches)
  EXPECT(head_algorithmic_bytes(topk(1ll << 40, 1, 1, DFX_F32, 1, DFX_S32)) == 8 * (1ull << 40));
  {
    const uintptr_t far = (uintptr_t)1 << 47;  // an operand of 2^42 bytes against a neighbour on either side
    EXPECT(plan_overlap(far, 1ull << 42, far + (1ull << 42) - 1, 1) && !plan_overlap(far, 1ull << 42, far + (1ull << 42), 16) &&
           !plan_overlap(far, 1ull << 42, far - 16, 16) && plan_overlap(far, 1ull << 42, far - 16, 17));
  }
  EXPECT(plan_overlap(100, 10, 109, 5) && !plan_overlap(100, 10, 110, 5) && !plan_overlap(110, 5, 100, 10) && plan_overlap(100, 10, 90, 11));
  EXPECT(head_algorithmic_bytes(topk(70, 21, 32, DFX_U8, 1, DFX_U8)) == 70 * 21 + 70);
  EXPECT(head_algorithmic_bytes(topk(3, 1000, 1000, DFX_F32, 5, DFX_S32)) == 3 * 1000 * 4 + 3 * 5 * 4);
  EXPECT(head_algorithmic_bytes(softmax(70, 21, 32, DFX_S8, DFX_F32, 32)) == 70 * 21 + 70 * 21 * 4);
  if (g_bad) {
    printf("head_plan_check: %d checks FAILED\n", g_bad);
    return 1;
  }
  printf("head plans: validation, classes, table bounds, grids and the 2^40 limit hold\n");
  return 0;
}
