// nms_plan_check -- host-only check of csrc/nms_plan.h (no GPU, no HIP): the scan's block step (the very function the scan
// kernel compiles) driven over whole suppression masks exactly as the kernel drives it -- removed bitmap, diagonal tile,
// OR of the kept rows -- against a brute-force greedy walk, on random, empty, full and block-diagonal masks; the enumeration
// of the upper triangle of tiles; every bound of the validation; and one printed plan per point, which
// tests/test_nms_cpu.py compares with its Python mirror.  SAN=1 builds it under AddressSanitizer / UBSan (host/Makefile).
//   nms_plan_check
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../csrc/nms_plan.h"

using namespace dfx;

static unsigned long long g_state = 88172645463325252ull;
static unsigned long long rnd() {
  g_state ^= g_state << 13;
  g_state ^= g_state >> 7;
  g_state ^= g_state << 17;
  return g_state;
}

static int g_bad = 0;
#define CHECK(cond, ...)                         \
  do {                                           \
    if (!(cond)) {                               \
      printf("FAILED %s:%d: ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);                       \
      printf("\n");                              \
      ++g_bad;                                   \
    }                                            \
  } while (0)

// S[i][j], i < j: i suppresses j.  kind 0 random with density 1/den, 1 empty, 2 full, 3 block-diagonal (inside 64-blocks only),
// 4 only across blocks
static std::vector<std::vector<char> > make_relation(int n, int kind, int den) {
  std::vector<std::vector<char> > S(n, std::vector<char>(n, 0));
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j) {
      const bool same = i / NMS_TILE == j / NMS_TILE;
      const bool hit = rnd() % den == 0;
      S[i][j] = kind == 1 ? 0 : kind == 2 ? 1 : kind == 3 ? (same && hit) : kind == 4 ? (!same && hit) : hit;
    }
  return S;
}

static std::vector<int> brute(const std::vector<std::vector<char> > &S, const std::vector<char> &valid, int nv, int max_out) {
  std::vector<int> keep;
  for (int j = 0; j < nv && (int)keep.size() < max_out; ++j) {
    if (!valid[j]) continue;
    bool sup = false;
    for (int i : keep) sup = sup || S[i][j];
    if (!sup) keep.push_back(j);
  }
  return keep;
}

// the scan kernel's walk on the host: mask [n64 * 64][n64] words, only the upper triangle filled
static std::vector<int> scan(const std::vector<std::vector<char> > &S, const std::vector<char> &valid, int n, int nv, int max_out) {
  const int n64 = nms_blocks(n), per = n64 * NMS_TILE;
  std::vector<uint64_t> mask((size_t)per * n64, ~(uint64_t)0);  // (unwritten words hold garbage)
  std::vector<uint16_t> tiles(nms_tiles(n));
  nms_enumerate_tiles(n, tiles.data());
  for (uint16_t t : tiles) {
    const int rb = t & 0xff, cb = t >> 8;
    if (cb * NMS_TILE >= nv) continue;
    for (int l = 0; l < NMS_TILE; ++l) {
      const int row = rb * NMS_TILE + l;
      uint64_t w = 0;
      for (int c = 0; c < NMS_TILE; ++c) {
        const int col = cb * NMS_TILE + c;
        if (row < nv && col < nv && col > row && valid[row] && valid[col] && S[row][col]) w |= (uint64_t)1 << c;
      }
      mask[(size_t)row * n64 + cb] = w;
    }
  }
  std::vector<int> keep;
  uint64_t removed[NMS_MAX_BLOCKS] = {0};
  const int nb = (nv + NMS_TILE - 1) / NMS_TILE;
  int cnt = 0;
  for (int b = 0; b < nb && cnt < max_out; ++b) {
    uint64_t diag[NMS_TILE], v = 0;
    for (int l = 0; l < NMS_TILE; ++l) {
      diag[l] = mask[(size_t)(b * NMS_TILE + l) * n64 + b];
      const int row = b * NMS_TILE + l;
      if (row < nv && valid[row]) v |= (uint64_t)1 << l;
    }
    const uint64_t kept = nms_block_scan(diag, v & ~removed[b], max_out - cnt);
    for (int l = 0; l < NMS_TILE; ++l)
      if (kept >> l & 1) {
        keep.push_back(b * NMS_TILE + l);
        for (int w = b + 1; w < nb; ++w) removed[w] |= mask[(size_t)(b * NMS_TILE + l) * n64 + w];
      }
    cnt = (int)keep.size();
  }
  return keep;
}

static void check_scan() {
  int cases = 0;
  const int ns[] = {1, 2, 63, 64, 65, 127, 128, 130, 200, 257};
  for (int rep = 0; rep < 60; ++rep)
    for (int n : ns)
      for (int kind = 0; kind < 5; ++kind) {
        const int den = 2 + (int)(rnd() % 40);
        std::vector<std::vector<char> > S = make_relation(n, kind, den);
        std::vector<char> valid(n, 1);
        if (rep % 3 == 1)
          for (int i = 0; i < n; ++i) valid[i] = rnd() % 5 != 0;
        const int nvs[] = {n, (int)(rnd() % (n + 1)), 0};
        for (int nv : nvs) {
          const std::vector<int> all = brute(S, valid, nv, n);
          const int k = (int)all.size();
          const int outs[] = {1, k > 1 ? k - 1 : 1, k > 0 ? k : 1, k + 1 <= n ? k + 1 : n, n};
          for (int mo : outs) {
            const std::vector<int> want = brute(S, valid, nv, mo), got = scan(S, valid, n, nv, mo);
            CHECK(want == got, "scan n %d nv %d kind %d max_out %d: %zu kept against %zu", n, nv, kind, mo, got.size(), want.size());
            ++cases;
          }
        }
      }
  // the block step alone: budget, empty candidates, a row that removes everything
  uint64_t diag[NMS_TILE];
  for (int t = 0; t < NMS_TILE; ++t) diag[t] = t == 63 ? 0 : ~(uint64_t)0 << (t + 1);
  CHECK(nms_block_scan(diag, ~(uint64_t)0, 64) == 1, "full tile");
  CHECK(nms_block_scan(diag, ~(uint64_t)1, 64) == 2, "full tile without row 0");
  CHECK(nms_block_scan(diag, 0, 64) == 0, "no candidates");
  memset(diag, 0, sizeof(diag));
  CHECK(nms_block_scan(diag, ~(uint64_t)0, 64) == ~(uint64_t)0, "empty tile");
  CHECK(nms_block_scan(diag, ~(uint64_t)0, 3) == 7, "budget 3");
  CHECK(nms_block_scan(diag, (uint64_t)1 << 63, 1) == (uint64_t)1 << 63, "row 63");
  cases += 6;
  printf("scan: %d cases against the brute-force greedy walk\n", cases);
}

static void check_tiles() {
  for (int n = 1; n <= DFX_NMS_MAX_N; n += (n < 300 ? 1 : 97)) {
    const int b = nms_blocks(n);
    std::vector<uint16_t> t(nms_tiles(n));
    CHECK(nms_enumerate_tiles(n, t.data()) == (int)t.size() && (int)t.size() == b * (b + 1) / 2, "tile count n %d", n);
    std::vector<char> seen((size_t)b * b, 0);
    for (uint16_t e : t) {
      const int rb = e & 0xff, cb = e >> 8;
      CHECK(rb <= cb && cb < b && !seen[(size_t)rb * b + cb], "tile (%d, %d) of n %d", rb, cb, n);
      if (rb < b && cb < b) seen[(size_t)rb * b + cb] = 1;
    }
  }
  CHECK(nms_blocks(DFX_NMS_MAX_N) == NMS_MAX_BLOCKS && NMS_MAX_BLOCKS == 64, "one u64 per lane");
  printf("tiles: ok\n");
}

static dfx_nms_desc good() {
  dfx_nms_desc d;
  memset(&d, 0, sizeof(d));
  d.bs = 2; d.n = 100; d.max_out = 50; d.keep_ld = 50; d.mode = DFX_NMS_DECODE; d.per_class = 1; d.classes = 80;
  d.anchors_per_pixel = 9; d.n_anchors = 1000; d.row_bytes = 36; d.idx_ld = 100; d.iou_thr = 0.5f; d.force_path = -1;
  return d;
}
#define BAD(stmt)                                                  \
  do {                                                             \
    dfx_nms_desc d = good();                                       \
    stmt;                                                          \
    CHECK(nms_validate(d, nullptr) == DFX_ERR_INVALID, "accepted: %s", #stmt); \
    ++n_bad;                                                       \
  } while (0)
#define GOOD(stmt)                                                 \
  do {                                                             \
    dfx_nms_desc d = good();                                       \
    stmt;                                                          \
    const char *why;                                               \
    CHECK(nms_validate(d, &why) == DFX_OK, "refused (%s): %s", why, #stmt); \
  } while (0)

static void check_validation() {
  int n_bad = 0;
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  GOOD((void)0);
  BAD(d.bs = 0); BAD(d.n = 0); BAD(d.n = 4097); GOOD(d.n = 4096; d.idx_ld = 4096); BAD(d.max_out = 0); BAD(d.max_out = 101);
  GOOD(d.max_out = 100; d.keep_ld = 100); BAD(d.keep_ld = 49); BAD(d.mode = 2); BAD(d.mode = -1); BAD(d.per_class = 2);
  BAD(d.force_path = 2); BAD(d.force_path = -2); GOOD(d.force_path = DFX_NMS_MASK); GOOD(d.force_path = DFX_NMS_GENERIC);
  BAD(d.classes = 0); BAD(d.anchors_per_pixel = 0); BAD(d.n_anchors = 0);
  BAD(d.n_anchors = 26843546; d.classes = 80); GOOD(d.n_anchors = 26843545; d.classes = 80); GOOD(d.n_anchors = 2147483647; d.classes = 1);
  BAD(d.iou_thr = inf); BAD(d.iou_thr = -inf); BAD(d.iou_thr = nan); GOOD(d.iou_thr = -1.f); GOOD(d.iou_thr = 2.f);
  BAD(d.idx_ld = 99); BAD(d.row_bytes = 35); GOOD(d.row_bytes = 1024); BAD(d.clip_w = nan); BAD(d.clip_h = nan);
  BAD(d.clip_w = 10.f; d.clip_h = -1.f); GOOD(d.clip_w = 10.f; d.clip_h = 0.f); GOOD(d.clip_w = 0.f; d.clip_h = -5.f);
  // BOXES mode reads idx only with per_class, and none of the decode fields
  GOOD(d.mode = DFX_NMS_BOXES; d.per_class = 0; d.idx_ld = 0; d.row_bytes = 0; d.clip_w = nan);
  BAD(d.mode = DFX_NMS_BOXES; d.idx_ld = 99);
  printf("validation: %d refusals\n", n_bad);
}

int main() {
  check_scan();
  check_tiles();
  check_validation();
  const int pts[][2] = {{1, 1}, {3, 63}, {1, 64}, {3, 65}, {2, 128}, {1, 130}, {8, 1000}, {1, 2000}, {8, 200}, {1, 4096}, {8, 4096}};
  for (const auto &p : pts) {
    const NmsScratch s = nms_scratch(p[0], p[1]);
    CHECK(s.off_lab % 16 == 0 && s.off_mask % 16 == 0 && s.off_tiles % 8 == 0 && s.bytes % 16 == 0, "scratch alignment");
    printf("plan bs=%d n=%d : blocks=%d tiles=%d prep=%d mask=%d scan=%d scratch=%zu\n", p[0], p[1], nms_blocks(p[1]), nms_tiles(p[1]),
           nms_prep_grid(p[0], p[1]), nms_mask_grid(p[0], p[1]), nms_image_grid(p[0]), s.bytes);
  }
  printf("lds mask=%d generic=%d launches mask=%d generic=%d auto_min_n=%d auto_min_out=%d\n", nms_lds_bytes(DFX_NMS_MASK), nms_lds_bytes(DFX_NMS_GENERIC),
         nms_launches(DFX_NMS_MASK), nms_launches(DFX_NMS_GENERIC), NMS_MASK_AUTO_MIN_N, NMS_MASK_AUTO_MIN_OUT);
  {  // the auto rule
    dfx_nms_desc d = good();
    d.n = 200; d.idx_ld = 200; d.max_out = 100; d.keep_ld = 100;
    CHECK(nms_path(d) == DFX_NMS_MASK, "auto at n 200, max_out 100");
    d.max_out = 99;
    CHECK(nms_path(d) == DFX_NMS_GENERIC, "auto at max_out 99");
    d.max_out = 100; d.n = 199;
    CHECK(nms_path(d) == DFX_NMS_GENERIC, "auto at n 199");
    d.force_path = DFX_NMS_MASK;
    CHECK(nms_path(d) == DFX_NMS_MASK, "forced");
  }
  if (g_bad) {
    printf("nms_plan_check: %d checks FAILED\n", g_bad);
    return 1;
  }
  printf("nms_plan_check: ok\n");
  return 0;
}
