// select_plan_check -- host-only check of csrc/select_plan.h (no GPU, no HIP): the image-wide top-K's descriptor
// validation, the chunk plan and scratch layout, and the threshold / quota scan over a histogram slab against a brute-force
// sort.  Part of `all`; `make -B ../tools/select_plan_check SAN=1` builds it under AddressSanitizer / UBSan.
// It prints one "plan ..." line per point of tests/select_ref.py's plan_points(), which tests/test_select_cpu.py compares
// with the Python mirror, and "select_plan_check: ok" at the end.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../csrc/select_plan.h"

using namespace dfx;

static int g_fail = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);             \
      ++g_fail;                                                            \
    }                                                                      \
  } while (0)

static unsigned rnd_state = 12345;
static unsigned rnd() {
  rnd_state = rnd_state * 1664525u + 1013904223u;
  return rnd_state >> 8;
}

struct Cand {
  int key, chunk, ord;
};

// one slab of `chunks` histograms and k: the scan against "sort all candidates by (key descending, position ascending),
// take the first k"
static void scan_case(const std::vector<unsigned> &slab, int chunks, int k) {
  std::vector<unsigned> total(SELECT_BINS, 0);
  for (int c = 0; c < chunks; ++c)
    for (int b = 0; b < SELECT_BINS; ++b) total[b] += slab[(size_t)c * SELECT_BINS + b];
  const SelectThreshold th = select_threshold(total.data(), k);
  std::vector<unsigned> gt(chunks), eq(chunks), plan((size_t)SELECT_CHUNK_WORDS * chunks);
  for (int c = 0; c < chunks; ++c) {
    unsigned g = 0;
    for (int b = th.t + 1; b < SELECT_BINS; ++b) g += slab[(size_t)c * SELECT_BINS + b];
    gt[c] = g;
    eq[c] = slab[(size_t)c * SELECT_BINS + th.t];
  }
  select_chunk_offsets(gt.data(), eq.data(), chunks, th.n_gt, th.quota, plan.data());

  // brute force: positions are ordered by (chunk, ordinal inside the chunk); which ordinal a key has inside its chunk
  // does not matter for the counts checked here, so the keys of a chunk are laid out bin by bin
  std::vector<Cand> all;
  for (int c = 0; c < chunks; ++c) {
    int ord = 0;
    for (int b = 0; b < SELECT_BINS; ++b)
      for (unsigned i = 0; i < slab[(size_t)c * SELECT_BINS + b]; ++i) all.push_back({b, c, ord++});
  }
  std::sort(all.begin(), all.end(), [](const Cand &x, const Cand &y) {
    if (x.key != y.key) return x.key > y.key;
    if (x.chunk != y.chunk) return x.chunk < y.chunk;
    return x.ord < y.ord;
  });
  const size_t want = std::min(all.size(), (size_t)k);
  CHECK(th.count == want);
  CHECK(th.n_gt + th.quota == th.count);
  CHECK(th.t >= 0 && th.t < SELECT_BINS);
  if (want) {
    CHECK(all[want - 1].key == th.t);  // the threshold key is the key of the last one taken
  } else {
    CHECK(th.t == 0 && th.quota == 0 && th.n_gt == 0);
  }
  std::vector<unsigned> took_gt(chunks, 0), took_eq(chunks, 0);
  for (size_t i = 0; i < want; ++i) {
    if (all[i].key > th.t) ++took_gt[all[i].chunk];
    else ++took_eq[all[i].chunk];
  }
  unsigned off_gt = 0, off_eq = th.n_gt;
  for (int c = 0; c < chunks; ++c) {
    CHECK(took_gt[c] == gt[c]);                                   // every key above t is taken
    CHECK(plan[SELECT_CHUNK_WORDS * c + 1] == took_eq[c]);        // the tie bin: the lowest chunks first
    CHECK(plan[SELECT_CHUNK_WORDS * c + 0] == off_gt);            // the ranges tile [0, count)
    CHECK(plan[SELECT_CHUNK_WORDS * c + 2] == off_eq);
    off_gt += gt[c];
    off_eq += took_eq[c];
  }
  CHECK(off_gt == th.n_gt && off_eq == th.count);
}

static void check_scan() {
  int cases = 0;
  for (int round = 0; round < 400; ++round) {
    const int chunks = 1 + (int)(rnd() % 6);
    std::vector<unsigned> slab((size_t)chunks * SELECT_BINS, 0);
    const int kind = round % 4;  // 0: sparse random, 1: dense in few bins, 2: all equal, 3: empty or nearly
    size_t n = 0;
    for (int c = 0; c < chunks; ++c) {
      if (kind == 0) {
        for (int i = 0; i < 12; ++i) slab[(size_t)c * SELECT_BINS + rnd() % SELECT_BINS] += rnd() % 4;
      } else if (kind == 1) {
        for (int i = 0; i < 3; ++i) slab[(size_t)c * SELECT_BINS + 100 + rnd() % 3] += rnd() % 40;
      } else if (kind == 2) {
        slab[(size_t)c * SELECT_BINS + 77] = 1 + rnd() % 30;
      } else if (rnd() % 3 == 0) {
        slab[(size_t)c * SELECT_BINS + (rnd() % 2 ? 0 : 255)] = rnd() % 2;
      }
    }
    for (unsigned v : slab) n += v;
    const int ks[] = {1, 2, 7, (int)n - 1, (int)n, (int)n + 1, (int)(n / 2), 4096, 1 + (int)(rnd() % 64)};
    for (int k : ks) {
      if (k < 1 || k > DFX_SELECT_MAX_K) continue;
      scan_case(slab, chunks, k);
      ++cases;
    }
  }
  printf("scan: %d cases against the brute-force sort\n", cases);
}

static dfx_select_desc base_desc() {
  dfx_select_desc d;
  memset(&d, 0, sizeof(d));
  d.bs = 2; d.h = 5; d.w = 7; d.c = 21; d.src_ld = 32; d.src_dt = DFX_U8; d.k = 100; d.idx_ld = 100;
  d.peak = DFX_SELECT_PEAK3; d.min_val = 0; d.n_gather = 0; d.force_path = -1;
  return d;
}

static void check_validate() {
  dfx_select_desc d = base_desc();
  CHECK(select_validate(d, nullptr) == DFX_OK);
  CHECK(select_hist_class(d) && select_path(d) == DFX_SELECT_GENERIC);  // 5 * 7 * 32 bytes: below the auto rule's 4096
  d.h = 8; d.w = 16;
  CHECK(select_path(d) == DFX_SELECT_HIST);                              // 4096 bytes
  d.w = 15;
  CHECK(select_path(d) == DFX_SELECT_GENERIC);
  d.w = 64; d.c = 33; d.src_ld = 33;
  CHECK(select_path(d) == DFX_SELECT_GENERIC);                           // outside the class at any size
  d.force_path = DFX_SELECT_GENERIC; d.c = 21; d.src_ld = 32;
  CHECK(select_path(d) == DFX_SELECT_GENERIC);
  d = base_desc();
#define BAD(stmt, code)                        \
  do {                                         \
    dfx_select_desc b = base_desc();           \
    stmt;                                      \
    const char *why = nullptr;                 \
    CHECK(select_validate(b, &why) == (code)); \
    CHECK(why && *why);                        \
  } while (0)
  BAD(b.bs = 0, DFX_ERR_INVALID);
  BAD(b.h = 0, DFX_ERR_INVALID);
  BAD(b.w = -1, DFX_ERR_INVALID);
  BAD(b.c = 0, DFX_ERR_INVALID);
  BAD(b.c = 65536; b.src_ld = 65536, DFX_ERR_INVALID);
  BAD(b.src_ld = 20, DFX_ERR_INVALID);
  BAD(b.src_ld = 65536, DFX_ERR_INVALID);
  BAD(b.src_dt = 9, DFX_ERR_INVALID);
  BAD(b.src_dt = DFX_UNDEF, DFX_ERR_INVALID);
  BAD(b.k = 0, DFX_ERR_INVALID);
  BAD(b.k = 4097; b.idx_ld = 4097, DFX_ERR_INVALID);
  BAD(b.idx_ld = 99, DFX_ERR_INVALID);
  BAD(b.peak = 2, DFX_ERR_INVALID);
  BAD(b.force_path = 2, DFX_ERR_INVALID);
  BAD(b.force_path = -2, DFX_ERR_INVALID);
  BAD(b.min_val = 256, DFX_ERR_INVALID);
  BAD(b.min_val = -1, DFX_ERR_INVALID);
  BAD(b.src_dt = DFX_S8; b.min_val = 128, DFX_ERR_INVALID);
  BAD(b.src_dt = DFX_S8; b.min_val = -129, DFX_ERR_INVALID);
  BAD(b.n_gather = 5, DFX_ERR_INVALID);
  BAD(b.n_gather = -1, DFX_ERR_INVALID);
  BAD(b.n_gather = 1; b.row_bytes[0] = 0; b.pixel_stride_bytes[0] = 8, DFX_ERR_INVALID);
  BAD(b.n_gather = 1; b.row_bytes[0] = 1025; b.pixel_stride_bytes[0] = 2048, DFX_ERR_INVALID);
  BAD(b.n_gather = 2; b.row_bytes[0] = 8; b.pixel_stride_bytes[0] = 8; b.row_bytes[1] = 8; b.pixel_stride_bytes[1] = 7, DFX_ERR_INVALID);
  BAD(b.h = 65536; b.w = 32768; b.c = 1; b.src_ld = 1, DFX_ERR_INVALID);           // h * w * c = 2^31
  BAD(b.bs = 2; b.h = 46341; b.w = 46341; b.c = 1; b.src_ld = 512, DFX_ERR_INVALID);  // bs * h * w * src_ld > 2^40
  BAD(b.h = 2147483647; b.w = 2147483647, DFX_ERR_INVALID);
  BAD(b.src_dt = DFX_S32, DFX_ERR_UNSUPPORTED);
  BAD(b.src_dt = DFX_F32; b.min_val = -5, DFX_ERR_UNSUPPORTED);
  BAD(b.src_dt = DFX_F32; b.k = 0, DFX_ERR_INVALID);  // everything invalid is found before anything unsupported
#undef BAD
  // the limits themselves are admitted
  d = base_desc();
  d.h = 1; d.w = 2147483647; d.c = 1; d.src_ld = 1; d.bs = 512;  // 2^31 - 1 elements per image, bs * .. just below 2^40
  CHECK(select_validate(d, nullptr) == DFX_OK);
  d = base_desc();
  d.src_dt = DFX_S8; d.min_val = -128; d.k = 4096; d.idx_ld = 4096; d.n_gather = 4;
  for (int i = 0; i < 4; ++i) { d.row_bytes[i] = 1024; d.pixel_stride_bytes[i] = 65536; }
  CHECK(select_validate(d, nullptr) == DFX_OK);
  d.src_ld = 33; d.c = 33;
  CHECK(!select_hist_class(d));
  // extents and overlap
  d = base_desc();
  CHECK(select_src_extent(d) == (2ull * 35 - 1) * 32 + 21);
  CHECK(select_idx_extent(d, 4) == (100ull + 100) * 4 && select_idx_extent(d, 1) == 200);
  d.n_gather = 1; d.row_bytes[0] = 8; d.pixel_stride_bytes[0] = 12;
  CHECK(select_gather_src_extent(d, 0) == 69ull * 12 + 8 && select_gather_dst_extent(d, 0) == 2ull * 100 * 8);
  CHECK(plan_overlap(100, 10, 109, 1) && !plan_overlap(100, 10, 110, 1) && !plan_overlap(100, 10, 90, 10) && plan_overlap(100, 10, 90, 11));
  CHECK(select_algorithmic_bytes(d) == 2ull * 35 * 21 + 2 * 100 * 4 + 2 * 4 + 2ull * 2 * 100 * 8);
  CHECK(select_sort_size(1) == 64 && select_sort_size(64) == 64 && select_sort_size(65) == 128 && select_sort_size(4096) == 4096);
  CHECK(select_key8(0x80, DFX_S8) == 0 && select_key8(0x7f, DFX_S8) == 255 && select_key8(0xff, DFX_U8) == 255 && select_key8(select_key8(0x91, DFX_S8), DFX_S8) == 0x91);
}

static void print_plan(int bs, long long px, int ld, int cus, long long forced) {
  const SelectPlan p = select_plan(bs, px, ld, cus, forced);
  const SelectScratch s = select_scratch(bs, p.chunks, 100);
  CHECK(p.chunk_px >= 1 && p.chunks >= 1 && p.chunks <= SELECT_MAX_CHUNKS);
  CHECK((long long)p.chunk_px * p.chunks >= px && (long long)p.chunk_px * (p.chunks - 1) < px);  // the chunks tile the image, none is empty
  CHECK(p.grid >= 1 && p.grid <= SELECT_MAX_GRID && p.items == (long long)bs * p.chunks);
  CHECK(s.off_plan % 16 == 0 && s.off_cand % 16 == 0 && s.off_plan >= (size_t)bs * p.chunks * SELECT_BINS * 4 && s.bytes >= s.off_cand + (size_t)bs * 100 * 8);
  printf("plan bs=%d px=%lld ld=%d cus=%d forced=%lld : chunk_px=%d chunks=%d items=%lld grid=%d scratch=%zu\n", bs, px, ld, cus, forced,
         p.chunk_px, p.chunks, p.items, p.grid, s.bytes);
}

static void check_plans() {
  // the shapes of the test tables (tests/select_ref.py: SHAPES x the 16-byte leading dimensions of CLD, bs 3, the three
  // chunk settings), the benchmark's points and a few at the clamps
  const int shapes[5][2] = {{5, 7}, {1, 1}, {1, 9}, {9, 1}, {13, 16}};
  const int lds[4] = {80, 32, 16, 96};
  for (auto &hw : shapes)
    for (int ld : lds) {
      const long long forced[3] = {1, std::max(1, 2 * hw[1] - 1), 0};
      for (long long f : forced) print_plan(3, (long long)hw[0] * hw[1], ld, 256, f);
    }
  print_plan(1, 128 * 128, 80, 256, 0);
  print_plan(8, 128 * 128, 80, 256, 0);
  print_plan(32, 128 * 128, 80, 256, 0);
  print_plan(1, 100 * 136, 720, 256, 0);
  print_plan(8, 100 * 136, 720, 256, 0);
  print_plan(1, 200 * 304, 16, 256, 0);
  print_plan(128, 1, 1008, 256, 0);
  print_plan(1, 1, 1008, 304, 0);
  print_plan(2, 3000000, 16, 256, 0);
  print_plan(2, 3000000, 16, 256, 5);  // a forced chunk size is raised until an image has at most 1024 chunks
  print_plan(1000, 64, 16, 8, 0);
  printf("lds hist=%d generic=%d launches hist=%d generic=%d\n", select_lds_bytes(DFX_SELECT_HIST), select_lds_bytes(DFX_SELECT_GENERIC),
         select_launches(DFX_SELECT_HIST), select_launches(DFX_SELECT_GENERIC));
  CHECK(select_lds_hist() <= 65536 && select_lds_scan() <= 65536 && select_lds_generic() <= 65536 && select_lds_sort() <= 65536);
}

int main() {
  check_scan();
  check_validate();
  check_plans();
  if (g_fail) {
    printf("select_plan_check: %d FAILED\n", g_fail);
    return 1;
  }
  printf("select_plan_check: ok\n");
  return 0;
}
