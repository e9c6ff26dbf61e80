// se_plan_check.cc -- host-only view of the squeeze kernel's plan (csrc/se_plan.h): no GPU, no HIP.  Walks a sweep of
// shapes, device sizes and forced slice counts and checks what the kernel relies on: the slices cover every pixel of
// an image exactly once and none is empty; the lanes of a workgroup cover every pixel of their slice exactly once; a
// lane's packed accumulators take at most 257 pixels between two flushes; the lane layout fits the workgroup and the
// second reduction stage fits its LDS array; the planner's own slices have at least 64 pixels.  Part of `make all`;
// SAN=1 builds it under AddressSanitizer / UBSan:
//   make -B ../tools/se_plan_check SAN=1 && ../tools/se_plan_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../csrc/se_plan.h"

using namespace dfx;

// the kernel's walk of one lane: pixels p0 + pl, + pln, ... in runs of at most SE_FLUSH; marks what it visits
static int walk_lane(int p0, int p1, int pl, int pln, std::vector<unsigned char> *seen, int *longest) {
  int visited = 0;
  int p = p0 + pl;
  while (p < p1) {
    int run = 0;
    for (int k = 0; k < SE_FLUSH && p < p1; ++k, p += pln) {
      if (seen) ++(*seen)[(size_t)(p - p0)];
      ++run;
    }
    if (run > *longest) *longest = run;
    visited += run;
  }
  return visited;
}

static int check_plan(long long bs, int px, int c, int cus, long long forced) {
  const SePlan p = se_plan(bs, px, c, cus, forced);
  if (p.groups != c / 16 || p.gl < 1 || p.gl > SE_THREADS || p.gl * p.gchunks < p.groups || p.gl * (p.gchunks - 1) >= p.groups) return 1;
  if (p.pln < 1 || p.gl * p.pln > SE_THREADS) return 2;
  if (p.parts < 1 || p.parts > p.pln || (p.parts > 1 && 16 * p.gl * p.parts > SE_THREADS)) return 3;
  if (p.slices < 1 || p.slices > px) return 4;
  if (forced > 0 && p.slices != (forced < px ? forced : px)) return 5;
  if (forced <= 0 && p.slices > 1 && px / p.slices < SE_MIN_SLICE_PX) return 6;
  if (forced <= 0 && p.slices == 1 && bs * p.gchunks < 2ll * cus && px >= 2 * SE_MIN_SLICE_PX) return 7;  // more work was there to cut
  if (p.items != bs * p.slices * p.gchunks) return 8;
  if (se_slice_begin(px, p.slices, 0) != 0 || se_slice_begin(px, p.slices, p.slices) != px) return 9;
  // every slice, or a sample of them where there are very many
  const int step = p.slices > 4096 ? p.slices / 1024 : 1;
  for (int s = 0; s < p.slices; s += (s < 512 || s >= p.slices - 512) ? 1 : step) {
    const int p0 = se_slice_begin(px, p.slices, s), p1 = se_slice_begin(px, p.slices, s + 1);
    if (p1 <= p0) return 10;  // empty, or pixels out of order
    std::vector<unsigned char> seen((size_t)(p1 - p0), 0);
    int total = 0, longest = 0;
    for (int pl = 0; pl < p.pln; ++pl) {
      const int n = walk_lane(p0, p1, pl, p.pln, &seen, &longest);
      if (n != se_lane_pixels(p0, p1, pl, p.pln)) return 11;
      total += n;
    }
    if (total != p1 - p0) return 12;
    for (unsigned char v : seen)
      if (v != 1) return 13;
    if (longest > SE_FLUSH || longest != se_flush_run(se_lane_pixels(p0, p1, 0, p.pln))) return 14;
  }
  return 0;
}

int main() {
  static const int pxs[] = {1, 2, 9, 45, 49, 63, 64, 127, 128, 196, 256, 257, 258, 514, 561, 784, 3136, 12544, 65793, 1 << 20, SE_MAX_PX};
  static const int cs[] = {16, 32, 48, 64, 96, 144, 240, 480, 672, 1152, 2048, 4096, 4112, 16384};
  static const long long bss[] = {1, 2, 3, 32, 64, 1000};
  static const int cuss[] = {1, 80, 256, 304};
  static const long long forced[] = {0, 1, 2, 3, 7, 1000000, 1ll << 40};
  int cases = 0, bad = 0;
  for (int px : pxs)
    for (int c : cs)
      for (long long bs : bss)
        for (int cus : cuss)
          for (long long f : forced) {
            // (the long walks on a few shapes only)
            if (px > 65793 && !(bs == 1 && cus == 256 && (f == 0 || f == 3) && (c == 16 || c == 1152 || c == 16384))) continue;
            ++cases;
            const int rc = check_plan(bs, px, c, cus, f);
            if (rc) {
              ++bad;
              printf("FAIL (%d) bs %lld px %d c %d cus %d forced %lld\n", rc, bs, px, c, cus, f);
            }
          }
  // a forced count of every pixel: one-pixel slices
  for (int px : {1, 5, 257, 4097}) {
    ++cases;
    const int rc = check_plan(2, px, 32, 256, px);
    if (rc) {
      ++bad;
      printf("FAIL (%d) one-pixel slices of %d pixels\n", rc, px);
    }
  }
  if (bad) return 1;
  printf("all %d squeeze plans cover every pixel exactly once, leave no slice empty and flush within %d pixels\n", cases, SE_FLUSH);
  return 0;
}
