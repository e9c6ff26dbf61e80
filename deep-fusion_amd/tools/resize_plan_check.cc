// resize_plan_check.cc -- host-only view of the activation resize's per-axis tables (csrc/resize_plan.h): no GPU, no HIP.
//   resize_plan_check <in> <out> <nearest|bilinear> <half_pixel|align_corners|asymmetric>
// prints one line per output index: "o i0 i1 w0 w1", the weights as hex floats, so that tests/test_resize_cpu.py can
// compare them bit for bit with the numpy tables of tests/resize_ref.py.  Without arguments it walks a table of sizes in
// all modes and checks what the kernels rely on: indices inside the source, i0 <= i1 <= i0 + 1, non-decreasing, weights
// in [0, 1].  Part of `make all`; SAN=1 builds it under AddressSanitizer / UBSan:
//   make -B ../tools/resize_plan_check SAN=1 && ../tools/resize_plan_check
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../csrc/resize_plan.h"

static int check_axis(int in, int out, int algo, int coord) {
  dfx::ResizeAxis t;
  if (!dfx::resize_axis_plan(in, out, algo, coord, t)) return 1;
  if ((int)t.i0.size() != out || (int)t.i1.size() != out || (int)t.w0.size() != out || (int)t.w1.size() != out) return 1;
  for (int o = 0; o < out; ++o) {
    const int a = t.i0[o], b = t.i1[o];
    if (a < 0 || b >= in || b < a || b > a + 1) return 1;
    if (o && (a < t.i0[o - 1] || b < t.i1[o - 1])) return 1;
    if (!(t.w1[o] >= 0.0f && t.w1[o] < 1.0f) || t.w0[o] != 1.0f - t.w1[o]) return 1;
    if (algo == DFX_RESIZE_NEAREST && (a != b || t.w0[o] != 1.0f || t.w1[o] != 0.0f)) return 1;
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 5) {
    const int in = atoi(argv[1]), out = atoi(argv[2]);
    const int algo = !strcmp(argv[3], "nearest") ? DFX_RESIZE_NEAREST : !strcmp(argv[3], "bilinear") ? DFX_RESIZE_BILINEAR : -1;
    const int coord = !strcmp(argv[4], "half_pixel") ? DFX_COORD_HALF_PIXEL
                      : !strcmp(argv[4], "align_corners") ? DFX_COORD_ALIGN_CORNERS
                      : !strcmp(argv[4], "asymmetric") ? DFX_COORD_ASYMMETRIC : -1;
    dfx::ResizeAxis t;
    if (!dfx::resize_axis_plan(in, out, algo, coord, t)) {
      fprintf(stderr, "resize_plan_check: no plan for in %d out %d %s %s\n", in, out, argv[3], argv[4]);
      return 2;
    }
    for (int o = 0; o < out; ++o) printf("%d %d %d %a %a\n", o, t.i0[o], t.i1[o], (double)t.w0[o], (double)t.w1[o]);
    return 0;
  }
  if (argc != 1) {
    fprintf(stderr, "usage: %s [<in> <out> <nearest|bilinear> <half_pixel|align_corners|asymmetric>]\n", argv[0]);
    return 2;
  }
  static const int sizes[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 14, 17, 23, 33, 37, 129, 513, 65535};
  const int ns = (int)(sizeof(sizes) / sizeof(sizes[0]));
  int cases = 0, bad = 0;
  for (int i = 0; i < ns; ++i)
    for (int j = 0; j < ns; ++j)
      for (int algo = 0; algo < 2; ++algo)
        for (int coord = 0; coord < 3; ++coord) {
          ++cases;
          if (check_axis(sizes[i], sizes[j], algo, coord)) {
            ++bad;
            printf("FAIL in %d out %d algo %d coord %d\n", sizes[i], sizes[j], algo, coord);
          }
        }
  dfx::ResizeAxis t;  // refused: sizes outside 1 .. 65535, unknown modes
  if (dfx::resize_axis_plan(0, 4, 0, 0, t) || dfx::resize_axis_plan(4, 65536, 0, 0, t) || dfx::resize_axis_plan(4, 4, 2, 0, t) ||
      dfx::resize_axis_plan(4, 4, 0, 3, t)) {
    ++bad;
    printf("FAIL a bad argument was planned\n");
  }
  if (bad) return 1;
  printf("all %d axis plans keep their indices inside the source and their weights in [0, 1)\n", cases);
  return 0;
}
