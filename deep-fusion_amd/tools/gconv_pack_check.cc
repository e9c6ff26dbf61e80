// gconv_pack_check -- host-only check of the grouped conv's weight packer (csrc/gconv_pack.h), meant to be built with
// the host sanitizers; it needs no GPU and no HIP:
//   g++ -std=c++11 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/gconv_pack_check.cc -o tools/gconv_pack_check
// Packs every (c, cpg) the MFMA kernel's tests use from weights without a zero byte, into a buffer of exactly
// gconv_pack_bytes() bytes, and checks every byte of the image: inside the output channel's group it is the weight the
// header's formula names, outside it is zero, and every weight lands exactly once.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../csrc/gconv_pack.h"

int main() {
  const int shapes[][2] = {{32, 4}, {32, 8}, {32, 16}, {32, 32}, {96, 4}, {96, 8}, {96, 16}, {96, 32}, {128, 4}, {128, 8},
                           {128, 16}, {128, 32}, {160, 4}, {160, 8}, {160, 16}, {160, 32}, {256, 4}, {256, 8}, {256, 16},
                           {256, 32}, {64, 64}, {128, 64}, {192, 64}};
  unsigned seed = 12345;
  for (const auto &sh : shapes) {
    const int c = sh[0], cpg = sh[1], nib = dfx::gconv_pack_nib(cpg);
    std::vector<int8_t> w((size_t)c * cpg * 9);
    for (auto &v : w) {
      seed = seed * 1664525u + 1013904223u;
      const int x = (int)(seed >> 24) - 128;
      v = (int8_t)(x == 0 ? 77 : x);  // no zero weights: a zero in the image is an off-group byte
    }
    const size_t bytes = dfx::gconv_pack_bytes(c, cpg);
    std::vector<unsigned char> img(bytes, 0xEE);  // exactly sized: the sanitizer sees a byte too many
    dfx::gconv_pack(w.data(), c, cpg, img.data());
    size_t nonzero = 0;
    for (int ob = 0; ob < c / 32; ++ob)
      for (int tap = 0; tap < 9; ++tap)
        for (int j = 0; j < nib; ++j) {
          const int ib = nib == 2 ? (ob & ~1) + j : ob;
          for (int lane = 0; lane < 64; ++lane)
            for (int b = 0; b < 16; ++b) {
              const int o = 32 * ob + (lane & 31), i = 32 * ib + 16 * (lane >> 5) + b;
              const bool in_group = i / cpg == o / cpg;
              const unsigned char got = img[((((size_t)ob * 9 + tap) * nib + j) * 64 + lane) * 16 + b];
              const unsigned char want = in_group ? (unsigned char)w[((size_t)o * cpg + i % cpg) * 9 + tap] : 0;
              if (got != want) {
                printf("c %d cpg %d: block %d tap %d input block %d lane %d byte %d: got %u want %u (%s)\n", c, cpg, ob, tap, ib,
                       lane, b, got, want, in_group ? "in group" : "OFF GROUP");
                return 1;
              }
              nonzero += got != 0;
            }
        }
    if (nonzero != w.size()) {
      printf("c %d cpg %d: %zu weights in the image, %zu given\n", c, cpg, nonzero, w.size());
      return 1;
    }
    printf("c %3d cpg %2d: %7zu bytes, %6zu weights in place, %7zu off-group bytes zero\n", c, cpg, bytes, nonzero, bytes - nonzero);
  }
  printf("gconv_pack_check: all %zu shapes packed, every off-group byte zero\n", sizeof(shapes) / sizeof(shapes[0]));
  return 0;
}
