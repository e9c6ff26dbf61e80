// fc_pack_check -- host-only check of the fully-connected op's weight packer (csrc/fc_pack.h), meant to be built with
// the host sanitizers; it needs no GPU and no HIP:
//   g++ -std=c++11 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/fc_pack_check.cc -o tools/fc_pack_check
// Packs (oc, ic, ih, iw) shapes with full and partial oc blocks from weights without a zero byte, into a buffer of
// exactly fc_pack_bytes() bytes, and checks every byte of the image against a plain index formula: byte b of lane
// `lane` of fragment j of k-step ks of block ob is w[o][c][y][x] with o = 32 ob + lane % 32 and
// (y * iw + x) * ic + c = 64 ks + 32 j + 16 (lane / 32) + b, zero for the padding rows o >= oc, and every weight
// lands exactly once.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../csrc/fc_pack.h"

int main() {
  const int shapes[][4] = {{1, 64, 1, 1},  {10, 64, 1, 1}, {32, 192, 1, 1}, {33, 16, 2, 2},  {96, 64, 1, 3}, {130, 64, 7, 7},
                           {33, 2048, 1, 1}, {7, 32, 2, 3}, {64, 4, 4, 4},   {1000, 128, 1, 1}, {5, 2, 8, 4},  {40, 16, 3, 4}};
  unsigned seed = 4321;
  for (const auto &sh : shapes) {
    const int oc = sh[0], ic = sh[1], ih = sh[2], iw = sh[3], K = ic * ih * iw, nks = K / 64;
    if (K % 64) {
      printf("shape oc %d ic %d %dx%d: K = %d is outside the class\n", oc, ic, ih, iw, K);
      return 1;
    }
    std::vector<int8_t> w((size_t)oc * K);
    for (auto &v : w) {
      seed = seed * 1664525u + 1013904223u;
      const int x = (int)(seed >> 24) - 128;
      v = (int8_t)(x == 0 ? 77 : x);  // no zero weights: a zero in the image is a padding byte
    }
    const size_t bytes = dfx::fc_pack_bytes(oc, K);
    std::vector<unsigned char> img(bytes, 0xEE);  // exactly sized: the sanitizer sees a byte too many
    dfx::fc_pack(w.data(), oc, ic, ih, iw, img.data());
    size_t nonzero = 0;
    const int nob = (oc + 31) / 32;
    if (bytes != (size_t)nob * nks * 2048) {
      printf("oc %d K %d: %zu bytes, want %zu\n", oc, K, bytes, (size_t)nob * nks * 2048);
      return 1;
    }
    for (int ob = 0; ob < nob; ++ob)
      for (int ks = 0; ks < nks; ++ks)
        for (int j = 0; j < 2; ++j)
          for (int lane = 0; lane < 64; ++lane)
            for (int b = 0; b < 16; ++b) {
              const int o = 32 * ob + lane % 32, k = 64 * ks + 32 * j + 16 * (lane / 32) + b;
              const int c = k % ic, pix = k / ic, x = pix % iw, y = pix / iw;
              const unsigned char got = img[((((size_t)ob * nks + ks) * 2 + j) * 64 + lane) * 16 + b];
              const unsigned char want = o < oc ? (unsigned char)w[(((size_t)o * ic + c) * ih + y) * iw + x] : 0;
              if (got != want) {
                printf("oc %d ic %d %dx%d: block %d k-step %d fragment %d lane %d byte %d (o %d c %d y %d x %d): got %u want %u (%s)\n",
                       oc, ic, ih, iw, ob, ks, j, lane, b, o, c, y, x, got, want, o < oc ? "weight" : "PADDING ROW");
                return 1;
              }
              nonzero += got != 0;
            }
    if (nonzero != w.size()) {
      printf("oc %d K %d: %zu weights in the image, %zu given\n", oc, K, nonzero, w.size());
      return 1;
    }
    printf("oc %4d ic %4d %dx%d: %8zu bytes, %7zu weights in place, %6zu padding bytes zero\n", oc, ic, ih, iw, bytes, nonzero,
           bytes - nonzero);
  }
  printf("fc_pack_check: all %zu shapes packed, every padding row zero\n", sizeof(shapes) / sizeof(shapes[0]));
  return 0;
}
