// imgconv_pack_check -- host-only check of the first-layer conv's weight packer (csrc/imgconv_pack.h), meant to be built
// with the host sanitizers; it needs no GPU and no HIP:
//   g++ -std=c++11 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/imgconv_pack_check.cc -o tools/imgconv_pack_check
// Packs every (window, ic, oc) of the MFMA kernel's class from weights without a zero byte, into a buffer of exactly
// imgconv_pack_bytes() bytes, and checks every byte of the image against the K layout written out here a second time,
// independently of imgconv_pack_tap: a live byte is the weight the layout names, every other byte (the 8th tap of a 7x7
// row, the 4th tap of a 3x3 row, the upper half of the 3x3's second step, the 4th channel of a 3-channel pixel) is
// zero, and every weight lands exactly once.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../csrc/imgconv_pack.h"

int main() {
  unsigned seed = 4321;
  int nshapes = 0;
  for (int k : {7, 3})
    for (int ic : {3, 4})
      for (int oc : {32, 64, 96, 128}) {
        const int nt = dfx::imgconv_pack_steps(k);
        if (nt != (k == 7 ? 7 : 2)) {
          printf("k %d: %d steps\n", k, nt);
          return 1;
        }
        std::vector<int8_t> w((size_t)oc * ic * k * k);
        for (auto &v : w) {
          seed = seed * 1664525u + 1013904223u;
          const int x = (int)(seed >> 24) - 128;
          v = (int8_t)(x == 0 ? 77 : x);  // no zero weights: a zero in the image is a dead byte
        }
        const size_t bytes = dfx::imgconv_pack_bytes(oc, k);
        std::vector<unsigned char> img(bytes, 0xEE);  // exactly sized: the sanitizer sees a byte too many
        dfx::imgconv_pack(w.data(), oc, ic, k, img.data());
        size_t nonzero = 0;
        for (int ob = 0; ob < oc / 32; ++ob)
          for (int t = 0; t < nt; ++t)
            for (int lane = 0; lane < 64; ++lane)
              for (int b = 0; b < 16; ++b) {
                const int o = 32 * ob + (lane & 31), h = lane >> 5, j = b >> 2, c = b & 3;
                int ky, kx;
                bool live;
                if (k == 7) {
                  ky = t;
                  kx = 4 * h + j;
                  live = kx <= 6;
                } else if (t == 0) {
                  ky = h;
                  kx = j;
                  live = j <= 2;
                } else {
                  ky = 2;
                  kx = j;
                  live = j <= 2 && h == 0;
                }
                live = live && c < ic;
                const unsigned char got = img[(((size_t)ob * nt + t) * 64 + lane) * 16 + b];
                const unsigned char want = live ? (unsigned char)w[(((size_t)o * ic + c) * k + ky) * k + kx] : 0;
                if (got != want) {
                  printf("k %d ic %d oc %d: block %d step %d lane %d byte %d: got %u want %u (%s)\n", k, ic, oc, ob, t, lane, b, got,
                         want, live ? "live" : "DEAD BYTE");
                  return 1;
                }
                nonzero += got != 0;
              }
        if (nonzero != w.size()) {
          printf("k %d ic %d oc %d: %zu weights in the image, %zu given\n", k, ic, oc, nonzero, w.size());
          return 1;
        }
        printf("k %d ic %d oc %3d: %6zu bytes, %5zu weights in place, %6zu dead bytes zero\n", k, ic, oc, bytes, nonzero, bytes - nonzero);
        ++nshapes;
      }
  printf("imgconv_pack_check: all %d shapes packed, every dead byte zero\n", nshapes);
  return 0;
}
