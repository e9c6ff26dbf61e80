// deconv_pack_check -- host-only check of the transposed conv's weight packer (csrc/deconv_pack.h), meant to be built
// with the host sanitizers; it needs no GPU and no HIP:
//   g++ -std=c++11 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/deconv_pack_check.cc -o tools/deconv_pack_check
// Packs every window of the MFMA kernel's class (2x2, 3x3, 4x4) for several (ic, oc) from weights without a zero byte,
// into a buffer of exactly deconv_pack_bytes() bytes, and checks every byte of the image against the layout written
// out here a second time, by flat byte position and independently of deconv_pack_frag: a live byte is the weight the
// layout names, the zero row / column of a 3x3 window (ky = 3 or kx = 3) is zero, and every source weight lands
// exactly once (none lost, none doubled).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../csrc/deconv_pack.h"

int main() {
  unsigned seed = 8642;
  int nshapes = 0;
  for (int k : {2, 3, 4})
    for (int ic : {32, 64, 160})
      for (int oc : {32, 96, 160}) {
        const int t = k == 2 ? 1 : 2;
        if (dfx::deconv_pack_t(k) != t) {
          printf("k %d: %d taps per axis\n", k, dfx::deconv_pack_t(k));
          return 1;
        }
        std::vector<int8_t> w((size_t)oc * ic * k * k);
        for (auto &v : w) {
          seed = seed * 1664525u + 1013904223u;
          const int x = (int)(seed >> 24) - 128;
          v = (int8_t)(x == 0 ? 77 : x);  // no zero weights: a zero in the image is a dead byte
        }
        const size_t bytes = dfx::deconv_pack_bytes(oc, ic, k);
        if (bytes != (size_t)(oc / 32) * (ic / 32) * 4 * t * t * 1024 || dfx::deconv_pack_block_bytes(ic, k) * (oc / 32) != bytes) {
          printf("k %d ic %d oc %d: %zu bytes\n", k, ic, oc, bytes);
          return 1;
        }
        std::vector<unsigned char> img(bytes, 0xEE);  // exactly sized: the sanitizer sees a byte too many
        dfx::deconv_pack(w.data(), oc, ic, k, img.data());
        std::vector<unsigned char> seen(w.size(), 0);
        size_t nonzero = 0;
        for (size_t pos = 0; pos < bytes; ++pos) {
          // [ob][s][a][b][j][l][lane][16], innermost first
          size_t q = pos;
          const int e = (int)(q % 16); q /= 16;
          const int lane = (int)(q % 64); q /= 64;
          const int l = (int)(q % t); q /= t;
          const int j = (int)(q % t); q /= t;
          const int b = (int)(q % 2); q /= 2;
          const int a = (int)(q % 2); q /= 2;
          const int s = (int)(q % (ic / 32)); q /= (ic / 32);
          const int ob = (int)q;
          const int o = 32 * ob + (lane & 31), i = 32 * s + 16 * (lane >> 5) + e, ky = a + 2 * j, kx = b + 2 * l;
          const bool live = ky < k && kx < k;
          const size_t wi = (((size_t)o * ic + i) * k + (live ? ky : 0)) * k + (live ? kx : 0);
          const unsigned char want = live ? (unsigned char)w[wi] : 0;
          if (img[pos] != want) {
            printf("k %d ic %d oc %d: byte %zu (block %d step %d parity %d,%d tap %d,%d lane %d byte %d): got %u want %u (%s)\n", k, ic,
                   oc, pos, ob, s, a, b, j, l, lane, e, img[pos], want, live ? "live" : "ZERO ROW / COLUMN");
            return 1;
          }
          if (live && seen[wi]++) {
            printf("k %d ic %d oc %d: weight %zu packed twice\n", k, ic, oc, wi);
            return 1;
          }
          nonzero += img[pos] != 0;
        }
        for (size_t wi = 0; wi < w.size(); ++wi)
          if (!seen[wi]) {
            printf("k %d ic %d oc %d: weight %zu lost\n", k, ic, oc, wi);
            return 1;
          }
        if (nonzero != w.size()) {
          printf("k %d ic %d oc %d: %zu weights in the image, %zu given\n", k, ic, oc, nonzero, w.size());
          return 1;
        }
        printf("k %d ic %3d oc %3d: %7zu bytes, %6zu weights in place, %6zu dead bytes zero\n", k, ic, oc, bytes, nonzero, bytes - nonzero);
        ++nshapes;
      }
  printf("deconv_pack_check: all %d shapes packed, every dead byte zero\n", nshapes);
  return 0;
}
