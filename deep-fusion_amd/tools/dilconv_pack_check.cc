// dilconv_pack_check -- host-only check of the dilated conv's weight packer (csrc/dilconv_pack.h), meant to be built with
// the host sanitizers; it needs no GPU and no HIP:
//   g++ -std=c++11 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/dilconv_pack_check.cc -o tools/dilconv_pack_check
// For every (ic, oc, slab) of a table -- ic = 96 at 2 K-steps per slab (an uneven last slab) and oc = 160 (chunks of
// 4 + 1 blocks) among them -- it packs weights without a zero byte into a buffer of exactly dilconv_pack_bytes() bytes
// that was filled with a sentinel, then walks the image the way the kernel does: chunk by chunk, slab by slab (the
// pieces dilconv_pack_slab / dilconv_pack_slab_bytes name), K-step by K-step, tap by tap, block by block, lane by lane.
// The pieces must tile the image exactly (no gap, no overlap, nothing beyond the end), unpacking must reproduce every
// weight exactly once, and no byte may be left unwritten.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../csrc/dilconv_pack.h"

struct Case { int ic, oc, slab; };

int main() {
  unsigned seed = 9753;
  const Case cases[] = {{32, 32, 1}, {32, 160, 1}, {96, 32, 1}, {96, 32, 2}, {96, 32, 3}, {96, 32, 8}, {96, 160, 2},
                        {64, 96, 1}, {160, 128, 3}, {320, 256, 2}, {2048, 32, 3}};
  int ncases = 0;
  for (const Case &c : cases) {
    const int ic = c.ic, oc = c.oc, slab = c.slab, ksteps = ic / 32, cblocks = oc / 32;
    std::vector<int8_t> w((size_t)oc * ic * 9);
    for (auto &v : w) {
      seed = seed * 1664525u + 1013904223u;
      const int x = (int)(seed >> 24) - 128;
      v = (int8_t)(x == 0 ? 77 : x);  // no zero weights: a zero in the image would be a dead byte
    }
    const size_t bytes = dfx::dilconv_pack_bytes(oc, ic);
    if (bytes != w.size()) {  // 32 x 32 x 9 weights per KB-fragment triple: the image has no padding at all
      printf("ic %d oc %d: %zu bytes for %zu weights\n", ic, oc, bytes, w.size());
      return 1;
    }
    std::vector<unsigned char> img(bytes, 0);  // exactly sized: the sanitizer sees a byte too many
    dfx::dilconv_pack(w.data(), oc, ic, img.data());
    for (size_t pos = 0; pos < bytes; ++pos)
      if (img[pos] == 0) {  // zero can only be the fill: the packer left the byte out
        printf("ic %d oc %d: byte %zu of the image was not written\n", ic, oc, pos);
        return 1;
      }
    std::vector<int8_t> back(w.size(), 0);
    std::vector<unsigned char> seen(w.size(), 0);
    const int nchunks = (cblocks + dfx::DL_PACK_CHUNK - 1) / dfx::DL_PACK_CHUNK, nslabs = (ksteps + slab - 1) / slab;
    size_t expect = 0;  // where the next piece must start
    for (int chunk = 0; chunk < nchunks; ++chunk) {
      const int nb = dfx::dilconv_pack_nb(oc, chunk);
      if (nb != (cblocks - 4 * chunk < 4 ? cblocks - 4 * chunk : 4)) {
        printf("ic %d oc %d: chunk %d has %d blocks\n", ic, oc, chunk, nb);
        return 1;
      }
      for (int j = 0; j < nslabs; ++j) {
        const size_t off = dfx::dilconv_pack_slab(oc, ic, chunk, j, slab), len = dfx::dilconv_pack_slab_bytes(oc, ic, chunk, j, slab);
        const int ns = ksteps - j * slab < slab ? ksteps - j * slab : slab;
        if (off != expect || len != (size_t)ns * 9 * nb * 1024 || off + len > bytes) {
          printf("ic %d oc %d slab %d: piece (chunk %d, slab %d) at %zu + %zu, expected at %zu\n", ic, oc, slab, chunk, j, off, len, expect);
          return 1;
        }
        expect = off + len;
        // the kernel's reading order inside the piece
        const unsigned char *p = img.data() + off;
        for (int s = 0; s < ns; ++s)
          for (int tap = 0; tap < 9; ++tap)
            for (int obl = 0; obl < nb; ++obl)
              for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 16; ++e, ++p) {
                  const int o = 32 * (4 * chunk + obl) + (lane & 31), i = 32 * (j * slab + s) + 16 * (lane >> 5) + e;
                  const size_t wi = ((size_t)o * ic + i) * 9 + tap;
                  if (seen[wi]++) {
                    printf("ic %d oc %d slab %d: weight %zu read twice\n", ic, oc, slab, wi);
                    return 1;
                  }
                  back[wi] = (int8_t)*p;
                }
      }
    }
    if (expect != bytes) {
      printf("ic %d oc %d slab %d: the pieces end at %zu of %zu bytes\n", ic, oc, slab, expect, bytes);
      return 1;
    }
    for (size_t wi = 0; wi < w.size(); ++wi)
      if (!seen[wi] || back[wi] != w[wi]) {
        printf("ic %d oc %d slab %d: weight %zu %s (got %d want %d)\n", ic, oc, slab, wi, seen[wi] ? "wrong" : "lost", back[wi], w[wi]);
        return 1;
      }
    // dilconv_pack_frag agrees with the walk: spot-check the last fragment
    if (dfx::dilconv_pack_frag(oc, ic, cblocks - 1, ksteps - 1, 8) != bytes - 1024) {
      printf("ic %d oc %d: the last fragment is at %zu\n", ic, oc, dfx::dilconv_pack_frag(oc, ic, cblocks - 1, ksteps - 1, 8));
      return 1;
    }
    printf("ic %4d oc %3d slab %d: %8zu bytes in %d chunks x %d slabs, every weight back in place, no byte unwritten\n", ic, oc, slab, bytes,
           nchunks, nslabs);
    ++ncases;
  }
  printf("dilconv_pack_check: all %d cases unpacked to the weights they were packed from\n", ncases);
  return 0;
}
