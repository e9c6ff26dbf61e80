// gconv_pack.h -- host-only: the weight image of the grouped conv's MFMA kernel (gconv.cuh).  No HIP in here, so that
// the packer can be built and run on its own (tools/gconv_pack_check.cc, under the host sanitizers).
//
// Class: 3x3 window, ic == oc == c a multiple of 32, cpg = c / groups in {4, 8, 16, 32, 64}.
// Image: [ob][tap][j < nib][lane][16] with nib = 1 (cpg <= 32: output block ob reads input block ob) or 2 (cpg = 64:
// input blocks 2 (ob / 2) + j).  Byte b of lane = W[o = 32 ob + (lane & 31)][i = 32 ib + 16 (lane >> 5) + b][tap] of
// the block-diagonal dense weights, i.e. w[o][i - g(o) * cpg][tap] inside o's group and ZERO outside: the order of
// conv_direct.cuh's W0d fragments.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace dfx {

inline int gconv_pack_nib(int cpg) { return cpg == 64 ? 2 : 1; }
inline size_t gconv_pack_bytes(int c, int cpg) { return (size_t)(c / 32) * 9 * gconv_pack_nib(cpg) * 1024; }

// wei: s8 {c, cpg, 3, 3} row-major; out: gconv_pack_bytes(c, cpg) bytes
inline void gconv_pack(const int8_t *wei, int c, int cpg, unsigned char *out) {
  const int nib = gconv_pack_nib(cpg);
  memset(out, 0, gconv_pack_bytes(c, cpg));
  for (int ob = 0; ob < c / 32; ++ob)
    for (int tap = 0; tap < 9; ++tap)
      for (int j = 0; j < nib; ++j) {
        const int ib = nib == 2 ? (ob & ~1) + j : ob;
        unsigned char *frag = out + (((size_t)ob * 9 + tap) * nib + j) * 1024;
        for (int lane = 0; lane < 64; ++lane) {
          const int o = 32 * ob + (lane & 31);
          const int i0 = (o / cpg) * cpg;  // first input channel of o's group
          for (int b = 0; b < 16; ++b) {
            const int i = 32 * ib + 16 * (lane >> 5) + b;
            if (i >= i0 && i < i0 + cpg) frag[lane * 16 + b] = (unsigned char)wei[((size_t)o * cpg + (i - i0)) * 9 + tap];
          }
        }
      }
}

}  // namespace dfx
