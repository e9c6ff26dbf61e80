// deconv_pack.h -- host-only: the weight image of the transposed conv's MFMA kernel (deconv.cuh).  No HIP in here, so
// that the packer can be built and run on its own (tools/deconv_pack_check.cc, under the host sanitizers).
//
// Class: stride 2; window 2x2, 3x3 or 4x4 (kh == kw == k); ic and oc multiples of 32.  The kernel works on the window
// KE = 2 T with T = 1 (k = 2) or T = 2 (k = 3 or 4): a 3x3 window is a 4x4 one whose last row and column are zero.
// Output parity (a, b) = ((oy + pad_t) % 2, (ox + pad_l) % 2) is a dense T x T conv with the sub-kernel
// w[:, :, a + 2 j, b + 2 l], j, l < T (deconv.cuh).
// Image: [ob][s][a][b][j][l][lane][16] with ob < oc / 32 the output block and s < ic / 32 the K-step.  Byte e of lane =
//   w[o = 32 ob + (lane & 31)][i = 32 s + 16 (lane >> 5) + e][ky = a + 2 j][kx = b + 2 l],  ZERO where ky >= k or kx >= k:
// the order of gconv_pack.h's fragments (the A operand of v_mfma_i32_32x32x32_i8).
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace dfx {

inline int deconv_pack_t(int k) { return k == 2 ? 1 : 2; }
// bytes of one output block's fragments
inline size_t deconv_pack_block_bytes(int ic, int k) { return (size_t)(ic / 32) * 4 * deconv_pack_t(k) * deconv_pack_t(k) * 1024; }
inline size_t deconv_pack_bytes(int oc, int ic, int k) { return (size_t)(oc / 32) * deconv_pack_block_bytes(ic, k); }
// offset of the fragment (ob, s, a, b, j, l)
inline size_t deconv_pack_frag(int ic, int k, int ob, int s, int a, int b, int j, int l) {
  const int t = deconv_pack_t(k);
  return ((((((size_t)ob * (ic / 32) + s) * 2 + a) * 2 + b) * t + j) * t + l) * 1024;
}

// wei: s8 {oc, ic, k, k} row-major; out: deconv_pack_bytes(oc, ic, k) bytes
inline void deconv_pack(const int8_t *wei, int oc, int ic, int k, unsigned char *out) {
  const int t = deconv_pack_t(k);
  memset(out, 0, deconv_pack_bytes(oc, ic, k));
  for (int ob = 0; ob < oc / 32; ++ob)
    for (int s = 0; s < ic / 32; ++s)
      for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b)
          for (int j = 0; j < t; ++j)
            for (int l = 0; l < t; ++l) {
              const int ky = a + 2 * j, kx = b + 2 * l;
              if (ky >= k || kx >= k) continue;  // the zero row / column of a 3x3 window
              unsigned char *frag = out + deconv_pack_frag(ic, k, ob, s, a, b, j, l);
              for (int lane = 0; lane < 64; ++lane) {
                const int o = 32 * ob + (lane & 31);
                for (int e = 0; e < 16; ++e) {
                  const int i = 32 * s + 16 * (lane >> 5) + e;
                  frag[lane * 16 + e] = (unsigned char)wei[(((size_t)o * ic + i) * k + ky) * k + kx];
                }
              }
            }
}

}  // namespace dfx
