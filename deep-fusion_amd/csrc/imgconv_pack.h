// imgconv_pack.h -- host-only: the weight image of the first-layer conv's MFMA kernel (imgconv.cuh).  No HIP in here,
// so that the packer can be built and run on its own (tools/imgconv_pack_check.cc, under the host sanitizers).
//
// Class: k x k window with k in {7, 3}, ic in {3, 4}, oc a multiple of 32.  The contraction runs over K-steps of 32
// bytes: 8 input pixels of 4 bytes each (a 3-channel pixel is repacked to 4 bytes, the 4th meets a zero weight).
// Lane half h = lane >> 5 holds pixels 4 h .. 4 h + 3 of the step, byte b of a lane is (pixel j = b >> 2, channel
// c = b & 3):
//   k = 7: step t is kernel row t: (ky, kx) = (t, 4 h + j); kx = 7 is a zero weight                         7 steps
//   k = 3: step 0 holds rows 0 and 1 in the two halves: (ky, kx) = (h, j); step 1 row 2 in half 0: (2, j);
//          j = 3 and half 1 of step 1 are zero weights                                                       2 steps
// Image: [ob][step][lane][16], byte b of lane = w[o = 32 ob + (lane & 31)][c][ky][kx] or ZERO.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace dfx {

inline int imgconv_pack_steps(int k) { return k == 7 ? 7 : 2; }
inline size_t imgconv_pack_bytes(int oc, int k) { return (size_t)(oc / 32) * imgconv_pack_steps(k) * 1024; }

// the tap that (step t, lane half h, pixel j of the half) reads; false: a zero weight
inline bool imgconv_pack_tap(int k, int t, int h, int j, int *ky, int *kx) {
  if (k == 7) {
    *ky = t;
    *kx = 4 * h + j;
    return *kx < 7;
  }
  *ky = t == 0 ? h : 2;
  *kx = j;
  return j < 3 && !(t == 1 && h == 1);
}

// wei: s8 {oc, ic, k, k} row-major; out: imgconv_pack_bytes(oc, k) bytes
inline void imgconv_pack(const int8_t *wei, int oc, int ic, int k, unsigned char *out) {
  const int nt = imgconv_pack_steps(k);
  memset(out, 0, imgconv_pack_bytes(oc, k));
  for (int ob = 0; ob < oc / 32; ++ob)
    for (int t = 0; t < nt; ++t) {
      unsigned char *frag = out + ((size_t)ob * nt + t) * 1024;
      for (int lane = 0; lane < 64; ++lane) {
        const int o = 32 * ob + (lane & 31), h = lane >> 5;
        for (int j = 0; j < 4; ++j) {
          int ky, kx;
          if (!imgconv_pack_tap(k, t, h, j, &ky, &kx)) continue;
          for (int c = 0; c < ic && c < 4; ++c)
            frag[lane * 16 + 4 * j + c] = (unsigned char)wei[(((size_t)o * ic + c) * k + ky) * k + kx];
        }
      }
    }
}

}  // namespace dfx
