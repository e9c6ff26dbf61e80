// fc_pack.h -- host-only: the weight image of the fully-connected op's MFMA kernel (fc.cuh).  No HIP in here, so that
// the packer can be built and run on its own (tools/fc_pack_check.cc, under the host sanitizers).
//
// Class: K = ih * iw * ic a multiple of 64; any oc.  The caller's weights are plain oihw {oc, ic, ih, iw} (a flattened
// CHW classifier); the kernel contracts over src's order, k = (y * iw + x) * ic + c.
// Image: [ob < ceil(oc / 32)][ks < K / 64][j < 2][lane < 64][16]: one k-step of 64 is two fragments of 1 KB, each the
// A operand of one v_mfma_i32_32x32x32_i8.  Byte b of lane = W[o = 32 ob + (lane & 31)][k = 64 ks + 32 j + 16 (lane >> 5) + b]
// and ZERO for the rows o >= oc of the last block.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace dfx {

inline int fc_pack_blocks(int oc) { return (oc + 31) / 32; }
inline size_t fc_pack_bytes(int oc, int k) { return (size_t)fc_pack_blocks(oc) * (size_t)(k / 64) * 2048; }

// offset in wei {oc, ic, ih, iw} of the weight that meets src's element k = (y * iw + x) * ic + c of output channel o
inline size_t fc_wei_offset(int o, int k, int ic, int ih, int iw) {
  const int c = k % ic, x = (k / ic) % iw, y = k / (ic * iw);
  return (((size_t)o * ic + c) * ih + y) * iw + x;
}

// wei: s8 {oc, ic, ih, iw} row-major; out: fc_pack_bytes(oc, ic * ih * iw) bytes
inline void fc_pack(const int8_t *wei, int oc, int ic, int ih, int iw, unsigned char *out) {
  const int k_total = ic * ih * iw, nks = k_total / 64;
  memset(out, 0, fc_pack_bytes(oc, k_total));
  uint32_t *off = new uint32_t[k_total];  // where element k of a channel's row sits: the same for every channel
  for (int k = 0; k < k_total; ++k) off[k] = (uint32_t)fc_wei_offset(0, k, ic, ih, iw);
  for (int ob = 0; ob < fc_pack_blocks(oc); ++ob)
    for (int ks = 0; ks < nks; ++ks)
      for (int j = 0; j < 2; ++j) {
        unsigned char *frag = out + (((size_t)ob * nks + ks) * 2 + j) * 1024;
        for (int lane = 0; lane < 64; ++lane) {
          const int o = 32 * ob + (lane & 31);
          if (o >= oc) continue;
          const int8_t *row = wei + (size_t)o * k_total;
          const uint32_t *ok = off + 64 * ks + 32 * j + 16 * (lane >> 5);
          for (int b = 0; b < 16; ++b) frag[lane * 16 + b] = (unsigned char)row[ok[b]];
        }
      }
  delete[] off;
}

}  // namespace dfx
