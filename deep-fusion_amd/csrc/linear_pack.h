// linear_pack.h -- host-only: the device image of the token linear op (linear.cuh) and the proof of its fast requant route.
// No HIP in here, so that the packer can be built and run on its own (tools/linear_plan_check.cc, under the host sanitizers).
//
// The caller's weights are plain row-major s8 {n, k} (an nn.Linear weight).  Weight section:
//   [nb < ceil(n / 128)][ks < ceil(k / 64)][f < 4][j < 2][lane < 64][16]
// One (nb, ks) block of 8 KB is exactly what the tile kernel holds in LDS for a slab: eight A operands of
// v_mfma_i32_32x32x32_i8, each 1 KB in lane order.  Byte b of lane =
//   W[o = 128 nb + 32 f + (lane & 31)][c = 64 ks + 32 j + 16 (lane >> 5) + b],   ZERO where o >= n or c >= k.
// Then comp | bias | scale, 128 entries per n-block (entries n .. stay 0): comp[o] = 128 * sum_c W[o][c] (what a u8 source
// staged as a ^ 0x80 needs added back), bias as f32 (requant_host.h's conversion), scale (a single scale expanded).
// The table section is written by lin_pack_table.
#pragma once

#include <string.h>

#include "linear_plan.h"
#include "requant_host.h"

namespace dfx {

// offset in the weight section of W[o][c]
inline size_t lin_wei_offset(int o, int c, int k) {
  const int nb = o / LIN_BN, f = (o % LIN_BN) / 32, r = o % 32;
  const int ks = c / LIN_KS, j = (c % LIN_KS) / 32, hh = (c % 32) / 16, b = c % 16;
  return ((size_t)nb * (size_t)lin_nslabs(k) + (size_t)ks) * LIN_WBLOCK + (size_t)(((f * 2 + j) * 64 + hh * 32 + r) * 16 + b);
}

// The bound of |acc| the route's proof uses: a u8 source is within 0 .. 255, so |acc| <= 255 * max(P, N); an s8 source is
// within -128 .. 127, so |acc| <= 128 * (P + N).  P, N: the sums of the channel's positive / negative weights' magnitudes.
inline double lin_acc_bound(int src_dt, long long pos, long long neg_mag) {
  return src_dt == DFX_U8 ? 255.0 * (double)(pos > neg_mag ? pos : neg_mag) : 128.0 * (double)(pos + neg_mag);
}

// Fills img[0 .. off_table) (img has lin_image(n, k).bytes bytes; the table section is left alone).
// Returns whether EVERY channel passes fast_ok_2p30 (requant_host.h) with its bound.
inline bool lin_pack(const dfx_linear_desc &d, const int8_t *wei, const void *bia, const float *scales, unsigned char *img) {
  const int n = d.n, k = d.k;
  const LinImage im = lin_image(n, k);
  memset(img, 0, im.off_table);
  int32_t *comp = (int32_t *)(img + im.off_comp);
  float *bias = (float *)(img + im.off_bias), *scale = (float *)(img + im.off_scale);
  bool fast = true;
  for (int o = 0; o < n; ++o) {
    const int8_t *row = wei + (size_t)o * k;
    long long pos = 0, neg = 0;
    for (int c0 = 0; c0 < k; c0 += 16) {  // a 16-byte piece is contiguous in the image
      const int len = k - c0 < 16 ? k - c0 : 16;
      memcpy(img + lin_wei_offset(o, c0, k), row + c0, (size_t)len);
      for (int b = 0; b < len; ++b) (row[c0 + b] > 0 ? pos : neg) += row[c0 + b];
    }
    comp[o] = (int32_t)(128 * (pos + neg));
    bias[o] = d.bia_dt == DFX_UNDEF ? 0.0f : bias_to_f32(bia, d.bia_dt, o);
    scale[o] = scales[d.nscales == 1 ? 0 : o];
    fast = fast_ok_2p30(lin_acc_bound(d.src_dt, pos, -neg), bias[o], scale[o]) && fast;
  }
  return fast;
}

inline void lin_pack_table(const dfx_linear_desc &d, const uint8_t *lut, unsigned char *img) { memcpy(img + lin_image(d.n, d.k).off_table, lut, 256); }

}  // namespace dfx
