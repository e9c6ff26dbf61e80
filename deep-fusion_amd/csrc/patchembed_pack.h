// patchembed_pack.h -- host-only: the device image of the patch-embedding op (patchembed.cuh) and the proof of its fast
// requant route.  No HIP in here (tools/patchembed_plan_check.cc builds it under the host sanitizers).
//
// The caller's weights are plain oihw s8 {oc, ic, ph, pw}.  pe_permute brings them to {oc, K} with K in the order
// (ky, kx, i) -- the order in which a patch's bytes lie in an NHWC image, run after run -- and lin_pack of linear_pack.h
// packs that matrix AS IT IS: the weight section, comp, bias and scale are dfx_linear's image of the same {n, k} matrix, and
// lin_wei_offset addresses it.  With a table the packer is handed the per-channel max_t |table[t][o]| as an f32 bias, so
// that lin_pack's proof is (B + max_t |table|) * |scale| <= 2^30, and the bias section is zeroed afterwards (the kernels read
// the table instead).
#pragma once

#include <math.h>
#include <string.h>

#include <vector>

#include "linear_pack.h"
#include "patchembed_plan.h"

namespace dfx {

// out {oc, K}: out[o][(ky * pw + kx) * ic + i] = wei[((o * ic + i) * ph + ky) * pw + kx]
inline void pe_permute(const dfx_patchembed_desc &d, const int8_t *wei, int8_t *out) {
  const int k = pe_k(d);
  for (int o = 0; o < d.oc; ++o)
    for (int i = 0; i < d.ic; ++i)
      for (int ky = 0; ky < d.ph; ++ky)
        for (int kx = 0; kx < d.pw; ++kx)
          out[(size_t)o * k + (size_t)(ky * d.pw + kx) * d.ic + i] = wei[(((size_t)o * d.ic + i) * d.ph + ky) * d.pw + kx];
}

// tmax[o] = max_t |table[t][o]|; false where an entry is not finite
inline bool pe_scan_table(const dfx_patchembed_desc &d, const float *table, long long ld, float *tmax) {
  for (int o = 0; o < d.oc; ++o) tmax[o] = 0.0f;
  const long long tokens = pe_tokens(d);
  for (long long t = 0; t < tokens; ++t)
    for (int o = 0; o < d.oc; ++o) {
      const float v = table[t * ld + o];
      if (!std::isfinite(v)) return false;
      if (fabsf(v) > tmax[o]) tmax[o] = fabsf(v);
    }
  return true;
}

// the table section (out: its first float): rows of pe_table_ld(oc) floats, the pad 0
inline void pe_pack_table(const dfx_patchembed_desc &d, const float *table, long long ld, float *out) {
  const int tld = pe_table_ld(d.oc);
  const long long tokens = pe_tokens(d);
  for (long long t = 0; t < tokens; ++t) {
    memcpy(out + t * tld, table + t * ld, (size_t)d.oc * 4);
    for (int o = d.oc; o < tld; ++o) out[t * tld + o] = 0.0f;
  }
}

// Fills img[0 .. off_table): linear_pack.h's sections and the K offset table.  wperm: pe_permute's matrix.  tmax: the
// table's per-channel maximum where the descriptor has a table (nullptr: no table given yet, proved as if it were 0).
// Returns whether EVERY channel passes fast_ok_2p30.
inline bool pe_pack(const dfx_patchembed_desc &d, const int8_t *wperm, const void *bia, const float *scales, const float *tmax, unsigned char *img) {
  const PeImage im = pe_image(d);
  const bool as_bias = d.table && tmax;
  const bool fast = lin_pack(pe_gemm(d, as_bias), wperm, as_bias ? (const void *)tmax : bia, scales, img);
  if (as_bias) memset(img + im.lin.off_bias, 0, im.lin.off_scale - im.lin.off_bias);
  memset(img + im.off_ktab, 0, im.off_table - im.off_ktab);
  pe_fill_ktab(d, (int32_t *)(img + im.off_ktab));
  return fast;
}

}  // namespace dfx
