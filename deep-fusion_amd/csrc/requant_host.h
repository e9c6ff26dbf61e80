// requant_host.h -- host-only: the per-channel requantisation constants (compensation, bias as f32, scale) of the ops
// whose activations are stored as u8 - 128, and the proof of their fast requant route, written once for every op that
// calls requant_consts() (the conv op takes the small helpers only: its proofs are others, conv_weights.h).  No HIP in here, so that
// it can be built and run on its own (tools/requant_host_check.cc, under the host sanitizers).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cmath>

#include "../../include/dfx.h"

namespace dfx {

inline const char *dt_name(int dt) { return dt == DFX_F32 ? "f32" : dt == DFX_S32 ? "s32" : dt == DFX_S8 ? "s8" : "u8"; }

inline size_t round16(size_t v) { return (v + 15) & ~(size_t)15; }

inline float bias_to_f32(const void *b, int dt, int c) {
  switch (dt) {  // vcvtdq2ps after vpmovsxbd / vpmovzxbd / vmovups, jit_conv_kernel.cc:235-255
    case DFX_F32: return ((const float *)b)[c];
    case DFX_S32: return (float)((const int32_t *)b)[c];
    case DFX_S8: return (float)((const int8_t *)b)[c];
    case DFX_U8: return (float)((const uint8_t *)b)[c];
  }
  return 0.0f;
}

// One channel's precondition of the fast requant route (dwconv.cuh dw_store<FAST>, gconv.cuh gc_quarter<FAST>,
// dwpw.cuh's stage 1).  The accumulator is exact on both routes (integer dot products, the compensation is an integer
// start value) and so are the add and the multiply; only the conversion differs.  amax = 255 * max(P, N) bounds |acc|,
// P and N being the sums of the channel's positive and negative taps.  With bias and scale finite the f32 result is
// within a relative 2^-22 of (acc + bias) * scale, so a bound of 2^30 keeps everything far from +-2^31, where the
// hardware conversions (saturating) and vcvtps2dq (0x80000000) part ways; no NaN can arise.
inline bool fast_ok_2p30(double amax, float bias, float scale) {
  if (!std::isfinite(bias) || !std::isfinite(scale)) return false;
  return (amax + std::fabs((double)bias)) * std::fabs((double)scale) <= 1073741824.0;  // 2^30
}

// Fills comp[k] = 128 * (sum of the taps), bias[k] (0 where bia_dt is DFX_UNDEF) and scale[k] (scales[0] broadcast
// where nscales == 1) for channels k < n with `taps` taps each, tap(k, i) being the weight of channel k's tap i.
// Returns whether EVERY channel passes fast_ok_2p30.
template <class Tap>
inline bool requant_consts(int n, size_t taps, Tap tap, const void *bia, int bia_dt, const float *scales, int nscales,
                           int32_t *comp, float *bias, float *scale) {
  bool fast = true;
  for (int k = 0; k < n; ++k) {
    long long pos = 0, neg = 0;
    for (size_t i = 0; i < taps; ++i) {
      const int v = tap(k, i);
      (v > 0 ? pos : neg) += v;
    }
    comp[k] = (int32_t)(128 * (pos + neg));
    bias[k] = bia_dt == DFX_UNDEF ? 0.0f : bias_to_f32(bia, bia_dt, k);
    scale[k] = scales[nscales == 1 ? 0 : k];
    fast = fast_ok_2p30(255.0 * (double)(pos > -neg ? pos : -neg), bias[k], scale[k]) && fast;
  }
  return fast;
}

}  // namespace dfx
