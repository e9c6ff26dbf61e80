// linear_host.h -- what tools/linear_check.cc compares with: the scalar restatement of the int8 token linear
// op's arithmetic (include/dfx.h: exact integer accumulation, a separately rounded add and multiply, the x86 conversion and
// saturations, the optional byte table).  Host only.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "dfx.h"

namespace linear_host {

inline size_t esize(int dt) { return (dt == DFX_F32 || dt == DFX_S32) ? 4 : 1; }

// vcvtps2dq under the round mode: NaN and everything outside s32 give 0x80000000
inline int32_t cvt_x86(float f, int rm) {
  if (!(f >= -2147483648.0f && f < 2147483648.0f)) return INT32_MIN;
  return (int32_t)(rm == DFX_ROUND_DOWN ? floorf(f) : nearbyintf(f));
}

inline float bias_f32(const void *b, int dt, int o) {
  switch (dt) {
    case DFX_F32: return ((const float *)b)[o];
    case DFX_S32: return (float)((const int32_t *)b)[o];
    case DFX_S8: return (float)((const int8_t *)b)[o];
    case DFX_U8: return (float)((const uint8_t *)b)[o];
  }
  return 0.0f;
}

// dst: as it was before the op; the elements n .. dst_ld - 1 of a row stay.  lut_in_dt DFX_UNDEF: no table.
inline void reference(const unsigned char *src, int src_dt, long long rows, long long src_ld, int k, const int8_t *wei, int n, const void *bia, int bia_dt,
                      const float *scales, int nscales, bool relu, int rm, int dst_dt, long long dst_ld, const uint8_t *lut, int lut_in_dt,
                      std::vector<unsigned char> &dst) {
  const int req = lut_in_dt != DFX_UNDEF ? lut_in_dt : dst_dt;
  const bool do_relu = relu || req == DFX_U8;
  const size_t ds = esize(dst_dt);
  for (long long m = 0; m < rows; ++m) {
    const unsigned char *row = src + (size_t)m * (size_t)src_ld;
    for (int o = 0; o < n; ++o) {
      const int8_t *w = wei + (size_t)o * k;
      long long acc = 0;
      for (int c = 0; c < k; ++c) acc += (long long)(src_dt == DFX_U8 ? (int)row[c] : (int)(signed char)row[c]) * w[c];
      volatile float f = (float)(int32_t)acc;
      f = f + (bia_dt != DFX_UNDEF ? bias_f32(bia, bia_dt, o) : 0.0f);
      f = f * scales[nscales == 1 ? 0 : o];
      float v = f;
      if (do_relu && 0.0f > v) v = 0.0f;  // vmaxps(zero, v): NaN passes
      unsigned char *out = &dst[((size_t)m * (size_t)dst_ld + o) * ds];
      if (req == DFX_F32) {
        memcpy(out, &v, 4);
      } else if (req == DFX_S32) {
        const int32_t q = cvt_x86(v, rm);
        memcpy(out, &q, 4);
      } else {
        const int32_t q = cvt_x86(v, rm);
        unsigned t = req == DFX_S8 ? (unsigned)(q < -128 ? -128 : q > 127 ? 127 : q) & 0xffu : ((unsigned)q > 255u ? 255u : (unsigned)q);
        if (lut_in_dt != DFX_UNDEF) t = lut[lut_in_dt == DFX_U8 ? t : (t ^ 0x80u)];
        *out = (unsigned char)t;
      }
    }
  }
}

// the valid n elements of every row (the op leaves the pad elements of dst's device copy as they are)
inline bool rows_differ(const void *got, const std::vector<unsigned char> &want, long long rows, long long ld, int n, size_t es) {
  for (long long r = 0; r < rows; ++r)
    if (memcmp((const unsigned char *)got + (size_t)r * ld * es, &want[(size_t)r * ld * es], (size_t)n * es) != 0) return true;
  return false;
}

}  // namespace linear_host
