// patchembed_host.h -- what tools/patchembed_check.cc and tools/bench_patchembed.cc compare with: the scalar restatement of the
// int8 patch-embedding op's arithmetic (include/dfx.h: the exact integer sum over (i, ky, kx) of a patch against the oihw
// weights, one separately rounded add of the bias or of the token table's entry, one multiply, the x86 conversion and
// saturations), the token layout and the prefix rows.  Host only.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

#include "dfx.h"
#include "linear_host.h"

namespace patchembed_host {

using linear_host::esize;

// dst: as it was before the op ({bs * img_rows, dst_ld} elements); what the op does not write stays.  table: th * tw * oc floats
// or null; prefix: t0 * oc elements of dst's type or null.
inline void reference(const unsigned char *src, int src_dt, int bs, int ih, int iw, int ic, int ph, int pw, const int8_t *wei, int oc, const void *bia,
                      int bia_dt, const float *table, const float *scales, int nscales, bool relu, int rm, int dst_dt, int t0, long long img_rows,
                      long long dst_ld, const void *prefix, std::vector<unsigned char> &dst) {
  const int th = ih / ph, tw = iw / pw;
  const bool do_relu = relu || dst_dt == DFX_U8;
  const size_t ds = esize(dst_dt);
  for (int b = 0; b < bs; ++b) {
    for (int ty = 0; ty < th; ++ty)
      for (int tx = 0; tx < tw; ++tx) {
        const int t = ty * tw + tx;
        for (int o = 0; o < oc; ++o) {
          long long acc = 0;
          for (int i = 0; i < ic; ++i)
            for (int ky = 0; ky < ph; ++ky)
              for (int kx = 0; kx < pw; ++kx) {
                const unsigned char x = src[(((size_t)b * ih + ty * ph + ky) * iw + tx * pw + kx) * ic + i];
                acc += (long long)(src_dt == DFX_U8 ? (int)x : (int)(signed char)x) * wei[(((size_t)o * ic + i) * ph + ky) * pw + kx];
              }
          volatile float f = (float)(int32_t)acc;
          if (table) f = f + table[(size_t)t * oc + o];
          else if (bia_dt != DFX_UNDEF) f = f + linear_host::bias_f32(bia, bia_dt, o);
          f = f * scales[nscales == 1 ? 0 : o];
          float v = f;
          if (do_relu && 0.0f > v) v = 0.0f;  // vmaxps(zero, v): NaN passes
          unsigned char *out = &dst[(((size_t)b * img_rows + t0 + t) * (size_t)dst_ld + o) * ds];
          if (dst_dt == DFX_F32) {
            memcpy(out, &v, 4);
          } else if (dst_dt == DFX_S32) {
            const int32_t q = linear_host::cvt_x86(v, rm);
            memcpy(out, &q, 4);
          } else {
            const int32_t q = linear_host::cvt_x86(v, rm);
            *out = (unsigned char)(dst_dt == DFX_S8 ? (unsigned)(q < -128 ? -128 : q > 127 ? 127 : q) & 0xffu : ((unsigned)q > 255u ? 255u : (unsigned)q));
          }
        }
      }
    if (prefix)
      for (int r = 0; r < t0; ++r)
        memcpy(&dst[((size_t)b * img_rows + r) * (size_t)dst_ld * ds], (const unsigned char *)prefix + (size_t)r * oc * ds, (size_t)oc * ds);
  }
}

// what the op writes: the oc valid elements of the token rows and, with a prefix, of the prefix rows of every image
inline bool written_differ(const void *got, const std::vector<unsigned char> &want, int bs, long long img_rows, int t0, long long tokens, bool prefix,
                           long long ld, int oc, size_t es) {
  for (int b = 0; b < bs; ++b)
    for (long long r = prefix ? 0 : t0; r < t0 + tokens; ++r) {
      const size_t at = ((size_t)b * img_rows + r) * ld * es;
      if (memcmp((const unsigned char *)got + at, &want[at], (size_t)oc * es) != 0) return true;
    }
  return false;
}

}  // namespace patchembed_host
