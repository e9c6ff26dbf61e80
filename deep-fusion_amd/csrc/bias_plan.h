// bias_plan.h -- host-only, plain C++: what the logit bias of the batched matrix product and of the attention
// (dfx_bmm_set_bias / dfx_attn_set_bias, dfx_logit_bias_desc of include/dfx.h) decides before a kernel runs: the layout's
// validation against a dfx_bmm_desc, the extent of the caller's host table, the device image the library owns and the
// index function the kernels use on it, the scan of the addressed entries (max |finite entry|, "has -inf", +inf / NaN
// refused), the distinct bytes of the tables and the proof of the fast requant route with a bias.
// No HIP in here, so that it can be built and run on its own (tools/bias_plan_check.cc, under the host sanitizers).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cmath>

#include "bmm_plan.h"

namespace dfx {

constexpr unsigned long long BIAS_IMAGE_MAX_BYTES = 1ull << 30;

// rows of a table: m, or one row broadcast over m (ld == 0)
inline long long bias_rows(const dfx_bmm_desc &d, const dfx_logit_bias_desc &b) { return b.ld == 0 ? 1 : d.m; }
// columns of an image row: n rounded up to 32, pads zero, so that a lane's 16-byte load of 4 adjacent n of a tile of 32 is
// always aligned and inside the row (n <= 2^31 - 32: bmm_validate)
inline long long bias_cols(const dfx_bmm_desc &d) { return ((long long)d.n + 31) / 32 * 32; }
inline long long bias_tables(const dfx_logit_bias_desc &b) { return (long long)b.period0 * b.period1; }

// one past the largest float index of the caller's table that is addressed (128 bits: no overflow)
inline unsigned __int128 bias_host_span(const dfx_bmm_desc &d, const dfx_logit_bias_desc &b) {
  return (unsigned __int128)(b.period0 - 1) * (unsigned __int128)b.s0 + (unsigned __int128)(b.period1 - 1) * (unsigned __int128)b.s1 +
         (unsigned __int128)(bias_rows(d, b) - 1) * (unsigned __int128)b.ld + (unsigned __int128)d.n;
}
inline unsigned long long bias_host_elems(const dfx_bmm_desc &d, const dfx_logit_bias_desc &b) { return (unsigned long long)bias_host_span(d, b); }

inline unsigned __int128 bias_image_elems128(const dfx_bmm_desc &d, const dfx_logit_bias_desc &b) {
  return (unsigned __int128)bias_tables(b) * (unsigned __int128)bias_rows(d, b) * (unsigned __int128)bias_cols(d);
}
inline unsigned long long bias_image_elems(const dfx_bmm_desc &d, const dfx_logit_bias_desc &b) { return (unsigned long long)bias_image_elems128(d, b); }
inline unsigned long long bias_image_bytes(const dfx_bmm_desc &d, const dfx_logit_bias_desc &b) { return bias_image_elems(d, b) * sizeof(float); }

// DFX_OK, or the code dfx_bmm_set_bias returns with *why set to the reason, for a layout against a VALID descriptor.
// Everything DFX_ERR_INVALID is found before the one DFX_ERR_UNSUPPORTED.
inline int bias_validate(const dfx_bmm_desc &d, const dfx_logit_bias_desc &b, const char **why) {
  const char *dummy;
  if (!why) why = &dummy;
  *why = "";
  if (b.period0 < 1 || b.period0 > d.batch0) return *why = "period0 outside 1 .. batch0", DFX_ERR_INVALID;
  if (b.period1 < 1 || b.period1 > d.batch1) return *why = "period1 outside 1 .. batch1", DFX_ERR_INVALID;
  if (b.s0 < 0 || b.s1 < 0 || b.ld < 0) return *why = "negative stride", DFX_ERR_INVALID;
  if (b.ld != 0 && b.ld < d.n) return *why = "ld below n (0 broadcasts one row over m)", DFX_ERR_INVALID;
  if (bias_host_span(d, b) >= (unsigned __int128)BMM_MAX_ELEMS) return *why = "the table's index range reaches 2^40 floats", DFX_ERR_INVALID;
  if (bias_image_elems128(d, b) * sizeof(float) > (unsigned __int128)BIAS_IMAGE_MAX_BYTES)
    return *why = "the device image {period0 * period1, m or 1, up32(n)} f32 exceeds 2^30 bytes", DFX_ERR_UNSUPPORTED;
  return DFX_OK;
}

// THE IMAGE INDEX, as the kernels compute it: table (b0 % period0, b1 % period1), row m (0 where the image has one row), col n
inline size_t bias_image_index(int period0, int period1, long long rows, long long cols, long long b0, long long b1, long long m, long long n) {
  const long long t = (b0 % period0) * period1 + (b1 % period1);
  return (size_t)((t * rows + (rows == 1 ? 0 : m)) * cols + n);
}
inline size_t bias_host_index(const dfx_logit_bias_desc &b, long long p0, long long p1, long long m, long long n) {
  return (size_t)(p0 * b.s0 + p1 * b.s1 + m * b.ld + n);
}

struct BiasScan {
  double max_abs = 0.0;   // over the finite addressed entries
  bool has_ninf = false;  // a -inf among them
};
// DFX_OK, or DFX_ERR_INVALID for a +inf or NaN among the addressed entries
inline int bias_scan(const dfx_bmm_desc &d, const dfx_logit_bias_desc &b, const float *table, BiasScan *out) {
  BiasScan s;
  const long long rows = bias_rows(d, b);
  for (long long p0 = 0; p0 < b.period0; ++p0)
    for (long long p1 = 0; p1 < b.period1; ++p1)
      for (long long m = 0; m < rows; ++m) {
        const float *row = table + bias_host_index(b, p0, p1, m, 0);
        for (long long n = 0; n < d.n; ++n) {
          const float v = row[n];
          if (std::isnan(v) || (std::isinf(v) && v > 0)) return DFX_ERR_INVALID;
          if (std::isinf(v)) s.has_ninf = true;
          else if (std::fabs((double)v) > s.max_abs) s.max_abs = std::fabs((double)v);
        }
      }
  if (out) *out = s;
  return DFX_OK;
}

// the device image: img has bias_image_elems floats; pads (n .. up32(n) - 1 of every row) are zero
inline void bias_fill_image(const dfx_bmm_desc &d, const dfx_logit_bias_desc &b, const float *table, float *img) {
  const long long rows = bias_rows(d, b), cols = bias_cols(d);
  for (long long p0 = 0; p0 < b.period0; ++p0)
    for (long long p1 = 0; p1 < b.period1; ++p1)
      for (long long m = 0; m < rows; ++m) {
        const float *src = table + bias_host_index(b, p0, p1, m, 0);
        float *dst = img + bias_image_index(b.period0, b.period1, rows, cols, p0, p1, m, 0);
        for (long long n = 0; n < d.n; ++n) dst[n] = src[n];
        for (long long n = d.n; n < cols; ++n) dst[n] = 0.0f;
      }
}

// the distinct bytes of the tables: a period whose stride is 0 addresses one table (dfx_bmm_query's algorithmic_bytes)
inline unsigned long long bias_distinct_bytes(const dfx_bmm_desc &d, const dfx_logit_bias_desc &b) {
  const unsigned long long t0 = b.s0 == 0 ? 1 : (unsigned long long)b.period0, t1 = b.s1 == 0 ? 1 : (unsigned long long)b.period1;
  return t0 * t1 * (unsigned long long)bias_rows(d, b) * (unsigned long long)d.n * sizeof(float);
}

// the fast requant route's proof with a bias: bmm_fast_ok's conditions with (bound + max |bias|) * |scale| <= 2^30
// (requant_host.h's fast_ok_2p30) and NO non-finite entry: gc_quarter<FAST>'s (int)rintf is not defined on -inf
inline bool bmm_fast_ok_biased(const dfx_bmm_desc &d, const float *scales, const BiasScan &s) {
  if (d.round_mode != DFX_ROUND_NEAREST || s.has_ninf || !std::isfinite(s.max_abs)) return false;
  const double bound = bmm_acc_bound(d);
  for (int i = 0; i < d.nscales; ++i) {
    if (!std::isfinite(scales[i])) return false;
    if ((bound + s.max_abs) * std::fabs((double)scales[i]) > 1073741824.0) return false;  // 2^30
  }
  return true;
}

}  // namespace dfx
