// resize_plan.h -- the per-axis tables of the activation resize (dfx_resize_* of include/dfx.h): for every output index
// the two source indices and their two weights.  Plain C++ with no HIP: resize_api.hip uploads what this builds,
// tools/resize_plan_check.cc prints it (under sanitizers too) and tests/resize_ref.py re-derives it in numpy.  This is
// the only place that computes the tables: the kernels read them, so one kernel serves all three coordinate modes.
// All index arithmetic is exact 64-bit integer arithmetic; the one float operation per entry is w1's division.
#pragma once

#include <stdint.h>

#include <vector>

#include "../../include/dfx.h"

namespace dfx {

constexpr int RESIZE_MAX_SIZE = 65535;  // remainders and denominators stay below 2^24: float(.) of them is exact

struct ResizeAxis {
  std::vector<int32_t> i0, i1;
  std::vector<float> w0, w1;
};

// false for a size outside 1 .. RESIZE_MAX_SIZE or an unknown algo / coord (nothing is written then)
inline bool resize_axis_plan(int in, int out, int algo, int coord, ResizeAxis &t) {
  if (in < 1 || in > RESIZE_MAX_SIZE || out < 1 || out > RESIZE_MAX_SIZE) return false;
  if (algo != DFX_RESIZE_NEAREST && algo != DFX_RESIZE_BILINEAR) return false;
  if (coord != DFX_COORD_HALF_PIXEL && coord != DFX_COORD_ALIGN_CORNERS && coord != DFX_COORD_ASYMMETRIC) return false;
  t.i0.assign((size_t)out, 0);
  t.i1.assign((size_t)out, 0);
  t.w0.assign((size_t)out, 1.0f);
  t.w1.assign((size_t)out, 0.0f);
  const int64_t n = in, m = out;
  for (int64_t o = 0; o < m; ++o) {
    int64_t num, den;
    if (coord == DFX_COORD_HALF_PIXEL) { num = (2 * o + 1) * n - m; den = 2 * m; }
    else if (coord == DFX_COORD_ALIGN_CORNERS) { num = m == 1 ? 0 : o * (n - 1); den = m == 1 ? 1 : m - 1; }
    else { num = o * n; den = m; }
    if (algo == DFX_RESIZE_BILINEAR) {
      if (num < 0) num = 0;
      int64_t a = num / den;
      if (a > n - 1) a = n - 1;
      const int64_t b = a + 1 < n - 1 ? a + 1 : n - 1;
      const float w1 = (float)(num % den) / (float)den;
      t.i0[(size_t)o] = (int32_t)a;
      t.i1[(size_t)o] = (int32_t)b;
      t.w1[(size_t)o] = w1;
      t.w0[(size_t)o] = 1.0f - w1;
    } else {
      int64_t idx;
      if (coord == DFX_COORD_HALF_PIXEL) idx = ((2 * o + 1) * n) / (2 * m);
      else if (coord == DFX_COORD_ASYMMETRIC) idx = (o * n) / m;
      else idx = (2 * num + den) / (2 * den);  // round half up
      if (idx > n - 1) idx = n - 1;
      t.i0[(size_t)o] = t.i1[(size_t)o] = (int32_t)idx;
    }
  }
  return true;
}

}  // namespace dfx
