// roialign_host.h -- the scalar restatement of RoIAlign (include/dfx.h, dfx_roialign_desc) the tools compare the device
// against, and the generators roialign_check and bench_roialign share.  Plain C++; every floating-point step is one float
// operation in the order of the definition (the host Makefile neither contracts nor reassociates).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "dfx.h"

struct RoiRng {  // xorshift64*
  uint64_t s;
  explicit RoiRng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 1) {}
  uint32_t next() {
    s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
    return (uint32_t)((s * 0x2545F4914F6CDD1Dull) >> 32);
  }
  float uniform(float lo, float hi) { return lo + (hi - lo) * (float)(next() >> 8) * (1.0f / 16777216.0f); }
};

// n boxes over a w x h image: sizes log-uniform between min_side and max_side, centres anywhere, a few reaching outside
inline void roi_random_boxes(RoiRng &g, int n, float w, float h, float min_side, float max_side, float *out) {
  for (int i = 0; i < n; ++i) {
    const float bw = min_side * std::exp(g.uniform(0.f, 1.f) * std::log(max_side / min_side));
    const float bh = min_side * std::exp(g.uniform(0.f, 1.f) * std::log(max_side / min_side));
    const float cx = g.uniform(0.f, w), cy = g.uniform(0.f, h);
    out[4 * i] = cx - 0.5f * bw; out[4 * i + 1] = cy - 0.5f * bh; out[4 * i + 2] = cx + 0.5f * bw; out[4 * i + 3] = cy + 0.5f * bh;
  }
}

// torchvision's LevelMapper as area thresholds (capi.roi_level_thresholds): levels k_min .. k_max
inline void roi_level_thresholds(int k_min, int k_max, float *thr, double s0 = 224.0, double k0 = 4.0, double eps = 1e-6) {
  for (int k = k_min + 1; k <= k_max; ++k) {
    const double side = s0 * std::exp2((double)k - k0 - eps);
    thr[k - k_min - 1] = (float)(side * side);
  }
}

struct RoiHostAxis {
  int lo, hi;
  float l, h;
  bool valid;
};
inline RoiHostAxis roi_host_axis(float start, float bin, int p, int i, int S, int L) {
  const float a = (float)p * bin;
  const float b = start + a;
  const float c = (float)i + 0.5f;
  const float d = c * bin;
  const float e = d / (float)S;
  float y = b + e;
  RoiHostAxis r = {0, 0, 0.f, 0.f, false};
  r.valid = y >= -1.0f && y <= (float)L;
  if (!r.valid) return r;
  if (y <= 0.f) y = 0.f;
  int yl = (int)y, yh;
  if (yl >= L - 1) {
    yh = yl = L - 1;
    y = (float)yl;
  } else {
    yh = yl + 1;
  }
  r.lo = yl; r.hi = yh;
  r.l = y - (float)yl;
  r.h = 1.0f - r.l;
  return r;
}

template <typename T> inline T roi_host_cvt(float v) {
  const float r = std::nearbyint(v);  // ties to even in the default rounding mode
  const float lo = (T)-1 < (T)0 ? -128.f : 0.f, hi = (T)-1 < (T)0 ? 127.f : 255.f;
  return (T)(r < lo ? lo : r > hi ? hi : r);
}
template <> inline float roi_host_cvt<float>(float v) { return v; }

// dst {R, ph, pw, dst_ld}: elements c .. dst_ld-1 are left alone
template <typename T>
void roialign_host(const dfx_roialign_desc &d, const T *const *src, const float *boxes, const int32_t *count, const int32_t *batch_idx, T *dst) {
  const long long R = d.mode == DFX_ROI_LIST ? d.n : (long long)d.bs * d.n;
  const int S = d.sampling_ratio;
  for (long long r = 0; r < R; ++r) {
    T *out = dst + (size_t)r * d.ph * d.pw * d.dst_ld;
    int img;
    bool live;
    if (d.mode == DFX_ROI_BATCHED) {
      img = (int)(r / d.n);
      int nv = d.n;
      if (count) nv = count[img] < 0 ? 0 : count[img] > d.n ? d.n : count[img];
      live = (int)(r % d.n) < nv;
    } else {
      img = batch_idx[r];
      live = img >= 0 && img < d.bs;
    }
    if (!live) {
      for (int px = 0; px < d.ph * d.pw; ++px)
        for (int ch = 0; ch < d.c; ++ch) out[(size_t)px * d.dst_ld + ch] = (T)0;
      continue;
    }
    const float x1 = boxes[4 * r], y1 = boxes[4 * r + 1], x2 = boxes[4 * r + 2], y2 = boxes[4 * r + 3];
    const float dw = x2 - x1, dh = y2 - y1;
    const float area = dw * dh;
    int lv = 0;
    for (int i = 0; i + 1 < d.levels; ++i)
      if (area >= d.level_area_thr[i]) ++lv;
    const int H = d.h[lv], W = d.w[lv], ld = d.src_ld[lv];
    const T *im = src[lv] + (size_t)img * H * W * ld;
    const float s = d.spatial_scale[lv], o = d.aligned ? 0.5f : 0.0f;
    float rsw = x1 * s; rsw = rsw - o;
    float rsh = y1 * s; rsh = rsh - o;
    float rew = x2 * s; rew = rew - o;
    float reh = y2 * s; reh = reh - o;
    float rw = rew - rsw, rh = reh - rsh;
    if (!d.aligned) {
      rw = rw > 1.0f ? rw : 1.0f;
      rh = rh > 1.0f ? rh : 1.0f;
    }
    const float bw = rw / (float)d.pw, bh = rh / (float)d.ph;
    for (int p = 0; p < d.ph; ++p)
      for (int q = 0; q < d.pw; ++q)
        for (int ch = 0; ch < d.c; ++ch) {
          float acc = 0.0f;
          for (int iy = 0; iy < S; ++iy) {
            const RoiHostAxis y = roi_host_axis(rsh, bh, p, iy, S, H);
            for (int ix = 0; ix < S; ++ix) {
              const RoiHostAxis x = roi_host_axis(rsw, bw, q, ix, S, W);
              if (!y.valid || !x.valid) continue;  // adds +0.0f: the bits of acc stay
              const float w1 = y.h * x.h, w2 = y.h * x.l, w3 = y.l * x.h, w4 = y.l * x.l;
              const float t1 = w1 * (float)im[((size_t)y.lo * W + x.lo) * ld + ch], t2 = w2 * (float)im[((size_t)y.lo * W + x.hi) * ld + ch];
              const float t3 = w3 * (float)im[((size_t)y.hi * W + x.lo) * ld + ch], t4 = w4 * (float)im[((size_t)y.hi * W + x.hi) * ld + ch];
              float sm = t1 + t2;
              sm = sm + t3;
              sm = sm + t4;
              acc = acc + sm;
            }
          }
          out[((size_t)p * d.pw + q) * d.dst_ld + ch] = roi_host_cvt<T>(acc / (float)(S * S));
        }
  }
}
