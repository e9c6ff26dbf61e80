// nms_host.h -- the scalar host loop nms_check compares the library with and bench_nms times as "what a caller does today":
// the box decode and the greedy NMS of include/dfx.h (dfx_nms_desc), one f32 operation per step in the order written there.
// Plain C++; the tools are built for baseline x86-64, which has no fused multiply-add to contract the steps into.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "dfx.h"

struct NmsHostBox { float x1, y1, x2, y2; };

static inline float nms_host_clip(float x, float hi) {
  x = x < 0.0f ? 0.0f : x;
  return x > hi ? hi : x;
}

static inline bool nms_host_over(const NmsHostBox &a, const NmsHostBox &b, float thr) {
  const float area_a = (a.x2 - a.x1) * (a.y2 - a.y1), area_b = (b.x2 - b.x1) * (b.y2 - b.y1);
  const float xx1 = a.x1 > b.x1 ? a.x1 : b.x1, yy1 = a.y1 > b.y1 ? a.y1 : b.y1;
  const float xx2 = a.x2 < b.x2 ? a.x2 : b.x2, yy2 = a.y2 < b.y2 ? a.y2 : b.y2;
  float w = xx2 - xx1, h = yy2 - yy1;
  w = w > 0.0f ? w : 0.0f;
  h = h > 0.0f ? h : 0.0f;
  const float inter = w * h;
  const float u = (area_a + area_b) - inter;
  return inter / u > thr;
}

// keep {bs, max_out} (keep_ld = max_out), count {bs}, boxes_out {bs, max_out, 4} or null; host pointers throughout
static inline void nms_host(const dfx_nms_desc &d, const float *boxes, const int32_t *idx, const uint8_t *deltas, const float *anchors,
                            const float *tab_c, const float *tab_s, const int32_t *count_in, int32_t *keep, int32_t *count, float *boxes_out) {
  std::vector<NmsHostBox> bx((size_t)d.n);
  std::vector<int> lab((size_t)d.n);
  const bool reads_idx = d.mode == DFX_NMS_DECODE || d.per_class;
  const long long entries = (long long)d.n_anchors * d.classes;
  for (int r = 0; r < d.bs; ++r) {
    int nv = d.n;
    if (count_in) nv = count_in[r] < 0 ? 0 : count_in[r] > d.n ? d.n : count_in[r];
    for (int j = 0; j < nv; ++j) {
      int e = 0;
      bool ok = true;
      if (reads_idx) {
        e = idx[(size_t)r * d.idx_ld + j];
        ok = e >= 0 && e < entries;
      }
      lab[j] = !ok ? -1 : d.per_class ? e % d.classes : 0;
      NmsHostBox b = {0, 0, 0, 0};
      if (d.mode == DFX_NMS_BOXES) {
        memcpy(&b, boxes + ((size_t)r * d.n + j) * 4, 16);
      } else if (ok) {
        const int g = e / d.classes, a = g % d.anchors_per_pixel;
        const uint8_t *q = deltas + ((size_t)r * d.n + j) * d.row_bytes + 4 * a;
        const float *A = anchors + (size_t)g * 4;
        const float aw = A[2] - A[0], ah = A[3] - A[1];
        const float acx = A[0] + 0.5f * aw, acy = A[1] + 0.5f * ah;
        const float cx = acx + tab_c[q[0]] * aw, cy = acy + tab_c[q[1]] * ah;
        const float w = aw * tab_s[q[2]], hh = ah * tab_s[q[3]];
        const float hw = 0.5f * w, hhh = 0.5f * hh;
        b.x1 = cx - hw; b.y1 = cy - hhh; b.x2 = cx + hw; b.y2 = cy + hhh;
        if (d.clip_w > 0.0f) {
          b.x1 = nms_host_clip(b.x1, d.clip_w); b.x2 = nms_host_clip(b.x2, d.clip_w);
          b.y1 = nms_host_clip(b.y1, d.clip_h); b.y2 = nms_host_clip(b.y2, d.clip_h);
        }
      }
      bx[j] = b;
    }
    int32_t *kp = keep + (size_t)r * d.max_out;
    int cnt = 0;
    for (int j = 0; j < nv && cnt < d.max_out; ++j) {
      if (lab[j] < 0) continue;
      bool sup = false;
      for (int i = 0; i < cnt && !sup; ++i) sup = lab[kp[i]] == lab[j] && nms_host_over(bx[kp[i]], bx[j], d.iou_thr);
      if (!sup) kp[cnt++] = j;
    }
    count[r] = cnt;
    for (int i = 0; i < d.max_out; ++i) {
      if (boxes_out) {
        const NmsHostBox z = {0, 0, 0, 0};
        memcpy(boxes_out + ((size_t)r * d.max_out + i) * 4, i < cnt ? &bx[kp[i]] : &z, 16);
      }
      if (i >= cnt) kp[i] = -1;
    }
  }
}

// ---- seeded generators shared by the two tools ----------------------------------------------------------------------------
struct NmsRng {
  uint64_t s;
  explicit NmsRng(uint64_t seed) : s(seed * 2654435761u + 88172645463325252ull) {}
  uint32_t next() {
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;
    return (uint32_t)(s >> 32);
  }
  float uniform(float lo, float hi) { return lo + (hi - lo) * (float)(next() >> 8) / 16777216.0f; }
};

// n boxes around `clusters` centres in a 1024 x 1024 image: sides 24 .. 56, centres within +-jitter of their cluster's
static inline void nms_clustered_boxes(NmsRng &g, int n, int clusters, float jitter, float *out) {
  std::vector<float> cx((size_t)clusters), cy((size_t)clusters);
  for (int c = 0; c < clusters; ++c) { cx[c] = g.uniform(32, 992); cy[c] = g.uniform(32, 992); }
  for (int j = 0; j < n; ++j) {
    const int c = (int)(g.next() % (uint32_t)clusters);
    const float x = cx[c] + g.uniform(-jitter, jitter), y = cy[c] + g.uniform(-jitter, jitter);
    const float w = g.uniform(24, 56), h = g.uniform(24, 56);
    out[4 * j + 0] = x - 0.5f * w; out[4 * j + 1] = y - 0.5f * h; out[4 * j + 2] = x + 0.5f * w; out[4 * j + 3] = y + 0.5f * h;
  }
}
