// nms_check -- runs deepfusion::box_nms of the drop-in C++ API (include/deepfusion.h) and compares every result, bit for
// bit, with the scalar loop of nms_host.h: both overloads, per class and class-agnostic, count_in, max_out that cuts the walk
// off, no boxes_out.  A last case chains conv() -> select_top_k() -> box_nms() on the device with no host step in between,
// everything submitted asynchronously and two frames in flight at once.  Prints one line per case, "ok" or "DIFFERENT";
// exits non-zero on a difference.
//   nms_check
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "cli_flags.h"
#include "deepfusion.h"
#include "dfx.h"
#include "nms_host.h"

using namespace deepfusion;
typedef memory::dtype DT;

static std::unique_ptr<memory> mk(int n, int c, int h, int w, DT dt, memory::format f = memory::format::nhwc) {
  return std::unique_ptr<memory>(new memory(memory::nchw_dims{n, c, h, w}, f, dt));
}

static void tables(std::array<float, 256> &tc, std::array<float, 256> &ts) {  // u8 deltas, zero point 128, step 1/32, weights 10 / 5
  for (int q = 0; q < 256; ++q) {
    const double d = (q - 128) / 32.0;
    tc[q] = (float)(d / 10.0);
    ts[q] = (float)std::exp(std::min(d / 5.0, std::log(1000.0 / 16)));
  }
}

static int report(const char *name, const std::string &what, bool bad) {
  printf("nms_check %-18s %s: %s\n", name, what.c_str(), bad ? "DIFFERENT from the scalar reference" : "ok");
  return bad ? 1 : 0;
}

struct Want {
  std::vector<int32_t> keep, count;
  std::vector<float> boxes;
};
static Want want_of(const dfx_nms_desc &d, const float *boxes, const int32_t *idx, const uint8_t *deltas, const float *anchors, const float *tc,
                    const float *ts, const int32_t *count_in) {
  Want w;
  w.keep.assign((size_t)d.bs * d.max_out, 0);
  w.count.assign(d.bs, 0);
  w.boxes.assign((size_t)d.bs * d.max_out * 4, 0);
  nms_host(d, boxes, idx, deltas, anchors, tc, ts, count_in, w.keep.data(), w.count.data(), w.boxes.data());
  return w;
}
static bool differs(const Want &w, memory &keep, memory &count, memory *bout) {
  bool bad = memcmp(keep.host_data(), w.keep.data(), w.keep.size() * 4) != 0;
  bad = bad || memcmp(count.host_data(), w.count.data(), w.count.size() * 4) != 0;
  if (bout) bad = bad || memcmp(bout->host_data(), w.boxes.data(), w.boxes.size() * 4) != 0;
  return bad;
}

static int check_boxes(const char *name, int bs, int n, int max_out, int classes, float thr, bool with_count, bool with_boxes, NmsRng &g) {
  auto boxes = mk(bs, 4, n, 1, DT::f32);
  for (int r = 0; r < bs; ++r) nms_clustered_boxes(g, n, std::max(1, n / 10), 8.f, (float *)boxes->data() + (size_t)r * n * 4);
  auto idx = mk(bs, n, 1, 1, DT::s32);
  for (size_t i = 0; i < idx->size(); ++i) ((int32_t *)idx->data())[i] = (int32_t)(g.next() % 1000u) * std::max(1, classes) + (int32_t)(g.next() % (uint32_t)std::max(1, classes));
  auto cin = mk(bs, 1, 1, 1, DT::s32);
  for (int r = 0; r < bs; ++r) ((int32_t *)cin->data())[r] = r == 0 ? n / 2 : r == 1 ? n + 3 : 0;
  auto keep = mk(bs, max_out, 1, 1, DT::s32), count = mk(bs, 1, 1, 1, DT::s32);
  auto bout = mk(bs, 4, max_out, 1, DT::f32);
  memset(keep->data(), 0xCD, keep->buffer_size());
  memset(count->data(), 0xCD, count->buffer_size());
  memset(bout->data(), 0xCD, bout->buffer_size());
  dfx_nms_desc d;
  memset(&d, 0, sizeof(d));
  d.bs = bs; d.n = n; d.max_out = max_out; d.keep_ld = max_out; d.mode = DFX_NMS_BOXES; d.per_class = classes > 0; d.classes = std::max(1, classes);
  d.anchors_per_pixel = 1; d.n_anchors = 2147483647 / d.classes; d.idx_ld = n; d.iou_thr = thr;
  const Want w = want_of(d, (const float *)boxes->host_data(), (const int32_t *)idx->host_data(), nullptr, nullptr, nullptr, nullptr,
                         with_count ? (const int32_t *)cin->host_data() : nullptr);
  box_nms(boxes, classes > 0 ? idx.get() : nullptr, with_count ? cin.get() : nullptr, keep, count, with_boxes ? bout.get() : nullptr, thr, classes)->submit();
  char what[200];
  snprintf(what, sizeof(what), "boxes bs %d n %d max_out %d %s thr %.2f%s%s, counts %d..", bs, n, max_out, classes > 0 ? "per class" : "agnostic", thr,
           with_count ? " +count_in" : "", with_boxes ? " +boxes_out" : "", w.count[0]);
  return report(name, what, differs(w, *keep, *count, with_boxes ? bout.get() : nullptr));
}

static void fill_anchors(memory &anchors, int cells, int apx, NmsRng &g) {  // cells in clusters, apx shapes per cell
  float *a = (float *)anchors.data();
  std::vector<float> c((size_t)cells * 4);
  nms_clustered_boxes(g, cells, std::max(1, cells / 6), 10.f, c.data());
  for (int p = 0; p < cells; ++p)
    for (int s = 0; s < apx; ++s) {
      const float cx = 0.5f * (c[4 * p] + c[4 * p + 2]), cy = 0.5f * (c[4 * p + 1] + c[4 * p + 3]);
      const float hw = 16.f + 4.f * (float)(s % 3), hh = 16.f + 4.f * (float)((s / 3) % 3);
      float *o = a + ((size_t)p * apx + s) * 4;
      o[0] = cx - hw; o[1] = cy - hh; o[2] = cx + hw; o[3] = cy + hh;
    }
}

static int check_decode(const char *name, int bs, int n, int max_out, int classes, bool per_class, int apx, int row_c, float thr, float clip_w,
                        float clip_h, NmsRng &g) {
  const int cells = 200, na = cells * apx;
  auto idx = mk(bs, n, 1, 1, DT::s32);
  for (size_t i = 0; i < idx->size(); ++i) ((int32_t *)idx->data())[i] = (int32_t)(g.next() % (uint32_t)(na * classes));
  ((int32_t *)idx->data())[3] = -1;                       // invalid entries inside the count
  ((int32_t *)idx->data())[n - 1] = na * classes;
  auto deltas = mk(bs, row_c, n, 1, DT::u8);
  for (size_t i = 0; i < deltas->buffer_size(); ++i) ((uint8_t *)deltas->data())[i] = (uint8_t)(g.next() & 0xff);
  auto anchors = mk(na, 4, 1, 1, DT::f32);
  fill_anchors(*anchors, cells, apx, g);
  std::array<float, 256> tc, ts;
  tables(tc, ts);
  auto keep = mk(bs, max_out, 1, 1, DT::s32), count = mk(bs, 1, 1, 1, DT::s32);
  auto bout = mk(bs, 4, max_out, 1, DT::f32);
  memset(keep->data(), 0xCD, keep->buffer_size());
  memset(count->data(), 0xCD, count->buffer_size());
  memset(bout->data(), 0xCD, bout->buffer_size());
  dfx_nms_desc d;
  memset(&d, 0, sizeof(d));
  d.bs = bs; d.n = n; d.max_out = max_out; d.keep_ld = max_out; d.mode = DFX_NMS_DECODE; d.per_class = per_class; d.classes = classes;
  d.anchors_per_pixel = apx; d.n_anchors = na; d.row_bytes = row_c; d.idx_ld = n; d.iou_thr = thr; d.clip_w = clip_w; d.clip_h = clip_h;
  const Want w = want_of(d, nullptr, (const int32_t *)idx->host_data(), (const uint8_t *)deltas->host_data(), (const float *)anchors->host_data(),
                         tc.data(), ts.data(), nullptr);
  box_nms(idx, deltas, anchors, tc, ts, nullptr, keep, count, bout.get(), thr, classes, per_class, apx, clip_w, clip_h)->submit();
  char what[200];
  snprintf(what, sizeof(what), "decode bs %d n %d max_out %d classes %d %s A %d row %d thr %.2f clip %g x %g, counts %d..", bs, n, max_out, classes,
           per_class ? "per class" : "agnostic", apx, row_c, thr, clip_w, clip_h, w.count[0]);
  return report(name, what, differs(w, *keep, *count, bout.get()));
}

// conv() -> select_top_k() -> box_nms(): heat map, idx, count and the gathered delta rows never leave the device in
// between; two frames with their own tensors and ops are in flight at once
static int frames_detector(NmsRng &g) {
  const int bs = 2, ic = 32, oc = 32, h = 12, w = 10, apx = 3, classes = 5, k = 200, max_out = 50, frames = 2;
  const float thr = 0.5f, clip_w = 160.f, clip_h = 192.f;
  auto wei = mk(oc, ic, 3, 3, DT::s8, memory::format::OIhw4i16o4i);
  std::vector<s8> w0(wei->size());
  for (auto &v : w0) v = (s8)((int)(g.next() % 9u) - 4);
  reorder_weights(w0.data(), wei);
  std::unique_ptr<memory> bia;
  auto anchors = mk(h * w * apx, 4, 1, 1, DT::f32);
  for (int p = 0; p < h * w; ++p)
    for (int s = 0; s < apx; ++s) {
      float *o = (float *)anchors->data() + ((size_t)p * apx + s) * 4;
      const float cx = 16.f * (float)(p % w) + 8.f, cy = 16.f * (float)(p / w) + 8.f, hw = 16.f + 6.f * (float)s, hh = 28.f - 6.f * (float)s;
      o[0] = cx - hw; o[1] = cy - hh; o[2] = cx + hw; o[3] = cy + hh;
    }
  std::array<float, 256> tc, ts;
  tables(tc, ts);
  struct Frame {
    std::unique_ptr<memory> src, heat, dmap, idx, count, rows, keep, kcount, bout;
    std::unique_ptr<op> cv, sel, nms;
  } f[frames];
  for (int t = 0; t < frames; ++t) {
    f[t].src = mk(bs, ic, h, w, DT::u8);
    for (size_t i = 0; i < f[t].src->size(); ++i) ((uint8_t *)f[t].src->data())[i] = (uint8_t)(g.next() % 64u);
    f[t].heat = mk(bs, oc, h, w, DT::u8);
    f[t].dmap = mk(bs, 4 * apx, h, w, DT::u8);
    for (size_t i = 0; i < f[t].dmap->size(); ++i) ((uint8_t *)f[t].dmap->data())[i] = (uint8_t)(96u + g.next() % 64u);
    f[t].idx = mk(bs, k, 1, 1, DT::s32);
    f[t].count = mk(bs, 1, 1, 1, DT::s32);
    f[t].rows = mk(bs, 4 * apx, k, 1, DT::u8);
    f[t].keep = mk(bs, max_out, 1, 1, DT::s32);
    f[t].kcount = mk(bs, 1, 1, 1, DT::s32);
    f[t].bout = mk(bs, 4, max_out, 1, DT::f32);
    f[t].cv = conv(f[t].src, wei, bia, {1, 1}, {1, 1}, f[t].heat, true, {1.f / 16});
    f[t].sel = select_top_k(f[t].heat, f[t].idx, nullptr, f[t].count, k, false, 24, apx * classes, {f[t].dmap.get()}, {f[t].rows.get()});
    f[t].nms = box_nms(f[t].idx, f[t].rows, anchors, tc, ts, f[t].count.get(), f[t].keep, f[t].kcount, f[t].bout.get(), thr, classes, true, apx, clip_w,
                       clip_h);
  }
  for (int t = 0; t < frames; ++t) {
    f[t].cv->submit_async();
    f[t].sel->submit_async();
    f[t].nms->submit_async();
  }
  for (int t = frames - 1; t >= 0; --t) {
    f[t].nms->wait();
    f[t].sel->wait();
    f[t].cv->wait();
  }
  bool bad = false;
  int c00 = 0, k00 = 0;
  for (int t = 0; t < frames; ++t) {
    for (memory *m : {f[t].heat.get(), f[t].idx.get(), f[t].count.get(), f[t].rows.get(), f[t].keep.get(), f[t].kcount.get(), f[t].bout.get()}) m->download();
    // the select stage by its definition: value descending, element index ascending over the first apx * classes channels
    const uint8_t *hb = (const uint8_t *)f[t].heat->host_data(), *dm = (const uint8_t *)f[t].dmap->host_data();
    const int c = apx * classes;
    std::vector<int32_t> sidx((size_t)bs * k, -1), scount(bs, 0);
    std::vector<uint8_t> srows((size_t)bs * k * 4 * apx, 0);
    for (int n = 0; n < bs; ++n) {
      std::vector<std::pair<int, int> > cand;
      for (int p = 0; p < h * w; ++p)
        for (int ch = 0; ch < c; ++ch) {
          const int v = hb[((size_t)n * h * w + p) * oc + ch];
          if (v >= 24) cand.push_back(std::make_pair(-v, p * c + ch));
        }
      std::sort(cand.begin(), cand.end());
      scount[n] = (int)std::min<size_t>(cand.size(), (size_t)k);
      for (int j = 0; j < scount[n]; ++j) {
        sidx[(size_t)n * k + j] = cand[j].second;
        memcpy(&srows[((size_t)n * k + j) * 4 * apx], dm + ((size_t)n * h * w + cand[j].second / c) * 4 * apx, 4 * apx);
      }
    }
    bad = bad || memcmp(sidx.data(), f[t].idx->host_data(), sidx.size() * 4) != 0 || memcmp(srows.data(), f[t].rows->host_data(), srows.size()) != 0;
    dfx_nms_desc d;
    memset(&d, 0, sizeof(d));
    d.bs = bs; d.n = k; d.max_out = max_out; d.keep_ld = max_out; d.mode = DFX_NMS_DECODE; d.per_class = 1; d.classes = classes;
    d.anchors_per_pixel = apx; d.n_anchors = h * w * apx; d.row_bytes = 4 * apx; d.idx_ld = k; d.iou_thr = thr; d.clip_w = clip_w; d.clip_h = clip_h;
    const Want wt = want_of(d, nullptr, sidx.data(), srows.data(), (const float *)anchors->host_data(), tc.data(), ts.data(), scount.data());
    bad = bad || differs(wt, *f[t].keep, *f[t].kcount, f[t].bout.get());
    bad = bad || scount[0] < 10 || wt.count[0] < 2 || wt.count[0] >= scount[0];  // (a frame that kept nothing or everything would check little)
    if (t == 0) { c00 = scount[0]; k00 = wt.count[0]; }
  }
  char what[200];
  snprintf(what, sizeof(what), "bs 2 12x10 32 -> 15/32 u8, select k 200 min 24 + 12-byte delta rows (count %d), decode A 3 x 5 classes, kept %d; 2 frames in flight",
           c00, k00);
  return report("conv->select->nms", what, bad);
}

int main() {
  NmsRng g(2026);
  int bad = 0, n = 0;
  bad += check_boxes("agnostic", 2, 300, 300, 0, 0.5f, false, true, g); ++n;
  bad += check_boxes("per class", 3, 1000, 100, 80, 0.5f, false, true, g); ++n;
  bad += check_boxes("count_in", 3, 130, 130, 3, 0.3f, true, true, g); ++n;
  bad += check_boxes("cut, no boxes_out", 2, 2000, 7, 0, 0.7f, false, false, g); ++n;
  bad += check_boxes("one", 1, 1, 1, 0, 0.5f, false, true, g); ++n;
  bad += check_decode("retinanet", 2, 1000, 300, 80, true, 9, 36, 0.5f, 0.f, 0.f, g); ++n;
  bad += check_decode("rpn clip", 2, 2000, 1000, 1, false, 3, 16, 0.7f, 800.f, 600.f, g); ++n;
  bad += check_decode("ssd", 3, 200, 200, 21, true, 6, 24, 0.45f, 1024.f, 1024.f, g); ++n;
  bad += frames_detector(g); ++n;
  if (bad) {
    printf("nms_check: %d of %d cases FAILED\n", bad, n);
    return 1;
  }
  printf("nms_check: every case identical to the scalar reference (%d cases)\n", n);
  return 0;
}
