// roialign_check -- runs deepfusion::roi_align of the drop-in C++ API (include/deepfusion.h) and compares every result, bit
// for bit, with the scalar restatement of roialign_host.h: u8 / s8 / f32, one to four levels, the batched form with and
// without count, the list form with indices outside the batch, c_valid below C.  A last case chains box_nms() ->
// roi_align() on the device, submitted asynchronously with no host step in between.  Prints one line per case, "ok" or
// "DIFFERENT", then PASS or FAIL; exits non-zero on a difference.
//   roialign_check
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
#include "roialign_host.h"

using namespace deepfusion;
typedef memory::dtype DT;

static std::unique_ptr<memory> mk(int n, int c, int h, int w, DT dt) {
  return std::unique_ptr<memory>(new memory(memory::nchw_dims{n, c, h, w}, memory::format::nhwc, dt));
}

static int report(const char *name, const std::string &what, bool bad) {
  printf("roialign_check %-14s %s: %s\n", name, what.c_str(), bad ? "DIFFERENT from the scalar reference" : "ok");
  return bad ? 1 : 0;
}

template <typename T> struct dt_of;
template <> struct dt_of<uint8_t> { static DT v() { return DT::u8; } static int code() { return DFX_U8; } static const char *name() { return "u8"; } };
template <> struct dt_of<int8_t> { static DT v() { return DT::s8; } static int code() { return DFX_S8; } static const char *name() { return "s8"; } };
template <> struct dt_of<float> { static DT v() { return DT::f32; } static int code() { return DFX_F32; } static const char *name() { return "f32"; } };

template <typename T> static void fill(memory &m, RoiRng &g) {
  T *p = (T *)m.data();
  for (size_t i = 0; i < m.size(); ++i) p[i] = sizeof(T) == 4 ? (T)g.uniform(-60.f, 60.f) : (T)(g.next() & 0xff);
}

// levels of an image of img_w x img_h at strides 4, 8, 16, 32 ...; list = the list form with some indices outside the batch
template <typename T>
static int check(const char *name, int bs, int n, int levels, int C, int c_valid, int img_w, int img_h, int ph, int pw, int S, bool aligned, bool list,
                 bool with_count, RoiRng &g) {
  std::vector<std::unique_ptr<memory> > lv;
  std::vector<memory *> lp;
  std::vector<float> scales, thr(levels > 1 ? levels - 1 : 0);
  dfx_roialign_desc d;
  memset(&d, 0, sizeof(d));
  for (int l = 0; l < levels; ++l) {
    const int st = 4 << l, h = std::max(1, img_h / st), w = std::max(1, img_w / st);
    lv.push_back(mk(bs, C, h, w, dt_of<T>::v()));
    fill<T>(*lv.back(), g);
    lp.push_back(lv.back().get());
    scales.push_back(1.0f / (float)st);
    d.h[l] = h; d.w[l] = w; d.src_ld[l] = C; d.spatial_scale[l] = scales.back();
  }
  if (levels > 1) roi_level_thresholds(2, 1 + levels, thr.data(), 56.0);
  for (int i = 0; i + 1 < levels; ++i) d.level_area_thr[i] = thr[i];
  const int R = list ? n : bs * n;
  auto boxes = list ? mk(R, 4, 1, 1, DT::f32) : mk(bs, 4, n, 1, DT::f32);
  roi_random_boxes(g, R, (float)img_w, (float)img_h, 6.f, (float)std::max(img_w, img_h), (float *)boxes->data());
  auto count = mk(bs, 1, 1, 1, DT::s32);
  for (int r = 0; r < bs; ++r) ((int32_t *)count->data())[r] = r == 0 ? n / 2 : r == 1 ? n + 3 : -1;
  auto bidx = mk(R, 1, 1, 1, DT::s32);
  for (int i = 0; i < R; ++i) ((int32_t *)bidx->data())[i] = i % 7 == 3 ? -1 : i % 11 == 5 ? bs : (int32_t)(g.next() % (uint32_t)bs);
  auto dst = mk(R, C, ph, pw, dt_of<T>::v());
  memset(dst->data(), 0xCD, dst->buffer_size());
  d.bs = bs; d.n = n; d.mode = list ? DFX_ROI_LIST : DFX_ROI_BATCHED; d.levels = levels; d.c = c_valid > 0 ? c_valid : C; d.dt = dt_of<T>::code();
  d.ph = ph; d.pw = pw; d.sampling_ratio = S; d.aligned = aligned; d.dst_ld = C;
  std::vector<T> want((size_t)R * ph * pw * C);
  memset(want.data(), 0xCD, want.size() * sizeof(T));
  std::vector<const T *> sp;
  for (auto &m : lv) sp.push_back((const T *)m->host_data());
  roialign_host<T>(d, sp.data(), (const float *)boxes->host_data(), !list && with_count ? (const int32_t *)count->host_data() : nullptr,
                   list ? (const int32_t *)bidx->host_data() : nullptr, want.data());
  roi_align(lp, scales, thr, boxes.get(), !list && with_count ? count.get() : nullptr, list ? bidx.get() : nullptr, dst, S, aligned, c_valid)->submit();
  size_t nonzero = 0;
  for (size_t i = 0; i < want.size(); ++i) nonzero += want[i] != (T)0;
  char what[200];
  snprintf(what, sizeof(what), "%s bs %d n %d %s%s, %d level(s) C %d (valid %d), %dx%d S %d aligned %d, %zu of %zu non-zero", dt_of<T>::name(), bs, n,
           list ? "list" : "batched", with_count ? " +count" : "", levels, C, d.c, ph, pw, S, (int)aligned, nonzero, want.size());
  // channels c_valid .. C-1 of dst are not written by the op: only the valid ones are compared
  bool differs = false;
  const T *got = (const T *)dst->host_data();
  for (size_t px = 0; px < (size_t)R * ph * pw && !differs; ++px) differs = memcmp(got + px * C, want.data() + px * C, (size_t)d.c * sizeof(T)) != 0;
  return report(name, what, differs || nonzero == 0);
}

// box_nms() -> roi_align(): kept boxes and count never leave the device in between
static int chain(RoiRng &g) {
  const int bs = 2, n = 300, max_out = 60, C = 32, img_w = 256, img_h = 192, levels = 3;
  const float iou = 0.5f;
  auto boxes = mk(bs, 4, n, 1, DT::f32);
  roi_random_boxes(g, bs * n, (float)img_w, (float)img_h, 10.f, 200.f, (float *)boxes->data());
  auto keep = mk(bs, max_out, 1, 1, DT::s32), count = mk(bs, 1, 1, 1, DT::s32);
  auto bout = mk(bs, 4, max_out, 1, DT::f32);
  std::vector<std::unique_ptr<memory> > lv;
  std::vector<memory *> lp;
  std::vector<float> scales, thr(levels - 1);
  dfx_roialign_desc d;
  memset(&d, 0, sizeof(d));
  for (int l = 0; l < levels; ++l) {
    const int st = 4 << l;
    lv.push_back(mk(bs, C, img_h / st, img_w / st, DT::u8));
    fill<uint8_t>(*lv.back(), g);
    lp.push_back(lv.back().get());
    scales.push_back(1.0f / (float)st);
    d.h[l] = img_h / st; d.w[l] = img_w / st; d.src_ld[l] = C; d.spatial_scale[l] = scales.back();
  }
  roi_level_thresholds(2, 4, thr.data(), 56.0);
  for (int i = 0; i + 1 < levels; ++i) d.level_area_thr[i] = thr[i];
  auto dst = mk(bs * max_out, C, 7, 7, DT::u8);
  auto nms = box_nms(boxes, nullptr, nullptr, keep, count, bout.get(), iou, 0);
  auto roi = roi_align(lp, scales, thr, bout.get(), count.get(), nullptr, dst, 2, true);
  nms->submit_async();
  roi->submit_async();
  roi->wait();
  nms->wait();
  for (memory *m : {keep.get(), count.get(), bout.get(), dst.get()}) m->download();
  dfx_nms_desc nd;
  memset(&nd, 0, sizeof(nd));
  nd.bs = bs; nd.n = n; nd.max_out = max_out; nd.keep_ld = max_out; nd.mode = DFX_NMS_BOXES; nd.classes = 1; nd.anchors_per_pixel = 1;
  nd.n_anchors = 2147483647; nd.idx_ld = n; nd.iou_thr = iou;
  std::vector<int32_t> wkeep((size_t)bs * max_out), wcount(bs);
  std::vector<float> wbox((size_t)bs * max_out * 4);
  nms_host(nd, (const float *)boxes->host_data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, wkeep.data(), wcount.data(), wbox.data());
  d.bs = bs; d.n = max_out; d.mode = DFX_ROI_BATCHED; d.levels = levels; d.c = C; d.dt = DFX_U8; d.ph = d.pw = 7; d.sampling_ratio = 2; d.aligned = 1;
  d.dst_ld = C;
  std::vector<uint8_t> want((size_t)bs * max_out * 49 * C);
  std::vector<const uint8_t *> sp;
  for (auto &m : lv) sp.push_back((const uint8_t *)m->host_data());
  roialign_host<uint8_t>(d, sp.data(), wbox.data(), wcount.data(), nullptr, want.data());
  bool bad = memcmp(bout->host_data(), wbox.data(), wbox.size() * 4) != 0 || memcmp(count->host_data(), wcount.data(), wcount.size() * 4) != 0;
  bad = bad || memcmp(dst->host_data(), want.data(), want.size()) != 0;
  char what[200];
  snprintf(what, sizeof(what), "bs 2 n 300 -> kept %d / %d, 3 levels C 32 u8, 7x7 S 2 aligned, asynchronous", wcount[0], wcount[1]);
  return report("nms->roialign", what, bad);
}

int main() {
  RoiRng g(2026);
  int bad = 0, n = 0;
  bad += check<uint8_t>("fpn box head", 2, 100, 4, 64, 0, 320, 256, 7, 7, 2, false, false, true, g); ++n;
  bad += check<uint8_t>("mask head", 3, 20, 4, 32, 0, 320, 256, 14, 14, 2, true, false, false, g); ++n;
  bad += check<int8_t>("list", 2, 77, 2, 16, 0, 128, 96, 5, 3, 3, true, true, false, g); ++n;
  bad += check<float>("f32 c4", 1, 40, 1, 8, 0, 64, 64, 14, 14, 2, true, false, false, g); ++n;
  bad += check<float>("f32 list", 3, 33, 3, 6, 0, 96, 128, 2, 2, 4, false, true, false, g); ++n;
  bad += check<uint8_t>("c_valid", 2, 9, 2, 32, 20, 64, 48, 3, 3, 1, false, false, true, g); ++n;
  bad += check<int8_t>("1x1 map", 2, 5, 1, 16, 0, 4, 4, 64, 1, 4, true, false, false, g); ++n;
  bad += chain(g); ++n;
  if (bad) {
    printf("roialign_check: %d of %d cases differ\nFAIL\n", bad, n);
    return 1;
  }
  printf("roialign_check: every case identical to the scalar reference (%d cases)\nPASS\n", n);
  return 0;
}
