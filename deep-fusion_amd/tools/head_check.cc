// head_check -- runs deepfusion::argmax / top_k / softmax of the drop-in C++ API (include/deepfusion.h) and compares every
// result, bit for bit, with a scalar reference in this file: top-k by a sequential insertion under the total order of
// include/dfx.h (integers as themselves, f32 by totalOrder on the bit pattern, the lower channel first among equals),
// softmax as float(E[d]) / float(S) with an exact integer S and rint(p * out_scale) clamped for a u8 dst.  Two frames chain
// ops on the device with no host step in between: inner_product() -> top_k() and resize() -> argmax(), submitted
// asynchronously and compared with the reference on the producer's downloaded result; a last one keeps two head ops of one
// source in flight at once.  Prints one line per case, "ok" or "DIFFERENT"; exits non-zero on a difference.
//   head_check
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "cli_flags.h"
#include "deepfusion.h"
#include "dfx.h"

using namespace deepfusion;
typedef memory::dtype DT;

static std::unique_ptr<memory> mk(int n, int c, int h, int w, DT dt, memory::format f = memory::format::nhwc) {
  return std::unique_ptr<memory>(new memory(memory::nchw_dims{n, c, h, w}, f, dt));
}
static size_t esize(DT dt) { return (dt == DT::f32 || dt == DT::s32) ? 4 : 1; }

// the element's place in the total order, as a signed 64-bit number
static long long order_of(const unsigned char *p, DT dt) {
  if (dt == DT::u8) return *p;
  if (dt == DT::s8) return *(const signed char *)p;
  uint32_t bits;
  memcpy(&bits, p, 4);
  if (dt == DT::s32) return (int32_t)bits;
  const long long mag = bits & 0x7fffffffu;
  return (bits >> 31) ? -mag - 1 : mag;
}

// idx as int32 {rows, k}; val as raw elements {rows, k}
static void ref_topk(const unsigned char *src, DT dt, long long rows, int ld, int c, int k, std::vector<int32_t> &idx, std::vector<unsigned char> &val) {
  const size_t es = esize(dt);
  idx.assign((size_t)rows * k, 0);
  val.assign((size_t)rows * k * es, 0);
  for (long long r = 0; r < rows; ++r) {
    const unsigned char *row = src + (size_t)r * ld * es;
    std::vector<int> best;
    for (int j = 0; j < c; ++j) {
      size_t at = best.size();
      while (at > 0 && order_of(row + (size_t)j * es, dt) > order_of(row + (size_t)best[at - 1] * es, dt)) --at;  // strictly: ties keep the lower channel first
      best.insert(best.begin() + at, j);
      if ((int)best.size() > k) best.pop_back();
    }
    for (int t = 0; t < k; ++t) {
      idx[(size_t)r * k + t] = best[t];
      memcpy(&val[((size_t)r * k + t) * es], row + (size_t)best[t] * es, es);
    }
  }
}

static void ref_softmax(const unsigned char *src, DT dt, long long rows, int ld, int c, const std::array<uint32_t, 256> &E, DT dst_dt, int dst_ld, float out_scale,
                        std::vector<unsigned char> &dst) {  // dst: as it was before the op; the pad elements stay
  const size_t ds = esize(dst_dt);
  for (long long r = 0; r < rows; ++r) {
    const unsigned char *row = src + (size_t)r * ld;
    int m = -1000;
    for (int j = 0; j < c; ++j) m = std::max(m, (int)order_of(row + j, dt));
    uint64_t sum = 0;
    for (int j = 0; j < c; ++j) sum += E[m - (int)order_of(row + j, dt)];
    const float fs = (float)(uint32_t)sum;
    for (int j = 0; j < c; ++j) {
      volatile float p = (float)E[m - (int)order_of(row + j, dt)] / fs;
      unsigned char *o = &dst[((size_t)r * dst_ld + j) * ds];
      if (dst_dt == DT::f32) {
        const float f = p;
        memcpy(o, &f, 4);
      } else {
        volatile float v = p * out_scale;
        const float q = nearbyintf(v);
        *o = (unsigned char)(q < 0.f ? 0.f : q > 255.f ? 255.f : q);
      }
    }
  }
}

static void fill(memory &m, Lcg &g, int c_valid) {  // pad channels hold the largest values
  const DT dt = m.data_type();
  const int C = m.std_dims()[1];
  void *p = m.data();
  for (size_t i = 0; i < m.size(); ++i) {
    const unsigned r = g.next();
    const bool pad = (int)(i % C) >= c_valid;
    if (dt == DT::f32) {
      float v = (float)((int)(r % 401) - 200) * 0.25f;
      if (r % 29 == 0) v = -0.0f;
      if (r % 31 == 0) v = INFINITY;
      uint32_t bits;
      memcpy(&bits, &v, 4);
      if (r % 37 == 0) bits = 0xffc00000u | (r & 0xffff);  // -NaN with a payload
      if (r % 41 == 0) bits = 0x7fc00000u | (r & 0xffff);  // +NaN with a payload
      if (pad) bits = 0x7fffffffu;
      memcpy((char *)p + i * 4, &bits, 4);
    } else if (dt == DT::s32) {
      ((int32_t *)p)[i] = pad ? 2147483647 : (r % 5 == 0 ? (int32_t)(r * 2654435761u) : (int32_t)(r % 7) - 3);
    } else if (dt == DT::s8) {
      ((int8_t *)p)[i] = pad ? 127 : (int8_t)((int)(r % 200) - 128);
    } else {
      ((uint8_t *)p)[i] = pad ? 255 : (uint8_t)(r % 230);
    }
  }
}

static std::array<uint32_t, 256> exp_table(double step, int c) {
  std::array<uint32_t, 256> e;
  const double top = (double)(0xffffffffu / (uint32_t)c);
  for (int d = 0; d < 256; ++d) e[d] = (uint32_t)std::floor(std::exp(-d * step) * top);
  return e;
}

static int report(const char *name, const std::string &what, bool bad) {
  printf("head_check %-14s %s: %s\n", name, what.c_str(), bad ? "DIFFERENT from the scalar reference" : "ok");
  return bad ? 1 : 0;
}

static bool idx_differs(memory &idx, const std::vector<int32_t> &want) {
  const void *p = idx.host_data();
  for (size_t i = 0; i < want.size(); ++i) {
    const int got = idx.data_type() == DT::u8 ? ((const uint8_t *)p)[i] : ((const int32_t *)p)[i];
    if (got != want[i]) return true;
  }
  return false;
}

// the c valid channels of every row (the op leaves the pad elements of dst's device copy as they are)
static bool rows_differ(const void *got, const std::vector<unsigned char> &want, long long rows, int ld, int c, size_t es) {
  for (long long r = 0; r < rows; ++r)
    if (memcmp((const unsigned char *)got + (size_t)r * ld * es, &want[(size_t)r * ld * es], (size_t)c * es) != 0) return true;
  return false;
}

static int check_topk(const char *name, int bs, int C, int h, int w, DT dt, DT idx_dt, int k, int c_valid, bool with_val, Lcg &g) {
  auto src = mk(bs, C, h, w, dt);
  fill(*src, g, c_valid ? c_valid : C);
  auto idx = mk(bs, k, h, w, idx_dt);
  auto val = mk(bs, k, h, w, dt);
  memset(idx->data(), 0xCD, idx->buffer_size());
  memset(val->data(), 0xCD, val->buffer_size());
  std::vector<int32_t> wi;
  std::vector<unsigned char> wv;
  ref_topk((const unsigned char *)src->host_data(), dt, (long long)bs * h * w, C, c_valid ? c_valid : C, k, wi, wv);
  auto op = (k == 1 && !with_val) ? argmax(src, idx, c_valid) : top_k(src, idx, with_val ? val.get() : nullptr, k, c_valid);
  op->submit();
  bool bad = idx_differs(*idx, wi);
  if (with_val) bad = bad || memcmp(val->host_data(), wv.data(), wv.size()) != 0;
  char what[160];
  snprintf(what, sizeof(what), "bs %d %dx%d c %d/%d k %d%s", bs, h, w, c_valid ? c_valid : C, C, k, with_val ? " +val" : "");
  return report(name, what, bad);
}

static int check_softmax(const char *name, int bs, int C, int h, int w, DT dt, DT dst_dt, int dst_C, int c_valid, float out_scale, double step, Lcg &g) {
  auto src = mk(bs, C, h, w, dt);
  const int c = c_valid ? c_valid : C;
  fill(*src, g, c);
  auto dst = mk(bs, dst_C, h, w, dst_dt);
  memset(dst->data(), 0xCD, dst->buffer_size());
  std::vector<unsigned char> want(dst->buffer_size(), 0xCD);
  const std::array<uint32_t, 256> E = exp_table(step, c);
  ref_softmax((const unsigned char *)src->host_data(), dt, (long long)bs * h * w, C, c, E, dst_dt, dst_C, out_scale, want);
  softmax(src, E, dst, out_scale, c_valid)->submit();
  char what[160];
  snprintf(what, sizeof(what), "bs %d %dx%d c %d/%d -> %s ld %d", bs, h, w, c, C, dst_dt == DT::f32 ? "f32" : "u8", dst_C);
  return report(name, what, rows_differ(dst->host_data(), want, (long long)bs * h * w, dst_C, c, esize(dst_dt)));
}

// inner_product() -> top_k(), both submitted asynchronously: the logits never leave the device in between
static int frame_classifier(Lcg &g) {
  const int bs = 4, c = 64, oc = 1000, k = 5;
  auto src = mk(bs, c, 1, 1, DT::u8);
  auto wei = mk(oc, c, 1, 1, DT::s8, memory::format::oihw);
  for (size_t i = 0; i < src->size(); ++i) ((uint8_t *)src->data())[i] = (uint8_t)(g.next() % 256);
  for (size_t i = 0; i < wei->size(); ++i) ((int8_t *)wei->data())[i] = (int8_t)((int)(g.next() % 256) - 128);
  std::unique_ptr<memory> bia;
  auto logits = mk(bs, oc, 1, 1, DT::s32);
  auto idx = mk(bs, k, 1, 1, DT::s32);
  auto val = mk(bs, k, 1, 1, DT::s32);
  auto fc = inner_product(src, wei, bia, logits);
  auto tk = top_k(logits, idx, val.get(), k);
  fc->submit_async();
  tk->submit_async();
  tk->wait();
  fc->wait();
  logits->download();
  idx->download();
  val->download();
  std::vector<int32_t> wi;
  std::vector<unsigned char> wv;
  ref_topk((const unsigned char *)logits->host_data(), DT::s32, bs, oc, oc, k, wi, wv);
  const bool bad = idx_differs(*idx, wi) || memcmp(val->host_data(), wv.data(), wv.size()) != 0;
  return report("fc->top_k", "bs 4 64 -> 1000 s32, k 5 +val, asynchronous", bad);
}

// resize() -> argmax(): a segmentation net's last two layers
static int frame_segmentation(Lcg &g) {
  const int bs = 2, C = 32, c = 21;
  auto small = mk(bs, C, 9, 11, DT::u8);
  fill(*small, g, c);
  auto logits = mk(bs, C, 33, 41, DT::u8);
  auto idx = mk(bs, 1, 33, 41, DT::u8);
  auto rs = resize(small, logits, resize_algo::bilinear, resize_coord::align_corners);
  auto am = argmax(logits, idx, c);
  rs->submit_async();
  am->submit_async();
  am->wait();
  rs->wait();
  logits->download();
  idx->download();
  std::vector<int32_t> wi;
  std::vector<unsigned char> wv;
  ref_topk((const unsigned char *)logits->host_data(), DT::u8, (long long)bs * 33 * 41, C, c, 1, wi, wv);
  return report("resize->argmax", "bs 2 9x11 -> 33x41 c 21/32, asynchronous", idx_differs(*idx, wi));
}

// two head ops of one source in flight at once
static int frame_two_in_flight(Lcg &g) {
  const int bs = 3, C = 32, c = 19, h = 17, w = 13;
  auto src = mk(bs, C, h, w, DT::s8);
  fill(*src, g, c);
  auto idx = mk(bs, 1, h, w, DT::s32);
  auto prob = mk(bs, C, h, w, DT::u8);
  memset(prob->data(), 0xCD, prob->buffer_size());
  const std::array<uint32_t, 256> E = exp_table(0.125, c);
  auto am = argmax(src, idx, c);
  auto sm = softmax(src, E, prob, 255.f, c);
  am->submit_async();
  sm->submit_async();
  sm->wait();
  am->wait();
  idx->download();
  prob->download();
  std::vector<int32_t> wi;
  std::vector<unsigned char> wv, wp(prob->buffer_size(), 0xCD);
  ref_topk((const unsigned char *)src->host_data(), DT::s8, (long long)bs * h * w, C, c, 1, wi, wv);
  ref_softmax((const unsigned char *)src->host_data(), DT::s8, (long long)bs * h * w, C, c, E, DT::u8, C, 255.f, wp);
  const bool bad = idx_differs(*idx, wi) || rows_differ(prob->host_data(), wp, (long long)bs * h * w, C, c, 1);
  return report("two in flight", "argmax + softmax of one s8 tensor, submit_async on both", bad);
}

int main() {
  Lcg g(4242);
  int bad = 0, n = 0;
  bad += check_topk("seg argmax", 2, 32, 5, 7, DT::u8, DT::u8, 1, 21, false, g); ++n;
  bad += check_topk("ade argmax", 1, 160, 9, 11, DT::s8, DT::s32, 1, 150, false, g); ++n;
  bad += check_topk("argmax +val", 2, 48, 3, 5, DT::u8, DT::u8, 1, 33, true, g); ++n;
  bad += check_topk("top5 f32", 3, 1000, 1, 1, DT::f32, DT::s32, 5, 0, true, g); ++n;
  bad += check_topk("top8 s32", 2, 40, 3, 3, DT::s32, DT::u8, 8, 37, true, g); ++n;
  bad += check_topk("top5 s8", 4, 1008, 1, 1, DT::s8, DT::s32, 5, 1000, false, g); ++n;
  bad += check_topk("odd ld", 3, 21, 4, 5, DT::u8, DT::u8, 3, 0, true, g); ++n;
  bad += check_softmax("seg softmax", 2, 32, 5, 7, DT::u8, DT::u8, 32, 21, 255.f, 0.0625, g); ++n;
  bad += check_softmax("seg softmax", 2, 32, 5, 7, DT::s8, DT::f32, 21, 21, 255.f, 0.125, g); ++n;
  bad += check_softmax("cls softmax", 3, 1008, 1, 1, DT::s8, DT::f32, 1000, 1000, 255.f, 0.05, g); ++n;
  bad += check_softmax("odd ld", 3, 21, 4, 5, DT::u8, DT::u8, 23, 0, 100.f, 0.25, g); ++n;
  bad += frame_classifier(g); ++n;
  bad += frame_segmentation(g); ++n;
  bad += frame_two_in_flight(g); ++n;
  if (bad) {
    printf("head_check: %d of %d cases FAILED\n", bad, n);
    return 1;
  }
  printf("head_check: every case identical to the scalar reference (%d cases)\n", n);
  return 0;
}
