// select_check -- runs deepfusion::select_top_k of the drop-in C++ API (include/deepfusion.h) and compares every result,
// bit for bit, with a scalar reference in this file: the candidates by the definition of include/dfx.h (>= min_val; with
// peak3 also >= every 3x3 neighbour of the same channel inside the image), std::sort by (value descending, element index
// ascending), the first k, idx -1 / val 0 / zero gather rows from the count on.  One frame chains conv() -> select_top_k()
// on the device with no host step in between, both submitted asynchronously; a last one keeps two select ops of one heat map
// in flight at once.  Prints one line per case, "ok" or "DIFFERENT"; exits non-zero on a difference.
//   select_check
#include <algorithm>
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
static int value_of(const unsigned char *p, DT dt) { return dt == DT::u8 ? (int)*p : (int)*(const signed char *)p; }

struct Want {
  std::vector<int32_t> idx, count;
  std::vector<unsigned char> val;
  std::vector<std::vector<unsigned char> > rows;  // per gather map: {bs, k, row bytes}
};

// src: nhwc {bs, h, w, C}, c valid channels; gsrc[i]: {bs, h, w, rb[i]} bytes
static Want ref_select(const unsigned char *src, DT dt, int bs, int h, int w, int C, int c, int k, bool peak3, int min_val,
                       const std::vector<const unsigned char *> &gsrc, const std::vector<int> &rb) {
  Want r;
  r.idx.assign((size_t)bs * k, -1);
  r.val.assign((size_t)bs * k, 0);
  r.count.assign(bs, 0);
  for (size_t i = 0; i < gsrc.size(); ++i) r.rows.push_back(std::vector<unsigned char>((size_t)bs * k * rb[i], 0));
  for (int n = 0; n < bs; ++n) {
    const unsigned char *img = src + (size_t)n * h * w * C;
    std::vector<std::pair<int, int> > cand;  // (-value, e): ascending pairs are the op's order
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x)
        for (int ch = 0; ch < c; ++ch) {
          const int v = value_of(img + ((size_t)y * w + x) * C + ch, dt);
          bool ok = v >= min_val;
          for (int dy = -1; ok && peak3 && dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
              const int yy = y + dy, xx = x + dx;
              if (yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
              if (value_of(img + ((size_t)yy * w + xx) * C + ch, dt) > v) ok = false;
            }
          if (ok) cand.push_back(std::make_pair(-v, (y * w + x) * c + ch));
        }
    std::sort(cand.begin(), cand.end());
    const int cnt = (int)std::min<size_t>(cand.size(), (size_t)k);
    r.count[n] = cnt;
    for (int j = 0; j < cnt; ++j) {
      const int e = cand[j].second, p = e / c;
      r.idx[(size_t)n * k + j] = e;
      r.val[(size_t)n * k + j] = img[(size_t)p * C + e % c];
      for (size_t i = 0; i < gsrc.size(); ++i)
        memcpy(&r.rows[i][((size_t)n * k + j) * rb[i]], gsrc[i] + ((size_t)n * h * w + p) * rb[i], rb[i]);
    }
  }
  return r;
}

static void fill_scores(memory &m, Lcg &g, int c_valid) {  // a sparse heat map with ties; pad channels hold the largest value
  const DT dt = m.data_type();
  const int C = m.std_dims()[1];
  unsigned char *p = (unsigned char *)m.data();
  for (size_t i = 0; i < m.size(); ++i) {
    const unsigned r = g.next();
    int v = (int)(r % 7) * 3;                  // the floor: few distinct values
    if (r % 11 == 0) v = 100 + (int)(r % 5) * 30;
    if (r % 97 == 0) v = 255;
    if (dt == DT::s8) v -= 128;
    if ((int)(i % C) >= c_valid) v = dt == DT::s8 ? 127 : 255;
    p[i] = (unsigned char)v;
  }
}

static int report(const char *name, const std::string &what, bool bad) {
  printf("select_check %-16s %s: %s\n", name, what.c_str(), bad ? "DIFFERENT from the scalar reference" : "ok");
  return bad ? 1 : 0;
}

static bool differs(const Want &want, memory &idx, memory *val, memory &count, const std::vector<memory *> &gdst) {
  bool bad = memcmp(idx.host_data(), want.idx.data(), want.idx.size() * 4) != 0;
  bad = bad || memcmp(count.host_data(), want.count.data(), want.count.size() * 4) != 0;
  if (val) bad = bad || memcmp(val->host_data(), want.val.data(), want.val.size()) != 0;
  for (size_t i = 0; i < gdst.size(); ++i) bad = bad || memcmp(gdst[i]->host_data(), want.rows[i].data(), want.rows[i].size()) != 0;
  return bad;
}

static int check_select(const char *name, int bs, int C, int h, int w, DT dt, int k, bool peak3, int min_val, int c_valid, bool with_val,
                        int n_gather, Lcg &g) {
  const int c = c_valid ? c_valid : C;
  auto src = mk(bs, C, h, w, dt);
  fill_scores(*src, g, c);
  auto idx = mk(bs, k, 1, 1, DT::s32);
  auto val = mk(bs, k, 1, 1, dt);
  auto count = mk(bs, 1, 1, 1, DT::s32);
  memset(idx->data(), 0xCD, idx->buffer_size());
  memset(val->data(), 0xCD, val->buffer_size());
  memset(count->data(), 0xCD, count->buffer_size());
  // gather maps: wh as 2 x f32 and a 4 x u8 box code
  const DT gdt[2] = {DT::f32, DT::u8};
  const int gc[2] = {2, 4};
  std::vector<std::unique_ptr<memory> > gs, gd;
  std::vector<memory *> gsp, gdp;
  std::vector<const unsigned char *> gbytes;
  std::vector<int> rb;
  for (int i = 0; i < n_gather; ++i) {
    gs.push_back(mk(bs, gc[i], h, w, gdt[i]));
    gd.push_back(mk(bs, gc[i], k, 1, gdt[i]));
    unsigned char *p = (unsigned char *)gs.back()->data();
    for (size_t b = 0; b < gs.back()->buffer_size(); ++b) p[b] = (unsigned char)(g.next() & 0xff);
    memset(gd.back()->data(), 0xCD, gd.back()->buffer_size());
    gsp.push_back(gs.back().get());
    gdp.push_back(gd.back().get());
    gbytes.push_back((const unsigned char *)gs.back()->host_data());
    rb.push_back(gc[i] * (int)esize(gdt[i]));
  }
  const int mv = min_val == select_all_values ? (dt == DT::s8 ? -128 : 0) : min_val;
  const Want want = ref_select((const unsigned char *)src->host_data(), dt, bs, h, w, C, c, k, peak3, mv, gbytes, rb);
  select_top_k(src, idx, with_val ? val.get() : nullptr, count, k, peak3, min_val, c_valid, gsp, gdp)->submit();
  char what[200];
  snprintf(what, sizeof(what), "bs %d %dx%d c %d/%d %s k %d min %d%s, %d gather maps, counts %d..", bs, h, w, c, C, peak3 ? "peak3" : "all", k, mv,
           with_val ? " +val" : "", n_gather, want.count[0]);
  return report(name, what, differs(want, *idx, with_val ? val.get() : nullptr, *count, gdp));
}

// conv() -> select_top_k(): the u8 heat map never leaves the device in between; a second select op (no peak filter, a
// threshold) reads the same heat map on its own stream, so two ops are in flight behind the conv
static int frame_detector(Lcg &g) {
  const int bs = 2, ic = 32, oc = 32, h = 12, w = 10, classes = 20, k = 50, k2 = 300;
  auto src = mk(bs, ic, h, w, DT::u8);
  for (size_t i = 0; i < src->size(); ++i) ((uint8_t *)src->data())[i] = (uint8_t)(g.next() % 64);
  auto wei = mk(oc, ic, 3, 3, DT::s8, memory::format::OIhw4i16o4i);
  std::vector<s8> w0(wei->size());
  for (auto &v : w0) v = (s8)((int)(g.next() % 9) - 4);
  reorder_weights(w0.data(), wei);
  std::unique_ptr<memory> bia;
  auto heat = mk(bs, oc, h, w, DT::u8);
  auto wh = mk(bs, 2, h, w, DT::f32);
  for (size_t b = 0; b < wh->buffer_size(); ++b) ((unsigned char *)wh->data())[b] = (unsigned char)(g.next() & 0xff);
  auto idx = mk(bs, k, 1, 1, DT::s32), idx2 = mk(bs, k2, 1, 1, DT::s32);
  auto val = mk(bs, k, 1, 1, DT::u8), val2 = mk(bs, k2, 1, 1, DT::u8);
  auto count = mk(bs, 1, 1, 1, DT::s32), count2 = mk(bs, 1, 1, 1, DT::s32);
  auto boxes = mk(bs, 2, k, 1, DT::f32);
  auto cv = conv(src, wei, bia, {1, 1}, {1, 1}, heat, true, {1.f / 16});
  auto s1 = select_top_k(heat, idx, val.get(), count, k, true, 1, classes, {wh.get()}, {boxes.get()});
  auto s2 = select_top_k(heat, idx2, val2.get(), count2, k2, false, 40, classes);
  cv->submit_async();
  s1->submit_async();
  s2->submit_async();
  s2->wait();
  s1->wait();
  cv->wait();
  heat->download();
  for (memory *m : {idx.get(), val.get(), count.get(), boxes.get(), idx2.get(), val2.get(), count2.get()}) m->download();
  const unsigned char *hb = (const unsigned char *)heat->host_data();
  const Want w1 = ref_select(hb, DT::u8, bs, h, w, oc, classes, k, true, 1, {(const unsigned char *)wh->host_data()}, {8});
  const Want w2 = ref_select(hb, DT::u8, bs, h, w, oc, classes, k2, false, 40, {}, {});
  int distinct[256] = {0}, nd = 0;
  for (size_t i = 0; i < heat->size(); ++i) nd += !distinct[hb[i]]++;
  bool bad = nd < 8;  // (a conv that gave a flat map would check nothing)
  bad = bad || differs(w1, *idx, val.get(), *count, {boxes.get()}) || differs(w2, *idx2, val2.get(), *count2, {});
  char what[160];
  snprintf(what, sizeof(what), "bs 2 12x10 32 -> 20/32 u8; peak3 k 50 + wh rows (counts %d, %d) and all k 300 min 40 (counts %d, %d), asynchronous", w1.count[0],
           w1.count[1], w2.count[0], w2.count[1]);
  return report("conv->select x2", what, bad);
}

int main() {
  Lcg g(777);
  int bad = 0, n = 0;
  bad += check_select("centernet", 2, 80, 16, 16, DT::u8, 100, true, select_all_values, 0, true, 2, g); ++n;
  bad += check_select("padded classes", 3, 32, 5, 7, DT::s8, 7, true, -100, 21, true, 1, g); ++n;
  bad += check_select("threshold", 2, 96, 13, 16, DT::u8, 1000, false, 100, 91, true, 2, g); ++n;
  bad += check_select("k above n", 2, 16, 3, 3, DT::u8, 4096, false, select_all_values, 1, true, 0, g); ++n;
  bad += check_select("none pass", 2, 32, 5, 7, DT::u8, 20, false, 255, 21, true, 1, g); ++n;
  bad += check_select("row matrix", 4, 1008, 1, 1, DT::s8, 100, false, select_all_values, 1000, false, 0, g); ++n;
  bad += check_select("odd ld", 3, 7, 9, 4, DT::s8, 33, true, select_all_values, 5, true, 1, g); ++n;
  bad += frame_detector(g); ++n;
  if (bad) {
    printf("select_check: %d of %d cases FAILED\n", bad, n);
    return 1;
  }
  printf("select_check: every case identical to the scalar reference (%d cases)\n", n);
  return 0;
}
