// bench_catconv -- times the concat + pointwise conv op on MI355X through the public C ABI (include/dfx.h), four legs
// in ONE process on the same device buffers:
//   (a) dfx_catconv_submit, fused path (one launch)
//   (b) dfx_concat_submit + dfx_conv_submit back to back            (what a caller does without the op)
//   (c) dfx_conv_submit alone on the pre-concatenated tensor         (the fused launch's byte-for-byte twin)
//   (d) dfx_catconv_submit with force_path = DFX_CATCONV_TWO_LAUNCH  (the op's own fallback)
// Protocol: every timed submit works on the next of several buffer sets (>= 768 MB in rotation, so that the 256 MiB
// Infinity Cache serves no leg); per shape `rounds` rounds; a round times each leg in turn (a, b, c, d, so that drift
// hits all alike) as `iter` back-to-back submits between two device events on one stream, after `burning_iter` warm-up submits of
// every leg.  Reported: the median round of each leg in us per submit, the ratios the op is judged by, and the HBM
// fraction of (a): algorithmic_bytes / time against 8 TB/s.  The four results are compared byte for byte first.
//   bench_catconv [-iter 200] [-burning_iter 50] [-rounds 7] [-shape k]   (k: 0..3, default all)
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cli_flags.h"
#include "dfx.h"

#define CK(x)                                                                  \
  do {                                                                         \
    if ((x) != DFX_OK) {                                                       \
      fprintf(stderr, "%s failed: %s\n", #x, dfx_last_error());                \
      exit(1);                                                                 \
    }                                                                          \
  } while (0)

struct Shape {
  const char *name;
  int bs, h, w, oc, dst_dt;
  std::vector<int32_t> ch;
};

static double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

int main(int argc, char **argv) {
  Flags f(argc, argv);
  const int iters = f.geti("iter", 200), burn = f.geti("burning_iter", 50), rounds = f.geti("rounds", 7), only = f.geti("shape", -1);
  const std::vector<Shape> shapes = {
      {"N128 56x56 128+128 -> 64 u8", 128, 56, 56, 64, DFX_U8, {128, 128}},
      {"N128 28x28 64+128+32+32 -> 128 u8", 128, 28, 28, 128, DFX_U8, {64, 128, 32, 32}},
      {"N64 28x28 256+8x32 -> 128 u8", 64, 28, 28, 128, DFX_U8, {256, 32, 32, 32, 32, 32, 32, 32, 32}},
      {"N128 56x56 128+128 -> 64 s32", 128, 56, 56, 64, DFX_S32, {128, 128}},
  };
  char dev[256];
  CK(dfx_device_name(dev, sizeof(dev)));
  printf("bench_catconv on %s: iter %d, burning_iter %d, rounds %d (median round reported)\n", dev, iters, burn, rounds);
  for (size_t si = 0; si < shapes.size(); ++si) {
    if (only >= 0 && (int)si != only) continue;
    const Shape &s = shapes[si];
    const size_t px = (size_t)s.bs * s.h * s.w;
    int ic = 0;
    for (int c : s.ch) ic += c;
    const size_t esz = (s.dst_dt == DFX_U8 || s.dst_dt == DFX_S8) ? 1 : 4, dst_bytes = px * s.oc * esz;
    Lcg g(99 + (uint32_t)si);
    // buffer sets: every timed submit works on the next set, enough sets to cycle through >= 768 MB of branches + dst
    // (three times the 256 MiB Infinity Cache), so that no leg is served from it.  Leg (c) has a pre-concatenated
    // tensor per set; leg (b) concatenates into ONE scratch buffer, as the op's own two-launch path (d) does.
    size_t set_bytes = dst_bytes;
    for (int c : s.ch) set_bytes += px * c;
    const int nsets = (int)std::min<size_t>(64, std::max<size_t>(2, ((size_t)768 << 20) / set_bytes + 1));
    std::vector<std::vector<void *>> d_src(nsets, std::vector<void *>(s.ch.size()));
    std::vector<void *> d_pre(nsets), d_out(nsets);
    for (int q = 0; q < nsets; ++q) {
      for (size_t k = 0; k < s.ch.size(); ++k) {
        std::vector<uint8_t> hsrc(px * s.ch[k]);
        for (auto &v : hsrc) v = (uint8_t)(g.next() % 256);
        CK(dfx_mem_alloc_device(&d_src[q][k], hsrc.size()));
        CK(dfx_memcpy_h2d(d_src[q][k], hsrc.data(), hsrc.size(), nullptr));
        CK(dfx_stream_sync(nullptr));
      }
      CK(dfx_mem_alloc_device(&d_pre[q], px * ic));
      CK(dfx_mem_alloc_device(&d_out[q], dst_bytes));
    }
    void *d_cat = nullptr, *d_dst[4];
    CK(dfx_mem_alloc_device(&d_cat, px * ic));
    for (auto &p : d_dst) CK(dfx_mem_alloc_device(&p, dst_bytes));
    // weights
    std::vector<int8_t> w((size_t)s.oc * ic), wb(w.size());
    for (auto &v : w) v = (int8_t)((int)(g.next() % 21) - 10);
    CK(dfx_reorder_oihw_to_blocked(w.data(), wb.data(), s.oc, ic, 1, 1));
    std::vector<int32_t> bias(s.oc);
    for (auto &v : bias) v = (int)(g.next() % 2001) - 1000;
    const float scale = 1.0f / 512;
    // handles
    dfx_catconv_desc cd;
    memset(&cd, 0, sizeof(cd));
    cd.n_inputs = (int)s.ch.size(); cd.bs = s.bs; cd.h = s.h; cd.w = s.w; cd.oc = s.oc; cd.dst_dt = s.dst_dt;
    cd.bia_dt = DFX_S32; cd.relu = 1; cd.round_mode = DFX_ROUND_NEAREST; cd.nscales = 1; cd.channels = s.ch.data();
    dfx_catconv_t *fused = nullptr, *two = nullptr;
    cd.force_path = DFX_CATCONV_FUSED;
    CK(dfx_catconv_create(&cd, &fused));
    cd.force_path = DFX_CATCONV_TWO_LAUNCH;
    CK(dfx_catconv_create(&cd, &two));
    CK(dfx_catconv_set_weights(fused, wb.data(), bias.data(), &scale));
    CK(dfx_catconv_set_weights(two, wb.data(), bias.data(), &scale));
    dfx_concat_desc kd;
    memset(&kd, 0, sizeof(kd));
    kd.n_inputs = cd.n_inputs; kd.bs = s.bs; kd.h = s.h; kd.w = s.w; kd.dt = DFX_U8; kd.channels = s.ch.data();
    dfx_concat_t *cat = nullptr;
    CK(dfx_concat_create(&kd, &cat));
    dfx_conv_desc vd;
    memset(&vd, 0, sizeof(vd));
    vd.bs = s.bs; vd.ic = ic; vd.ih = vd.oh = s.h; vd.iw = vd.ow = s.w; vd.oc = s.oc; vd.kh = vd.kw = vd.sh = vd.sw = 1;
    vd.dst_dt = s.dst_dt; vd.bia0_dt = DFX_S32; vd.conv0_relu = 1; vd.conv0_nscales = vd.conv1_nscales = 1; vd.force_variant = -1;
    dfx_conv_t *conv = nullptr;
    CK(dfx_conv_create(&vd, &conv));
    CK(dfx_conv_set_weights(conv, wb.data(), bias.data(), &scale, nullptr, nullptr, nullptr));
    dfx_catconv_info fi, ti;
    dfx_conv_info vi;
    CK(dfx_catconv_query(fused, &fi));
    CK(dfx_catconv_query(two, &ti));
    CK(dfx_conv_query(conv, &vi));
    dfx_stream_t st = nullptr;
    CK(dfx_stream_create(&st));
    // q < 0: the comparison run on set 0, every leg into a buffer of its own
    auto leg = [&](int which, int q) {
      const int qq = q < 0 ? 0 : q;
      const void *const *srcs = (const void *const *)d_src[qq].data();
      void *out = q < 0 ? d_dst[which] : d_out[qq];
      switch (which) {
        case 0: CK(dfx_catconv_submit(fused, srcs, out, st)); break;
        case 1: CK(dfx_concat_submit(cat, srcs, d_cat, st)); CK(dfx_conv_submit(conv, d_cat, out, st)); break;
        case 2: CK(dfx_conv_submit(conv, d_pre[qq], out, st)); break;
        case 3: CK(dfx_catconv_submit(two, srcs, out, st)); break;
      }
    };
    for (int q = 0; q < nsets; ++q) CK(dfx_concat_submit(cat, (const void *const *)d_src[q].data(), d_pre[q], st));  // (c)'s inputs
    for (int which = 0; which < 4; ++which) leg(which, -1);
    CK(dfx_stream_sync(st));
    {  // same bytes from every leg
      std::vector<uint8_t> r0(dst_bytes), r(dst_bytes);
      CK(dfx_memcpy_d2h(r0.data(), d_dst[1], dst_bytes, st));
      CK(dfx_stream_sync(st));
      for (int k : {0, 2, 3}) {
        CK(dfx_memcpy_d2h(r.data(), d_dst[k], dst_bytes, st));
        CK(dfx_stream_sync(st));
        if (memcmp(r0.data(), r.data(), dst_bytes) != 0) {
          fprintf(stderr, "bench_catconv: leg %c differs from concat + conv on %s\n", "abcd"[k], s.name);
          return 1;
        }
      }
    }
    int turn = 0;
    for (int which = 0; which < 4; ++which)
      for (int i = 0; i < burn; ++i) leg(which, turn++ % nsets);
    CK(dfx_stream_sync(st));
    dfx_event_t e0, e1;
    CK(dfx_event_create(&e0));
    CK(dfx_event_create(&e1));
    std::vector<double> us[4];
    for (int r = 0; r < rounds; ++r)
      for (int which = 0; which < 4; ++which) {
        CK(dfx_event_record(e0, st));
        for (int i = 0; i < iters; ++i) leg(which, turn++ % nsets);
        CK(dfx_event_record(e1, st));
        float ms = 0;
        CK(dfx_event_elapsed_ms(e0, e1, &ms));
        us[which].push_back(1e3 * ms / iters);
      }
    const double a = median(us[0]), b = median(us[1]), c = median(us[2]), d = median(us[3]);
    printf("\n%s   (results of the four legs byte-identical; %d buffer sets of %.1f MB in rotation)\n", s.name, nsets, set_bytes / 1e6);
    printf("  fused kernel     %s  grid %d lds %d\n", fi.kernel_name, fi.grid, fi.lds_bytes);
    printf("  conv kernel      %s  grid %d lds %d\n", vi.kernel_name, vi.grid, vi.lds_bytes);
    printf("  (a) fused op                 %8.2f us   min %.2f max %.2f\n", a, *std::min_element(us[0].begin(), us[0].end()), *std::max_element(us[0].begin(), us[0].end()));
    printf("  (b) concat + conv            %8.2f us   min %.2f max %.2f\n", b, *std::min_element(us[1].begin(), us[1].end()), *std::max_element(us[1].begin(), us[1].end()));
    printf("  (c) conv alone               %8.2f us   min %.2f max %.2f\n", c, *std::min_element(us[2].begin(), us[2].end()), *std::max_element(us[2].begin(), us[2].end()));
    printf("  (d) op, two-launch path      %8.2f us   min %.2f max %.2f\n", d, *std::min_element(us[3].begin(), us[3].end()), *std::max_element(us[3].begin(), us[3].end()));
    printf("  a/c %.3f   b/a %.2f x (traffic ratio %.2f)   d/b %.3f\n", a / c, b / a, (double)ti.algorithmic_bytes / (double)fi.algorithmic_bytes, d / b);
    printf("  (a) %.1f MB algorithmic -> %.2f TB/s = %.2f of 8 TB/s;  %.1f TOP/s\n", fi.algorithmic_bytes / 1e6,
           fi.algorithmic_bytes / a / 1e6, fi.algorithmic_bytes / a / 1e6 / 8.0, fi.algorithmic_ops / a / 1e6);
    CK(dfx_event_destroy(e0));
    CK(dfx_event_destroy(e1));
    CK(dfx_stream_sync(st));
    CK(dfx_catconv_destroy(fused));
    CK(dfx_catconv_destroy(two));
    CK(dfx_concat_destroy(cat));
    CK(dfx_conv_destroy(conv));
    CK(dfx_stream_destroy(st));
    for (int q = 0; q < nsets; ++q) {
      for (void *p : d_src[q]) CK(dfx_mem_free_device(p));
      CK(dfx_mem_free_device(d_pre[q]));
      CK(dfx_mem_free_device(d_out[q]));
    }
    CK(dfx_mem_free_device(d_cat));
    for (void *p : d_dst) CK(dfx_mem_free_device(p));
  }
  return 0;
}
