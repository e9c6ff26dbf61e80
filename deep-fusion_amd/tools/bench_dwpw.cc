// bench_dwpw -- times the depthwise + pointwise conv op on MI355X through the public C ABI (include/dfx.h), in ONE
// process on the same device buffers:
//   (a) dfx_dwpw_submit, fused path (one launch, the u8 tensor between the stages in LDS)
//   (b) dfx_dwconv_submit + dfx_conv_submit as two ops through a u8 buffer: what a caller does without the op
//   (c) dfx_dwconv_submit alone
//   (d) dfx_dwpw_submit, two-launch path
// Protocol (bench_catconv's): every timed submit works on the next of several buffer sets (>= 768 MB in rotation, so
// that the 256 MiB Infinity Cache serves no leg); per shape `rounds` rounds; a round times each leg in turn as `iter`
// back-to-back submits between two device events on one stream, after `burning_iter` warm-up submits of every leg.
// Reported: the median round of each leg in us per submit, a/b, a/c, the traffic ratio (b)'s bytes / (a)'s bytes and
// the fraction of 8 TB/s on algorithmic_bytes.  (a), (b) and (d) are compared byte for byte first.  -cold_cache adds
// one-launch-at-a-time legs of (a) with warm caches and with 512 MiB of scratch rewritten before every launch.
//   bench_dwpw [-iter 100] [-burning_iter 20] [-rounds 5] [-shape k] [-rotate_mb 768] [-cold_cache]   (k: index, default all)
#include <algorithm>
#include <chrono>
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
  int bs, hw, c, oc, s, dst_dt;
};

static double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

int main(int argc, char **argv) {
  Flags f(argc, argv);
  const int iters = f.geti("iter", 100), burn = f.geti("burning_iter", 20), rounds = f.geti("rounds", 5), only = f.geti("shape", -1);
  const bool cold = f.getb("cold_cache", false);
  const size_t rotate_mb = (size_t)std::max(1, f.geti("rotate_mb", 768));
  const std::vector<Shape> shapes = {
      {"N128 112x112 32->64 s1 u8", 128, 112, 32, 64, 1, DFX_U8},
      {"N128 112x112->56x56 64->128 s2 u8", 128, 112, 64, 128, 2, DFX_U8},
      {"N128 56x56 128->128 s1 u8", 128, 56, 128, 128, 1, DFX_U8},
      {"N128 56x56->28x28 128->256 s2 u8", 128, 56, 128, 256, 2, DFX_U8},
      {"N128 28x28 256->256 s1 u8", 128, 28, 256, 256, 1, DFX_U8},
      {"N128 56x56 128->128 s1 s32", 128, 56, 128, 128, 1, DFX_S32},
  };
  char dev[256];
  CK(dfx_device_name(dev, sizeof(dev)));
  printf("bench_dwpw on %s: iter %d, burning_iter %d, rounds %d (median round reported)\n", dev, iters, burn, rounds);
  for (size_t si = 0; si < shapes.size(); ++si) {
    if (only >= 0 && (int)si != only) continue;
    const Shape &s = shapes[si];
    const int o = (s.hw + 2 - 3) / s.s + 1;
    const size_t src_bytes = (size_t)s.bs * s.hw * s.hw * s.c, mid_bytes = (size_t)s.bs * o * o * s.c;
    const size_t esz = (s.dst_dt == DFX_U8 || s.dst_dt == DFX_S8) ? 1 : 4, dst_bytes = (size_t)s.bs * o * o * s.oc * esz;
    Lcg g(277 + (uint32_t)si);
    const size_t set_bytes = src_bytes + mid_bytes + dst_bytes;
    const int nsets = (int)std::min<size_t>(64, std::max<size_t>(2, (rotate_mb << 20) / set_bytes + 1));
    std::vector<void *> d_src(nsets), d_mid(nsets), d_out(nsets);
    {
      std::vector<uint8_t> hsrc(src_bytes);
      for (int q = 0; q < nsets; ++q) {
        for (auto &v : hsrc) v = (uint8_t)(g.next() % 256);
        CK(dfx_mem_alloc_device(&d_src[q], src_bytes));
        CK(dfx_memcpy_h2d(d_src[q], hsrc.data(), src_bytes, nullptr));
        CK(dfx_stream_sync(nullptr));
        CK(dfx_mem_alloc_device(&d_mid[q], mid_bytes));
        CK(dfx_mem_alloc_device(&d_out[q], dst_bytes));
      }
    }
    void *d_chk[3];
    for (auto &q : d_chk) CK(dfx_mem_alloc_device(&q, dst_bytes));
    std::vector<int8_t> w((size_t)s.c * 9), w1((size_t)s.oc * s.c), w1b(w1.size());
    for (auto &v : w) v = (int8_t)((int)(g.next() % 21) - 10);
    for (auto &v : w1) v = (int8_t)((int)(g.next() % 21) - 10);
    CK(dfx_reorder_oihw_to_blocked(w1.data(), w1b.data(), s.oc, s.c, 1, 1));
    std::vector<int32_t> bias0(s.c), bias1(s.oc);
    for (auto &v : bias0) v = (int)(g.next() % 201) - 100;
    for (auto &v : bias1) v = (int)(g.next() % 201) - 100;
    const float scale0 = 1.0f / 64, scale1 = 1.0f / 512;
    // (a), (d)
    dfx_dwpw_desc pd;
    memset(&pd, 0, sizeof(pd));
    pd.bs = s.bs; pd.c = s.c; pd.ih = pd.iw = s.hw; pd.oh = pd.ow = o; pd.kh = pd.kw = 3; pd.sh = pd.sw = s.s;
    pd.pad_t = pd.pad_l = 1; pd.oc = s.oc; pd.dst_dt = s.dst_dt; pd.bia0_dt = pd.bia1_dt = DFX_S32; pd.relu = 1;
    pd.nscales0 = pd.nscales1 = 1;
    dfx_dwpw_t *fused = nullptr, *two = nullptr;
    pd.force_path = DFX_DWPW_FUSED;
    CK(dfx_dwpw_create(&pd, &fused));
    pd.force_path = DFX_DWPW_TWO_LAUNCH;
    CK(dfx_dwpw_create(&pd, &two));
    pd.force_path = -1;
    dfx_dwpw_t *aut = nullptr;
    CK(dfx_dwpw_create(&pd, &aut));
    CK(dfx_dwpw_set_weights(fused, w.data(), bias0.data(), &scale0, w1b.data(), bias1.data(), &scale1));
    CK(dfx_dwpw_set_weights(two, w.data(), bias0.data(), &scale0, w1b.data(), bias1.data(), &scale1));
    dfx_dwpw_info fi, ti, ai;
    CK(dfx_dwpw_query(fused, &fi));
    CK(dfx_dwpw_query(two, &ti));
    CK(dfx_dwpw_query(aut, &ai));
    CK(dfx_dwpw_destroy(aut));
    // (b), (c)
    dfx_dwconv_desc dd;
    memset(&dd, 0, sizeof(dd));
    dd.bs = s.bs; dd.c = s.c; dd.ih = dd.iw = s.hw; dd.oh = dd.ow = o; dd.kh = dd.kw = 3; dd.sh = dd.sw = s.s;
    dd.pad_t = dd.pad_l = 1; dd.dst_dt = DFX_U8; dd.bia_dt = DFX_S32; dd.relu = 1; dd.nscales = 1; dd.force_path = -1;
    dfx_dwconv_t *dw = nullptr;
    CK(dfx_dwconv_create(&dd, &dw));
    CK(dfx_dwconv_set_weights(dw, w.data(), bias0.data(), &scale0));
    dfx_conv_desc vd;
    memset(&vd, 0, sizeof(vd));
    vd.bs = s.bs; vd.ic = s.c; vd.oc = s.oc; vd.ih = vd.iw = vd.oh = vd.ow = o; vd.kh = vd.kw = vd.sh = vd.sw = 1;
    vd.dst_dt = s.dst_dt; vd.bia0_dt = DFX_S32; vd.conv0_relu = 1; vd.conv0_nscales = vd.conv1_nscales = 1; vd.force_variant = -1;
    dfx_conv_t *conv = nullptr;
    CK(dfx_conv_create(&vd, &conv));
    CK(dfx_conv_set_weights(conv, w1b.data(), bias1.data(), &scale1, nullptr, nullptr, nullptr));
    dfx_dwconv_info di;
    dfx_conv_info vi;
    CK(dfx_dwconv_query(dw, &di));
    CK(dfx_conv_query(conv, &vi));
    dfx_stream_t st = nullptr;
    CK(dfx_stream_create(&st));
    const int nlegs = 4;
    auto leg = [&](int which, int q, void *out) {
      switch (which) {
        case 0: CK(dfx_dwpw_submit(fused, d_src[q], out, st)); break;
        case 1:
          CK(dfx_dwconv_submit(dw, d_src[q], d_mid[q], st));
          CK(dfx_conv_submit(conv, d_mid[q], out, st));
          break;
        case 2: CK(dfx_dwconv_submit(dw, d_src[q], d_mid[q], st)); break;
        case 3: CK(dfx_dwpw_submit(two, d_src[q], out, st)); break;
      }
    };
    {  // same bytes from every leg that computes the block
      std::vector<uint8_t> r[3];
      const int legs[3] = {0, 1, 3};
      for (int i = 0; i < 3; ++i) {
        leg(legs[i], 0, d_chk[i]);
        r[i].resize(dst_bytes);
        CK(dfx_memcpy_d2h(r[i].data(), d_chk[i], dst_bytes, st));
      }
      CK(dfx_stream_sync(st));
      if (memcmp(r[0].data(), r[1].data(), dst_bytes) != 0 || memcmp(r[2].data(), r[1].data(), dst_bytes) != 0) {
        fprintf(stderr, "bench_dwpw: the op differs from dwconv + conv on %s\n", s.name);
        return 1;
      }
    }
    int turn = 0;
    for (int which = 0; which < nlegs; ++which)
      for (int i = 0; i < burn; ++i, ++turn) leg(which, turn % nsets, d_out[turn % nsets]);
    CK(dfx_stream_sync(st));
    dfx_event_t e0, e1;
    CK(dfx_event_create(&e0));
    CK(dfx_event_create(&e1));
    std::vector<double> us[4];
    for (int r = 0; r < rounds; ++r)
      for (int which = 0; which < nlegs; ++which) {
        CK(dfx_event_record(e0, st));
        for (int i = 0; i < iters; ++i, ++turn) leg(which, turn % nsets, d_out[turn % nsets]);
        CK(dfx_event_record(e1, st));
        float ms = 0;
        CK(dfx_event_elapsed_ms(e0, e1, &ms));
        us[which].push_back(1e3 * ms / iters);
      }
    const double a = median(us[0]), b = median(us[1]), c = median(us[2]), d = median(us[3]);
    auto mn = [&](int i) { return *std::min_element(us[i].begin(), us[i].end()); };
    auto mx = [&](int i) { return *std::max_element(us[i].begin(), us[i].end()); };
    printf("\n%s   (all legs byte-identical; %d buffer sets of %.1f MB in rotation)\n", s.name, nsets, set_bytes / 1e6);
    printf("  fused kernel     %s  grid %d x %d lds %d\n", fi.kernel_name, fi.grid, fi.block, fi.lds_bytes);
    printf("  two ops          %s | %s\n", di.kernel_name, vi.kernel_name);
    printf("  auto path        %s\n", ai.path == DFX_DWPW_FUSED ? "fused" : "two launches");
    printf("  (a) fused                    %8.2f us   min %.2f max %.2f\n", a, mn(0), mx(0));
    printf("  (b) dwconv + conv, two ops   %8.2f us   min %.2f max %.2f\n", b, mn(1), mx(1));
    printf("  (c) dwconv alone             %8.2f us   min %.2f max %.2f\n", c, mn(2), mx(2));
    printf("  (d) the op's two-launch path %8.2f us   min %.2f max %.2f\n", d, mn(3), mx(3));
    printf("  a/b %.3f   a/c %.3f   traffic b/a %.2f x (%.1f MB / %.1f MB)   (a) %.2f TB/s = %.2f of 8 TB/s, HBM floor %.2f us\n", a / b,
           a / c, (double)ti.algorithmic_bytes / fi.algorithmic_bytes, ti.algorithmic_bytes / 1e6, fi.algorithmic_bytes / 1e6,
           fi.algorithmic_bytes / a / 1e6, fi.algorithmic_bytes / a / 1e6 / 8.0, fi.algorithmic_bytes / 8e6);
    if (cold) {
      const size_t scratch_bytes = 512u << 20;
      void *scratch = nullptr;
      CK(dfx_mem_alloc_device(&scratch, scratch_bytes));
      auto now = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
      double sum[2] = {0, 0};
      const int n = std::min(iters, 30);
      for (int cc = 0; cc < 2; ++cc)
        for (int i = 0; i < n; ++i) {
          if (cc) CK(dfx_memset_device(scratch, i & 0xff, scratch_bytes, st));
          CK(dfx_stream_sync(st));
          const double t0 = now();
          leg(0, i % nsets, d_out[i % nsets]);
          CK(dfx_stream_sync(st));
          sum[cc] += now() - t0;
        }
      CK(dfx_mem_free_device(scratch));
      printf("  (a) one launch at a time, host clock: warm %.2f us, COLD (512 MiB scratch rewritten before each) %.2f us\n", sum[0] / n, sum[1] / n);
    }
    CK(dfx_event_destroy(e0));
    CK(dfx_event_destroy(e1));
    CK(dfx_stream_sync(st));
    CK(dfx_dwpw_destroy(fused));
    CK(dfx_dwpw_destroy(two));
    CK(dfx_dwconv_destroy(dw));
    CK(dfx_conv_destroy(conv));
    CK(dfx_stream_destroy(st));
    for (int q = 0; q < nsets; ++q) {
      CK(dfx_mem_free_device(d_src[q]));
      CK(dfx_mem_free_device(d_mid[q]));
      CK(dfx_mem_free_device(d_out[q]));
    }
    for (void *q : d_chk) CK(dfx_mem_free_device(q));
  }
  return 0;
}
