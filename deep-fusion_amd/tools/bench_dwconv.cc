// bench_dwconv -- times the depthwise conv op on MI355X through the public C ABI (include/dfx.h) against three
// yardsticks, in ONE process on the same device buffers:
//   (a) dfx_dwconv_submit
//   (b) dfx_pool_submit, max pooling with the same window, stride, padding and tensor: for u8 it moves identical bytes
//       with the same access pattern
//   (c) dfx_conv_submit of the dense conv with block-diagonal weights where c <= 128: what a caller had to do without
//       the op
//   (d) the HBM floor: algorithmic_bytes / 8 TB/s
// Protocol (bench_catconv's): every timed submit works on the next of several buffer sets (>= 768 MB in rotation, so
// that the 256 MiB Infinity Cache serves no leg); per shape `rounds` rounds; a round times each leg in turn as `iter`
// back-to-back submits between two device events on one stream, after `burning_iter` warm-up submits of every leg.
// Reported: the median round of each leg in us per submit, a / b, c / a and the HBM fraction of (a).  (a) and (c) are
// compared byte for byte first.  -cold_cache adds one-launch-at-a-time legs of (a) with warm caches and with 512 MiB of
// scratch rewritten before every launch.
//   bench_dwconv [-iter 100] [-burning_iter 20] [-rounds 5] [-shape k] [-rotate_mb 768] [-cold_cache]   (k: index, default all)
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
  int bs, hw, c, k, s, dst_dt;
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
      {"N128 112x112x32 3x3 s1 u8", 128, 112, 32, 3, 1, DFX_U8},
      {"N128 112x112x64 3x3 s2 u8", 128, 112, 64, 3, 2, DFX_U8},
      {"N128 56x56x128 3x3 s1 u8", 128, 56, 128, 3, 1, DFX_U8},
      {"N128 56x56x128 3x3 s2 u8", 128, 56, 128, 3, 2, DFX_U8},
      {"N128 28x28x256 3x3 s1 u8", 128, 28, 256, 3, 1, DFX_U8},
      {"N128 14x14x512 3x3 s1 u8", 128, 14, 512, 3, 1, DFX_U8},
      {"N128 7x7x1024 3x3 s1 u8", 128, 7, 1024, 3, 1, DFX_U8},
      {"N128 28x28x96 5x5 s1 u8", 128, 28, 96, 5, 1, DFX_U8},
      {"N128 14x14x672 5x5 s1 u8", 128, 14, 672, 5, 1, DFX_U8},
      {"N128 14x14x672 5x5 s2 u8", 128, 14, 672, 5, 2, DFX_U8},
      {"N128 56x56x128 3x3 s1 s32", 128, 56, 128, 3, 1, DFX_S32},
  };
  char dev[256];
  CK(dfx_device_name(dev, sizeof(dev)));
  printf("bench_dwconv on %s: iter %d, burning_iter %d, rounds %d (median round reported)\n", dev, iters, burn, rounds);
  for (size_t si = 0; si < shapes.size(); ++si) {
    if (only >= 0 && (int)si != only) continue;
    const Shape &s = shapes[si];
    const int p = s.k / 2, o = (s.hw + 2 * p - s.k) / s.s + 1;
    const size_t src_bytes = (size_t)s.bs * s.hw * s.hw * s.c;
    const size_t esz = (s.dst_dt == DFX_U8 || s.dst_dt == DFX_S8) ? 1 : 4, outs = (size_t)s.bs * o * o * s.c, dst_bytes = outs * esz;
    Lcg g(199 + (uint32_t)si);
    const size_t set_bytes = src_bytes + dst_bytes;
    const int nsets = (int)std::min<size_t>(64, std::max<size_t>(2, (rotate_mb << 20) / set_bytes + 1));
    std::vector<void *> d_src(nsets), d_out(nsets);
    {
      std::vector<uint8_t> hsrc(src_bytes);
      for (int q = 0; q < nsets; ++q) {
        for (auto &v : hsrc) v = (uint8_t)(g.next() % 256);
        CK(dfx_mem_alloc_device(&d_src[q], src_bytes));
        CK(dfx_memcpy_h2d(d_src[q], hsrc.data(), src_bytes, nullptr));
        CK(dfx_stream_sync(nullptr));
        CK(dfx_mem_alloc_device(&d_out[q], dst_bytes));
      }
    }
    void *d_chk[2];
    for (auto &q : d_chk) CK(dfx_mem_alloc_device(&q, dst_bytes));
    std::vector<int8_t> w((size_t)s.c * s.k * s.k);
    for (auto &v : w) v = (int8_t)((int)(g.next() % 21) - 10);
    std::vector<int32_t> bias(s.c);
    for (auto &v : bias) v = (int)(g.next() % 201) - 100;
    const float scale = 1.0f / 64;
    // (a)
    dfx_dwconv_desc dd;
    memset(&dd, 0, sizeof(dd));
    dd.bs = s.bs; dd.c = s.c; dd.ih = dd.iw = s.hw; dd.oh = dd.ow = o; dd.kh = dd.kw = s.k; dd.sh = dd.sw = s.s;
    dd.pad_t = dd.pad_l = p; dd.dst_dt = s.dst_dt; dd.bia_dt = DFX_S32; dd.relu = 1; dd.round_mode = DFX_ROUND_NEAREST;
    dd.nscales = 1; dd.force_path = -1;
    dfx_dwconv_t *dw = nullptr;
    CK(dfx_dwconv_create(&dd, &dw));
    CK(dfx_dwconv_set_weights(dw, w.data(), bias.data(), &scale));
    dfx_dwconv_info di;
    CK(dfx_dwconv_query(dw, &di));
    // (b): u8 pooling moves the u8 op's bytes; for a 4-byte dst it still reads the same source
    dfx_pool_desc pd;
    memset(&pd, 0, sizeof(pd));
    pd.bs = s.bs; pd.c = s.c; pd.ih = pd.iw = s.hw; pd.oh = pd.ow = o; pd.kh = pd.kw = s.k; pd.sh = pd.sw = s.s;
    pd.pad_t = pd.pad_l = p; pd.dt = DFX_U8; pd.algo = DFX_POOL_MAX;
    dfx_pool_t *pool = nullptr;
    CK(dfx_pool_create(&pd, &pool));
    // (c)
    dfx_conv_t *conv = nullptr;
    dfx_conv_info vi;
    memset(&vi, 0, sizeof(vi));
    if (s.c <= 128) {
      std::vector<int8_t> full((size_t)s.c * s.c * s.k * s.k, 0), blk(full.size());
      for (int ch = 0; ch < s.c; ++ch)
        memcpy(&full[((size_t)ch * s.c + ch) * s.k * s.k], &w[(size_t)ch * s.k * s.k], (size_t)s.k * s.k);
      CK(dfx_reorder_oihw_to_blocked(full.data(), blk.data(), s.c, s.c, s.k, s.k));
      dfx_conv_desc vd;
      memset(&vd, 0, sizeof(vd));
      vd.bs = s.bs; vd.ic = vd.oc = s.c; vd.ih = vd.iw = s.hw; vd.oh = vd.ow = o; vd.kh = vd.kw = s.k; vd.sh = vd.sw = s.s;
      vd.pad_t = vd.pad_l = p; vd.dst_dt = s.dst_dt; vd.bia0_dt = DFX_S32; vd.conv0_relu = 1;
      vd.conv0_nscales = vd.conv1_nscales = 1; vd.force_variant = -1;
      CK(dfx_conv_create(&vd, &conv));
      CK(dfx_conv_set_weights(conv, blk.data(), bias.data(), &scale, nullptr, nullptr, nullptr));
      CK(dfx_conv_query(conv, &vi));
    }
    dfx_stream_t st = nullptr;
    CK(dfx_stream_create(&st));
    const int nlegs = conv ? 3 : 2;
    auto leg = [&](int which, int q) {
      switch (which) {
        case 0: CK(dfx_dwconv_submit(dw, d_src[q], d_out[q], st)); break;
        case 1: CK(dfx_pool_submit(pool, d_src[q], d_out[q], st)); break;
        case 2: CK(dfx_conv_submit(conv, d_src[q], d_out[q], st)); break;
      }
    };
    if (conv) {  // same bytes from the op and from the dense conv
      CK(dfx_dwconv_submit(dw, d_src[0], d_chk[0], st));
      CK(dfx_conv_submit(conv, d_src[0], d_chk[1], st));
      std::vector<uint8_t> r0(dst_bytes), r1(dst_bytes);
      CK(dfx_memcpy_d2h(r0.data(), d_chk[0], dst_bytes, st));
      CK(dfx_memcpy_d2h(r1.data(), d_chk[1], dst_bytes, st));
      CK(dfx_stream_sync(st));
      if (memcmp(r0.data(), r1.data(), dst_bytes) != 0) {
        fprintf(stderr, "bench_dwconv: the op differs from the dense conv with diagonal weights on %s\n", s.name);
        return 1;
      }
    }
    int turn = 0;
    for (int which = 0; which < nlegs; ++which)
      for (int i = 0; i < burn; ++i) leg(which, turn++ % nsets);
    CK(dfx_stream_sync(st));
    dfx_event_t e0, e1;
    CK(dfx_event_create(&e0));
    CK(dfx_event_create(&e1));
    std::vector<double> us[3];
    for (int r = 0; r < rounds; ++r)
      for (int which = 0; which < nlegs; ++which) {
        CK(dfx_event_record(e0, st));
        for (int i = 0; i < iters; ++i) leg(which, turn++ % nsets);
        CK(dfx_event_record(e1, st));
        float ms = 0;
        CK(dfx_event_elapsed_ms(e0, e1, &ms));
        us[which].push_back(1e3 * ms / iters);
      }
    const double a = median(us[0]), b = median(us[1]), c = conv ? median(us[2]) : 0.0;
    const double floor_us = di.algorithmic_bytes / 8e6;
    printf("\n%s   (%s; %d buffer sets of %.1f MB in rotation)\n", s.name, conv ? "op byte-identical to the dense conv" : "no dense twin: c > 128",
           nsets, set_bytes / 1e6);
    printf("  kernel           %s  grid %d x %d lds %d\n", di.kernel_name, di.grid, di.block, di.lds_bytes);
    printf("  (a) dwconv                   %8.2f us   min %.2f max %.2f\n", a, *std::min_element(us[0].begin(), us[0].end()), *std::max_element(us[0].begin(), us[0].end()));
    printf("  (b) max pooling, same window %8.2f us   min %.2f max %.2f\n", b, *std::min_element(us[1].begin(), us[1].end()), *std::max_element(us[1].begin(), us[1].end()));
    if (conv) printf("  (c) dense conv, diagonal W   %8.2f us   min %.2f max %.2f   [%s]\n", c, *std::min_element(us[2].begin(), us[2].end()), *std::max_element(us[2].begin(), us[2].end()), vi.kernel_name);
    printf("  (d) HBM floor                %8.2f us   (%.1f MB algorithmic at 8 TB/s)\n", floor_us, di.algorithmic_bytes / 1e6);
    printf("  a/b %.3f", a / b);
    if (conv) printf("   c/a %.2f x", c / a);
    printf("   (a) %.2f TB/s = %.2f of 8 TB/s;  %.2f G outputs/s, %.2f us per output-per-lane-instruction at this size\n",
           di.algorithmic_bytes / a / 1e6, di.algorithmic_bytes / a / 1e6 / 8.0, outs / a / 1e3, outs / 39.3e6);
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
          leg(0, i % nsets);
          CK(dfx_stream_sync(st));
          sum[cc] += now() - t0;
        }
      CK(dfx_mem_free_device(scratch));
      printf("  (a) one launch at a time, host clock: warm %.2f us, COLD (512 MiB scratch rewritten before each) %.2f us\n", sum[0] / n, sum[1] / n);
    }
    CK(dfx_event_destroy(e0));
    CK(dfx_event_destroy(e1));
    CK(dfx_stream_sync(st));
    CK(dfx_dwconv_destroy(dw));
    CK(dfx_pool_destroy(pool));
    if (conv) CK(dfx_conv_destroy(conv));
    CK(dfx_stream_destroy(st));
    for (int q = 0; q < nsets; ++q) {
      CK(dfx_mem_free_device(d_src[q]));
      CK(dfx_mem_free_device(d_out[q]));
    }
    for (void *q : d_chk) CK(dfx_mem_free_device(q));
  }
  return 0;
}
