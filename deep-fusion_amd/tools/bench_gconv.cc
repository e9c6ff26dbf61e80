// bench_gconv -- times the grouped conv op on MI355X through the public C ABI (include/dfx.h) against what a caller had
// to run without it, in ONE process on the same device buffers:
//   (a) dfx_gconv_submit
//   (b) dfx_conv_submit of the dense conv on block-diagonal weights (groups x the MACs and the weight bytes)
//   (c) the HBM floor: src + dst + weights of (a) at 8 TB/s
//   (t) dfx_gconv_submit of a handle created under DFX_GCONV_TILE=1: the same kernel with its input staged as a halo
//       tile in LDS instead of loaded per tap from global memory (the A/B of DESIGN 4.9)
// Shapes: the 3x3 layers of ResNeXt-50 32x4d at N = 64 with u8 output, its three stride-2 transitions, and the cpg-64
// layer of ResNeXt-101 32x8d's last stage.
// Protocol (bench_dwconv's): every timed submit works on the next of several buffer sets (>= 768 MB in rotation, so
// that the 256 MiB Infinity Cache serves no leg); per shape `rounds` rounds; a round times each leg in turn as `iter`
// back-to-back submits between two device events on one stream, after `burning_iter` warm-up submits of every leg.
// Reported: the median round of each leg in us per submit, a/b and a/c.  (a) and (b) are compared byte for byte first.
// -cold_cache adds one-launch-at-a-time legs of (a) with warm caches and with 512 MiB of scratch rewritten before every
// launch.
//   bench_gconv [-iter 100] [-burning_iter 20] [-rounds 5] [-shape k] [-rotate_mb 768] [-cold_cache]   (k: index, default all)
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
  int bs, hw, c, cpg, s;
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
      {"N64 56x56x128 cpg4 s1", 64, 56, 128, 4, 1},
      {"N64 28x28x256 cpg8 s1", 64, 28, 256, 8, 1},
      {"N64 14x14x512 cpg16 s1", 64, 14, 512, 16, 1},
      {"N64 7x7x1024 cpg32 s1", 64, 7, 1024, 32, 1},
      {"N64 56x56x256 cpg8 s2", 64, 56, 256, 8, 2},
      {"N64 28x28x512 cpg16 s2", 64, 28, 512, 16, 2},
      {"N64 14x14x1024 cpg32 s2", 64, 14, 1024, 32, 2},
      {"N64 7x7x2048 cpg64 s1 (32x8d)", 64, 7, 2048, 64, 1},
  };
  char dev[256];
  CK(dfx_device_name(dev, sizeof(dev)));
  printf("bench_gconv on %s: iter %d, burning_iter %d, rounds %d (median round reported)\n", dev, iters, burn, rounds);
  for (size_t si = 0; si < shapes.size(); ++si) {
    if (only >= 0 && (int)si != only) continue;
    const Shape &s = shapes[si];
    const int k = 3, p = 1, o = (s.hw + 2 * p - k) / s.s + 1, groups = s.c / s.cpg;
    const size_t src_bytes = (size_t)s.bs * s.hw * s.hw * s.c, dst_bytes = (size_t)s.bs * o * o * s.c;
    Lcg g(299 + (uint32_t)si);
    const size_t set_bytes = src_bytes + dst_bytes;
    const int nsets = (int)std::max<size_t>(2, (rotate_mb << 20) / set_bytes + 1);
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
    std::vector<int8_t> w((size_t)s.c * s.cpg * k * k);
    for (auto &v : w) v = (int8_t)((int)(g.next() % 21) - 10);
    std::vector<int32_t> bias(s.c);
    for (auto &v : bias) v = (int)(g.next() % 201) - 100;
    const float scale = 1.0f / (16.0f * (float)s.cpg);
    // (a)
    dfx_gconv_desc gd;
    memset(&gd, 0, sizeof(gd));
    gd.bs = s.bs; gd.ic = gd.oc = s.c; gd.ih = gd.iw = s.hw; gd.oh = gd.ow = o; gd.groups = groups; gd.kh = gd.kw = k;
    gd.sh = gd.sw = s.s; gd.pad_t = gd.pad_l = p; gd.dst_dt = DFX_U8; gd.bia_dt = DFX_S32; gd.relu = 1;
    gd.round_mode = DFX_ROUND_NEAREST; gd.nscales = 1; gd.force_path = -1;
    dfx_gconv_t *gc = nullptr;
    CK(dfx_gconv_create(&gd, &gc));
    CK(dfx_gconv_set_weights(gc, w.data(), bias.data(), &scale));
    dfx_gconv_info gi;
    CK(dfx_gconv_query(gc, &gi));
    // (t)
    dfx_gconv_t *gt = nullptr;
    dfx_gconv_info ti;
    CK(dfx_debug_set_tuning("DFX_GCONV_TILE", "1"));
    CK(dfx_gconv_create(&gd, &gt));
    CK(dfx_debug_set_tuning("DFX_GCONV_TILE", nullptr));
    CK(dfx_gconv_set_weights(gt, w.data(), bias.data(), &scale));
    CK(dfx_gconv_query(gt, &ti));
    // (b)
    dfx_conv_t *conv = nullptr;
    dfx_conv_info vi;
    memset(&vi, 0, sizeof(vi));
    {
      std::vector<int8_t> full((size_t)s.c * s.c * k * k, 0), blk(full.size());
      for (int ch = 0; ch < s.c; ++ch)  // W[o][g(o) * cpg + i] = w[o][i]
        memcpy(&full[((size_t)ch * s.c + (size_t)(ch / s.cpg) * s.cpg) * k * k], &w[(size_t)ch * s.cpg * k * k], (size_t)s.cpg * k * k);
      CK(dfx_reorder_oihw_to_blocked(full.data(), blk.data(), s.c, s.c, k, k));
      dfx_conv_desc vd;
      memset(&vd, 0, sizeof(vd));
      vd.bs = s.bs; vd.ic = vd.oc = s.c; vd.ih = vd.iw = s.hw; vd.oh = vd.ow = o; vd.kh = vd.kw = k; vd.sh = vd.sw = s.s;
      vd.pad_t = vd.pad_l = p; vd.dst_dt = DFX_U8; vd.bia0_dt = DFX_S32; vd.conv0_relu = 1;
      vd.conv0_nscales = vd.conv1_nscales = 1; vd.force_variant = -1;
      CK(dfx_conv_create(&vd, &conv));
      CK(dfx_conv_set_weights(conv, blk.data(), bias.data(), &scale, nullptr, nullptr, nullptr));
      CK(dfx_conv_query(conv, &vi));
    }
    dfx_stream_t st = nullptr;
    CK(dfx_stream_create(&st));
    const int nlegs = 3;
    auto leg = [&](int which, int q) {
      if (which == 0) CK(dfx_gconv_submit(gc, d_src[q], d_out[q], st));
      else if (which == 1) CK(dfx_conv_submit(conv, d_src[q], d_out[q], st));
      else CK(dfx_gconv_submit(gt, d_src[q], d_out[q], st));
    };
    {  // same bytes from the op and from the dense conv
      CK(dfx_gconv_submit(gc, d_src[0], d_chk[0], st));
      CK(dfx_conv_submit(conv, d_src[0], d_chk[1], st));
      std::vector<uint8_t> r0(dst_bytes), r1(dst_bytes);
      CK(dfx_memcpy_d2h(r0.data(), d_chk[0], dst_bytes, st));
      CK(dfx_memcpy_d2h(r1.data(), d_chk[1], dst_bytes, st));
      CK(dfx_stream_sync(st));
      if (memcmp(r0.data(), r1.data(), dst_bytes) != 0) {
        fprintf(stderr, "bench_gconv: the op differs from the dense conv with block-diagonal weights on %s\n", s.name);
        return 1;
      }
      CK(dfx_gconv_submit(gt, d_src[0], d_chk[1], st));
      CK(dfx_memcpy_d2h(r1.data(), d_chk[1], dst_bytes, st));
      CK(dfx_stream_sync(st));
      if (memcmp(r0.data(), r1.data(), dst_bytes) != 0) {
        fprintf(stderr, "bench_gconv: the LDS-tile variant differs from the op on %s\n", s.name);
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
    const double a = median(us[0]), b = median(us[1]), t = median(us[2]);
    const double floor_us = gi.algorithmic_bytes / 8e6;
    printf("\n%s   (op and its LDS-tile variant byte-identical to the dense conv; %d buffer sets of %.1f MB in rotation)\n", s.name, nsets, set_bytes / 1e6);
    printf("  kernel           %s  grid %d x %d lds %d\n", gi.kernel_name, gi.grid, gi.block, gi.lds_bytes);
    printf("  (a) gconv                    %8.2f us   min %.2f max %.2f\n", a, *std::min_element(us[0].begin(), us[0].end()), *std::max_element(us[0].begin(), us[0].end()));
    printf("  (b) dense conv, block-diag W %8.2f us   min %.2f max %.2f   [%s]\n", b, *std::min_element(us[1].begin(), us[1].end()), *std::max_element(us[1].begin(), us[1].end()), vi.kernel_name);
    printf("  (c) HBM floor                %8.2f us   (%.1f MB algorithmic at 8 TB/s)\n", floor_us, gi.algorithmic_bytes / 1e6);
    printf("  a/b %.3f   a/c %.2f   (a) %.2f TB/s = %.2f of 8 TB/s, %.1f TOP/s of the groups' own MACs\n", a / b, a / floor_us,
           gi.algorithmic_bytes / a / 1e6, gi.algorithmic_bytes / a / 1e6 / 8.0, gi.algorithmic_ops / a / 1e6);
    printf("  (t) gconv, input via LDS tile %7.2f us   min %.2f max %.2f   [%s  grid %d x %d lds %d]   t/a %.3f\n", t,
           *std::min_element(us[2].begin(), us[2].end()), *std::max_element(us[2].begin(), us[2].end()), ti.kernel_name, ti.grid, ti.block,
           ti.lds_bytes, t / a);
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
    CK(dfx_gconv_destroy(gc));
    CK(dfx_gconv_destroy(gt));
    CK(dfx_conv_destroy(conv));
    CK(dfx_stream_destroy(st));
    for (int q = 0; q < nsets; ++q) {
      CK(dfx_mem_free_device(d_src[q]));
      CK(dfx_mem_free_device(d_out[q]));
    }
    for (void *q : d_chk) CK(dfx_mem_free_device(q));
  }
  return 0;
}
