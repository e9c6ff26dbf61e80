// bench_imgconv -- times the first-layer conv op on MI355X through the public C ABI (include/dfx.h) against what a caller
// had to run without it, in ONE process on the same device buffers:
//   (a) dfx_imgconv_submit on auto
//   (b) dfx_imgconv_submit on the generic path (force_path = DFX_IMGCONV_GENERIC)
//   (c) the recipe without the op: dfx_reorder_submit 3 -> 16 channels, then dfx_conv_submit on the padded tensor (two
//       launches)
//   (d) dfx_conv_submit alone on a tensor that is already padded
// and prints, per shape, the HBM floor (algorithmic_bytes of (a) at 8 TB/s) and the matrix floor (algorithmic_ops of (a)
// at the dense int8 peak, 5.033 POP/s).
// Shapes: ResNet-50 conv1 (224^2, 7x7 / 2 -> 64), VGG-16 conv1_1 (224^2, 3x3 / 1 -> 64), MobileNetV2 conv1 (224^2,
// 3x3 / 2 -> 32) and Inception-v3 conv1 (299^2, 3x3 / 2 pad 0 -> 32), each at N = 1, 32 and 128, u8 output.
// Protocol (bench_gconv's): every timed submit works on the next of several buffer sets (>= 768 MB in rotation, so that
// the 256 MiB Infinity Cache serves no leg); per shape `rounds` rounds; a round times each leg in turn as `iter`
// back-to-back submits between two device events on one stream, after `burning_iter` warm-up submits of every leg.
// Reported: the median round of each leg in us per submit and the ratios.  (a), (b) and (c) are compared byte for byte
// first.  -cold_cache adds one-launch-at-a-time legs of (a) with warm caches and with 512 MiB of scratch rewritten
// before every launch.
//   bench_imgconv [-iter 100] [-burning_iter 20] [-rounds 5] [-shape k] [-rotate_mb 768] [-cold_cache]   (k: index, default all)
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
  int bs, hw, k, s, p, oc;
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
  std::vector<Shape> shapes;
  for (int n : {1, 32, 128}) {
    shapes.push_back({"ResNet-50 conv1 224x224x3 7x7/2 -> 64", n, 224, 7, 2, 3, 64});
    shapes.push_back({"VGG-16 conv1_1 224x224x3 3x3/1 -> 64", n, 224, 3, 1, 1, 64});
    shapes.push_back({"MobileNetV2 conv1 224x224x3 3x3/2 -> 32", n, 224, 3, 2, 1, 32});
    shapes.push_back({"Inception-v3 conv1 299x299x3 3x3/2 p0 -> 32", n, 299, 3, 2, 0, 32});
  }
  char dev[256];
  CK(dfx_device_name(dev, sizeof(dev)));
  printf("bench_imgconv on %s: iter %d, burning_iter %d, rounds %d (median round reported)\n", dev, iters, burn, rounds);
  for (size_t si = 0; si < shapes.size(); ++si) {
    if (only >= 0 && (int)si != only) continue;
    const Shape &s = shapes[si];
    const int ic = 3, o = (s.hw + 2 * s.p - s.k) / s.s + 1;
    const size_t px = (size_t)s.bs * s.hw * s.hw;
    const size_t src_bytes = px * ic, pad_bytes = px * 16, dst_bytes = (size_t)s.bs * o * o * s.oc;
    Lcg g(577 + (uint32_t)si);
    const size_t set_bytes = src_bytes + pad_bytes + dst_bytes;
    const int nsets = (int)std::max<size_t>(2, (rotate_mb << 20) / set_bytes + 1);
    std::vector<void *> d_src(nsets), d_pad(nsets), d_out(nsets);
    {
      std::vector<uint8_t> hsrc(src_bytes);
      for (auto &v : hsrc) v = (uint8_t)(g.next() % 256);
      for (int q = 0; q < nsets; ++q) {
        CK(dfx_mem_alloc_device(&d_src[q], src_bytes));
        CK(dfx_memcpy_h2d(d_src[q], hsrc.data(), src_bytes, nullptr));
        CK(dfx_stream_sync(nullptr));
        CK(dfx_mem_alloc_device(&d_pad[q], pad_bytes));
        CK(dfx_mem_alloc_device(&d_out[q], dst_bytes));
      }
    }
    void *d_chk[3];
    for (auto &q : d_chk) CK(dfx_mem_alloc_device(&q, dst_bytes));
    std::vector<int8_t> w((size_t)s.oc * ic * s.k * s.k);
    for (auto &v : w) v = (int8_t)((int)(g.next() % 21) - 10);
    std::vector<int32_t> bias(s.oc);
    for (auto &v : bias) v = (int)(g.next() % 201) - 100;
    const float scale = 1.0f / (16.0f * (float)(s.k * ic));
    // (a), (b)
    dfx_imgconv_desc id;
    memset(&id, 0, sizeof(id));
    id.bs = s.bs; id.ic = ic; id.ih = id.iw = s.hw; id.oc = s.oc; id.oh = id.ow = o; id.kh = id.kw = s.k;
    id.sh = id.sw = s.s; id.pad_t = id.pad_l = s.p; id.dst_dt = DFX_U8; id.bia_dt = DFX_S32; id.relu = 1;
    id.round_mode = DFX_ROUND_NEAREST; id.nscales = 1; id.force_path = -1;
    dfx_imgconv_t *ia = nullptr, *ib = nullptr;
    CK(dfx_imgconv_create(&id, &ia));
    id.force_path = DFX_IMGCONV_GENERIC;
    CK(dfx_imgconv_create(&id, &ib));
    CK(dfx_imgconv_set_weights(ia, w.data(), bias.data(), &scale));
    CK(dfx_imgconv_set_weights(ib, w.data(), bias.data(), &scale));
    dfx_imgconv_info ai, bi;
    CK(dfx_imgconv_query(ia, &ai));
    CK(dfx_imgconv_query(ib, &bi));
    // (c), (d)
    dfx_reorder_t *ro = nullptr;
    dfx_conv_t *conv = nullptr;
    dfx_conv_info vi;
    dfx_reorder_info ri;
    {
      dfx_reorder_desc rd;
      memset(&rd, 0, sizeof(rd));
      rd.bs = s.bs; rd.h = rd.w = s.hw; rd.src_c = ic; rd.dst_c = 16; rd.src_fmt = rd.dst_fmt = DFX_FMT_NHWC;
      rd.src_dt = rd.dst_dt = DFX_U8; rd.round_mode = DFX_ROUND_NEAREST; rd.n_scales = 0;
      CK(dfx_reorder_create(&rd, nullptr, &ro));
      CK(dfx_reorder_query(ro, &ri));
      std::vector<int8_t> full((size_t)s.oc * 16 * s.k * s.k, 0), blk(full.size());
      for (int ch = 0; ch < s.oc; ++ch)  // W[o][i] = w[o][i] for i < ic, 0 on the padding channels
        memcpy(&full[(size_t)ch * 16 * s.k * s.k], &w[(size_t)ch * ic * s.k * s.k], (size_t)ic * s.k * s.k);
      CK(dfx_reorder_oihw_to_blocked(full.data(), blk.data(), s.oc, 16, s.k, s.k));
      dfx_conv_desc vd;
      memset(&vd, 0, sizeof(vd));
      vd.bs = s.bs; vd.ic = 16; vd.oc = s.oc; vd.ih = vd.iw = s.hw; vd.oh = vd.ow = o; vd.kh = vd.kw = s.k; vd.sh = vd.sw = s.s;
      vd.pad_t = vd.pad_l = s.p; vd.dst_dt = DFX_U8; vd.bia0_dt = DFX_S32; vd.conv0_relu = 1;
      vd.conv0_nscales = vd.conv1_nscales = 1; vd.force_variant = -1;
      CK(dfx_conv_create(&vd, &conv));
      CK(dfx_conv_set_weights(conv, blk.data(), bias.data(), &scale, nullptr, nullptr, nullptr));
      CK(dfx_conv_query(conv, &vi));
    }
    dfx_stream_t st = nullptr;
    CK(dfx_stream_create(&st));
    for (int q = 0; q < nsets; ++q) CK(dfx_reorder_submit(ro, d_src[q], d_pad[q], st));  // (d)'s input
    const int nlegs = 4;
    auto leg = [&](int which, int q) {
      if (which == 0) CK(dfx_imgconv_submit(ia, d_src[q], d_out[q], st));
      else if (which == 1) CK(dfx_imgconv_submit(ib, d_src[q], d_out[q], st));
      else if (which == 2) {
        CK(dfx_reorder_submit(ro, d_src[q], d_pad[q], st));
        CK(dfx_conv_submit(conv, d_pad[q], d_out[q], st));
      } else CK(dfx_conv_submit(conv, d_pad[q], d_out[q], st));
    };
    {  // same bytes from the op, from its generic path and from the recipe
      CK(dfx_imgconv_submit(ia, d_src[0], d_chk[0], st));
      CK(dfx_imgconv_submit(ib, d_src[0], d_chk[1], st));
      CK(dfx_conv_submit(conv, d_pad[0], d_chk[2], st));
      std::vector<uint8_t> r0(dst_bytes), r1(dst_bytes), r2(dst_bytes);
      CK(dfx_memcpy_d2h(r0.data(), d_chk[0], dst_bytes, st));
      CK(dfx_memcpy_d2h(r1.data(), d_chk[1], dst_bytes, st));
      CK(dfx_memcpy_d2h(r2.data(), d_chk[2], dst_bytes, st));
      CK(dfx_stream_sync(st));
      if (memcmp(r0.data(), r1.data(), dst_bytes) != 0 || memcmp(r0.data(), r2.data(), dst_bytes) != 0) {
        fprintf(stderr, "bench_imgconv: the op, its generic path and reorder + conv differ on %s N %d\n", s.name, s.bs);
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
    std::vector<double> us[4];
    for (int r = 0; r < rounds; ++r)
      for (int which = 0; which < nlegs; ++which) {
        CK(dfx_event_record(e0, st));
        for (int i = 0; i < iters; ++i) leg(which, turn++ % nsets);
        CK(dfx_event_record(e1, st));
        float ms = 0;
        CK(dfx_event_elapsed_ms(e0, e1, &ms));
        us[which].push_back(1e3 * ms / iters);
      }
    const double a = median(us[0]), b = median(us[1]), c = median(us[2]), d = median(us[3]);
    const double floor_us = ai.algorithmic_bytes / 8e6, mfloor_us = ai.algorithmic_ops / 5.033e9;
    auto lo = [&](int i) { return *std::min_element(us[i].begin(), us[i].end()); };
    auto hi = [&](int i) { return *std::max_element(us[i].begin(), us[i].end()); };
    printf("\nN %d  %s   (op, generic path and reorder + conv byte-identical; %d buffer sets of %.1f MB in rotation)\n", s.bs, s.name, nsets,
           set_bytes / 1e6);
    printf("  (a) imgconv, auto            %9.2f us   min %.2f max %.2f   [%s  grid %d x %d lds %d]\n", a, lo(0), hi(0), ai.kernel_name,
           ai.grid, ai.block, ai.lds_bytes);
    printf("  (b) imgconv, generic path    %9.2f us   min %.2f max %.2f   [%s]\n", b, lo(1), hi(1), bi.kernel_name);
    printf("  (c) reorder 3->16 + conv     %9.2f us   min %.2f max %.2f   [%s ; %s]\n", c, lo(2), hi(2), ri.kernel_name, vi.kernel_name);
    printf("  (d) conv on a padded tensor  %9.2f us   min %.2f max %.2f\n", d, lo(3), hi(3));
    printf("  HBM floor %.2f us (%.2f MB algorithmic at 8 TB/s)   matrix floor %.2f us (%.3f GOP at 5.033 POP/s)\n", floor_us,
           ai.algorithmic_bytes / 1e6, mfloor_us, ai.algorithmic_ops / 1e9);
    printf("  a/b %.3f   a/c %.3f   a/d %.3f   a/HBM floor %.2f   (a) %.2f TB/s, %.1f TOP/s\n", a / b, a / c, a / d, a / floor_us,
           ai.algorithmic_bytes / a / 1e6, ai.algorithmic_ops / a / 1e6);
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
    CK(dfx_imgconv_destroy(ia));
    CK(dfx_imgconv_destroy(ib));
    CK(dfx_reorder_destroy(ro));
    CK(dfx_conv_destroy(conv));
    CK(dfx_stream_destroy(st));
    for (int q = 0; q < nsets; ++q) {
      CK(dfx_mem_free_device(d_src[q]));
      CK(dfx_mem_free_device(d_pad[q]));
      CK(dfx_mem_free_device(d_out[q]));
    }
    for (void *q : d_chk) CK(dfx_mem_free_device(q));
  }
  return 0;
}
