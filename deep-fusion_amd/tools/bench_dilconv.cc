// bench_dilconv -- times the dilated conv op on MI355X through the public C ABI (include/dfx.h) against what a caller
// had to run without it, in ONE process on the same device buffers:
//   (m) dfx_dilconv_submit on the MFMA path (force_path = DFX_DILCONV_MFMA): the leg the auto rule is decided from
//   (g) dfx_dilconv_submit on the generic path (force_path = DFX_DILCONV_GENERIC)
//   (c) the recipe without the op: dfx_conv_submit on the zero-stuffed ((k - 1) d + 1)^2 window, where dfx_conv_create
//       accepts that descriptor (window * ic <= 65025); "not expressible" otherwise
// and prints, per layer, what auto picks, the HBM floor (algorithmic_bytes at 8 TB/s) and the matrix floor
// (algorithmic_ops at the dense int8 peak, 5.033 POP/s).
// Layers, 3x3 stride 1 pad = d, u8 output, each at N = 1 and N = 16: the ASPP branches of DeepLabv3 at output stride 16
// on a ResNet-50 backbone (33x33, 2048 -> 256, d = 6 / 12 / 18) and on MobileNetV2 (33x33, 320 -> 256, d = 6 / 12 / 18),
// and a dilated ResNet's res4 (65x65, 256 -> 256, d = 2) and res5 (65x65, 512 -> 512, d = 4).
// Protocol (bench_deconv's): every timed submit works on the next of several buffer sets (>= 768 MB in rotation, so
// that the 256 MiB Infinity Cache serves no leg); per layer `rounds` rounds; a round times each leg in turn as
// back-to-back submits between two device events on one stream, after `burning_iter` warm-up submits of every leg.  A
// leg whose submit takes long runs fewer than `iter` submits per round (about 30 ms' worth; at least 3, or 1 where a
// single submit takes more than 10 ms).  Reported: the median round of each leg in us per submit and the ratios.  All
// legs are compared byte for byte first.
//   bench_dilconv [-iter 100] [-burning_iter 20] [-rounds 5] [-shape k] [-rotate_mb 768] [-bs n] [-ih n] [-ic n] [-oc n] [-ab 1]
//   (k: index, default all; -bs / -ih / -ic / -oc override the layer: a tiny smoke run; -ab 1 times leg (m) alone: the
//   A/B runs of the tuning switches DFX_DILCONV_SLAB / DFX_DILCONV_STRIPS, which need no second look at the other legs)
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
  int bs, ic, oc, ih, iw, d;  // 3x3, stride 1, pad = d
};

static double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

int main(int argc, char **argv) {
  Flags f(argc, argv);
  const int iters = f.geti("iter", 100), burn = f.geti("burning_iter", 20), rounds = f.geti("rounds", 5), only = f.geti("shape", -1);
  const int bs_override = f.geti("bs", 0), ih_override = f.geti("ih", 0), ic_override = f.geti("ic", 0), oc_override = f.geti("oc", 0);
  const bool ab = f.geti("ab", 0) != 0;
  const size_t rotate_mb = (size_t)std::max(1, f.geti("rotate_mb", 768));
  std::vector<Shape> shapes;
  for (int bs : {1, 16}) {
    for (int d : {6, 12, 18}) shapes.push_back({"ASPP ResNet-50 33x33 2048->256", bs, 2048, 256, 33, 33, d});
    for (int d : {6, 12, 18}) shapes.push_back({"ASPP MobileNetV2 33x33 320->256", bs, 320, 256, 33, 33, d});
    shapes.push_back({"Dilated ResNet res4 65x65 256->256", bs, 256, 256, 65, 65, 2});
    shapes.push_back({"Dilated ResNet res5 65x65 512->512", bs, 512, 512, 65, 65, 4});
  }
  char dev[256];
  CK(dfx_device_name(dev, sizeof(dev)));
  printf("bench_dilconv on %s: iter %d, burning_iter %d, rounds %d (median round reported)\n", dev, iters, burn, rounds);
  for (size_t si = 0; si < shapes.size(); ++si) {
    if (only >= 0 && (int)si != only) continue;
    Shape s = shapes[si];
    if (bs_override > 0) s.bs = bs_override;
    if (ih_override > 0) s.ih = s.iw = ih_override;
    if (ic_override > 0) s.ic = ic_override;
    if (oc_override > 0) s.oc = oc_override;
    const int oh = s.ih, ow = s.iw, e = 2 * s.d + 1;  // pad = d keeps the size; e: the stuffed window
    const size_t src_bytes = (size_t)s.bs * s.ih * s.iw * s.ic, dst_bytes = (size_t)s.bs * oh * ow * s.oc;
    Lcg g(1313 + (uint32_t)si);
    const size_t set_bytes = src_bytes + dst_bytes;
    const int nsets = (int)std::max<size_t>(2, (rotate_mb << 20) / set_bytes + 1);
    std::vector<void *> d_src(nsets), d_out(nsets);
    {
      std::vector<uint8_t> hsrc(src_bytes);
      for (auto &v : hsrc) v = (uint8_t)(g.next() % 256);
      for (int q = 0; q < nsets; ++q) {
        CK(dfx_mem_alloc_device(&d_src[q], src_bytes));
        CK(dfx_mem_alloc_device(&d_out[q], dst_bytes));
        CK(dfx_memcpy_h2d(d_src[q], hsrc.data(), src_bytes, nullptr));
        CK(dfx_stream_sync(nullptr));
      }
    }
    void *d_chk[3];
    for (auto &q : d_chk) CK(dfx_mem_alloc_device(&q, dst_bytes));
    std::vector<int8_t> w((size_t)s.oc * s.ic * 9);
    for (auto &v : w) v = (int8_t)((int)(g.next() % 21) - 10);
    std::vector<int32_t> bias(s.oc);
    for (auto &v : bias) v = (int)(g.next() % 201) - 100;
    const float scale = 1.0f / (16.0f * (float)(9 * s.ic / 4));
    // (m), (g), and what auto picks
    dfx_dilconv_desc dd;
    memset(&dd, 0, sizeof(dd));
    dd.bs = s.bs; dd.ic = s.ic; dd.ih = s.ih; dd.iw = s.iw; dd.oc = s.oc; dd.oh = oh; dd.ow = ow; dd.kh = dd.kw = 3;
    dd.sh = dd.sw = 1; dd.dh = dd.dw = s.d; dd.pad_t = dd.pad_l = s.d; dd.dst_dt = DFX_U8; dd.bia_dt = DFX_S32; dd.relu = 1;
    dd.round_mode = DFX_ROUND_NEAREST; dd.nscales = 1; dd.force_path = -1;
    dfx_dilconv_t *da = nullptr, *dg = nullptr, *dm = nullptr;
    CK(dfx_dilconv_create(&dd, &da));
    dd.force_path = DFX_DILCONV_GENERIC;
    CK(dfx_dilconv_create(&dd, &dg));
    dd.force_path = DFX_DILCONV_MFMA;
    if (dfx_dilconv_create(&dd, &dm) != DFX_OK) dm = nullptr;  // outside the MFMA kernel's class (an override)
    CK(dfx_dilconv_set_weights(dg, w.data(), bias.data(), &scale));
    if (dm) CK(dfx_dilconv_set_weights(dm, w.data(), bias.data(), &scale));
    dfx_dilconv_info ai, gi, mi;
    CK(dfx_dilconv_query(da, &ai));
    CK(dfx_dilconv_query(dg, &gi));
    memset(&mi, 0, sizeof(mi));
    if (dm) CK(dfx_dilconv_query(dm, &mi));
    // (c)
    dfx_conv_t *conv = nullptr;
    char cname[96] = "";
    if (!ab && (long long)e * e * s.ic <= 65025) {
      dfx_conv_desc vd;
      memset(&vd, 0, sizeof(vd));
      vd.bs = s.bs; vd.ic = s.ic; vd.oc = s.oc; vd.ih = s.ih; vd.iw = s.iw; vd.oh = oh; vd.ow = ow; vd.kh = vd.kw = e; vd.sh = vd.sw = 1;
      vd.pad_t = vd.pad_l = s.d; vd.dst_dt = DFX_U8; vd.bia0_dt = DFX_S32; vd.conv0_relu = 1;
      vd.conv0_nscales = vd.conv1_nscales = 1; vd.force_variant = -1;
      if (dfx_conv_create(&vd, &conv) == DFX_OK) {
        std::vector<int8_t> wz((size_t)s.oc * s.ic * e * e, 0), blk(wz.size());
        for (size_t oi = 0; oi < (size_t)s.oc * s.ic; ++oi)
          for (int ky = 0; ky < 3; ++ky)
            for (int kx = 0; kx < 3; ++kx) wz[(oi * e + (size_t)ky * s.d) * e + (size_t)kx * s.d] = w[oi * 9 + 3 * ky + kx];
        CK(dfx_reorder_oihw_to_blocked(wz.data(), blk.data(), s.oc, s.ic, e, e));
        CK(dfx_conv_set_weights(conv, blk.data(), bias.data(), &scale, nullptr, nullptr, nullptr));
        dfx_conv_info vi;
        CK(dfx_conv_query(conv, &vi));
        memcpy(cname, vi.kernel_name, sizeof(cname));
      } else {
        conv = nullptr;
      }
    }
    dfx_stream_t st = nullptr;
    CK(dfx_stream_create(&st));
    // legs: 0 (m), 1 (g), 2 (c)
    const bool has[3] = {dm != nullptr, !ab, conv != nullptr};
    auto leg = [&](int which, void *src, void *out) {
      if (which == 0) CK(dfx_dilconv_submit(dm, src, out, st));
      else if (which == 1) CK(dfx_dilconv_submit(dg, src, out, st));
      else CK(dfx_conv_submit(conv, src, out, st));
    };
    {  // same bytes from every leg
      std::vector<std::vector<uint8_t>> r(3, std::vector<uint8_t>(dst_bytes));
      for (int which = 0; which < 3; ++which) {
        if (!has[which]) continue;
        leg(which, d_src[0], d_chk[which]);
        CK(dfx_memcpy_d2h(r[which].data(), d_chk[which], dst_bytes, st));
      }
      CK(dfx_stream_sync(st));
      for (int which : {0, 2})
        if (has[1] && has[which] && memcmp(r[1].data(), r[which].data(), dst_bytes) != 0) {
          fprintf(stderr, "bench_dilconv: leg %d differs from the generic path on %s d %d N %d\n", which, s.name, s.d, s.bs);
          return 1;
        }
    }
    dfx_event_t e0, e1;
    CK(dfx_event_create(&e0));
    CK(dfx_event_create(&e1));
    int turn = 0, n_of[3] = {iters, iters, iters};
    for (int which = 0; which < 3; ++which) {  // one timed submit sizes the leg: about 30 ms per round
      if (!has[which]) continue;
      CK(dfx_event_record(e0, st));
      leg(which, d_src[turn % nsets], d_out[turn % nsets]);
      ++turn;
      CK(dfx_event_record(e1, st));
      float ms = 0;
      CK(dfx_event_elapsed_ms(e0, e1, &ms));
      n_of[which] = std::max(ms > 10.0f ? 1 : 3, std::min(iters, (int)(30.0f / std::max(ms, 1e-3f))));
      for (int i = 0; i < std::min(burn, n_of[which]); ++i, ++turn) leg(which, d_src[turn % nsets], d_out[turn % nsets]);
    }
    CK(dfx_stream_sync(st));
    std::vector<double> us[3];
    for (int r = 0; r < rounds; ++r)
      for (int which = 0; which < 3; ++which) {
        if (!has[which]) continue;
        CK(dfx_event_record(e0, st));
        for (int i = 0; i < n_of[which]; ++i, ++turn) leg(which, d_src[turn % nsets], d_out[turn % nsets]);
        CK(dfx_event_record(e1, st));
        float ms = 0;
        CK(dfx_event_elapsed_ms(e0, e1, &ms));
        us[which].push_back(1e3 * ms / n_of[which]);
      }
    const double m = has[0] ? median(us[0]) : 0.0, gen = has[1] ? median(us[1]) : 0.0, c = has[2] ? median(us[2]) : 0.0;
    const double floor_us = ai.algorithmic_bytes / 8e6, mfloor_us = ai.algorithmic_ops / 5.033e9;
    auto lo = [&](int i) { return *std::min_element(us[i].begin(), us[i].end()); };
    auto hi = [&](int i) { return *std::max_element(us[i].begin(), us[i].end()); };
    printf("\nN %d  %s d %d   (all legs byte-identical; %d buffer sets of %.1f MB in rotation; auto picks %s)\n", s.bs, s.name, s.d, nsets,
           set_bytes / 1e6, ai.path == DFX_DILCONV_MFMA ? "MFMA" : "generic");
    if (has[0])
      printf("  (m) dilconv, MFMA path     %12.2f us   min %.2f max %.2f   x%d   [%s  grid %d x %d lds %d]\n", m, lo(0), hi(0), n_of[0],
             mi.kernel_name, mi.grid, mi.block, mi.lds_bytes);
    else
      printf("  (m) outside the MFMA kernel's class\n");
    if (has[1]) printf("  (g) dilconv, generic path  %12.2f us   min %.2f max %.2f   x%d   [%s]\n", gen, lo(1), hi(1), n_of[1], gi.kernel_name);
    if (ab)
      printf("  (g), (c) not timed (-ab 1)\n");
    else if (has[2])
      printf("  (c) conv on %dx%d stuffed weights %8.2f us   min %.2f max %.2f   x%d   [%s]\n", e, e, c, lo(2), hi(2), n_of[2], cname);
    else
      printf("  (c) not expressible: a %dx%d window on %d channels is %lld taps, beyond 65025\n", e, e, s.ic, (long long)e * e * s.ic);
    printf("  HBM floor %.2f us (%.2f MB algorithmic at 8 TB/s)   matrix floor %.2f us (%.3f GOP at 5.033 POP/s)\n", floor_us,
           ai.algorithmic_bytes / 1e6, mfloor_us, ai.algorithmic_ops / 1e9);
    if (has[0]) {
      if (has[1]) printf("  m/g %.4f", m / gen);
      if (has[2]) printf("   m/c %.3f", m / c);
      printf("   m/HBM floor %.2f   m/matrix floor %.2f   (m) %.3f TB/s, %.1f TOP/s\n", m / floor_us, m / mfloor_us, ai.algorithmic_bytes / m / 1e6,
             ai.algorithmic_ops / m / 1e6);
    }
    CK(dfx_event_destroy(e0));
    CK(dfx_event_destroy(e1));
    CK(dfx_stream_sync(st));
    CK(dfx_dilconv_destroy(da));
    CK(dfx_dilconv_destroy(dg));
    if (dm) CK(dfx_dilconv_destroy(dm));
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
