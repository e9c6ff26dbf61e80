// bench_deconv -- times the transposed conv op on MI355X through the public C ABI (include/dfx.h) against what a caller
// had to run without it, in ONE process on the same device buffers:
//   (a) dfx_deconv_submit on auto
//   (b) dfx_deconv_submit on the generic path (force_path = DFX_DECONV_GENERIC)
//   (c) the recipe without the op: a stride-1 conv with flipped weights on a tensor that was zero-stuffed IN ADVANCE on
//       the host -- dfx_conv_submit where the dense conv can express the layer (symmetric padding, derived output size),
//       dfx_gconv_submit with groups = 1 otherwise.  The stuffing itself (s^2 times the bytes to write) is NOT timed,
//       which flatters this leg.
//   (m) dfx_deconv_submit on the MFMA path (force_path = DFX_DECONV_MFMA), where the shape is in its class: the leg
//       the auto rule is decided from
// and prints, per layer, the HBM floor (algorithmic_bytes of (a) at 8 TB/s) and the matrix floor (algorithmic_ops of (a)
// at the dense int8 peak, 5.033 POP/s).
// Layers: U-Net up-convs 2x2 / 2 (512 -> 256 at 56x56, 256 -> 128 at 112x112, N = 8), the Mask R-CNN mask head (2x2 / 2,
// 256 -> 256, 14x14, N = 256), pose / CenterNet heads 4x4 / 2 pad 1 (256 -> 256 at 16x12, 32x24, 64x48, N = 32), DCGAN
// 4x4 / 2 pad 1 (512 -> 256 at 8x8, 128 -> 64 at 32x32, N = 64) and a Keras-style 3x3 / 2 pad 1 output_padding 1 decoder
// layer (128 -> 64, 64x64, N = 16); u8 output.
// Protocol (bench_imgconv's): every timed submit works on the next of several buffer sets (>= 768 MB in rotation, so
// that the 256 MiB Infinity Cache serves no leg); per layer `rounds` rounds; a round times each leg in turn as
// back-to-back submits between two device events on one stream, after `burning_iter` warm-up submits of every leg.  A
// leg whose submit takes long runs fewer than `iter` submits per round (about 30 ms' worth, at least 3).  Reported: the
// median round of each leg in us per submit and the ratios.  All legs are compared byte for byte first.
//   bench_deconv [-iter 100] [-burning_iter 20] [-rounds 5] [-shape k] [-rotate_mb 768] [-bs n]   (k: index, default all)
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
  int bs, ic, oc, ih, iw, k, p, op;  // stride 2 throughout; op: output_padding
};

static double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

int main(int argc, char **argv) {
  Flags f(argc, argv);
  const int iters = f.geti("iter", 100), burn = f.geti("burning_iter", 20), rounds = f.geti("rounds", 5), only = f.geti("shape", -1);
  const int bs_override = f.geti("bs", 0);
  const size_t rotate_mb = (size_t)std::max(1, f.geti("rotate_mb", 768));
  const std::vector<Shape> shapes = {
      {"U-Net up-conv 2x2/2 512->256 56x56", 8, 512, 256, 56, 56, 2, 0, 0},
      {"U-Net up-conv 2x2/2 256->128 112x112", 8, 256, 128, 112, 112, 2, 0, 0},
      {"Mask-head 2x2/2 256->256 14x14", 256, 256, 256, 14, 14, 2, 0, 0},
      {"Pose head 4x4/2 p1 256->256 16x12", 32, 256, 256, 16, 12, 4, 1, 0},
      {"Pose head 4x4/2 p1 256->256 32x24", 32, 256, 256, 32, 24, 4, 1, 0},
      {"Pose head 4x4/2 p1 256->256 64x48", 32, 256, 256, 64, 48, 4, 1, 0},
      {"DCGAN 4x4/2 p1 512->256 8x8", 64, 512, 256, 8, 8, 4, 1, 0},
      {"DCGAN 4x4/2 p1 128->64 32x32", 64, 128, 64, 32, 32, 4, 1, 0},
      {"Keras decoder 3x3/2 p1 op1 128->64 64x64", 16, 128, 64, 64, 64, 3, 1, 1},
  };
  char dev[256];
  CK(dfx_device_name(dev, sizeof(dev)));
  printf("bench_deconv on %s: iter %d, burning_iter %d, rounds %d (median round reported)\n", dev, iters, burn, rounds);
  for (size_t si = 0; si < shapes.size(); ++si) {
    if (only >= 0 && (int)si != only) continue;
    Shape s = shapes[si];
    if (bs_override > 0) s.bs = bs_override;
    const int S = 2, oh = (s.ih - 1) * S - 2 * s.p + s.k + s.op, ow = (s.iw - 1) * S - 2 * s.p + s.k + s.op;
    const int sth = (s.ih - 1) * S + 1, stw = (s.iw - 1) * S + 1, tp = s.k - 1 - s.p;  // the stuffed tensor, the twin's padding
    const size_t src_bytes = (size_t)s.bs * s.ih * s.iw * s.ic, stuffed_bytes = (size_t)s.bs * sth * stw * s.ic;
    const size_t dst_bytes = (size_t)s.bs * oh * ow * s.oc;
    Lcg g(977 + (uint32_t)si);
    const size_t set_bytes = src_bytes + stuffed_bytes + dst_bytes;
    const int nsets = (int)std::max<size_t>(2, (rotate_mb << 20) / set_bytes + 1);
    std::vector<void *> d_src(nsets), d_stuffed(nsets), d_out(nsets);
    {
      std::vector<uint8_t> hsrc(src_bytes), hst(stuffed_bytes, 0);
      for (auto &v : hsrc) v = (uint8_t)(g.next() % 256);
      for (int n = 0; n < s.bs; ++n)
        for (int y = 0; y < s.ih; ++y)
          for (int x = 0; x < s.iw; ++x)
            memcpy(&hst[(((size_t)n * sth + (size_t)y * S) * stw + (size_t)x * S) * s.ic], &hsrc[(((size_t)n * s.ih + y) * s.iw + x) * s.ic], (size_t)s.ic);
      for (int q = 0; q < nsets; ++q) {
        CK(dfx_mem_alloc_device(&d_src[q], src_bytes));
        CK(dfx_mem_alloc_device(&d_stuffed[q], stuffed_bytes));
        CK(dfx_mem_alloc_device(&d_out[q], dst_bytes));
        CK(dfx_memcpy_h2d(d_src[q], hsrc.data(), src_bytes, nullptr));
        CK(dfx_memcpy_h2d(d_stuffed[q], hst.data(), stuffed_bytes, nullptr));
        CK(dfx_stream_sync(nullptr));
      }
    }
    void *d_chk[4];
    for (auto &q : d_chk) CK(dfx_mem_alloc_device(&q, dst_bytes));
    std::vector<int8_t> w((size_t)s.oc * s.ic * s.k * s.k), wf(w.size());
    for (auto &v : w) v = (int8_t)((int)(g.next() % 21) - 10);
    for (size_t oi = 0; oi < (size_t)s.oc * s.ic; ++oi)
      for (int t = 0; t < s.k * s.k; ++t) wf[oi * s.k * s.k + t] = w[oi * s.k * s.k + (s.k * s.k - 1 - t)];
    std::vector<int32_t> bias(s.oc);
    for (auto &v : bias) v = (int)(g.next() % 201) - 100;
    const float scale = 1.0f / (16.0f * (float)(s.k * s.k * s.ic / 4));
    // (a), (b), (m)
    dfx_deconv_desc dd;
    memset(&dd, 0, sizeof(dd));
    dd.bs = s.bs; dd.ic = s.ic; dd.ih = s.ih; dd.iw = s.iw; dd.oc = s.oc; dd.oh = oh; dd.ow = ow; dd.kh = dd.kw = s.k;
    dd.sh = dd.sw = S; dd.pad_t = dd.pad_l = s.p; dd.dst_dt = DFX_U8; dd.bia_dt = DFX_S32; dd.relu = 1;
    dd.round_mode = DFX_ROUND_NEAREST; dd.nscales = 1; dd.force_path = -1;
    dfx_deconv_t *da = nullptr, *db = nullptr, *dm = nullptr;
    CK(dfx_deconv_create(&dd, &da));
    dd.force_path = DFX_DECONV_GENERIC;
    CK(dfx_deconv_create(&dd, &db));
    dd.force_path = DFX_DECONV_MFMA;
    if (dfx_deconv_create(&dd, &dm) != DFX_OK) dm = nullptr;  // outside the MFMA kernel's class
    CK(dfx_deconv_set_weights(da, w.data(), bias.data(), &scale));
    CK(dfx_deconv_set_weights(db, w.data(), bias.data(), &scale));
    if (dm) CK(dfx_deconv_set_weights(dm, w.data(), bias.data(), &scale));
    dfx_deconv_info ai, bi, mi;
    CK(dfx_deconv_query(da, &ai));
    CK(dfx_deconv_query(db, &bi));
    memset(&mi, 0, sizeof(mi));
    if (dm) CK(dfx_deconv_query(dm, &mi));
    // (c)
    dfx_conv_t *conv = nullptr;
    dfx_gconv_t *gconv = nullptr;
    char cname[96] = "";
    if (s.op == 0) {
      std::vector<int8_t> blk(wf.size());
      CK(dfx_reorder_oihw_to_blocked(wf.data(), blk.data(), s.oc, s.ic, s.k, s.k));
      dfx_conv_desc vd;
      memset(&vd, 0, sizeof(vd));
      vd.bs = s.bs; vd.ic = s.ic; vd.oc = s.oc; vd.ih = sth; vd.iw = stw; vd.oh = oh; vd.ow = ow; vd.kh = vd.kw = s.k; vd.sh = vd.sw = 1;
      vd.pad_t = vd.pad_l = tp; vd.dst_dt = DFX_U8; vd.bia0_dt = DFX_S32; vd.conv0_relu = 1;
      vd.conv0_nscales = vd.conv1_nscales = 1; vd.force_variant = -1;
      CK(dfx_conv_create(&vd, &conv));
      CK(dfx_conv_set_weights(conv, blk.data(), bias.data(), &scale, nullptr, nullptr, nullptr));
      dfx_conv_info vi;
      CK(dfx_conv_query(conv, &vi));
      memcpy(cname, vi.kernel_name, sizeof(cname));
    } else {
      dfx_gconv_desc gd;
      memset(&gd, 0, sizeof(gd));
      gd.bs = s.bs; gd.ic = s.ic; gd.oc = s.oc; gd.ih = sth; gd.iw = stw; gd.oh = oh; gd.ow = ow; gd.groups = 1; gd.kh = gd.kw = s.k;
      gd.sh = gd.sw = 1; gd.pad_t = gd.pad_l = tp; gd.dst_dt = DFX_U8; gd.bia_dt = DFX_S32; gd.relu = 1; gd.nscales = 1; gd.force_path = -1;
      CK(dfx_gconv_create(&gd, &gconv));
      CK(dfx_gconv_set_weights(gconv, wf.data(), bias.data(), &scale));
      dfx_gconv_info gi;
      CK(dfx_gconv_query(gconv, &gi));
      memcpy(cname, gi.kernel_name, sizeof(cname));
    }
    dfx_stream_t st = nullptr;
    CK(dfx_stream_create(&st));
    const int nlegs = dm ? 4 : 3;
    auto leg = [&](int which, void *src, void *stuffed, void *out) {
      if (which == 0) CK(dfx_deconv_submit(da, src, out, st));
      else if (which == 1) CK(dfx_deconv_submit(db, src, out, st));
      else if (which == 2) {
        if (conv) CK(dfx_conv_submit(conv, stuffed, out, st));
        else CK(dfx_gconv_submit(gconv, stuffed, out, st));
      } else CK(dfx_deconv_submit(dm, src, out, st));
    };
    {  // same bytes from every leg
      std::vector<std::vector<uint8_t>> r(nlegs, std::vector<uint8_t>(dst_bytes));
      for (int which = 0; which < nlegs; ++which) {
        leg(which, d_src[0], d_stuffed[0], d_chk[which]);
        CK(dfx_memcpy_d2h(r[which].data(), d_chk[which], dst_bytes, st));
      }
      CK(dfx_stream_sync(st));
      for (int which = 1; which < nlegs; ++which)
        if (memcmp(r[0].data(), r[which].data(), dst_bytes) != 0) {
          fprintf(stderr, "bench_deconv: leg %d differs from the op on auto on %s N %d\n", which, s.name, s.bs);
          return 1;
        }
    }
    dfx_event_t e0, e1;
    CK(dfx_event_create(&e0));
    CK(dfx_event_create(&e1));
    int turn = 0, n_of[4] = {iters, iters, iters, iters};
    for (int which = 0; which < nlegs; ++which) {  // one timed submit sizes the leg: about 30 ms per round, 3 .. iters submits
      CK(dfx_event_record(e0, st));
      leg(which, d_src[turn % nsets], d_stuffed[turn % nsets], d_out[turn % nsets]);
      ++turn;
      CK(dfx_event_record(e1, st));
      float ms = 0;
      CK(dfx_event_elapsed_ms(e0, e1, &ms));
      n_of[which] = std::max(3, std::min(iters, (int)(30.0f / std::max(ms, 1e-3f))));
      for (int i = 0; i < std::min(burn, n_of[which]); ++i, ++turn) leg(which, d_src[turn % nsets], d_stuffed[turn % nsets], d_out[turn % nsets]);
    }
    CK(dfx_stream_sync(st));
    std::vector<double> us[4];
    for (int r = 0; r < rounds; ++r)
      for (int which = 0; which < nlegs; ++which) {
        CK(dfx_event_record(e0, st));
        for (int i = 0; i < n_of[which]; ++i, ++turn) leg(which, d_src[turn % nsets], d_stuffed[turn % nsets], d_out[turn % nsets]);
        CK(dfx_event_record(e1, st));
        float ms = 0;
        CK(dfx_event_elapsed_ms(e0, e1, &ms));
        us[which].push_back(1e3 * ms / n_of[which]);
      }
    const double a = median(us[0]), b = median(us[1]), c = median(us[2]), m = dm ? median(us[3]) : 0.0;
    const double floor_us = ai.algorithmic_bytes / 8e6, mfloor_us = ai.algorithmic_ops / 5.033e9;
    auto lo = [&](int i) { return *std::min_element(us[i].begin(), us[i].end()); };
    auto hi = [&](int i) { return *std::max_element(us[i].begin(), us[i].end()); };
    printf("\nN %d  %s -> %dx%d   (all legs byte-identical; %d buffer sets of %.1f MB in rotation)\n", s.bs, s.name, oh, ow, nsets, set_bytes / 1e6);
    printf("  (a) deconv, auto                  %10.2f us   min %.2f max %.2f   x%d   [%s  grid %d x %d lds %d]\n", a, lo(0), hi(0), n_of[0],
           ai.kernel_name, ai.grid, ai.block, ai.lds_bytes);
    printf("  (b) deconv, generic path          %10.2f us   min %.2f max %.2f   x%d   [%s]\n", b, lo(1), hi(1), n_of[1], bi.kernel_name);
    printf("  (c) %s on a pre-stuffed tensor  %10.2f us   min %.2f max %.2f   x%d   [%s] (stuffing not timed)\n", conv ? "conv " : "gconv", c, lo(2),
           hi(2), n_of[2], cname);
    if (dm)
      printf("  (m) deconv, MFMA path             %10.2f us   min %.2f max %.2f   x%d   [%s  grid %d x %d lds %d]\n", m, lo(3), hi(3), n_of[3],
             mi.kernel_name, mi.grid, mi.block, mi.lds_bytes);
    else
      printf("  (m) outside the MFMA kernel's class\n");
    printf("  HBM floor %.2f us (%.2f MB algorithmic at 8 TB/s)   matrix floor %.2f us (%.3f GOP at 5.033 POP/s)\n", floor_us,
           ai.algorithmic_bytes / 1e6, mfloor_us, ai.algorithmic_ops / 1e9);
    printf("  a/b %.3f   a/c %.3f   a/HBM floor %.2f   (a) %.2f TB/s, %.1f TOP/s", a / b, a / c, a / floor_us, ai.algorithmic_bytes / a / 1e6,
           ai.algorithmic_ops / a / 1e6);
    if (dm) printf("   m/b %.3f   m/c %.3f   m/HBM floor %.2f", m / b, m / c, m / floor_us);
    printf("\n");
    CK(dfx_event_destroy(e0));
    CK(dfx_event_destroy(e1));
    CK(dfx_stream_sync(st));
    CK(dfx_deconv_destroy(da));
    CK(dfx_deconv_destroy(db));
    if (dm) CK(dfx_deconv_destroy(dm));
    if (conv) CK(dfx_conv_destroy(conv));
    if (gconv) CK(dfx_gconv_destroy(gconv));
    CK(dfx_stream_destroy(st));
    for (int q = 0; q < nsets; ++q) {
      CK(dfx_mem_free_device(d_src[q]));
      CK(dfx_mem_free_device(d_stuffed[q]));
      CK(dfx_mem_free_device(d_out[q]));
    }
    for (void *q : d_chk) CK(dfx_mem_free_device(q));
  }
  return 0;
}
