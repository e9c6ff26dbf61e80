// bench_fc -- times the fully-connected op on MI355X through the public C ABI (include/dfx.h) against the only way to
// run the layer without it, in ONE process:
//   (a) dfx_fc_submit on auto
//   (b) dfx_fc_submit of handles created under DFX_FC_SPLITK=n, for every n of -splitk (the sweep the planner's
//       constants come from)
//   (c) dfx_conv_submit of the same layer as a conv whose window is the whole image (stride 1, no padding), where
//       dfx_conv can express it; for oc that is no multiple of 16 (the 1000-class heads) oc is padded to the next one
//       with zero weights and the line says so -- a caller would need a cropping pass on top
//   (d) the HBM floor: src + weights + dst at 8 TB/s
// Layers: the classifier heads of ResNet-50, VGG-16 (fc6, fc7, fc8) and MobileNetV2 at the batch sizes of -bs.
// Protocol (bench_gconv's): the op is bound by its WEIGHT stream, so every leg has several handles with their own copy
// of the weights and their own src / dst, and every timed submit works on the next of them (-rotate_mb in rotation, at
// most -max_sets handles, so that the 256 MiB Infinity Cache serves no leg where that many fit); per layer `rounds`
// rounds; a round times each leg in turn as `iter` back-to-back submits between two device events on one stream, after
// `burning_iter` warm-up submits of every leg.  Reported: the median round of each leg in us per submit.  (a), (b) and
// (c) are compared byte for byte first.  -cold_cache adds one-launch-at-a-time legs of (a) with warm caches and with
// 512 MiB of scratch rewritten before every launch.
//   bench_fc [-iter 50] [-burning_iter 10] [-rounds 5] [-shape k] [-bs 1,8,64,128] [-splitk 1,2,4,8,16,32] [-rotate_mb 768]
//            [-max_sets 8] [-cold_cache] [-noconv]
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
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
  int ic, ih, iw, oc;
};

static double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

struct Leg {
  std::string label;
  std::vector<dfx_fc_t *> fc;   // one handle per set (own weights), or ...
  std::vector<dfx_conv_t *> cv;  // ... the conv leg's
  std::vector<double> us;
  char kernel[96];
  int splitk, grid, block, lds;
};

int main(int argc, char **argv) {
  Flags f(argc, argv);
  const int iters = f.geti("iter", 50), burn = f.geti("burning_iter", 10), rounds = f.geti("rounds", 5), only = f.geti("shape", -1);
  const bool cold = f.getb("cold_cache", false), with_conv = f.getb("conv", true);
  const size_t rotate_mb = (size_t)std::max(1, f.geti("rotate_mb", 768));
  const int max_sets = std::max(2, f.geti("max_sets", 8));
  const std::vector<int> batches = Flags::split_ints(f.gets("bs", "1,8,64,128"));
  const std::vector<int> sweep = Flags::split_ints(f.gets("splitk", "1,2,4,8,16,32"));
  const std::vector<Shape> shapes = {
      {"ResNet-50 head 2048 -> 1000", 2048, 1, 1, 1000},
      {"VGG fc6 7x7x512 -> 4096", 512, 7, 7, 4096},
      {"VGG fc7 4096 -> 4096", 4096, 1, 1, 4096},
      {"VGG fc8 4096 -> 1000", 4096, 1, 1, 1000},
      {"MobileNetV2 head 1280 -> 1000", 1280, 1, 1, 1000},
  };
  char dev[256];
  CK(dfx_device_name(dev, sizeof(dev)));
  printf("bench_fc on %s: iter %d, burning_iter %d, rounds %d (median round reported)\n", dev, iters, burn, rounds);
  for (size_t si = 0; si < shapes.size(); ++si) {
    if (only >= 0 && (int)si != only) continue;
    const Shape &s = shapes[si];
    const int K = s.ic * s.ih * s.iw, ocp = (s.oc + 15) / 16 * 16;
    Lcg g(911 + (uint32_t)si);
    std::vector<int8_t> w((size_t)s.oc * K);
    for (auto &v : w) v = (int8_t)((int)(g.next() % 21) - 10);
    std::vector<int32_t> bias(ocp, 0);
    for (int o = 0; o < s.oc; ++o) bias[o] = (int)(g.next() % 201) - 100;
    const float scale = 1.0f / (4.0f * (float)K);
    std::vector<int8_t> wblk;  // (c): oc padded with zero rows, OIhw4i16o4i
    if (with_conv) {
      std::vector<int8_t> full((size_t)ocp * K, 0);
      memcpy(full.data(), w.data(), w.size());
      wblk.resize(full.size());
      CK(dfx_reorder_oihw_to_blocked(full.data(), wblk.data(), ocp, s.ic, s.ih, s.iw));
    }
    for (int bs : batches) {
      const size_t src_bytes = (size_t)bs * K, dst_bytes = (size_t)bs * s.oc, cdst_bytes = (size_t)bs * ocp;
      const size_t set_bytes = src_bytes + w.size() + dst_bytes;
      const int nsets = (int)std::min<size_t>((size_t)max_sets, std::max<size_t>(2, (rotate_mb << 20) / set_bytes + 1));
      std::vector<void *> d_src(nsets), d_out(nsets);
      {
        std::vector<uint8_t> hsrc(src_bytes);
        for (int q = 0; q < nsets; ++q) {
          for (auto &v : hsrc) v = (uint8_t)(g.next() % 256);
          CK(dfx_mem_alloc_device(&d_src[q], src_bytes));
          CK(dfx_memcpy_h2d(d_src[q], hsrc.data(), src_bytes, nullptr));
          CK(dfx_stream_sync(nullptr));
          CK(dfx_mem_alloc_device(&d_out[q], cdst_bytes));
        }
      }
      dfx_fc_desc fd;
      memset(&fd, 0, sizeof(fd));
      fd.bs = bs; fd.ic = s.ic; fd.ih = s.ih; fd.iw = s.iw; fd.oc = s.oc; fd.dst_dt = DFX_U8; fd.bia_dt = DFX_S32; fd.relu = 1;
      fd.round_mode = DFX_ROUND_NEAREST; fd.nscales = 1; fd.force_path = -1;
      std::vector<Leg> legs;
      auto add_fc = [&](const std::string &label, const char *splitk) {
        Leg l;
        l.label = label;
        if (splitk) CK(dfx_debug_set_tuning("DFX_FC_SPLITK", splitk));
        for (int q = 0; q < nsets; ++q) {
          dfx_fc_t *h = nullptr;
          CK(dfx_fc_create(&fd, &h));
          CK(dfx_fc_set_weights(h, w.data(), bias.data(), &scale));
          l.fc.push_back(h);
        }
        if (splitk) CK(dfx_debug_set_tuning("DFX_FC_SPLITK", nullptr));
        dfx_fc_info i;
        CK(dfx_fc_query(l.fc[0], &i));
        memcpy(l.kernel, i.kernel_name, sizeof(l.kernel));
        l.splitk = i.splitk; l.grid = i.grid; l.block = i.block; l.lds = i.lds_bytes;
        legs.push_back(l);
      };
      add_fc("(a) fc, auto", nullptr);
      dfx_fc_info ai;
      CK(dfx_fc_query(legs[0].fc[0], &ai));
      int last = -1;
      for (int n : sweep) {
        if (std::min(n, K / 64) == last) continue;  // clamped to the k-steps: the same plan again
        last = std::min(n, K / 64);
        add_fc("(b) fc, splitk " + std::to_string(last), std::to_string(n).c_str());
      }
      bool have_conv = false;
      std::string conv_note;
      if (with_conv) {
        dfx_conv_desc vd;
        memset(&vd, 0, sizeof(vd));
        vd.bs = bs; vd.ic = s.ic; vd.oc = ocp; vd.ih = s.ih; vd.iw = s.iw; vd.oh = vd.ow = 1; vd.kh = s.ih; vd.kw = s.iw; vd.sh = vd.sw = 1;
        vd.dst_dt = DFX_U8; vd.bia0_dt = DFX_S32; vd.conv0_relu = 1; vd.conv0_nscales = vd.conv1_nscales = 1; vd.force_variant = -1;
        Leg l;
        l.label = ocp == s.oc ? "(c) conv, full-image window" : "(c) conv, full-image window, oc padded to " + std::to_string(ocp);
        for (int q = 0; q < nsets; ++q) {
          dfx_conv_t *h = nullptr;
          if (dfx_conv_create(&vd, &h) != DFX_OK) {
            conv_note = dfx_last_error();
            break;
          }
          CK(dfx_conv_set_weights(h, wblk.data(), bias.data(), &scale, nullptr, nullptr, nullptr));
          l.cv.push_back(h);
        }
        if ((int)l.cv.size() == nsets) {
          dfx_conv_info vi;
          CK(dfx_conv_query(l.cv[0], &vi));
          memcpy(l.kernel, vi.kernel_name, sizeof(l.kernel));
          l.splitk = 0; l.grid = vi.grid; l.block = vi.block; l.lds = vi.lds_bytes;
          legs.push_back(l);
          have_conv = true;
        } else {
          for (dfx_conv_t *h : l.cv) CK(dfx_conv_destroy(h));
        }
      }
      dfx_stream_t st = nullptr;
      CK(dfx_stream_create(&st));
      auto submit = [&](Leg &l, int q) {
        if (!l.fc.empty()) CK(dfx_fc_submit(l.fc[q], d_src[q], d_out[q], st));
        else CK(dfx_conv_submit(l.cv[q], d_src[q], d_out[q], st));
      };
      {  // the same bytes from every leg (the conv's rows are ocp wide: compare the first oc of each)
        std::vector<uint8_t> r0(dst_bytes), r1(cdst_bytes);
        for (size_t li = 0; li < legs.size(); ++li) {
          submit(legs[li], 0);
          const bool is_conv = legs[li].fc.empty();
          CK(dfx_memcpy_d2h(li == 0 ? r0.data() : r1.data(), d_out[0], is_conv ? cdst_bytes : dst_bytes, st));
          CK(dfx_stream_sync(st));
          if (li == 0) continue;
          bool same = true;
          for (int n = 0; n < bs && same; ++n)
            same = memcmp(&r0[(size_t)n * s.oc], &r1[(size_t)n * (is_conv ? ocp : s.oc)], s.oc) == 0;
          if (!same) {
            fprintf(stderr, "bench_fc: %s differs from (a) on %s, bs %d\n", legs[li].label.c_str(), s.name, bs);
            return 1;
          }
        }
      }
      int turn = 0;
      for (Leg &l : legs)
        for (int i = 0; i < burn; ++i) submit(l, turn++ % nsets);
      CK(dfx_stream_sync(st));
      dfx_event_t e0, e1;
      CK(dfx_event_create(&e0));
      CK(dfx_event_create(&e1));
      for (int r = 0; r < rounds; ++r)
        for (Leg &l : legs) {
          CK(dfx_event_record(e0, st));
          for (int i = 0; i < iters; ++i) submit(l, turn++ % nsets);
          CK(dfx_event_record(e1, st));
          float ms = 0;
          CK(dfx_event_elapsed_ms(e0, e1, &ms));
          l.us.push_back(1e3 * ms / iters);
        }
      const double a = median(legs[0].us), floor_us = ai.algorithmic_bytes / 8e6;
      printf("\n%s, bs %d   (all legs byte-identical; %d handle / buffer sets of %.1f MB in rotation)\n", s.name, bs, nsets, set_bytes / 1e6);
      for (Leg &l : legs) {
        const double m = median(l.us);
        printf("  %-52s %9.2f us   min %.2f max %.2f   x(a) %.3f   [%s  grid %d x %d lds %d]\n", l.label.c_str(), m,
               *std::min_element(l.us.begin(), l.us.end()), *std::max_element(l.us.begin(), l.us.end()), m / a, l.kernel, l.grid, l.block, l.lds);
      }
      if (with_conv && !have_conv) printf("  (c) conv, full-image window: dfx_conv cannot express the layer (%s)\n", conv_note.c_str());
      printf("  (d) HBM floor %.2f us (%.2f MB algorithmic at 8 TB/s)   a/d %.2f   (a) weights %.3f TB/s, %.2f TOP/s\n", floor_us,
             ai.algorithmic_bytes / 1e6, a / floor_us, (double)w.size() / a / 1e6, ai.algorithmic_ops / a / 1e6);
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
            submit(legs[0], cc ? i % nsets : 0);
            CK(dfx_stream_sync(st));
            sum[cc] += now() - t0;
          }
        CK(dfx_mem_free_device(scratch));
        printf("  (a) one launch at a time, host clock: warm (one handle) %.2f us, COLD (512 MiB scratch rewritten before each) %.2f us\n",
               sum[0] / n, sum[1] / n);
      }
      CK(dfx_event_destroy(e0));
      CK(dfx_event_destroy(e1));
      CK(dfx_stream_sync(st));
      for (Leg &l : legs) {
        for (dfx_fc_t *h : l.fc) CK(dfx_fc_destroy(h));
        for (dfx_conv_t *h : l.cv) CK(dfx_conv_destroy(h));
      }
      CK(dfx_stream_destroy(st));
      for (int q = 0; q < nsets; ++q) {
        CK(dfx_mem_free_device(d_src[q]));
        CK(dfx_mem_free_device(d_out[q]));
      }
    }
  }
  return 0;
}
