// bench_patchembed -- times the int8 patch-embedding op (dfx_patchembed_*) on MI355X through the C ABI, s8 out, with a token table:
//   ViT-B/16 and ViT-L/16 at 224 and at 384, ViT-B/32 at 224 (u8 RGB), the Swin-T / ConvNeXt-T 4x4 stem (u8 RGB, oc 96), a
//   ConvNeXt 2x2 downsample 96 -> 192 (s8, 56 x 56), each at bs 1, 8 and 64
// Legs, alternating at every point, on the same commit: the tile kernel at BM 128 and at BM 64 and the generic kernel, forced;
// and two yardsticks of existing code: (a) dfx_imgconv on auto with k = s on the same image, where ic <= 4 (what a caller had
// before this op); (b) dfx_linear's tile kernel on the patch matrix gathered on the host, same rows, K and n, the gather not
// timed (what the in-kernel gather and the table cost).  Neither yardstick adds a table, so their bytes are not compared; the
// three legs of the op are compared byte for byte with one another.  Device-resident, back-to-back submits between two events;
// every window lasts at least -window_ms (the number of submits per window is set from a calibration run of each leg), the
// figure is the median of -rounds rounds, the extremes are printed.  Printed: us per submit (min .. max), TOP/s of
// algorithmic_ops and its share of the 4600 TOP/s int8 matrix peak, TB/s of algorithmic_bytes and its share of the 8 TB/s HBM
// peak.  The submits rotate over enough buffer sets to exceed -rotate_mb (default 768: three times the 256 MiB Infinity Cache).
//   bench_patchembed [-window_ms 3] [-burning_iter 5] [-rounds 5] [-rotate_mb 768] [-only <substring of a point's name>] [-nogeneric]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "cli_flags.h"
#include "dfx.h"

struct Net {
  const char *name;
  int size, patch, ic, oc, src_dt;
};
struct Leg {
  std::string name, kernel;
  std::function<void(size_t)> submit;  // on buffer set s
  std::function<void()> destroy;
  bool compare;                        // dst holds the op's bytes
  int iters;
  std::vector<double> us;
  std::vector<unsigned char> out;
};

static void check(int rc, const char *what) {
  if (rc != DFX_OK) { fprintf(stderr, "%s failed (%d): %s\n", what, rc, dfx_last_error()); exit(1); }
}

int main(int argc, char **argv) {
  Flags f(argc, argv);
  const int burn = f.geti("burning_iter", 5), rounds = f.geti("rounds", 5);
  const double window_ms = f.geti("window_ms", 3);
  const std::string only = f.gets("only", "");
  const bool with_generic = f.getb("generic", true);
  const size_t rotate = (size_t)f.geti("rotate_mb", 768) << 20;
  const Net nets[] = {{"vit-b/16 224", 224, 16, 3, 768, DFX_U8},  {"vit-l/16 224", 224, 16, 3, 1024, DFX_U8}, {"vit-b/16 384", 384, 16, 3, 768, DFX_U8},
                      {"vit-l/16 384", 384, 16, 3, 1024, DFX_U8}, {"vit-b/32 224", 224, 32, 3, 768, DFX_U8},  {"swin-t stem 224", 224, 4, 3, 96, DFX_U8},
                      {"convnext down 56", 56, 2, 96, 192, DFX_S8}};
  printf("bench_patchembed: windows of at least %.0f ms after %d warm-up submits, median of %d rounds (min .. max), legs alternating; buffers in rotation: %zu MiB%s\n",
         window_ms, burn, rounds, rotate >> 20, rotate ? "" : " (one set: warm caches)");
  printf("%-26s %-11s %9s %21s %8s %6s %7s %6s  %s\n", "point", "leg", "us", "(min .. max)", "TOP/s", "%peak", "TB/s", "%hbm", "kernel name, submits per window");
  dfx_event_t e0, e1;
  check(dfx_event_create(&e0), "event create");
  check(dfx_event_create(&e1), "event create");
  for (const Net &nt : nets)
    for (int bs : {1, 8, 64}) {
      char pname[64];
      snprintf(pname, sizeof(pname), "%s bs%d", nt.name, bs);
      if (!only.empty() && !strstr(pname, only.c_str())) continue;
      const int th = nt.size / nt.patch, k = nt.patch * nt.patch * nt.ic;
      const long long tokens = (long long)th * th, rows = bs * tokens;
      const size_t sbytes = (size_t)bs * nt.size * nt.size * nt.ic, obytes = (size_t)rows * nt.oc;
      const size_t nsets = std::max<size_t>(1, std::min<size_t>(4096, (rotate + sbytes + obytes - 1) / (sbytes + obytes)));
      auto step = [](size_t b) { return (b + 255) / 256 * 256; };
      std::vector<unsigned char> hs(sbytes), hg(sbytes);
      std::vector<int8_t> w((size_t)nt.oc * k), wl(w.size());
      Lcg g(13);
      for (size_t i = 0; i < sbytes; ++i) hs[i] = (unsigned char)(g.next() & 0xff);
      for (auto &x : w) x = (int8_t)((int)(g.next() & 0xff) - 128);
      // the patch matrix {rows, K} and the {oc, K} weights in the op's K order (ky, kx, i), for dfx_linear
      for (int b = 0; b < bs; ++b)
        for (int ty = 0; ty < th; ++ty)
          for (int tx = 0; tx < th; ++tx)
            for (int ky = 0; ky < nt.patch; ++ky)
              memcpy(&hg[(((size_t)b * tokens + ty * th + tx) * nt.patch + ky) * nt.patch * nt.ic],
                     &hs[(((size_t)b * nt.size + ty * nt.patch + ky) * nt.size + (size_t)tx * nt.patch) * nt.ic], (size_t)nt.patch * nt.ic);
      for (int o = 0; o < nt.oc; ++o)
        for (int i = 0; i < nt.ic; ++i)
          for (int ky = 0; ky < nt.patch; ++ky)
            for (int kx = 0; kx < nt.patch; ++kx)
              wl[(size_t)o * k + (size_t)(ky * nt.patch + kx) * nt.ic + i] = w[(((size_t)o * nt.ic + i) * nt.patch + ky) * nt.patch + kx];
      const double sd = (nt.src_dt == DFX_U8 ? 147.0 : 74.0) * 74.0 * std::sqrt((double)k);
      const float scale = (float)(40.0 / sd);
      std::vector<float> table((size_t)tokens * nt.oc);
      for (auto &x : table) x = (float)(((double)(g.next() % 2001) - 1000.0) * 0.001 * sd / 3.0);
      void *ds = nullptr, *dg = nullptr, *dd = nullptr;
      check(dfx_mem_alloc_device(&ds, step(sbytes) * nsets), "device alloc");
      check(dfx_mem_alloc_device(&dg, step(sbytes) * nsets), "device alloc");
      check(dfx_mem_alloc_device(&dd, step(obytes) * nsets), "device alloc");
      for (size_t s = 0; s < nsets; ++s) {
        check(dfx_memcpy_h2d((char *)ds + s * step(sbytes), hs.data(), sbytes, nullptr), "H2D");
        check(dfx_memcpy_h2d((char *)dg + s * step(sbytes), hg.data(), sbytes, nullptr), "H2D");
      }
      check(dfx_stream_sync(nullptr), "sync");
      auto src_of = [&](size_t s) { return (char *)ds + s * step(sbytes); };
      auto mat_of = [&](size_t s) { return (char *)dg + s * step(sbytes); };
      auto dst_of = [&](size_t s) { return (char *)dd + s * step(obytes); };

      std::vector<Leg> legs;
      uint64_t ops = 0, bytes = 0;
      const struct { const char *name; int path; const char *bm; } own[] = {{"tile128", DFX_PATCHEMBED_TILE, "128"}, {"tile64", DFX_PATCHEMBED_TILE, "64"},
                                                                            {"generic", DFX_PATCHEMBED_GENERIC, nullptr}};
      for (const auto &l : own) {
        if (l.path == DFX_PATCHEMBED_GENERIC && !with_generic) continue;
        dfx_patchembed_desc d;
        memset(&d, 0, sizeof(d));
        d.bs = bs; d.ih = nt.size; d.iw = nt.size; d.ic = nt.ic; d.ph = nt.patch; d.pw = nt.patch; d.th = th; d.tw = th; d.oc = nt.oc;
        d.src_dt = nt.src_dt; d.dst_dt = DFX_S8; d.bia_dt = DFX_UNDEF; d.round_mode = DFX_ROUND_NEAREST; d.nscales = 1; d.table = 1; d.tok_offset = 0;
        d.force_path = l.path; d.img_rows = tokens; d.dst_ld = nt.oc;
        dfx_patchembed_t *h = nullptr;
        check(dfx_debug_set_tuning("DFX_PATCHEMBED_BM", l.bm), "set tuning");
        check(dfx_patchembed_create(&d, &h), "patchembed create");
        check(dfx_debug_set_tuning("DFX_PATCHEMBED_BM", nullptr), "set tuning");
        check(dfx_patchembed_set_weights(h, w.data(), nullptr, &scale), "patchembed set_weights");
        check(dfx_patchembed_set_table(h, table.data(), nt.oc), "patchembed set_table");
        dfx_patchembed_info info;
        check(dfx_patchembed_query(h, &info), "patchembed query");
        ops = info.algorithmic_ops;
        bytes = info.algorithmic_bytes;
        legs.push_back(Leg{l.name, info.kernel_name, [=](size_t s) { check(dfx_patchembed_submit(h, src_of(s), dst_of(s), nullptr), "patchembed submit"); },
                           [=]() { dfx_patchembed_destroy(h); }, true, 0, {}, {}});
      }
      if (nt.ic <= 4 && nt.src_dt == DFX_U8) {  // (a) dfx_imgconv on auto, window == stride, no padding
        dfx_imgconv_desc d;
        memset(&d, 0, sizeof(d));
        d.bs = bs; d.ic = nt.ic; d.ih = nt.size; d.iw = nt.size; d.oc = nt.oc; d.oh = th; d.ow = th; d.kh = nt.patch; d.kw = nt.patch; d.sh = nt.patch; d.sw = nt.patch;
        d.dst_dt = DFX_S8; d.bia_dt = DFX_UNDEF; d.round_mode = DFX_ROUND_NEAREST; d.nscales = 1; d.force_path = -1;
        dfx_imgconv_t *h = nullptr;
        check(dfx_imgconv_create(&d, &h), "imgconv create");
        check(dfx_imgconv_set_weights(h, w.data(), nullptr, &scale), "imgconv set_weights");
        dfx_imgconv_info info;
        check(dfx_imgconv_query(h, &info), "imgconv query");
        legs.push_back(Leg{"(a)imgconv", info.kernel_name, [=](size_t s) { check(dfx_imgconv_submit(h, src_of(s), dst_of(s), nullptr), "imgconv submit"); },
                           [=]() { dfx_imgconv_destroy(h); }, false, 0, {}, {}});
      }
      {  // (b) dfx_linear's tile kernel on the gathered patch matrix
        dfx_linear_desc d;
        memset(&d, 0, sizeof(d));
        d.rows = rows; d.k = k; d.n = nt.oc; d.src_dt = nt.src_dt; d.dst_dt = DFX_S8; d.bia_dt = DFX_UNDEF; d.round_mode = DFX_ROUND_NEAREST;
        d.nscales = 1; d.lut_in_dt = DFX_UNDEF; d.force_path = DFX_LINEAR_TILE; d.src_ld = k; d.dst_ld = nt.oc;
        dfx_linear_t *h = nullptr;
        check(dfx_linear_create(&d, &h), "linear create");
        check(dfx_linear_set_weights(h, wl.data(), nullptr, &scale), "linear set_weights");
        dfx_linear_info info;
        check(dfx_linear_query(h, &info), "linear query");
        legs.push_back(Leg{"(b)linear", info.kernel_name, [=](size_t s) { check(dfx_linear_submit(h, mat_of(s), dst_of(s), nullptr), "linear submit"); },
                           [=]() { dfx_linear_destroy(h); }, false, 0, {}, {}});
      }

      size_t turn = 0;
      auto window = [&](Leg &l, int iters) {
        for (int i = 0; i < burn; ++i) l.submit(turn++ % nsets);
        check(dfx_event_record(e0, nullptr), "record");
        for (int i = 0; i < iters; ++i) l.submit(turn++ % nsets);
        check(dfx_event_record(e1, nullptr), "record");
        float ms = 0;
        check(dfx_event_elapsed_ms(e0, e1, &ms), "elapsed");
        return (double)ms;
      };
      for (Leg &l : legs) {  // calibration: submits per window for at least window_ms
        const double ms = window(l, 4) / 4;
        l.iters = (int)std::min(20000.0, std::max(4.0, std::ceil(window_ms * 1.25 / std::max(ms, 1e-4))));
      }
      for (int r = 0; r < rounds; ++r)
        for (Leg &l : legs) {
          l.us.push_back(window(l, l.iters) * 1000.0 / l.iters);
          if (r == 0 && l.compare) {
            l.out.resize(obytes);
            check(dfx_memcpy_d2h(l.out.data(), dst_of((turn - 1) % nsets), obytes, nullptr), "D2H");
            check(dfx_stream_sync(nullptr), "sync");
          }
        }
      for (Leg &l : legs) {
        std::sort(l.us.begin(), l.us.end());
        const double med = l.us[l.us.size() / 2], tops = (double)ops / med / 1e6, tbs = (double)bytes / med / 1e6;
        printf("%-26s %-11s %9.2f (%8.2f .. %8.2f) %8.1f %6.2f %7.3f %6.2f  %s, %d submits\n", pname, l.name.c_str(), med, l.us.front(), l.us.back(), tops,
               100.0 * tops / 4600.0, tbs, 100.0 * tbs / 8.0, l.kernel.c_str(), l.iters);
      }
      fflush(stdout);
      for (Leg &l : legs)
        if (l.compare && l.out != legs[0].out) { fprintf(stderr, "leg %s disagrees with leg %s on %s\n", l.name.c_str(), legs[0].name.c_str(), pname); return 1; }
      for (Leg &l : legs) l.destroy();
      dfx_mem_free_device(ds);
      dfx_mem_free_device(dg);
      dfx_mem_free_device(dd);
    }
  dfx_event_destroy(e0);
  dfx_event_destroy(e1);
  return 0;
}
