// bench_linear -- times the int8 token linear op (dfx_linear_*) on MI355X through the C ABI, s8 in and out:
//   ViT-B           rows 1576 (bs 8) and 12608 (bs 64): 768->2304 (QKV), 768->768 (proj), 768->3072 + table (fc1), 3072->768 (fc2)
//   Swin stage 1    rows 9408: 96->288, 96->384 + table, 384->96
//   DETR encoder    rows 1700: 256->256, 256->2048, 2048->256
// Legs, alternating at every point, on the same commit and operands: the tile kernel at BM 128 and at BM 64 and the generic
// kernel, forced; dfx_bmm's MFMA kernel with the weights as a device B and no bias (the yardstick of the auto rule); dfx_fc
// and the 1x1 dfx_conv on a u8 copy of src where their shapes allow (no table: their result is not compared).  Device-resident,
// back-to-back submits between two events; every window lasts at least -window_ms (the number of submits per window is set
// from a calibration run of each leg), the figure is the median of -rounds rounds, the extremes are printed.  Printed: us
// per submit (min .. max), TOP/s of algorithmic_ops and its share of the 4600 TOP/s int8 matrix peak, TB/s of
// algorithmic_bytes.  The submits rotate over enough buffer sets to exceed -rotate_mb (default 768: three times the 256 MiB
// Infinity Cache); -rotate_mb 0 times one set over and over (warm caches).  The three linear legs are compared byte for byte
// with one another, and with the bmm leg where the point has no bias and no table.
//   bench_linear [-window_ms 3] [-burning_iter 5] [-rounds 5] [-rotate_mb 768] [-only <substring of a point's name>] [-nogeneric]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "cli_flags.h"
#include "dfx.h"

struct Point {
  std::string name;
  long long rows;
  int k, n;
  bool table;
};
struct Leg {
  std::string name, kernel;
  std::function<void(size_t)> submit;  // on buffer set s
  std::function<void()> destroy;
  bool compare;                        // dst holds the linear op's bytes
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
  const Point points[] = {
      {"vit-b bs8 1576 768->2304", 1576, 768, 2304, false},   {"vit-b bs8 1576 768->768", 1576, 768, 768, false},
      {"vit-b bs8 1576 768->3072 +lut", 1576, 768, 3072, true}, {"vit-b bs8 1576 3072->768", 1576, 3072, 768, false},
      {"vit-b bs64 12608 768->2304", 12608, 768, 2304, false}, {"vit-b bs64 12608 768->768", 12608, 768, 768, false},
      {"vit-b bs64 12608 768->3072 +lut", 12608, 768, 3072, true}, {"vit-b bs64 12608 3072->768", 12608, 3072, 768, false},
      {"swin s1 9408 96->288", 9408, 96, 288, false},        {"swin s1 9408 96->384 +lut", 9408, 96, 384, true},
      {"swin s1 9408 384->96", 9408, 384, 96, false},        {"detr 1700 256->256", 1700, 256, 256, false},
      {"detr 1700 256->2048", 1700, 256, 2048, false},       {"detr 1700 2048->256", 1700, 2048, 256, false}};
  printf("bench_linear: windows of at least %.0f ms after %d warm-up submits, median of %d rounds (min .. max), legs alternating; buffers in rotation: %zu MiB%s\n",
         window_ms, burn, rounds, rotate >> 20, rotate ? "" : " (one set: warm caches)");
  printf("%-34s %-9s %9s %19s %8s %6s %7s  %s\n", "point", "leg", "us", "(min .. max)", "TOP/s", "%peak", "TB/s", "kernel name, submits per window");
  dfx_event_t e0, e1;
  check(dfx_event_create(&e0), "event create");
  check(dfx_event_create(&e1), "event create");
  for (const Point &p : points) {
    if (!only.empty() && !strstr(p.name.c_str(), only.c_str())) continue;
    const size_t sbytes = (size_t)p.rows * p.k, obytes = (size_t)p.rows * p.n;
    const size_t nsets = std::max<size_t>(1, std::min<size_t>(4096, (rotate + sbytes + obytes - 1) / (sbytes + obytes)));
    auto step = [](size_t b) { return (b + 255) / 256 * 256; };
    std::vector<unsigned char> hs(sbytes), hu(sbytes);
    std::vector<int8_t> w((size_t)p.n * p.k);
    Lcg g(11);
    for (size_t i = 0; i < sbytes; ++i) {
      hs[i] = (unsigned char)(g.next() & 0xff);
      hu[i] = hs[i] ^ 0x80;  // the u8 copy: value + 128
    }
    for (auto &x : w) x = (int8_t)((int)(g.next() & 0xff) - 128);
    const float scale = (float)(40.0 / (74.0 * 74.0 * std::sqrt((double)p.k)));
    std::vector<uint8_t> lut(256);
    for (int i = 0; i < 256; ++i) lut[i] = (uint8_t)(i * 7 + 3);
    void *ds = nullptr, *du = nullptr, *dd = nullptr, *dw = nullptr;
    check(dfx_mem_alloc_device(&ds, step(sbytes) * nsets), "device alloc");
    check(dfx_mem_alloc_device(&du, step(sbytes) * nsets), "device alloc");
    check(dfx_mem_alloc_device(&dd, step(obytes) * nsets), "device alloc");
    check(dfx_mem_alloc_device(&dw, w.size()), "device alloc");
    for (size_t s = 0; s < nsets; ++s) {
      check(dfx_memcpy_h2d((char *)ds + s * step(sbytes), hs.data(), sbytes, nullptr), "H2D");
      check(dfx_memcpy_h2d((char *)du + s * step(sbytes), hu.data(), sbytes, nullptr), "H2D");
    }
    check(dfx_memcpy_h2d(dw, w.data(), w.size(), nullptr), "H2D");
    check(dfx_stream_sync(nullptr), "sync");
    auto src_of = [&](size_t s) { return (char *)ds + s * step(sbytes); };
    auto u8_of = [&](size_t s) { return (char *)du + s * step(sbytes); };
    auto dst_of = [&](size_t s) { return (char *)dd + s * step(obytes); };

    std::vector<Leg> legs;
    uint64_t ops = 0, bytes = 0;
    const struct { const char *name; int path; const char *bm; } lin[] = {{"tile128", DFX_LINEAR_TILE, "128"}, {"tile64", DFX_LINEAR_TILE, "64"},
                                                                          {"generic", DFX_LINEAR_GENERIC, nullptr}};
    for (const auto &l : lin) {
      if (l.path == DFX_LINEAR_GENERIC && !with_generic) continue;
      dfx_linear_desc d;
      memset(&d, 0, sizeof(d));
      d.rows = p.rows; d.k = p.k; d.n = p.n; d.src_dt = DFX_S8; d.dst_dt = DFX_S8; d.bia_dt = DFX_UNDEF; d.round_mode = DFX_ROUND_NEAREST;
      d.nscales = 1; d.lut_in_dt = p.table ? DFX_S8 : DFX_UNDEF; d.force_path = l.path; d.src_ld = p.k; d.dst_ld = p.n;
      dfx_linear_t *h = nullptr;
      check(dfx_debug_set_tuning("DFX_LINEAR_BM", l.bm), "set tuning");
      check(dfx_linear_create(&d, &h), "linear create");
      check(dfx_debug_set_tuning("DFX_LINEAR_BM", nullptr), "set tuning");
      check(dfx_linear_set_weights(h, w.data(), nullptr, &scale), "linear set_weights");
      if (p.table) check(dfx_linear_set_table(h, lut.data()), "linear set_table");
      dfx_linear_info info;
      check(dfx_linear_query(h, &info), "linear query");
      ops = info.algorithmic_ops;
      bytes = info.algorithmic_bytes;
      legs.push_back(Leg{l.name, info.kernel_name, [=](size_t s) { check(dfx_linear_submit(h, src_of(s), dst_of(s), nullptr), "linear submit"); },
                         [=]() { dfx_linear_destroy(h); }, true, 0, {}, {}});
    }
    {  // dfx_bmm's MFMA kernel: one matrix, B = the weights on the device
      dfx_bmm_desc d;
      memset(&d, 0, sizeof(d));
      d.batch0 = 1; d.batch1 = 1; d.m = (int)p.rows; d.n = p.n; d.k = p.k; d.trans_b = 1; d.a_dt = DFX_S8; d.b_dt = DFX_S8; d.dst_dt = DFX_S8;
      d.round_mode = DFX_ROUND_NEAREST; d.nscales = 1; d.force_path = DFX_BMM_MFMA; d.lda = p.k; d.ldb = p.k; d.ldc = p.n;
      dfx_bmm_t *h = nullptr;
      check(dfx_bmm_create(&d, &h), "bmm create");
      check(dfx_bmm_set_scales(h, &scale), "bmm set_scales");
      dfx_bmm_info info;
      check(dfx_bmm_query(h, &info), "bmm query");
      legs.push_back(Leg{"bmm", info.kernel_name, [=](size_t s) { check(dfx_bmm_submit(h, src_of(s), dw, dst_of(s), nullptr), "bmm submit"); },
                         [=]() { dfx_bmm_destroy(h); }, !p.table, 0, {}, {}});
    }
    if (p.rows * (long long)p.n < (1ll << 31)) {  // dfx_fc on the u8 copy (ih = iw = 1): another arithmetic (the values differ by 128 * sum(w))
      dfx_fc_desc d;
      memset(&d, 0, sizeof(d));
      d.bs = (int)p.rows; d.ic = p.k; d.ih = 1; d.iw = 1; d.oc = p.n; d.dst_dt = DFX_S8; d.bia_dt = DFX_UNDEF; d.round_mode = DFX_ROUND_NEAREST;
      d.nscales = 1; d.force_path = -1;
      dfx_fc_t *h = nullptr;
      check(dfx_fc_create(&d, &h), "fc create");
      check(dfx_fc_set_weights(h, w.data(), nullptr, &scale), "fc set_weights");
      dfx_fc_info info;
      check(dfx_fc_query(h, &info), "fc query");
      legs.push_back(Leg{"fc(u8)", info.kernel_name, [=](size_t s) { check(dfx_fc_submit(h, u8_of(s), dst_of(s), nullptr), "fc submit"); },
                         [=]() { dfx_fc_destroy(h); }, false, 0, {}, {}});
    }
    if (p.k % 16 == 0 && p.n % 16 == 0) {  // the 1x1 dfx_conv on the u8 copy: one image of rows x 1 pixels
      dfx_conv_desc d;
      memset(&d, 0, sizeof(d));
      d.bs = 1; d.ic = p.k; d.ih = (int)p.rows; d.iw = 1; d.oc = p.n; d.oh = (int)p.rows; d.ow = 1; d.kh = 1; d.kw = 1; d.sh = 1; d.sw = 1;
      d.dst_dt = DFX_S8; d.bia0_dt = DFX_UNDEF; d.bia1_dt = DFX_UNDEF; d.conv0_round_mode = DFX_ROUND_NEAREST; d.conv1_round_mode = DFX_ROUND_NEAREST;
      d.conv0_nscales = 1; d.conv1_nscales = 1; d.force_variant = -1;
      dfx_conv_t *h = nullptr;
      if (dfx_conv_create(&d, &h) == DFX_OK) {
        std::vector<int8_t> blk(w.size());
        check(dfx_reorder_oihw_to_blocked(w.data(), blk.data(), p.n, p.k, 1, 1), "reorder weights");
        check(dfx_conv_set_weights(h, blk.data(), nullptr, &scale, nullptr, nullptr, nullptr), "conv set_weights");
        dfx_conv_info info;
        check(dfx_conv_query(h, &info), "conv query");
        legs.push_back(Leg{"conv1x1(u8)", info.kernel_name, [=](size_t s) { check(dfx_conv_submit(h, u8_of(s), dst_of(s), nullptr), "conv submit"); },
                           [=]() { dfx_conv_destroy(h); }, false, 0, {}, {}});
      } else {
        printf("%-34s %-9s not available: %s\n", p.name.c_str(), "conv1x1", dfx_last_error());
      }
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
      const double med = l.us[l.us.size() / 2], tops = (double)ops / med / 1e6;
      printf("%-34s %-9s %9.2f (%7.2f .. %7.2f) %8.1f %6.2f %7.3f  %s, %d submits\n", p.name.c_str(), l.name.c_str(), med, l.us.front(), l.us.back(), tops,
             100.0 * tops / 4600.0, (double)bytes / med / 1e6, l.kernel.c_str(), l.iters);
    }
    for (Leg &l : legs)
      if (l.compare && l.out != legs[0].out) { fprintf(stderr, "leg %s disagrees with leg %s on %s\n", l.name.c_str(), legs[0].name.c_str(), p.name.c_str()); return 1; }
    for (Leg &l : legs) l.destroy();
    dfx_mem_free_device(ds);
    dfx_mem_free_device(du);
    dfx_mem_free_device(dd);
    dfx_mem_free_device(dw);
  }
  dfx_event_destroy(e0);
  dfx_event_destroy(e1);
  return 0;
}
