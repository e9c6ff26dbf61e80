// bench_lnorm -- times the int8 layer norm / RMS norm (dfx_lnorm_*) on MI355X through the C ABI:
//   ViT-B         {8 * 197, 768} and {64 * 197, 768}
//   Swin-T        the four stages on 64 images: {64 * 3136, 96}, {64 * 784, 192}, {64 * 196, 384}, {64 * 49, 768}
//   DETR          {2 * 850, 256};  MobileViT {64 * 256, 144};  long rows {4096, 1280}, {2048, 4096}, {512, 16384}
// each s8 -> s8 without and with shifts and s8 -> f32 in LAYER mode, and ViT-B bs 64 in RMS mode as well.
// Legs, alternating at every point: the row kernel and the generic kernel, forced.  Device-resident, back-to-back submits
// between two events; every window lasts at least -window_ms (the number of submits per window is set from a calibration
// run of each leg), the figure is the median of -rounds rounds.  Printed: us per submit, the ratio to the generic kernel,
// TB/s of algorithmic_bytes and the floor algorithmic_bytes / 5.9 TB/s (what a calibrated copy reaches) with the ratio to
// it.  The submits rotate over enough buffer sets to exceed -rotate_mb (default 768: three times the 256 MiB Infinity
// Cache); -rotate_mb 0 times one set over and over (warm caches).  The results of both legs are compared byte for byte.
//   bench_lnorm [-window_ms 3] [-burning_iter 5] [-rounds 5] [-rotate_mb 768] [-only <substring of a point's name>]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "cli_flags.h"
#include "dfx.h"

struct Point {
  std::string name;
  long long rows;
  int c, mode, dst_dt;
  bool shift;
};

static void check(int rc, const char *what) {
  if (rc != DFX_OK) { fprintf(stderr, "%s failed (%d): %s\n", what, rc, dfx_last_error()); exit(1); }
}

int main(int argc, char **argv) {
  Flags f(argc, argv);
  const int burn = f.geti("burning_iter", 5), rounds = f.geti("rounds", 5);
  const double window_ms = f.geti("window_ms", 3);
  const std::string only = f.gets("only", "");
  const size_t rotate = (size_t)f.geti("rotate_mb", 768) << 20;
  const struct { const char *n; long long rows; int c; } shapes[] = {
      {"vit-b bs8 1576x768", 8 * 197, 768},     {"vit-b bs64 12608x768", 64 * 197, 768}, {"swin-t s1 200704x96", 64 * 3136, 96},
      {"swin-t s2 50176x192", 64 * 784, 192},   {"swin-t s3 12544x384", 64 * 196, 384},  {"swin-t s4 3136x768", 64 * 49, 768},
      {"detr 1700x256", 2 * 850, 256},          {"mobilevit 16384x144", 64 * 256, 144},  {"4096x1280", 4096, 1280},
      {"2048x4096", 2048, 4096},                {"512x16384", 512, 16384}};
  std::vector<Point> points;
  for (const auto &s : shapes) {
    points.push_back({std::string(s.n) + " s8->s8", s.rows, s.c, DFX_LNORM_LAYER, DFX_S8, false});
    points.push_back({std::string(s.n) + " s8->s8 shift", s.rows, s.c, DFX_LNORM_LAYER, DFX_S8, true});
    points.push_back({std::string(s.n) + " s8->f32", s.rows, s.c, DFX_LNORM_LAYER, DFX_F32, false});
    if (s.rows == 64 * 197) points.push_back({std::string(s.n) + " s8->s8 rms", s.rows, s.c, DFX_LNORM_RMS, DFX_S8, false});
  }
  printf("bench_lnorm: windows of at least %.0f ms after %d warm-up submits, median of %d rounds, legs alternating; buffers in rotation: %zu MiB%s\n",
         window_ms, burn, rounds, rotate >> 20, rotate ? "" : " (one set: warm caches)");
  printf("%-36s %-8s %9s %7s %8s %9s %7s  %s\n", "point", "leg", "us", "/gen", "TB/s", "floor us", "/floor", "kernel name, grid, submits per window");
  dfx_event_t e0, e1;
  check(dfx_event_create(&e0), "event create");
  check(dfx_event_create(&e1), "event create");
  const char *leg_name[2] = {"row", "generic"};
  for (const Point &p : points) {
    if (!only.empty() && !strstr(p.name.c_str(), only.c_str())) continue;
    const size_t osz = p.dst_dt == DFX_F32 ? 4 : 1;
    const size_t sbytes = (size_t)p.rows * p.c, obytes = (size_t)p.rows * p.c * osz;
    const size_t nsets = std::max<size_t>(1, std::min<size_t>(4096, (rotate + sbytes + obytes - 1) / (sbytes + obytes)));
    auto step = [](size_t b) { return (b + 255) / 256 * 256; };
    std::vector<unsigned char> hs(sbytes);
    Lcg g(7);
    for (size_t k = 0; k < sbytes; ++k) hs[k] = (unsigned char)(g.next() & 0xff);
    std::vector<float> gamma(p.c), beta(p.c);
    std::vector<uint8_t> shift(p.c);
    for (int k = 0; k < p.c; ++k) {
      gamma[k] = ((float)(g.next() % 2001) - 1000.f) * 0.03f;
      beta[k] = ((float)(g.next() % 2001) - 1000.f) * 0.01f;
      shift[k] = (uint8_t)(g.next() % 8);
    }
    void *ds = nullptr, *dd = nullptr;
    check(dfx_mem_alloc_device(&ds, step(sbytes) * nsets), "device alloc");
    check(dfx_mem_alloc_device(&dd, step(obytes) * nsets), "device alloc");
    for (size_t k = 0; k < nsets; ++k) check(dfx_memcpy_h2d((char *)ds + k * step(sbytes), hs.data(), sbytes, nullptr), "H2D");
    check(dfx_stream_sync(nullptr), "sync");

    dfx_lnorm_t *h[2] = {nullptr, nullptr};
    dfx_lnorm_info info[2];
    for (int k = 0; k < 2; ++k) {
      dfx_lnorm_desc d;
      memset(&d, 0, sizeof(d));
      d.rows = p.rows; d.mode = p.mode; d.src_dt = DFX_S8; d.dst_dt = p.dst_dt; d.c = p.c; d.src_ld = p.c; d.dst_ld = p.c;
      d.eps = 0.25f; d.force_path = k;
      check(dfx_lnorm_create(&d, &h[k]), "lnorm create");
      check(dfx_lnorm_set_params(h[k], gamma.data(), beta.data(), p.shift ? shift.data() : nullptr), "set_params");
      check(dfx_lnorm_query(h[k], &info[k]), "query");
    }
    size_t turn = 0;
    auto launch = [&](int k) {
      const size_t s = turn++ % nsets;
      check(dfx_lnorm_submit(h[k], (char *)ds + s * step(sbytes), (char *)dd + s * step(obytes), nullptr), "lnorm submit");
    };
    auto window = [&](int k, int iters) {
      for (int i = 0; i < burn; ++i) launch(k);
      check(dfx_event_record(e0, nullptr), "record");
      for (int i = 0; i < iters; ++i) launch(k);
      check(dfx_event_record(e1, nullptr), "record");
      float ms = 0;
      check(dfx_event_elapsed_ms(e0, e1, &ms), "elapsed");
      return (double)ms;
    };
    int iters[2];
    for (int k = 0; k < 2; ++k) {  // calibration: submits per window for at least window_ms
      const double ms = window(k, 10) / 10;
      iters[k] = (int)std::min(20000.0, std::max(20.0, std::ceil(window_ms * 1.25 / std::max(ms, 1e-4))));
    }
    std::vector<double> us[2];
    std::vector<unsigned char> out[2];
    for (int r = 0; r < rounds; ++r)
      for (int k = 0; k < 2; ++k) {
        us[k].push_back(window(k, iters[k]) * 1000.0 / iters[k]);
        if (r == 0) {
          out[k].resize(obytes);
          check(dfx_memcpy_d2h(out[k].data(), (char *)dd + ((turn - 1) % nsets) * step(obytes), obytes, nullptr), "D2H");
          check(dfx_stream_sync(nullptr), "sync");
        }
      }
    double med[2] = {0, 0};
    for (int k = 0; k < 2; ++k) {
      std::sort(us[k].begin(), us[k].end());
      med[k] = us[k][us[k].size() / 2];
    }
    for (int k = 0; k < 2; ++k) {
      const double tbs = (double)info[k].algorithmic_bytes / med[k] / 1e6, floor_us = (double)info[k].algorithmic_bytes / 5.9e6;
      printf("%-36s %-8s %9.2f %7.3f %8.3f %9.2f %7.2f  %s, grid %d, %d submits\n", p.name.c_str(), leg_name[k], med[k], med[k] / med[DFX_LNORM_GENERIC], tbs,
             floor_us, med[k] / floor_us, info[k].kernel_name, info[k].grid, iters[k]);
    }
    if (out[0] != out[1]) { fprintf(stderr, "the row and the generic kernels disagree on %s\n", p.name.c_str()); return 1; }
    for (int k = 0; k < 2; ++k) dfx_lnorm_destroy(h[k]);
    dfx_mem_free_device(ds);
    dfx_mem_free_device(dd);
  }
  dfx_event_destroy(e0);
  dfx_event_destroy(e1);
  return 0;
}
