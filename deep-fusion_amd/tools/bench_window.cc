// bench_window -- times the window partition / reverse op (dfx_window_*) on MI355X through the C ABI, s8 tokens:
//   Swin-T at 224   the four stages 56x56x96, 28x28x192, 14x14x384, 7x7x768 under window 7, shift 0 and 3, bs 1 and 64:
//                   the partition, and for the shifted block the reverse as well
//   detection       200x304x96, bs 2, window 7 (padding on both axes), shift 0 and 3, partition and reverse
//   patch merging   the three gathers 56x56x96, 28x28x192, 14x14x384 (2 x 2, column-major), bs 1 and 64
// Legs, alternating at every point: the row kernel and the generic kernel, forced.  Device-resident, back-to-back submits
// between two events; every window lasts at least -window_ms (the number of submits per window is set from a calibration
// run of each leg), the figure is the median of -rounds rounds.  Printed: us per submit, the ratio to the generic kernel,
// TB/s of algorithmic_bytes and the floor algorithmic_bytes / 5.9 TB/s (what a calibrated copy reaches) with the ratio to
// it.  The submits rotate over enough buffer sets to exceed -rotate_mb (default 768: three times the 256 MiB Infinity
// Cache); -rotate_mb 0 times one set over and over (warm caches).  The results of both legs are compared byte for byte.
//   bench_window [-window_ms 3] [-burning_iter 5] [-rounds 5] [-rotate_mb 768] [-only <substring of a point's name>]
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
  int dir, bs, h, w, c, win, shift, order;
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
  std::vector<Point> points;
  const struct { const char *n; int hw, c; } stages[] = {{"swin-t s1 56x56x96", 56, 96}, {"swin-t s2 28x28x192", 28, 192}, {"swin-t s3 14x14x384", 14, 384}, {"swin-t s4 7x7x768", 7, 768}};
  for (int bs : {1, 64})
    for (const auto &s : stages) {
      const std::string n = std::string(s.n) + " bs" + std::to_string(bs);
      points.push_back({n + " part", DFX_WINDOW_PARTITION, bs, s.hw, s.hw, s.c, 7, 0, DFX_WINDOW_ROW_MAJOR});
      points.push_back({n + " part shift3", DFX_WINDOW_PARTITION, bs, s.hw, s.hw, s.c, 7, 3, DFX_WINDOW_ROW_MAJOR});
      points.push_back({n + " rev shift3", DFX_WINDOW_REVERSE, bs, s.hw, s.hw, s.c, 7, 3, DFX_WINDOW_ROW_MAJOR});
    }
  for (int shift : {0, 3})
    for (int dir : {(int)DFX_WINDOW_PARTITION, (int)DFX_WINDOW_REVERSE})
      points.push_back({std::string("det 200x304x96 bs2 ") + (dir ? "rev" : "part") + (shift ? " shift3" : ""), dir, 2, 200, 304, 96, 7, shift, DFX_WINDOW_ROW_MAJOR});
  for (int bs : {1, 64})
    for (int k = 0; k < 3; ++k)
      points.push_back({std::string("merge ") + std::to_string(stages[k].hw) + "x" + std::to_string(stages[k].hw) + "x" + std::to_string(stages[k].c) + " bs" + std::to_string(bs),
                        DFX_WINDOW_PARTITION, bs, stages[k].hw, stages[k].hw, stages[k].c, 2, 0, DFX_WINDOW_COL_MAJOR});
  printf("bench_window: windows of at least %.0f ms after %d warm-up submits, median of %d rounds, legs alternating; buffers in rotation: %zu MiB%s\n",
         window_ms, burn, rounds, rotate >> 20, rotate ? "" : " (one set: warm caches)");
  printf("%-40s %-8s %9s %7s %8s %9s %7s  %s\n", "point", "leg", "us", "/gen", "TB/s", "floor us", "/floor", "kernel name, grid, submits per window");
  dfx_event_t e0, e1;
  check(dfx_event_create(&e0), "event create");
  check(dfx_event_create(&e1), "event create");
  const char *leg_name[2] = {"row", "generic"};
  for (const Point &p : points) {
    if (!only.empty() && !strstr(p.name.c_str(), only.c_str())) continue;
    const int hp = (p.h + p.win - 1) / p.win * p.win, wp = (p.w + p.win - 1) / p.win * p.win;
    const size_t gbytes = (size_t)p.bs * p.h * p.w * p.c, wbytes = (size_t)p.bs * hp * wp * p.c;
    const size_t sbytes = p.dir == DFX_WINDOW_PARTITION ? gbytes : wbytes, obytes = p.dir == DFX_WINDOW_PARTITION ? wbytes : gbytes;
    const size_t nsets = std::max<size_t>(1, std::min<size_t>(4096, (rotate + sbytes + obytes - 1) / (sbytes + obytes)));
    auto step = [](size_t b) { return (b + 255) / 256 * 256; };
    std::vector<unsigned char> hs(sbytes);
    Lcg g(7);
    for (size_t k = 0; k < sbytes; ++k) hs[k] = (unsigned char)(g.next() & 0xff);
    void *ds = nullptr, *dd = nullptr;
    check(dfx_mem_alloc_device(&ds, step(sbytes) * nsets), "device alloc");
    check(dfx_mem_alloc_device(&dd, step(obytes) * nsets), "device alloc");
    for (size_t k = 0; k < nsets; ++k) check(dfx_memcpy_h2d((char *)ds + k * step(sbytes), hs.data(), sbytes, nullptr), "H2D");
    check(dfx_stream_sync(nullptr), "sync");

    dfx_window_t *h[2] = {nullptr, nullptr};
    dfx_window_info info[2];
    for (int k = 0; k < 2; ++k) {
      dfx_window_desc d;
      memset(&d, 0, sizeof(d));
      d.dir = p.dir; d.dt = DFX_S8; d.bs = p.bs; d.h = p.h; d.w = p.w; d.c = p.c; d.wh = d.ww = p.win; d.shift_y = d.shift_x = p.shift;
      d.order = p.order; d.grid_ld = d.win_ld = p.c; d.pad_value = 0; d.force_path = k;
      check(dfx_window_create(&d, &h[k]), "window create");
      check(dfx_window_query(h[k], &info[k]), "query");
    }
    size_t turn = 0;
    auto launch = [&](int k) {
      const size_t s = turn++ % nsets;
      check(dfx_window_submit(h[k], (char *)ds + s * step(sbytes), (char *)dd + s * step(obytes), nullptr), "window submit");
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
      printf("%-40s %-8s %9.2f %7.3f %8.3f %9.2f %7.2f  %s, grid %d, %d submits\n", p.name.c_str(), leg_name[k], med[k], med[k] / med[DFX_WINDOW_GENERIC], tbs,
             floor_us, med[k] / floor_us, info[k].kernel_name, info[k].grid, iters[k]);
    }
    if (out[0] != out[1]) { fprintf(stderr, "the row and the generic kernels disagree on %s\n", p.name.c_str()); return 1; }
    for (int k = 0; k < 2; ++k) dfx_window_destroy(h[k]);
    dfx_mem_free_device(ds);
    dfx_mem_free_device(dd);
  }
  dfx_event_destroy(e0);
  dfx_event_destroy(e1);
  return 0;
}
