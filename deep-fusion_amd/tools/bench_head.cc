// bench_head -- times the net head (dfx_head_*: channel top-k / argmax and softmax) on MI355X through the C ABI:
//   segmentation  argmax u8 -> u8 and softmax u8 -> u8 at 1x65x65x21/32 (the launch floor), 16x129x129x21/32, 4x513x513x21/32,
//                 8x512x1024x19/32, 8x128x128x150/160; top-5 s8 at 4x513x513x21/32 (short rows outside the pixel class)
//   classifier    top-5 (s32 idx) and softmax (f32 dst; s8 src only) on {bs, 1000} s8 (ld 1008) and f32 at bs 1, 8, 128
// Legs, alternating at every point: every path whose class holds the point, forced (pixel, row, generic).  Device-resident,
// back-to-back submits between two events, the median of -rounds rounds per leg; TB/s of algorithmic_bytes (valid channels +
// outputs) and that as a share of the 8 TB/s HBM peak and of the 5.9 TB/s a calibrated copy reaches.  The submits rotate
// over enough buffer sets to exceed -rotate_mb (default 768: three times the 256 MiB Infinity Cache); -rotate_mb 0 times one
// set over and over (warm caches).  The results of all legs are compared byte for byte.
//   bench_head [-iter 50] [-burning_iter 5] [-rounds 3] [-rotate_mb 768] [-only <substring of a point's name>]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "cli_flags.h"
#include "dfx.h"

struct Point {
  const char *name;
  long long rows;
  int c, ld;
  int src_dt, mode, k, dst_dt;
};

static void check(int rc, const char *what) {
  if (rc != DFX_OK) { fprintf(stderr, "%s failed (%d): %s\n", what, rc, dfx_last_error()); exit(1); }
}
static size_t esize(int dt) { return (dt == DFX_F32 || dt == DFX_S32) ? 4 : 1; }

int main(int argc, char **argv) {
  Flags f(argc, argv);
  const int burn = f.geti("burning_iter", 5), iters = f.geti("iter", 50), rounds = f.geti("rounds", 3);
  const std::string only = f.gets("only", "");
  const size_t rotate = (size_t)f.geti("rotate_mb", 768) << 20;
  std::vector<Point> points;
  const struct { const char *n; long long rows; int c, ld; } seg[] = {
      {"1x65x65x21/32", 65ll * 65, 21, 32}, {"16x129x129x21/32", 16ll * 129 * 129, 21, 32}, {"4x513x513x21/32", 4ll * 513 * 513, 21, 32},
      {"8x512x1024x19/32", 8ll * 512 * 1024, 19, 32}, {"8x128x128x150/160", 8ll * 128 * 128, 150, 160}};
  static char names[64][64];
  int nn = 0;
  for (int mode : {DFX_HEAD_TOPK, DFX_HEAD_SOFTMAX})
    for (const auto &s : seg) {
      snprintf(names[nn], sizeof(names[nn]), "%s u8 %s", mode == DFX_HEAD_TOPK ? "argmax" : "softmax", s.n);
      points.push_back({names[nn++], s.rows, s.c, s.ld, DFX_U8, mode, 1, DFX_U8});
    }
  points.push_back({"top5 s8 4x513x513x21/32", 4ll * 513 * 513, 21, 32, DFX_S8, DFX_HEAD_TOPK, 5, DFX_U8});
  for (int bs : {1, 8, 128}) {
    snprintf(names[nn], sizeof(names[nn]), "top5 s8 %dx1000/1008", bs);
    points.push_back({names[nn++], bs, 1000, 1008, DFX_S8, DFX_HEAD_TOPK, 5, DFX_S32});
    snprintf(names[nn], sizeof(names[nn]), "top5 f32 %dx1000", bs);
    points.push_back({names[nn++], bs, 1000, 1000, DFX_F32, DFX_HEAD_TOPK, 5, DFX_S32});
    snprintf(names[nn], sizeof(names[nn]), "softmax s8 %dx1000/1008", bs);
    points.push_back({names[nn++], bs, 1000, 1008, DFX_S8, DFX_HEAD_SOFTMAX, 0, DFX_F32});
  }
  printf("bench_head: %d timed submits per round after %d warm-up submits, median of %d rounds, legs alternating; buffers in rotation: %zu MiB%s\n",
         iters, burn, rounds, rotate >> 20, rotate ? "" : " (one set: warm caches)");
  printf("%-34s %-8s %10s %8s %6s %6s  %s\n", "point", "leg", "us", "TB/s", "%8.0", "%5.9", "kernel name, grid");
  dfx_event_t e0, e1;
  check(dfx_event_create(&e0), "event create");
  check(dfx_event_create(&e1), "event create");
  const char *leg_name[3] = {"pixel", "row", "generic"};
  for (const Point &p : points) {
    if (!only.empty() && !strstr(p.name, only.c_str())) continue;
    const bool softmax = p.mode == DFX_HEAD_SOFTMAX;
    const int out_ld = softmax ? p.c : p.k;
    const size_t sbytes = (size_t)p.rows * p.ld * esize(p.src_dt), obytes = (size_t)p.rows * out_ld * esize(p.dst_dt);
    const size_t nsets = std::max<size_t>(1, std::min<size_t>(4096, (rotate + sbytes + obytes - 1) / (sbytes + obytes)));
    auto step = [](size_t b) { return (b + 255) / 256 * 256; };
    std::vector<unsigned char> hs(sbytes);
    Lcg g(7);
    if (p.src_dt == DFX_F32) {
      float *v = (float *)hs.data();
      for (size_t k = 0; k < sbytes / 4; ++k) v[k] = (float)((int)(g.next() % 20001) - 10000) * 0.01f;
    } else {
      for (size_t k = 0; k < sbytes; ++k) hs[k] = (unsigned char)(g.next() & 0xff);
    }
    void *ds = nullptr, *dd = nullptr;
    check(dfx_mem_alloc_device(&ds, step(sbytes) * nsets), "device alloc");
    check(dfx_mem_alloc_device(&dd, step(obytes) * nsets), "device alloc");
    for (size_t k = 0; k < nsets; ++k) check(dfx_memcpy_h2d((char *)ds + k * step(sbytes), hs.data(), sbytes, nullptr), "H2D");
    check(dfx_stream_sync(nullptr), "sync");
    uint32_t E[256];
    for (int d = 0; d < 256; ++d) E[d] = (uint32_t)std::floor(std::exp(-d * 0.0625) * (double)(0xffffffffu / (uint32_t)p.c));

    dfx_head_t *h[3] = {nullptr, nullptr, nullptr};
    dfx_head_info info[3];
    for (int k = 0; k < 3; ++k) {
      dfx_head_desc d;
      memset(&d, 0, sizeof(d));
      d.rows = p.rows; d.mode = p.mode; d.src_dt = p.src_dt; d.dst_dt = p.dst_dt; d.c = p.c; d.src_ld = p.ld;
      d.dst_ld = out_ld; d.idx_ld = out_ld; d.k = p.k; d.out_scale = 255.0f; d.force_path = k;
      const int rc = dfx_head_create(&d, &h[k]);
      if (rc == DFX_ERR_UNSUPPORTED) continue;  // outside the path's class
      check(rc, "head create");
      if (softmax) check(dfx_head_set_table(h[k], E), "set_table");
      check(dfx_head_query(h[k], &info[k]), "query");
    }
    size_t turn = 0;
    auto launch = [&](int k) {
      const size_t s = turn++ % nsets;
      check(dfx_head_submit(h[k], (char *)ds + s * step(sbytes), (char *)dd + s * step(obytes), nullptr, nullptr), "head submit");
    };
    std::vector<double> us[3];
    std::vector<unsigned char> out[3];
    for (int r = 0; r < rounds; ++r)
      for (int k = 0; k < 3; ++k) {
        if (!h[k]) continue;
        for (int i = 0; i < burn; ++i) launch(k);
        check(dfx_event_record(e0, nullptr), "record");
        for (int i = 0; i < iters; ++i) launch(k);
        check(dfx_event_record(e1, nullptr), "record");
        float ms = 0;
        check(dfx_event_elapsed_ms(e0, e1, &ms), "elapsed");
        us[k].push_back(ms * 1000.0 / iters);
        if (r == 0) {
          out[k].resize(obytes);
          check(dfx_memcpy_d2h(out[k].data(), (char *)dd + ((turn - 1) % nsets) * step(obytes), obytes, nullptr), "D2H");
          check(dfx_stream_sync(nullptr), "sync");
        }
      }
    double med[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k) {
      if (!h[k]) continue;
      std::sort(us[k].begin(), us[k].end());
      med[k] = us[k][us[k].size() / 2];
      const double tbs = (double)info[k].algorithmic_bytes / med[k] / 1e6;
      printf("%-34s %-8s %10.2f %8.3f %6.1f %6.1f  %s, grid %d\n", p.name, leg_name[k], med[k], tbs, 100.0 * tbs / 8.0, 100.0 * tbs / 5.9, info[k].kernel_name,
             info[k].grid);
    }
    printf("%-34s time / generic time:", "");
    for (int k = 0; k < 2; ++k)
      if (h[k]) printf(" %s %.3f", leg_name[k], med[k] / med[DFX_HEAD_GENERIC]);
    printf("; %zu buffer sets\n", nsets);
    for (int k = 0; k < 2; ++k)
      if (h[k] && out[k] != out[DFX_HEAD_GENERIC]) { fprintf(stderr, "the %s and the generic kernels disagree on %s\n", leg_name[k], p.name); return 1; }
    for (int k = 0; k < 3; ++k) dfx_head_destroy(h[k]);
    dfx_mem_free_device(ds);
    dfx_mem_free_device(dd);
  }
  dfx_event_destroy(e0);
  dfx_event_destroy(e1);
  return 0;
}
