// bench_select -- times the image-wide top-K with peak filter (dfx_select_*) on MI355X through the C ABI:
//   centernet   128x128x80 u8, peak3, k 100, bs 1 / 8 / 32
//   retinanet   one level 100x136x720 u8, all, min_val 128, k 1000, bs 1 / 8
//   rpn         200x304x3/16 u8, all, k 2000, bs 1
//   classifier  {bs, 1000} (ld 1008) s8, all, k 100, bs 1 / 128
//   small       8x8, 16x16, 32x32, 64x64 x 64 u8 (4 KiB to 256 KiB per image), peak3, k 100: where the two paths cross
// Legs, alternating at every point: the histogram path and the generic kernel, forced.  Device-resident, back-to-back submits
// between two events, the median of -rounds rounds per leg; TB/s of the valid src bytes, and the time as a multiple of the
// floor of reading src (every byte of it, pad channels included) once at the 5.9 TB/s a calibrated copy reaches.  The submits
// rotate over enough buffer sets to exceed -rotate_mb (default 768: three times the 256 MiB Infinity Cache); -rotate_mb 0
// times one set over and over (warm caches).  idx, val and count of the two legs are compared byte for byte.
//   bench_select [-iter 30] [-burning_iter 3] [-rounds 3] [-rotate_mb 768] [-only <substring of a point's name>]
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "cli_flags.h"
#include "dfx.h"

struct Point {
  const char *name;
  int bs, h, w, c, ld, dt, peak, min_val, k;
};

static void check(int rc, const char *what) {
  if (rc != DFX_OK) { fprintf(stderr, "%s failed (%d): %s\n", what, rc, dfx_last_error()); exit(1); }
}

int main(int argc, char **argv) {
  Flags f(argc, argv);
  const int burn = f.geti("burning_iter", 3), iters = f.geti("iter", 30), rounds = f.geti("rounds", 3);
  const std::string only = f.gets("only", "");
  const size_t rotate = (size_t)f.geti("rotate_mb", 768) << 20;
  const Point points[] = {
      {"centernet 1x128x128x80 peak3 k100", 1, 128, 128, 80, 80, DFX_U8, DFX_SELECT_PEAK3, 0, 100},
      {"centernet 8x128x128x80 peak3 k100", 8, 128, 128, 80, 80, DFX_U8, DFX_SELECT_PEAK3, 0, 100},
      {"centernet 32x128x128x80 peak3 k100", 32, 128, 128, 80, 80, DFX_U8, DFX_SELECT_PEAK3, 0, 100},
      {"retinanet 1x100x136x720 min128 k1000", 1, 100, 136, 720, 720, DFX_U8, DFX_SELECT_ALL, 128, 1000},
      {"retinanet 8x100x136x720 min128 k1000", 8, 100, 136, 720, 720, DFX_U8, DFX_SELECT_ALL, 128, 1000},
      {"rpn 1x200x304x3/16 k2000", 1, 200, 304, 3, 16, DFX_U8, DFX_SELECT_ALL, 0, 2000},
      {"classifier 1x1000/1008 s8 k100", 1, 1, 1, 1000, 1008, DFX_S8, DFX_SELECT_ALL, -128, 100},
      {"classifier 128x1000/1008 s8 k100", 128, 1, 1, 1000, 1008, DFX_S8, DFX_SELECT_ALL, -128, 100},
      {"small 1x8x8x64 peak3 k100", 1, 8, 8, 64, 64, DFX_U8, DFX_SELECT_PEAK3, 0, 100},
      {"small 8x8x8x64 peak3 k100", 8, 8, 8, 64, 64, DFX_U8, DFX_SELECT_PEAK3, 0, 100},
      {"small 1x16x16x64 peak3 k100", 1, 16, 16, 64, 64, DFX_U8, DFX_SELECT_PEAK3, 0, 100},
      {"small 8x16x16x64 peak3 k100", 8, 16, 16, 64, 64, DFX_U8, DFX_SELECT_PEAK3, 0, 100},
      {"small 1x32x32x64 peak3 k100", 1, 32, 32, 64, 64, DFX_U8, DFX_SELECT_PEAK3, 0, 100},
      {"small 8x32x32x64 peak3 k100", 8, 32, 32, 64, 64, DFX_U8, DFX_SELECT_PEAK3, 0, 100},
      {"small 1x64x64x64 peak3 k100", 1, 64, 64, 64, 64, DFX_U8, DFX_SELECT_PEAK3, 0, 100},
  };
  printf("bench_select: %d timed submits per round after %d warm-up submits, median of %d rounds, legs alternating; buffers in rotation: %zu MiB%s\n",
         iters, burn, rounds, rotate >> 20, rotate ? "" : " (one set: warm caches)");
  printf("%-40s %-8s %10s %8s %8s  %s\n", "point", "leg", "us", "TB/s", "x floor", "kernel name, chunks x pixels, grid");
  dfx_event_t e0, e1;
  check(dfx_event_create(&e0), "event create");
  check(dfx_event_create(&e1), "event create");
  const char *leg_name[2] = {"hist", "generic"};
  for (const Point &p : points) {
    if (!only.empty() && !strstr(p.name, only.c_str())) continue;
    const size_t sbytes = (size_t)p.bs * p.h * p.w * p.ld, valid = (size_t)p.bs * p.h * p.w * p.c;
    const size_t ibytes = (size_t)p.bs * p.k * 4, vbytes = (size_t)p.bs * p.k, cbytes = (size_t)p.bs * 4;
    const size_t nsets = std::max<size_t>(1, std::min<size_t>(4096, (rotate + sbytes - 1) / sbytes));
    auto step = [](size_t b) { return (b + 255) / 256 * 256; };
    // a skewed map: most scores low, few high, ties everywhere
    std::vector<unsigned char> hs(sbytes);
    Lcg g(7);
    for (size_t i = 0; i < sbytes; ++i) {
      const unsigned v = ((g.next() & 0xff) * (g.next() & 0xff)) >> 8;
      hs[i] = (unsigned char)(p.dt == DFX_S8 ? v ^ 0x80u : v);
    }
    void *ds = nullptr, *di = nullptr, *dv = nullptr, *dc = nullptr;
    check(dfx_mem_alloc_device(&ds, step(sbytes) * nsets), "device alloc");
    check(dfx_mem_alloc_device(&di, step(ibytes) * nsets), "device alloc");
    check(dfx_mem_alloc_device(&dv, step(vbytes) * nsets), "device alloc");
    check(dfx_mem_alloc_device(&dc, step(cbytes) * nsets), "device alloc");
    for (size_t k = 0; k < nsets; ++k) check(dfx_memcpy_h2d((char *)ds + k * step(sbytes), hs.data(), sbytes, nullptr), "H2D");
    check(dfx_stream_sync(nullptr), "sync");

    dfx_select_t *h[2] = {nullptr, nullptr};
    dfx_select_info info[2];
    for (int k = 0; k < 2; ++k) {
      dfx_select_desc d;
      memset(&d, 0, sizeof(d));
      d.bs = p.bs; d.h = p.h; d.w = p.w; d.c = p.c; d.src_ld = p.ld; d.src_dt = p.dt; d.k = p.k; d.idx_ld = p.k;
      d.peak = p.peak; d.min_val = p.min_val; d.force_path = k;
      check(dfx_select_create(&d, &h[k]), "select create");
      check(dfx_select_query(h[k], &info[k]), "query");
    }
    size_t turn = 0;
    auto launch = [&](int k) {
      const size_t s = turn++ % nsets;
      check(dfx_select_submit(h[k], (char *)ds + s * step(sbytes), (char *)di + s * step(ibytes), (char *)dv + s * step(vbytes),
                              (char *)dc + s * step(cbytes), nullptr, nullptr, nullptr),
            "select submit");
    };
    std::vector<double> us[2];
    std::vector<unsigned char> out[2];
    for (int r = 0; r < rounds; ++r)
      for (int k = 0; k < 2; ++k) {
        for (int i = 0; i < burn; ++i) launch(k);
        check(dfx_event_record(e0, nullptr), "record");
        for (int i = 0; i < iters; ++i) launch(k);
        check(dfx_event_record(e1, nullptr), "record");
        float ms = 0;
        check(dfx_event_elapsed_ms(e0, e1, &ms), "elapsed");
        us[k].push_back(ms * 1000.0 / iters);
        if (r == 0) {
          const size_t s = (turn - 1) % nsets;
          out[k].resize(ibytes + vbytes + cbytes);
          check(dfx_memcpy_d2h(out[k].data(), (char *)di + s * step(ibytes), ibytes, nullptr), "D2H");
          check(dfx_memcpy_d2h(out[k].data() + ibytes, (char *)dv + s * step(vbytes), vbytes, nullptr), "D2H");
          check(dfx_memcpy_d2h(out[k].data() + ibytes + vbytes, (char *)dc + s * step(cbytes), cbytes, nullptr), "D2H");
          check(dfx_stream_sync(nullptr), "sync");
        }
      }
    double med[2] = {0, 0};
    const double floor_us = (double)sbytes / 5.9e6;
    for (int k = 0; k < 2; ++k) {
      std::sort(us[k].begin(), us[k].end());
      med[k] = us[k][us[k].size() / 2];
      printf("%-40s %-8s %10.2f %8.3f %8.1f  %s, %d x %d, grid %d\n", p.name, leg_name[k], med[k], (double)valid / med[k] / 1e6, med[k] / floor_us,
             info[k].kernel_name, info[k].chunks, info[k].chunk_pixels, info[k].grid);
    }
    int first_count;
    memcpy(&first_count, out[1].data() + ibytes + vbytes, 4);
    printf("%-40s hist time / generic time: %.3f; floor %.2f us; count[0] %d; %zu buffer sets\n", "", med[0] / med[1], floor_us, first_count, nsets);
    if (out[0] != out[1]) { fprintf(stderr, "the histogram path and the generic kernel disagree on %s\n", p.name); return 1; }
    for (int k = 0; k < 2; ++k) dfx_select_destroy(h[k]);
    dfx_mem_free_device(ds);
    dfx_mem_free_device(di);
    dfx_mem_free_device(dv);
    dfx_mem_free_device(dc);
  }
  dfx_event_destroy(e0);
  dfx_event_destroy(e1);
  return 0;
}
