// bench_nms -- times the box decode + greedy NMS (dfx_nms_*) on MI355X through the C ABI:
//   retinanet   one level: n 1000, 80 classes, per class, thr 0.5, max_out 100 and 300, A 9
//   rpn         n 2000, class-agnostic, thr 0.7, max_out 1000, A 3
//   ssd         n 200, 21 classes, per class, thr 0.45, max_out 200, A 6
//   worst       n 4096, class-agnostic, thr 0.5, max_out 4096, at a low and a high kept fraction (boxes only)
//   few, small  n 1000 with max_out 20, and n 100: below the detectors' sizes, where the two paths cross (boxes only)
// each at bs 1 and 8, in DECODE mode (idx + delta rows + anchors) and in BOXES mode.  The boxes come from the seeded
// generator of nms_host.h (clusters of overlapping boxes; the anchors of DECODE mode are such boxes too, the delta bytes are
// small); the kept fraction of every point is printed.
// Legs, alternating at every point: the mask path and the generic kernel, forced, device-resident, back-to-back submits
// between two events; and "host": what a caller without this op does -- a D2H copy of idx + delta rows (or boxes) and
// count, the scalar decode + greedy NMS of nms_host.h, an H2D copy of keep, count and the kept boxes -- wall clock per frame,
// of which the copies are also stated alone (5 frames per round).  Median of -rounds rounds per leg.  The submits rotate over enough buffer sets
// to exceed -rotate_mb (default 768: three times the 256 MiB Infinity Cache), at most 16384 sets: the line of a point says
// how many MiB that came to.  keep, count and boxes_out of the three legs are compared byte for byte.
//   bench_nms [-iter 30] [-burning_iter 3] [-rounds 3] [-rotate_mb 768] [-only <substring of a point's name>]
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "cli_flags.h"
#include "dfx.h"
#include "nms_host.h"

struct Point {
  const char *name;
  int bs, n, max_out, mode, per_class, classes, apx, clusters;
  float thr, jitter;
};

static void check(int rc, const char *what) {
  if (rc != DFX_OK) { fprintf(stderr, "%s failed (%d): %s\n", what, rc, dfx_last_error()); exit(1); }
}
static double now_us() {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int main(int argc, char **argv) {
  Flags f(argc, argv);
  const int burn = f.geti("burning_iter", 3), iters = f.geti("iter", 30), rounds = f.geti("rounds", 3);
  const std::string only = f.gets("only", "");
  const size_t rotate = (size_t)f.geti("rotate_mb", 768) << 20;
  const int D = DFX_NMS_DECODE, B = DFX_NMS_BOXES;
  const Point points[] = {
      {"retinanet 1x1000 decode c80 out100", 1, 1000, 100, D, 1, 80, 9, 60, 0.5f, 8.f},
      {"retinanet 8x1000 decode c80 out100", 8, 1000, 100, D, 1, 80, 9, 60, 0.5f, 8.f},
      {"retinanet 1x1000 decode c80 out300", 1, 1000, 300, D, 1, 80, 9, 60, 0.5f, 8.f},
      {"retinanet 8x1000 decode c80 out300", 8, 1000, 300, D, 1, 80, 9, 60, 0.5f, 8.f},
      {"retinanet 1x1000 boxes c80 out100", 1, 1000, 100, B, 1, 80, 9, 60, 0.5f, 8.f},
      {"retinanet 8x1000 boxes c80 out100", 8, 1000, 100, B, 1, 80, 9, 60, 0.5f, 8.f},
      {"retinanet 1x1000 boxes c80 out300", 1, 1000, 300, B, 1, 80, 9, 60, 0.5f, 8.f},
      {"retinanet 8x1000 boxes c80 out300", 8, 1000, 300, B, 1, 80, 9, 60, 0.5f, 8.f},
      {"rpn 1x2000 decode agnostic out1000", 1, 2000, 1000, D, 0, 1, 3, 150, 0.7f, 8.f},
      {"rpn 8x2000 decode agnostic out1000", 8, 2000, 1000, D, 0, 1, 3, 150, 0.7f, 8.f},
      {"rpn 1x2000 boxes agnostic out1000", 1, 2000, 1000, B, 0, 1, 3, 150, 0.7f, 8.f},
      {"rpn 8x2000 boxes agnostic out1000", 8, 2000, 1000, B, 0, 1, 3, 150, 0.7f, 8.f},
      {"ssd 1x200 decode c21 out200", 1, 200, 200, D, 1, 21, 6, 20, 0.45f, 8.f},
      {"ssd 8x200 decode c21 out200", 8, 200, 200, D, 1, 21, 6, 20, 0.45f, 8.f},
      {"ssd 1x200 boxes c21 out200", 1, 200, 200, B, 1, 21, 6, 20, 0.45f, 8.f},
      {"ssd 8x200 boxes c21 out200", 8, 200, 200, B, 1, 21, 6, 20, 0.45f, 8.f},
      {"few 1x1000 boxes c80 out20", 1, 1000, 20, B, 1, 80, 9, 60, 0.5f, 8.f},
      {"few 8x1000 boxes c80 out20", 8, 1000, 20, B, 1, 80, 9, 60, 0.5f, 8.f},
      {"small 1x100 boxes agnostic out100", 1, 100, 100, B, 0, 1, 1, 10, 0.5f, 8.f},
      {"small 8x100 boxes agnostic out100", 8, 100, 100, B, 0, 1, 1, 10, 0.5f, 8.f},
      {"worst 1x4096 boxes low kept", 1, 4096, 4096, B, 0, 1, 1, 40, 0.5f, 4.f},
      {"worst 8x4096 boxes low kept", 8, 4096, 4096, B, 0, 1, 1, 40, 0.5f, 4.f},
      {"worst 1x4096 boxes high kept", 1, 4096, 4096, B, 0, 1, 1, 4000, 0.5f, 24.f},
      {"worst 8x4096 boxes high kept", 8, 4096, 4096, B, 0, 1, 1, 4000, 0.5f, 24.f},
  };
  printf("bench_nms: %d timed submits per round after %d warm-up submits, median of %d rounds, legs alternating; buffers in rotation: up to %zu MiB%s\n",
         iters, burn, rounds, rotate >> 20, rotate ? "" : " (one set: warm caches)");
  printf("%-38s %-8s %10s  %s\n", "point", "leg", "us", "kernel name / parts");
  dfx_event_t e0, e1;
  check(dfx_event_create(&e0), "event create");
  check(dfx_event_create(&e1), "event create");
  float tc[256], ts[256];
  for (int q = 0; q < 256; ++q) {
    const double d = (q - 128) / 32.0;
    tc[q] = (float)(d / 10.0);
    ts[q] = (float)std::exp(std::min(d / 5.0, std::log(1000.0 / 16)));
  }
  const char *leg_name[3] = {"mask", "generic", "host"};
  for (const Point &p : points) {
    if (!only.empty() && !strstr(p.name, only.c_str())) continue;
    const bool decode = p.mode == D;
    const size_t e = (size_t)p.bs * p.n;
    const int row_bytes = 4 * p.apx, na = decode ? p.n * 4 : 1000;
    // the problem, one seed per point
    NmsRng g(1000 + (uint64_t)(&p - points));
    std::vector<float> boxes(e * 4), anchors((size_t)na * 4);
    std::vector<int32_t> idx(e);
    std::vector<uint8_t> deltas(e * row_bytes);
    for (int r = 0; r < p.bs; ++r) nms_clustered_boxes(g, p.n, p.clusters, p.jitter, boxes.data() + (size_t)r * p.n * 4);
    nms_clustered_boxes(g, na, p.clusters, p.jitter, anchors.data());
    for (auto &v : idx) v = (int32_t)(g.next() % (uint32_t)na) * p.classes + (int32_t)(g.next() % (uint32_t)p.classes);
    for (auto &v : deltas) v = (uint8_t)(112u + g.next() % 32u);
    dfx_nms_desc d;
    memset(&d, 0, sizeof(d));
    d.bs = p.bs; d.n = p.n; d.max_out = p.max_out; d.keep_ld = p.max_out; d.mode = p.mode; d.per_class = p.per_class; d.classes = p.classes;
    d.anchors_per_pixel = p.apx; d.n_anchors = na; d.row_bytes = row_bytes; d.idx_ld = p.n; d.iou_thr = p.thr;
    // one input block per set: boxes | idx | deltas, 256-byte steps; outputs keep | count | boxes_out likewise
    auto step = [](size_t b) { return (b + 255) / 256 * 256; };
    const bool reads_idx = decode || p.per_class;
    const size_t o_box = 0, o_idx = decode ? 0 : step(e * 16), o_del = o_idx + (reads_idx ? step(e * 4) : 0);
    const size_t in_bytes = o_del + (decode ? step(e * row_bytes) : 0);
    const size_t kb = (size_t)p.bs * p.max_out * 4, cb = (size_t)p.bs * 4, bb = (size_t)p.bs * p.max_out * 16;
    const size_t o_cnt = step(kb), o_bo = o_cnt + step(cb), out_bytes = o_bo + step(bb);
    const size_t nsets = std::max<size_t>(1, std::min<size_t>(16384, (rotate + in_bytes - 1) / in_bytes));
    std::vector<uint8_t> hin(in_bytes, 0);
    if (!decode) memcpy(hin.data() + o_box, boxes.data(), e * 16);
    if (reads_idx) memcpy(hin.data() + o_idx, idx.data(), e * 4);
    if (decode) memcpy(hin.data() + o_del, deltas.data(), e * row_bytes);
    void *din = nullptr, *dout = nullptr, *danc = nullptr, *dtab = nullptr, *pin = nullptr, *pout = nullptr;
    check(dfx_mem_alloc_device(&din, in_bytes * nsets), "device alloc");
    check(dfx_mem_alloc_device(&dout, out_bytes * nsets), "device alloc");
    check(dfx_mem_alloc_device(&danc, anchors.size() * 4), "device alloc");
    check(dfx_mem_alloc_device(&dtab, 2048), "device alloc");
    check(dfx_mem_alloc_host(&pin, in_bytes), "host alloc");
    check(dfx_mem_alloc_host(&pout, out_bytes), "host alloc");
    for (size_t k = 0; k < nsets; ++k) check(dfx_memcpy_h2d((char *)din + k * in_bytes, hin.data(), in_bytes, nullptr), "H2D");
    check(dfx_memcpy_h2d(danc, anchors.data(), anchors.size() * 4, nullptr), "H2D");
    check(dfx_memcpy_h2d(dtab, tc, 1024, nullptr), "H2D");
    check(dfx_memcpy_h2d((char *)dtab + 1024, ts, 1024, nullptr), "H2D");
    check(dfx_stream_sync(nullptr), "sync");

    dfx_nms_t *h[2] = {nullptr, nullptr};
    dfx_nms_info info[2];
    for (int k = 0; k < 2; ++k) {
      d.force_path = k;
      check(dfx_nms_create(&d, &h[k]), "nms create");
      check(dfx_nms_query(h[k], &info[k]), "query");
    }
    size_t turn = 0;
    double copy_us = 0;  // of the host leg's last frame
    auto io_of = [&](size_t s) {
      dfx_nms_io io;
      memset(&io, 0, sizeof(io));
      char *in = (char *)din + s * in_bytes, *out = (char *)dout + s * out_bytes;
      if (!decode) io.boxes = in + o_box;
      if (reads_idx) io.idx = in + o_idx;
      if (decode) { io.deltas = in + o_del; io.anchors = danc; io.tab_c = dtab; io.tab_s = (char *)dtab + 1024; }
      io.keep = out; io.count = out + o_cnt; io.boxes_out = out + o_bo;
      return io;
    };
    auto launch = [&](int k) {
      const size_t s = turn++ % nsets;
      const dfx_nms_io io = io_of(s);
      if (k < 2) {
        check(dfx_nms_submit(h[k], &io, nullptr), "nms submit");
        return;
      }
      // what a caller does today
      const double t0 = now_us();
      check(dfx_memcpy_d2h(pin, (char *)din + s * in_bytes, in_bytes, nullptr), "D2H");
      check(dfx_stream_sync(nullptr), "sync");
      const double t1 = now_us();
      const char *hp = (const char *)pin;
      char *op = (char *)pout;
      nms_host(d, (const float *)(hp + o_box), (const int32_t *)(hp + o_idx), (const uint8_t *)(hp + o_del), anchors.data(), tc, ts, nullptr,
               (int32_t *)op, (int32_t *)(op + o_cnt), (float *)(op + o_bo));
      const double t2 = now_us();
      check(dfx_memcpy_h2d((char *)dout + s * out_bytes, pout, out_bytes, nullptr), "H2D");
      check(dfx_stream_sync(nullptr), "sync");
      copy_us = (t1 - t0) + (now_us() - t2);
    };
    std::vector<double> us[3], copies;
    std::vector<uint8_t> out[3];
    for (int r = 0; r < rounds; ++r)
      for (int k = 0; k < 3; ++k) {
        for (int i = 0; i < (k < 2 ? burn : 1); ++i) launch(k);
        if (k < 2) {
          check(dfx_event_record(e0, nullptr), "record");
          for (int i = 0; i < iters; ++i) launch(k);
          check(dfx_event_record(e1, nullptr), "record");
          float ms = 0;
          check(dfx_event_elapsed_ms(e0, e1, &ms), "elapsed");
          us[k].push_back(ms * 1000.0 / iters);
        } else {
          const double t0 = now_us();
          double c = 0;
          const int hi = std::min(iters, 5);  // (the scalar loop takes up to a second per frame)
          for (int i = 0; i < hi; ++i) { launch(k); c += copy_us; }
          us[k].push_back((now_us() - t0) / hi);
          copies.push_back(c / hi);
        }
        if (r == 0) {
          const size_t s = (turn - 1) % nsets;
          std::vector<uint8_t> raw(out_bytes);
          check(dfx_memcpy_d2h(raw.data(), (char *)dout + s * out_bytes, out_bytes, nullptr), "D2H");
          check(dfx_stream_sync(nullptr), "sync");
          out[k].insert(out[k].end(), raw.begin(), raw.begin() + kb);
          out[k].insert(out[k].end(), raw.begin() + o_cnt, raw.begin() + o_cnt + cb);
          out[k].insert(out[k].end(), raw.begin() + o_bo, raw.begin() + o_bo + bb);
        }
      }
    double med[3];
    for (int k = 0; k < 3; ++k) {
      std::sort(us[k].begin(), us[k].end());
      med[k] = us[k][us[k].size() / 2];
    }
    std::sort(copies.begin(), copies.end());
    for (int k = 0; k < 2; ++k)
      printf("%-38s %-8s %10.2f  %s, tiles %d, grids %d / %d / %d\n", p.name, leg_name[k], med[k], info[k].kernel_name, info[k].tiles, info[k].grid_prep,
             info[k].grid_mask, info[k].grid_scan);
    printf("%-38s %-8s %10.2f  of which the two copies %.2f us (%zu bytes down, %zu up)\n", p.name, leg_name[2], med[2], copies[copies.size() / 2], in_bytes,
           out_bytes);
    long long kept = 0;
    for (int r = 0; r < p.bs; ++r) {
      int32_t c;
      memcpy(&c, out[1].data() + kb + 4 * (size_t)r, 4);
      kept += c;
    }
    printf("%-38s mask / generic: %.3f; mask / host: %.3f; generic / host: %.3f; kept %.1f %% of n (%.1f per image); %zu sets, %.0f MiB in rotation\n", "",
           med[0] / med[1], med[0] / med[2], med[1] / med[2], 100.0 * (double)kept / (double)e, (double)kept / p.bs, nsets,
           (double)(in_bytes * nsets) / 1048576.0);
    if (out[0] != out[1] || out[0] != out[2]) { fprintf(stderr, "the legs disagree on %s\n", p.name); return 1; }
    for (int k = 0; k < 2; ++k) dfx_nms_destroy(h[k]);
    dfx_mem_free_device(din);
    dfx_mem_free_device(dout);
    dfx_mem_free_device(danc);
    dfx_mem_free_device(dtab);
    dfx_mem_free_host(pin);
    dfx_mem_free_host(pout);
  }
  dfx_event_destroy(e0);
  dfx_event_destroy(e1);
  return 0;
}
