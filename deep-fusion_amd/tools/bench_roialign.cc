// bench_roialign -- times RoIAlign (dfx_roialign_*) on MI355X through the C ABI:
//   box head   Faster R-CNN-FPN: 4 levels of 200x304, 100x152, 50x76, 25x38 x 256 (an 800 x 1216 image at strides 4 .. 32),
//              n 1000 RoIs per image, 7x7 bins, S 2, levels by torchvision's LevelMapper; u8 at bs 1 and 8, f32 at bs 1 and 8
//   mask head  the same maps, n 100, 14x14
//   c4 head    1 level 50x76x1024 u8 (stride 16), n 300, 14x14
// The boxes come from the seeded generator of roialign_host.h (sides log-uniform from 16 to 600 pixels), dense, no count.
// Legs, alternating at every point: the tile kernel and the generic kernel, forced, device-resident, back-to-back submits
// between two events.  Median of -rounds rounds per leg.  The submits rotate over enough sets of (levels, boxes, dst) to
// exceed -rotate_mb (default 768: three times the 256 MiB Infinity Cache): the line of a point says how many.  dst of the
// two legs is compared byte for byte.  Per point: us per leg, the ratio, GB/s of dst written, and the distance to the floor
// max(dst bytes / -write_gbs, corner bytes / -l2_gbs) with the bound that binds (defaults 5900 GB/s of streamed stores and
// 17000 GB/s of L2 gather reads).
//   bench_roialign [-iter 20] [-burning_iter 3] [-rounds 3] [-rotate_mb 768] [-write_gbs 5900] [-l2_gbs 17000]
//                  [-only <substring of a point's name>]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "cli_flags.h"
#include "dfx.h"
#include "roialign_host.h"

struct Point {
  const char *name;
  int bs, n, levels, c, dt, ph, pw, S;
};

static void check(int rc, const char *what) {
  if (rc != DFX_OK) { fprintf(stderr, "%s failed (%d): %s\n", what, rc, dfx_last_error()); exit(1); }
}

int main(int argc, char **argv) {
  Flags f(argc, argv);
  const int burn = f.geti("burning_iter", 3), iters = f.geti("iter", 20), rounds = f.geti("rounds", 3);
  const std::string only = f.gets("only", "");
  const size_t rotate = (size_t)f.geti("rotate_mb", 768) << 20;
  const double write_tbs = f.geti("write_gbs", 5900) / 1000.0, l2_tbs = f.geti("l2_gbs", 17000) / 1000.0;
  const Point points[] = {
      {"box head fpn u8 1x1000 7x7", 1, 1000, 4, 256, DFX_U8, 7, 7, 2},   {"box head fpn u8 8x1000 7x7", 8, 1000, 4, 256, DFX_U8, 7, 7, 2},
      {"mask head fpn u8 1x100 14x14", 1, 100, 4, 256, DFX_U8, 14, 14, 2}, {"mask head fpn u8 8x100 14x14", 8, 100, 4, 256, DFX_U8, 14, 14, 2},
      {"c4 head u8 1x300 14x14 c1024", 1, 300, 1, 1024, DFX_U8, 14, 14, 2}, {"c4 head u8 8x300 14x14 c1024", 8, 300, 1, 1024, DFX_U8, 14, 14, 2},
      {"box head fpn f32 1x1000 7x7", 1, 1000, 4, 256, DFX_F32, 7, 7, 2},  {"box head fpn f32 8x1000 7x7", 8, 1000, 4, 256, DFX_F32, 7, 7, 2},
  };
  printf("bench_roialign: %d timed submits per round after %d warm-up submits, median of %d rounds, legs alternating; buffers in rotation: up to %zu MiB; "
         "floor: %.1f TB/s of stores, %.1f TB/s of L2 reads\n", iters, burn, rounds, rotate >> 20, write_tbs, l2_tbs);
  printf("%-30s %-8s %10s  %s\n", "point", "leg", "us", "kernel name / plan");
  dfx_event_t e0, e1;
  check(dfx_event_create(&e0), "event create");
  check(dfx_event_create(&e1), "event create");
  const char *leg_name[2] = {"tile", "generic"};
  for (const Point &p : points) {
    if (!only.empty() && !strstr(p.name, only.c_str())) continue;
    const size_t es = p.dt == DFX_F32 ? 4 : 1, R = (size_t)p.bs * p.n;
    dfx_roialign_desc d;
    memset(&d, 0, sizeof(d));
    d.bs = p.bs; d.n = p.n; d.mode = DFX_ROI_BATCHED; d.levels = p.levels; d.c = p.c; d.dt = p.dt; d.ph = p.ph; d.pw = p.pw; d.sampling_ratio = p.S;
    d.aligned = 0; d.dst_ld = p.c;
    const int first_stride = p.levels == 1 ? 16 : 4;
    size_t off[5] = {0, 0, 0, 0, 0};
    auto step = [](size_t b) { return (b + 255) / 256 * 256; };
    for (int l = 0; l < p.levels; ++l) {
      const int st = first_stride << l;
      d.h[l] = 800 / st; d.w[l] = 1216 / st; d.src_ld[l] = p.c; d.spatial_scale[l] = 1.0f / (float)st;
      off[l + 1] = off[l] + step((size_t)p.bs * d.h[l] * d.w[l] * p.c * es);
    }
    if (p.levels > 1) roi_level_thresholds(2, 1 + p.levels, d.level_area_thr);
    const size_t o_box = off[p.levels], in_bytes = o_box + step(R * 16), out_bytes = step(R * p.ph * p.pw * p.c * es);
    const size_t nsets = std::max<size_t>(1, std::min<size_t>(64, (rotate + in_bytes + out_bytes - 1) / (in_bytes + out_bytes)));
    RoiRng g(1000 + (uint64_t)(&p - points));
    std::vector<uint8_t> hin(in_bytes, 0);
    if (p.dt == DFX_F32) {
      float *v = (float *)hin.data();
      for (size_t i = 0; i < o_box / 4; ++i) v[i] = g.uniform(-4.f, 4.f);
    } else {
      for (size_t i = 0; i < o_box; ++i) hin[i] = (uint8_t)(g.next() & 0xff);
    }
    roi_random_boxes(g, (int)R, 1216.f, 800.f, 16.f, 600.f, (float *)(hin.data() + o_box));
    void *din = nullptr, *dout = nullptr;
    check(dfx_mem_alloc_device(&din, in_bytes * nsets), "device alloc");
    check(dfx_mem_alloc_device(&dout, out_bytes * nsets), "device alloc");
    for (size_t k = 0; k < nsets; ++k) check(dfx_memcpy_h2d((char *)din + k * in_bytes, hin.data(), in_bytes, nullptr), "H2D");
    check(dfx_stream_sync(nullptr), "sync");
    dfx_roialign_t *h[2] = {nullptr, nullptr};
    dfx_roialign_info info[2];
    for (int k = 0; k < 2; ++k) {
      d.force_path = k;
      check(dfx_roialign_create(&d, &h[k]), "roialign create");
      check(dfx_roialign_query(h[k], &info[k]), "query");
    }
    size_t turn = 0;
    auto launch = [&](int k) {
      const size_t s = turn++ % nsets;
      dfx_roialign_io io;
      memset(&io, 0, sizeof(io));
      char *in = (char *)din + s * in_bytes;
      for (int l = 0; l < p.levels; ++l) io.src[l] = in + off[l];
      io.boxes = in + o_box;
      io.dst = (char *)dout + s * out_bytes;
      check(dfx_roialign_submit(h[k], &io, nullptr), "roialign submit");
    };
    std::vector<double> us[2];
    std::vector<uint8_t> out[2];
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
          out[k].resize(out_bytes);
          check(dfx_memcpy_d2h(out[k].data(), (char *)dout + ((turn - 1) % nsets) * out_bytes, out_bytes, nullptr), "D2H");
          check(dfx_stream_sync(nullptr), "sync");
        }
      }
    double med[2];
    for (int k = 0; k < 2; ++k) {
      std::sort(us[k].begin(), us[k].end());
      med[k] = us[k][us[k].size() / 2];
      printf("%-30s %-8s %10.2f  %s, grid %d x %d, lds %d, rows per group %d\n", p.name, leg_name[k], med[k], info[k].kernel_name, info[k].grid, info[k].block,
             info[k].lds_bytes, info[k].rows_per_group);
    }
    const double dst_b = (double)R * p.ph * p.pw * p.c * es, corner_b = dst_b * p.S * p.S * 4;
    const double t_w = dst_b / (write_tbs * 1e6), t_l2 = corner_b / (l2_tbs * 1e6);  // us
    const double floor_us = std::max(t_w, t_l2);
    size_t nonzero = 0;
    for (uint8_t v : out[1]) nonzero += v != 0;
    printf("%-30s tile / generic: %.3f; dst %.1f MB at %.0f GB/s (tile) %.0f GB/s (generic); floor %.2f us (%s binds: stores %.2f us, corner reads %.2f us): "
           "tile at %.2fx, generic at %.2fx the floor; %zu sets, %.0f MiB in rotation; %.0f %% of dst non-zero\n",
           "", med[0] / med[1], dst_b / 1e6, dst_b / med[0] / 1e3, dst_b / med[1] / 1e3, floor_us, t_w >= t_l2 ? "the store stream" : "the L2 corner reads", t_w, t_l2,
           med[0] / floor_us, med[1] / floor_us, nsets, (double)((in_bytes + out_bytes) * nsets) / 1048576.0, 100.0 * (double)nonzero / (double)out[1].size());
    if (out[0] != out[1]) { fprintf(stderr, "the legs disagree on %s\n", p.name); return 1; }
    for (int k = 0; k < 2; ++k) dfx_roialign_destroy(h[k]);
    dfx_mem_free_device(din);
    dfx_mem_free_device(dout);
  }
  dfx_event_destroy(e0);
  dfx_event_destroy(e1);
  return 0;
}
