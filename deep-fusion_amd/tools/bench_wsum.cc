// bench_wsum -- times the scaled element-wise sum (dfx_wsum_*) on MI355X through the C ABI, on the joins of the networks
// the library names, at N = 1 and 128 (16 for the FPN point).  Legs, alternating at every point:
//   (a) the op on the vec kernel    (b) the op on the generic kernel
//   (c) what a caller had to run without the op, as the sum of its launches: dfx_eltwise alone where the branches share one
//       scale and dtype, else one dfx_reorder per branch into the common scale followed by dfx_eltwise (that rounds twice:
//       its bytes are not compared); no leg (c) where no older op expresses the join (a table)
// Device-resident, back-to-back submits between two events, the median of -rounds rounds per leg; TB/s of
// algorithmic_bytes (all inputs + dst).  The submits rotate over enough buffer sets to exceed -rotate_mb (default 768: three
// times the 256 MiB Infinity Cache); -rotate_mb 0 times one set over and over (warm caches).  The results of (a) and (b) are
// compared byte for byte.
//   bench_wsum [-iter 50] [-burning_iter 5] [-rounds 3] [-rotate_mb 768] [-only <substring of a point's name>]
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
  int hw, c;
  int n;
  int src_dt[2];
  int dst_dt;
  bool per_channel, relu, table, equal_scale;
  int batches[2];
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
  const Point points[] = {
      {"res2 shortcut 56x56x256 u8+u8 relu", 56, 256, 2, {DFX_U8, DFX_U8}, DFX_U8, false, true, false, true, {1, 128}},
      {"res2 shortcut 56x56x256 u8+s32 relu", 56, 256, 2, {DFX_U8, DFX_S32}, DFX_U8, false, true, false, false, {1, 128}},
      {"mobilenetv2 14x14x96 s8+s8", 14, 96, 2, {DFX_S8, DFX_S8}, DFX_S8, false, false, false, false, {1, 128}},
      {"fpn 64x64x256 u8+u8 per-channel", 64, 256, 2, {DFX_U8, DFX_U8}, DFX_U8, true, false, false, false, {1, 16}},
      {"h-swish table 112x112x32 s8->u8", 112, 32, 1, {DFX_S8, DFX_S8}, DFX_U8, false, false, true, false, {1, 128}},
  };
  printf("bench_wsum: %d timed submits per round after %d warm-up submits, median of %d rounds, legs alternating; buffers in rotation: %zu MiB%s\n",
         iters, burn, rounds, rotate >> 20, rotate ? "" : " (one set: warm caches)");
  printf("%-38s %3s %-12s %10s %8s  %s\n", "point", "N", "leg", "us", "TB/s", "kernel name / launches");
  dfx_event_t e0, e1;
  check(dfx_event_create(&e0), "event create");
  check(dfx_event_create(&e1), "event create");
  int vec_wins = 0, npoints = 0;
  for (const Point &p : points) {
    if (!only.empty() && !strstr(p.name, only.c_str())) continue;
    for (int bs : p.batches) {
      const size_t elems = (size_t)bs * p.hw * p.hw * p.c;
      size_t sbytes[2], dbytes = elems * esize(p.dst_dt), set_bytes = dbytes;
      for (int i = 0; i < p.n; ++i) set_bytes += (sbytes[i] = elems * esize(p.src_dt[i]));
      const size_t nsets = std::max<size_t>(1, std::min<size_t>(4096, (rotate + set_bytes - 1) / set_bytes));
      auto step = [](size_t b) { return (b + 255) / 256 * 256; };
      // per tensor one allocation of nsets copies, each 256-byte aligned; tmp: the reordered branches of leg (c)
      void *ds[2] = {nullptr, nullptr}, *dt[2] = {nullptr, nullptr}, *dd = nullptr;
      Lcg g(7);
      for (int i = 0; i < p.n; ++i) {
        std::vector<unsigned char> hs(sbytes[i]);
        if (p.src_dt[i] == DFX_S32) {
          int32_t *v = (int32_t *)hs.data();
          for (size_t k = 0; k < elems; ++k) v[k] = (int32_t)(g.next() % 20001) - 10000;
        } else {
          for (size_t k = 0; k < hs.size(); ++k) hs[k] = (unsigned char)(g.next() & 0xff);
        }
        check(dfx_mem_alloc_device(&ds[i], step(sbytes[i]) * nsets), "device alloc");
        check(dfx_mem_alloc_device(&dt[i], step(dbytes) * nsets), "device alloc");
        for (size_t k = 0; k < nsets; ++k) check(dfx_memcpy_h2d((char *)ds[i] + k * step(sbytes[i]), hs.data(), sbytes[i], nullptr), "H2D");
      }
      check(dfx_mem_alloc_device(&dd, step(dbytes) * nsets), "device alloc");
      check(dfx_stream_sync(nullptr), "sync");

      // scales: the equal-scale point adds as dfx_eltwise does; s32 carries a conv's accumulator scale
      std::vector<float> sc[2];
      for (int i = 0; i < p.n; ++i) {
        sc[i].resize(p.per_channel ? p.c : 1);
        for (size_t k = 0; k < sc[i].size(); ++k)
          sc[i][k] = p.equal_scale ? 1.0f : (p.src_dt[i] == DFX_S32 ? 0.011f : (i ? 0.61f : 0.83f)) * (1.0f + 0.002f * (float)(k % 50));
      }
      uint8_t lut[256];
      for (int i = 0; i < 256; ++i) {  // h-swish of t / 16, in steps of 1 / 32
        const double x = (i - 128) / 16.0, y = x * std::min(std::max(x + 3.0, 0.0), 6.0) / 6.0;
        lut[i] = (uint8_t)std::min(255.0, std::max(0.0, std::nearbyint(y * 32.0)));
      }
      enum { VEC, GENERIC, OLD, NLEGS };
      const char *leg_name[NLEGS] = {"(a) vec", "(b) generic", "(c) before"};
      dfx_wsum_t *ws[2] = {nullptr, nullptr};
      dfx_wsum_info info[2];
      for (int k = 0; k < 2; ++k) {
        dfx_wsum_desc d;
        memset(&d, 0, sizeof(d));
        d.bs = bs; d.h = p.hw; d.w = p.hw; d.c = p.c; d.n_inputs = p.n;
        for (int i = 0; i < p.n; ++i) { d.src_dt[i] = p.src_dt[i]; d.nscales[i] = (int)sc[i].size(); }
        d.dst_dt = p.dst_dt; d.round_mode = DFX_ROUND_NEAREST; d.post_relu = p.relu;
        d.lut_in_dt = p.table ? DFX_S8 : DFX_UNDEF;
        d.force_path = k == VEC ? DFX_WSUM_VEC : DFX_WSUM_GENERIC;
        check(dfx_wsum_create(&d, &ws[k]), "wsum create");
        const float *sp[2] = {sc[0].data(), p.n > 1 ? sc[1].data() : nullptr};
        check(dfx_wsum_set_params(ws[k], sp, nullptr, p.table ? lut : nullptr), "set_params");
        check(dfx_wsum_query(ws[k], &info[k]), "query");
      }
      // leg (c)
      const bool have_old = !p.table;
      dfx_reorder_t *ro[2] = {nullptr, nullptr};
      dfx_eltwise_t *el = nullptr;
      std::string old_name = "n/a";
      if (have_old) {
        dfx_eltwise_desc ed = {p.n, (int64_t)elems, p.dst_dt, p.relu};
        check(dfx_eltwise_create(&ed, &el), "eltwise create");
        old_name = "eltwise";
        if (!p.equal_scale) {
          for (int i = 0; i < p.n; ++i) {
            dfx_reorder_desc rd = {bs, p.hw, p.hw, p.c, p.c, DFX_FMT_NHWC, DFX_FMT_NHWC, p.src_dt[i], p.dst_dt, DFX_ROUND_NEAREST, (int)sc[i].size()};
            check(dfx_reorder_create(&rd, sc[i].data(), &ro[i]), "reorder create");
          }
          old_name = std::to_string(p.n) + " x reorder + eltwise";
        }
      }
      size_t turn = 0;
      auto launch = [&](int k) {
        const size_t s = turn++ % nsets;
        const void *src[2] = {(char *)ds[0] + s * step(sbytes[0]), p.n > 1 ? (char *)ds[1] + s * step(sbytes[1]) : nullptr};
        void *dst = (char *)dd + s * step(dbytes);
        if (k != OLD) {
          check(dfx_wsum_submit(ws[k], src, dst, nullptr), "wsum submit");
          return;
        }
        const void *in[2] = {src[0], src[1]};
        if (!p.equal_scale)
          for (int i = 0; i < p.n; ++i) {
            void *tmp = (char *)dt[i] + s * step(dbytes);
            check(dfx_reorder_submit(ro[i], src[i], tmp, nullptr), "reorder submit");
            in[i] = tmp;
          }
        check(dfx_eltwise_submit(el, in, dst, nullptr), "eltwise submit");
      };
      std::vector<double> us[NLEGS];
      std::vector<unsigned char> out[2];
      for (int r = 0; r < rounds; ++r)
        for (int k = 0; k < NLEGS; ++k) {
          if (k == OLD && !have_old) continue;
          for (int i = 0; i < burn; ++i) launch(k);
          check(dfx_event_record(e0, nullptr), "record");
          for (int i = 0; i < iters; ++i) launch(k);
          check(dfx_event_record(e1, nullptr), "record");
          float ms = 0;
          check(dfx_event_elapsed_ms(e0, e1, &ms), "elapsed");
          us[k].push_back(ms * 1000.0 / iters);
          if (r == 0 && k != OLD) {
            out[k].resize(dbytes);
            check(dfx_memcpy_d2h(out[k].data(), (char *)dd + ((turn - 1) % nsets) * step(dbytes), dbytes, nullptr), "D2H");
            check(dfx_stream_sync(nullptr), "sync");
          }
        }
      double med[NLEGS] = {0, 0, 0};
      for (int k = 0; k < NLEGS; ++k) {
        if (us[k].empty()) {
          printf("%-38s %3d %-12s %10s %8s  %s\n", p.name, bs, leg_name[k], "-", "-", "no older op expresses a table");
          continue;
        }
        std::sort(us[k].begin(), us[k].end());
        med[k] = us[k][us[k].size() / 2];
        printf("%-38s %3d %-12s %10.2f %8.3f  %s\n", p.name, bs, leg_name[k], med[k], (double)info[0].algorithmic_bytes / med[k] / 1e6,
               k == OLD ? old_name.c_str() : info[k].kernel_name);
      }
      ++npoints;
      if (med[VEC] < 0.95 * med[GENERIC]) ++vec_wins;
      printf("%-38s %3d vec / generic time %.3f", "", bs, med[VEC] / med[GENERIC]);
      if (have_old) printf("; vec / before time %.3f", med[VEC] / med[OLD]);
      printf("; grid %d, LDS %d bytes, %zu buffer sets\n", info[VEC].grid, info[VEC].lds_bytes, nsets);
      if (out[VEC] != out[GENERIC]) { fprintf(stderr, "the vec and the generic kernels disagree on %s\n", p.name); return 1; }
      for (int k = 0; k < 2; ++k) dfx_wsum_destroy(ws[k]);
      for (int i = 0; i < 2; ++i)
        if (ro[i]) dfx_reorder_destroy(ro[i]);
      if (el) dfx_eltwise_destroy(el);
      for (int i = 0; i < 2; ++i) { dfx_mem_free_device(ds[i]); dfx_mem_free_device(dt[i]); }
      dfx_mem_free_device(dd);
    }
  }
  printf("vec more than 5 %% faster than generic on %d of %d points\n", vec_wins, npoints);
  dfx_event_destroy(e0);
  dfx_event_destroy(e1);
  return 0;
}
