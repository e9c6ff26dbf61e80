// bench_se -- times the squeeze-and-excitation op (dfx_se_*) on MI355X through the C ABI, on the SE blocks of
// EfficientNet-B0 and SE-ResNeXt-50 at N = 1 and 32.  Legs, alternating at every point:
//   (a) the whole op on the band kernels    (b) the whole op on the generic kernels
//   (c) DFX_SE_SQUEEZE against dfx_pool with the window of the image, on the same buffers
//   (d) DFX_SE_GATE and DFX_SE_SQUEEZE on the band kernels: with (a), the three launches' times by difference
//       (squeeze = squeeze mode less the excite kernel's short form, excite = gate - squeeze, scale = whole - gate)
// Device-resident, back-to-back submits between two events, the median of -rounds rounds per leg; TB/s of
// algorithmic_bytes (the whole op: src twice + dst).  The submits rotate over enough (src, dst) sets to exceed -rotate_mb
// (default 768: three times the 256 MiB Infinity Cache); -rotate_mb 0 times one set over and over (warm caches).  The
// results of (a) and (b), and of the two sides of (c), are compared byte for byte.
//   bench_se [-iter 100] [-burning_iter 10] [-rounds 3] [-rotate_mb 768] [-only <substring of a point's name>] [-n 1,32]
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
  int hw, c, cr;
};

static void check(int rc, const char *what) {
  if (rc != DFX_OK) { fprintf(stderr, "%s failed (%d): %s\n", what, rc, dfx_last_error()); exit(1); }
}

int main(int argc, char **argv) {
  Flags f(argc, argv);
  const int burn = f.geti("burning_iter", 10), iters = f.geti("iter", 100), rounds = f.geti("rounds", 3);
  const std::string only = f.gets("only", "");
  const size_t rotate = (size_t)f.geti("rotate_mb", 768) << 20;
  const std::vector<int> batches = Flags::split_ints(f.gets("n", "1,32"));
  const Point points[] = {
      {"effnet-b0 112x112x32 -> 8", 112, 32, 8},     {"effnet-b0 56x56x96 -> 4", 56, 96, 4},       {"effnet-b0 56x56x144 -> 6", 56, 144, 6},
      {"effnet-b0 28x28x240 -> 10", 28, 240, 10},    {"effnet-b0 14x14x480 -> 20", 14, 480, 20},   {"effnet-b0 14x14x672 -> 28", 14, 672, 28},
      {"effnet-b0 7x7x1152 -> 48", 7, 1152, 48},     {"se-resnext50 56x56x256 -> 16", 56, 256, 16}, {"se-resnext50 7x7x2048 -> 128", 7, 2048, 128},
  };
  printf("bench_se: %d timed submits per round after %d warm-up submits, median of %d rounds, legs alternating; buffers in rotation: %zu MiB%s\n",
         iters, burn, rounds, rotate >> 20, rotate ? "" : " (one set: warm caches)");
  printf("%-30s %3s %-14s %10s %8s  %s\n", "point", "N", "leg", "us", "TB/s", "kernel name");
  dfx_event_t e0, e1;
  check(dfx_event_create(&e0), "event create");
  check(dfx_event_create(&e1), "event create");
  int generic_faster = 0, npoints = 0;
  for (const Point &p : points) {
    if (!only.empty() && !strstr(p.name, only.c_str())) continue;
    for (int bs : batches) {
      const size_t sb = (size_t)bs * p.hw * p.hw * p.c, zb = (size_t)bs * p.c;
      std::vector<unsigned char> hs(sb);
      Lcg g(7);
      for (size_t i = 0; i < sb; ++i) hs[i] = (unsigned char)(g.next() & 0xff);
      std::vector<int8_t> w1((size_t)p.cr * p.c), w2((size_t)p.c * p.cr);
      for (auto &v : w1) v = (int8_t)((int)(g.next() % 255) - 127);
      for (auto &v : w2) v = (int8_t)((int)(g.next() % 255) - 127);
      uint8_t lut[256];
      for (int i = 0; i < 256; ++i) lut[i] = (uint8_t)nearbyint(255.0 / (1.0 + exp(-(double)(i - 128) / 24.0)));
      const float s1 = 96.0f / (sqrtf((float)p.c) * 64.0f * 73.0f), s2 = 48.0f / (sqrtf((float)p.cr) * 60.0f * 73.0f), so = 1.0f / 255.0f;
      // nsets copies of (src, dst, z), each 256-byte aligned inside three allocations
      const size_t sstep = (sb + 255) / 256 * 256, zstep = (zb + 255) / 256 * 256;
      const size_t nsets = std::max<size_t>(1, std::min<size_t>(4096, (rotate + 2 * sstep - 1) / (2 * sstep)));
      void *ds = nullptr, *dd = nullptr, *dz = nullptr;
      check(dfx_mem_alloc_device(&ds, sstep * nsets), "device alloc");
      check(dfx_mem_alloc_device(&dd, sstep * nsets), "device alloc");
      check(dfx_mem_alloc_device(&dz, zstep * nsets), "device alloc");
      for (size_t k = 0; k < nsets; ++k) check(dfx_memcpy_h2d((char *)ds + k * sstep, hs.data(), sb, nullptr), "H2D");
      check(dfx_stream_sync(nullptr), "sync");

      enum { WHOLE_BAND, WHOLE_GENERIC, SQUEEZE_BAND, POOL, GATE_BAND, NLEGS };
      const char *leg_name[NLEGS] = {"(a) band", "(b) generic", "(c) squeeze", "(c) dfx_pool", "(d) gate"};
      dfx_se_t *se[NLEGS] = {nullptr, nullptr, nullptr, nullptr, nullptr};
      dfx_pool_t *pool = nullptr;
      dfx_se_info info[NLEGS];
      memset(info, 0, sizeof(info));
      const int modes[NLEGS] = {DFX_SE_SCALE, DFX_SE_SCALE, DFX_SE_SQUEEZE, -1, DFX_SE_GATE};
      const int paths[NLEGS] = {DFX_SE_BAND, DFX_SE_GENERIC, DFX_SE_BAND, -1, DFX_SE_BAND};
      for (int k = 0; k < NLEGS; ++k) {
        if (k == POOL) continue;
        dfx_se_desc d = {bs, p.c, p.hw, p.hw, p.cr, modes[k], DFX_UNDEF, DFX_UNDEF, DFX_ROUND_NEAREST, 1, 1, 1, paths[k]};
        check(dfx_se_create(&d, &se[k]), "se create");
        if (modes[k] != DFX_SE_SQUEEZE) check(dfx_se_set_weights(se[k], w1.data(), nullptr, &s1, w2.data(), nullptr, &s2, lut, &so), "set_weights");
        check(dfx_se_query(se[k], &info[k]), "query");
      }
      dfx_pool_desc pd = {bs, p.c, p.hw, p.hw, 1, 1, p.hw, p.hw, 1, 1, 0, 0, DFX_U8, DFX_POOL_AVG_EXCLUDE_PADDING};
      check(dfx_pool_create(&pd, &pool), "pool create");
      size_t turn = 0;
      auto launch = [&](int k) {
        const size_t i = turn++ % nsets;
        void *src = (char *)ds + i * sstep;
        if (k == POOL) check(dfx_pool_submit(pool, src, (char *)dz + i * zstep, nullptr), "pool submit");
        else check(dfx_se_submit(se[k], src, modes[k] == DFX_SE_SCALE ? (void *)((char *)dd + i * sstep) : (void *)((char *)dz + i * zstep), nullptr), "se submit");
      };
      std::vector<double> us[NLEGS];
      std::vector<unsigned char> out[NLEGS];
      for (int r = 0; r < rounds; ++r)
        for (int k = 0; k < NLEGS; ++k) {
          // (the one-thread-per-output pool is slow on the large maps: a tenth of the submits there)
          const int it = k == POOL ? std::max(3, iters / 10) : iters, bn = k == POOL ? 2 : burn;
          for (int i = 0; i < bn; ++i) launch(k);
          check(dfx_event_record(e0, nullptr), "record");
          for (int i = 0; i < it; ++i) launch(k);
          check(dfx_event_record(e1, nullptr), "record");
          float ms = 0;
          check(dfx_event_elapsed_ms(e0, e1, &ms), "elapsed");
          us[k].push_back(ms * 1000.0 / it);
          if (r == 0) {
            const size_t i = (turn - 1) % nsets;
            const bool whole = k != POOL && modes[k] == DFX_SE_SCALE;
            out[k].resize(whole ? sb : zb);
            check(dfx_memcpy_d2h(out[k].data(), whole ? (char *)dd + i * sstep : (char *)dz + i * zstep, out[k].size(), nullptr), "D2H");
            check(dfx_stream_sync(nullptr), "sync");
          }
        }
      double med[NLEGS];
      for (int k = 0; k < NLEGS; ++k) {
        std::sort(us[k].begin(), us[k].end());
        med[k] = us[k][us[k].size() / 2];
        const double bytes = k == POOL ? (double)(sb + zb) : (double)info[k].algorithmic_bytes;
        printf("%-30s %3d %-14s %10.2f %8.3f  %s\n", p.name, bs, leg_name[k], med[k], bytes / med[k] / 1e6, k == POOL ? "pool_kernel<u8> avg" : info[k].kernel_name);
      }
      ++npoints;
      if (med[WHOLE_GENERIC] < 0.95 * med[WHOLE_BAND]) ++generic_faster;
      printf("%-30s %3d band / generic time %.3f; squeeze / dfx_pool time %.3f; by difference: excite %.2f us, scale %.2f us (%.3f TB/s of src + dst); slices %d\n",
             "", bs, med[WHOLE_BAND] / med[WHOLE_GENERIC], med[SQUEEZE_BAND] / med[POOL], med[GATE_BAND] - med[SQUEEZE_BAND],
             med[WHOLE_BAND] - med[GATE_BAND], 2.0 * (double)sb / std::max(1e-3, med[WHOLE_BAND] - med[GATE_BAND]) / 1e6, info[WHOLE_BAND].slices);
      if (out[WHOLE_BAND] != out[WHOLE_GENERIC]) { fprintf(stderr, "the band and the generic kernels disagree on %s\n", p.name); return 1; }
      if (out[SQUEEZE_BAND] != out[POOL]) { fprintf(stderr, "squeeze mode and dfx_pool disagree on %s\n", p.name); return 1; }
      for (int k = 0; k < NLEGS; ++k) dfx_se_destroy(se[k]);
      dfx_pool_destroy(pool);
      dfx_mem_free_device(ds); dfx_mem_free_device(dd); dfx_mem_free_device(dz);
    }
  }
  printf("generic more than 5 %% faster than band on %d of %d points\n", generic_faster, npoints);
  dfx_event_destroy(e0);
  dfx_event_destroy(e1);
  return 0;
}
