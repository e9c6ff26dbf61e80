// bench_attn -- times the fused int8 attention (dfx_attn_*) on MI355X through the C ABI: forced DFX_ATTN_FUSED (one launch, the
// logits and probabilities on chip) against forced DFX_ATTN_CHAIN (dfx_bmm, dfx_head's softmax, dfx_bmm on their own auto
// paths, L and P through the handle's scratch) in ONE process on the same buffers, the legs alternating; s8 Q, K, V and O
// over head-sliced {bs, T, heads * d} tensors, the context written back interleaved:
//   ViT-B            bs 8 and 64, heads 12, T 197, d 64
//   Swin stage       192 windows (64 x 3 heads), T 49, d 32
//   DETR encoder     bs 2, heads 8, T 850, d 32
//   non-local block  bs 1 and 4, one head, T 4096, d = dv = 256
// bench_bmm's protocol: device-resident, back-to-back submits between two events; a timed window holds at least -iter
// submits and at least -window_us (default 3000) of work; the median of -rounds rounds per leg with the fastest and the
// slowest round next to it.  The submits rotate over enough buffer sets to exceed -rotate_mb (default 768: three times the 256
// MiB Infinity Cache); -rotate_mb 0 times one set over and over (warm caches).  Next to each time: the floor, Q, K, V and O read
// or written once at the 8 TB/s HBM peak, and the strips (workgroups of the fused kernel) of the point.  The results of the two
// legs are compared byte for byte.
//   bench_attn [-iter 20] [-burning_iter 3] [-rounds 5] [-window_us 3000] [-rotate_mb 768] [-only <substring>]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "attn_host.h"

static void check(int rc, const char *what) {
  if (rc != DFX_OK) { fprintf(stderr, "%s failed (%d): %s\n", what, rc, dfx_last_error()); exit(1); }
}

int main(int argc, char **argv) {
  Flags f(argc, argv);
  const int burn = f.geti("burning_iter", 3), iters = f.geti("iter", 20), rounds = f.geti("rounds", 5);
  const double window_us = f.geti("window_us", 3000);
  const std::string only = f.gets("only", "");
  const size_t rotate = (size_t)f.geti("rotate_mb", 768) << 20;
  const struct { const char *n; int bs, heads, t, d; } nets[] = {{"ViT-B bs8", 8, 12, 197, 64}, {"ViT-B bs64", 64, 12, 197, 64},
                                                                 {"Swin 64x3 windows", 64, 3, 49, 32}, {"DETR bs2", 2, 8, 850, 32},
                                                                 {"non-local bs1", 1, 1, 4096, 256}, {"non-local bs4", 4, 1, 4096, 256}};
  printf("bench_attn: at least %d timed submits and %.0f us per window after %d warm-up submits, median (min .. max) of %d rounds, legs "
         "alternating; buffers in rotation: %zu MiB%s\n", iters, window_us, burn, rounds, rotate >> 20, rotate ? "" : " (one set: warm caches)");
  printf("%-20s %-6s %10s %21s %6s %9s %8s %8s  %s\n", "point", "leg", "us", "(min .. max)", "n", "floor us", "TOP/s", "TB/s", "kernel name, grid, LDS");
  dfx_event_t e0, e1;
  check(dfx_event_create(&e0), "event create");
  check(dfx_event_create(&e1), "event create");
  const char *leg_name[2] = {"fused", "chain"};
  for (const auto &n : nets) {
    const std::string name = n.n;
    if (!only.empty() && name.find(only) == std::string::npos) continue;
    const AttnShape s = attn_heads(n.bs, n.heads, n.t, n.d, DFX_S8, DFX_S8);
    const size_t qb = (size_t)s.q_elems(), kb = (size_t)s.k_elems(), vb = (size_t)s.v_elems(), ob = (size_t)s.o_elems() * attn_esize(s.dst_dt);
    const size_t set = qb + kb + vb + ob;
    const size_t nsets = std::max<size_t>(1, std::min<size_t>(4096, (rotate + set - 1) / set));
    auto step = [](size_t b) { return (b + 255) / 256 * 256; };
    std::vector<unsigned char> hq(qb), hk(kb), hv(vb), hz(ob, 0);
    attn_fill(hq, 7);
    attn_fill(hk, 11);
    attn_fill(hv, 13);
    void *dq = nullptr, *dk = nullptr, *dv = nullptr, *dout = nullptr;
    check(dfx_mem_alloc_device(&dq, step(qb) * nsets), "device alloc");
    check(dfx_mem_alloc_device(&dk, step(kb) * nsets), "device alloc");
    check(dfx_mem_alloc_device(&dv, step(vb) * nsets), "device alloc");
    check(dfx_mem_alloc_device(&dout, step(ob) * nsets), "device alloc");
    for (size_t k = 0; k < nsets; ++k) {
      check(dfx_memcpy_h2d((char *)dq + k * step(qb), hq.data(), qb, nullptr), "H2D");
      check(dfx_memcpy_h2d((char *)dk + k * step(kb), hk.data(), kb, nullptr), "H2D");
      check(dfx_memcpy_h2d((char *)dv + k * step(vb), hv.data(), vb, nullptr), "H2D");
      check(dfx_memcpy_h2d((char *)dout + k * step(ob), hz.data(), ob, nullptr), "H2D");
    }
    check(dfx_stream_sync(nullptr), "sync");
    const float logit_scale = 40.0f / (74.0f * 74.0f * std::sqrt((float)s.d)), out_scale = 1.0f / 256.0f;
    std::vector<uint32_t> table(256);
    attn_softmax_table(table.data(), 0.0625, s.tk);
    dfx_attn_t *h[2] = {nullptr, nullptr};
    dfx_attn_info info[2];
    for (int k = 0; k < 2; ++k) {
      const dfx_attn_desc d = s.desc(1, k == 0 ? DFX_ATTN_FUSED : DFX_ATTN_CHAIN);
      check(dfx_attn_create(&d, &h[k]), "attn create");
      check(dfx_attn_set_table(h[k], table.data()), "set_table");
      check(dfx_attn_set_scales(h[k], logit_scale, &out_scale), "set_scales");
      check(dfx_attn_query(h[k], &info[k]), "query");
    }
    size_t turn = 0;
    auto launch = [&](int k) {
      const size_t t = turn++ % nsets;
      check(dfx_attn_submit(h[k], (char *)dq + t * step(qb), (char *)dk + t * step(kb), (char *)dv + t * step(vb), (char *)dout + t * step(ob), nullptr),
            "attn submit");
    };
    auto timed = [&](int k, int cnt) {
      check(dfx_event_record(e0, nullptr), "record");
      for (int i = 0; i < cnt; ++i) launch(k);
      check(dfx_event_record(e1, nullptr), "record");
      float ms = 0;
      check(dfx_event_elapsed_ms(e0, e1, &ms), "elapsed");
      return (double)ms * 1000.0 / cnt;
    };
    std::vector<double> us[2];
    std::vector<unsigned char> out[2];
    int per[2] = {iters, iters};  // submits per timed window
    for (int r = 0; r < rounds; ++r)
      for (int k = 0; k < 2; ++k) {
        if (r == 0) {
          (void)timed(k, 1);  // also the first warm-up submit
          out[k].resize(ob);
          check(dfx_memcpy_d2h(out[k].data(), (char *)dout + ((turn - 1) % nsets) * step(ob), ob, nullptr), "D2H");
          check(dfx_stream_sync(nullptr), "sync");
          const double probe = timed(k, iters);  // sizes the window; not counted
          per[k] = std::max(iters, (int)std::min(100000.0, std::ceil(window_us / std::max(probe, 0.1))));
        }
        for (int i = 0; i < burn; ++i) launch(k);
        us[k].push_back(timed(k, per[k]));
      }
    double med[2] = {0, 0};
    const double floor_us = (double)info[0].algorithmic_bytes / 8.0e6;  // 8 TB/s
    for (int k = 0; k < 2; ++k) {
      std::sort(us[k].begin(), us[k].end());
      med[k] = us[k][us[k].size() / 2];
      printf("%-20s %-6s %10.2f (%8.2f .. %8.2f) %6d %9.2f %8.2f %8.3f  %s, grid %d, lds %d\n", name.c_str(), leg_name[k], med[k], us[k].front(),
             us[k].back(), per[k], floor_us, (double)info[k].algorithmic_ops / med[k] / 1e6, (double)info[k].algorithmic_bytes / med[k] / 1e6,
             info[k].kernel_name, info[k].grid, info[k].lds_bytes);
    }
    const long long strips = (long long)s.batch0 * s.batch1 * ((s.tq + 31) / 32);
    printf("%-20s fused time / chain time: %.3f; spread of the rounds: fused %.1f %%, chain %.1f %%; tq %d tk %d d %d dv %d, %d matrices, %lld strips; "
           "%zu buffer sets\n", "", med[0] / med[1], 100.0 * (us[0].back() - us[0].front()) / med[0], 100.0 * (us[1].back() - us[1].front()) / med[1],
           s.tq, s.tk, s.d, s.dv, s.batch0 * s.batch1, strips, nsets);
    if (out[0] != out[1]) { fprintf(stderr, "the fused kernel and the chain disagree on %s\n", name.c_str()); return 1; }
    for (int k = 0; k < 2; ++k) dfx_attn_destroy(h[k]);
    dfx_mem_free_device(dq);
    dfx_mem_free_device(dk);
    dfx_mem_free_device(dv);
    dfx_mem_free_device(dout);
  }
  dfx_event_destroy(e0);
  dfx_event_destroy(e1);
  return 0;
}
