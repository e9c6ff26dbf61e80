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
// BIASED LEGS (dfx_attn_set_bias): every point is also timed with a logit bias on both forced paths, the four legs alternating
// in the same rounds on the same buffers: the Swin stage with one {T, T} table per (window, head) (period0 = nW = 64, period1 =
// heads: relative-position bias plus a shifted-window mask), every other point with a key-padding row per image (period0 =
// bs, period1 = 1, ld = 0: the last tenth of the keys masked).  Finite entries are +-32 logit steps, masked entries the finite
// value of dfa.attention_bias (the fast route stays proved).  The two biased legs are compared byte for byte and must differ
// from the unbiased result.  -bias 0 times the two unbiased legs alone, as before the bias existed.  -bias_table1 1 gives the
// points that have a key-padding row ONE whole {T, T} table instead (periods 1, 1): every lane reads its own row of a table all
// matrices share, where the row layout has all lanes of a wave read the same 16 bytes.
// -t <T> (with -bs, -heads, -d) times ONE point of that shape instead of the six.
//   bench_attn [-iter 20] [-bias 1] [-bias_table1 0] [-t 0 -bs 8 -heads 12 -d 64] [-burning_iter 3] [-rounds 5] [-window_us 3000] [-rotate_mb 768] [-only <substring>]
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
  const int nleg = f.geti("bias", 1) ? 4 : 2;
  const bool table1 = f.geti("bias_table1", 0) != 0;
  const struct { const char *n; int bs, heads, t, d; } nets[] = {{"ViT-B bs8", 8, 12, 197, 64}, {"ViT-B bs64", 64, 12, 197, 64},
                                                                 {"Swin 64x3 windows", 64, 3, 49, 32}, {"DETR bs2", 2, 8, 850, 32},
                                                                 {"non-local bs1", 1, 1, 4096, 256}, {"non-local bs4", 4, 1, 4096, 256}};
  printf("bench_attn: at least %d timed submits and %.0f us per window after %d warm-up submits, median (min .. max) of %d rounds, legs "
         "alternating; buffers in rotation: %zu MiB%s\n", iters, window_us, burn, rounds, rotate >> 20, rotate ? "" : " (one set: warm caches)");
  printf("%-20s %-6s %10s %21s %6s %9s %8s %8s  %s\n", "point", "leg", "us", "(min .. max)", "n", "floor us", "TOP/s", "TB/s", "kernel name, grid, LDS");
  dfx_event_t e0, e1;
  check(dfx_event_create(&e0), "event create");
  check(dfx_event_create(&e1), "event create");
  const char *leg_name[4] = {"fused", "chain", "fused+b", "chain+b"};
  const int custom_t = f.geti("t", 0);
  for (auto n : nets) {
    if (custom_t > 0) {
      if (std::string(n.n) != nets[0].n) continue;  // (once)
      n.n = "custom"; n.bs = f.geti("bs", 8); n.heads = f.geti("heads", 12); n.t = custom_t; n.d = f.geti("d", 64);
    }
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
    // the bias of the biased legs: whole tables per (window, head) at the Swin point, a key-padding row per image elsewhere
    const bool windows = s.tq == 49;
    dfx_logit_bias_desc bd;
    bd.period0 = table1 && !windows ? 1 : s.batch0; bd.period1 = windows ? s.batch1 : 1;
    bd.ld = windows || table1 ? s.tk : 0;
    bd.s1 = windows ? (long long)s.tq * s.tk : 0;
    bd.s0 = windows ? bd.s1 * s.batch1 : s.tk;
    const float masked = -(128.0f * 128.0f * (float)s.d + std::ceil(129.0f / logit_scale));
    std::vector<float> bias((size_t)bd.period0 * bd.period1 * (bd.ld ? s.tq : 1) * s.tk);
    {
      unsigned lcg = 12345u;
      for (size_t i = 0; i < bias.size(); ++i) {
        lcg = lcg * 1664525u + 1013904223u;
        bias[i] = ((float)(lcg >> 8) / 16777216.0f * 64.0f - 32.0f) / logit_scale;
        const int n = (int)(i % (size_t)s.tk);
        if (windows ? (lcg >> 4) % 10 == 0 && n != 0 : n >= s.tk - s.tk / 10) bias[i] = masked;  // (key 0 of a window row is never masked)
      }
    }
    dfx_attn_t *h[4] = {nullptr, nullptr, nullptr, nullptr};
    dfx_attn_info info[4];
    for (int k = 0; k < nleg; ++k) {
      const dfx_attn_desc d = s.desc(1, k % 2 == 0 ? DFX_ATTN_FUSED : DFX_ATTN_CHAIN);
      check(dfx_attn_create(&d, &h[k]), "attn create");
      check(dfx_attn_set_table(h[k], table.data()), "set_table");
      check(dfx_attn_set_scales(h[k], logit_scale, &out_scale), "set_scales");
      if (k >= 2) check(dfx_attn_set_bias(h[k], &bd, bias.data()), "set_bias");
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
    std::vector<double> us[4];
    std::vector<unsigned char> out[4];
    int per[4] = {iters, iters, iters, iters};  // submits per timed window
    for (int r = 0; r < rounds; ++r)
      for (int k = 0; k < nleg; ++k) {
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
    double med[4] = {0, 0, 0, 0};
    const double floor_us = (double)info[0].algorithmic_bytes / 8.0e6;  // 8 TB/s
    for (int k = 0; k < nleg; ++k) {
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
    if (nleg == 4) {
      printf("%-20s biased: fused time / chain time: %.3f; biased / unbiased: fused %.3f, chain %.3f; spread of the rounds: fused+b %.1f %%, chain+b %.1f %%; "
             "%d x %d tables of %s, %.1f KiB\n", "", med[2] / med[3], med[2] / med[0], med[3] / med[1], 100.0 * (us[2].back() - us[2].front()) / med[2],
             100.0 * (us[3].back() - us[3].front()) / med[3], bd.period0, bd.period1, bd.ld ? "{tq, tk}" : "one key-padding row", (double)bias.size() * 4 / 1024.0);
      if (out[2] != out[3]) { fprintf(stderr, "the biased fused kernel and the biased chain disagree on %s\n", name.c_str()); return 1; }
      if (out[2] == out[0]) { fprintf(stderr, "the bias changes nothing on %s\n", name.c_str()); return 1; }
    }
    for (int k = 0; k < nleg; ++k) dfx_attn_destroy(h[k]);
    dfx_mem_free_device(dq);
    dfx_mem_free_device(dk);
    dfx_mem_free_device(dv);
    dfx_mem_free_device(dout);
  }
  dfx_event_destroy(e0);
  dfx_event_destroy(e1);
  return 0;
}
