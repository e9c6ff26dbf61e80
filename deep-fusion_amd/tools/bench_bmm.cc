// bench_bmm -- times the batched int8 matrix product (dfx_bmm_*) on MI355X through the C ABI, both products of an attention
// block (Q.K^T: s8 x s8 -> s8 logits;  P.V: u8 x s8 -> s8 context, written back interleaved) over head-sliced tensors:
//   ViT-B            bs 8 and 64, heads 12, T 197 (ld 208), d 64
//   Swin window      G = 64 * 3, T 49 (ld 64), d 32
//   DETR encoder     bs 2, heads 8, T 850 (ld 864), d 32
//   non-local block  bs 1 and 4, one head, T 4096, d 256: logits and context
// Legs, alternating at every point: the MFMA kernel and the generic kernel, forced, and, where the point is ONE matrix in
// the NT form (batch 1: the non-local logits), dfx_fc on the same buffers with B as its weights -- what a caller had before
// this op: bs = M, K, oc = N, u8 src (the same bytes), s8 dst, dfx_fc_set_weights OUTSIDE the timed region (it packs on the
// host; with two activations a caller would pay it per frame).  A generic leg whose first submit takes more than -skip_ms
// (default 1000) is timed on that one submit only and marked.  Device-resident, back-to-back submits between two events; a
// timed window holds at least -iter submits and at least -window_us (default 3000) of work, so that small points are timed
// over hundreds of submits; the median of -rounds rounds per leg with the fastest and the slowest round next to it; TOP/s of
// algorithmic_ops and TB/s of algorithmic_bytes, and those as shares of the 4.6 POP/s dense int8 matrix peak and of the 8
// TB/s HBM peak.  The submits rotate over enough buffer sets to exceed -rotate_mb (default 768: three times the 256 MiB
// Infinity Cache); -rotate_mb 0 times one set over and over (warm caches).  The results of the two bmm legs are compared
// byte for byte.
// BIASED LEG (dfx_bmm_set_bias): every point is also timed on the forced MFMA kernel with a logit bias, in the same rounds on
// the same buffers: the Swin point with one {M, N} table per (window, head) (period0 = 64, period1 = 3), every other point
// with one row per image (period0 = bs, period1 = 1, ld = 0: a key-padding row at Q.K^T, its last tenth masked).  Finite
// entries are +-32 output steps, masked entries the finite value of dfa.attention_bias (the fast route stays proved).  Its
// result is compared byte for byte with ONE submit of the biased generic kernel and must differ from the unbiased result.
// -bias 0 leaves the leg out, as before the bias existed.
//   bench_bmm [-iter 20] [-bias 1] [-burning_iter 3] [-rounds 5] [-window_us 3000] [-rotate_mb 768] [-skip_ms 1000] [-only <substring>]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "bmm_host.h"

struct Point {
  std::string name;
  BmmShape s;
};

static void check(int rc, const char *what) {
  if (rc != DFX_OK) { fprintf(stderr, "%s failed (%d): %s\n", what, rc, dfx_last_error()); exit(1); }
}

int main(int argc, char **argv) {
  Flags f(argc, argv);
  const int burn = f.geti("burning_iter", 3), iters = f.geti("iter", 20), rounds = f.geti("rounds", 5);
  const double skip_ms = f.geti("skip_ms", 1000), window_us = f.geti("window_us", 3000);
  const std::string only = f.gets("only", "");
  const size_t rotate = (size_t)f.geti("rotate_mb", 768) << 20;
  const bool biased = f.geti("bias", 1) != 0;
  std::vector<Point> points;
  const struct { const char *n; int bs, heads, t, d; } nets[] = {{"ViT-B bs8", 8, 12, 197, 64}, {"ViT-B bs64", 64, 12, 197, 64},
                                                                 {"Swin 64x3 windows", 64, 3, 49, 32}, {"DETR bs2", 2, 8, 850, 32},
                                                                 {"non-local bs1", 1, 1, 4096, 256}, {"non-local bs4", 4, 1, 4096, 256}};
  for (const auto &n : nets)
    for (int pv = 0; pv < 2; ++pv)
      points.push_back({std::string(n.n) + (pv ? " P.V" : " Q.K^T"), bmm_attention(n.bs, n.heads, n.t, n.d, pv, pv ? DFX_U8 : DFX_S8, DFX_S8)});
  printf("bench_bmm: at least %d timed submits and %.0f us per window after %d warm-up submits, median (min .. max) of %d rounds, legs alternating; "
         "buffers in rotation: %zu MiB%s\n", iters, window_us, burn, rounds, rotate >> 20, rotate ? "" : " (one set: warm caches)");
  printf("%-26s %-8s %10s %21s %6s %8s %7s %8s %6s  %s\n", "point", "leg", "us", "(min .. max)", "n", "TOP/s", "%4600", "TB/s", "%8.0", "kernel name, grid");
  dfx_event_t e0, e1;
  check(dfx_event_create(&e0), "event create");
  check(dfx_event_create(&e1), "event create");
  const char *leg_name[4] = {"mfma", "generic", "dfx_fc", "mfma+b"};
  for (const Point &p : points) {
    if (!only.empty() && p.name.find(only) == std::string::npos) continue;
    const BmmShape &s = p.s;
    const size_t abytes = (size_t)s.a_elems(), bbytes = (size_t)s.b_elems(), cbytes = (size_t)s.c_elems() * bmm_esize(s.dst_dt);
    const size_t set = abytes + bbytes + cbytes;
    const size_t nsets = std::max<size_t>(1, std::min<size_t>(4096, (rotate + set - 1) / set));
    auto step = [](size_t b) { return (b + 255) / 256 * 256; };
    std::vector<unsigned char> ha(abytes), hb(bbytes), hz(cbytes, 0);  // (C starts as zeros: its pad columns are compared too)
    bmm_fill(ha, 7);
    bmm_fill(hb, 11);
    void *da = nullptr, *db = nullptr, *dc = nullptr;
    check(dfx_mem_alloc_device(&da, step(abytes) * nsets), "device alloc");
    check(dfx_mem_alloc_device(&db, step(bbytes) * nsets), "device alloc");
    check(dfx_mem_alloc_device(&dc, step(cbytes) * nsets), "device alloc");
    for (size_t k = 0; k < nsets; ++k) {
      check(dfx_memcpy_h2d((char *)da + k * step(abytes), ha.data(), abytes, nullptr), "H2D");
      check(dfx_memcpy_h2d((char *)db + k * step(bbytes), hb.data(), bbytes, nullptr), "H2D");
      check(dfx_memcpy_h2d((char *)dc + k * step(cbytes), hz.data(), cbytes, nullptr), "H2D");
    }
    check(dfx_stream_sync(nullptr), "sync");
    // a scale that centres the s8 output (about 40 per standard deviation)
    const float scale = 40.0f / ((s.a_dt == DFX_U8 ? 147.0f : 74.0f) * 74.0f * std::sqrt((float)s.k));
    // handles: the two unbiased kernels, then (leg 3) the biased MFMA kernel and the biased generic kernel that checks it
    dfx_bmm_t *h[4] = {nullptr, nullptr, nullptr, nullptr};
    dfx_bmm_info info[4];
    const bool windows = s.m == 49;
    dfx_logit_bias_desc bd;
    bd.period0 = s.batch0; bd.period1 = windows ? s.batch1 : 1;
    bd.ld = windows ? s.n : 0;
    bd.s1 = windows ? (long long)s.m * s.n : 0;
    bd.s0 = windows ? bd.s1 * s.batch1 : s.n;
    const float masked = -((s.a_dt == DFX_U8 ? 255.0f : 128.0f) * 128.0f * (float)s.k + std::ceil(129.0f / scale));
    std::vector<float> bias((size_t)bd.period0 * bd.period1 * (windows ? s.m : 1) * s.n);
    {
      unsigned lcg = 12345u;
      for (size_t i = 0; i < bias.size(); ++i) {
        lcg = lcg * 1664525u + 1013904223u;
        bias[i] = ((float)(lcg >> 8) / 16777216.0f * 64.0f - 32.0f) / scale;
        const int n = (int)(i % (size_t)s.n);
        if (windows ? (lcg >> 4) % 10 == 0 : n >= s.n - s.n / 10) bias[i] = masked;
      }
    }
    for (int k = 0; k < (biased ? 4 : 2); ++k) {
      const dfx_bmm_desc d = s.desc(1, k % 2);
      check(dfx_bmm_create(&d, &h[k]), "bmm create");
      check(dfx_bmm_set_scales(h[k], &scale), "set_scales");
      if (k >= 2) check(dfx_bmm_set_bias(h[k], &bd, bias.data()), "set_bias");
      check(dfx_bmm_query(h[k], &info[k]), "query");
    }
    // leg 2: dfx_fc where the point is one NT matrix with packed rows (lda = ldb = k, ldc = n)
    dfx_fc_t *fc = nullptr;
    dfx_fc_info fc_info;
    if (s.batch0 * s.batch1 == 1 && s.trans_b && s.lda == s.k && s.ldb == s.k && s.ldc == s.n) {
      dfx_fc_desc fd;
      memset(&fd, 0, sizeof(fd));
      fd.bs = s.m; fd.ic = s.k; fd.ih = fd.iw = 1; fd.oc = s.n; fd.dst_dt = s.dst_dt; fd.bia_dt = DFX_UNDEF; fd.round_mode = DFX_ROUND_NEAREST;
      fd.nscales = 1; fd.force_path = -1;
      check(dfx_fc_create(&fd, &fc), "fc create");
      check(dfx_fc_set_weights(fc, (const int8_t *)hb.data(), nullptr, &scale), "fc set_weights");  // outside the timed region
      check(dfx_fc_query(fc, &fc_info), "fc query");
    }
    std::vector<int> legs = {0, 1};
    if (fc) legs.push_back(2);
    if (biased) legs.push_back(3);
    size_t turn = 0;
    auto launch = [&](int k) {
      const size_t t = turn++ % nsets;
      if (k == 2) check(dfx_fc_submit(fc, (char *)da + t * step(abytes), (char *)dc + t * step(cbytes), nullptr), "fc submit");
      else check(dfx_bmm_submit(h[k == 3 ? 2 : k], (char *)da + t * step(abytes), (char *)db + t * step(bbytes), (char *)dc + t * step(cbytes), nullptr), "bmm submit");
    };
    auto timed = [&](int k, int n) {
      check(dfx_event_record(e0, nullptr), "record");
      for (int i = 0; i < n; ++i) launch(k);
      check(dfx_event_record(e1, nullptr), "record");
      float ms = 0;
      check(dfx_event_elapsed_ms(e0, e1, &ms), "elapsed");
      return (double)ms * 1000.0 / n;
    };
    std::vector<double> us[4];
    std::vector<unsigned char> out[4];
    bool single[4] = {false, false, false, false};
    int per[4] = {iters, iters, iters, iters};  // submits per timed window
    for (int r = 0; r < rounds; ++r)
      for (int k : legs) {
        if (single[k]) continue;
        if (r == 0) {
          const double first = timed(k, 1);  // also the first warm-up submit
          if (first > skip_ms * 1000.0) {
            single[k] = true;
            us[k].push_back(first);
          }
          out[k].resize(cbytes);
          check(dfx_memcpy_d2h(out[k].data(), (char *)dc + ((turn - 1) % nsets) * step(cbytes), cbytes, nullptr), "D2H");
          check(dfx_stream_sync(nullptr), "sync");
          if (single[k]) continue;
          const double probe = timed(k, iters);  // sizes the window; not counted
          per[k] = std::max(iters, (int)std::min(100000.0, std::ceil(window_us / std::max(probe, 0.1))));
        }
        for (int i = 0; i < burn; ++i) launch(k);
        us[k].push_back(timed(k, per[k]));
      }
    double med[4] = {0, 0, 0, 0};
    for (int k : legs) {
      std::sort(us[k].begin(), us[k].end());
      med[k] = us[k][us[k].size() / 2];
      const dfx_bmm_info &bi = info[k == 3 ? 2 : k];
      const uint64_t ops = k == 2 ? fc_info.algorithmic_ops : bi.algorithmic_ops, bytes = k == 2 ? fc_info.algorithmic_bytes : bi.algorithmic_bytes;
      const double tops = (double)ops / med[k] / 1e6, tbs = (double)bytes / med[k] / 1e6;
      printf("%-26s %-8s %10.2f (%8.2f .. %8.2f) %6d %8.2f %7.2f %8.3f %6.1f  %s, grid %d%s\n", p.name.c_str(), leg_name[k], med[k], us[k].front(),
             us[k].back(), single[k] ? 1 : per[k], tops, 100.0 * tops / 4600.0, tbs, 100.0 * tbs / 8.0, k == 2 ? fc_info.kernel_name : bi.kernel_name,
             k == 2 ? fc_info.grid : bi.grid, single[k] ? " (one submit: beyond -skip_ms)" : "");
    }
    printf("%-26s mfma time / generic time: %.3f", "", med[0] / med[1]);
    if (fc) printf("; mfma time / dfx_fc time: %.3f (set_weights not timed)", med[0] / med[2]);
    printf("; m %d n %d k %d, %d matrices; %zu buffer sets\n", s.m, s.n, s.k, s.batch0 * s.batch1, nsets);
    if (out[0] != out[1]) { fprintf(stderr, "the mfma and the generic kernels disagree on %s\n", p.name.c_str()); return 1; }
    if (biased) {
      printf("%-26s biased mfma time / mfma time: %.3f; spread of the rounds: mfma %.1f %%, mfma+b %.1f %%; %d x %d tables of %s, %.1f KiB\n", "", med[3] / med[0],
             100.0 * (us[0].back() - us[0].front()) / med[0], 100.0 * (us[3].back() - us[3].front()) / med[3], bd.period0, bd.period1,
             windows ? "{m, n}" : "one row", (double)bias.size() * 4 / 1024.0);
      // one submit of the biased generic kernel into set 0: the biased MFMA kernel's bytes must be its bytes
      std::vector<unsigned char> ref(cbytes);
      check(dfx_bmm_submit(h[3], da, db, dc, nullptr), "bmm submit");
      check(dfx_memcpy_d2h(ref.data(), dc, cbytes, nullptr), "D2H");
      check(dfx_stream_sync(nullptr), "sync");
      if (out[3] != ref) { fprintf(stderr, "the biased mfma and the biased generic kernels disagree on %s\n", p.name.c_str()); return 1; }
      if (out[3] == out[0]) { fprintf(stderr, "the bias changes nothing on %s\n", p.name.c_str()); return 1; }
    }
    for (int k = 0; k < 4; ++k) dfx_bmm_destroy(h[k]);
    dfx_fc_destroy(fc);
    dfx_mem_free_device(da);
    dfx_mem_free_device(db);
    dfx_mem_free_device(dc);
  }
  dfx_event_destroy(e0);
  dfx_event_destroy(e1);
  return 0;
}
