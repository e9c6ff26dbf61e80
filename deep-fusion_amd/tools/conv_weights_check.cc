// conv_weights_check -- host-only driver and check of csrc/conv_weights.h, everything dfx_conv_set_weights computes before it
// uploads: the weight images of every kernel family and the requant-route proofs.  No HIP: it builds with SAN=1 (ASan + UBSan)
// and runs anywhere.
//   conv_weights_check < cases.txt   one case per line, conv_plan_check's format extended by a weight recipe: the 25 integers of
//                                    dfx_conv_desc, the device's CU count, the workgroups per CU, then KEY=VALUE tuning switches
//                                    and @key=value recipe items in any order.  The desc is planned with conv_plan(), the inputs
//                                    are generated from the recipe, packed, and one line is printed: "rc=<code> <message>" for a
//                                    refusal, otherwise
//                                      routes=<stage 0>,<stage 1> roles=. block=. w0=<bytes> w1=. cst=. h0=<hash> h1=. hc=. name=<kernel>
//                                    the routes numbered as dfx_debug_conv_requant numbers them (0 exact, 1 fast, 2 magic, 3 fma,
//                                    -1 no such stage), the hashes 64-bit FNV-1a over each region's own bytes.
//                                    tests/golden/conv_weights.json holds such lines, recorded on an MI355X from the library as it
//                                    was before this code left dfx_api.hip.
//   conv_weights_check < /dev/null   the self-check: for every family and a handful of shapes every byte of each weight image is
//                                    the weight the layout comment names for its position (or 0 where it says padding), the
//                                    region sizes are what the plan sized, and the switches force the routes they promise.
//
// The recipe (<s> = 0 for conv0, 1 for the 1x1 stage; tests/conv_weights_golden.py generates the same inputs in Python).  All
// arithmetic is on unsigned 64-bit integers, wrapping:
//   mix(z):  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31   (splitmix64's finaliser)
//   rnd(seed, s, k) = mix((k + 1) * 0x9E3779B97F4A7C15 + seed * 0xD1B54A32D192ED03 + s)
//   @seed=N            default 1
//   @r<s>=R            random weights: weight k of the stage, k its index in the natural order [oc][ic][kh][kw] ([oc1][oc]),
//                      is (rnd(seed, s, k) >> 32) % (2 R + 1) - R.  Default R = 3
//   @p<s>=P @n<s>=N    instead, weights with PRESCRIBED sums: the K weights of channel c are zero but for the run
//                      127 x (P / 127), P % 127 (if not 0), -128 x (N / 128), -(N % 128) (if not 0) written from position
//                      (5 c) % K on, wrapping.  Needs ceil(P / 127) + ceil(N / 128) <= K
//   @c<s>=C            ... for channel C only, the others stay random (default -1: every channel)
//   @s<s>=BITS         the scale, as the hexadecimal bits of an f32 (default 3B800000 = 2^-8); @t<s>=BITS: the scale of odd
//                      channels where the desc has per-channel scales (default: the same)
//   @b<s>=B            every channel's bias, an integer converted to the desc's bias dtype (default 0);
//   @f<s>=BITS         an f32 added to it where that dtype is f32 (a non-integer bias)
//   @inputs=1          print "inputs=<hash>" of the generated inputs instead of packing them (see print_inputs)
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../csrc/conv_weights.h"

using namespace dfx;

static int g_bad = 0;
static std::string g_case;
#define EXPECT(cond)                                                                                        \
  do {                                                                                                      \
    if (!(cond)) {                                                                                          \
      if (++g_bad <= 20) printf("conv_weights_check: line %d: %s [%s]\n", __LINE__, #cond, g_case.c_str()); \
    }                                                                                                       \
  } while (0)

static std::vector<std::pair<std::string, std::string> > g_tuning, g_recipe;
static int g_per_cu = 1;
static const char *find(const std::vector<std::pair<std::string, std::string> > &kv, const char *key) {
  for (const auto &e : kv)
    if (e.first == key) return e.second.c_str();
  return nullptr;
}
static const char *tune_of(const char *key) { return find(g_tuning, key); }
static long long recipe_int(const std::string &key, long long dflt) {
  const char *v = find(g_recipe, key.c_str());
  return v ? strtoll(v, nullptr, 10) : dflt;
}
static float recipe_f32(const std::string &key, uint32_t dflt_bits) {
  const char *v = find(g_recipe, key.c_str());
  const uint32_t bits = v ? (uint32_t)strtoul(v, nullptr, 16) : dflt_bits;
  float f;
  memcpy(&f, &bits, 4);
  return f;
}

static int plan(const dfx_conv_desc &d, int ncu, ConvPlan *p, const char **why) {
  memset(p, 0, sizeof(*p));
  const int rc = conv_validate(d, why);
  if (rc) return rc;
  ConvEnv env;
  env.ncu = ncu;
  env.tune = tune_of;
  env.wg_per_cu = [](void *, const ConvPlan &) { return g_per_cu; };
  env.ctx = nullptr;
  return conv_plan(d, env, p, why);
}

// ---- the generator
static uint64_t mix(uint64_t z) {
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static uint64_t rnd(uint64_t seed, uint64_t s, uint64_t k) { return mix((k + 1) * 0x9E3779B97F4A7C15ull + seed * 0xD1B54A32D192ED03ull + s); }

struct Inputs {
  std::vector<int8_t> nat0, nat1;  // natural order [oc][ic][kh][kw], [oc1][oc]
  std::vector<int8_t> blk0, blk1;  // the reference's blocked layout: what dfx_conv_set_weights takes
  std::vector<float> scales0, scales1;
  std::vector<unsigned char> bia0, bia1;
};

static void gen_stage(int s, int nch, int K, int nscales, int bia_dt, std::vector<int8_t> &nat, std::vector<float> &scales,
                      std::vector<unsigned char> &bia) {
  const std::string S = s ? "1" : "0";
  const uint64_t seed = (uint64_t)recipe_int("@seed", 1);
  const long long R = recipe_int("@r" + S, 3), P = recipe_int("@p" + S, -1), N = recipe_int("@n" + S, -1), only = recipe_int("@c" + S, -1);
  nat.assign((size_t)nch * K, 0);
  for (int c = 0; c < nch; ++c) {
    int8_t *w = nat.data() + (size_t)c * K;
    if ((P >= 0 || N >= 0) && (only < 0 || only == c)) {
      std::vector<int> run;
      const long long p = P < 0 ? 0 : P, n = N < 0 ? 0 : N;
      for (long long i = 0; i < p / 127; ++i) run.push_back(127);
      if (p % 127) run.push_back((int)(p % 127));
      for (long long i = 0; i < n / 128; ++i) run.push_back(-128);
      if (n % 128) run.push_back(-(int)(n % 128));
      if ((long long)run.size() > K) run.resize(K);  // (a recipe that does not fit: the golden's CPU test refuses such cases)
      for (size_t j = 0; j < run.size(); ++j) w[((size_t)5 * c + j) % K] = (int8_t)run[j];
    } else {
      for (int k = 0; k < K; ++k) w[k] = (int8_t)((long long)((rnd(seed, s, (uint64_t)c * K + k) >> 32) % (uint64_t)(2 * R + 1)) - R);
    }
  }
  const float sc = recipe_f32("@s" + S, 0x3B800000u);
  uint32_t sc_bits;
  memcpy(&sc_bits, &sc, 4);
  const float sc_odd = recipe_f32("@t" + S, sc_bits);
  scales.assign(nscales > 1 ? nch : 1, sc);
  for (size_t c = 1; c < scales.size(); c += 2) scales[c] = sc_odd;
  const long long B = recipe_int("@b" + S, 0);
  const float frac = recipe_f32("@f" + S, 0u);
  bia.assign((size_t)nch * 4 + 4, 0);
  for (int c = 0; c < nch; ++c) {
    if (bia_dt == DFX_F32) { const float v = (float)B + frac; memcpy(&bia[4 * (size_t)c], &v, 4); }
    else if (bia_dt == DFX_S32) { const int32_t v = (int32_t)B; memcpy(&bia[4 * (size_t)c], &v, 4); }
    else if (bia_dt == DFX_S8 || bia_dt == DFX_U8) bia[c] = (unsigned char)(B & 0xff);
  }
}

static void generate(const dfx_conv_desc &d, Inputs *in) {
  const int ntap = d.kh * d.kw;
  gen_stage(0, d.oc, d.ic * ntap, d.conv0_nscales, d.bia0_dt, in->nat0, in->scales0, in->bia0);
  in->blk0.assign(in->nat0.size(), 0);
  for (int o = 0; o < d.oc; ++o)
    for (int i = 0; i < d.ic; ++i)
      for (int t = 0; t < ntap; ++t)
        in->blk0[blocked_offset(o, i, t / d.kw, t % d.kw, d.ic, d.kh, d.kw)] = in->nat0[((size_t)o * d.ic + i) * ntap + t];
  if (!d.oc1x1) return;
  gen_stage(1, d.oc1x1, d.oc, d.conv1_nscales, d.bia1_dt, in->nat1, in->scales1, in->bia1);
  in->blk1.assign(in->nat1.size(), 0);
  for (int o = 0; o < d.oc1x1; ++o)
    for (int i = 0; i < d.oc; ++i) in->blk1[blocked_offset(o, i, 0, 0, d.oc, 1, 1)] = in->nat1[(size_t)o * d.oc + i];
}

static int pack(const dfx_conv_desc &d, const ConvPlan &p, const Inputs &in, ConvWeights *w, const char **why) {
  const bool fused = d.oc1x1 > 0;
  return conv_pack_weights(d, p, tune_of, in.blk0.data(), d.bia0_dt == DFX_UNDEF ? nullptr : in.bia0.data(), in.scales0.data(),
                           fused ? in.blk1.data() : nullptr, fused && d.bia1_dt != DFX_UNDEF ? in.bia1.data() : nullptr,
                           fused ? in.scales1.data() : nullptr, w, why);
}

static bool resident(const ConvPlan &p) { return p.variant == DFX_VARIANT_MFMA_FUSED || p.variant == DFX_VARIANT_MFMA_CONV; }

// the routes as dfx_debug_conv_requant numbers them
static void routes_of(const dfx_conv_desc &d, const ConvPlan &p, const ConvWeights &w, int out[2]) {
  const bool fused = d.oc1x1 > 0;
  if (p.variant == DFX_VARIANT_MFMA_STREAM && p.direct) {
    out[0] = w.m0 ? 3 : w.fast ? 1 : 0;
    out[1] = !fused ? -1 : w.m1 ? w.m1 : w.fast ? 1 : 0;
  } else if (p.variant == DFX_VARIANT_MFMA_STREAM) {
    out[0] = w.fast ? 1 : 0;
    out[1] = fused ? out[0] : -1;
  } else if (p.variant != DFX_VARIANT_GENERIC) {
    out[0] = w.mode0;
    out[1] = fused ? w.mode1 : -1;
  } else {
    out[0] = 0;
    out[1] = fused ? 0 : -1;
  }
}

static unsigned long long fnv1a(const uint8_t *p, size_t n) {
  unsigned long long h = 0xcbf29ce484222325ull;
  for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
  return h;
}

// @inputs=1: one hash over what the recipe generated -- both blocked weight arrays, both scale arrays, both bias arrays in
// their dtype -- instead of the packed line (tests/test_conv_weights_cpu.py holds the Python generator against it)
static void print_inputs(const dfx_conv_desc &d, const Inputs &in) {
  auto bias_bytes = [](int n, int dt) { return dt == DFX_UNDEF ? (size_t)0 : (size_t)n * conv_dt_size(dt); };
  // (a position-weighted sum, which numpy can form without a loop: byte i of the concatenation adds (byte + 1) * (2 i + 1) * c)
  uint64_t h = 0, i = 0;
  auto add = [&](const void *pv, size_t n) {
    const uint8_t *p = (const uint8_t *)pv;
    for (size_t k = 0; k < n; ++k, ++i) h += (uint64_t)(p[k] + 1) * ((2 * i + 1) * 0x9E3779B97F4A7C15ull);
  };
  add(in.blk0.data(), in.blk0.size());
  add(in.blk1.data(), in.blk1.size());
  add(in.scales0.data(), in.scales0.size() * 4);
  add(in.scales1.data(), in.scales1.size() * 4);
  add(in.bia0.data(), bias_bytes(d.oc, d.bia0_dt));
  add(in.bia1.data(), d.oc1x1 ? bias_bytes(d.oc1x1, d.bia1_dt) : 0);
  printf("inputs=%016llx\n", (unsigned long long)h);
}

static void print_weights(const dfx_conv_desc &d, const ConvPlan &p, const ConvWeights &w) {
  int r[2];
  routes_of(d, p, w, r);
  printf("routes=%d,%d roles=%d block=%d w0=%zu w1=%zu cst=%zu h0=%016llx h1=%016llx hc=%016llx name=%s\n", r[0], r[1], (int)w.roles, w.block,
         w.n_w0, w.n_w1, w.n_cst, fnv1a(w.image.data(), w.n_w0), fnv1a(w.image.data() + w.off_w1, w.n_w1),
         fnv1a(w.image.data() + w.off_cst, w.n_cst), w.kernel_name);
}

// ---- the self-check: the layout comments of conv_mfma.cuh, conv_stream.cuh and conv_direct.cuh as plain index formulas over
//      the NATURAL weight arrays, written without the fragment writers
struct Natural {
  const dfx_conv_desc &d;
  const Inputs &in;
  int w0(int oc, int ic, int tap) const {
    return (oc < d.oc && ic < d.ic) ? in.nat0[((size_t)oc * d.ic + ic) * (d.kh * d.kw) + tap] : 0;
  }
  int w1(int oc1, int oc) const { return (oc1 < d.oc1x1 && oc < d.oc) ? in.nat1[(size_t)oc1 * d.oc + oc] : 0; }
  // byte b of lane of the W1 fragment (1x1 group g1, column block cc, conv0 block blk)
  int w1_frag(int G, int g1, int cc, int blk, int lane, int b) const {
    return w1(32 * G * g1 + G * (lane & 31) + cc, 32 * blk + 8 * (b >> 2) + 4 * (lane >> 5) + (b & 3));
  }
};

static void check_image(const dfx_conv_desc &d, const ConvPlan &p, const Inputs &in, const ConvWeights &w) {
  const Natural nat = {d, in};
  const bool fused = d.oc1x1 > 0;
  const int ntap = d.kh * d.kw, G = p.G;
  const int8_t *img = (const int8_t *)w.image.data();
  EXPECT(w.off_w1 >= w.n_w0 && w.off_cst >= w.off_w1 + w.n_w1 && w.image.size() >= w.off_cst + w.n_cst && w.off_w1 % 16 == 0 && w.off_cst % 16 == 0);
  size_t bad0 = 0, bad1 = 0;
  if (p.variant == DFX_VARIANT_GENERIC) {
    EXPECT(w.n_w0 == in.blk0.size() && memcmp(img, in.blk0.data(), w.n_w0) == 0);
    EXPECT(w.n_w1 == in.blk1.size() && (!fused || memcmp(img + w.off_w1, in.blk1.data(), w.n_w1) == 0));
    EXPECT(w.n_cst == (size_t)12 * (d.oc + d.oc1x1));
    return;
  }
  if (resident(p)) {
    const int ICB = p.icb, OCB = p.ocb, NCB = d.oc1x1 / 32;
    EXPECT(w.n_w0 == (size_t)OCB * 9 * ICB * 1024 && w.n_w1 == (size_t)NCB * OCB * 1024 && w.n_cst == (size_t)mfma_cst_floats(d.oc, d.oc1x1) * 4);
    // LDS: weights, constants, control block, then MFMA_NB tile slots
    EXPECT((size_t)p.lds == w.image.size() + (size_t)(p.roles_ok ? RL_CTRL_BYTES : MFMA_CTRL_BYTES) + (size_t)MFMA_NB * p.geom.tile_stride);
    for (size_t off = 0; off < w.n_w0; ++off) {  // [r][tap][c][lane][16]
      const int j = off % 16, lane = off / 16 % 64, c = off / 1024 % ICB, tap = off / 1024 / ICB % 9, r = (int)(off / 1024 / ICB / 9);
      const int oc = fused ? 32 * r + (lane & 31) : G * (lane & 31) + r;
      bad0 += img[off] != nat.w0(oc, 32 * c + 16 * (lane >> 5) + j, tap);
    }
    for (size_t off = 0; off < w.n_w1; ++off) {  // [cb][r][lane][16], cb = cg * G + cc
      const int j = off % 16, lane = off / 16 % 64, r = off / 1024 % OCB, cb = (int)(off / 1024 / OCB);
      bad1 += img[w.off_w1 + off] != nat.w1_frag(G, cb / G, cb % G, r, lane, j);
    }
  } else if (p.direct) {
    const DirectGeom &g = p.dgeom;
    EXPECT(w.n_w0 == (size_t)g.ocb * g.icb * ntap * 1024 && w.n_w1 == (size_t)g.n_g1 * g.ocb * G * 1024 && w.n_cst == (size_t)12 * 32 * (g.ocb + G * g.n_g1));
    if (p.pw) EXPECT(w.n_w0 == (size_t)p.pwgeom.off_cst && (size_t)p.pwgeom.off_stage == round16(w.n_w0 + w.n_cst) && w.n_w1 == 0);
    else EXPECT((size_t)(p.lds - g.off_cst) == round16(w.n_cst));
    for (size_t off = 0; off < w.n_w0; ++off) {  // W0d[ob][kb = icb * ntap + tap][lane][16]
      const int b = off % 16, lane = off / 16 % 64, tap = off / 1024 % ntap, icb = off / 1024 / ntap % g.icb, ob = (int)(off / 1024 / ntap / g.icb);
      bad0 += img[off] != nat.w0(32 * ob + (lane & 31), 32 * icb + 16 * (lane >> 5) + b, tap);
    }
    for (size_t off = 0; off < w.n_w1; ++off) {  // W1d[g1][blk][cc][lane][16]
      const int b = off % 16, lane = off / 16 % 64, cc = off / 1024 % G, blk = off / 1024 / G % g.ocb, g1 = (int)(off / 1024 / G / g.ocb);
      bad1 += img[w.off_w1 + off] != nat.w1_frag(G, g1, cc, blk, lane, b);
    }
  } else {
    const StreamGeom &g = p.sgeom;
    const int OCC = p.occ;
    EXPECT(w.n_w0 == (size_t)g.s0_steps * 2 * OCC * 1024 && w.n_w1 == (fused ? (size_t)g.n_g1 * g.ks2 * 2 * G * 1024 : 0) &&
           w.n_cst == (size_t)12 * 32 * (g.ocb + G * g.n_g1));
    if (fused) EXPECT((size_t)(p.lds - g.off_cst) == round16((size_t)12 * 32 * g.ocb));  // (stage 0's constants live in LDS)
    size_t off = 0;  // the kernel's walk: oc chunk, ic chunk, step = 2 k-blocks x OCC fragments
    for (int occ = 0; occ < g.n_occ; ++occ)
      for (int icc = 0; icc < g.n_icc; ++icc) {
        const int kbn = std::min(2, g.icb - 2 * icc), ns = ntap * kbn;
        for (int s2 = 0; s2 < (ns + 1) / 2; ++s2)
          for (int j = 0; j < 2; ++j)
            for (int r = 0; r < OCC; ++r)
              for (int lane = 0; lane < 64; ++lane)
                for (int b = 0; b < 16; ++b, ++off) {
                  const int s = 2 * s2 + j;
                  const int oc = fused ? 32 * (occ * OCC + r) + (lane & 31) : 32 * OCC * occ + OCC * (lane & 31) + r;
                  const int want = s >= ns ? 0 : nat.w0(oc, 64 * icc + 32 * (s % kbn) + 16 * (lane >> 5) + b, s / kbn);
                  bad0 += off >= w.n_w0 || img[off] != want;
                }
      }
    EXPECT(off == w.n_w0);
    for (size_t o1 = 0; o1 < w.n_w1; ++o1) {  // [g1][step][k-block of the step][cc][lane][16]
      const int b = o1 % 16, lane = o1 / 16 % 64, cc = o1 / 1024 % G, blk = o1 / 1024 / G % (2 * g.ks2), g1 = (int)(o1 / 1024 / G / (2 * g.ks2));
      bad1 += img[w.off_w1 + o1] != (blk >= g.ocb ? 0 : nat.w1_frag(G, g1, cc, blk, lane, b));
    }
  }
  EXPECT(bad0 == 0);
  EXPECT(bad1 == 0);
}

static dfx_conv_desc desc(int bs, int ic, int ih, int iw, int oc, int oc1, int k, int s, int pad, int dst, int fv = -1) {
  dfx_conv_desc d;
  memset(&d, 0, sizeof(d));
  d.bs = bs; d.ic = ic; d.ih = ih; d.iw = iw; d.oc = oc; d.kh = d.kw = k; d.sh = d.sw = s; d.pad_t = d.pad_l = pad;
  d.oh = (ih + 2 * pad - k) / s + 1; d.ow = (iw + 2 * pad - k) / s + 1;
  d.oc1x1 = oc1; d.dst_dt = dst; d.conv0_nscales = d.conv1_nscales = 1; d.force_variant = fv; d.fuse_pool = 0;
  d.bia0_dt = DFX_S32; d.bia1_dt = oc1 ? DFX_S32 : DFX_UNDEF;
  return d;
}

static int self_check() {
  int families[5] = {0, 0, 0, 0, 0}, packed = 0, top[2] = {0, 0};
  auto one = [&](const dfx_conv_desc &d, int per_cu, int want0, int want1) {
    char buf[200];
    snprintf(buf, sizeof(buf), "bs %d ic %d %dx%d oc %d oc1 %d k%d s%d p%d dt%d fv%d /%d +%d switches", d.bs, d.ic, d.ih, d.iw, d.oc, d.oc1x1, d.kh,
             d.sh, d.pad_t, d.dst_dt, d.force_variant, per_cu, (int)g_tuning.size());
    g_case = buf;
    g_per_cu = per_cu;
    ConvPlan p;
    const char *why = nullptr;
    EXPECT(plan(d, 256, &p, &why) == DFX_OK);
    Inputs in;
    generate(d, &in);
    ConvWeights w;
    EXPECT(pack(d, p, in, &w, &why) == DFX_OK && why[0] == 0);
    ++packed;
    families[resident(p) ? 0 : p.variant == DFX_VARIANT_GENERIC ? 4 : p.pw ? 3 : p.direct ? 2 : 1]++;
    check_image(d, p, in, w);
    int r[2];
    routes_of(d, p, w, r);
    if (want0 >= 0) EXPECT(r[0] == want0 && r[1] == (d.oc1x1 ? want1 : -1));
    top[0] = std::max(top[0], r[0]);
    top[1] = std::max(top[1], r[1]);
    EXPECT(w.block == ((resident(p) && w.roles) ? RL_THREADS : p.block));
    EXPECT(w.roles ? strstr(w.kernel_name, "conv_mfma_roles_kernel<") == w.kernel_name : strncmp(w.kernel_name, p.kernel_name, strcspn(p.kernel_name, "<")) == 0);
  };
  const int dsts[] = {DFX_U8, DFX_S32};
  for (int pass = 0; pass < 3; ++pass) {  // (the default recipe's small random weights and scale 2^-8 pass every proof)
    g_tuning.clear();
    if (pass == 1) g_tuning.push_back(std::make_pair(std::string("DFX_NO_FAST"), std::string("1")));
    if (pass == 2) g_tuning.push_back(std::make_pair(std::string("DFX_NO_MAGIC"), std::string("1")));
    const int cap = pass == 0 ? -1 : pass == 1 ? 0 : 1;
    for (int dst : dsts) {
      // resident: fused and unfused, every channel count, roles-eligible shapes
      for (int ic : {32, 64})
        for (int oc : {32, 64})
          for (int oc1 : {0, 32, 96, 128, 256}) one(desc(2, ic, 9, 7, oc, oc1, 3, 1, 1, dst), 1, cap, cap);
      // streamed: channel counts that are no multiple of 32, 64-channel chunks with one and two blocks, padding k-blocks
      one(desc(4, 16, 28, 28, 16, 32, 3, 1, 1, dst), 3, cap, cap);
      one(desc(4, 48, 28, 28, 48, 32, 3, 1, 1, dst), 2, cap, cap);
      one(desc(4, 48, 17, 19, 80, 0, 5, 1, 2, dst), 2, cap, cap);
      one(desc(2, 96, 7, 7, 64, 48, 3, 1, 1, dst), 2, cap, cap);
      one(desc(1, 128, 14, 14, 256, 0, 1, 1, 0, dst), 2, cap, cap);
      one(desc(1, 32, 28, 28, 32, 64, 3, 1, 1, dst, DFX_VARIANT_MFMA_STREAM), 3, cap, cap);
      // direct: fused with G = 4 and G = 2, oc / oc1x1 that pad their blocks, unfused; pointwise; scalar
      one(desc(1, 128, 3, 3, 128, 512, 3, 1, 1, dst), 2, cap, cap);
      one(desc(16, 96, 28, 28, 96, 96, 3, 1, 1, dst), 2, cap, cap);
      one(desc(1, 64, 5, 5, 64, 64, 5, 1, 2, dst), 3, cap, cap);
      one(desc(4, 80, 12, 10, 80, 80, 3, 1, 1, dst), 2, cap, cap);
      one(desc(32, 128, 28, 28, 128, 0, 3, 1, 1, dst), 2, cap, cap);
      one(desc(1, 256, 3, 3, 64, 0, 1, 1, 0, dst), 5, cap, cap);
      one(desc(1, 32, 9, 7, 32, 64, 3, 1, 1, dst, DFX_VARIANT_GENERIC), 1, 0, 0);
      one(desc(1, 48, 5, 5, 16, 0, 3, 1, 1, dst, DFX_VARIANT_GENERIC), 1, 0, 0);
    }
  }
  g_tuning.clear();
  for (int f = 0; f < 5; ++f) EXPECT(families[f] > 0);
  EXPECT(top[0] == 3 && top[1] == 3);  // (every route number occurs without a switch)
  if (g_bad) {
    printf("conv_weights_check: %d checks FAILED\n", g_bad);
    return 1;
  }
  printf("conv weights: %d images (resident %d, streamed %d, direct %d, pointwise %d, scalar %d): every byte is the weight its layout "
         "names, sizes are the plan's, the switches cap the routes\n", packed, families[0], families[1], families[2], families[3], families[4]);
  return 0;
}

int main() {
  static char line[8192];
  int ncases = 0;
  while (fgets(line, sizeof(line), stdin)) {
    int32_t v[27];
    int n = 0;
    char *save = nullptr;
    g_tuning.clear();
    g_recipe.clear();
    for (char *tok = strtok_r(line, " \t\r\n", &save); tok; tok = strtok_r(nullptr, " \t\r\n", &save)) {
      if (n < 27) {
        v[n++] = (int32_t)strtol(tok, nullptr, 10);
      } else if (char *eq = strchr(tok, '=')) {
        (tok[0] == '@' ? g_recipe : g_tuning).push_back(std::make_pair(std::string(tok, eq - tok), std::string(eq + 1)));
      }
    }
    if (n == 0) continue;
    ++ncases;
    if (n < 27) {
      printf("rc=-1 conv_weights_check: a case needs 25 descriptor integers, the CU count and the workgroups per CU\n");
      continue;
    }
    dfx_conv_desc d;
    static_assert(sizeof(d) == 25 * sizeof(int32_t), "dfx_conv_desc is 25 int32_t");
    memcpy(&d, v, sizeof(d));
    g_per_cu = v[26];
    ConvPlan p;
    const char *why = "";
    int rc = plan(d, v[25], &p, &why);
    ConvWeights w;
    if (!rc) {
      Inputs in;
      generate(d, &in);
      if (find(g_recipe, "@inputs")) {
        print_inputs(d, in);
        continue;
      }
      rc = pack(d, p, in, &w, &why);
    }
    if (rc) printf("rc=%d %s\n", rc, why);
    else print_weights(d, p, w);
  }
  return ncases ? 0 : self_check();
}
