// conv_weights.h -- host-only, plain C++: everything dfx_conv_set_weights computes before it uploads anything.  Two things:
//   * the weight images whose byte order the MFMA kernel families walk (conv_mfma.cuh / conv_mfma_roles.cuh,
//     conv_stream.cuh, conv_direct.cuh / conv_pw.cuh), built from ONE W0-fragment writer and ONE W1-fragment writer, and
//     the scalar kernel's plain copy;
//   * the proofs, from the ACTUAL weights, of which cheaper requant arithmetic still gives the reference's bytes (routes:
//     0 exact, 1 fast, 2 magic, 3 fma -- dfx_debug_conv_requant's numbering), one named predicate per proof over ONE pass
//     that sums each channel's positive and negative weights, and the constants each route reads.
// The switches DFX_NO_FAST and DFX_NO_MAGIC arrive through the ConvTune callback like the planner's.  No HIP in here, so
// that it can be built, run and diffed on its own (tools/conv_weights_check.cc, under the host sanitizers;
// tests/golden/conv_weights.json holds routes and image hashes recorded before this code left dfx_api.hip).
#pragma once

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "conv_plan.h"

namespace dfx {

// byte offset of W[o][i][kh][kw] in the reference's blocked weight layout (dfx_blocked_offset of the C ABI)
inline size_t blocked_offset(int o, int i, int kh, int kw, int I, int KH, int KW) {
  // [o/16][i/16][kh][kw][(i%16)/4][o%16][i%4], jit_conv_kernel.cc:333-338
  const size_t nb_ic = (size_t)I / 16;
  return ((((size_t)(o / 16) * nb_ic + (size_t)(i / 16)) * KH + kh) * KW + kw) * 256 +
         (size_t)((i % 16) / 4) * 64 + (size_t)(o % 16) * 4 + (size_t)(i % 4);
}

struct ConvWeights {
  // ---- the image: one host byte image [W0 | W1 | constants]; W0 starts at 0.  n_* are the regions' own sizes (a region
  //      may be followed by padding up to the next offset or the image's end)
  std::vector<uint8_t> image;
  size_t off_w1, off_cst;
  size_t n_w0, n_w1, n_cst;
  // ---- the routes, one field per value the handle stores
  int mode0, mode1, s0_uniform;  // resident kernels (MfmaGeom)
  float s0_value;
  bool roles;                    // the WEIGHTS allow the role-specialised kernel's requant modes
  int fast;                      // conv_stream.cuh (StreamGeom), conv_direct.cuh / conv_pw.cuh (DirectGeom)
  int m0, m1;                    // conv_direct.cuh / conv_pw.cuh (DirectGeom)
  // ---- what the roles decision changes (otherwise the plan's)
  char kernel_name[96];
  int block;
};

inline bool tune_on(ConvTune tune, const char *key) {
  const char *e = tune(key);
  return e && atoi(e) != 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// P / N.  Per channel, from the ACTUAL weights: P = sum of positive weights, N = -sum of negative
// ones.  With activations stored as u8 - 128 in [-128, 127] the raw MFMA accumulator lies in
// [-(128 P + 127 N), 127 P + 128 N]; comp = 128 * (P - N) turns it into the reference's s32
// accumulator, |true acc| <= 255 * max(P, N).
struct ChanPN {
  double P, N;
  double lo() const { return -(128.0 * P + 127.0 * N); }  // raw accumulator's range
  double hi() const { return 127.0 * P + 128.0 * N; }
  double comp() const { return 128.0 * (P - N); }
  double amax() const { return 255.0 * std::max(P, N); }
};

// the one pass over the weights: pn0[oc] of conv0, pn1[oc1] of the 1x1 stage (empty for an unfused op)
inline void conv_channel_pn(const dfx_conv_desc &d, const int8_t *wei, const int8_t *wei1, std::vector<ChanPN> &pn0,
                            std::vector<ChanPN> &pn1) {
  // (the blocked layout in memory order: byte k of a block of 16 output channels belongs to channel (k >> 2) & 15)
  struct Pass {
    static void run(const int8_t *w, int nch, size_t per_block, std::vector<ChanPN> &pn) {
      const ChanPN zero = {0.0, 0.0};
      pn.assign(nch, zero);
      for (int ob = 0; ob < nch / 16; ++ob)
        for (size_t k = 0; k < per_block; ++k) {
          const int v = w[ob * per_block + k];
          ChanPN &c = pn[16 * ob + ((k >> 2) & 15)];
          (v > 0 ? c.P : c.N) += std::abs(v);
        }
    }
  };
  Pass::run(wei, d.oc, (size_t)16 * d.ic * d.kh * d.kw, pn0);
  Pass::run(wei1, d.oc1x1, (size_t)16 * d.oc, pn1);
}

// ---------------------------------------------------------------------------------------------------------------------
// The proofs, one predicate each.

// Resident kernels' "fast" (magnitude only): rounding to nearest-even (the caller checks the round mode), every value
// finite and |f| < 2^31 so the x86 overflow / NaN results of vcvtps2dq cannot occur
inline bool fast_magnitude_ok(const ChanPN &c, float bias, float scale) {
  if (!std::isfinite(bias) || !std::isfinite(scale)) return false;
  return (c.amax() + std::fabs((double)bias)) * std::fabs((double)scale) * 1.0001 + 2.0 < 2147480000.0;
}

// Stream / direct kernels' "fast": one channel's precondition of the fast requant path (conv_mfma.cuh store_group<FAST>):
// amax bounds |true accumulator|; comp + bias must fold into ONE exact f32 add (bias
// integer-valued, |comp + bias| < 2^24, |acc + bias| < 2^24) and nothing may reach +-2^31.
inline bool fast_fold_ok(const ChanPN &c, float bias, float scale) {
  if (!std::isfinite(bias) || !std::isfinite(scale)) return false;
  const double amax = c.amax(), comp = c.comp(), b = bias;
  if (b != std::floor(b)) return false;
  const double lim = 16777216.0;  // 2^24
  if (std::fabs(comp + b) >= lim || amax + std::fabs(b) >= lim || std::fabs(comp) + amax >= lim) return false;
  return (amax + std::fabs(b)) * std::fabs((double)scale) * 1.0001 + 2.0 < 2147480000.0;
}

// "magic", accumulator started from bits(1.5 * 2^23) + comp + bias (stage 0 of a fused op):
// bias integer-valued and raw + comp + bias inside the binade, i.e. |.| < 2^22
inline bool magic0_ok(const ChanPN &c, float bias) {
  const double b = bias, cb = c.comp() + b;
  if (b != std::floor(b)) return false;
  return c.lo() + cb > -4194304.0 && c.hi() + cb < 4194304.0;
}

// "magic", accumulator started from the inline constant 1/(2 pi) = 0x3E22F983 (ulp 2^-26):
// raw within the mantissa's room; k = (comp + bias - 2^23 - 0x22F983) exactly representable;
// |acc + bias| < 2^24; scale * 2^26 finite
inline bool magic1_ok(const ChanPN &c, float bias, float scale) {
  const double b = bias, cb = c.comp() + b;
  if (b != std::floor(b)) return false;
  const double lo = c.lo(), hi = c.hi();
  if (lo < (double)MAGIC1_LO || hi > (double)MAGIC1_HI) return false;
  if (std::fabs(cb - 8388608.0 - (double)0x22F983) >= 16777216.0) return false;
  if (std::fabs(lo + cb) >= 16777216.0 || std::fabs(hi + cb) >= 16777216.0) return false;
  return std::isfinite(scale * 67108864.0f);
}

// "fma" (stage 0 of the role-specialised kernel, conv_mfma_roles.cuh, and of conv_direct.cuh / conv_pw.cuh): accumulator
// started from bits(2^23) + comp + bias.  t = acc + bias must stay inside (-2^23, 2^23): non-negative t then reads as the
// float 2^23 + t, negative t as 2^23 - |t|/2; fma(x, s, -2^23 s) = t * s with one rounding (2^23 s is exact)
// or something negative that the stage's ReLU + u8 saturation turn into 0 like the reference's negative
// product -- which needs s >= 0.  bias integer-valued; |acc| <= 2^24 follows (0 is a possible acc).
inline bool fma0_ok(const ChanPN &c, float bias, float scale) {
  const double b = bias, cb = c.comp() + b;
  if (b != std::floor(b) || !(scale >= 0.0f) || !std::isfinite(scale * 8388608.0f)) return false;
  return c.lo() + cb > -8388608.0 && c.hi() + cb < 8388608.0;
}

// "fma" for stage 1: (x + B) * C = fma(x, C, B * C) with one rounding when
// the addend B * C = (comp + bias - 2^23 - 0x22F983) * scale is exactly representable -- power-of-two scales
// and a few others; checked per channel in double (a 24-bit integer times a 24-bit mantissa is exact there)
inline bool fma1_exact(const ChanPN &c, float bias, float scale) {
  const double k = c.comp() + (double)bias - 8388608.0 - (double)0x22F983;
  const double prod = k * (double)scale;
  return std::isfinite(prod) && (double)(float)prod == prod;
}

// ---------------------------------------------------------------------------------------------------------------------
// Constants.  Slot A is an integer (bit copy into the f32 array), B and C are floats.
inline void put_i(void *dst, int32_t v) { memcpy(dst, &v, 4); }
inline void put_f(void *dst, float v) { memcpy(dst, &v, 4); }

// A stage whose accumulator STARTS from slot A (stage 0 of a fused resident op; stage 0 of conv_direct.cuh / conv_pw.cuh):
// route 3 "fma": bits(2^23) + comp + bias, and the fma's addend -2^23 * scale (exact) in slot B; route 2 "magic":
// bits(1.5 * 2^23) + comp + bias; otherwise the compensation alone
inline void start_consts(int route, const ChanPN &c, float bias, float scale, int32_t *A, float *B, float *C) {
  const int32_t comp = (int32_t)c.comp();
  *A = route == 3 ? MAGIC3_BITS + comp + (int32_t)bias : route == 2 ? MAGIC0_BITS + comp + (int32_t)bias : comp;  // accumulator start value
  *B = route == 3 ? -8388608.0f * scale : bias;
  *C = scale;
}

// A stage that requantises accumulator BITS which started from `acc_bits` (MAGIC1_BITS in the resident kernels, whose
// slot A brings them back to the reference's s32 accumulator; 0 in conv_direct.cuh, whose stage-1 start is the kernel's)
inline void inline_consts(int route, int32_t acc_bits, const ChanPN &c, float bias, float scale, int32_t *A, float *B, float *C) {
  const int32_t comp = (int32_t)c.comp();
  *A = comp - acc_bits;  // acc bits + A = the reference's s32 accumulator
  if (route == 3) {  // fma(x, C, B): B = (comp + bias - 2^23 - 0x22F983) * scale (proven exact), C = scale * 2^26
    *B = (float)(((double)comp + (double)bias - 8388608.0 - (double)0x22F983) * (double)scale);
    *C = scale * 67108864.0f;
  } else if (route == 2) {
    *B = (float)((double)comp + (double)bias - 8388608.0 - (double)0x22F983) * 1.4901161193847656e-08f;  // * 2^-26, exact
    *C = scale * 67108864.0f;                                                                           // * 2^26, exact
  } else {
    *B = bias;
    *C = scale;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Fragments: 1 KB each, 64 lanes x 16 bytes, zero where a channel lies past oc / ic / oc1x1.

// W0 fragment of input block `icblock` (32 channels) and tap `tap`: byte b of lane
//   = W0[oc(lane)][32 * icblock + 16 * (lane >> 5) + b][tap],   oc(lane) = oc_base + oc_step * (lane & 31)
// oc_step == 1: the natural order (A operand, row = channel); > 1: the store stage's channel permutation (B operand)
inline void w0_fragment(uint8_t *dst, const dfx_conv_desc &d, const int8_t *wei, int oc_base, int oc_step, int icblock, int tap) {
  const int kh = tap / d.kw, kw = tap % d.kw;
  for (int lane = 0; lane < 64; ++lane) {
    const int oc = oc_base + oc_step * (lane & 31), ic0 = 32 * icblock + 16 * (lane >> 5);
    if (oc >= d.oc || ic0 >= d.ic) continue;  // (ic is a multiple of 16: the lane's 16 channels are one block of the blocked layout)
    const int8_t *src = wei + blocked_offset(oc, ic0, kh, kw, d.ic, d.kh, d.kw);
    for (int b = 0; b < 16; ++b) dst[16 * lane + b] = (uint8_t)src[(b >> 2) * 64 + (b & 3)];
  }
}

// W1 fragment of 1x1 group g1, column block cc of its G, and conv0 block blk: byte b of lane
//   = W1[32 * G * g1 + G * (lane & 31) + cc][32 * blk + 8 * (b >> 2) + 4 * (lane >> 5) + (b & 3)]   (mid's k order)
inline void w1_fragment(uint8_t *dst, const dfx_conv_desc &d, const int8_t *wei1, int G, int g1, int cc, int blk) {
  for (int lane = 0; lane < 64; ++lane) {
    const int oc1 = 32 * G * g1 + G * (lane & 31) + cc;
    if (oc1 >= d.oc1x1) continue;
    for (int b = 0; b < 16; ++b) {
      const int oc = 32 * blk + 8 * (b >> 2) + 4 * (lane >> 5) + (b & 3);
      if (oc < d.oc) dst[16 * lane + b] = (uint8_t)wei1[blocked_offset(oc1, oc, 0, 0, d.oc, 1, 1)];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The families.

struct ConvStageIn {  // one stage's per-channel inputs as f32: bias (0 without one) and scale (count 1 = broadcast)
  std::vector<float> bias, scale;
  ConvStageIn(int n, const void *bia, int bia_dt, const float *scales, int nscales) : bias(n), scale(n) {
    for (int c = 0; c < n; ++c) {
      bias[c] = bia_dt == DFX_UNDEF ? 0.0f : bias_to_f32(bia, bia_dt, c);
      scale[c] = scales[nscales > 1 ? c : 0];
    }
  }
};

// Resident kernels (conv_mfma.cuh, conv_mfma_roles.cuh): the image in LDS order [W0 fragments | W1 fragments | constants]
//   W0 fragments [r][tap][c]: fused: A operand, row = oc 32r + rho.  unfused: B operand with the channel
//                permutation of the store stage (G == OCB): column lam of block r = oc G*lam + r
//   W1 fragments [cb][r]: cb = cg*G + cc
//   constants in the kernel's layout: the storing stage's B and C as pairs {k, k} (conv_geom.h, mfma_cst_floats)
inline void pack_resident(const dfx_conv_desc &d, const ConvPlan &p, ConvTune tune, const int8_t *wei, const int8_t *wei1,
                          const std::vector<ChanPN> &pn0, const std::vector<ChanPN> &pn1, const ConvStageIn &in0,
                          const ConvStageIn &in1, const float *scales0, ConvWeights *out) {
  const bool fused = d.oc1x1 > 0;
  const int OC = d.oc, OC1 = d.oc1x1, ICB = p.icb, OCB = p.ocb, G = p.G, NCB = OC1 / 32;
  out->n_w0 = (size_t)OCB * 9 * ICB * 1024;
  out->n_w1 = (size_t)NCB * OCB * 1024;
  out->n_cst = (size_t)mfma_cst_floats(OC, OC1) * 4;
  out->off_w1 = out->n_w0;
  out->off_cst = out->n_w0 + out->n_w1;
  out->image = std::vector<uint8_t>(out->off_cst + round16(out->n_cst), 0);
  uint8_t *o = out->image.data();
  for (int r = 0; r < OCB; ++r)
    for (int tap = 0; tap < 9; ++tap)
      for (int c = 0; c < ICB; ++c, o += 1024) w0_fragment(o, d, wei, fused ? 32 * r : r, fused ? 1 : G, c, tap);
  for (int cb = 0; cb < NCB; ++cb)
    for (int r = 0; r < OCB; ++r, o += 1024) w1_fragment(o, d, wei1, G, cb / G, cb % G, r);

  // ---- requant mode per stage (conv_mfma.cuh header; emit_group)
  const bool no_fast = tune_on(tune, "DFX_NO_FAST");    // testing aid: exact paths
  const bool no_magic = tune_on(tune, "DFX_NO_MAGIC");  // testing aid: no magic paths
  int mode0 = (d.conv0_round_mode == DFX_ROUND_NEAREST && !no_fast) ? 2 : 0;
  for (int oc = 0; oc < OC && mode0; ++oc) {
    if (!fast_magnitude_ok(pn0[oc], in0.bias[oc], in0.scale[oc])) mode0 = 0;
    else if (mode0 == 2 && !(fused ? magic0_ok(pn0[oc], in0.bias[oc]) : magic1_ok(pn0[oc], in0.bias[oc], in0.scale[oc]))) mode0 = 1;
  }
  int mode1 = (fused && d.conv1_round_mode == DFX_ROUND_NEAREST && !no_fast) ? 2 : 0;
  for (int o1 = 0; o1 < OC1 && mode1; ++o1) {
    if (!fast_magnitude_ok(pn1[o1], in1.bias[o1], in1.scale[o1])) mode1 = 0;
    else if (mode1 == 2 && !magic1_ok(pn1[o1], in1.bias[o1], in1.scale[o1])) mode1 = 1;
  }
  if (no_magic) { mode0 = std::min(mode0, 1); mode1 = std::min(mode1, 1); }
  bool roles = p.roles_ok && fused && mode1 == 2 && d.conv0_round_mode == DFX_ROUND_NEAREST && !no_fast && !no_magic;
  for (int oc = 0; oc < OC && roles; ++oc)
    if (!fast_magnitude_ok(pn0[oc], in0.bias[oc], in0.scale[oc]) || !fma0_ok(pn0[oc], in0.bias[oc], in0.scale[oc])) roles = false;
  if (roles) mode0 = 3;
  if (roles) {  // stage 1's "fma": the role-specialised kernel only
    bool fma1 = true;
    for (int o1 = 0; o1 < OC1 && fma1; ++o1) fma1 = fma1_exact(pn1[o1], in1.bias[o1], in1.scale[o1]);
    if (fma1) mode1 = 3;
  }
  if (p.variant == DFX_VARIANT_MFMA_FUSED) {
    // (the suffix names stage 1's requant route: "fma" = one v_fma_f32 per value, admitted where the addend is exactly
    //  representable -- power-of-two scales and a few others; "magic" = v_add_f32 + v_mul_f32)
    if (roles) snprintf(out->kernel_name, sizeof(out->kernel_name), "conv_mfma_roles_kernel<%d,%d,%d,%d>/%s", ICB, OCB, NCB, d.dst_dt,
                        mode1 == 3 ? "fma" : "magic");
    else snprintf(out->kernel_name, sizeof(out->kernel_name), "conv_mfma_fused_kernel<%d,%d,%d,%d>", ICB, OCB, G, d.dst_dt);
    out->block = roles ? RL_THREADS : MFMA_THREADS;
  }
  out->mode0 = mode0;
  out->mode1 = mode1;
  out->roles = roles;
  out->s0_uniform = (fused && d.conv0_nscales == 1) ? 1 : 0;
  out->s0_value = scales0[0];

  // ---- constants: fused A0 B0 C0 A1 {B1,B1} {C1,C1}; unfused A0 {B0,B0} {C0,C0}
  uint8_t *cst = out->image.data() + out->off_cst;
  int32_t A;
  float B, C;
  for (int oc = 0; oc < OC; ++oc) {
    if (fused) {
      start_consts(mode0, pn0[oc], in0.bias[oc], in0.scale[oc], &A, &B, &C);
      put_i(cst + 4 * (size_t)oc, A);
      put_f(cst + 4 * (size_t)(OC + oc), B);
      put_f(cst + 4 * (size_t)(2 * OC + oc), C);
    } else {
      inline_consts(mode0, MAGIC1_BITS, pn0[oc], in0.bias[oc], in0.scale[oc], &A, &B, &C);
      put_i(cst + 4 * (size_t)oc, A);
      for (int k = 0; k < 2; ++k) {
        put_f(cst + 4 * (size_t)(OC + 2 * oc + k), B);
        put_f(cst + 4 * (size_t)(3 * OC + 2 * oc + k), C);
      }
    }
  }
  for (int o1 = 0; o1 < OC1; ++o1) {
    inline_consts(mode1, MAGIC1_BITS, pn1[o1], in1.bias[o1], in1.scale[o1], &A, &B, &C);
    put_i(cst + 4 * (size_t)(3 * OC + o1), A);
    for (int k = 0; k < 2; ++k) {
      put_f(cst + 4 * (size_t)(3 * OC + OC1 + 2 * o1 + k), B);
      put_f(cst + 4 * (size_t)(3 * OC + 3 * OC1 + 2 * o1 + k), C);
    }
  }
}

// Streamed- and direct-weight kernels: the image [conv0 fragments | conv1 fragments | consts].
//   conv_stream.cuh: a step = 2 k-blocks x (OCC | G) fragments, in the exact order the kernel walks them (oc chunk, ic
//     chunk, step; 1x1 group, step); padding k-blocks are zero.  fused: A operand, row = channel 32*(occ*OCC + r) + rho.
//     unfused: B operand with the store stage's channel permutation: column lam of block r = 32*OCC*occ + OCC*lam + r
//   conv_direct.cuh / conv_pw.cuh: W0d[ob][kb = icb * ntap + tap], W1d[g1][blk][cc]
//   consts: comp0 (s32) bias0 scale0 [OCP each] comp1 (s32) bias1 scale1 [OC1P each]; padding channels are all-zero (their
//     intermediate is 0 and meets zero 1x1 weights)
inline int pack_streamed(const dfx_conv_desc &d, const ConvPlan &p, ConvTune tune, const int8_t *wei, const int8_t *wei1,
                         const std::vector<ChanPN> &pn0, const std::vector<ChanPN> &pn1, const ConvStageIn &in0,
                         const ConvStageIn &in1, ConvWeights *out, const char **why) {
  const bool fused = d.oc1x1 > 0, direct = p.direct != 0;
  const int OC = d.oc, OC1 = d.oc1x1, G = p.G, ntap = d.kh * d.kw;
  const int ocb = direct ? p.dgeom.ocb : p.sgeom.ocb, n_g1 = direct ? p.dgeom.n_g1 : p.sgeom.n_g1;
  const int OCP = 32 * ocb, OC1P = 32 * G * n_g1;
  if (direct) {
    out->n_w0 = (size_t)ocb * p.dgeom.icb * ntap * 1024;
    out->n_w1 = (size_t)n_g1 * ocb * G * 1024;
  } else {
    out->n_w0 = (size_t)p.sgeom.s0_steps * 2 * p.occ * 1024;
    out->n_w1 = fused ? (size_t)n_g1 * p.sgeom.ks2 * 2 * G * 1024 : 0;
  }
  out->n_cst = (size_t)3 * (OCP + OC1P) * 4;
  out->off_w1 = out->n_w0;
  out->off_cst = out->n_w0 + out->n_w1;
  out->image = std::vector<uint8_t>(out->off_cst + out->n_cst, 0);
  uint8_t *o = out->image.data();
  if (direct) {
    for (int ob = 0; ob < ocb; ++ob)
      for (int icb = 0; icb < p.dgeom.icb; ++icb)
        for (int tap = 0; tap < ntap; ++tap, o += 1024) w0_fragment(o, d, wei, 32 * ob, 1, icb, tap);
    for (int g1 = 0; g1 < n_g1; ++g1)
      for (int blk = 0; blk < ocb; ++blk)
        for (int cc = 0; cc < G; ++cc, o += 1024) w1_fragment(o, d, wei1, G, g1, cc, blk);
    if (o != out->image.data() + out->off_cst) return *why = "internal: direct pack size mismatch", DFX_ERR_HIP;
  } else {
    const StreamGeom &g = p.sgeom;
    const int OCC = p.occ;
    for (int occ = 0; occ < g.n_occ; ++occ)
      for (int icc = 0; icc < g.n_icc; ++icc) {
        const int kbn = std::min(2, g.icb - 2 * icc), ns = ntap * kbn;
        for (int s = 0; s < (ns + 1) / 2 * 2; ++s)
          for (int r = 0; r < OCC; ++r, o += 1024)
            if (s < ns)  // (else a padding k-block: zero weights)
              w0_fragment(o, d, wei, fused ? 32 * (occ * OCC + r) : 32 * OCC * occ + r, fused ? 1 : OCC, 2 * icc + s % kbn, s / kbn);
      }
    if (o != out->image.data() + out->n_w0) return *why = "internal: conv0 pack size mismatch", DFX_ERR_HIP;
    for (int g1 = 0; g1 < n_g1; ++g1)
      for (int blk = 0; blk < 2 * g.ks2; ++blk)
        for (int cc = 0; cc < G; ++cc, o += 1024)
          if (blk < g.ocb) w1_fragment(o, d, wei1, G, g1, cc, blk);
  }

  // ---- "fast" is ONE switch for both stages: proven for every channel of both; the bias slots then hold comp + bias
  //      (an exact f32)
  bool fast = d.conv0_round_mode == DFX_ROUND_NEAREST && (OC1 == 0 || d.conv1_round_mode == DFX_ROUND_NEAREST);
  for (int c = 0; c < OC; ++c) fast = fast && fast_fold_ok(pn0[c], in0.bias[c], in0.scale[c]);
  for (int c = 0; c < OC1; ++c) fast = fast && fast_fold_ok(pn1[c], in1.bias[c], in1.scale[c]);
  fast = fast && !tune_on(tune, "DFX_NO_FAST");
  out->fast = fast ? 1 : 0;
  // Requant without int -> float conversions (conv_direct.cuh, round 3), proven per channel from the actual
  // weights like the modes of the resident kernels:
  //   m0  stage 0 "fma": start value bits(2^23) + comp + bias, t = acc + bias inside (-2^23, 2^23), bias
  //       integer-valued, scale >= 0: comp slot <- start bits, bias slot <- -2^23 * scale
  //   m1  stage 1 "magic" (u8 output through the 16-byte store path only): start 1/(2 pi), conditions of
  //       magic1_ok; bias slot <- (comp + bias - 2^23 - 0x22F983) * 2^-26, scale slot <- scale * 2^26 (m1 = 2),
  //       or bias slot <- (comp + bias - 2^23 - 0x22F983) * scale where that product is exact for every channel:
  //       one fma (m1 = 3)
  bool m0 = false, m1 = false, fma1 = true;
  if (direct && fast && !tune_on(tune, "DFX_NO_MAGIC")) {
    // (stage 0's "fma" route relies on the unsigned saturation of a u8 result: the fused intermediate, or a u8 dst)
    m0 = OC1 > 0 || d.dst_dt == DFX_U8;
    for (int c = 0; c < OC && m0; ++c) m0 = fma0_ok(pn0[c], in0.bias[c], in0.scale[c]);
    m1 = d.dst_dt == DFX_U8 && G == 4 && OC1 > 0;
    for (int c = 0; c < OC1 && m1; ++c) {
      m1 = magic1_ok(pn1[c], in1.bias[c], in1.scale[c]);
      fma1 = fma1 && fma1_exact(pn1[c], in1.bias[c], in1.scale[c]);
    }
    m1 = m1 && m0;  // (the kernels specialise on "both stages without conversions": conv_direct.cuh, QM)
  }
  out->m0 = m0 ? 1 : 0;
  out->m1 = m1 ? (fma1 ? 3 : 2) : 0;

  uint8_t *cst = out->image.data() + out->off_cst;
  int32_t A;
  float B, C;
  for (int c = 0; c < OC; ++c) {
    start_consts(m0 ? 3 : 0, pn0[c], in0.bias[c], in0.scale[c], &A, &B, &C);
    if (fast && !m0) B = (float)((double)A + (double)in0.bias[c]);
    put_i(cst + 4 * (size_t)c, A);
    put_f(cst + 4 * (size_t)(OCP + c), B);
    put_f(cst + 4 * (size_t)(2 * OCP + c), C);
  }
  for (int c = 0; c < OC1; ++c) {
    inline_consts(out->m1, 0, pn1[c], in1.bias[c], in1.scale[c], &A, &B, &C);
    if (fast && !m1) B = (float)((double)A + (double)in1.bias[c]);
    put_i(cst + 4 * (size_t)(3 * OCP + c), A);
    put_f(cst + 4 * (size_t)(3 * OCP + OC1P + c), B);
    put_f(cst + 4 * (size_t)(3 * OCP + 2 * OC1P + c), C);
  }
  return DFX_OK;
}

// The scalar kernel (conv_generic.hip) follows the reference's arithmetic step by step: the weights as they came, at
// 16-byte-aligned offsets, and [comp0 b0 s0 comp1 b1 s1] per real channel with the compensations 0
inline void pack_generic(const dfx_conv_desc &d, const int8_t *wei, const int8_t *wei1, const ConvStageIn &in0,
                         const ConvStageIn &in1, ConvWeights *out) {
  const int OC = d.oc, OC1 = d.oc1x1;
  out->n_w0 = (size_t)OC * d.ic * d.kh * d.kw;
  out->n_w1 = (size_t)OC1 * OC;
  out->n_cst = (size_t)3 * (OC + OC1) * 4;
  out->off_w1 = round16(out->n_w0);
  out->off_cst = round16(out->off_w1 + out->n_w1);
  out->image = std::vector<uint8_t>(out->off_cst + out->n_cst, 0);
  memcpy(out->image.data(), wei, out->n_w0);
  if (OC1) memcpy(out->image.data() + out->off_w1, wei1, out->n_w1);
  uint8_t *cst = out->image.data() + out->off_cst;
  for (int c = 0; c < OC; ++c) {
    put_f(cst + 4 * (size_t)(OC + c), in0.bias[c]);
    put_f(cst + 4 * (size_t)(2 * OC + c), in0.scale[c]);
  }
  for (int c = 0; c < OC1; ++c) {
    put_f(cst + 4 * (size_t)(3 * OC + OC1 + c), in1.bias[c]);
    put_f(cst + 4 * (size_t)(3 * OC + 2 * OC1 + c), in1.scale[c]);
  }
}

// Everything dfx_conv_set_weights computes on the host, for the plan `p` of the validated descriptor `d`: the image, the
// routes, kernel name and block into *out.  The pointers are the caller's arguments, already checked against the
// descriptor (wei1 / scales1 of a fused op, a bias where its dtype is set).  DFX_OK, or a code with *why set.
inline int conv_pack_weights(const dfx_conv_desc &d, const ConvPlan &p, ConvTune tune, const int8_t *wei, const void *bia0,
                             const float *scales0, const int8_t *wei1, const void *bia1, const float *scales1, ConvWeights *out,
                             const char **why) {
  *why = "";
  out->mode0 = out->mode1 = out->s0_uniform = out->fast = out->m0 = out->m1 = 0;
  out->s0_value = 0.0f;
  out->roles = false;
  out->block = p.block;
  snprintf(out->kernel_name, sizeof(out->kernel_name), "%s", p.kernel_name);
  const ConvStageIn in0(d.oc, bia0, d.bia0_dt, scales0, d.conv0_nscales), in1(d.oc1x1, bia1, d.bia1_dt, scales1, d.conv1_nscales);
  if (p.variant == DFX_VARIANT_GENERIC) {
    pack_generic(d, wei, wei1, in0, in1, out);
    return DFX_OK;
  }
  std::vector<ChanPN> pn0, pn1;
  conv_channel_pn(d, wei, wei1, pn0, pn1);
  if (p.variant == DFX_VARIANT_MFMA_STREAM) return pack_streamed(d, p, tune, wei, wei1, pn0, pn1, in0, in1, out, why);
  pack_resident(d, p, tune, wei, wei1, pn0, pn1, in0, in1, scales0, out);
  return DFX_OK;
}

}  // namespace dfx
