// attn_host.h -- what attn_check and bench_attn share: a shape record with the library's addressing, densely packed strides,
// the head-sliced strides of an attention tensor, the softmax table's recipe, a seeded fill and the scalar restatement of the
// op as the chain it is defined by (include/dfx.h): bmm_host.h's matrix product for the logits and the context, dfx_head's
// table softmax between them.  Host only.
#pragma once

#include "bmm_host.h"

struct AttnShape {
  int batch0, batch1, tq, tk, d, dv;
  int q_dt, dst_dt, relu, rm;
  float prob_scale;
  long long q_s0, q_s1, ldq, k_s0, k_s1, ldk, v_s0, v_s1, ldv, o_s0, o_s1, ldo;
  long long span(long long s0, long long s1, long long ld, long long rows, long long cols, bool read) const {
    return (batch0 - 1) * s0 + (batch1 - 1) * s1 + (rows - 1) * ld + (read ? BmmShape::row_end(cols, ld) : cols);
  }
  // elements of each operand's storage: q, k and v up to the valid columns of their last row rounded up to 16 (within the
  // leading dimension): what the library may read
  long long q_elems() const { return span(q_s0, q_s1, ldq, tq, d, true); }
  long long k_elems() const { return span(k_s0, k_s1, ldk, tk, d, true); }
  long long v_elems() const { return span(v_s0, v_s1, ldv, tk, dv, true); }
  long long o_elems() const { return span(o_s0, o_s1, ldo, tq, dv, false); }
  dfx_attn_desc desc(int nscales, int force_path) const {
    dfx_attn_desc a;
    memset(&a, 0, sizeof(a));
    a.batch0 = batch0; a.batch1 = batch1; a.tq = tq; a.tk = tk; a.d = d; a.dv = dv;
    a.q_dt = q_dt; a.k_dt = DFX_S8; a.v_dt = DFX_S8; a.dst_dt = dst_dt; a.relu = relu; a.round_mode = rm; a.nscales = nscales;
    a.force_path = force_path; a.prob_scale = prob_scale;
    a.q_s0 = q_s0; a.q_s1 = q_s1; a.ldq = ldq; a.k_s0 = k_s0; a.k_s1 = k_s1; a.ldk = ldk;
    a.v_s0 = v_s0; a.v_s1 = v_s1; a.ldv = ldv; a.o_s0 = o_s0; a.o_s1 = o_s1; a.ldo = ldo;
    return a;
  }
  // the two products of the chain over host copies of L and P, {G, tq, up16(tk)}
  BmmShape logits() const {
    BmmShape s;
    memset(&s, 0, sizeof(s));
    const long long ldl = bmm_up16(tk);
    s.batch0 = batch0; s.batch1 = batch1; s.m = tq; s.n = tk; s.k = d; s.trans_b = 1; s.a_dt = q_dt; s.dst_dt = DFX_S8; s.rm = rm;
    s.a_s0 = q_s0; s.a_s1 = q_s1; s.lda = ldq; s.b_s0 = k_s0; s.b_s1 = k_s1; s.ldb = ldk;
    s.ldc = ldl; s.c_s1 = ldl * tq; s.c_s0 = s.c_s1 * batch1;
    return s;
  }
  BmmShape context() const {
    BmmShape s;
    memset(&s, 0, sizeof(s));
    const long long ldl = bmm_up16(tk);
    s.batch0 = batch0; s.batch1 = batch1; s.m = tq; s.n = dv; s.k = tk; s.trans_b = 0; s.a_dt = DFX_U8; s.dst_dt = dst_dt; s.relu = relu; s.rm = rm;
    s.lda = ldl; s.a_s1 = ldl * tq; s.a_s0 = s.a_s1 * batch1;
    s.b_s0 = v_s0; s.b_s1 = v_s1; s.ldb = ldv; s.c_s0 = o_s0; s.c_s1 = o_s1; s.ldc = ldo;
    return s;
  }
};

inline size_t attn_esize(int dt) { return bmm_esize(dt); }

// self-attention over {bs, t, heads * d} tensors: Q, K, V and the context head-sliced in place
inline AttnShape attn_heads(int bs, int heads, int t, int d, int q_dt, int dst_dt) {
  AttnShape s;
  memset(&s, 0, sizeof(s));
  const long long hd = (long long)heads * d;
  s.batch0 = bs; s.batch1 = heads; s.tq = s.tk = t; s.d = s.dv = d; s.q_dt = q_dt; s.dst_dt = dst_dt; s.prob_scale = 255.0f;
  s.q_s0 = s.k_s0 = s.v_s0 = s.o_s0 = t * hd;
  s.q_s1 = s.k_s1 = s.v_s1 = s.o_s1 = d;
  s.ldq = s.ldk = s.ldv = s.ldo = hd;
  return s;
}

inline void attn_fill(std::vector<unsigned char> &v, uint32_t seed) { bmm_fill(v, seed); }

// E[i] = floor(exp(-i * step) * floor((2^32 - 1) / c)): the recipe of include/dfx.h
inline void attn_softmax_table(uint32_t *e, double step, int c) {
  const double top = (double)(0xffffffffu / (uint32_t)c);
  for (int i = 0; i < 256; ++i) e[i] = (uint32_t)std::floor(std::exp(-(double)i * step) * top);
}

// dfx_head's table softmax of one row of s8 logits -> u8 probabilities
inline void attn_host_softmax(const signed char *l, int c, const uint32_t *e, float prob_scale, unsigned char *p) {
  int mx = -128;
  for (int j = 0; j < c; ++j) mx = l[j] > mx ? l[j] : mx;
  uint32_t sum = 0;
  for (int j = 0; j < c; ++j) sum += e[mx - l[j]];
  const float fs = (float)sum;
  for (int j = 0; j < c; ++j) {
    volatile float pr = (float)e[mx - l[j]] / fs;
    volatile float v = pr * prob_scale;
    float r = nearbyintf(v);
    r = (v != v) ? 0.0f : r;
    r = r < 0.0f ? 0.0f : (r > 255.0f ? 255.0f : r);
    p[j] = (unsigned char)r;
  }
}

// O's valid elements as bit patterns, {batch0, batch1, tq, dv} row-major (1-byte types in the low byte)
inline std::vector<uint32_t> attn_host_values(const AttnShape &s, const unsigned char *q, const unsigned char *k, const unsigned char *v,
                                              const uint32_t *table, float logit_scale, const float *out_scales, int nscales) {
  const BmmShape ls = s.logits(), cs = s.context();
  const long long ldl = ls.ldc;
  std::vector<unsigned char> l((size_t)s.batch0 * s.batch1 * s.tq * ldl, 0xCD), p(l.size(), 0xCD);
  std::vector<uint32_t> out;
  for (int b0 = 0; b0 < s.batch0; ++b0)
    for (int b1 = 0; b1 < s.batch1; ++b1)
      for (int m = 0; m < s.tq; ++m) {
        const size_t row = (size_t)(b0 * ls.c_s0 + b1 * ls.c_s1 + (long long)m * ldl);
        for (int n = 0; n < s.tk; ++n) l[row + n] = (unsigned char)bmm_host_value(ls, q, k, &logit_scale, 1, b0, b1, m, n);
        attn_host_softmax((const signed char *)&l[row], s.tk, table, s.prob_scale, &p[row]);
      }
  for (int b0 = 0; b0 < s.batch0; ++b0)
    for (int b1 = 0; b1 < s.batch1; ++b1)
      for (int m = 0; m < s.tq; ++m)
        for (int j = 0; j < s.dv; ++j) out.push_back(bmm_host_value(cs, p.data(), v, out_scales, nscales, b0, b1, m, j));
  return out;
}
