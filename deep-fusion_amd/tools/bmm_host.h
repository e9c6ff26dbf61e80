// bmm_host.h -- what bmm_check and bench_bmm share: a shape record with the library's addressing, densely packed strides,
// the head-sliced strides of an attention tensor, the scalar restatement of the op (include/dfx.h: exact integer sum,
// float(acc) * scale, ReLU, the x86 conversion and saturations) and a seeded fill.  Host only.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "cli_flags.h"
#include "dfx.h"

struct BmmShape {
  int batch0, batch1, m, n, k, trans_b;
  int a_dt, dst_dt, relu, rm;
  long long a_s0, a_s1, lda, b_s0, b_s1, ldb, c_s0, c_s1, ldc;
  long long brows() const { return trans_b ? n : k; }
  long long bcols() const { return trans_b ? k : n; }
  // elements of each operand's storage: a and b up to the valid columns of their last row rounded up to 16 (within the
  // leading dimension): what the library may read
  static long long row_end(long long cols, long long ld) { return ld < (cols + 15) / 16 * 16 ? ld : (cols + 15) / 16 * 16; }
  long long a_elems() const { return (batch0 - 1) * a_s0 + (batch1 - 1) * a_s1 + (long long)(m - 1) * lda + row_end(k, lda); }
  long long b_elems() const { return (batch0 - 1) * b_s0 + (batch1 - 1) * b_s1 + (brows() - 1) * ldb + row_end(bcols(), ldb); }
  long long c_elems() const { return (batch0 - 1) * c_s0 + (batch1 - 1) * c_s1 + (long long)(m - 1) * ldc + n; }
  dfx_bmm_desc desc(int nscales, int force_path) const {
    dfx_bmm_desc d;
    memset(&d, 0, sizeof(d));
    d.batch0 = batch0; d.batch1 = batch1; d.m = m; d.n = n; d.k = k; d.trans_b = trans_b;
    d.a_dt = a_dt; d.b_dt = DFX_S8; d.dst_dt = dst_dt; d.relu = relu; d.round_mode = rm; d.nscales = nscales; d.force_path = force_path;
    d.a_s0 = a_s0; d.a_s1 = a_s1; d.lda = lda; d.b_s0 = b_s0; d.b_s1 = b_s1; d.ldb = ldb; d.c_s0 = c_s0; d.c_s1 = c_s1; d.ldc = ldc;
    return d;
  }
};

inline long long bmm_up16(long long v) { return (v + 15) / 16 * 16; }
inline size_t bmm_esize(int dt) { return (dt == DFX_F32 || dt == DFX_S32) ? 4 : 1; }

// {batch0, batch1} matrices packed one behind the other, leading dimensions rounded up to 16
inline BmmShape bmm_dense(int batch0, int batch1, int m, int n, int k, int trans_b, int a_dt, int dst_dt) {
  BmmShape s;
  memset(&s, 0, sizeof(s));
  s.batch0 = batch0; s.batch1 = batch1; s.m = m; s.n = n; s.k = k; s.trans_b = trans_b; s.a_dt = a_dt; s.dst_dt = dst_dt;
  s.lda = bmm_up16(k); s.a_s1 = s.lda * m; s.a_s0 = s.a_s1 * batch1;
  s.ldb = bmm_up16(s.bcols()); s.b_s1 = s.ldb * s.brows(); s.b_s0 = s.b_s1 * batch1;
  s.ldc = bmm_up16(n); s.c_s1 = s.ldc * m; s.c_s0 = s.c_s1 * batch1;
  return s;
}

// Q.K^T (pv = 0) or P.V (pv = 1) of an attention block over a {bs, t, heads * d} tensor: Q, K, V and the context head-sliced
// in place, the logits / probabilities {bs, heads, t, up16(t)}
inline BmmShape bmm_attention(int bs, int heads, int t, int d, int pv, int a_dt, int dst_dt) {
  BmmShape s;
  memset(&s, 0, sizeof(s));
  const long long hd = (long long)heads * d, lt = bmm_up16(t);
  s.batch0 = bs; s.batch1 = heads; s.a_dt = a_dt; s.dst_dt = dst_dt;
  if (!pv) {
    s.m = t; s.n = t; s.k = d; s.trans_b = 1;
    s.a_s0 = t * hd; s.a_s1 = d; s.lda = hd;
    s.b_s0 = t * hd; s.b_s1 = d; s.ldb = hd;
    s.c_s0 = heads * t * lt; s.c_s1 = t * lt; s.ldc = lt;
  } else {
    s.m = t; s.n = d; s.k = t; s.trans_b = 0;
    s.a_s0 = heads * t * lt; s.a_s1 = t * lt; s.lda = lt;
    s.b_s0 = t * hd; s.b_s1 = d; s.ldb = hd;
    s.c_s0 = t * hd; s.c_s1 = d; s.ldc = hd;
  }
  return s;
}

inline void bmm_fill(std::vector<unsigned char> &v, uint32_t seed) {
  Lcg g(seed);
  for (size_t i = 0; i < v.size(); ++i) v[i] = (unsigned char)(g.next() >> 3);
}

inline int32_t bmm_cvt_x86(float f, int rm) {
  if (!(f >= -2147483648.0f && f < 2147483648.0f)) return INT32_MIN;
  return (int32_t)(rm ? floorf(f) : nearbyintf(f));
}

// one element of C as its bit pattern (1-byte types in the low byte)
inline uint32_t bmm_host_value(const BmmShape &s, const unsigned char *a, const unsigned char *b, const float *scales, int nscales, int b0,
                               int b1, int m, int n) {
  const unsigned char *ap = a + b0 * s.a_s0 + b1 * s.a_s1 + (long long)m * s.lda;
  const unsigned char *bp = b + b0 * s.b_s0 + b1 * s.b_s1 + (s.trans_b ? (long long)n * s.ldb : n);
  const long long step = s.trans_b ? 1 : s.ldb;
  long long acc = 0;
  for (int k = 0; k < s.k; ++k) acc += (long long)(s.a_dt == DFX_U8 ? (int)ap[k] : (int)(signed char)ap[k]) * (int)(signed char)bp[k * step];
  volatile float f = (float)(int32_t)acc;
  f = f * scales[nscales == 1 ? 0 : n];
  float r = f;
  if ((s.relu || s.dst_dt == DFX_U8) && 0.0f > r) r = 0.0f;
  uint32_t bits;
  if (s.dst_dt == DFX_F32) {
    memcpy(&bits, &r, 4);
    return bits;
  }
  const int32_t v = bmm_cvt_x86(r, s.rm);
  if (s.dst_dt == DFX_S32) return (uint32_t)v;
  if (s.dst_dt == DFX_S8) return (uint32_t)(unsigned char)(signed char)(v < -128 ? -128 : v > 127 ? 127 : v);
  return (uint32_t)((uint32_t)v > 255u ? 255u : (uint32_t)v);
}
