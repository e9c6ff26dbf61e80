// se_check -- runs deepfusion::squeeze_excite and deepfusion::global_avg_pool of the drop-in C++ API (include/deepfusion.h)
// over a few layers and compares every result, bit for bit, with a scalar loop in this file: the exact channel sums,
// rint(float(sum) / float(pixels)), the two s32 dot products with float(acc) + bias, * scale (two roundings), the ReLU and
// the x86 conversion, the table lookup, and float(src * gate) * out_scale converted the same way.  Half of the layers
// run in place (dst is src).  A second submit after the weights changed on the host must re-pack them.  Exits non-zero
// on the first difference.
//   se_check
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "cli_flags.h"
#include "deepfusion.h"

using namespace deepfusion;

static std::unique_ptr<memory> mk(int n, int c, int h, int w, memory::format fmt, memory::dtype dt) {
  return std::unique_ptr<memory>(new memory(memory::nchw_dims{n, c, h, w}, fmt, dt));
}

struct Layer {
  const char *name;
  int bs, c, h, w, cr;
  memory::dtype bia1_dt, bia2_dt;  // undef: no bias
  bool per_channel, in_place;
  round_mode rm;
};

// vcvtps2dq: nearest-even or floor; NaN / out of range -> 0x80000000
static int32_t cvt_x86(float f, round_mode rm) {
  if (!(f >= -2147483648.0f && f < 2147483648.0f)) return INT32_MIN;
  return (int32_t)(rm == round_mode::down ? floorf(f) : nearbyintf(f));
}

static float bias_at(const void *bia, memory::dtype dt, int k) {
  if (!bia) return 0.0f;
  if (dt == memory::dtype::f32) return ((const float *)bia)[k];
  if (dt == memory::dtype::s32) return (float)((const int32_t *)bia)[k];
  if (dt == memory::dtype::s8) return (float)((const int8_t *)bia)[k];
  return (float)((const uint8_t *)bia)[k];
}

static float requant(int32_t acc, float bias, float scale, bool relu) {
  volatile float f = (float)acc;
  f = f + bias;
  f = f * scale;
  if (relu && 0.0f > f) f = 0.0f;
  return f;
}

static uint8_t sat_u8(int32_t v) { return (uint8_t)((uint32_t)v > 255u ? 255u : (uint32_t)v); }

// z {bs, c}: the global average
static std::vector<uint8_t> scalar_squeeze(const Layer &l, const uint8_t *src) {
  const int px = l.h * l.w;
  std::vector<uint8_t> z((size_t)l.bs * l.c);
  for (int n = 0; n < l.bs; ++n)
    for (int c = 0; c < l.c; ++c) {
      int32_t sum = 0;
      for (int p = 0; p < px; ++p) sum += src[((size_t)n * px + p) * l.c + c];
      volatile float q = (float)sum / (float)px;
      const int v = (int)nearbyintf(q);
      z[(size_t)n * l.c + c] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
    }
  return z;
}

static std::vector<uint8_t> scalar_ref(const Layer &l, const uint8_t *src, const s8 *w1, const void *b1, const s8 *w2, const void *b2,
                                       const std::array<u8, 256> &lut, const std::vector<float> &s1, const std::vector<float> &s2,
                                       const std::vector<float> &so) {
  const int px = l.h * l.w;
  const std::vector<uint8_t> z = scalar_squeeze(l, src);
  std::vector<uint8_t> out((size_t)l.bs * px * l.c), h(l.cr), g(l.c);
  for (int n = 0; n < l.bs; ++n) {
    for (int j = 0; j < l.cr; ++j) {
      int32_t acc = 0;
      for (int c = 0; c < l.c; ++c) acc += (int32_t)z[(size_t)n * l.c + c] * (int32_t)w1[(size_t)j * l.c + c];
      h[j] = sat_u8(cvt_x86(requant(acc, bias_at(b1, l.bia1_dt, j), s1[s1.size() == 1 ? 0 : j], true), l.rm));
    }
    for (int c = 0; c < l.c; ++c) {
      int32_t acc = 0;
      for (int j = 0; j < l.cr; ++j) acc += (int32_t)h[j] * (int32_t)w2[(size_t)c * l.cr + j];
      const int32_t t = cvt_x86(requant(acc, bias_at(b2, l.bia2_dt, c), s2[s2.size() == 1 ? 0 : c], false), l.rm);
      g[c] = lut[(t < -128 ? -128 : t > 127 ? 127 : t) + 128];
    }
    for (int p = 0; p < px; ++p)
      for (int c = 0; c < l.c; ++c) {
        const size_t i = ((size_t)n * px + p) * l.c + c;
        out[i] = sat_u8(cvt_x86(requant((int32_t)src[i] * (int32_t)g[c], 0.0f, so[so.size() == 1 ? 0 : c], true), l.rm));
      }
  }
  return out;
}

static std::unique_ptr<memory> make_bias(memory::dtype dt, int n, Lcg &g) {
  std::unique_ptr<memory> bia;
  if (dt == memory::dtype::undef) return bia;
  bia.reset(new memory(memory::dims{n}, memory::format::x, dt));
  void *p = bia->data();
  for (int k = 0; k < n; ++k) {
    const int v = (int)(g.next() % 4001) - 2000;
    if (dt == memory::dtype::f32) ((float *)p)[k] = (float)v * 0.5f;
    else if (dt == memory::dtype::s32) ((int32_t *)p)[k] = v;
    else if (dt == memory::dtype::s8) ((int8_t *)p)[k] = (int8_t)(v % 128);
    else ((uint8_t *)p)[k] = (uint8_t)(v & 0xff);
  }
  return bia;
}

static int run(const Layer &l, Lcg &g) {
  const auto nhwc = memory::format::nhwc;
  const int px = l.h * l.w;
  auto src = mk(l.bs, l.c, l.h, l.w, nhwc, memory::dtype::u8);
  uint8_t *sp = (uint8_t *)src->data();
  for (int n = 0; n < l.bs; ++n)
    for (int c = 0; c < l.c; ++c) {  // an amplitude per (image, channel), so that the channel means differ
      const unsigned amp = 1 + g.next() % 255;
      for (int p = 0; p < px; ++p) sp[((size_t)n * px + p) * l.c + c] = (uint8_t)((g.next() % 256) * amp / 255);
    }
  const std::vector<uint8_t> src_copy(sp, sp + src->size());
  auto wei1 = mk(l.cr, l.c, 1, 1, memory::format::oihw, memory::dtype::s8);
  auto wei2 = mk(l.c, l.cr, 1, 1, memory::format::oihw, memory::dtype::s8);
  for (auto *w : {wei1.get(), wei2.get()}) {
    s8 *wp = (s8 *)w->data();
    for (size_t i = 0; i < w->size(); ++i) wp[i] = (s8)((int)(g.next() % 255) - 127);
  }
  auto bia1 = make_bias(l.bia1_dt, l.cr, g), bia2 = make_bias(l.bia2_dt, l.c, g);
  std::array<u8, 256> lut;
  for (int i = 0; i < 256; ++i) lut[i] = (u8)nearbyint(255.0 / (1.0 + exp(-(double)(i - 128) / 24.0)));
  std::vector<float> s1(l.per_channel ? l.cr : 1), s2(l.per_channel ? l.c : 1), so(l.per_channel ? l.c : 1);
  for (size_t k = 0; k < s1.size(); ++k) s1[k] = 96.0f / (sqrtf((float)l.c) * 64.0f * 73.0f) * (1.0f + 0.01f * (float)(k % 7));
  for (size_t k = 0; k < s2.size(); ++k) s2[k] = 48.0f / (sqrtf((float)l.cr) * 60.0f * 73.0f) * (1.0f + 0.01f * (float)(k % 5));
  for (size_t k = 0; k < so.size(); ++k) so[k] = (1.0f + 0.02f * (float)(k % 3)) / 255.0f;

  int bad = 0;
  // the first stage alone
  auto z = mk(l.bs, l.c, 1, 1, nhwc, memory::dtype::u8);
  memset(z->data(), 0xA5, z->buffer_size());
  auto gap = global_avg_pool(src, z);
  gap->submit();
  const std::vector<uint8_t> zwant = scalar_squeeze(l, src_copy.data());
  const bool zbad = memcmp(zwant.data(), z->host_data(), zwant.size()) != 0;
  bad += zbad;

  std::unique_ptr<memory> other;
  if (!l.in_place) {
    other = mk(l.bs, l.c, l.h, l.w, nhwc, memory::dtype::u8);
    memset(other->data(), 0xA5, other->buffer_size());
  }
  std::unique_ptr<memory> &dst = l.in_place ? src : other;
  auto se = squeeze_excite(src, wei1, bia1, wei2, bia2, lut, dst, s1, s2, so, l.rm);
  se->submit();
  std::vector<uint8_t> want = scalar_ref(l, src_copy.data(), (const s8 *)wei1->host_data(), bia1 ? bia1->host_data() : nullptr,
                                         (const s8 *)wei2->host_data(), bia2 ? bia2->host_data() : nullptr, lut, s1, s2, so);
  const bool sbad = memcmp(want.data(), dst->host_data(), want.size()) != 0;
  bad += sbad;
  printf("se_check %-12s bs %2d  %3dx%-3dx%4d -> %3d%s: global_avg_pool %s; squeeze_excite %s\n", l.name, l.bs, l.h, l.w, l.c, l.cr,
         l.in_place ? " in place" : "", zbad ? "DIFFERENT from the scalar loop" : "identical", sbad ? "DIFFERENT from the scalar loop" : "identical");
  if (!bad) {  // a second submit after the weights changed on the host must re-pack them
    s8 *w = (s8 *)wei2->data();
    for (size_t i = 0; i < wei2->size(); i += 2) w[i] = (s8)-w[i];
    memcpy(src->data(), src_copy.data(), src_copy.size());
    se->submit();
    want = scalar_ref(l, src_copy.data(), (const s8 *)wei1->host_data(), bia1 ? bia1->host_data() : nullptr, (const s8 *)wei2->host_data(),
                      bia2 ? bia2->host_data() : nullptr, lut, s1, s2, so);
    if (memcmp(want.data(), dst->host_data(), want.size()) != 0) {
      printf("se_check %-12s: DIFFERENT after the weights changed\n", l.name);
      bad = 1;
    }
  }
  return bad ? 1 : 0;
}

int main() {
  Lcg g(4242);
  const auto U = memory::dtype::undef;
  const std::vector<Layer> layers = {
      {"effnet_b0_a", 2, 32, 28, 28, 8, memory::dtype::s32, memory::dtype::s32, false, false, round_mode::nearest},
      {"effnet_b0_g", 3, 1152, 7, 7, 48, memory::dtype::f32, U, true, true, round_mode::nearest},
      {"mnv3_c72", 2, 72, 14, 14, 24, U, memory::dtype::s8, true, false, round_mode::down},
      {"c17_cr5", 3, 17, 5, 9, 5, memory::dtype::u8, memory::dtype::f32, false, true, round_mode::nearest},
      {"regnety_c48", 1, 48, 33, 17, 12, U, U, true, true, round_mode::down},
      {"pixel", 4, 64, 1, 1, 4, memory::dtype::s32, memory::dtype::s32, false, false, round_mode::nearest},
  };
  int bad = 0;
  for (const Layer &l : layers) bad += run(l, g);
  if (bad) {
    printf("se_check: %d of %zu layers FAILED\n", bad, layers.size());
    return 1;
  }
  printf("se_check: every layer identical to the scalar loop (%zu layers)\n", layers.size());
  return 0;
}
