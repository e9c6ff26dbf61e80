// fc_check -- runs deepfusion::inner_product of the drop-in C++ API (include/deepfusion.h) over a few layers and
// compares every result, bit for bit, with a scalar loop in this file: the s32 dot product of the NHWC source with the
// plain oihw weights, then float(acc) + bias, * scale (two roundings), the ReLU and the x86 conversion.  Where the dense
// conv can express the layer (c, oc % 16 == 0) it also compares with conv() on a window of the whole image.  A second
// submit after the weights changed on the host must re-pack them.  Exits non-zero on the first difference.
//   fc_check
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
  int bs, c, h, w, oc;
  memory::dtype dst_dt, bia_dt;  // bia_dt undef: no bias
  bool relu, per_channel;
  round_mode rm;
};

static size_t esize(memory::dtype dt) { return (dt == memory::dtype::f32 || dt == memory::dtype::s32) ? 4 : 1; }

// vcvtps2dq: nearest-even or floor; NaN / out of range -> 0x80000000
static int32_t cvt_x86(float f, round_mode rm) {
  if (!(f >= -2147483648.0f && f < 2147483648.0f)) return INT32_MIN;
  return (int32_t)(rm == round_mode::down ? floorf(f) : nearbyintf(f));
}

// the expected bytes of dst {bs, oc}
static std::vector<unsigned char> scalar_ref(const Layer &l, const uint8_t *src, const s8 *wei, const void *bia, const std::vector<float> &sc) {
  std::vector<unsigned char> out((size_t)l.bs * l.oc * esize(l.dst_dt));
  for (int n = 0; n < l.bs; ++n)
    for (int o = 0; o < l.oc; ++o) {
      int32_t acc = 0;
      for (int c = 0; c < l.c; ++c)
        for (int y = 0; y < l.h; ++y)
          for (int x = 0; x < l.w; ++x)
            acc += (int32_t)src[(((size_t)n * l.h + y) * l.w + x) * l.c + c] * (int32_t)wei[(((size_t)o * l.c + c) * l.h + y) * l.w + x];
      volatile float f = (float)acc;
      if (bia) {
        float b = 0.0f;
        if (l.bia_dt == memory::dtype::f32) b = ((const float *)bia)[o];
        else if (l.bia_dt == memory::dtype::s32) b = (float)((const int32_t *)bia)[o];
        else if (l.bia_dt == memory::dtype::s8) b = (float)((const int8_t *)bia)[o];
        else b = (float)((const uint8_t *)bia)[o];
        f = f + b;
      }
      f = f * sc[sc.size() == 1 ? 0 : o];
      if ((l.relu || l.dst_dt == memory::dtype::u8) && 0.0f > f) f = 0.0f;
      const size_t i = (size_t)n * l.oc + o;
      const float fv = f;
      if (l.dst_dt == memory::dtype::f32) memcpy(&out[4 * i], &fv, 4);
      else {
        const int32_t v = cvt_x86(fv, l.rm);
        if (l.dst_dt == memory::dtype::s32) memcpy(&out[4 * i], &v, 4);
        else if (l.dst_dt == memory::dtype::s8) out[i] = (unsigned char)(int8_t)(v < -128 ? -128 : v > 127 ? 127 : v);
        else out[i] = (unsigned char)((uint32_t)v > 255u ? 255u : (uint32_t)v);
      }
    }
  return out;
}

static int run(const Layer &l, Lcg &g) {
  const auto nhwc = memory::format::nhwc;
  const int K = l.c * l.h * l.w;
  auto src = mk(l.bs, l.c, l.h, l.w, nhwc, memory::dtype::u8);
  uint8_t *sp = (uint8_t *)src->data();
  for (size_t i = 0; i < src->size(); ++i) sp[i] = (uint8_t)(g.next() % 256);
  auto wei = mk(l.oc, l.c, l.h, l.w, memory::format::oihw, memory::dtype::s8);
  s8 *wp = (s8 *)wei->data();
  for (size_t i = 0; i < wei->size(); ++i) wp[i] = (s8)((int)(g.next() % 256) - 128);
  std::unique_ptr<memory> bia;
  if (l.bia_dt != memory::dtype::undef) {
    bia.reset(new memory(memory::dims{l.oc}, memory::format::x, l.bia_dt));
    void *p = bia->data();
    for (int k = 0; k < l.oc; ++k) {
      const int v = (int)(g.next() % 2001) - 1000;
      if (l.bia_dt == memory::dtype::f32) ((float *)p)[k] = (float)v * 0.5f;
      else if (l.bia_dt == memory::dtype::s32) ((int32_t *)p)[k] = v;
      else if (l.bia_dt == memory::dtype::s8) ((int8_t *)p)[k] = (int8_t)(v % 128);
      else ((uint8_t *)p)[k] = (uint8_t)(v & 0xff);
    }
  }
  std::vector<float> sc(l.per_channel ? l.oc : 1);
  for (size_t k = 0; k < sc.size(); ++k) sc[k] = (0.012f + 0.00002f * (float)k) / sqrtf((float)K);
  auto got = mk(l.bs, l.oc, 1, 1, nhwc, l.dst_dt);
  memset(got->data(), 0xA5, got->buffer_size());
  auto fc = inner_product(src, wei, bia, got, l.relu, sc, l.rm);
  fc->submit();
  std::vector<unsigned char> want = scalar_ref(l, (const uint8_t *)src->host_data(), (const s8 *)wei->host_data(), bia ? bia->host_data() : nullptr, sc);
  int bad = 0;
  if (want.size() != got->buffer_size() || memcmp(want.data(), got->host_data(), want.size()) != 0) bad = 1;
  const bool dense = l.c % 16 == 0 && l.oc % 16 == 0;
  const char *twin = "no dense twin";
  std::unique_ptr<memory> dwei, cwant;
  std::unique_ptr<op> cv;
  if (dense && !bad) {
    dwei.reset(new memory(memory::nchw_dims{l.oc, l.c, l.h, l.w}, memory::format::OIhw4i16o4i, memory::dtype::s8));
    reorder_weights((const s8 *)wei->host_data(), dwei);
    cwant = mk(l.bs, l.oc, 1, 1, nhwc, l.dst_dt);
    memset(cwant->data(), 0x5A, cwant->buffer_size());
    cv = conv(src, dwei, bia, {1, 1}, {0, 0}, cwant, l.relu, sc, l.rm);
    cv->submit();
    twin = "conv() identical";
    if (memcmp(cwant->host_data(), got->host_data(), cwant->buffer_size()) != 0) {
      twin = "conv() DIFFERENT";
      bad = 1;
    }
  }
  printf("fc_check %-14s bs %3d  %dx%dx%d (K %5d) -> %4d: %s; %s\n", l.name, l.bs, l.h, l.w, l.c, K, l.oc,
         bad ? "DIFFERENT from the scalar loop" : "identical to the scalar loop", twin);
  if (!bad) {  // a second submit after the weights changed on the host must re-pack them
    s8 *w2 = (s8 *)wei->data();
    for (size_t i = 0; i < wei->size(); i += 2) w2[i] = (s8)(w2[i] == -128 ? 127 : -w2[i]);
    fc->submit();
    want = scalar_ref(l, (const uint8_t *)src->host_data(), (const s8 *)wei->host_data(), bia ? bia->host_data() : nullptr, sc);
    if (memcmp(want.data(), got->host_data(), want.size()) != 0) {
      printf("fc_check %-14s: DIFFERENT after the weights changed\n", l.name);
      bad = 1;
    }
  }
  return bad;
}

int main() {
  Lcg g(777);
  const auto U = memory::dtype::undef;
  const std::vector<Layer> layers = {
      {"head1000_s8", 3, 256, 1, 1, 1000, memory::dtype::s8, memory::dtype::s32, false, true, round_mode::nearest},
      {"pool7x7_u8", 5, 64, 7, 7, 33, memory::dtype::u8, memory::dtype::f32, false, false, round_mode::nearest},
      {"vec_f32", 33, 192, 1, 1, 10, memory::dtype::f32, U, true, false, round_mode::nearest},
      {"b130_s32", 130, 64, 1, 3, 48, memory::dtype::s32, memory::dtype::s8, false, true, round_mode::down},
      {"twin3x3_u8", 4, 32, 3, 3, 48, memory::dtype::u8, memory::dtype::u8, false, true, round_mode::nearest},
      {"rgb5x5_s8", 2, 3, 5, 5, 7, memory::dtype::s8, memory::dtype::s32, true, false, round_mode::down},
      {"k100_s32", 6, 100, 1, 1, 16, memory::dtype::s32, U, false, false, round_mode::nearest},
  };
  int bad = 0;
  for (const Layer &l : layers) bad += run(l, g);
  if (bad) {
    printf("fc_check: %d of %zu layers FAILED\n", bad, layers.size());
    return 1;
  }
  printf("fc_check: every layer identical to the scalar loop (%zu layers)\n", layers.size());
  return 0;
}
