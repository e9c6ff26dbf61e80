// dwpw_check -- runs deepfusion::depthwise_separable_conv of the drop-in C++ API (include/deepfusion.h) over a few
// layers, with shapes inside and outside the one-launch kernel's class, and compares every result, byte for byte, with
// depthwise_conv() (u8) followed by the 1x1 conv() of the same API: the op's defining property.  The C++ layer leaves
// the path to the library's auto rule, which today takes two launches for all of them; the one-launch kernel is tested
// through the C ABI (tests/test_gpu_dwpw.py).  Exits non-zero on the first difference.  With an output directory it
// dumps every input and result as raw files: the tests compare them with the numpy reference and the
// DEEPFUSION_DEVICES settings against each other.
//   dwpw_check [outdir]
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "cli_flags.h"
#include "deepfusion.h"

using namespace deepfusion;

static void dump(const std::string &path, const void *p, size_t bytes) {
  FILE *f = fopen(path.c_str(), "wb");
  if (!f || fwrite(p, 1, bytes, f) != bytes) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(2); }
  fclose(f);
}

static std::unique_ptr<memory> mk(int n, int c, int h, int w, memory::format fmt, memory::dtype dt) {
  return std::unique_ptr<memory>(new memory(memory::nchw_dims{n, c, h, w}, fmt, dt));
}

struct Layer {
  const char *name;
  int bs, c, ih, iw, k, s, p, oh, ow, oc;  // oh = 0: derived (in + 2p - k) / s + 1
  memory::dtype dst_dt, bia0_dt, bia1_dt;  // undef: no bias
  bool relu, per_channel0, per_channel1;
  round_mode rm0, rm1;
};

static std::unique_ptr<memory> mk_bias(int n, memory::dtype dt, Lcg &g) {
  std::unique_ptr<memory> bia;
  if (dt == memory::dtype::undef) return bia;
  bia.reset(new memory(memory::dims{n}, memory::format::x, dt));
  void *p = bia->data();
  for (int k = 0; k < n; ++k) {
    const int v = (int)(g.next() % 2001) - 1000;
    if (dt == memory::dtype::f32) ((float *)p)[k] = (float)v * 0.5f;
    else if (dt == memory::dtype::s32) ((int32_t *)p)[k] = v;
    else if (dt == memory::dtype::s8) ((int8_t *)p)[k] = (int8_t)(v % 128);
    else ((uint8_t *)p)[k] = (uint8_t)(v & 0xff);
  }
  return bia;
}

static int run(const Layer &l, Lcg &g, const std::string &out) {
  const auto nhwc = memory::format::nhwc;
  const bool derived = l.oh == 0;
  const int oh = derived ? (l.ih + 2 * l.p - l.k) / l.s + 1 : l.oh, ow = derived ? (l.iw + 2 * l.p - l.k) / l.s + 1 : l.ow;
  auto src = mk(l.bs, l.c, l.ih, l.iw, nhwc, memory::dtype::u8);
  uint8_t *sp = (uint8_t *)src->data();
  for (size_t i = 0; i < src->size(); ++i) sp[i] = (uint8_t)(g.next() % 256);
  auto wei = mk(l.c, 1, l.k, l.k, memory::format::oihw, memory::dtype::s8);
  s8 *wp = (s8 *)wei->data();
  for (size_t i = 0; i < wei->size(); ++i) wp[i] = (s8)((int)(g.next() % 256) - 128);
  std::vector<s8> w1((size_t)l.oc * l.c);
  for (auto &v : w1) v = (s8)((int)(g.next() % 256) - 128);
  auto wei_pw = mk(l.oc, l.c, 1, 1, memory::format::OIhw4i16o4i, memory::dtype::s8);
  reorder_weights(w1.data(), wei_pw);
  auto bia0 = mk_bias(l.c, l.bia0_dt, g), bia1 = mk_bias(l.oc, l.bia1_dt, g);
  std::vector<float> sc0(l.per_channel0 ? l.c : 1), sc1(l.per_channel1 ? l.oc : 1);
  for (size_t k = 0; k < sc0.size(); ++k) sc0[k] = 0.0015f + 0.00002f * (float)k;
  for (size_t k = 0; k < sc1.size(); ++k) sc1[k] = 0.0004f + 0.000002f * (float)k;
  auto got = mk(l.bs, l.oc, oh, ow, nhwc, l.dst_dt);
  memset(got->data(), 0xA5, got->buffer_size());
  auto op = depthwise_separable_conv(src, wei, bia0, {l.s, l.s}, {l.p, l.p}, wei_pw, bia1, got, l.relu, sc0, sc1, l.rm0, l.rm1);
  op->submit();
  if (!out.empty()) {
    const std::string b = out + "/" + l.name;
    dump(b + "_src.bin", src->host_data(), src->buffer_size());
    dump(b + "_wdw.bin", wei->host_data(), wei->buffer_size());
    dump(b + "_wpw.bin", w1.data(), w1.size());
    if (bia0) dump(b + "_bia0.bin", bia0->host_data(), bia0->buffer_size());
    if (bia1) dump(b + "_bia1.bin", bia1->host_data(), bia1->buffer_size());
    dump(b + "_scales0.bin", sc0.data(), sc0.size() * sizeof(float));
    dump(b + "_scales1.bin", sc1.data(), sc1.size() * sizeof(float));
    dump(b + "_dst.bin", got->host_data(), got->buffer_size());
  }
  // the two ops
  auto mid = mk(l.bs, l.c, oh, ow, nhwc, memory::dtype::u8);
  auto want = mk(l.bs, l.oc, oh, ow, nhwc, l.dst_dt);
  memset(want->data(), 0x5A, want->buffer_size());
  auto dw = depthwise_conv(src, wei, bia0, {l.s, l.s}, {l.p, l.p}, mid, true, sc0, l.rm0);
  auto pw = conv(mid, wei_pw, bia1, {1, 1}, {0, 0}, want, l.relu, sc1, l.rm1);
  dw->submit();
  pw->submit();
  size_t bad = memcmp(want->host_data(), got->host_data(), want->buffer_size()) != 0;
  printf("dwpw_check %-12s c %4d -> oc %4d %dx%d k%d s%d p%d -> %dx%d: %s\n", l.name, l.c, l.oc, l.ih, l.iw, l.k, l.s, l.p, oh, ow,
         bad ? "DIFFERENT" : "identical");
  // a second submit after the weights changed on the host must re-pack them
  if (!bad) {
    std::vector<unsigned char> before((const unsigned char *)got->host_data(), (const unsigned char *)got->host_data() + got->buffer_size());
    s8 *w2 = (s8 *)wei->data();
    for (size_t i = 0; i < wei->size(); i += 2) w2[i] = (s8)(w2[i] == -128 ? 127 : -w2[i]);
    op->submit();
    if (memcmp(before.data(), got->host_data(), before.size()) == 0) {
      printf("dwpw_check %-12s: UNCHANGED after the weights changed\n", l.name);
      bad = 1;
    }
    if (!bad) {
      dw->submit();
      pw->submit();
      if (memcmp(want->host_data(), got->host_data(), want->buffer_size()) != 0) {
        printf("dwpw_check %-12s: DIFFERENT after the weights changed\n", l.name);
        bad = 1;
      }
    }
  }
  return bad ? 1 : 0;
}

int main(int argc, char **argv) {
  const std::string out = argc > 1 ? argv[1] : "";
  Lcg g(5151);
  const auto U = memory::dtype::undef;
  const auto N = round_mode::nearest, D = round_mode::down;
  const std::vector<Layer> layers = {
      {"s1_u8", 3, 32, 9, 11, 3, 1, 1, 0, 0, 64, memory::dtype::u8, memory::dtype::s32, memory::dtype::s32, false, false, false, N, N},
      {"s2_s8", 4, 64, 8, 7, 3, 2, 1, 0, 0, 128, memory::dtype::s8, U, memory::dtype::s8, true, true, true, D, N},
      {"same_s32", 3, 32, 8, 7, 3, 2, 0, 4, 4, 64, memory::dtype::s32, memory::dtype::u8, memory::dtype::f32, false, true, false, N, D},
      {"c96_f32", 3, 96, 7, 45, 3, 1, 1, 0, 0, 256, memory::dtype::f32, memory::dtype::s8, memory::dtype::s32, true, false, true, N, N},
      {"k5_u8", 5, 48, 6, 9, 5, 1, 2, 0, 0, 32, memory::dtype::u8, memory::dtype::s32, U, false, false, false, N, N},
      {"oc96_s8", 3, 32, 5, 5, 3, 1, 1, 0, 0, 96, memory::dtype::s8, memory::dtype::f32, memory::dtype::s32, false, true, true, N, N},
  };
  int bad = 0;
  for (const Layer &l : layers) bad += run(l, g, out);
  if (bad) {
    printf("dwpw_check: %d of %zu layers FAILED\n", bad, layers.size());
    return 1;
  }
  printf("dwpw_check: all %zu layers ran, every one identical to depthwise_conv() + conv()\n", layers.size());
  return 0;
}
