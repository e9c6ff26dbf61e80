// imgconv_check -- runs deepfusion::image_conv of the drop-in C++ API (include/deepfusion.h) over a few first layers and
// compares every result, byte for byte, with what a caller had to run without it: reorder() of the image to 16
// channels followed by conv() on weights zero-padded to 16 input channels (the op's defining property, where the dense
// conv can express the layer: oc % 16 == 0, symmetric padding, derived output size).  Exits non-zero on the first
// difference.  With an output directory it dumps every input and result as raw files: the tests compare them with the
// numpy reference and the DEEPFUSION_DEVICES settings against each other.
//   imgconv_check [outdir]
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
  int bs, c, oc, ih, iw, k, s, p, oh, ow;  // c: input channels; oh = 0: derived (in + 2p - k) / s + 1
  memory::dtype dst_dt, bia_dt;            // bia_dt undef: no bias
  bool relu, per_channel;
  round_mode rm;
};

static int run(const Layer &l, Lcg &g, const std::string &out) {
  const auto nhwc = memory::format::nhwc;
  const bool derived = l.oh == 0;
  const int oh = derived ? (l.ih + 2 * l.p - l.k) / l.s + 1 : l.oh, ow = derived ? (l.iw + 2 * l.p - l.k) / l.s + 1 : l.ow;
  auto src = mk(l.bs, l.c, l.ih, l.iw, nhwc, memory::dtype::u8);
  uint8_t *sp = (uint8_t *)src->data();
  for (size_t i = 0; i < src->size(); ++i) sp[i] = (uint8_t)(g.next() % 256);
  auto wei = mk(l.oc, l.c, l.k, l.k, memory::format::oihw, memory::dtype::s8);
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
  for (size_t k = 0; k < sc.size(); ++k) sc[k] = (0.0015f + 0.00002f * (float)k) / (float)(l.c * l.k) * 6.0f;
  auto got = mk(l.bs, l.oc, oh, ow, nhwc, l.dst_dt);
  memset(got->data(), 0xA5, got->buffer_size());
  auto ic = image_conv(src, wei, bia, {l.s, l.s}, {l.p, l.p}, got, l.relu, sc, l.rm);
  ic->submit();
  if (!out.empty()) {
    const std::string b = out + "/" + l.name;
    dump(b + "_src.bin", src->host_data(), src->buffer_size());
    dump(b + "_wei.bin", wei->host_data(), wei->buffer_size());
    if (bia) dump(b + "_bia.bin", bia->host_data(), bia->buffer_size());
    dump(b + "_scales.bin", sc.data(), sc.size() * sizeof(float));
    dump(b + "_dst.bin", got->host_data(), got->buffer_size());
  }
  size_t bad = 0;
  const bool dense = derived && l.oc % 16 == 0;
  std::unique_ptr<memory> src16, dwei, want;
  std::unique_ptr<op> ro, cv;
  auto fill_dense = [&] {
    std::vector<s8> full((size_t)l.oc * 16 * l.k * l.k, 0);
    const s8 *w = (const s8 *)wei->host_data();
    for (int o = 0; o < l.oc; ++o)  // W[o][i] = w[o][i] for i < c, 0 on the padding channels
      memcpy(&full[(size_t)o * 16 * l.k * l.k], w + (size_t)o * l.c * l.k * l.k, (size_t)l.c * l.k * l.k);
    reorder_weights(full.data(), dwei);
  };
  if (dense) {
    src16 = mk(l.bs, 16, l.ih, l.iw, nhwc, memory::dtype::u8);
    memset(src16->data(), 0x77, src16->buffer_size());
    ro = reorder(src, src16);
    dwei.reset(new memory(memory::nchw_dims{l.oc, 16, l.k, l.k}, memory::format::OIhw4i16o4i, memory::dtype::s8));
    fill_dense();
    want = mk(l.bs, l.oc, oh, ow, nhwc, l.dst_dt);
    memset(want->data(), 0x5A, want->buffer_size());
    cv = conv(src16, dwei, bia, {l.s, l.s}, {l.p, l.p}, want, l.relu, sc, l.rm);
    ro->submit();
    cv->submit();
    if (memcmp(want->host_data(), got->host_data(), want->buffer_size()) != 0) bad = 1;
  }
  printf("imgconv_check %-12s c %d -> %3d %dx%d k%d s%d p%d -> %dx%d: %s\n", l.name, l.c, l.oc, l.ih, l.iw, l.k, l.s, l.p, oh, ow,
         !dense ? "ran (no dense twin)" : bad ? "DIFFERENT" : "identical");
  // a second submit after the weights changed on the host must re-pack them
  if (!bad) {
    std::vector<unsigned char> before((const unsigned char *)got->host_data(), (const unsigned char *)got->host_data() + got->buffer_size());
    s8 *w2 = (s8 *)wei->data();
    for (size_t i = 0; i < wei->size(); i += 2) w2[i] = (s8)(w2[i] == -128 ? 127 : -w2[i]);
    ic->submit();
    if (memcmp(before.data(), got->host_data(), before.size()) == 0) {
      printf("imgconv_check %-12s: UNCHANGED after the weights changed\n", l.name);
      bad = 1;
    }
    if (dense && !bad) {
      fill_dense();
      cv->submit();
      if (memcmp(want->host_data(), got->host_data(), want->buffer_size()) != 0) {
        printf("imgconv_check %-12s: DIFFERENT after the weights changed\n", l.name);
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
  const std::vector<Layer> layers = {
      {"res_k7_u8", 3, 3, 64, 20, 23, 7, 2, 3, 0, 0, memory::dtype::u8, memory::dtype::s32, false, false, round_mode::nearest},
      {"vgg_k3_s8", 4, 3, 64, 9, 11, 3, 1, 1, 0, 0, memory::dtype::s8, U, true, true, round_mode::down},
      {"mob_k3s2_s32", 5, 3, 32, 12, 9, 3, 2, 1, 0, 0, memory::dtype::s32, memory::dtype::f32, false, true, round_mode::nearest},
      {"rgba_k7_f32", 3, 4, 96, 15, 15, 7, 2, 3, 0, 0, memory::dtype::f32, memory::dtype::s8, true, false, round_mode::nearest},
      {"incep_p0_u8", 3, 3, 32, 15, 17, 3, 2, 0, 0, 0, memory::dtype::u8, memory::dtype::u8, false, true, round_mode::nearest},
      {"same_u8", 3, 3, 32, 8, 7, 3, 2, 0, 4, 4, memory::dtype::u8, memory::dtype::u8, false, true, round_mode::nearest},
      {"gray_k5_s8", 3, 1, 48, 9, 9, 5, 1, 2, 0, 0, memory::dtype::s8, memory::dtype::s32, false, false, round_mode::nearest},
      {"alex_k11_u8", 2, 3, 7, 23, 27, 11, 4, 2, 0, 0, memory::dtype::u8, U, false, false, round_mode::nearest},
  };
  int bad = 0;
  for (const Layer &l : layers) bad += run(l, g, out);
  if (bad) {
    printf("imgconv_check: %d of %zu layers FAILED\n", bad, layers.size());
    return 1;
  }
  printf("imgconv_check: all %zu layers ran, every dense twin identical to reorder() + conv() on the padded image\n", layers.size());
  return 0;
}
