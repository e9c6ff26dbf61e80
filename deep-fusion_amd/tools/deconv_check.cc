// deconv_check -- runs deepfusion::deconvolution of the drop-in C++ API (include/deepfusion.h) over a few up-conv layers
// and compares every result, byte for byte, with what a caller had to run without it: grouped_conv() with groups = 1,
// stride 1 and padding k - 1 - pad on a zero-stuffed copy of the activation with spatially flipped weights (the op's
// defining property 1).  Exits non-zero on the first difference.  With an output directory it dumps every input and
// result as raw files: the tests compare them with the numpy reference and the DEEPFUSION_DEVICES settings against
// each other.
//   deconv_check [outdir]
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
  int bs, c, oc, ih, iw, k, s, p, oh, ow;  // c: input channels; oh = 0: derived (in - 1) * s - 2 p + k
  memory::dtype dst_dt, bia_dt;            // bia_dt undef: no bias
  bool relu, per_channel;
  round_mode rm;
};

static int run(const Layer &l, Lcg &g, const std::string &out) {
  const auto nhwc = memory::format::nhwc;
  const int oh = l.oh ? l.oh : (l.ih - 1) * l.s - 2 * l.p + l.k, ow = l.ow ? l.ow : (l.iw - 1) * l.s - 2 * l.p + l.k;
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
  for (size_t k = 0; k < sc.size(); ++k) sc[k] = (0.0015f + 0.00002f * (float)k) / (float)(l.c * (l.k + l.s - 1) / l.s) * 6.0f;
  auto got = mk(l.bs, l.oc, oh, ow, nhwc, l.dst_dt);
  memset(got->data(), 0xA5, got->buffer_size());
  auto dc = deconvolution(src, wei, bia, {l.s, l.s}, {l.p, l.p}, got, l.relu, sc, l.rm);
  dc->submit();
  if (!out.empty()) {
    const std::string b = out + "/" + l.name;
    dump(b + "_src.bin", src->host_data(), src->buffer_size());
    dump(b + "_wei.bin", wei->host_data(), wei->buffer_size());
    if (bia) dump(b + "_bia.bin", bia->host_data(), bia->buffer_size());
    dump(b + "_scales.bin", sc.data(), sc.size() * sizeof(float));
    dump(b + "_dst.bin", got->host_data(), got->buffer_size());
  }
  // the twin: the stuffed tensor {bs, (ih-1) s + 1, (iw-1) s + 1, c} and the flipped weights w[o][i][k-1-ky][k-1-kx]
  const int sth = (l.ih - 1) * l.s + 1, stw = (l.iw - 1) * l.s + 1;
  auto stuffed = mk(l.bs, l.c, sth, stw, nhwc, memory::dtype::u8);
  auto fwei = mk(l.oc, l.c, l.k, l.k, memory::format::oihw, memory::dtype::s8);
  auto fill_twin = [&] {
    uint8_t *tp = (uint8_t *)stuffed->data();
    memset(tp, 0, stuffed->buffer_size());
    const uint8_t *hs = (const uint8_t *)src->host_data();
    for (int n = 0; n < l.bs; ++n)
      for (int y = 0; y < l.ih; ++y)
        for (int x = 0; x < l.iw; ++x)
          memcpy(tp + (((size_t)n * sth + (size_t)y * l.s) * stw + (size_t)x * l.s) * l.c, hs + (((size_t)n * l.ih + y) * l.iw + x) * l.c, (size_t)l.c);
    const s8 *w = (const s8 *)wei->host_data();
    s8 *fw = (s8 *)fwei->data();
    const int kk = l.k * l.k;
    for (size_t oi = 0; oi < (size_t)l.oc * l.c; ++oi)
      for (int t = 0; t < kk; ++t) fw[oi * kk + t] = w[oi * kk + (kk - 1 - t)];
  };
  fill_twin();
  auto want = mk(l.bs, l.oc, oh, ow, nhwc, l.dst_dt);
  memset(want->data(), 0x5A, want->buffer_size());
  auto gc = grouped_conv(stuffed, fwei, bia, 1, {1, 1}, {l.k - 1 - l.p, l.k - 1 - l.p}, want, l.relu, sc, l.rm);
  gc->submit();
  size_t bad = memcmp(want->host_data(), got->host_data(), want->buffer_size()) != 0;
  printf("deconv_check %-12s %3d -> %3d %dx%d k%d s%d p%d -> %dx%d: %s\n", l.name, l.c, l.oc, l.ih, l.iw, l.k, l.s, l.p, oh, ow,
         bad ? "DIFFERENT" : "identical");
  // a second submit after the weights changed on the host must re-pack them
  if (!bad) {
    std::vector<unsigned char> before((const unsigned char *)got->host_data(), (const unsigned char *)got->host_data() + got->buffer_size());
    s8 *w2 = (s8 *)wei->data();
    for (size_t i = 0; i < wei->size(); i += 2) w2[i] = (s8)(w2[i] == -128 ? 127 : -w2[i]);
    dc->submit();
    if (memcmp(before.data(), got->host_data(), before.size()) == 0) {
      printf("deconv_check %-12s: UNCHANGED after the weights changed\n", l.name);
      bad = 1;
    }
    if (!bad) {
      fill_twin();
      gc->submit();
      if (memcmp(want->host_data(), got->host_data(), want->buffer_size()) != 0) {
        printf("deconv_check %-12s: DIFFERENT after the weights changed\n", l.name);
        bad = 1;
      }
    }
  }
  return bad ? 1 : 0;
}

int main(int argc, char **argv) {
  const std::string out = argc > 1 ? argv[1] : "";
  Lcg g(6161);
  const auto U = memory::dtype::undef;
  const std::vector<Layer> layers = {
      {"unet_k2_u8", 3, 64, 32, 7, 9, 2, 2, 0, 0, 0, memory::dtype::u8, memory::dtype::s32, false, false, round_mode::nearest},
      {"pose_k4_s8", 4, 32, 64, 5, 6, 4, 2, 1, 0, 0, memory::dtype::s8, U, true, true, round_mode::down},
      {"keras_k3_s32", 5, 32, 32, 6, 5, 3, 2, 1, 12, 10, memory::dtype::s32, memory::dtype::f32, false, true, round_mode::nearest},
      {"gan_k4p0_f32", 3, 64, 96, 4, 4, 4, 2, 0, 0, 0, memory::dtype::f32, memory::dtype::s8, true, false, round_mode::nearest},
      {"crop_k4_u8", 3, 32, 32, 5, 7, 4, 2, 1, 9, 13, memory::dtype::u8, memory::dtype::u8, false, true, round_mode::nearest},
      {"holes_s3_s8", 3, 3, 7, 4, 5, 2, 3, 0, 0, 0, memory::dtype::s8, memory::dtype::s32, false, false, round_mode::nearest},
      {"rgb_k5_u8", 2, 20, 3, 6, 5, 5, 2, 2, 12, 10, memory::dtype::u8, U, false, false, round_mode::nearest},
  };
  int bad = 0;
  for (const Layer &l : layers) bad += run(l, g, out);
  if (bad) {
    printf("deconv_check: %d of %zu layers FAILED\n", bad, layers.size());
    return 1;
  }
  printf("deconv_check: all %zu layers ran, every one identical to grouped_conv() on the stuffed tensor with flipped weights\n", layers.size());
  return 0;
}
