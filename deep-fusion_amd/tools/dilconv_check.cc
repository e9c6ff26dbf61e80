// dilconv_check -- runs deepfusion::dilated_conv of the drop-in C++ API (include/deepfusion.h) over a few dilated layers
// and compares every result, byte for byte, with what a caller had to run without it: grouped_conv() with groups = 1 on
// the zero-stuffed ((k - 1) d + 1)^2 window (the op's defining property 1).  Exits non-zero on the first difference.
// With an output directory it dumps every input and result as raw files: the tests compare them with the numpy
// reference and the DEEPFUSION_DEVICES settings against each other.
//   dilconv_check [outdir]
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
  int bs, c, oc, ih, iw, k, s, dh, dw, pt, pl, oh, ow;  // c: input channels; oh = 0: derived (in + 2 p - ((k-1) d + 1)) / s + 1
  memory::dtype dst_dt, bia_dt;                         // bia_dt undef: no bias
  bool relu, per_channel;
  round_mode rm;
};

static int run(const Layer &l, Lcg &g, const std::string &out) {
  const auto nhwc = memory::format::nhwc;
  const int eh = (l.k - 1) * l.dh + 1, ew = (l.k - 1) * l.dw + 1;  // the stuffed window
  const int oh = l.oh ? l.oh : (l.ih + 2 * l.pt - eh) / l.s + 1, ow = l.ow ? l.ow : (l.iw + 2 * l.pl - ew) / l.s + 1;
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
  auto dc = dilated_conv(src, wei, bia, {l.s, l.s}, {l.dh, l.dw}, {l.pt, l.pl}, got, l.relu, sc, l.rm);
  dc->submit();
  if (!out.empty()) {
    const std::string b = out + "/" + l.name;
    dump(b + "_src.bin", src->host_data(), src->buffer_size());
    dump(b + "_wei.bin", wei->host_data(), wei->buffer_size());
    if (bia) dump(b + "_bia.bin", bia->host_data(), bia->buffer_size());
    dump(b + "_scales.bin", sc.data(), sc.size() * sizeof(float));
    dump(b + "_dst.bin", got->host_data(), got->buffer_size());
  }
  // the twin: the zero-stuffed weights wz[o][i][ky dh][kx dw] = w[o][i][ky][kx], where grouped_conv accepts the window
  const bool twin = (long long)eh * ew * l.c <= 65025;
  if (!twin) {
    printf("dilconv_check %-12s %3d -> %3d %dx%d k%d s%d d%dx%d p%d,%d -> %dx%d: ran (the stuffed window is not expressible)\n", l.name, l.c,
           l.oc, l.ih, l.iw, l.k, l.s, l.dh, l.dw, l.pt, l.pl, oh, ow);
    return 0;
  }
  auto zwei = mk(l.oc, l.c, eh, ew, memory::format::oihw, memory::dtype::s8);
  auto fill_twin = [&] {
    const s8 *w = (const s8 *)wei->host_data();
    s8 *zw = (s8 *)zwei->data();
    memset(zw, 0, zwei->buffer_size());
    for (size_t oi = 0; oi < (size_t)l.oc * l.c; ++oi)
      for (int ky = 0; ky < l.k; ++ky)
        for (int kx = 0; kx < l.k; ++kx) zw[(oi * eh + (size_t)ky * l.dh) * ew + (size_t)kx * l.dw] = w[(oi * l.k + ky) * l.k + kx];
  };
  fill_twin();
  auto want = mk(l.bs, l.oc, oh, ow, nhwc, l.dst_dt);
  memset(want->data(), 0x5A, want->buffer_size());
  auto gc = grouped_conv(src, zwei, bia, 1, {l.s, l.s}, {l.pt, l.pl}, want, l.relu, sc, l.rm);
  gc->submit();
  size_t bad = memcmp(want->host_data(), got->host_data(), want->buffer_size()) != 0;
  printf("dilconv_check %-12s %3d -> %3d %dx%d k%d s%d d%dx%d p%d,%d -> %dx%d: %s\n", l.name, l.c, l.oc, l.ih, l.iw, l.k, l.s, l.dh, l.dw,
         l.pt, l.pl, oh, ow, bad ? "DIFFERENT" : "identical");
  // a second submit after the weights changed on the host must re-pack them
  if (!bad) {
    std::vector<unsigned char> before((const unsigned char *)got->host_data(), (const unsigned char *)got->host_data() + got->buffer_size());
    s8 *w2 = (s8 *)wei->data();
    for (size_t i = 0; i < wei->size(); i += 2) w2[i] = (s8)(w2[i] == -128 ? 127 : -w2[i]);
    dc->submit();
    if (memcmp(before.data(), got->host_data(), before.size()) == 0) {
      printf("dilconv_check %-12s: UNCHANGED after the weights changed\n", l.name);
      bad = 1;
    }
    if (!bad) {
      fill_twin();
      gc->submit();
      if (memcmp(want->host_data(), got->host_data(), want->buffer_size()) != 0) {
        printf("dilconv_check %-12s: DIFFERENT after the weights changed\n", l.name);
        bad = 1;
      }
    }
  }
  return bad ? 1 : 0;
}

int main(int argc, char **argv) {
  const std::string out = argc > 1 ? argv[1] : "";
  Lcg g(7272);
  const auto U = memory::dtype::undef;
  const std::vector<Layer> layers = {
      {"aspp_d2_u8", 3, 64, 32, 9, 7, 3, 1, 2, 2, 2, 2, 0, 0, memory::dtype::u8, memory::dtype::s32, false, false, round_mode::nearest},
      {"aspp_d6_s8", 4, 32, 160, 8, 8, 3, 1, 6, 6, 6, 6, 0, 0, memory::dtype::s8, U, true, true, round_mode::down},
      {"slabs_s32", 5, 96, 32, 6, 5, 3, 1, 3, 1, 1, 0, 0, 0, memory::dtype::s32, memory::dtype::f32, false, true, round_mode::nearest},
      {"crop_f32", 3, 32, 64, 11, 9, 3, 1, 2, 5, 0, 0, 6, 3, memory::dtype::f32, memory::dtype::s8, true, false, round_mode::nearest},
      {"far_d18_u8", 2, 64, 32, 7, 5, 3, 1, 18, 18, 18, 18, 0, 0, memory::dtype::u8, memory::dtype::u8, false, true, round_mode::nearest},
      {"s2_k5_d3_s8", 3, 3, 5, 15, 14, 5, 2, 3, 3, 6, 6, 0, 0, memory::dtype::s8, memory::dtype::s32, false, false, round_mode::nearest},
      {"odd_k3_u8", 2, 20, 7, 6, 5, 3, 1, 2, 2, 2, 2, 0, 0, memory::dtype::u8, U, false, false, round_mode::nearest},
  };
  int bad = 0;
  for (const Layer &l : layers) bad += run(l, g, out);
  if (bad) {
    printf("dilconv_check: %d of %zu layers FAILED\n", bad, layers.size());
    return 1;
  }
  printf("dilconv_check: all %zu layers ran, every one identical to grouped_conv() on the zero-stuffed window where that exists\n", layers.size());
  return 0;
}
