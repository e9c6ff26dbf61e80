// catconv_check -- compares deepfusion::concat_conv with concat() -> conv() of the same drop-in C++ API
// (include/deepfusion.h), byte for byte, over a few joins: shapes inside the one-launch kernel's class and outside
// it, every dst type, with and without bias, one and per-channel scales, both round modes.  Exits non-zero on the
// first difference.  With an output directory it also dumps every concat_conv result as a raw file (used to compare
// DEEPFUSION_DEVICES settings against each other).
//   catconv_check [outdir]
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

struct Join {
  const char *name;
  int bs, h, w, oc;
  std::vector<int> ch;
  memory::dtype dst_dt, bia_dt;  // bia_dt undef: no bias
  bool relu, per_channel;
  round_mode rm;
};

static int run(const Join &j, Lcg &g, const std::string &out) {
  const auto nhwc = memory::format::nhwc;
  int ic = 0;
  for (int c : j.ch) ic += c;
  std::vector<std::unique_ptr<memory>> srcs;
  for (int c : j.ch) {
    srcs.push_back(mk(j.bs, c, j.h, j.w, nhwc, memory::dtype::u8));
    uint8_t *p = (uint8_t *)srcs.back()->data();
    for (size_t i = 0; i < srcs.back()->size(); ++i) p[i] = (uint8_t)(g.next() % 256);
  }
  std::unique_ptr<memory> wei(new memory(memory::nchw_dims{j.oc, ic, 1, 1}, memory::format::OIhw4i16o4i, memory::dtype::s8));
  std::vector<s8> w((size_t)j.oc * ic);
  for (auto &v : w) v = (s8)((int)(g.next() % 41) - 20);
  reorder_weights(w.data(), wei);
  std::unique_ptr<memory> bia;
  if (j.bia_dt != memory::dtype::undef) {
    bia.reset(new memory(memory::dims{j.oc}, memory::format::x, j.bia_dt));
    for (int k = 0; k < j.oc; ++k) {
      const int v = (int)(g.next() % 2001) - 1000;
      void *p = bia->data();
      if (j.bia_dt == memory::dtype::f32) ((float *)p)[k] = (float)v * 0.5f;
      else if (j.bia_dt == memory::dtype::s32) ((int32_t *)p)[k] = v;
      else if (j.bia_dt == memory::dtype::s8) ((int8_t *)p)[k] = (int8_t)(v % 128);
      else ((uint8_t *)p)[k] = (uint8_t)(v & 0xff);
    }
  }
  std::vector<float> sc(j.per_channel ? j.oc : 1);
  for (size_t k = 0; k < sc.size(); ++k) sc[k] = 0.002f + 0.0001f * (float)k;
  auto cat = mk(j.bs, ic, j.h, j.w, nhwc, memory::dtype::u8);
  auto want = mk(j.bs, j.oc, j.h, j.w, nhwc, j.dst_dt), got = mk(j.bs, j.oc, j.h, j.w, nhwc, j.dst_dt);
  memset(want->data(), 0x5A, want->buffer_size());
  memset(got->data(), 0xA5, got->buffer_size());
  auto c0 = concat(srcs, cat);
  auto c1 = conv(cat, wei, bia, {1, 1}, {0, 0}, want, j.relu, sc, j.rm);
  auto cc = concat_conv(srcs, wei, bia, got, j.relu, sc, j.rm);
  c0->submit();
  c1->submit();
  cc->submit();
  const unsigned char *a = (const unsigned char *)want->host_data(), *b = (const unsigned char *)got->host_data();
  size_t bad = 0, first = 0;
  for (size_t i = 0; i < want->buffer_size(); ++i)
    if (a[i] != b[i] && bad++ == 0) first = i;
  if (!out.empty()) dump(out + "/" + j.name + "_dst.bin", got->host_data(), got->buffer_size());
  printf("catconv_check %-12s ic %4d oc %3d px %6d: %s", j.name, ic, j.oc, j.bs * j.h * j.w, bad ? "DIFFERENT" : "identical");
  if (bad) printf(" (%zu of %zu bytes, first at %zu: %u vs %u)", bad, want->buffer_size(), first, a[first], b[first]);
  printf("\n");
  // a second submit after the weights changed on the host must re-pack them
  if (!bad) {
    s8 *wp = (s8 *)wei->data();
    for (size_t i = 0; i < wei->size(); i += 7) wp[i] = (s8)(-wp[i]);
    c1->submit();
    cc->submit();
    if (memcmp(want->host_data(), got->host_data(), want->buffer_size()) != 0) {
      printf("catconv_check %-12s: DIFFERENT after the weights changed\n", j.name);
      bad = 1;
    }
  }
  return bad ? 1 : 0;
}

int main(int argc, char **argv) {
  const std::string out = argc > 1 ? argv[1] : "";
  Lcg g(777);
  const auto U = memory::dtype::undef;
  const std::vector<Join> joins = {
      {"pair_u8", 3, 9, 11, 64, {128, 128}, memory::dtype::u8, memory::dtype::s32, false, false, round_mode::nearest},
      {"incept_s8", 4, 7, 5, 128, {64, 128, 32, 32}, memory::dtype::s8, U, true, true, round_mode::down},
      {"dense_s32", 2, 6, 6, 128, {256, 32, 32, 32, 32, 32, 32, 32, 32}, memory::dtype::s32, memory::dtype::f32, false, true, round_mode::nearest},
      {"pair_f32", 5, 4, 9, 256, {224, 32}, memory::dtype::f32, memory::dtype::s8, true, false, round_mode::nearest},
      {"odd16_u8", 3, 5, 7, 64, {16, 48, 192}, memory::dtype::u8, memory::dtype::u8, false, false, round_mode::nearest},
      {"ic384_u8", 3, 5, 7, 64, {128, 256}, memory::dtype::u8, U, true, true, round_mode::nearest},
      {"oc96_s32", 2, 8, 3, 96, {128, 128}, memory::dtype::s32, U, false, false, round_mode::nearest},
  };
  int bad = 0;
  for (const Join &j : joins) bad += run(j, g, out);
  if (bad) {
    printf("catconv_check: %d of %zu joins DIFFER\n", bad, joins.size());
    return 1;
  }
  printf("catconv_check: all %zu joins identical to concat() -> conv()\n", joins.size());
  return 0;
}
