// linear_check -- runs deepfusion::linear of the drop-in C++ API (include/deepfusion.h) and compares every result, bit for
// bit, with the scalar reference of tools/linear_host.h: the sequence of include/dfx.h (exact integer accumulation, one
// separately rounded add and multiply, the x86 conversion, the optional byte table).  One frame chains layer_norm() ->
// linear() (QKV) -> linear() (a projection reading a k_valid slice) on the device with no host step in between, submitted
// asynchronously.  With a directory argument it also runs the cases a test wrote there (cases.txt:
//   case <name> <bs> <C> <h> <w> <k> <n> <dst_C> <src_dt> <dst_dt> <bia_dt> <relu> <rm> <nscales> <lut_in_dt> <async>
// with <name>.src / .wei / .bia / .scales / .lut / .dst beside it; .dst is the expected storage of dst) against BOTH the file
// and the scalar reference.  Prints one line per case, "ok" or "DIFFERENT"; exits non-zero on a difference.
//   linear_check [directory]
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "cli_flags.h"
#include "deepfusion.h"
#include "dfx.h"
#include "linear_host.h"

using namespace deepfusion;
typedef memory::dtype DT;

static std::unique_ptr<memory> mk(int n, int c, int h, int w, DT dt, memory::format f = memory::format::nhwc) {
  return std::unique_ptr<memory>(new memory(memory::nchw_dims{n, c, h, w}, f, dt));
}
static int code(DT dt) { return dt == DT::f32 ? DFX_F32 : dt == DT::s32 ? DFX_S32 : dt == DT::s8 ? DFX_S8 : dt == DT::u8 ? DFX_U8 : DFX_UNDEF; }
static DT dtype_of(int c) { return c == DFX_F32 ? DT::f32 : c == DFX_S32 ? DT::s32 : c == DFX_S8 ? DT::s8 : c == DFX_U8 ? DT::u8 : DT::undef; }
static const char *dname(DT dt) { return dt == DT::f32 ? "f32" : dt == DT::s32 ? "s32" : dt == DT::s8 ? "s8" : dt == DT::u8 ? "u8" : "none"; }

static int report(const char *name, const std::string &what, bool bad) {
  printf("linear_check %-14s %s: %s\n", name, what.c_str(), bad ? "DIFFERENT from the reference" : "ok");
  return bad ? 1 : 0;
}
static void fill(memory &m, Lcg &g) {
  for (size_t i = 0; i < m.buffer_size(); ++i) ((uint8_t *)m.data())[i] = (uint8_t)(g.next() & 0xff);
}
static std::unique_ptr<memory> make_bias(int n, DT dt, double amp, Lcg &g) {
  std::unique_ptr<memory> bia;
  if (dt == DT::undef) return bia;
  bia.reset(new memory(memory::dims{n}, memory::format::x, dt));
  for (int o = 0; o < n; ++o) {
    const double v = ((double)(g.next() % 2001) - 1000.0) * 0.001 * amp;
    if (dt == DT::f32) ((float *)bia->data())[o] = (float)v;
    else if (dt == DT::s32) ((int32_t *)bia->data())[o] = (int32_t)v;
    else ((uint8_t *)bia->data())[o] = (uint8_t)(g.next() & 0xff);
  }
  return bia;
}
// scales that centre a 1-byte output (standard deviation about 40), near 0.37 for a 4-byte one
static std::vector<float> make_scales(int n, int k, DT src_dt, DT req, bool per_channel) {
  const double sd = (src_dt == DT::u8 ? 147.0 : 74.0) * 74.0 * std::sqrt((double)k);
  const float s = (req == DT::f32 || req == DT::s32) ? 0.37f : (float)(40.0 / sd);
  std::vector<float> out;
  if (!per_channel) return out.push_back(s), out;
  for (int o = 0; o < n; ++o) out.push_back(s * (0.5f + (float)o / (float)n));
  return out;
}
static std::vector<u8> make_table(Lcg &g) {  // a permutation of the 256 bytes: a wrong index cannot hide
  std::vector<u8> t(256);
  for (int i = 0; i < 256; ++i) t[i] = (u8)i;
  for (int i = 255; i > 0; --i) std::swap(t[i], t[g.next() % (i + 1)]);
  return t;
}

static int check_linear(const char *name, int bs, int C, int h, int w, int k_valid, int n, int dst_C, DT src_dt, DT dst_dt, DT bia_dt, bool relu,
                        round_mode rm, bool per_channel, DT table_in, bool use_async, Lcg &g) {
  const int k = k_valid ? k_valid : C;
  const long long rows = (long long)bs * h * w;
  auto src = mk(bs, C, h, w, src_dt);
  fill(*src, g);
  auto wei = mk(n, k, 1, 1, DT::s8, memory::format::oihw);
  fill(*wei, g);
  const DT req = table_in != DT::undef ? table_in : dst_dt;
  auto bia = make_bias(n, bia_dt, (src_dt == DT::u8 ? 147.0 : 74.0) * 74.0 * std::sqrt((double)k) / 3.0, g);
  const std::vector<float> scales = make_scales(n, k, src_dt, req, per_channel);
  const std::vector<u8> table = table_in != DT::undef ? make_table(g) : std::vector<u8>();
  auto dst = mk(bs, dst_C, h, w, dst_dt);
  memset(dst->data(), 0xCD, dst->buffer_size());
  std::vector<unsigned char> want(dst->buffer_size(), 0xCD);
  linear_host::reference((const unsigned char *)src->host_data(), code(src_dt), rows, C, k, (const int8_t *)wei->host_data(), n, bia ? bia->host_data() : nullptr,
                         code(bia_dt), scales.data(), (int)scales.size(), relu, rm == round_mode::down ? DFX_ROUND_DOWN : DFX_ROUND_NEAREST, code(dst_dt), dst_C,
                         table.empty() ? nullptr : table.data(), code(table_in), want);
  auto op = linear(src, wei, bia, dst, relu, scales, rm, k_valid, table, table_in);
  if (use_async) {
    op->submit_async();
    op->wait();
    dst->download();
  } else {
    op->submit();
  }
  char what[240];
  snprintf(what, sizeof(what), "bs %d %dx%d k %d/%d -> n %d/%d %s->%s bias %s%s%s%s%s %s", bs, h, w, k, C, n, dst_C, dname(src_dt), dname(dst_dt), dname(bia_dt),
           relu ? " relu" : "", rm == round_mode::down ? " down" : "", per_channel ? " per-n" : "", table.empty() ? "" : " +table", use_async ? "async" : "sync");
  return report(name, what, linear_host::rows_differ(dst->host_data(), want, rows, dst_C, n, linear_host::esize(code(dst_dt))));
}

// layer_norm() -> linear() (QKV, bias) -> linear() (reads the first C channels of the 3C-wide tensor in place), all submitted
// asynchronously: the tokens never leave the device in between
static int frame_norm_qkv_slice(Lcg &g) {
  const int bs = 2, T = 50, C = 64;
  auto src = mk(bs, C, T, 1, DT::s8);
  fill(*src, g);
  auto normed = mk(bs, C, T, 1, DT::s8);
  auto qkv = mk(bs, 3 * C, T, 1, DT::s8);
  auto out = mk(bs, C, T, 1, DT::s32);
  auto w1 = mk(3 * C, C, 1, 1, DT::s8, memory::format::oihw), w2 = mk(C, C, 1, 1, DT::s8, memory::format::oihw);
  fill(*w1, g);
  fill(*w2, g);
  auto b1 = make_bias(3 * C, DT::s32, 20000.0, g);
  std::unique_ptr<memory> none;
  std::vector<float> gamma, beta;
  for (int k = 0; k < C; ++k) {
    gamma.push_back(((float)(g.next() % 2001) - 1000.f) * 0.04f);
    beta.push_back(((float)(g.next() % 2001) - 1000.f) * 0.01f);
  }
  const std::vector<float> s1 = make_scales(3 * C, C, DT::s8, DT::s8, true), s2 = {0.37f};
  auto ln = layer_norm(src, gamma, beta, normed, 0.5f);
  auto l1 = linear(normed, w1, b1, qkv, false, s1);
  auto l2 = linear(qkv, w2, none, out, false, s2, round_mode::nearest, C);
  ln->submit_async();
  l1->submit_async();
  l2->submit_async();
  l2->wait();
  l1->wait();
  ln->wait();
  normed->download();
  qkv->download();
  out->download();
  const long long rows = (long long)bs * T;
  std::vector<unsigned char> wq(qkv->buffer_size(), 0), wo(out->buffer_size(), 0);
  linear_host::reference((const unsigned char *)normed->host_data(), DFX_S8, rows, C, C, (const int8_t *)w1->host_data(), 3 * C, b1->host_data(), DFX_S32,
                         s1.data(), (int)s1.size(), false, DFX_ROUND_NEAREST, DFX_S8, 3 * C, nullptr, DFX_UNDEF, wq);
  linear_host::reference(wq.data(), DFX_S8, rows, 3 * C, C, (const int8_t *)w2->host_data(), C, nullptr, DFX_UNDEF, s2.data(), 1, false, DFX_ROUND_NEAREST,
                         DFX_S32, C, nullptr, DFX_UNDEF, wo);
  const bool bad = memcmp(qkv->host_data(), wq.data(), wq.size()) != 0 || memcmp(out->host_data(), wo.data(), wo.size()) != 0;
  return report("norm->qkv->q", "bs 2 T 50 C 64: layer_norm -> linear 64->192 -> linear on the first 64 of 192, asynchronous", bad);
}

static bool read_file(const std::string &path, std::vector<unsigned char> &out, size_t want) {
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) return false;
  out.resize(want);
  const size_t n = want ? fread(out.data(), 1, want, f) : 0;
  const bool more = fgetc(f) != EOF;
  fclose(f);
  return n == want && !more;
}

static int run_directory(const std::string &dir, int *n_out) {
  FILE *f = fopen((dir + "/cases.txt").c_str(), "r");
  if (!f) { fprintf(stderr, "linear_check: cannot read %s/cases.txt\n", dir.c_str()); return 1; }
  int bad = 0, cnt = 0;
  char name[64];
  int bs, C, h, w, k, n, dst_C, sdt, ddt, bdt, relu, rm, nscales, lut_in, use_async;
  while (fscanf(f, " case %63s %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", name, &bs, &C, &h, &w, &k, &n, &dst_C, &sdt, &ddt, &bdt, &relu, &rm, &nscales,
                &lut_in, &use_async) == 16) {
    const long long rows = (long long)bs * h * w;
    const std::string base = dir + "/" + name;
    std::vector<unsigned char> fs, fw, fb, fsc, fl, fd;
    const size_t dbytes = (size_t)rows * dst_C * linear_host::esize(ddt);
    if (!read_file(base + ".src", fs, (size_t)rows * C) || !read_file(base + ".wei", fw, (size_t)n * k) || !read_file(base + ".dst", fd, dbytes) ||
        !read_file(base + ".scales", fsc, (size_t)nscales * 4) || (bdt != DFX_UNDEF && !read_file(base + ".bia", fb, (size_t)n * linear_host::esize(bdt))) ||
        (lut_in != DFX_UNDEF && !read_file(base + ".lut", fl, 256))) {
      fprintf(stderr, "linear_check: case %s: a file is missing or has the wrong size\n", name);
      fclose(f);
      return 1;
    }
    auto src = mk(bs, C, h, w, dtype_of(sdt));
    memcpy(src->data(), fs.data(), fs.size());
    auto wei = mk(n, k, 1, 1, DT::s8, memory::format::oihw);
    memcpy(wei->data(), fw.data(), fw.size());
    std::unique_ptr<memory> bia;
    if (bdt != DFX_UNDEF) {
      bia.reset(new memory(memory::dims{n}, memory::format::x, dtype_of(bdt)));
      memcpy(bia->data(), fb.data(), fb.size());
    }
    auto dst = mk(bs, dst_C, h, w, dtype_of(ddt));
    memset(dst->data(), 0xCD, dst->buffer_size());
    const std::vector<float> scales((const float *)fsc.data(), (const float *)fsc.data() + nscales);
    const std::vector<u8> table(fl.begin(), fl.end());
    std::vector<unsigned char> want(dbytes, 0xCD);
    linear_host::reference(fs.data(), sdt, rows, C, k, (const int8_t *)fw.data(), n, bdt != DFX_UNDEF ? fb.data() : nullptr, bdt, scales.data(), nscales, relu != 0,
                           rm, ddt, dst_C, lut_in != DFX_UNDEF ? fl.data() : nullptr, lut_in, want);
    auto op = linear(src, wei, bia, dst, relu != 0, scales, rm ? round_mode::down : round_mode::nearest, k == C ? 0 : k, table, dtype_of(lut_in));
    if (use_async) {
      op->submit_async();
      op->wait();
      dst->download();
    } else {
      op->submit();
    }
    const size_t es = linear_host::esize(ddt);
    const bool b_file = linear_host::rows_differ(dst->host_data(), fd, rows, dst_C, n, es);
    const bool b_ref = linear_host::rows_differ(dst->host_data(), want, rows, dst_C, n, es);
    char what[200];
    snprintf(what, sizeof(what), "bs %d %dx%d k %d/%d n %d/%d %s%s%s%s", bs, h, w, k, C, n, dst_C, lut_in != DFX_UNDEF ? "+table " : "", use_async ? "async" : "sync",
             b_file ? " [file differs]" : "", b_ref ? " [scalar reference differs]" : "");
    bad += report(name, what, b_file || b_ref);
    ++cnt;
  }
  fclose(f);
  *n_out = cnt;
  return bad;
}

int main(int argc, char **argv) {
  Lcg g(1301);
  const round_mode rn = round_mode::nearest, rd = round_mode::down;
  int bad = 0, n = 0;
  bad += check_linear("qkv", 2, 64, 50, 1, 0, 192, 192, DT::s8, DT::s8, DT::s32, false, rn, true, DT::undef, true, g); ++n;
  bad += check_linear("proj k_valid", 2, 192, 50, 1, 64, 64, 64, DT::s8, DT::s8, DT::f32, false, rn, false, DT::undef, true, g); ++n;
  bad += check_linear("fc1 +table", 2, 64, 50, 1, 0, 256, 256, DT::s8, DT::s8, DT::s32, false, rn, false, DT::s8, true, g); ++n;
  bad += check_linear("fc2 u8", 2, 256, 50, 1, 0, 64, 64, DT::u8, DT::s8, DT::s8, false, rd, true, DT::undef, false, g); ++n;
  bad += check_linear("swin window", 3, 96, 7, 7, 0, 288, 288, DT::s8, DT::u8, DT::u8, false, rn, false, DT::undef, true, g); ++n;
  bad += check_linear("odd sizes", 3, 21, 4, 5, 0, 33, 35, DT::u8, DT::s32, DT::undef, true, rn, true, DT::undef, false, g); ++n;
  bad += check_linear("f32 padded", 1, 100, 3, 3, 100, 7, 9, DT::s8, DT::f32, DT::s32, true, rd, false, DT::undef, true, g); ++n;
  bad += check_linear("one by one", 5, 1, 1, 1, 0, 1, 1, DT::u8, DT::u8, DT::undef, false, rn, false, DT::u8, false, g); ++n;
  bad += frame_norm_qkv_slice(g); ++n;
  if (argc > 1) {
    int m = 0;
    bad += run_directory(argv[1], &m);
    printf("linear_check: %d entries from %s\n", m, argv[1]);
    n += m;
  }
  if (bad) {
    printf("linear_check: %d of %d cases FAILED\n", bad, n);
    return 1;
  }
  printf("linear_check: every case identical to the reference (%d cases)\n", n);
  return 0;
}
