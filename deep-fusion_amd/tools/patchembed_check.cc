// patchembed_check -- runs deepfusion::patch_embed of the drop-in C++ API (include/deepfusion.h) and compares every result, bit
// for bit, with the scalar reference of tools/patchembed_host.h: the sequence of include/dfx.h (exact integer accumulation, one
// separately rounded add of the bias or the token table and one multiply, the x86 conversion), the token layout and the prefix
// rows.  One frame chains patch_embed() -> layer_norm() -> linear() on the device with no host step in between, submitted
// asynchronously (one op after the other through the host under DEEPFUSION_DEVICES).  With a directory argument it also runs the cases a test wrote there (cases.txt:
//   case <name> <bs> <ic> <ih> <iw> <ph> <pw> <oc> <dst_C> <H> <W> <t0> <src_dt> <dst_dt> <bia_dt> <relu> <rm> <nscales> <table> <prefix> <async>
// with <name>.src / .wei / .bia / .scales / .table / .prefix / .dst beside it; .dst is the expected storage of dst) against BOTH
// the file and the scalar reference.  Under DEEPFUSION_DEVICES=n every op is sharded over the batch.  Prints one line per case,
// "ok" or "DIFFERENT"; exits non-zero on a difference.
//   patchembed_check [directory]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "cli_flags.h"
#include "deepfusion.h"
#include "dfx.h"
#include "patchembed_host.h"

using namespace deepfusion;
typedef memory::dtype DT;

static std::unique_ptr<memory> mk(int n, int c, int h, int w, DT dt, memory::format f = memory::format::nhwc) {
  return std::unique_ptr<memory>(new memory(memory::nchw_dims{n, c, h, w}, f, dt));
}
static int code(DT dt) { return dt == DT::f32 ? DFX_F32 : dt == DT::s32 ? DFX_S32 : dt == DT::s8 ? DFX_S8 : dt == DT::u8 ? DFX_U8 : DFX_UNDEF; }
static DT dtype_of(int c) { return c == DFX_F32 ? DT::f32 : c == DFX_S32 ? DT::s32 : c == DFX_S8 ? DT::s8 : c == DFX_U8 ? DT::u8 : DT::undef; }
static const char *dname(DT dt) { return dt == DT::f32 ? "f32" : dt == DT::s32 ? "s32" : dt == DT::s8 ? "s8" : dt == DT::u8 ? "u8" : "none"; }

static int report(const char *name, const std::string &what, bool bad) {
  printf("patchembed_check %-14s %s: %s\n", name, what.c_str(), bad ? "DIFFERENT from the reference" : "ok");
  return bad ? 1 : 0;
}
static void fill(memory &m, Lcg &g) {
  for (size_t i = 0; i < m.buffer_size(); ++i) ((uint8_t *)m.data())[i] = (uint8_t)(g.next() & 0xff);
}
static double acc_sd(DT src_dt, int k) { return (src_dt == DT::u8 ? 147.0 : 74.0) * 74.0 * std::sqrt((double)k); }
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
static std::vector<float> make_scales(int n, int k, DT src_dt, DT dst_dt, bool per_channel) {
  const float s = (dst_dt == DT::f32 || dst_dt == DT::s32) ? 0.37f : (float)(40.0 / acc_sd(src_dt, k));
  std::vector<float> out;
  if (!per_channel) return out.push_back(s), out;
  for (int o = 0; o < n; ++o) out.push_back(s * (0.5f + (float)o / (float)n));
  return out;
}

static void run(op &o, memory &dst, bool use_async) {
  if (use_async) {
    o.submit_async();
    o.wait();
    dst.download();
  } else {
    o.submit();
  }
}

static int check_embed(const char *name, int bs, int ic, int ih, int iw, int ph, int pw, int oc, int dst_C, int t0, int slack, DT src_dt, DT dst_dt, DT bia_dt,
                       bool relu, round_mode rm, bool per_channel, bool with_table, bool with_prefix, bool use_async, Lcg &g) {
  const int th = ih / ph, tw = iw / pw, k = ph * pw * ic;
  const int img_rows = t0 + th * tw + slack;
  auto src = mk(bs, ic, ih, iw, src_dt);
  fill(*src, g);
  auto wei = mk(oc, ic, ph, pw, DT::s8, memory::format::oihw);
  fill(*wei, g);
  auto bia = make_bias(oc, with_table ? DT::undef : bia_dt, acc_sd(src_dt, k) / 3.0, g);
  const std::vector<float> scales = make_scales(oc, k, src_dt, dst_dt, per_channel);
  std::vector<float> table;
  if (with_table)
    for (int i = 0; i < th * tw * oc; ++i) table.push_back((float)(((double)(g.next() % 2001) - 1000.0) * 0.001 * acc_sd(src_dt, k) / 3.0));
  std::vector<u8> prefix;
  const size_t es = patchembed_host::esize(code(dst_dt));
  if (with_prefix)
    for (size_t i = 0; i < (size_t)t0 * oc * es; ++i) prefix.push_back((u8)(dst_dt == DT::f32 && i % 4 == 3 ? 0x41 : g.next() & 0xff));  // (finite floats)
  auto dst = mk(bs, dst_C, img_rows, 1, dst_dt);
  memset(dst->data(), 0xCD, dst->buffer_size());
  std::vector<unsigned char> want(dst->buffer_size(), 0xCD);
  patchembed_host::reference((const unsigned char *)src->host_data(), code(src_dt), bs, ih, iw, ic, ph, pw, (const int8_t *)wei->host_data(), oc,
                             bia ? bia->host_data() : nullptr, bia ? code(bia_dt) : DFX_UNDEF, table.empty() ? nullptr : table.data(), scales.data(), (int)scales.size(),
                             relu, rm == round_mode::down ? DFX_ROUND_DOWN : DFX_ROUND_NEAREST, code(dst_dt), t0, img_rows, dst_C,
                             prefix.empty() ? nullptr : prefix.data(), want);
  auto o = patch_embed(src, wei, bia, dst, relu, scales, rm, table, t0, prefix);
  run(*o, *dst, use_async);
  char what[260];
  snprintf(what, sizeof(what), "bs %d %dx%dx%d / %dx%d -> %d tokens of %d/%d, t0 %d rows %d %s->%s bias %s%s%s%s%s%s %s", bs, ih, iw, ic, ph, pw, th * tw, oc, dst_C, t0,
           img_rows, dname(src_dt), dname(dst_dt), bia ? dname(bia_dt) : "none", relu ? " relu" : "", rm == round_mode::down ? " down" : "", per_channel ? " per-oc" : "",
           with_table ? " +table" : "", with_prefix ? " +prefix" : "", use_async ? "async" : "sync");
  return report(name, what, patchembed_host::written_differ(dst->host_data(), want, bs, img_rows, t0, (long long)th * tw, with_prefix, dst_C, oc, es));
}

// patch_embed() (class token, position table) -> layer_norm() -> linear(), all submitted asynchronously: the tokens never leave
// the device in between
static int frame_embed_norm_linear(Lcg &g) {
  const int bs = 2, S = 32, P = 4, C = 64, T = (S / P) * (S / P), R = T + 1;
  auto img = mk(bs, 3, S, S, DT::u8);
  fill(*img, g);
  auto wei = mk(C, 3, P, P, DT::s8, memory::format::oihw);
  fill(*wei, g);
  auto tokens = mk(bs, C, R, 1, DT::s8);
  auto normed = mk(bs, C, R, 1, DT::s8);
  auto out = mk(bs, 2 * C, R, 1, DT::s32);
  auto w1 = mk(2 * C, C, 1, 1, DT::s8, memory::format::oihw);
  fill(*w1, g);
  std::unique_ptr<memory> none;
  std::vector<float> table, gamma, beta;
  for (int i = 0; i < T * C; ++i) table.push_back((float)(((double)(g.next() % 2001) - 1000.0) * 0.001 * acc_sd(DT::u8, 48) / 3.0));
  std::vector<u8> prefix;
  for (int i = 0; i < C; ++i) prefix.push_back((u8)(g.next() & 0xff));
  for (int k = 0; k < C; ++k) {
    gamma.push_back(((float)(g.next() % 2001) - 1000.f) * 0.04f);
    beta.push_back(((float)(g.next() % 2001) - 1000.f) * 0.01f);
  }
  const std::vector<float> s0 = make_scales(C, 48, DT::u8, DT::s8, true), s1 = {0.37f};
  auto pe = patch_embed(img, wei, none, tokens, false, s0, round_mode::nearest, table, 1, prefix);
  auto ln = layer_norm(tokens, gamma, beta, normed, 0.5f);
  auto l1 = linear(normed, w1, none, out, false, s1);
  const char *shards = getenv("DEEPFUSION_DEVICES");
  if (shards && *shards) {  // sharded ops work host to host: the chain runs through the host tensors
    pe->submit();
    ln->submit();
    l1->submit();
  } else {
    pe->submit_async();
    ln->submit_async();
    l1->submit_async();
    l1->wait();
    ln->wait();
    pe->wait();
    tokens->download();
    normed->download();
    out->download();
  }
  std::vector<unsigned char> wt(tokens->buffer_size(), 0), wo(out->buffer_size(), 0);
  patchembed_host::reference((const unsigned char *)img->host_data(), DFX_U8, bs, S, S, 3, P, P, (const int8_t *)wei->host_data(), C, nullptr, DFX_UNDEF, table.data(),
                             s0.data(), (int)s0.size(), false, DFX_ROUND_NEAREST, DFX_S8, 1, R, C, prefix.data(), wt);
  linear_host::reference((const unsigned char *)normed->host_data(), DFX_S8, (long long)bs * R, C, C, (const int8_t *)w1->host_data(), 2 * C, nullptr, DFX_UNDEF,
                         s1.data(), 1, false, DFX_ROUND_NEAREST, DFX_S32, 2 * C, nullptr, DFX_UNDEF, wo);
  const bool bad = memcmp(tokens->host_data(), wt.data(), wt.size()) != 0 || memcmp(out->host_data(), wo.data(), wo.size()) != 0;
  return report("embed->norm->fc", "bs 2 32x32x3 / 4x4 -> 1 + 64 tokens of 64: patch_embed -> layer_norm -> linear 64->128, asynchronous", bad);
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
  if (!f) { fprintf(stderr, "patchembed_check: cannot read %s/cases.txt\n", dir.c_str()); return 1; }
  int bad = 0, cnt = 0;
  char name[64];
  int bs, ic, ih, iw, ph, pw, oc, dst_C, H, W, t0, sdt, ddt, bdt, relu, rm, nscales, has_table, has_prefix, use_async;
  while (fscanf(f, " case %63s %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", name, &bs, &ic, &ih, &iw, &ph, &pw, &oc, &dst_C, &H, &W, &t0, &sdt, &ddt,
                &bdt, &relu, &rm, &nscales, &has_table, &has_prefix, &use_async) == 21) {
    const int th = ih / ph, tw = iw / pw;
    const long long img_rows = (long long)H * W;
    const size_t es = patchembed_host::esize(ddt);
    const std::string base = dir + "/" + name;
    std::vector<unsigned char> fs, fw, fb, fsc, ft, fp, fd;
    const size_t dbytes = (size_t)bs * img_rows * dst_C * es;
    if (!read_file(base + ".src", fs, (size_t)bs * ih * iw * ic) || !read_file(base + ".wei", fw, (size_t)oc * ic * ph * pw) || !read_file(base + ".dst", fd, dbytes) ||
        !read_file(base + ".scales", fsc, (size_t)nscales * 4) || (bdt != DFX_UNDEF && !read_file(base + ".bia", fb, (size_t)oc * patchembed_host::esize(bdt))) ||
        (has_table && !read_file(base + ".table", ft, (size_t)th * tw * oc * 4)) || (has_prefix && !read_file(base + ".prefix", fp, (size_t)t0 * oc * es))) {
      fprintf(stderr, "patchembed_check: case %s: a file is missing or has the wrong size\n", name);
      fclose(f);
      return 1;
    }
    auto src = mk(bs, ic, ih, iw, dtype_of(sdt));
    memcpy(src->data(), fs.data(), fs.size());
    auto wei = mk(oc, ic, ph, pw, DT::s8, memory::format::oihw);
    memcpy(wei->data(), fw.data(), fw.size());
    std::unique_ptr<memory> bia;
    if (bdt != DFX_UNDEF) {
      bia.reset(new memory(memory::dims{oc}, memory::format::x, dtype_of(bdt)));
      memcpy(bia->data(), fb.data(), fb.size());
    }
    auto dst = mk(bs, dst_C, H, W, dtype_of(ddt));
    memset(dst->data(), 0xCD, dst->buffer_size());
    const std::vector<float> scales((const float *)fsc.data(), (const float *)fsc.data() + nscales);
    const std::vector<float> table((const float *)ft.data(), (const float *)ft.data() + ft.size() / 4);
    const std::vector<u8> prefix(fp.begin(), fp.end());
    std::vector<unsigned char> want(dbytes, 0xCD);
    patchembed_host::reference(fs.data(), sdt, bs, ih, iw, ic, ph, pw, (const int8_t *)fw.data(), oc, bdt != DFX_UNDEF ? fb.data() : nullptr, bdt,
                               has_table ? table.data() : nullptr, scales.data(), nscales, relu != 0, rm, ddt, t0, img_rows, dst_C, has_prefix ? fp.data() : nullptr, want);
    auto o = patch_embed(src, wei, bia, dst, relu != 0, scales, rm ? round_mode::down : round_mode::nearest, table, t0, prefix);
    run(*o, *dst, use_async != 0);
    const bool b_file = patchembed_host::written_differ(dst->host_data(), fd, bs, img_rows, t0, (long long)th * tw, has_prefix != 0, dst_C, oc, es);
    const bool b_ref = patchembed_host::written_differ(dst->host_data(), want, bs, img_rows, t0, (long long)th * tw, has_prefix != 0, dst_C, oc, es);
    char what[200];
    snprintf(what, sizeof(what), "bs %d %dx%dx%d / %dx%d oc %d/%d t0 %d %s%s%s%s%s", bs, ih, iw, ic, ph, pw, oc, dst_C, t0, has_table ? "+table " : "",
             has_prefix ? "+prefix " : "", use_async ? "async" : "sync", b_file ? " [file differs]" : "", b_ref ? " [scalar reference differs]" : "");
    bad += report(name, what, b_file || b_ref);
    ++cnt;
  }
  fclose(f);
  *n_out = cnt;
  return bad;
}

int main(int argc, char **argv) {
  Lcg g(1401);
  const round_mode rn = round_mode::nearest, rd = round_mode::down;
  int bad = 0, n = 0;
  bad += check_embed("vit16 cls", 4, 3, 32, 48, 16, 16, 96, 96, 1, 0, DT::u8, DT::s8, DT::undef, false, rn, true, true, true, true, g); ++n;
  bad += check_embed("swin stem", 3, 3, 16, 20, 4, 4, 96, 96, 0, 0, DT::u8, DT::s8, DT::s32, false, rn, false, false, false, true, g); ++n;
  bad += check_embed("downsample s8", 2, 32, 6, 10, 2, 2, 70, 72, 0, 0, DT::s8, DT::s8, DT::f32, false, rd, true, false, false, false, g); ++n;
  bad += check_embed("deit 2 prefix", 5, 4, 9, 13, 4, 4, 33, 35, 2, 1, DT::u8, DT::u8, DT::undef, false, rn, false, true, true, true, g); ++n;
  bad += check_embed("vit14 generic", 2, 3, 28, 42, 14, 14, 40, 40, 1, 0, DT::u8, DT::s32, DT::s8, true, rn, true, false, false, false, g); ++n;
  bad += check_embed("f32 table", 3, 16, 6, 10, 3, 5, 129, 132, 1, 2, DT::s8, DT::f32, DT::undef, true, rd, false, true, true, true, g); ++n;
  bad += check_embed("one by one", 5, 1, 1, 1, 1, 1, 1, 1, 0, 0, DT::u8, DT::u8, DT::undef, false, rn, false, false, false, false, g); ++n;
  bad += frame_embed_norm_linear(g); ++n;
  if (argc > 1) {
    int m = 0;
    bad += run_directory(argv[1], &m);
    printf("patchembed_check: %d entries from %s\n", m, argv[1]);
    n += m;
  }
  if (bad) {
    printf("patchembed_check: %d of %d cases FAILED\n", bad, n);
    return 1;
  }
  printf("patchembed_check: every case identical to the reference (%d cases)\n", n);
  return 0;
}
