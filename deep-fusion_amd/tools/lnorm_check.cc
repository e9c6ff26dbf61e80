// lnorm_check -- runs deepfusion::layer_norm of the drop-in C++ API (include/deepfusion.h) and compares every result, bit
// for bit, with a scalar reference in this file: the sequence of include/dfx.h (exact 64-bit integer statistics, then one
// separately rounded f32 operation per step; sqrtf and the divisions of the host are correctly rounded).  One frame chains
// layer_norm() -> inner_product() on the device with no host step in between, submitted asynchronously; another keeps two
// norms of one source in flight at once.  With a directory argument it also runs the cases a test wrote there (cases.txt:
//   case <name> <bs> <C> <h> <w> <c_valid> <dst_C> <src_dt> <dst_dt> <mode> <has_beta> <has_shift> <async> <eps bits>
// with <name>.src / .gamma / .beta / .shift / .dst beside it; .dst is the expected storage of dst) against BOTH the file and
// the scalar reference.  Prints one line per case, "ok" or "DIFFERENT"; exits non-zero on a difference.
//   lnorm_check [directory]
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "cli_flags.h"
#include "deepfusion.h"
#include "dfx.h"

using namespace deepfusion;
typedef memory::dtype DT;

static std::unique_ptr<memory> mk(int n, int c, int h, int w, DT dt, memory::format f = memory::format::nhwc) {
  return std::unique_ptr<memory>(new memory(memory::nchw_dims{n, c, h, w}, f, dt));
}
static size_t esize(DT dt) { return (dt == DT::f32 || dt == DT::s32) ? 4 : 1; }

// dst: as it was before the op; the pad elements stay
static void ref_norm(const unsigned char *src, DT dt, long long rows, int ld, int c, const float *gamma, const float *beta, const u8 *shift, float eps,
                     norm_mode mode, DT dst_dt, int dst_ld, std::vector<unsigned char> &dst) {
  const size_t ds = esize(dst_dt);
  std::vector<long long> t(c);
  for (long long r = 0; r < rows; ++r) {
    const unsigned char *row = src + (size_t)r * ld;
    long long S = 0;
    unsigned long long Q = 0;
    for (int k = 0; k < c; ++k) {
      const long long x = dt == DT::u8 ? (long long)row[k] : (long long)(signed char)row[k];
      t[k] = x * (1ll << (shift ? shift[k] : 0));
      S += t[k];
      Q += (unsigned long long)(t[k] * t[k]);
    }
    volatile float v, a;
    const float fc = (float)c;
    if (mode == norm_mode::layer) {
      const long long D = (long long)c * (long long)Q - S * S;
      v = (float)D / (float)((long long)c * c);
      v = v + eps;
      a = 1.0f / sqrtf(v);
      a = a / fc;
    } else {
      v = (float)(long long)Q / fc;
      v = v + eps;
      a = 1.0f / sqrtf(v);
    }
    for (int k = 0; k < c; ++k) {
      const long long u = mode == norm_mode::layer ? (long long)c * t[k] - S : t[k];
      volatile float y = (float)u * a;
      y = y * gamma[k];
      y = y + (beta ? beta[k] : 0.0f);
      unsigned char *o = &dst[((size_t)r * dst_ld + k) * ds];
      const float f = y;
      if (dst_dt == DT::f32) {
        memcpy(o, &f, 4);
      } else {
        const float lo = dst_dt == DT::u8 ? 0.f : -128.f, hi = dst_dt == DT::u8 ? 255.f : 127.f;
        float q = f != f ? 0.f : nearbyintf(f);
        q = q < lo ? lo : q > hi ? hi : q;
        *o = (unsigned char)(int)q;
      }
    }
  }
}

static int report(const char *name, const std::string &what, bool bad) {
  printf("lnorm_check %-14s %s: %s\n", name, what.c_str(), bad ? "DIFFERENT from the reference" : "ok");
  return bad ? 1 : 0;
}

// the c valid channels of every row (the op leaves the pad elements of dst's device copy as they are)
static bool rows_differ(const void *got, const std::vector<unsigned char> &want, long long rows, int ld, int c, size_t es) {
  for (long long r = 0; r < rows; ++r)
    if (memcmp((const unsigned char *)got + (size_t)r * ld * es, &want[(size_t)r * ld * es], (size_t)c * es) != 0) return true;
  return false;
}

struct Params {
  std::vector<float> gamma, beta;
  std::vector<u8> shift;
};
static Params make_params(int c, bool with_beta, bool with_shift, float span, float offset, Lcg &g) {
  Params p;
  for (int k = 0; k < c; ++k) p.gamma.push_back(((float)(g.next() % 2001) - 1000.f) * 0.001f * span);
  if (with_beta)
    for (int k = 0; k < c; ++k) p.beta.push_back(((float)(g.next() % 2001) - 1000.f) * 0.0005f * span + offset);
  if (with_shift)
    for (int k = 0; k < c; ++k) p.shift.push_back((u8)(g.next() % 8));
  return p;
}
static void fill(memory &m, Lcg &g) {
  for (size_t i = 0; i < m.size(); ++i) ((uint8_t *)m.data())[i] = (uint8_t)(g.next() & 0xff);
}

static int check_norm(const char *name, int bs, int C, int h, int w, DT dt, DT dst_dt, int dst_C, int c_valid, norm_mode mode, bool with_beta,
                      bool with_shift, bool use_async, Lcg &g) {
  const int c = c_valid ? c_valid : C;
  auto src = mk(bs, C, h, w, dt);
  fill(*src, g);
  auto dst = mk(bs, dst_C, h, w, dst_dt);
  memset(dst->data(), 0xCD, dst->buffer_size());
  std::vector<unsigned char> want(dst->buffer_size(), 0xCD);
  const Params p = make_params(c, with_beta, with_shift, dst_dt == DT::f32 ? 1.f : 60.f, dst_dt == DT::u8 ? 120.f : 0.f, g);
  const float eps = 0.25f;
  ref_norm((const unsigned char *)src->host_data(), dt, (long long)bs * h * w, C, c, p.gamma.data(), with_beta ? p.beta.data() : nullptr,
           with_shift ? p.shift.data() : nullptr, eps, mode, dst_dt, dst_C, want);
  auto op = layer_norm(src, p.gamma, p.beta, dst, eps, mode, p.shift, c_valid);
  if (use_async) {
    op->submit_async();
    op->wait();
    dst->download();
  } else {
    op->submit();
  }
  char what[200];
  snprintf(what, sizeof(what), "%s bs %d %dx%d c %d/%d -> %s ld %d%s%s %s", mode == norm_mode::rms ? "rms" : "layer", bs, h, w, c, C,
           dst_dt == DT::f32 ? "f32" : dst_dt == DT::u8 ? "u8" : "s8", dst_C, with_beta ? "" : " no-beta", with_shift ? " shift" : "",
           use_async ? "async" : "sync");
  return report(name, what, rows_differ(dst->host_data(), want, (long long)bs * h * w, dst_C, c, esize(dst_dt)));
}

// layer_norm() -> inner_product(), both submitted asynchronously: the normalised tokens never leave the device in between
static int frame_norm_fc(Lcg &g) {
  const int bs = 4, c = 96, oc = 32;
  auto src = mk(bs, c, 1, 1, DT::s8);
  fill(*src, g);
  auto normed = mk(bs, c, 1, 1, DT::u8);
  auto wei = mk(oc, c, 1, 1, DT::s8, memory::format::oihw);
  for (size_t i = 0; i < wei->size(); ++i) ((int8_t *)wei->data())[i] = (int8_t)((int)(g.next() % 256) - 128);
  std::unique_ptr<memory> bia;
  auto logits = mk(bs, oc, 1, 1, DT::s32);
  const Params p = make_params(c, true, false, 60.f, 120.f, g);
  auto ln = layer_norm(src, p.gamma, p.beta, normed, 0.5f);
  auto fc = inner_product(normed, wei, bia, logits);
  ln->submit_async();
  fc->submit_async();
  fc->wait();
  ln->wait();
  normed->download();
  logits->download();
  std::vector<unsigned char> wn(normed->buffer_size(), 0);
  ref_norm((const unsigned char *)src->host_data(), DT::s8, bs, c, c, p.gamma.data(), p.beta.data(), nullptr, 0.5f, norm_mode::layer, DT::u8, c, wn);
  bool bad = memcmp(normed->host_data(), wn.data(), wn.size()) != 0;
  // the same inner product on the reference's tokens, uploaded from the host
  auto tokens = mk(bs, c, 1, 1, DT::u8);
  memcpy(tokens->data(), wn.data(), wn.size());
  auto logits2 = mk(bs, oc, 1, 1, DT::s32);
  inner_product(tokens, wei, bia, logits2)->submit();
  bad = bad || memcmp(logits->host_data(), logits2->host_data(), logits->buffer_size()) != 0;
  return report("norm->fc", "bs 4 c 96 s8 -> u8 -> 32 s32, asynchronous", bad);
}

// two norms of one source in flight at once
static int frame_two_in_flight(Lcg &g) {
  const int bs = 3, C = 112, c = 100, h = 5, w = 7;
  auto src = mk(bs, C, h, w, DT::u8);
  fill(*src, g);
  auto a = mk(bs, C, h, w, DT::s8);
  auto b = mk(bs, c, h, w, DT::f32);
  memset(a->data(), 0xCD, a->buffer_size());
  memset(b->data(), 0xCD, b->buffer_size());
  const Params pa = make_params(c, true, true, 60.f, 0.f, g), pb = make_params(c, false, false, 1.f, 0.f, g);
  auto la = layer_norm(src, pa.gamma, pa.beta, a, 0.125f, norm_mode::layer, pa.shift, c);
  auto lb = layer_norm(src, pb.gamma, pb.beta, b, 2.0f, norm_mode::rms, pb.shift, c);
  la->submit_async();
  lb->submit_async();
  lb->wait();
  la->wait();
  a->download();
  b->download();
  std::vector<unsigned char> wa(a->buffer_size(), 0xCD), wb(b->buffer_size(), 0xCD);
  const long long rows = (long long)bs * h * w;
  ref_norm((const unsigned char *)src->host_data(), DT::u8, rows, C, c, pa.gamma.data(), pa.beta.data(), pa.shift.data(), 0.125f, norm_mode::layer, DT::s8, C, wa);
  ref_norm((const unsigned char *)src->host_data(), DT::u8, rows, C, c, pb.gamma.data(), nullptr, nullptr, 2.0f, norm_mode::rms, DT::f32, c, wb);
  const bool bad = rows_differ(a->host_data(), wa, rows, C, c, 1) || rows_differ(b->host_data(), wb, rows, c, c, 4);
  return report("two in flight", "layer (shift) + rms of one u8 tensor, submit_async on both", bad);
}

static bool read_file(const std::string &path, std::vector<unsigned char> &out, size_t want) {
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) return false;
  out.resize(want);
  const size_t n = fread(out.data(), 1, want, f);
  const bool more = fgetc(f) != EOF;
  fclose(f);
  return n == want && !more;
}

static int run_directory(const std::string &dir, int *n_out) {
  FILE *f = fopen((dir + "/cases.txt").c_str(), "r");
  if (!f) { fprintf(stderr, "lnorm_check: cannot read %s/cases.txt\n", dir.c_str()); return 1; }
  int bad = 0, n = 0;
  char name[64];
  int bs, C, h, w, c, dst_C, sdt, ddt, mode, has_beta, has_shift, use_async;
  unsigned eps_bits;
  while (fscanf(f, " case %63s %d %d %d %d %d %d %d %d %d %d %d %d %x", name, &bs, &C, &h, &w, &c, &dst_C, &sdt, &ddt, &mode, &has_beta, &has_shift,
                &use_async, &eps_bits) == 14) {
    const DT dt = sdt == DFX_U8 ? DT::u8 : DT::s8, dst_dt = ddt == DFX_F32 ? DT::f32 : ddt == DFX_U8 ? DT::u8 : DT::s8;
    const norm_mode nm = mode == DFX_LNORM_RMS ? norm_mode::rms : norm_mode::layer;
    float eps;
    memcpy(&eps, &eps_bits, 4);
    const long long rows = (long long)bs * h * w;
    const std::string base = dir + "/" + name;
    std::vector<unsigned char> fs, fg, fb, fsh, fd;
    const size_t dbytes = (size_t)rows * dst_C * esize(dst_dt);
    if (!read_file(base + ".src", fs, (size_t)rows * C) || !read_file(base + ".gamma", fg, (size_t)c * 4) || !read_file(base + ".dst", fd, dbytes) ||
        (has_beta && !read_file(base + ".beta", fb, (size_t)c * 4)) || (has_shift && !read_file(base + ".shift", fsh, (size_t)c))) {
      fprintf(stderr, "lnorm_check: case %s: a file is missing or has the wrong size\n", name);
      fclose(f);
      return 1;
    }
    auto src = mk(bs, C, h, w, dt);
    memcpy(src->data(), fs.data(), fs.size());
    auto dst = mk(bs, dst_C, h, w, dst_dt);
    memset(dst->data(), 0xCD, dst->buffer_size());
    std::vector<float> gamma((const float *)fg.data(), (const float *)fg.data() + c), beta;
    if (has_beta) beta.assign((const float *)fb.data(), (const float *)fb.data() + c);
    std::vector<unsigned char> want(dbytes, 0xCD);
    ref_norm(fs.data(), dt, rows, C, c, gamma.data(), has_beta ? beta.data() : nullptr, has_shift ? fsh.data() : nullptr, eps, nm, dst_dt, dst_C, want);
    auto op = layer_norm(src, gamma, beta, dst, eps, nm, fsh, c == C ? 0 : c);
    if (use_async) {
      op->submit_async();
      op->wait();
      dst->download();
    } else {
      op->submit();
    }
    const bool b_file = rows_differ(dst->host_data(), fd, rows, dst_C, c, esize(dst_dt));
    const bool b_ref = rows_differ(dst->host_data(), want, rows, dst_C, c, esize(dst_dt));
    char what[200];
    snprintf(what, sizeof(what), "%s bs %d %dx%d c %d/%d ld %d %s%s%s", mode ? "rms" : "layer", bs, h, w, c, C, dst_C, use_async ? "async" : "sync",
             b_file ? " [file differs]" : "", b_ref ? " [scalar reference differs]" : "");
    bad += report(name, what, b_file || b_ref);
    ++n;
  }
  fclose(f);
  *n_out = n;
  return bad;
}

int main(int argc, char **argv) {
  Lcg g(977);
  int bad = 0, n = 0;
  bad += check_norm("swin", 2, 96, 7, 7, DT::s8, DT::s8, 96, 0, norm_mode::layer, true, false, false, g); ++n;
  bad += check_norm("vit", 1, 768, 197, 1, DT::s8, DT::s8, 768, 0, norm_mode::layer, true, true, false, g); ++n;
  bad += check_norm("vit rms f32", 2, 768, 5, 1, DT::u8, DT::f32, 768, 0, norm_mode::rms, false, false, true, g); ++n;
  bad += check_norm("c_valid", 3, 112, 4, 5, DT::u8, DT::u8, 128, 100, norm_mode::layer, true, true, false, g); ++n;
  bad += check_norm("odd ld", 3, 21, 4, 5, DT::s8, DT::u8, 23, 0, norm_mode::rms, true, false, true, g); ++n;
  bad += check_norm("one channel", 5, 1, 1, 1, DT::s8, DT::f32, 1, 0, norm_mode::layer, true, false, false, g); ++n;
  bad += check_norm("long", 2, 4097, 1, 1, DT::s8, DT::s8, 4097, 0, norm_mode::layer, true, true, false, g); ++n;
  bad += check_norm("longest", 1, 16384, 2, 1, DT::u8, DT::f32, 16384, 0, norm_mode::layer, true, true, true, g); ++n;
  bad += frame_norm_fc(g); ++n;
  bad += frame_two_in_flight(g); ++n;
  if (argc > 1) {
    int m = 0;
    bad += run_directory(argv[1], &m);
    printf("lnorm_check: %d entries from %s\n", m, argv[1]);
    n += m;
  }
  if (bad) {
    printf("lnorm_check: %d of %d cases FAILED\n", bad, n);
    return 1;
  }
  printf("lnorm_check: every case identical to the reference (%d cases)\n", n);
  return 0;
}
