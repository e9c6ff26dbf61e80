// bmm_check -- runs deepfusion::matmul of the drop-in C++ API (include/deepfusion.h) on the cases of a directory and compares
// every VALID element of C, bit for bit, with the expected storage given there (written by tests/test_gpu_bmm_cxx.py from
// tests/bmm_ref.py) and, as a second opinion, with the scalar restatement of tools/bmm_host.h.  A `chain` entry runs an int8
// attention block on the device with no host step in between: matmul (s8 x s8 -> s8 logits) -> softmax (u8) -> matmul
// (u8 x s8 -> s8 context, written back interleaved), submitted asynchronously, each tensor compared after the last wait.
// Prints one line per case, "ok" or "DIFFERENT"; exits non-zero on a difference.
//   bmm_check <dir>
//     <dir>/cases.txt   one case per line:
//        case  <name> batch0 batch1 m n k trans_b a_dt dst_dt relu rm nscales a_s0 a_s1 lda b_s0 b_s1 ldb c_s0 c_s1 ldc
//                      files <name>.a <name>.b <name>.scales (f32) <name>.c (expected storage of C)
//        chain <name> bs heads t d scale_qk scale_pv
//                      files <name>.q .k .v (s8 {bs, t, heads * d}) .table (256 u32) .logits .probs .context (expected)
#include <array>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "bmm_host.h"
#include "deepfusion.h"

using namespace deepfusion;
typedef memory::dtype DT;

static DT to_dt(int dfx) { return dfx == DFX_F32 ? DT::f32 : dfx == DFX_S32 ? DT::s32 : dfx == DFX_S8 ? DT::s8 : DT::u8; }
static std::unique_ptr<memory> flat(long long elems, DT dt) {
  return std::unique_ptr<memory>(new memory(memory::nchw_dims{1, (int)elems, 1, 1}, memory::format::nhwc, dt));
}
static std::vector<unsigned char> slurp(const std::string &path) {
  std::ifstream f(path.c_str(), std::ios::binary);
  if (!f) {
    printf("bmm_check: cannot read %s\n", path.c_str());
    exit(2);
  }
  return std::vector<unsigned char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
static void put(memory &m, const std::vector<unsigned char> &bytes) {
  if (bytes.size() != m.buffer_size()) {
    printf("bmm_check: a file has %zu bytes, its tensor %zu\n", bytes.size(), m.buffer_size());
    exit(2);
  }
  memcpy(m.data(), bytes.data(), bytes.size());
}
static matmul_shape api_shape(const BmmShape &s) {
  matmul_shape o;
  o.batch0 = s.batch0; o.batch1 = s.batch1; o.m = s.m; o.n = s.n; o.k = s.k; o.trans_b = s.trans_b != 0;
  o.a_s0 = s.a_s0; o.a_s1 = s.a_s1; o.lda = s.lda; o.b_s0 = s.b_s0; o.b_s1 = s.b_s1; o.ldb = s.ldb; o.c_s0 = s.c_s0; o.c_s1 = s.c_s1; o.ldc = s.ldc;
  return o;
}

// valid elements of `got` against `want` (both C's storage) and, when a / b are given, against the scalar restatement
static long long differ(const BmmShape &s, const unsigned char *got, const unsigned char *want, const unsigned char *a, const unsigned char *b,
                        const std::vector<float> &scales) {
  const size_t es = bmm_esize(s.dst_dt);
  long long bad = 0;
  for (int b0 = 0; b0 < s.batch0; ++b0)
    for (int b1 = 0; b1 < s.batch1; ++b1)
      for (int m = 0; m < s.m; ++m)
        for (int n = 0; n < s.n; ++n) {
          const size_t at = (size_t)(b0 * s.c_s0 + b1 * s.c_s1 + (long long)m * s.ldc + n) * es;
          if (memcmp(got + at, want + at, es) != 0) {
            ++bad;
            continue;
          }
          if (a) {
            const uint32_t v = bmm_host_value(s, a, b, scales.data(), (int)scales.size(), b0, b1, m, n);
            if (memcmp(got + at, &v, es) != 0) ++bad;
          }
        }
  return bad;
}
static bool report(const std::string &name, const char *what, long long bad) {
  printf("%-24s %-10s %s\n", name.c_str(), what, bad ? "DIFFERENT" : "ok");
  if (bad) printf("  %lld elements differ\n", bad);
  return bad != 0;
}

static bool run_case(const std::string &dir, std::istringstream &in) {
  std::string name;
  BmmShape s;
  int nscales = 1;
  in >> name >> s.batch0 >> s.batch1 >> s.m >> s.n >> s.k >> s.trans_b >> s.a_dt >> s.dst_dt >> s.relu >> s.rm >> nscales >> s.a_s0 >> s.a_s1 >>
      s.lda >> s.b_s0 >> s.b_s1 >> s.ldb >> s.c_s0 >> s.c_s1 >> s.ldc;
  if (!in) {
    printf("bmm_check: bad case line\n");
    exit(2);
  }
  const std::string base = dir + "/" + name;
  auto a = flat(s.a_elems(), to_dt(s.a_dt)), b = flat(s.b_elems(), DT::s8), c = flat(s.c_elems(), to_dt(s.dst_dt));
  put(*a, slurp(base + ".a"));
  put(*b, slurp(base + ".b"));
  const std::vector<unsigned char> sb = slurp(base + ".scales"), want = slurp(base + ".c");
  std::vector<float> scales(sb.size() / 4);
  memcpy(scales.data(), sb.data(), scales.size() * 4);
  if ((int)scales.size() != nscales || want.size() != c->buffer_size()) {
    printf("bmm_check: %s: scales or expected storage of the wrong size\n", name.c_str());
    exit(2);
  }
  matmul(a, b, c, api_shape(s), scales, s.relu != 0, s.rm ? round_mode::down : round_mode::nearest)->submit();
  return report(name, s.trans_b ? "nt" : "nn",
                differ(s, (const unsigned char *)c->host_data(), want.data(), (const unsigned char *)a->host_data(),
                       (const unsigned char *)b->host_data(), scales));
}

static bool run_chain(const std::string &dir, std::istringstream &in) {
  std::string name;
  int bs, heads, t, d;
  float scale_qk, scale_pv;
  in >> name >> bs >> heads >> t >> d >> scale_qk >> scale_pv;
  if (!in) {
    printf("bmm_check: bad chain line\n");
    exit(2);
  }
  const std::string base = dir + "/" + name;
  const BmmShape qk = bmm_attention(bs, heads, t, d, 0, DFX_S8, DFX_S8), pv = bmm_attention(bs, heads, t, d, 1, DFX_U8, DFX_S8);
  const int hd = heads * d, lt = (int)qk.ldc, rows = bs * heads * t;
  auto mk = [](int n, int c, int h, DT dt) { return std::unique_ptr<memory>(new memory(memory::nchw_dims{n, c, h, 1}, memory::format::nhwc, dt)); };
  auto q = mk(bs, hd, t, DT::s8), k = mk(bs, hd, t, DT::s8), v = mk(bs, hd, t, DT::s8), ctx = mk(bs, hd, t, DT::s8);
  auto logits = mk(rows, lt, 1, DT::s8), probs = mk(rows, lt, 1, DT::u8);
  put(*q, slurp(base + ".q"));
  put(*k, slurp(base + ".k"));
  put(*v, slurp(base + ".v"));
  const std::vector<unsigned char> tb = slurp(base + ".table");
  std::array<uint32_t, 256> table;
  if (tb.size() != sizeof(table)) {
    printf("bmm_check: %s.table must hold 256 u32\n", name.c_str());
    exit(2);
  }
  memcpy(table.data(), tb.data(), sizeof(table));
  const std::array<long long, 3> hs = attention_strides(bs, heads, t, d);
  if (hs[0] != qk.a_s0 || hs[1] != qk.a_s1 || hs[2] != qk.lda || hs[0] != pv.c_s0 || hs[1] != pv.c_s1 || hs[2] != pv.ldc) return report(name, "strides", 1);
  auto op1 = matmul(q, k, logits, api_shape(qk), {scale_qk});
  auto op2 = softmax(logits, table, probs, 255.f, t);
  auto op3 = matmul(probs, v, ctx, api_shape(pv), {scale_pv});
  op1->submit_async();
  op2->submit_async();
  op3->submit_async();
  op3->wait();
  op2->wait();
  op1->wait();
  logits->download();
  probs->download();
  ctx->download();
  const std::vector<unsigned char> wl = slurp(base + ".logits"), wp = slurp(base + ".probs"), wc = slurp(base + ".context");
  if (wl.size() != logits->buffer_size() || wp.size() != probs->buffer_size() || wc.size() != ctx->buffer_size()) {
    printf("bmm_check: %s: an expected tensor has the wrong size\n", name.c_str());
    exit(2);
  }
  bool bad = report(name, "logits", differ(qk, (const unsigned char *)logits->host_data(), wl.data(), nullptr, nullptr, {}));
  BmmShape pr = qk;  // the probabilities: the logits' layout, u8
  pr.dst_dt = DFX_U8;
  bad = report(name, "probs", differ(pr, (const unsigned char *)probs->host_data(), wp.data(), nullptr, nullptr, {})) || bad;
  bad = report(name, "context", differ(pv, (const unsigned char *)ctx->host_data(), wc.data(), nullptr, nullptr, {})) || bad;
  return bad;
}

int main(int argc, char **argv) {
  if (argc < 2) {
    printf("usage: bmm_check <dir>\n");
    return 2;
  }
  const std::string dir = argv[1];
  std::ifstream f((dir + "/cases.txt").c_str());
  if (!f) {
    printf("bmm_check: cannot read %s/cases.txt\n", dir.c_str());
    return 2;
  }
  std::string line;
  int n = 0;
  bool bad = false;
  while (std::getline(f, line)) {
    std::istringstream in(line);
    std::string kind;
    if (!(in >> kind)) continue;
    if (kind == "case") bad = run_case(dir, in) || bad;
    else if (kind == "chain") bad = run_chain(dir, in) || bad;
    else {
      printf("bmm_check: unknown entry %s\n", kind.c_str());
      return 2;
    }
    ++n;
  }
  printf("bmm_check: %d entries, %s\n", n, bad ? "DIFFERENCES" : "all ok");
  return bad ? 1 : 0;
}
