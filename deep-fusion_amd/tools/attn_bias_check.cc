// attn_bias_check -- runs the logit_bias overloads of deepfusion::attention and deepfusion::matmul of the drop-in C++ API
// (include/deepfusion.h) on the cases of a directory and compares every VALID element of the output, bit for bit, with the
// expected storage given there (written by tests/test_gpu_attn_bias_cxx.py from tests/attn_bias_ref.py).  A case is
// submitted synchronously or, with async = 1, asynchronously and compared after wait() and download().  Every case is also
// run WITHOUT the bias and must then differ from the expected storage: the overloads are not the unbiased ops.
// Prints one line per case, "ok" or "DIFFERENT"; exits non-zero on a difference.
//   attn_bias_check <dir>
//     <dir>/cases.txt   one case per line:
//        attn <name> batch0 batch1 tq tk d dv q_dt dst_dt relu rm nscales async prob_scale logit_scale
//                    q_s0 q_s1 ldq k_s0 k_s1 ldk v_s0 v_s1 ldv o_s0 o_s1 ldo  q_elems k_elems v_elems o_elems  period0 period1 s0 s1 ld
//                    files <name>.q .k .v .table (256 u32) .scales (f32) .bias (f32, the host table) .o (expected storage of O)
//        bmm <name> batch0 batch1 m n k trans_b a_dt dst_dt relu rm nscales async
//                    a_s0 a_s1 lda b_s0 b_s1 ldb c_s0 c_s1 ldc  a_elems b_elems c_elems  period0 period1 s0 s1 ld
//                    files <name>.a .b .scales .bias .c
#include <array>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "deepfusion.h"
#include "dfx.h"

using namespace deepfusion;
typedef memory::dtype DT;

static DT to_dt(int dfx) { return dfx == DFX_F32 ? DT::f32 : dfx == DFX_S32 ? DT::s32 : dfx == DFX_S8 ? DT::s8 : DT::u8; }
static size_t esize(int dfx) { return (dfx == DFX_F32 || dfx == DFX_S32) ? 4 : 1; }
static std::unique_ptr<memory> flat(long long elems, DT dt) {
  return std::unique_ptr<memory>(new memory(memory::nchw_dims{1, (int)elems, 1, 1}, memory::format::nhwc, dt));
}
static std::vector<unsigned char> slurp(const std::string &path) {
  std::ifstream f(path.c_str(), std::ios::binary);
  if (!f) {
    printf("attn_bias_check: cannot read %s\n", path.c_str());
    exit(2);
  }
  return std::vector<unsigned char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
static void put(memory &m, const std::vector<unsigned char> &bytes) {
  if (bytes.size() != m.buffer_size()) {
    printf("attn_bias_check: a file has %zu bytes, its tensor %zu\n", bytes.size(), m.buffer_size());
    exit(2);
  }
  memcpy(m.data(), bytes.data(), bytes.size());
}
static std::vector<float> floats(const std::string &path) {
  const std::vector<unsigned char> b = slurp(path);
  std::vector<float> out(b.size() / 4);
  memcpy(out.data(), b.data(), out.size() * 4);
  return out;
}
static logit_bias read_bias(const std::string &base, std::istringstream &in) {
  logit_bias b;
  in >> b.period0 >> b.period1 >> b.s0 >> b.s1 >> b.ld;
  b.table = floats(base + ".bias");
  return b;
}
static void run(op &o, memory &out, int async) {
  if (async) {
    o.submit_async();
    o.wait();
    out.download();
  } else {
    o.submit();
  }
}
// elements (of `es` bytes) of the valid {b0, b1, rows, cols} region that differ between got and want
static long long differing(const unsigned char *got, const unsigned char *want, int b0n, int b1n, int rows, int cols, long long s0, long long s1, long long ld,
                           size_t es) {
  long long bad = 0;
  for (int b0 = 0; b0 < b0n; ++b0)
    for (int b1 = 0; b1 < b1n; ++b1)
      for (int m = 0; m < rows; ++m)
        for (int j = 0; j < cols; ++j) {
          const size_t at = (size_t)(b0 * s0 + b1 * s1 + (long long)m * ld + j) * es;
          if (memcmp(got + at, want + at, es) != 0) ++bad;
        }
  return bad;
}
static bool report(const std::string &name, int async, long long bad, long long unbiased_bad) {
  const bool wrong = bad != 0 || unbiased_bad == 0;
  printf("%-24s %-6s %s\n", name.c_str(), async ? "async" : "sync", wrong ? "DIFFERENT" : "ok");
  if (bad) printf("  %lld elements differ\n", bad);
  if (!unbiased_bad) printf("  the op without the bias gives the same output\n");
  return wrong;
}

static bool run_attn(const std::string &dir, std::istringstream &in) {
  std::string name;
  attention_shape sh;
  int q_dt, dst_dt, relu, rm, nscales, async;
  float prob_scale, logit_scale;
  long long qe, ke, ve, oe;
  in >> name >> sh.batch0 >> sh.batch1 >> sh.tq >> sh.tk >> sh.d >> sh.dv >> q_dt >> dst_dt >> relu >> rm >> nscales >> async >> prob_scale >> logit_scale >>
      sh.q_s0 >> sh.q_s1 >> sh.ldq >> sh.k_s0 >> sh.k_s1 >> sh.ldk >> sh.v_s0 >> sh.v_s1 >> sh.ldv >> sh.o_s0 >> sh.o_s1 >> sh.ldo >> qe >> ke >> ve >> oe;
  const std::string base = dir + "/" + name;
  const logit_bias bias = read_bias(base, in);
  if (!in) {
    printf("attn_bias_check: bad attn line\n");
    exit(2);
  }
  auto q = flat(qe, to_dt(q_dt)), k = flat(ke, DT::s8), v = flat(ve, DT::s8), o = flat(oe, to_dt(dst_dt)), o2 = flat(oe, to_dt(dst_dt));
  put(*q, slurp(base + ".q"));
  put(*k, slurp(base + ".k"));
  put(*v, slurp(base + ".v"));
  const std::vector<unsigned char> tb = slurp(base + ".table"), want = slurp(base + ".o");
  const std::vector<float> scales = floats(base + ".scales");
  std::array<uint32_t, 256> table;
  if (tb.size() != sizeof(table) || (int)scales.size() != nscales || want.size() != o->buffer_size()) {
    printf("attn_bias_check: %s: table, scales or expected storage of the wrong size\n", name.c_str());
    exit(2);
  }
  memcpy(table.data(), tb.data(), sizeof(table));
  const round_mode r = rm ? round_mode::down : round_mode::nearest;
  auto biased = attention(q, k, v, table, o, sh, logit_scale, scales, bias, prob_scale, relu != 0, r);
  run(*biased, *o, async);
  auto plain = attention(q, k, v, table, o2, sh, logit_scale, scales, prob_scale, relu != 0, r);
  run(*plain, *o2, async);
  const size_t es = esize(dst_dt);
  return report(name, async, differing((const unsigned char *)o->host_data(), want.data(), sh.batch0, sh.batch1, sh.tq, sh.dv, sh.o_s0, sh.o_s1, sh.ldo, es),
                differing((const unsigned char *)o2->host_data(), want.data(), sh.batch0, sh.batch1, sh.tq, sh.dv, sh.o_s0, sh.o_s1, sh.ldo, es));
}

static bool run_bmm(const std::string &dir, std::istringstream &in) {
  std::string name;
  matmul_shape sh;
  int trans_b, a_dt, dst_dt, relu, rm, nscales, async;
  long long ae, be, ce;
  in >> name >> sh.batch0 >> sh.batch1 >> sh.m >> sh.n >> sh.k >> trans_b >> a_dt >> dst_dt >> relu >> rm >> nscales >> async >> sh.a_s0 >> sh.a_s1 >> sh.lda >>
      sh.b_s0 >> sh.b_s1 >> sh.ldb >> sh.c_s0 >> sh.c_s1 >> sh.ldc >> ae >> be >> ce;
  sh.trans_b = trans_b != 0;
  const std::string base = dir + "/" + name;
  const logit_bias bias = read_bias(base, in);
  if (!in) {
    printf("attn_bias_check: bad bmm line\n");
    exit(2);
  }
  auto a = flat(ae, to_dt(a_dt)), b = flat(be, DT::s8), c = flat(ce, to_dt(dst_dt)), c2 = flat(ce, to_dt(dst_dt));
  put(*a, slurp(base + ".a"));
  put(*b, slurp(base + ".b"));
  const std::vector<unsigned char> want = slurp(base + ".c");
  const std::vector<float> scales = floats(base + ".scales");
  if ((int)scales.size() != nscales || want.size() != c->buffer_size()) {
    printf("attn_bias_check: %s: scales or expected storage of the wrong size\n", name.c_str());
    exit(2);
  }
  const round_mode r = rm ? round_mode::down : round_mode::nearest;
  auto biased = matmul(a, b, c, sh, scales, bias, relu != 0, r);
  run(*biased, *c, async);
  auto plain = matmul(a, b, c2, sh, scales, relu != 0, r);
  run(*plain, *c2, async);
  const size_t es = esize(dst_dt);
  return report(name, async, differing((const unsigned char *)c->host_data(), want.data(), sh.batch0, sh.batch1, sh.m, sh.n, sh.c_s0, sh.c_s1, sh.ldc, es),
                differing((const unsigned char *)c2->host_data(), want.data(), sh.batch0, sh.batch1, sh.m, sh.n, sh.c_s0, sh.c_s1, sh.ldc, es));
}

int main(int argc, char **argv) {
  if (argc < 2) {
    printf("usage: attn_bias_check <dir>\n");
    return 2;
  }
  const std::string dir = argv[1];
  std::ifstream f((dir + "/cases.txt").c_str());
  if (!f) {
    printf("attn_bias_check: cannot read %s/cases.txt\n", dir.c_str());
    return 2;
  }
  std::string line;
  int n = 0;
  bool bad = false;
  while (std::getline(f, line)) {
    std::istringstream in(line);
    std::string kind;
    if (!(in >> kind)) continue;
    if (kind == "attn") bad = run_attn(dir, in) || bad;
    else if (kind == "bmm") bad = run_bmm(dir, in) || bad;
    else {
      printf("attn_bias_check: unknown entry %s\n", kind.c_str());
      return 2;
    }
    ++n;
  }
  printf("attn_bias_check: %d entries, %s\n", n, bad ? "DIFFERENCES" : "all ok");
  return bad ? 1 : 0;
}
