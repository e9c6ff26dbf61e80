// attn_check -- runs deepfusion::attention of the drop-in C++ API (include/deepfusion.h) on the cases of a directory and
// compares every VALID element of O, bit for bit, with the expected storage given there (written by
// tests/test_gpu_attn_cxx.py from tests/attn_ref.py) and, as a second opinion, with the scalar restatement of
// tools/attn_host.h (the chain of the matrix product, the table softmax and the matrix product).  A case is submitted
// synchronously or, with async = 1, asynchronously and compared after wait() and download().
// Prints one line per case, "ok" or "DIFFERENT"; exits non-zero on a difference.
//   attn_check <dir>
//     <dir>/cases.txt   one case per line:
//        case <name> batch0 batch1 tq tk d dv q_dt dst_dt relu rm nscales async prob_scale logit_scale
//                    q_s0 q_s1 ldq k_s0 k_s1 ldk v_s0 v_s1 ldv o_s0 o_s1 ldo
//                    files <name>.q .k .v .table (256 u32) .scales (f32) .o (expected storage of O)
#include <array>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "attn_host.h"
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
    printf("attn_check: cannot read %s\n", path.c_str());
    exit(2);
  }
  return std::vector<unsigned char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
static void put(memory &m, const std::vector<unsigned char> &bytes) {
  if (bytes.size() != m.buffer_size()) {
    printf("attn_check: a file has %zu bytes, its tensor %zu\n", bytes.size(), m.buffer_size());
    exit(2);
  }
  memcpy(m.data(), bytes.data(), bytes.size());
}

static bool run_case(const std::string &dir, std::istringstream &in) {
  std::string name;
  AttnShape s;
  memset(&s, 0, sizeof(s));
  int nscales = 1, async = 0;
  float logit_scale = 0;
  in >> name >> s.batch0 >> s.batch1 >> s.tq >> s.tk >> s.d >> s.dv >> s.q_dt >> s.dst_dt >> s.relu >> s.rm >> nscales >> async >> s.prob_scale >>
      logit_scale >> s.q_s0 >> s.q_s1 >> s.ldq >> s.k_s0 >> s.k_s1 >> s.ldk >> s.v_s0 >> s.v_s1 >> s.ldv >> s.o_s0 >> s.o_s1 >> s.ldo;
  if (!in) {
    printf("attn_check: bad case line\n");
    exit(2);
  }
  const std::string base = dir + "/" + name;
  auto q = flat(s.q_elems(), to_dt(s.q_dt)), k = flat(s.k_elems(), DT::s8), v = flat(s.v_elems(), DT::s8), o = flat(s.o_elems(), to_dt(s.dst_dt));
  put(*q, slurp(base + ".q"));
  put(*k, slurp(base + ".k"));
  put(*v, slurp(base + ".v"));
  const std::vector<unsigned char> tb = slurp(base + ".table"), sb = slurp(base + ".scales"), want = slurp(base + ".o");
  std::array<uint32_t, 256> table;
  std::vector<float> scales(sb.size() / 4);
  if (tb.size() != sizeof(table) || (int)scales.size() != nscales || want.size() != o->buffer_size()) {
    printf("attn_check: %s: table, scales or expected storage of the wrong size\n", name.c_str());
    exit(2);
  }
  memcpy(table.data(), tb.data(), sizeof(table));
  memcpy(scales.data(), sb.data(), scales.size() * 4);
  attention_shape sh;
  sh.batch0 = s.batch0; sh.batch1 = s.batch1; sh.tq = s.tq; sh.tk = s.tk; sh.d = s.d; sh.dv = s.dv;
  sh.q_s0 = s.q_s0; sh.q_s1 = s.q_s1; sh.ldq = s.ldq; sh.k_s0 = s.k_s0; sh.k_s1 = s.k_s1; sh.ldk = s.ldk;
  sh.v_s0 = s.v_s0; sh.v_s1 = s.v_s1; sh.ldv = s.ldv; sh.o_s0 = s.o_s0; sh.o_s1 = s.o_s1; sh.ldo = s.ldo;
  auto op = attention(q, k, v, table, o, sh, logit_scale, scales, s.prob_scale, s.relu != 0, s.rm ? round_mode::down : round_mode::nearest);
  if (async) {
    op->submit_async();
    op->wait();
    o->download();
  } else {
    op->submit();
  }
  const std::vector<uint32_t> host = attn_host_values(s, (const unsigned char *)q->host_data(), (const unsigned char *)k->host_data(),
                                                      (const unsigned char *)v->host_data(), table.data(), logit_scale, scales.data(), nscales);
  const unsigned char *got = (const unsigned char *)o->host_data();
  const size_t es = attn_esize(s.dst_dt);
  long long bad = 0;
  size_t i = 0;
  for (int b0 = 0; b0 < s.batch0; ++b0)
    for (int b1 = 0; b1 < s.batch1; ++b1)
      for (int m = 0; m < s.tq; ++m)
        for (int j = 0; j < s.dv; ++j, ++i) {
          const size_t at = (size_t)(b0 * s.o_s0 + b1 * s.o_s1 + (long long)m * s.ldo + j) * es;
          if (memcmp(got + at, want.data() + at, es) != 0 || memcmp(got + at, &host[i], es) != 0) ++bad;
        }
  printf("%-24s %-6s %s\n", name.c_str(), async ? "async" : "sync", bad ? "DIFFERENT" : "ok");
  if (bad) printf("  %lld elements differ\n", bad);
  return bad != 0;
}

int main(int argc, char **argv) {
  if (argc < 2) {
    printf("usage: attn_check <dir>\n");
    return 2;
  }
  const std::string dir = argv[1];
  std::ifstream f((dir + "/cases.txt").c_str());
  if (!f) {
    printf("attn_check: cannot read %s/cases.txt\n", dir.c_str());
    return 2;
  }
  std::string line;
  int n = 0;
  bool bad = false;
  while (std::getline(f, line)) {
    std::istringstream in(line);
    std::string kind;
    if (!(in >> kind)) continue;
    if (kind != "case") {
      printf("attn_check: unknown entry %s\n", kind.c_str());
      return 2;
    }
    bad = run_case(dir, in) || bad;
    ++n;
  }
  printf("attn_check: %d entries, %s\n", n, bad ? "DIFFERENCES" : "all ok");
  return bad ? 1 : 0;
}
