// wsum_check -- runs deepfusion::scaled_sum of the drop-in C++ API (include/deepfusion.h) over a few joins and compares
// every result, bit for bit, with dfx_wsum_submit_host of the C ABI on the same numbers and with a scalar loop in this
// file: float(src) * scale (one rounding), + the next product (two roundings), + bias, ReLU, rint or floor with NaN -> 0
// and the clamp, or the table.  Some joins run in place (dst is the first or the last source) and one gives a tensor twice.
// Prints a hash of every result: the bytes must not depend on DEEPFUSION_DEVICES.  Exits non-zero on the first difference.
//   wsum_check
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

static std::unique_ptr<memory> mk(int n, int c, int h, int w, DT dt) {
  return std::unique_ptr<memory>(new memory(memory::nchw_dims{n, c, h, w}, memory::format::nhwc, dt));
}

struct Join {
  const char *name;
  int bs, h, w, c;
  std::vector<DT> src;
  DT dst;
  std::vector<bool> per_channel;
  int bias;          // 0: none, 1: one, 2: per channel
  bool relu;
  DT table_in;       // undef: no table
  round_mode rm;
  int in_place;      // -1: no; else the source that is dst
  bool twice;        // source 1 is source 0's tensor
};

static size_t esize(DT dt) { return (dt == DT::f32 || dt == DT::s32) ? 4 : 1; }

static float load(const void *p, DT dt, size_t i) {
  if (dt == DT::f32) return ((const float *)p)[i];
  if (dt == DT::s32) return (float)((const int32_t *)p)[i];
  if (dt == DT::s8) return (float)((const int8_t *)p)[i];
  return (float)((const uint8_t *)p)[i];
}

static int cvt(float v, round_mode rm, bool is_u8) {
  if (v != v) return 0;
  const float r = rm == round_mode::down ? floorf(v) : nearbyintf(v);
  const float lo = is_u8 ? 0.0f : -128.0f, hi = is_u8 ? 255.0f : 127.0f;
  return (int)(r < lo ? lo : r > hi ? hi : r);
}

static std::vector<unsigned char> scalar_ref(const Join &j, const std::vector<std::vector<unsigned char>> &src,
                                             const std::vector<std::vector<float>> &scales, const std::vector<float> &bias,
                                             const std::vector<u8> &table) {
  const size_t elems = (size_t)j.bs * j.h * j.w * j.c;
  std::vector<unsigned char> out(elems * esize(j.dst));
  for (size_t i = 0; i < elems; ++i) {
    const int k = (int)(i % j.c);
    volatile float v = 0.0f;
    for (size_t s = 0; s < src.size(); ++s) {
      volatile float term = load(src[s].data(), j.src[s], i) * scales[s][scales[s].size() == 1 ? 0 : k];
      v = s == 0 ? term : v + term;
    }
    if (!bias.empty()) v = v + bias[bias.size() == 1 ? 0 : k];
    if (j.relu && 0.0f > v) v = 0.0f;
    if (j.table_in != DT::undef) out[i] = table[cvt(v, j.rm, j.table_in == DT::u8) + (j.table_in == DT::s8 ? 128 : 0)];
    else if (j.dst == DT::f32) { const float f = v; memcpy(&out[i * 4], &f, 4); }
    else out[i] = (unsigned char)cvt(v, j.rm, j.dst == DT::u8);
  }
  return out;
}

static unsigned long long fnv(const void *p, size_t n) {
  unsigned long long h = 1469598103934665603ull;
  for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char *)p)[i]) * 1099511628211ull;
  return h;
}

static int run(const Join &j, Lcg &g) {
  const size_t elems = (size_t)j.bs * j.h * j.w * j.c;
  const size_t n = j.src.size();
  std::vector<std::unique_ptr<memory>> srcs;
  std::vector<std::vector<unsigned char>> copy(n);
  for (size_t s = 0; s < n; ++s) {
    if (j.twice && s == 1) {
      copy[1] = copy[0];
      continue;
    }
    srcs.push_back(mk(j.bs, j.c, j.h, j.w, j.src[s]));
    void *p = srcs.back()->data();
    for (size_t i = 0; i < elems; ++i) {
      const unsigned r = g.next();
      if (j.src[s] == DT::f32) ((float *)p)[i] = (float)((int)(r % 2001) - 1000) * 0.25f;
      else if (j.src[s] == DT::s32) ((int32_t *)p)[i] = (r % 64 == 0) ? (int32_t)(r * 2654435761u) : (int32_t)(r % 3001) - 1500;
      else ((uint8_t *)p)[i] = (uint8_t)(r & 0xff);
    }
    copy[s].assign((unsigned char *)p, (unsigned char *)p + elems * esize(j.src[s]));
  }
  std::vector<std::vector<float>> scales(n);
  for (size_t s = 0; s < n; ++s) {
    scales[s].resize(j.per_channel[s] ? j.c : 1);
    for (size_t k = 0; k < scales[s].size(); ++k)
      scales[s][k] = (s % 2 ? -0.5f : 0.75f) * (1.0f + 0.25f * (float)(k % 5)) * (j.src[s] == DT::s32 ? 0.125f : 1.0f);
  }
  std::vector<float> bias(j.bias == 0 ? 0 : j.bias == 1 ? 1 : j.c);
  for (size_t k = 0; k < bias.size(); ++k) bias[k] = (float)((int)(k % 9) - 4) * 0.5f;
  std::vector<u8> table;
  if (j.table_in != DT::undef)
    for (int i = 0; i < 256; ++i) table.push_back((u8)((i * 167 + 13) & 0xff));  // a permutation

  // the C ABI on the same numbers, host to host
  dfx_wsum_desc d;
  memset(&d, 0, sizeof(d));
  d.bs = j.bs; d.h = j.h; d.w = j.w; d.c = j.c; d.n_inputs = (int)n;
  for (size_t s = 0; s < n; ++s) { d.src_dt[s] = (int)j.src[s]; d.nscales[s] = (int)scales[s].size(); }
  d.n_bias = (int)bias.size(); d.dst_dt = (int)j.dst;
  d.round_mode = j.rm == round_mode::down ? DFX_ROUND_DOWN : DFX_ROUND_NEAREST;
  d.post_relu = j.relu; d.lut_in_dt = (int)j.table_in; d.force_path = -1;
  dfx_wsum_t *h = nullptr;
  std::vector<const float *> sp;
  for (auto &s : scales) sp.push_back(s.data());
  std::vector<const void *> hp;
  for (auto &c : copy) hp.push_back(c.data());
  std::vector<unsigned char> abi(elems * esize(j.dst));
  if (dfx_wsum_create(&d, &h) != DFX_OK || dfx_wsum_set_params(h, sp.data(), bias.empty() ? nullptr : bias.data(), table.empty() ? nullptr : table.data()) != DFX_OK ||
      dfx_wsum_submit_host(h, hp.data(), abi.data()) != DFX_OK) {
    printf("wsum_check %-12s: the C ABI failed: %s\n", j.name, dfx_last_error());
    return 1;
  }
  dfx_wsum_info info;
  dfx_wsum_query(h, &info);
  dfx_wsum_destroy(h);

  // the C++ API.  The op takes a vector of unique_ptrs, so a tensor given twice is borrowed for the call: `lend` gives it
  // back on every way out of this function, an exception included (the library's own error_and_exit() ends the process).
  // dst is the source's own unique_ptr when the join runs in place.
  std::vector<std::unique_ptr<memory>> args;
  for (size_t s = 0, t = 0; s < n; ++s) {
    if (j.twice && s == 1) args.push_back(std::unique_ptr<memory>(args[0].get()));
    else args.push_back(std::move(srcs[t++]));
  }
  struct Lend {
    std::vector<std::unique_ptr<memory>> &v;
    bool on;
    ~Lend() { if (on) v[1].release(); }
  } lend{args, j.twice};
  std::unique_ptr<memory> other;
  if (j.in_place < 0) {
    other = mk(j.bs, j.c, j.h, j.w, j.dst);
    memset(other->data(), 0xA5, other->buffer_size());
  }
  std::unique_ptr<memory> &dst = j.in_place >= 0 ? args[j.in_place] : other;
  int bad = 0;
  {
    auto op = scaled_sum(args, scales, dst, bias, j.relu, table, j.table_in, j.rm);
    op->submit();
    const std::vector<unsigned char> want = scalar_ref(j, copy, scales, bias, table);
    const bool abad = memcmp(want.data(), abi.data(), want.size()) != 0;
    const bool cbad = memcmp(want.data(), dst->host_data(), want.size()) != 0;
    bad = abad || cbad;
    printf("wsum_check %-12s bs %2d %3dx%-3dx%4d n %zu%s: C ABI %s; scaled_sum %s; hash %016llx  %s\n", j.name, j.bs, j.h, j.w, j.c, n,
           j.in_place >= 0 ? " in place" : "", abad ? "DIFFERENT from the scalar loop" : "identical", cbad ? "DIFFERENT from the scalar loop" : "identical",
           fnv(dst->host_data(), want.size()), info.kernel_name);
  }
  return bad;
}

int main() {
  Lcg g(777);
  const DT U = DT::undef;
  const std::vector<Join> joins = {
      {"res_shortcut", 3, 14, 14, 64, {DT::u8, DT::u8}, DT::u8, {false, false}, 0, true, U, round_mode::nearest, -1, false},
      {"res_in_place", 2, 7, 7, 128, {DT::u8, DT::u8}, DT::u8, {true, false}, 2, true, U, round_mode::nearest, 0, false},
      {"mbv2_s8", 4, 14, 14, 96, {DT::s8, DT::s8}, DT::s8, {false, false}, 1, false, U, round_mode::down, 1, false},
      {"conv_s32", 2, 9, 11, 32, {DT::u8, DT::s32}, DT::u8, {false, true}, 2, true, U, round_mode::nearest, -1, false},
      {"mixed_f32", 3, 5, 3, 17, {DT::f32, DT::u8, DT::s8, DT::s32}, DT::f32, {true, false, true, false}, 0, false, U, round_mode::nearest, 0, false},
      {"hswish", 2, 12, 12, 32, {DT::s8}, DT::u8, {false}, 0, false, DT::s8, round_mode::nearest, -1, false},
      {"twice_c72", 2, 4, 4, 72, {DT::u8, DT::u8, DT::s8}, DT::s8, {false, true, false}, 1, false, DT::u8, round_mode::down, -1, true},
      {"pixel", 5, 1, 1, 1, {DT::s32}, DT::s8, {false}, 1, true, U, round_mode::nearest, -1, false},
  };
  int bad = 0;
  for (const Join &j : joins) bad += run(j, g);
  if (bad) {
    printf("wsum_check: %d of %zu joins FAILED\n", bad, joins.size());
    return 1;
  }
  printf("wsum_check: every join identical to the scalar loop (%zu joins)\n", joins.size());
  return 0;
}
