// reorder_check -- exercises deepfusion::reorder (include/deepfusion.h) through the drop-in C++ API: a few
// stand-alone reorders and a reorder -> conv -> reorder chain (f32 nchw activations quantised and transposed
// for the fused int8 conv, its s32 nhwc result scaled back to f32 nchw).  Dumps inputs and results as raw
// files; tests/test_gpu_reorder.py re-checks them against the CPU reference.
//   reorder_check <outdir>
#include <cstdio>
#include <cstring>
#include <string>

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

// half-integers in [-200, 400]: every other value is an exact rounding tie, both clamp bounds are crossed
static void fill_f32(memory &m, Lcg &g) {
  float *p = (float *)m.data();
  for (size_t i = 0; i < m.size(); ++i) p[i] = (float)((int)(g.next() % 1201) - 400) / 2.0f;
}

int main(int argc, char **argv) {
  const std::string out = argc > 1 ? argv[1] : ".";
  Lcg g(4242);
  const auto nchw = memory::format::nchw, nhwc = memory::format::nhwc;
  // ---- image entry: f32 nchw 3 channels -> u8 nhwc padded to 16, one scale ----
  {
    auto src = mk(3, 3, 10, 13, nchw, memory::dtype::f32), dst = mk(3, 16, 10, 13, nhwc, memory::dtype::u8);
    fill_f32(*src, g);
    auto r = reorder(src, dst, {0.5f});
    r->submit();
    dump(out + "/img_src.bin", src->host_data(), src->buffer_size());
    dump(out + "/img_dst.bin", dst->host_data(), dst->buffer_size());
  }
  // ---- s32 nhwc -> f32 nchw, per-channel scales ----
  {
    const int c = 24;
    auto src = mk(5, c, 7, 9, nhwc, memory::dtype::s32), dst = mk(5, c, 7, 9, nchw, memory::dtype::f32);
    int32_t *p = (int32_t *)src->data();
    for (size_t i = 0; i < src->size(); ++i) p[i] = (int)(g.next() % 20001) - 10000 + (i % 97 == 0 ? 16777217 : 0);
    std::vector<float> sc(c);
    for (int k = 0; k < c; ++k) sc[k] = 0.013f * (float)(k + 1);
    auto r = reorder(src, dst, sc);
    r->submit();
    dump(out + "/deq_src.bin", src->host_data(), src->buffer_size());
    dump(out + "/deq_sc.bin", sc.data(), sc.size() * 4);
    dump(out + "/deq_dst.bin", dst->host_data(), dst->buffer_size());
  }
  // ---- same layout with channel padding: f32 nhwc 17 -> s8 nhwc 32, round down, no scale ----
  {
    auto src = mk(4, 17, 5, 6, nhwc, memory::dtype::f32), dst = mk(4, 32, 5, 6, nhwc, memory::dtype::s8);
    fill_f32(*src, g);
    auto r = reorder(src, dst, {}, round_mode::down);
    r->submit();
    dump(out + "/pad_src.bin", src->host_data(), src->buffer_size());
    dump(out + "/pad_dst.bin", dst->host_data(), dst->buffer_size());
  }
  // ---- same layout, same channels: u8 nchw -> f32 nchw ----
  {
    auto src = mk(3, 40, 6, 8, nchw, memory::dtype::u8), dst = mk(3, 40, 6, 8, nchw, memory::dtype::f32);
    uint8_t *p = (uint8_t *)src->data();
    for (size_t i = 0; i < src->size(); ++i) p[i] = (uint8_t)(g.next() % 256);
    auto r = reorder(src, dst);
    r->submit();
    dump(out + "/flat_src.bin", src->host_data(), src->buffer_size());
    dump(out + "/flat_dst.bin", dst->host_data(), dst->buffer_size());
  }
  // ---- chain: f32 nchw -> [reorder] -> u8 nhwc -> [fused conv3x3 + relu + conv1x1, s32 out] -> s32 nhwc
  //      -> [reorder, per-channel scales] -> f32 nchw.  Single device: three submit_async() calls, the
  //      intermediates never visit the host.  With DEEPFUSION_DEVICES (batch shards work host to host) the
  //      same files come from synchronous submits. ----
  {
    const int bs = 5, ic = 32, ih = 9, iw = 11, oc = 32, oc1 = 32;
    auto x = mk(bs, ic, ih, iw, nchw, memory::dtype::f32), q = mk(bs, ic, ih, iw, nhwc, memory::dtype::u8);
    auto acc = mk(bs, oc1, ih, iw, nhwc, memory::dtype::s32), y = mk(bs, oc1, ih, iw, nchw, memory::dtype::f32);
    std::unique_ptr<memory> wei(new memory(memory::nchw_dims{oc, ic, 3, 3}, memory::format::OIhw4i16o4i, memory::dtype::s8));
    std::unique_ptr<memory> wei1(new memory(memory::nchw_dims{oc1, oc, 1, 1}, memory::format::OIhw4i16o4i, memory::dtype::s8));
    static const std::unique_ptr<memory> none;
    float *px = (float *)x->data();
    for (size_t i = 0; i < x->size(); ++i) px[i] = (float)((int)(g.next() % 801) - 100) / 8.0f;  // [-12.5, 87.5]
    std::vector<s8> w0(wei->size()), w1(wei1->size());
    for (auto &v : w0) v = (s8)((int)(g.next() % 21) - 10);
    for (auto &v : w1) v = (s8)((int)(g.next() % 21) - 10);
    reorder_weights(w0.data(), wei);
    reorder_weights(w1.data(), wei1);
    std::vector<float> sc_in(ic), sc_out(oc1);
    for (int k = 0; k < ic; ++k) sc_in[k] = 0.15f + 0.005f * (float)k;
    for (int k = 0; k < oc1; ++k) sc_out[k] = 0.001f * (float)(k + 3);
    auto r0 = reorder(x, q, sc_in);
    auto c = conv(q, wei, none, {1, 1}, {1, 1}, wei1, none, acc, true, {1.f / 256}, round_mode::nearest, false, {1.f / 8},
                  round_mode::nearest);
    auto r1 = reorder(acc, y, sc_out);
    const char *dv = getenv("DEEPFUSION_DEVICES");
    const bool sharded = dv && *dv && strcmp(dv, "1") != 0;
    if (!sharded) {
      r0->submit_async();
      memset(const_cast<void *>(q->host_data()), 0xEE, q->buffer_size());      // stale host bytes must not be uploaded
      c->submit_async();
      memset(const_cast<void *>(acc->host_data()), 0xEE, acc->buffer_size());
      r1->submit_async();
      r1->wait();
      y->download();
    } else {
      r0->submit();
      c->submit();
      r1->submit();
    }
    dump(out + "/chain_x.bin", x->host_data(), x->buffer_size());
    dump(out + "/chain_w0_oihw.bin", w0.data(), w0.size());
    dump(out + "/chain_w1_oihw.bin", w1.data(), w1.size());
    dump(out + "/chain_sc_in.bin", sc_in.data(), sc_in.size() * 4);
    dump(out + "/chain_sc_out.bin", sc_out.data(), sc_out.size() * 4);
    dump(out + "/chain_y.bin", y->host_data(), y->buffer_size());
  }
  printf("reorder_check: wrote results to %s\n", out.c_str());
  return 0;
}
