// pipeline_net.h -- one small network that uses 14 op classes of include/deepfusion.h once -- reorder, image_conv,
// depthwise_separable_conv, grouped_conv, dilated_conv, depthwise_conv, deconvolution, resize_add, concat_conv, conv,
// eltwise_sum, conv_relu_pool, concat, inner_product -- with the tensors staying on the device between the ops.  Shared by
// coherence_check.cc (a recording fake behind the API, no GPU) and pipeline_check.cc (the real libraries, whose numerics
// reference follows this table: it does not change lightly).  The other ten classes -- scaled_sum, head, layer_norm,
// linear, select, nms, roialign, matmul, attention, squeeze_excite -- are driven by token_net in coherence_check.cc
// (scenarios g and h) and by their own GPU tests.  Batch 3, so that two batch shards split 2 + 1.
//
//   x_f  f32 nchw {3,3,20,20}   the caller's input of frame f (F of them)
//   q    = reorder(x_f)                          u8 nhwc {3,3,20,20}     F ops, one per frame
//   a    = image_conv(q) 3x3 / 2, pad 1          {3,32,10,10}            MFMA class
//   b    = depthwise_separable_conv(a) 3x3 / 1   {3,64,10,10}
//   c    = grouped_conv(b) 3x3 / 2, groups 8     {3,64,5,5}              MFMA class
//   d    = dilated_conv(c) 3x3, d = 2, pad 2     {3,64,5,5}              MFMA class
//   d2   = depthwise_conv(d) 3x3 / 1             {3,64,5,5}
//   e    = deconvolution(d2) 2x2 / 2             {3,64,10,10}            MFMA class
//   e    = resize_add(d, lateral = e, dst = e)   nearest x2, in place    band class
//   f    = concat_conv({b, e}) 1x1 -> 64         {3,64,10,10}            two launches
//   g    = conv(f) 3x3 + 1x1, 64 -> 32 -> 64     {3,64,10,10}
//   h    = eltwise_sum({g, b}) + relu            {3,64,10,10}
//   i    = conv_relu_pool(h) 3x3 + 2x2 / 2 max   {3,64,5,5}
//   j    = concat({i, c, d})                     {3,192,5,5}
//   k_f  = inner_product(j) -> 10, f32           {3,10,1,1}              F ops, one per frame
//
// b, c and d have two or three readers on different streams; f, h and j join tensors of different producer streams; e is
// updated in place.  With F > 1 the F first ops all write q and the F last ops all read j: F frames can be in flight.
#pragma once
#include <initializer_list>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "deepfusion.h"

namespace pipeline {

using deepfusion::memory;
using deepfusion::op;
typedef std::unique_ptr<memory> mem_ptr;

// where the bytes of inputs, weights, biases and scales come from
struct source {
  virtual ~source() {}
  virtual void fill(const std::string &name, void *p, size_t bytes) = 0;
  virtual std::vector<float> scales(const std::string &name) = 0;
};

struct net {
  enum { N = 3, CLASSES = 10 };
  int F;
  std::vector<mem_ptr> x, k;
  mem_ptr q, a, b, c, d, d2, e, f, g, h, i, j;
  std::vector<mem_ptr> weights;                     // borrowed by the ops: they live as long as the net
  std::vector<std::unique_ptr<op>> first, last;     // F each
  std::vector<std::unique_ptr<op>> mid;             // the twelve ops between them, in submit order
  std::vector<std::string> mid_names;
  std::vector<memory *> mid_dst;                    // what each of them writes

  static mem_ptr act(int c, int h, int w, memory::dtype dt = memory::dtype::u8, memory::format fmt = memory::format::nhwc) {
    return mem_ptr(new memory(memory::nchw_dims{N, c, h, w}, fmt, dt));
  }
  // plain oihw s8 weights
  memory *wei(source &s, const std::string &name, int o, int i, int kh, int kw) {
    weights.emplace_back(new memory(memory::nchw_dims{o, i, kh, kw}, memory::format::oihw, memory::dtype::s8));
    s.fill(name, weights.back()->data(), weights.back()->buffer_size());
    return weights.back().get();
  }
  // OIhw4i16o4i weights, given as plain oihw
  memory *blocked(source &s, const std::string &name, int o, int i, int kh, int kw) {
    std::vector<deepfusion::s8> plain((size_t)o * i * kh * kw);
    s.fill(name, plain.data(), plain.size());
    weights.emplace_back(new memory(memory::nchw_dims{o, i, kh, kw}, memory::format::OIhw4i16o4i, memory::dtype::s8));
    deepfusion::reorder_weights(plain.data(), weights.back());
    return weights.back().get();
  }
  memory *bias(source &s, const std::string &name, int n) {
    weights.emplace_back(new memory(memory::dims{n}, memory::format::x, memory::dtype::s32));
    s.fill(name, weights.back()->data(), weights.back()->buffer_size());
    return weights.back().get();
  }
  // the factories take unique_ptr references and keep the raw pointers: lend them one for the call
  struct lent {
    std::vector<mem_ptr> v;
    explicit lent(std::initializer_list<memory *> ms) {
      for (memory *m : ms) v.emplace_back(m);
    }
    ~lent() {
      for (mem_ptr &p : v) p.release();
    }
    const mem_ptr &operator[](size_t n) const { return v[n]; }
  };
  void add(const char *name, std::unique_ptr<op> o) {
    mid_names.push_back(name);
    mid.push_back(std::move(o));
  }

  net(int frames, source &s) : F(frames) {
    using namespace deepfusion;
    const memory::dtype f32 = memory::dtype::f32;
    for (int n = 0; n < F; ++n) {
      x.push_back(act(3, 20, 20, f32, memory::format::nchw));
      k.push_back(act(CLASSES, 1, 1, f32));
    }
    q = act(3, 20, 20); a = act(32, 10, 10); b = act(64, 10, 10); c = act(64, 5, 5); d = act(64, 5, 5); d2 = act(64, 5, 5);
    e = act(64, 10, 10); f = act(64, 10, 10); g = act(64, 10, 10); h = act(64, 10, 10); i = act(64, 5, 5); j = act(192, 5, 5);
    for (int n = 0; n < F; ++n) first.push_back(reorder(x[n], q, s.scales("q_s")));
    {
      lent w{wei(s, "a_w", 32, 3, 3, 3), bias(s, "a_b", 32)};
      add("image_conv", image_conv(q, w[0], w[1], {2, 2}, {1, 1}, a, true, s.scales("a_s")));
    }
    {
      lent w{wei(s, "b_wdw", 32, 1, 3, 3), bias(s, "b_bdw", 32), blocked(s, "b_wpw", 64, 32, 1, 1), bias(s, "b_bpw", 64)};
      add("depthwise_separable_conv",
          depthwise_separable_conv(a, w[0], w[1], {1, 1}, {1, 1}, w[2], w[3], b, true, s.scales("b_s0"), s.scales("b_s1")));
    }
    {
      lent w{wei(s, "c_w", 64, 8, 3, 3), bias(s, "c_b", 64)};
      add("grouped_conv", grouped_conv(b, w[0], w[1], 8, {2, 2}, {1, 1}, c, true, s.scales("c_s")));
    }
    {
      lent w{wei(s, "d_w", 64, 64, 3, 3), bias(s, "d_b", 64)};
      add("dilated_conv", dilated_conv(c, w[0], w[1], {1, 1}, {2, 2}, {2, 2}, d, true, s.scales("d_s")));
    }
    {
      lent w{wei(s, "d2_w", 64, 1, 3, 3), bias(s, "d2_b", 64)};
      add("depthwise_conv", depthwise_conv(d, w[0], w[1], {1, 1}, {1, 1}, d2, true, s.scales("d2_s")));
    }
    {
      lent w{wei(s, "e_w", 64, 64, 2, 2), bias(s, "e_b", 64)};
      add("deconvolution", deconvolution(d2, w[0], w[1], {2, 2}, {0, 0}, e, true, s.scales("e_s")));
    }
    add("resize_add", resize_add(d, e, e, resize_algo::nearest, resize_coord::asymmetric, false));
    {
      lent w{blocked(s, "f_w", 64, 128, 1, 1), bias(s, "f_b", 64)}, srcs{b.get(), e.get()};
      add("concat_conv", concat_conv(srcs.v, w[0], w[1], f, true, s.scales("f_s")));
    }
    {
      lent w{blocked(s, "g_w0", 32, 64, 3, 3), bias(s, "g_b0", 32), blocked(s, "g_w1", 64, 32, 1, 1), bias(s, "g_b1", 64)};
      add("conv", conv(f, w[0], w[1], {1, 1}, {1, 1}, w[2], w[3], g, true, s.scales("g_s0"), round_mode::nearest, true,
                       s.scales("g_s1"), round_mode::nearest));
    }
    {
      lent srcs{g.get(), b.get()};
      add("eltwise_sum", eltwise_sum(srcs.v, h, true));
    }
    {
      lent w{blocked(s, "i_w", 64, 64, 3, 3), bias(s, "i_b", 64)};
      add("conv_relu_pool", conv_relu_pool(h, w[0], w[1], {1, 1}, {1, 1}, {2, 2}, {2, 2}, {0, 0}, i, true, s.scales("i_s")));
    }
    {
      lent srcs{i.get(), c.get(), d.get()};
      add("concat", concat(srcs.v, j, false));
    }
    mid_dst = {a.get(), b.get(), c.get(), d.get(), d2.get(), e.get(), e.get(), f.get(), g.get(), h.get(), i.get(), j.get()};
    lent w{wei(s, "k_w", CLASSES, 192, 5, 5), bias(s, "k_b", CLASSES)};
    for (int n = 0; n < F; ++n) last.push_back(inner_product(j, w[0], w[1], k[n], false, s.scales("k_s")));
  }

  // every intermediate, by the names of the table above ("e" is the tensor after the in-place resize_add)
  std::vector<std::pair<std::string, memory *>> intermediates() {
    return {{"q", q.get()}, {"a", a.get()}, {"b", b.get()}, {"c", c.get()}, {"d", d.get()}, {"d2", d2.get()}, {"e", e.get()},
            {"f", f.get()}, {"g", g.get()}, {"h", h.get()}, {"i", i.get()}, {"j", j.get()}};
  }
};

}  // namespace pipeline
