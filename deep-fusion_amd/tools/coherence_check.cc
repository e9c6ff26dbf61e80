// coherence_check -- is the host/device coherence protocol of host/deepfusion.cc (detail::memory_state, detail::op_state)
// free of data races when ops are chained with the tensors staying on the device?  No GPU: the program is
// host/deepfusion.cc + dfx_trace_stub.cc (a recording fake of the C ABI) + this file.  It drives the network of
// pipeline_net.h through include/deepfusion.h, marks its own reads and writes of tensor bytes in the trace, and then walks
// the trace with vector clocks: program order per stream and on the host thread, dfx_stream_wait_stream and
// dfx_stream_sync as the edges between them (work is enqueued by the host, so it follows everything the host had
// done or waited for by then; dfx_stream_destroy orders nothing).  The rule:
//     for every two accesses to overlapping bytes of one buffer, at least one of them a write, one happens-before the other.
// Every violating pair is printed; the exit status is non-zero on any, and on anything the fake itself refused (a
// destroyed stream used again, a range outside every allocation).
//   coherence_check <scenario> [--dump]     scenario: a | b | c | d | e | f | g | h  (f and h want DEEPFUSION_DEVICES=2
//                                           DFX_TRACE_DEVICES=2); a - f drive pipeline_net.h, g and h token_net below
//   --dump prints the trace, one line per record, in a form that two builds can be diffed by: every call of the C ABI in
//   call order (tests/golden/coherence/ holds the dumps of the revision before the op classes shared one skeleton)
//   coherence_check selftest-ordered | selftest-race     the checker on a hand-made trace through the C ABI itself: a
//     write, a read on another stream, a rewrite, a host write, with the edges that order them (exit 0) and without any
//     (four pairs and one use of a destroyed stream reported, exit 1)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "dfx.h"
#include "dfx_trace.h"
#include "pipeline_net.h"

using pipeline::memory;
using pipeline::net;

namespace {

std::map<int, std::string> g_names;  // allocation id -> tensor name

void name_tensor(const std::string &n, memory *m, bool device) {
  g_names[dfx_trace::buffer_of(m->host_data())] = n + " (host)";
  if (device) g_names[dfx_trace::buffer_of(m->device_data())] = n + " (device)";
}
std::string range_name(const dfx_trace::range &r) {
  auto it = g_names.find(r.buf);
  return it != g_names.end() ? it->second : dfx_trace::describe(r);
}

// no arithmetic runs, so the bytes do not matter: a fill only has to appear in the trace
struct marking_source : pipeline::source {
  void fill(const std::string &name, void *p, size_t bytes) override {
    memset(p, 1, bytes);
    if (dfx_trace::buffer_of(p) >= 0) dfx_trace::host_access(("fill " + name).c_str(), p, bytes, true);
  }
  std::vector<float> scales(const std::string &) override { return {1.f}; }
};

void fill(memory *m, const std::string &name, int byte = 2) {
  void *p = m->data();
  memset(p, byte, m->buffer_size());
  dfx_trace::host_access(("host fills " + name).c_str(), p, m->buffer_size(), true);
}
void read(memory *m, const std::string &name) {
  dfx_trace::host_access(("host reads " + name).c_str(), m->host_data(), m->buffer_size(), false);
}
std::string fr(const char *n, int f) { return std::string(n) + "_" + std::to_string(f); }

void name_all(net &n, bool device) {
  for (int f = 0; f < n.F; ++f) {
    name_tensor(fr("x", f), n.x[f].get(), device);
    name_tensor(fr("k", f), n.k[f].get(), device);
  }
  for (auto &t : n.intermediates()) name_tensor(t.first, t.second, device);
}

// (a) every op with submit(); the host reads every result
void scenario_a(net &n) {
  fill(n.x[0].get(), "x_0");
  n.first[0]->submit();
  read(n.q.get(), "q");
  for (size_t m = 0; m < n.mid.size(); ++m) {
    n.mid[m]->submit();
    read(n.mid_dst[m], "dst of " + n.mid_names[m]);
  }
  n.last[0]->submit();
  read(n.k[0].get(), "k_0");
}

// (b) one frame of submit_async(), one wait() on the last op, then the outputs are downloaded
void scenario_b(net &n) {
  fill(n.x[0].get(), "x_0");
  n.first[0]->submit_async();
  for (auto &o : n.mid) o->submit_async();
  n.last[0]->submit_async();
  n.last[0]->wait();
  n.k[0]->download();
  read(n.k[0].get(), "k_0");
  for (auto &t : n.intermediates()) {
    t.second->download();
    read(t.second, t.first);
  }
}

// (c) F frames in flight: nothing waits until every frame has been submitted
void scenario_c(net &n) {
  for (int f = 0; f < n.F; ++f) fill(n.x[f].get(), fr("x", f));
  for (int f = 0; f < n.F; ++f) {
    n.first[f]->submit_async();
    for (auto &o : n.mid) o->submit_async();
    n.last[f]->submit_async();
  }
  for (int f = 0; f < n.F; ++f) {
    n.last[f]->wait();
    n.k[f]->download();
    read(n.k[f].get(), fr("k", f));
  }
}

// (d) synchronous and asynchronous submits mixed, both ways round, and an input refilled between two frames
void scenario_d(net &n) {
  for (int frame = 0; frame < 2; ++frame) {
    if (frame) n.first[0]->wait();  // the upload of x_0 has finished: the host may rewrite it
    fill(n.x[0].get(), "x_0");
    n.first[0]->submit_async();
    for (size_t m = 0; m < n.mid.size(); ++m) {
      if ((m + frame) % 2) {
        n.mid[m]->submit_async();
      } else {
        n.mid[m]->submit();
        read(n.mid_dst[m], "dst of " + n.mid_names[m]);
      }
    }
    if (frame) {
      n.last[0]->submit_async();
      n.last[0]->wait();
      n.k[0]->download();
    } else {
      n.last[0]->submit();
    }
    read(n.k[0].get(), "k_0");
  }
}

// (e) ops destroyed while their launch is in flight (writers and readers), then other streams use the tensors
void scenario_e(net &n) {
  fill(n.x[0].get(), "x_0");
  fill(n.x[1].get(), "x_1");
  n.first[0]->submit_async();
  n.first[0].reset();        // the writer of q goes while it writes
  n.mid[0]->submit_async();  // image_conv reads q, writes a
  n.mid[0].reset();          // a reader (of q) and writer (of a) goes in flight
  n.first[1]->submit_async();  // another stream overwrites q: it must not wait on a stream that is gone
  for (size_t m = 1; m < n.mid.size(); ++m) {
    n.mid[m]->submit_async();
    if (m == 2 || m == 6 || m == 9) n.mid[m].reset();  // grouped_conv (reads b), resize_add (in place), eltwise_sum (two inputs)
  }
  n.mid[1]->submit_async();  // depthwise_separable_conv again: rewrites b, whose readers are partly gone
  n.mid[5].reset();          // deconvolution: no longer the last writer of e (resize_add was), still a reader of d2
  n.mid[4]->submit_async();  // depthwise_conv rewrites d2
  n.last[1]->submit();
  read(n.k[1].get(), "k_1");
  n.last[0]->submit_async();
  n.last[0].reset();
  n.k[0]->download();
  read(n.k[0].get(), "k_0");
}

// (f) batch shards (DEEPFUSION_DEVICES=2, batch 3): submit() per op, then submit_async() with the producer's wait() before
// every consumer, which is the documented contract there
void scenario_f(net &n) {
  scenario_a(n);
  fill(n.x[0].get(), "x_0");
  n.first[0]->submit_async();
  n.first[0]->wait();
  for (size_t m = 0; m < n.mid.size(); ++m) {
    n.mid[m]->submit_async();
    n.mid[m]->wait();
    read(n.mid_dst[m], "dst of " + n.mid_names[m]);
  }
  n.last[0]->submit_async();
  n.last[0]->wait();
  read(n.k[0].get(), "k_0");
}

// ---- token_net: the ten op classes pipeline_net.h does not use (it is shared with pipeline_check, whose numerics reference
// a change of it would break), chained on the device at batch 3.  The fake runs no arithmetic: shapes only have to pass
// the constructors' checks.  All tensors nhwc; a token is a pixel of a 2 x 2 image with 32 channels.
//   x        u8 {3,32,2,2}, anchors f32 {4,4,1,1}     the caller's inputs
//   ln       = layer_norm(x)                          s8 {3,32,2,2}      sharded under DEEPFUSION_DEVICES
//   lin      = linear(ln)  32 -> 32                   s8 {3,32,2,2}      borrowed weights
//   mm       = matmul(ln, lin^T) per image            s8 {3,4,2,2}
//   at       = attention(ln, lin, lin) per image      u8 {3,32,2,2}
//   ss       = scaled_sum({at, x})                    u8 {3,32,2,2}      sharded
//   se       = squeeze_excite(ss)  32 -> 8 -> 32      u8 {3,32,2,2}      sharded, borrowed weights
//   hd_idx, hd_val = top_k(se, k = 2)                 s32 / u8 {3,2,2,2} sharded, two outputs
//   sel_idx, sel_count, sel_val, gd = select_top_k(se, k = 4, gather ss -> gd)   s32 {3,4,1,1}, s32 {3,1,1,1}, u8 {3,4,1,1}, u8 {3,32,4,1}
//   keep, count2, boxes = box_nms(sel_idx, deltas = gd, anchors, count_in = sel_count)   decode form: two tables of its own
//   roi      = roi_align({ss}, boxes, count2)         u8 {6,32,2,2}
// ln has three readers on three streams, lin two, ss three, se two; at and x join in ss; sel_idx, sel_count and gd go from
// select to nms, boxes and count2 from nms to roi_align.
struct token_net {
  typedef pipeline::mem_ptr mem_ptr;
  typedef pipeline::net::lent lent;
  enum { N = 3, LAYER_NORM = 0, LINEAR, MATMUL, ATTENTION, SCALED_SUM, SQUEEZE_EXCITE, HEAD, SELECT, NMS, ROIALIGN };
  struct stage {
    std::string name;
    std::unique_ptr<pipeline::op> o;
    std::vector<std::pair<std::string, memory *>> outs;
    bool sharded;  // under DEEPFUSION_DEVICES > 1 the class works host to host
  };
  mem_ptr x, anchors, ln, lin, mm, at, ss, se, hd_idx, hd_val, sel_idx, sel_count, sel_val, gd, keep, count2, boxes, roi;
  std::vector<mem_ptr> weights;  // borrowed by linear and squeeze_excite
  memory *lin_w, *se_w1;
  std::vector<stage> ops;

  static mem_ptr act(int n, int c, int h, int w, memory::dtype dt) {
    return mem_ptr(new memory(memory::nchw_dims{n, c, h, w}, memory::format::nhwc, dt));
  }
  memory *wei(const std::string &name, int o, int i) {
    weights.emplace_back(new memory(memory::nchw_dims{o, i, 1, 1}, memory::format::oihw, memory::dtype::s8));
    fill(weights.back().get(), name);
    return weights.back().get();
  }
  memory *bias(const std::string &name, int n) {
    weights.emplace_back(new memory(memory::dims{n}, memory::format::x, memory::dtype::s32));
    fill(weights.back().get(), name);
    return weights.back().get();
  }
  void add(const char *name, std::unique_ptr<pipeline::op> o, bool sharded, std::vector<std::pair<std::string, memory *>> outs) {
    ops.push_back(stage{name, std::move(o), std::move(outs), sharded});
  }

  token_net() {
    using namespace deepfusion;
    typedef memory::dtype dt;
    x = act(N, 32, 2, 2, dt::u8); anchors = act(4, 4, 1, 1, dt::f32);
    ln = act(N, 32, 2, 2, dt::s8); lin = act(N, 32, 2, 2, dt::s8); mm = act(N, 4, 2, 2, dt::s8); at = act(N, 32, 2, 2, dt::u8);
    ss = act(N, 32, 2, 2, dt::u8); se = act(N, 32, 2, 2, dt::u8); hd_idx = act(N, 2, 2, 2, dt::s32); hd_val = act(N, 2, 2, 2, dt::u8);
    sel_idx = act(N, 4, 1, 1, dt::s32); sel_count = act(N, 1, 1, 1, dt::s32); sel_val = act(N, 4, 1, 1, dt::u8); gd = act(N, 32, 4, 1, dt::u8);
    keep = act(N, 2, 1, 1, dt::s32); count2 = act(N, 1, 1, 1, dt::s32); boxes = act(N, 4, 2, 1, dt::f32); roi = act(N * 2, 32, 2, 2, dt::u8);
    const std::array<long long, 3> st = attention_strides(N, 1, 4, 32);  // one head: a {4, 32} matrix per image
    std::array<uint32_t, 256> exp_table;
    std::array<u8, 256> gate_table;
    std::array<float, 256> tab;
    exp_table.fill(1); gate_table.fill(1); tab.fill(1.f);
    add("layer_norm", layer_norm(x, std::vector<float>(32, 1.f), {}, ln, 1.f), true, {{"ln", ln.get()}});
    {
      lent w{lin_w = wei("lin_w", 32, 32), bias("lin_b", 32)};
      add("linear", linear(ln, w[0], w[1], lin), false, {{"lin", lin.get()}});
    }
    add("matmul", matmul(ln, lin, mm, matmul_shape{N, 1, 4, 4, 32, true, st[0], st[1], st[2], st[0], st[1], st[2], 16, 4, 4}, {1.f}), false,
        {{"mm", mm.get()}});
    add("attention",
        attention(ln, lin, lin, exp_table, at,
                  attention_shape{N, 1, 4, 4, 32, 32, st[0], st[1], st[2], st[0], st[1], st[2], st[0], st[1], st[2], st[0], st[1], st[2]}, 1.f, {1.f}),
        false, {{"at", at.get()}});
    {
      lent srcs{at.get(), x.get()};
      add("scaled_sum", scaled_sum(srcs.v, {{1.f}, {1.f}}, ss), true, {{"ss", ss.get()}});
    }
    {
      lent w{se_w1 = wei("se_w1", 8, 32), bias("se_b1", 8), wei("se_w2", 32, 8), bias("se_b2", 32)};
      add("squeeze_excite", squeeze_excite(ss, w[0], w[1], w[2], w[3], gate_table, se), true, {{"se", se.get()}});
    }
    add("head", top_k(se, hd_idx, hd_val.get(), 2), true, {{"hd_idx", hd_idx.get()}, {"hd_val", hd_val.get()}});
    add("select", select_top_k(se, sel_idx, sel_val.get(), sel_count, 4, false, select_all_values, 0, {ss.get()}, {gd.get()}), false,
        {{"sel_idx", sel_idx.get()}, {"sel_count", sel_count.get()}, {"sel_val", sel_val.get()}, {"gd", gd.get()}});
    add("nms", box_nms(sel_idx, gd, anchors, tab, tab, sel_count.get(), keep, count2, boxes.get(), 0.5f, 1, false, 1), false,
        {{"keep", keep.get()}, {"count2", count2.get()}, {"boxes", boxes.get()}});
    add("roialign", roi_align({ss.get()}, {1.f}, {}, boxes.get(), count2.get(), nullptr, roi), false, {{"roi", roi.get()}});
  }

  void name_all(bool device) {
    name_tensor("x", x.get(), device);
    name_tensor("anchors", anchors.get(), device);
    for (stage &s : ops)
      for (auto &t : s.outs) name_tensor(t.first, t.second, device);
  }
  void read_outputs(stage &s, bool download) {
    for (auto &t : s.outs) {
      if (download) t.second->download();
      read(t.second, t.first);
    }
  }
};

// (g) the ten classes of token_net: each with submit() and its outputs read; then two frames of submit_async(), the second
// without a refill but with the weights of linear and squeeze_excite rewritten (the re-pack path: a stream sync, then
// set_weights), one wait() per op, the outputs downloaded; then scaled_sum and matmul destroyed while in flight
void scenario_g(token_net &n) {
  fill(n.x.get(), "x");
  fill(n.anchors.get(), "anchors");
  for (token_net::stage &s : n.ops) {
    s.o->submit();
    n.read_outputs(s, false);
  }
  for (int frame = 0; frame < 2; ++frame) {
    if (frame == 0) {
      fill(n.x.get(), "x");
    } else {
      fill(n.lin_w, "lin_w", 3);  // (other bytes: the hash moves)
      fill(n.se_w1, "se_w1", 3);
    }
    for (token_net::stage &s : n.ops) s.o->submit_async();
  }
  for (token_net::stage &s : n.ops) {
    s.o->wait();
    n.read_outputs(s, true);
  }
  n.ops[token_net::SCALED_SUM].o->submit_async();
  n.ops[token_net::SCALED_SUM].o.reset();      // a class that shards: the writer of ss goes while it writes
  n.ops[token_net::MATMUL].o->submit_async();
  n.ops[token_net::MATMUL].o.reset();          // a class that does not
  n.ops[token_net::SQUEEZE_EXCITE].o->submit_async();  // reads ss: it must not wait on a stream that is gone
  n.ops[token_net::HEAD].o->submit();
  n.read_outputs(n.ops[token_net::HEAD], false);
  n.mm->download();
  read(n.mm.get(), "mm");
}

// (h) token_net over batch shards (DEEPFUSION_DEVICES=2): layer_norm, scaled_sum, squeeze_excite and head shard and work host
// to host, the other six do not.  submit() per op, then submit_async() with the producer's wait() before every consumer,
// scenario f's contract; a class that does not shard leaves its result on the device, so it is downloaded behind the wait().
void scenario_h(token_net &n) {
  fill(n.x.get(), "x");
  fill(n.anchors.get(), "anchors");
  for (token_net::stage &s : n.ops) {
    s.o->submit();
    n.read_outputs(s, false);
  }
  fill(n.x.get(), "x");
  for (token_net::stage &s : n.ops) {
    s.o->submit_async();
    s.o->wait();
    n.read_outputs(s, !s.sharded);
  }
}

// ---- the happens-before check ----
typedef std::vector<unsigned> vclock;
void join(vclock &a, const vclock &b) {
  if (a.size() < b.size()) a.resize(b.size(), 0);
  for (size_t i = 0; i < b.size(); ++i)
    if (b[i] > a[i]) a[i] = b[i];
}
struct access {
  size_t rec;
  int thread;  // 0 = the host, else a stream
  unsigned tick;
  dfx_trace::range r;
};

int check(bool dump) {
  const std::vector<dfx_trace::record> &t = dfx_trace::records();
  std::map<const void *, int> thread_of;  // stream -> index of its clock; the default stream is a stream like any other
  std::vector<vclock> clocks(1);          // [0]: the host thread
  auto thread = [&](const void *s) {
    auto it = thread_of.find(s);
    if (it != thread_of.end()) return it->second;
    const int id = (int)clocks.size();
    thread_of[s] = id;
    clocks.emplace_back();
    return id;
  };
  auto tick = [&](int th) {
    if (clocks[th].size() <= (size_t)th) clocks[th].resize(th + 1, 0);
    return ++clocks[th][th];
  };
  std::map<int, std::vector<access>> by_buffer;
  int races = 0, waits = 0, syncs = 0, copies = 0, launches = 0;
  for (size_t n = 0; n < t.size(); ++n) {
    const dfx_trace::record &r = t[n];
    int th = 0;
    switch (r.k) {
      case dfx_trace::HOST: break;
      case dfx_trace::ACCESS:
        th = thread(r.stream);
        join(clocks[th], clocks[0]);
        if (r.name.find("memcpy") != std::string::npos) ++copies;
        else ++launches;
        break;
      case dfx_trace::SYNC:
        th = thread(r.stream);  // (thread() may grow `clocks`: no reference into it is held across a call)
        join(clocks[0], clocks[th]);
        ++syncs;
        break;
      case dfx_trace::WAIT: {
        th = thread(r.stream);
        const int from = thread(r.other);
        join(clocks[th], clocks[from]);
        ++waits;
        break;
      }
      case dfx_trace::STREAM_DESTROY: break;  // (orders nothing; the fake refuses a later use of the stream)
      case dfx_trace::NOTE: break;            // (a call that touches no memory and orders nothing: printed, nothing else)
    }
    if (dump) {
      printf("%s", r.name.c_str());
      if (r.k != dfx_trace::HOST && r.k != dfx_trace::NOTE) printf(" stream %d", thread(r.stream));
      if (r.k == dfx_trace::WAIT) printf(" waits for stream %d", thread(r.other));
      for (const dfx_trace::range &g : r.ranges) printf(" %s:%s[%zu+%zu]", g.write ? "W" : "R", range_name(g).c_str(), g.off, g.len);
      printf("\n");
    }
    if (r.k != dfx_trace::HOST && r.k != dfx_trace::ACCESS) continue;
    const unsigned now = tick(th);
    for (const dfx_trace::range &g : r.ranges) {
      std::vector<access> &prev = by_buffer[g.buf];
      for (const access &p : prev) {
        if (p.rec == n || (!p.r.write && !g.write)) continue;
        if (p.r.off + p.r.len <= g.off || g.off + g.len <= p.r.off) continue;
        // p was issued first: ordered iff this access has seen p's tick of p's thread
        const unsigned seen = (size_t)p.thread < clocks[th].size() ? clocks[th][p.thread] : 0;
        if (seen >= p.tick) continue;
        ++races;
        printf("RACE on %s: %s (%s, %s, record %zu) and %s (%s, %s, record %zu) are unordered\n", range_name(g).c_str(),
               t[p.rec].name.c_str(), p.thread ? ("stream " + std::to_string(p.thread)).c_str() : "host",
               p.r.write ? "write" : "read", p.rec, r.name.c_str(), th ? ("stream " + std::to_string(th)).c_str() : "host",
               g.write ? "write" : "read", n);
      }
      prev.push_back({n, th, now, g});
    }
  }
  for (const std::string &e : dfx_trace::stub_errors()) printf("STUB ERROR: %s\n", e.c_str());
  printf("records %zu launches %d copies %d syncs %d waits %d races %d stub_errors %zu\n", t.size(), launches, copies, syncs, waits,
         races, dfx_trace::stub_errors().size());
  return races || !dfx_trace::stub_errors().empty();
}

// can the checker see a race at all?  The same four accesses with and without the edges between them.
void selftest(bool ordered) {
  void *h1 = nullptr, *h2 = nullptr, *d = nullptr;
  dfx_stream_t a = nullptr, b = nullptr;
  dfx_mem_alloc_host(&h1, 64);
  dfx_mem_alloc_host(&h2, 64);
  dfx_mem_alloc_device(&d, 64);
  dfx_stream_create(&a);
  dfx_stream_create(&b);
  dfx_memcpy_h2d(d, h1, 64, a);                  // a writes d
  if (ordered) dfx_stream_wait_stream(b, a);
  dfx_memcpy_d2h(h2, d, 64, b);                  // b reads d: read after write
  if (ordered) dfx_stream_wait_stream(a, b);
  dfx_memcpy_h2d(static_cast<char *>(d) + 32, h1, 32, a);  // a rewrites half of d: write after read
  if (ordered) dfx_stream_sync(a);
  dfx_trace::host_access("host rewrites h1", h1, 8, true);  // the uploads read h1
  if (ordered) dfx_stream_sync(b);
  dfx_stream_destroy(b);
  if (!ordered) dfx_stream_wait_stream(a, b);    // a stream that is gone
  dfx_stream_destroy(a);
  dfx_mem_free_device(d);
  dfx_mem_free_host(h2);
  dfx_mem_free_host(h1);
}

}  // namespace

int main(int argc, char **argv) {
  if (argc > 1 && !strncmp(argv[1], "selftest-", 9)) {
    const bool ordered = !strcmp(argv[1], "selftest-ordered");
    selftest(ordered);
    const int bad = check(true);
    printf("selftest (%s): %s\n", ordered ? "ordered" : "unordered", bad ? "FAILED" : "race-free");
    return bad ? 1 : 0;
  }
  if (argc < 2 || strlen(argv[1]) != 1 || argv[1][0] < 'a' || argv[1][0] > 'h') {
    fprintf(stderr, "usage: coherence_check a|b|c|d|e|f|g|h [--dump] | selftest-ordered | selftest-race\n");
    return 2;
  }
  const char sc = argv[1][0];
  const bool dump = argc > 2 && !strcmp(argv[2], "--dump");
  if (sc == 'f' || sc == 'h') {
    const char *dv = getenv("DEEPFUSION_DEVICES");
    if (!dv || atoi(dv) < 2) {
      fprintf(stderr, "scenario %c wants DEEPFUSION_DEVICES=2\n", sc);
      return 2;
    }
  }
  if (sc == 'g' || sc == 'h') {
    token_net n;
    n.name_all(sc == 'g');
    if (sc == 'g') scenario_g(n);
    else scenario_h(n);
  } else {
    marking_source src;
    net n(sc == 'c' ? 4 : sc == 'e' ? 2 : 1, src);
    name_all(n, sc != 'f');
    switch (sc) {
      case 'a': scenario_a(n); break;
      case 'b': scenario_b(n); break;
      case 'c': scenario_c(n); break;
      case 'd': scenario_d(n); break;
      case 'e': scenario_e(n); break;
      default: scenario_f(n); break;
    }
  }  // (the net's destructors run inside the trace: ops first, then tensors)
  const int bad = check(dump);
  printf("scenario %c: %s\n", sc, bad ? "FAILED" : "race-free");
  return bad ? 1 : 0;
}
