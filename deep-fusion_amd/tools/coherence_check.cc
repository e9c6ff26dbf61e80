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
//   coherence_check <scenario> [--dump]     scenario: a | b | c | d | e | f  (f wants DEEPFUSION_DEVICES=2 DFX_TRACE_DEVICES=2)
//   --dump prints the trace, one line per record, in a form that two builds can be diffed by
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

void fill(memory *m, const std::string &name) {
  void *p = m->data();
  memset(p, 2, m->buffer_size());
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
    }
    if (dump) {
      printf("%s", r.name.c_str());
      if (r.k != dfx_trace::HOST) printf(" stream %d", thread(r.stream));
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
  if (argc < 2 || strlen(argv[1]) != 1 || argv[1][0] < 'a' || argv[1][0] > 'f') {
    fprintf(stderr, "usage: coherence_check a|b|c|d|e|f [--dump] | selftest-ordered | selftest-race\n");
    return 2;
  }
  const char sc = argv[1][0];
  const bool dump = argc > 2 && !strcmp(argv[2], "--dump");
  if (sc == 'f') {
    const char *dv = getenv("DEEPFUSION_DEVICES");
    if (!dv || atoi(dv) < 2) {
      fprintf(stderr, "scenario f wants DEEPFUSION_DEVICES=2\n");
      return 2;
    }
  }
  {
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
