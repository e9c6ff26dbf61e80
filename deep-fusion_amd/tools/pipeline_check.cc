// pipeline_check -- the network of pipeline_net.h (every op class of include/deepfusion.h once, chained, the tensors
// staying on the device) on the real libraries.  Inputs, weights, biases and scales are raw files written by
// tests/pipeline_ref.py; the tensors are dumped as raw files, which tests/test_gpu_pipeline.py compares bit for bit with
// the chained numpy / oracle references.
//   pipeline_check <mode> <indir> <outdir>
//     sync      submit() per op; every tensor is dumped (e0 = e after the deconvolution, before the in-place resize_add)
//     async     one frame of submit_async(), ONE wait() on the last op; k is downloaded and dumped, then every intermediate
//     frames    four frames in flight: F first ops write q, F last ops read j, no wait() until all are submitted; k_0 .. k_3
//     stepwise  submit_async() and wait() per op, the contract of batch shards (DEEPFUSION_DEVICES > 1); dumps like sync
#include <cstdio>
#include <cstring>
#include <string>

#include "pipeline_net.h"

using pipeline::memory;

static std::string g_in, g_out;

static std::vector<char> slurp(const std::string &name) {
  const std::string path = g_in + "/" + name + ".bin";
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) { fprintf(stderr, "cannot read %s\n", path.c_str()); exit(2); }
  std::vector<char> v;
  char buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return v;
}
static void dump(const std::string &name, memory *m) {
  const std::string path = g_out + "/" + name + ".bin";
  FILE *f = fopen(path.c_str(), "wb");
  if (!f || fwrite(m->host_data(), 1, m->buffer_size(), f) != m->buffer_size()) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(2); }
  fclose(f);
}

struct file_source : pipeline::source {
  void fill(const std::string &name, void *p, size_t bytes) override {
    const std::vector<char> v = slurp(name);
    if (v.size() != bytes) { fprintf(stderr, "%s.bin holds %zu bytes, the tensor %zu\n", name.c_str(), v.size(), bytes); exit(2); }
    memcpy(p, v.data(), bytes);
  }
  std::vector<float> scales(const std::string &name) override {
    const std::vector<char> v = slurp(name);
    if (v.empty() || v.size() % sizeof(float)) { fprintf(stderr, "%s.bin is no f32 vector\n", name.c_str()); exit(2); }
    std::vector<float> s(v.size() / sizeof(float));
    memcpy(s.data(), v.data(), v.size());
    return s;
  }
};

// the name a mid op's result is dumped under
static std::string dst_name(pipeline::net &n, size_t m) {
  if (n.mid_names[m] == "deconvolution") return "e0";
  for (auto &t : n.intermediates())
    if (t.second == n.mid_dst[m]) return t.first;
  return "?";
}

int main(int argc, char **argv) {
  if (argc != 4) { fprintf(stderr, "usage: pipeline_check sync|async|frames|stepwise <indir> <outdir>\n"); return 2; }
  const std::string mode = argv[1];
  g_in = argv[2];
  g_out = argv[3];
  if (mode != "sync" && mode != "async" && mode != "frames" && mode != "stepwise") { fprintf(stderr, "unknown mode %s\n", mode.c_str()); return 2; }
  file_source src;
  pipeline::net n(mode == "frames" ? 4 : 1, src);
  for (int f = 0; f < n.F; ++f) src.fill("x_" + std::to_string(f), n.x[f]->data(), n.x[f]->buffer_size());
  if (mode == "sync" || mode == "stepwise") {
    const bool step = mode == "stepwise";
    auto run = [&](deepfusion::op &o, memory *dst, const std::string &name) {
      if (step) {
        o.submit_async();
        o.wait();
        dst->download();  // (a no-op for a tensor that batch shards wrote on the host)
      } else {
        o.submit();
      }
      dump(name, dst);
    };
    run(*n.first[0], n.q.get(), "q");
    for (size_t m = 0; m < n.mid.size(); ++m) run(*n.mid[m], n.mid_dst[m], dst_name(n, m));
    run(*n.last[0], n.k[0].get(), "k");
  } else if (mode == "async") {
    n.first[0]->submit_async();
    for (auto &o : n.mid) o->submit_async();
    n.last[0]->submit_async();
    n.last[0]->wait();
    n.k[0]->download();
    dump("k", n.k[0].get());
    for (auto &t : n.intermediates()) {
      t.second->download();
      dump(t.first, t.second);
    }
  } else {
    for (int f = 0; f < n.F; ++f) {
      n.first[f]->submit_async();
      for (auto &o : n.mid) o->submit_async();
      n.last[f]->submit_async();
    }
    for (int f = 0; f < n.F; ++f) {
      n.last[f]->wait();
      n.k[f]->download();
      dump("k_" + std::to_string(f), n.k[f].get());
    }
  }
  printf("pipeline_check %s wrote results to %s\n", mode.c_str(), g_out.c_str());
  return 0;
}
