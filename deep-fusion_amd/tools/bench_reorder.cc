// bench_reorder -- times deepfusion::reorder on MI355X through the drop-in C++ API.  Flags and timing
// protocol in the style of bench_conv / bench_concat (burning_iter warm-up submits, iter timed submits, mean ms;
// -cold_cache adds the per-launch warm / cold legs).
//   bench_reorder -bs 128 -c 64 -h 56 -w 56 -src_dtype f32 -dst_dtype u8 -src_format nchw -dst_format nhwc -per_channel
//   bench_reorder -bs 128 -c 3 -dst_c 16 -h 224 -w 224 -cold_cache
#include <chrono>
#include <cmath>
#include <cstdio>

#include "cli_flags.h"
#include "deepfusion.h"
#include "dfx.h"

using namespace deepfusion;

static memory::dtype parse_dt(const std::string &s) {
  if (s == "f32") return memory::dtype::f32;
  if (s == "s32") return memory::dtype::s32;
  if (s == "s8") return memory::dtype::s8;
  if (s == "u8") return memory::dtype::u8;
  fprintf(stderr, "Unknow data type %s\n", s.c_str());
  exit(1);
}
static memory::format parse_fmt(const std::string &s) {
  if (s == "nchw") return memory::format::nchw;
  if (s == "nhwc") return memory::format::nhwc;
  fprintf(stderr, "Unknow format %s\n", s.c_str());
  exit(1);
}

// (see bench_concat.cc: 512 MiB of device scratch rewritten before every timed launch, next to the same
// per-launch protocol without the flush)
template <typename Op>
static void cold_cache_leg(Op &op, int iters, const char *what) {
  const size_t scratch_bytes = 512u << 20;
  void *scratch = nullptr;
  if (dfx_mem_alloc_device(&scratch, scratch_bytes) != DFX_OK) { fprintf(stderr, "cold_cache: %s\n", dfx_last_error()); exit(1); }
  auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  double sum[2] = {0, 0};
  for (int cold = 0; cold < 2; ++cold)
    for (int i = 0; i < iters; ++i) {
      if (cold) {
        dfx_memset_device(scratch, i & 0xff, scratch_bytes, nullptr);
        dfx_stream_sync(nullptr);
      }
      const double t0 = now();
      op->submit_async();
      op->wait();
      sum[cold] += now() - t0;
    }
  dfx_mem_free_device(scratch);
  printf("DeepFusion %s avg time (device resident, one launch at a time, warm caches): %f ms\n", what, sum[0] / iters);
  printf("DeepFusion %s avg time (device resident, one launch at a time, COLD caches: 512 MiB scratch rewritten before each): %f ms\n", what, sum[1] / iters);
}

int main(int argc, char **argv) {
  Flags f(argc, argv);
  const int burn = f.geti("burning_iter", 50), iters = f.geti("iter", 100);
  const int bs = f.geti("bs", 128), c = f.geti("c", 64), h = f.geti("h", 56), w = f.geti("w", 56);
  const int dst_c = f.geti("dst_c", c);
  const std::string sdt = f.gets("src_dtype", "f32"), ddt = f.gets("dst_dtype", "u8");
  const std::string sfm = f.gets("src_format", "nchw"), dfm = f.gets("dst_format", "nhwc");
  const bool per_channel = f.getb("per_channel", true);
  const memory::dtype sd = parse_dt(sdt), dd = parse_dt(ddt);
  std::unique_ptr<memory> src(new memory(memory::nchw_dims{bs, c, h, w}, parse_fmt(sfm), sd));
  std::unique_ptr<memory> dst(new memory(memory::nchw_dims{bs, dst_c, h, w}, parse_fmt(dfm), dd));
  Lcg g(1234);
  void *p = src->data();
  for (size_t i = 0; i < src->size(); ++i) {
    const int v = (int)(g.next() % 601) - 200;
    if (sd == memory::dtype::f32) ((float *)p)[i] = (float)v * 0.5f;
    else if (sd == memory::dtype::s32) ((int32_t *)p)[i] = v * 37;
    else if (sd == memory::dtype::s8) ((int8_t *)p)[i] = (int8_t)(v % 128);
    else ((uint8_t *)p)[i] = (uint8_t)(v & 0xff);
  }
  std::vector<float> sc(per_channel ? c : 1);
  for (size_t k = 0; k < sc.size(); ++k) sc[k] = 0.5f + 0.01f * (float)k;
  auto op = reorder(src, dst, sc, f.getb("round_down", false) ? round_mode::down : round_mode::nearest);
  auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  for (int i = 0; i < burn; ++i) op->submit();
  double t0 = now();
  for (int i = 0; i < iters; ++i) op->submit();
  const double host_ms = (now() - t0) / iters;
  for (int i = 0; i < burn; ++i) op->submit_async();
  op->wait();
  t0 = now();
  for (int i = 0; i < iters; ++i) op->submit_async();
  op->wait();
  const double dev_ms = (now() - t0) / iters;
  const int cl = c < dst_c ? c : dst_c;
  const double bytes = (double)bs * h * w * ((double)cl * (src->buffer_size() / src->size()) + (double)dst_c * (dst->buffer_size() / dst->size()));
  printf("Reorder {%d,%d,%d,%d} %s %s -> {%d,%d,%d,%d} %s %s, %d scale(s)\n", bs, c, h, w, sdt.c_str(), sfm.c_str(), bs, dst_c, h, w,
         ddt.c_str(), dfm.c_str(), (int)sc.size());
  printf("DeepFusion Reorder avg time (submit: H2D + kernel + D2H): %f ms\n", host_ms);
  printf("DeepFusion Reorder avg time (device resident):            %f ms  (%.1f GB/s)\n", dev_ms, bytes / dev_ms / 1e6);
  if (f.getb("cold_cache", false)) cold_cache_leg(op, iters, "Reorder");
  return 0;
}
