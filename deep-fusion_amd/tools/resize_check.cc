// resize_check -- device self-check of the activation resize (dfx_resize_*): every geometry x mode x dtype of a small
// table on both kernel paths, with and without the fused add, against a scalar host loop that reads the tables of
// csrc/resize_plan.h and evaluates the formula of include/dfx.h one element at a time.  Exit status 0 when every byte agrees.
//   resize_check -dump <dir>   instead runs deepfusion::resize / resize_add (the C++ layer, DEEPFUSION_DEVICES honoured) on
//                              four seeded cases and writes <case>_src.bin, <case>_add.bin and <case>_dst.bin there, for
//                              tests/test_gpu_resize.py to compare with its reference
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../csrc/resize_plan.h"
#include "cli_flags.h"
#include "deepfusion.h"
#include "dfx.h"

static size_t esize(int dt) { return dt == DFX_F32 || dt == DFX_S32 ? 4 : 1; }

static float load(const std::vector<unsigned char> &b, int dt, size_t i) {
  if (dt == DFX_F32) { float v; memcpy(&v, &b[i * 4], 4); return v; }
  return dt == DFX_S8 ? (float)(int8_t)b[i] : (float)b[i];
}

// volatile: every product and sum is rounded to f32 on its own, whatever the host compiler would like to contract
static float lerp(float a, float b, float w0, float w1) {
  volatile float p = a * w0, q = b * w1;
  volatile float r = p + q;
  return r;
}

static void host_resize(const dfx_resize_desc &d, const std::vector<unsigned char> &src, const std::vector<unsigned char> *add,
                        std::vector<unsigned char> &dst) {
  dfx::ResizeAxis ty, tx;
  dfx::resize_axis_plan(d.ih, d.oh, d.algo, d.coord, ty);
  dfx::resize_axis_plan(d.iw, d.ow, d.algo, d.coord, tx);
  const size_t es = esize(d.dt);
  for (int n = 0; n < d.bs; ++n)
    for (int oy = 0; oy < d.oh; ++oy)
      for (int ox = 0; ox < d.ow; ++ox)
        for (int k = 0; k < d.c; ++k) {
          const size_t o = (((size_t)n * d.oh + oy) * d.ow + ox) * d.c + k;
          auto at = [&](int y, int x) { return (((size_t)n * d.ih + y) * d.iw + x) * d.c + k; };
          if (d.algo == DFX_RESIZE_NEAREST) {
            memcpy(&dst[o * es], &src[at(ty.i0[oy], tx.i0[ox]) * es], es);
          } else {
            const float top = lerp(load(src, d.dt, at(ty.i0[oy], tx.i0[ox])), load(src, d.dt, at(ty.i0[oy], tx.i1[ox])), tx.w0[ox], tx.w1[ox]);
            const float bot = lerp(load(src, d.dt, at(ty.i1[oy], tx.i0[ox])), load(src, d.dt, at(ty.i1[oy], tx.i1[ox])), tx.w0[ox], tx.w1[ox]);
            const float v = lerp(top, bot, ty.w0[oy], ty.w1[oy]);
            if (d.dt == DFX_F32) memcpy(&dst[o * 4], &v, 4);
            else {
              long q = lrintf(v);  // (round to nearest even: the default rounding mode)
              const long lo = d.dt == DFX_S8 ? -128 : 0, hi = d.dt == DFX_S8 ? 127 : 255;
              q = q < lo ? lo : q > hi ? hi : q;
              dst[o] = (unsigned char)q;
            }
          }
          if (!add) continue;
          if (d.dt == DFX_F32) {
            float r, a;
            memcpy(&r, &dst[o * 4], 4); memcpy(&a, &(*add)[o * 4], 4);
            volatile float s = r + a;
            float f = s;
            if (d.post_relu && 0.0f > f) f = 0.0f;
            memcpy(&dst[o * 4], &f, 4);
          } else if (d.dt == DFX_S32) {
            int32_t r, a;
            memcpy(&r, &dst[o * 4], 4); memcpy(&a, &(*add)[o * 4], 4);
            long long s = (long long)r + a;
            if (d.post_relu && s < 0) s = 0;
            s = s < -2147483648LL ? -2147483648LL : s > 2147483647LL ? 2147483647LL : s;
            r = (int32_t)s;
            memcpy(&dst[o * 4], &r, 4);
          } else if (d.dt == DFX_S8) {
            int s = (int)(int8_t)dst[o] + (int)(int8_t)(*add)[o];
            const int lo = d.post_relu ? 0 : -128;
            dst[o] = (unsigned char)(int8_t)(s < lo ? lo : s > 127 ? 127 : s);
          } else {
            const int s = (int)dst[o] + (int)(*add)[o];
            dst[o] = (unsigned char)(s > 255 ? 255 : s);
          }
        }
}

static void write_file(const std::string &dir, const char *name, const void *p, size_t n) {
  FILE *fp = fopen((dir + "/" + name).c_str(), "wb");
  if (!fp || fwrite(p, 1, n, fp) != n) { fprintf(stderr, "cannot write %s/%s\n", dir.c_str(), name); exit(1); }
  fclose(fp);
}

static void fill_bytes(deepfusion::memory &m, Lcg &g) {
  unsigned char *p = (unsigned char *)m.data();
  if (m.data_type() == deepfusion::memory::dtype::f32) {
    for (size_t i = 0; i < m.size(); ++i) ((float *)p)[i] = ((int)(g.next() % 2001) - 1000) * 0.037f;
  } else {
    for (size_t i = 0; i < m.buffer_size(); ++i) p[i] = (unsigned char)(g.next() & 0xff);
  }
}

// the C++ layer: a: u8 bilinear half_pixel; b: f32 bilinear align_corners; c: s8 nearest + lateral + relu (submit_async /
// wait / download); d: u8 nearest x2 + lateral IN PLACE (the lateral is dst)
static int dump_cpp_layer(const std::string &dir) {
  using namespace deepfusion;
  typedef memory::nchw_dims dims;
  const memory::format nhwc = memory::format::nhwc;
  Lcg g(4321);
  {
    std::unique_ptr<memory> src(new memory(dims{3, 16, 5, 7}, nhwc, memory::dtype::u8)), dst(new memory(dims{3, 16, 10, 14}, nhwc, memory::dtype::u8));
    fill_bytes(*src, g);
    write_file(dir, "a_src.bin", src->host_data(), src->buffer_size());
    resize(src, dst, resize_algo::bilinear, resize_coord::half_pixel)->submit();
    write_file(dir, "a_dst.bin", dst->host_data(), dst->buffer_size());
  }
  {
    std::unique_ptr<memory> src(new memory(dims{3, 3, 9, 6}, nhwc, memory::dtype::f32)), dst(new memory(dims{3, 3, 4, 11}, nhwc, memory::dtype::f32));
    fill_bytes(*src, g);
    write_file(dir, "b_src.bin", src->host_data(), src->buffer_size());
    resize(src, dst, resize_algo::bilinear, resize_coord::align_corners)->submit();
    write_file(dir, "b_dst.bin", dst->host_data(), dst->buffer_size());
  }
  {
    std::unique_ptr<memory> src(new memory(dims{4, 5, 5, 7}, nhwc, memory::dtype::s8)), lat(new memory(dims{4, 5, 20, 28}, nhwc, memory::dtype::s8)),
        dst(new memory(dims{4, 5, 20, 28}, nhwc, memory::dtype::s8));
    fill_bytes(*src, g);
    fill_bytes(*lat, g);
    write_file(dir, "c_src.bin", src->host_data(), src->buffer_size());
    write_file(dir, "c_add.bin", lat->host_data(), lat->buffer_size());
    auto op = resize_add(src, lat, dst, resize_algo::nearest, resize_coord::asymmetric, true);
    op->submit_async();
    op->wait();
    dst->download();
    write_file(dir, "c_dst.bin", dst->host_data(), dst->buffer_size());
  }
  {
    std::unique_ptr<memory> src(new memory(dims{3, 32, 8, 8}, nhwc, memory::dtype::u8)), dst(new memory(dims{3, 32, 16, 16}, nhwc, memory::dtype::u8));
    fill_bytes(*src, g);
    fill_bytes(*dst, g);
    write_file(dir, "d_src.bin", src->host_data(), src->buffer_size());
    write_file(dir, "d_add.bin", dst->host_data(), dst->buffer_size());
    resize_add(src, dst, dst, resize_algo::nearest, resize_coord::asymmetric, false)->submit();
    write_file(dir, "d_dst.bin", dst->host_data(), dst->buffer_size());
  }
  printf("resize_check: wrote the C++ layer's four cases to %s\n", dir.c_str());
  return 0;
}

int main(int argc, char **argv) {
  Flags f(argc, argv);
  const std::string dump = f.gets("dump", "");
  if (!dump.empty()) return dump_cpp_layer(dump);
  const bool verbose = f.getb("verbose", false);
  static const int geoms[][4] = {{1, 1, 3, 5}, {5, 7, 20, 28}, {7, 5, 10, 9}, {9, 6, 4, 11}, {2, 2, 33, 33}, {17, 3, 3, 17}};
  static const int dts[] = {DFX_U8, DFX_S8, DFX_F32, DFX_S32};
  int runs = 0, bad = 0, band_runs = 0;
  Lcg g(99);
  for (const auto &gm : geoms)
    for (int dt : dts)
      for (int algo = 0; algo < 2; ++algo)
        for (int coord = 0; coord < 3; ++coord)
          for (int ci = 0; ci < 2; ++ci)
            for (int add = 0; add < 2; ++add)
              for (int path = 0; path < 2; ++path) {
                if (dt == DFX_S32 && algo == DFX_RESIZE_BILINEAR) continue;
                const size_t es = esize(dt);
                const int c = ci == 0 ? (int)(32 / es) : 5;  // 32 bytes of channels (the band kernel's class) or 5 channels
                if (path == DFX_RESIZE_BAND && ci == 1) continue;
                dfx_resize_desc d = {2, c, gm[0], gm[1], gm[2], gm[3], dt, algo, coord, add, add && coord == 1, path};
                std::vector<unsigned char> src((size_t)d.bs * d.ih * d.iw * c * es), lat((size_t)d.bs * d.oh * d.ow * c * es), want(lat.size()), got(lat.size());
                auto fill = [&](std::vector<unsigned char> &b) {
                  for (size_t i = 0; i < b.size() / es; ++i) {
                    if (dt == DFX_F32) { const float v = ((int)(g.next() % 2001) - 1000) * 0.037f; memcpy(&b[i * 4], &v, 4); }
                    else if (dt == DFX_S32) { const int32_t v = (int32_t)(g.next() * 131071u) - (int32_t)(g.next() * 65537u); memcpy(&b[i * 4], &v, 4); }
                    else b[i] = (unsigned char)(g.next() & 0xff);
                  }
                };
                fill(src); fill(lat);
                host_resize(d, src, add ? &lat : nullptr, want);
                dfx_resize_t *h = nullptr;
                if (dfx_resize_create(&d, &h) != DFX_OK) { fprintf(stderr, "create: %s\n", dfx_last_error()); return 1; }
                dfx_resize_info info;
                dfx_resize_query(h, &info);
                if (dfx_resize_submit_host(h, src.data(), add ? lat.data() : nullptr, got.data()) != DFX_OK) { fprintf(stderr, "submit_host: %s\n", dfx_last_error()); return 1; }
                dfx_resize_destroy(h);
                ++runs;
                band_runs += info.path == DFX_RESIZE_BAND;
                const bool ok = info.path == path && !memcmp(want.data(), got.data(), want.size());
                if (!ok) ++bad;
                if (!ok || verbose)
                  printf("%s %dx%d -> %dx%d c %d dt %d algo %d coord %d add %d: %s\n", ok ? "ok  " : "FAIL", gm[0], gm[1], gm[2], gm[3], c, dt, algo,
                         coord, add, info.kernel_name);
              }
  printf("resize_check: %d runs (%d on the band kernel), %d mismatches\n", runs, band_runs, bad);
  return bad ? 1 : 0;
}
