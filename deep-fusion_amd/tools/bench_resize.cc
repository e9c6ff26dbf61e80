// bench_resize -- times the two kernels of the activation resize (dfx_resize_*) on MI355X through the C ABI: the generic
// kernel and the band kernel (force_path), alternating, on the feature-map resizes of FPN, DeepLab v3+, PSPNet and a
// bilinear U-Net at N = 1 and 16.  Device-resident, back-to-back launches between two events, the median of -rounds rounds
// per kernel; GB/s of algorithmic_bytes (src + dst + add) and the share of the 8 TB/s HBM peak.  The launches rotate over
// enough (src, add, dst) sets to exceed -rotate_mb (default 768: three times the 256 MiB Infinity Cache, so that it serves
// neither kernel); -rotate_mb 0 times one set over and over (warm caches).  The two kernels' results are compared byte
// for byte at every point.
//   bench_resize [-iter 200] [-burning_iter 20] [-rounds 3] [-rotate_mb 768] [-only <substring of a point's name>]
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "cli_flags.h"
#include "dfx.h"

struct Point {
  const char *name;
  int c, ih, iw, oh, ow, dt, algo, coord, add;
};

static void check(int rc, const char *what) {
  if (rc != DFX_OK) { fprintf(stderr, "%s failed (%d): %s\n", what, rc, dfx_last_error()); exit(1); }
}

int main(int argc, char **argv) {
  Flags f(argc, argv);
  const int burn = f.geti("burning_iter", 20), iters = f.geti("iter", 200), rounds = f.geti("rounds", 3);
  const std::string only = f.gets("only", "");
  const size_t rotate = (size_t)f.geti("rotate_mb", 768) << 20;
  const Point points[] = {
      {"fpn nearest x2 + add 16->32 c256 u8", 256, 16, 16, 32, 32, DFX_U8, DFX_RESIZE_NEAREST, DFX_COORD_ASYMMETRIC, 1},
      {"fpn nearest x2 + add 32->64 c256 u8", 256, 32, 32, 64, 64, DFX_U8, DFX_RESIZE_NEAREST, DFX_COORD_ASYMMETRIC, 1},
      {"fpn nearest x2 + add 64->128 c256 u8", 256, 64, 64, 128, 128, DFX_U8, DFX_RESIZE_NEAREST, DFX_COORD_ASYMMETRIC, 1},
      {"deeplab aspp bilinear ac 33->129 c256 u8", 256, 33, 33, 129, 129, DFX_U8, DFX_RESIZE_BILINEAR, DFX_COORD_ALIGN_CORNERS, 0},
      {"deeplab logits bilinear ac 129->513 c21 u8 (outside the class)", 21, 129, 129, 513, 513, DFX_U8, DFX_RESIZE_BILINEAR, DFX_COORD_ALIGN_CORNERS, 0},
      {"deeplab logits bilinear ac 129->513 c32 u8 (c padded)", 32, 129, 129, 513, 513, DFX_U8, DFX_RESIZE_BILINEAR, DFX_COORD_ALIGN_CORNERS, 0},
      {"pspnet bilinear ac 6->60 c512 u8", 512, 6, 6, 60, 60, DFX_U8, DFX_RESIZE_BILINEAR, DFX_COORD_ALIGN_CORNERS, 0},
      {"unet bilinear hp x2 128->256 c64 u8", 64, 128, 128, 256, 256, DFX_U8, DFX_RESIZE_BILINEAR, DFX_COORD_HALF_PIXEL, 0},
      {"unet bilinear hp x2 128->256 c64 f32", 64, 128, 128, 256, 256, DFX_F32, DFX_RESIZE_BILINEAR, DFX_COORD_HALF_PIXEL, 0},
  };
  const char *rows_env = getenv("DFX_RESIZE_ROWS");
  printf("bench_resize: %d timed launches per round after %d warm-up launches, median of %d rounds, kernels alternating; buffers in rotation: %zu MiB%s; DFX_RESIZE_ROWS %s\n",
         iters, burn, rounds, rotate >> 20, rotate ? "" : " (one set: warm caches)", rows_env ? rows_env : "unset (auto)");
  printf("%-66s %3s %-8s %10s %10s %7s  %s\n", "point", "N", "kernel", "us", "GB/s", "of peak", "kernel name");
  dfx_event_t e0, e1;
  check(dfx_event_create(&e0), "event create");
  check(dfx_event_create(&e1), "event create");
  int slower = 0, inclass = 0;
  for (const Point &p : points) {
    if (!only.empty() && !strstr(p.name, only.c_str())) continue;
    for (int bs : {1, 16}) {
      const size_t es = p.dt == DFX_F32 ? 4 : 1;
      const size_t sb = (size_t)bs * p.ih * p.iw * p.c * es, db = (size_t)bs * p.oh * p.ow * p.c * es;
      std::vector<unsigned char> hs(sb), ha(db), out[2];
      Lcg g(7);
      for (size_t i = 0; i < sb / es; ++i) {
        if (p.dt == DFX_F32) { const float v = ((int)(g.next() % 2001) - 1000) * 0.01f; memcpy(&hs[i * 4], &v, 4); }
        else hs[i] = (unsigned char)(g.next() & 0xff);
      }
      for (size_t i = 0; i < db; ++i) ha[i] = (unsigned char)(g.next() & 0x7f);
      // nsets copies of (src, add, dst), each 256-byte aligned inside three allocations
      const size_t sstep = (sb + 255) / 256 * 256, dstep = (db + 255) / 256 * 256;
      const size_t nsets = std::max<size_t>(1, std::min<size_t>(4096, (rotate + sstep + 2 * dstep - 1) / (sstep + 2 * dstep)));
      void *ds = nullptr, *da = nullptr, *dd = nullptr;
      check(dfx_mem_alloc_device(&ds, sstep * nsets), "device alloc");
      check(dfx_mem_alloc_device(&da, dstep * nsets), "device alloc");
      check(dfx_mem_alloc_device(&dd, dstep * nsets), "device alloc");
      for (size_t k = 0; k < nsets; ++k) {
        check(dfx_memcpy_h2d((char *)ds + k * sstep, hs.data(), sb, nullptr), "H2D");
        check(dfx_memcpy_h2d((char *)da + k * dstep, ha.data(), db, nullptr), "H2D");
      }
      check(dfx_stream_sync(nullptr), "sync");
      size_t turn = 0;
      auto launch = [&](dfx_resize_t *hh) {
        const size_t k = turn++ % nsets;
        check(dfx_resize_submit(hh, (char *)ds + k * sstep, p.add ? (char *)da + k * dstep : nullptr, (char *)dd + k * dstep, nullptr), "submit");
      };
      dfx_resize_t *h[2] = {nullptr, nullptr};
      dfx_resize_info info[2];
      std::vector<double> us[2];
      int npaths = 0;
      for (int path = DFX_RESIZE_GENERIC; path >= DFX_RESIZE_BAND; --path) {  // h[0]: generic, h[1]: band
        dfx_resize_desc d = {bs, p.c, p.ih, p.iw, p.oh, p.ow, p.dt, p.algo, p.coord, p.add, 0, path};
        const int rc = dfx_resize_create(&d, &h[npaths]);
        if (rc == DFX_ERR_UNSUPPORTED) break;  // outside the band kernel's class
        check(rc, "resize create");
        check(dfx_resize_query(h[npaths], &info[npaths]), "query");
        ++npaths;
      }
      for (int r = 0; r < rounds; ++r)
        for (int k = 0; k < npaths; ++k) {
          for (int i = 0; i < burn; ++i) launch(h[k]);
          check(dfx_event_record(e0, nullptr), "record");
          for (int i = 0; i < iters; ++i) launch(h[k]);
          check(dfx_event_record(e1, nullptr), "record");
          float ms = 0;
          check(dfx_event_elapsed_ms(e0, e1, &ms), "elapsed");
          us[k].push_back(ms * 1000.0 / iters);
          if (r == 0) {
            out[k].resize(db);
            check(dfx_memcpy_d2h(out[k].data(), (char *)dd + ((turn - 1) % nsets) * dstep, db, nullptr), "D2H");
            check(dfx_stream_sync(nullptr), "sync");
          }
        }
      double med[2] = {0, 0};
      for (int k = 0; k < npaths; ++k) {
        std::sort(us[k].begin(), us[k].end());
        med[k] = us[k][us[k].size() / 2];
        const double gbs = (double)info[k].algorithmic_bytes / med[k] / 1e3;
        printf("%-66s %3d %-8s %10.2f %10.1f %6.1f%%  %s\n", p.name, bs, k == 0 ? "generic" : "band", med[k], gbs, gbs / 8000.0 * 100.0,
               info[k].kernel_name);
      }
      if (npaths == 2) {
        ++inclass;
        const bool same = out[0] == out[1];
        if (med[1] > med[0]) ++slower;
        printf("%-66s %3d band / generic time %.3f, results %s\n", "", bs, med[1] / med[0], same ? "identical" : "DIFFER");
        if (!same) { fprintf(stderr, "the two kernels disagree on %s\n", p.name); return 1; }
      }
      for (int k = 0; k < npaths; ++k) dfx_resize_destroy(h[k]);
      dfx_mem_free_device(ds); dfx_mem_free_device(da); dfx_mem_free_device(dd);
    }
  }
  printf("band kernel slower than the generic kernel on %d of %d in-class points\n", slower, inclass);
  dfx_event_destroy(e0);
  dfx_event_destroy(e1);
  return 0;
}
