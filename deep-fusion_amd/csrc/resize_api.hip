// resize_api.hip -- host side of the activation resize (dfx_resize_* of include/dfx.h): descriptor validation, the
// per-axis tables (resize_plan.h) and their upload, choice of the kernel path, launches.  The kernels are in resize.cuh.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "path_op.h"
#include "resize.cuh"
#include "resize_plan.h"

namespace dfx {
int launch_resize_generic(const ResizeArgs &a, int grid, hipStream_t s);
int launch_resize_band(const ResizeArgs &a, int grid, hipStream_t s);
}
using namespace dfx;

struct dfx_resize {
  dfx_resize_desc d;
  int device = 0;
  int path = DFX_RESIZE_GENERIC;
  ResizeArgs band = {}, generic = {};  // without the buffer pointers; `band` only on the band path
  int band_grid = 0, generic_grid = 0;
  void *d_tables = nullptr;            // y0 y1 x0 x1 (s32), wy0 wy1 wx0 wx1 (f32)
  HostStaging host;                    // dfx_resize_submit_host
  char kernel_name[96] = "";
};

namespace {

void release(dfx_resize *h) {
  if (!h) return;
  DeviceGuard dg(h->device);
  (void)hipFree(h->d_tables);
  h->host.release();
  delete h;
}

constexpr int kMaxBlocks = 256 * 8;  // grid-stride kernels: 8 workgroups per CU
// Band length (measured, profiles/resize/): 8 output rows for bilinear, where a long band rebuilds fewer horizontal
// interpolations; 2 for nearest, which has only a repeated source load to save.  Halved while the launch would have
// fewer than kFillBlocks workgroups.
constexpr int kBilinearRows = 8, kNearestRows = 2;
constexpr int kFillBlocks = 512;
// No tensor of more than 2^40 elements: far beyond any device's memory, and it keeps every size product below (element
// counts times 4 bytes, the sum of three tensors) inside 64 bits.
constexpr long long kMaxElems = 1ll << 40;

// launches since the library was loaded, by the kernel that ran ([DFX_RESIZE_BAND], [DFX_RESIZE_GENERIC]); process-wide,
// because submit does not write to the handle (dfx_debug_resize_launches)
LaunchCounts<2> g_launches;

int validate_resize(const dfx_resize_desc &d) {
  if (d.bs < 1 || d.c < 1) return fail(DFX_ERR_INVALID, "resize: bs and c must be at least 1");
  if (d.ih < 1 || d.iw < 1 || d.oh < 1 || d.ow < 1 || d.ih > RESIZE_MAX_SIZE || d.iw > RESIZE_MAX_SIZE || d.oh > RESIZE_MAX_SIZE ||
      d.ow > RESIZE_MAX_SIZE)
    return fail(DFX_ERR_INVALID, "resize: ih, iw, oh and ow must lie in 1 .. %d", RESIZE_MAX_SIZE);
  if (d.dt < DFX_F32 || d.dt > DFX_U8) return fail(DFX_ERR_INVALID, "resize: bad dtype");
  if (d.algo != DFX_RESIZE_NEAREST && d.algo != DFX_RESIZE_BILINEAR) return fail(DFX_ERR_INVALID, "resize: bad algo");
  if (d.coord != DFX_COORD_HALF_PIXEL && d.coord != DFX_COORD_ALIGN_CORNERS && d.coord != DFX_COORD_ASYMMETRIC)
    return fail(DFX_ERR_INVALID, "resize: bad coord");
  if ((d.add != 0 && d.add != 1) || (d.post_relu != 0 && d.post_relu != 1))
    return fail(DFX_ERR_INVALID, "resize: add and post_relu must be 0 or 1");
  if (d.post_relu && !d.add) return fail(DFX_ERR_INVALID, "resize: post_relu without add");
  if (d.force_path != -1 && d.force_path != DFX_RESIZE_BAND && d.force_path != DFX_RESIZE_GENERIC)
    return fail(DFX_ERR_INVALID, "resize: bad force_path");
  // ih * iw and oh * ow are below 2^32, so each quotient is exact and no product is formed before it is known to fit
  const long long per_c = kMaxElems / std::max((long long)d.ih * d.iw, (long long)d.oh * d.ow);
  if (d.c > per_c || d.bs > per_c / d.c) return fail(DFX_ERR_INVALID, "resize: a tensor of more than 2^40 elements");
  if (d.algo == DFX_RESIZE_BILINEAR && d.dt == DFX_S32) return fail(DFX_ERR_UNSUPPORTED, "resize: bilinear on s32");
  return DFX_OK;
}

bool band_class(const dfx_resize_desc &d) {
  const long long es = (long long)dt_size(d.dt);
  return ((long long)d.c * es) % 16 == 0 && (long long)d.ih * d.iw * d.c * es < (1ll << 31) &&
         (long long)d.oh * d.ow * d.c * es < (1ll << 31);
}

size_t src_bytes(const dfx_resize_desc &d) { return (size_t)d.bs * d.ih * d.iw * d.c * dt_size(d.dt); }
size_t dst_bytes(const dfx_resize_desc &d) { return (size_t)d.bs * d.oh * d.ow * d.c * dt_size(d.dt); }

int grid_for(long long items) {
  long long blocks = std::max(1ll, std::min<long long>((items + 255) / 256, kMaxBlocks));
  if (const char *e = tuning_value("DFX_RESIZE_MAX_GRID")) blocks = std::max(1ll, std::min(blocks, (long long)atoi(e)));  // testing aid
  return (int)blocks;
}

}  // namespace

extern "C" {

int dfx_resize_create(const dfx_resize_desc *desc, dfx_resize_t **out) {
  dfx_resize *h = nullptr;
  ResizeAxis ty, tx;
  const int rc = open_create("resize", desc, out, &h, [&](const dfx_resize_desc &d) {
    if (const int bad = validate_resize(d)) return bad;
    if (d.force_path == DFX_RESIZE_BAND && !band_class(d))
      return fail(DFX_ERR_UNSUPPORTED,
                  "resize_create: shape outside the band kernel's class (c * element size a multiple of 16; one image below 2^31 bytes)");
    if (!resize_axis_plan(d.ih, d.oh, d.algo, d.coord, ty) || !resize_axis_plan(d.iw, d.ow, d.algo, d.coord, tx))
      return fail(DFX_ERR_INVALID, "resize_create: no plan for this descriptor");
    return (int)DFX_OK;
  });
  if (rc) return rc;
  const dfx_resize_desc &d = *desc;
  // AUTO RULE (include/dfx.h): the band kernel everywhere in its class
  h->path = (band_class(d) && d.force_path != DFX_RESIZE_GENERIC) ? DFX_RESIZE_BAND : DFX_RESIZE_GENERIC;

  // one device buffer: the four index tables, then the four weight tables
  const size_t oh = (size_t)d.oh, ow = (size_t)d.ow, words = 4 * (oh + ow);
  std::vector<int32_t> img(words);
  int32_t *p = img.data();
  memcpy(p, ty.i0.data(), oh * 4); memcpy(p + oh, ty.i1.data(), oh * 4);
  memcpy(p + 2 * oh, tx.i0.data(), ow * 4); memcpy(p + 2 * oh + ow, tx.i1.data(), ow * 4);
  int32_t *w = p + 2 * (oh + ow);
  memcpy(w, ty.w0.data(), oh * 4); memcpy(w + oh, ty.w1.data(), oh * 4);
  memcpy(w + 2 * oh, tx.w0.data(), ow * 4); memcpy(w + 2 * oh + ow, tx.w1.data(), ow * 4);
  hipError_t e = hipMalloc(&h->d_tables, words * 4);
  if (e == hipSuccess) e = hipMemcpy(h->d_tables, img.data(), words * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    release(h);
    return fail(DFX_ERR_HIP, "resize_create: table upload: %s", hipGetErrorString(e));
  }
  ResizeArgs a = {};
  const int *ti = (const int *)h->d_tables;
  const float *tw = (const float *)h->d_tables + 2 * (oh + ow);
  a.y0 = ti; a.y1 = ti + oh; a.x0 = ti + 2 * oh; a.x1 = ti + 2 * oh + ow;
  a.wy0 = tw; a.wy1 = tw + oh; a.wx0 = tw + 2 * oh; a.wx1 = tw + 2 * oh + ow;
  a.bs = d.bs; a.c = d.c; a.ih = d.ih; a.iw = d.iw; a.oh = d.oh; a.ow = d.ow;
  a.dt = d.dt; a.algo = d.algo; a.relu = d.post_relu;
  a.rows = 1; a.bands = d.oh; a.groups = 0;
  a.total = (long long)d.bs * d.oh * d.ow * d.c;
  h->generic = a;
  h->generic_grid = grid_for(a.total);
  const char *algo = d.algo == DFX_RESIZE_NEAREST ? "nearest" : "bilinear";
  if (h->path == DFX_RESIZE_BAND) {
    a.groups = (int)((long long)d.c * (long long)dt_size(d.dt) / 16);
    const long long per_band = (long long)d.bs * d.ow * a.groups;
    int rows = d.algo == DFX_RESIZE_NEAREST ? kNearestRows : kBilinearRows;
    if (const char *e2 = tuning_value("DFX_RESIZE_ROWS")) rows = std::max(1, std::min(atoi(e2), RESIZE_MAX_SIZE));  // testing / tuning aid
    else
      while (rows > 1 && per_band * ((d.oh + rows - 1) / rows) < 256ll * kFillBlocks) rows = (rows + 1) / 2;
    a.rows = rows;
    a.bands = (d.oh + rows - 1) / rows;
    a.total = per_band * a.bands;
    h->band = a;
    h->band_grid = grid_for(a.total);
    snprintf(h->kernel_name, sizeof(h->kernel_name), "resize_band<%s,%s%s> %d rows per lane", dt_name(d.dt), algo,
             d.add ? (d.post_relu ? ",add,relu" : ",add") : "", rows);
  } else {
    snprintf(h->kernel_name, sizeof(h->kernel_name), "resize_generic<%s,%s%s>", dt_name(d.dt), algo,
             d.add ? (d.post_relu ? ",add,relu" : ",add") : "");
  }
  *out = h;
  return DFX_OK;
}

int dfx_resize_submit(dfx_resize_t *h, const void *src_dev, const void *add_dev, void *dst_dev, dfx_stream_t s) {
  if (!h || !src_dev || !dst_dev) return fail(DFX_ERR_INVALID, "resize_submit: null argument");
  if (h->d.add && !add_dev) return fail(DFX_ERR_INVALID, "resize_submit: the descriptor has add = 1 but no tensor to add was given");
  if (!h->d.add && add_dev) return fail(DFX_ERR_INVALID, "resize_submit: a tensor to add was given but the descriptor has add = 0");
  const uintptr_t all = (uintptr_t)src_dev | (uintptr_t)dst_dev | (uintptr_t)add_dev;
  if (all % dt_size(h->d.dt))
    return fail(DFX_ERR_INVALID, "resize_submit: src, add or dst not aligned to the element size (%d bytes)", (int)dt_size(h->d.dt));
  const uintptr_t s0 = (uintptr_t)src_dev, d0 = (uintptr_t)dst_dev;
  if (s0 < d0 + dst_bytes(h->d) && d0 < s0 + src_bytes(h->d)) return fail(DFX_ERR_INVALID, "resize_submit: dst overlaps src");
  // a lane reads the add operand at the offset it then writes, so add may BE dst; any other overlap would race
  const uintptr_t a0 = (uintptr_t)add_dev;
  if (add_dev && a0 != d0 && a0 < d0 + dst_bytes(h->d) && d0 < a0 + dst_bytes(h->d))
    return fail(DFX_ERR_INVALID, "resize_submit: the tensor to add overlaps dst without being dst");
  DeviceGuard dg(h->device);
  // 16-byte accesses need aligned buffers: others take the per-element kernel for this submit, as pooling does
  const bool band = h->path == DFX_RESIZE_BAND && all % 16 == 0;
  ResizeArgs a = band ? h->band : h->generic;  // per-launch copy: concurrent submits on several streams are independent
  a.src = (const unsigned char *)src_dev;
  a.add = (const unsigned char *)add_dev;
  a.dst = (unsigned char *)dst_dev;
  const int rc = band ? launch_resize_band(a, h->band_grid, (hipStream_t)s) : launch_resize_generic(a, h->generic_grid, (hipStream_t)s);
  return g_launches.launched("resize", rc, band ? DFX_RESIZE_BAND : DFX_RESIZE_GENERIC);
}

// test hook: how many submits have launched each kernel so far (shows the per-submit fallback, which query cannot)
int dfx_debug_resize_launches(int64_t out[2]) { return g_launches.read("resize", out); }

int dfx_resize_submit_host(dfx_resize_t *h, const void *src_host, const void *add_host, void *dst_host) {
  if (!h || !src_host || !dst_host) return fail(DFX_ERR_INVALID, "resize_submit_host: null argument");
  if ((h->d.add != 0) != (add_host != nullptr))
    return fail(DFX_ERR_INVALID, "resize_submit_host: the tensor to add must be given exactly when the descriptor has add = 1");
  DeviceGuard dg(h->device);
  const void *srcs[2] = {src_host, add_host};
  const size_t bytes[2] = {src_bytes(h->d), dst_bytes(h->d)};
  return h->host.run(h->d.add ? 2 : 1, srcs, bytes, dst_host, dst_bytes(h->d),
                     [h](const void *const *sv, void *dv, dfx_stream_t st) {
                       return dfx_resize_submit(h, sv[0], h->d.add ? sv[1] : nullptr, dv, st);
                     });
}

int dfx_resize_query(const dfx_resize_t *h, dfx_resize_info *info) {
  if (const int rc = open_query("resize", h, info)) return rc;
  const bool band = h->path == DFX_RESIZE_BAND;
  info->grid = band ? h->band_grid : h->generic_grid;
  info->block = 256;
  info->lds_bytes = 0;
  info->rows_per_lane = band ? h->band.rows : 1;
  info->algorithmic_bytes = (uint64_t)src_bytes(h->d) + (uint64_t)dst_bytes(h->d) * (h->d.add ? 2 : 1);
  return DFX_OK;
}

int dfx_resize_destroy(dfx_resize_t *h) {
  release(h);
  return DFX_OK;
}

}  // extern "C"
