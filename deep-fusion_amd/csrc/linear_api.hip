// linear_api.hip -- host side of the int8 token linear op (dfx_linear_* of include/dfx.h): descriptor validation, the path,
// the tile height and the grids (all planned in linear_plan.h), the device image and the requant route's proof
// (linear_pack.h), the overlap check and the choice of the kernel per submit, launches.  The kernels are in linear.cuh /
// linear.hip.  The op has its own handle: weighted_op.h's skeleton has no src dtype, no pitches and no table.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <new>
#include <vector>

#include "path_op.h"
#include "linear.cuh"
#include "linear_pack.h"
#include "linear_plan.h"

namespace dfx {
int launch_linear_tile(const LinArgs &a, int bm, int grid, int lds, hipStream_t s, bool fast);
int launch_linear_generic(const LinArgs &a, int grid, hipStream_t s);
}
using namespace dfx;

struct dfx_linear {
  dfx_linear_desc d;
  int device = 0;
  int path = DFX_LINEAR_GENERIC;
  int bm = LIN_BM_MAX;           // tile kernel: rows per tile
  int grid[2] = {0, 0};          // per path; [path] and [DFX_LINEAR_GENERIC] (the per-submit fallback) are used
  unsigned char *d_img = nullptr;  // packed weights | comp | bias | scale | table
  LinImage im = {};
  LinArgs args = {};             // everything but src / dst / vec; copied per launch
  std::atomic<int> weights_set{0}, table_set{0};
  int route = 0;                 // 0 exact, 1 fast (dfx_debug_conv_requant's numbering); tile path only
  HostStaging host;
  char kernel_name[96] = "";
};

namespace {

void release(dfx_linear *h) {
  if (!h) return;
  DeviceGuard dg(h->device);
  h->host.release();
  (void)hipFree(h->d_img);
  delete h;
}

// launches since the library was loaded, by the kernel that ran; process-wide, because submit does not write to the
// handle (dfx_debug_linear_launches)
LaunchCounts<2> g_launches;

void set_name(dfx_linear *h) {
  const dfx_linear_desc &d = h->d;
  const char *lut = lin_has_table(d) ? " +lut" : "";
  if (h->path == DFX_LINEAR_TILE)
    snprintf(h->kernel_name, sizeof(h->kernel_name), "linear_tile<%s,%s,bm%d> %s%s", dt_name(d.src_dt), dt_name(d.dst_dt), h->bm,
             !h->weights_set.load() ? "(no weights)" : h->route ? "fast" : "exact", lut);
  else
    snprintf(h->kernel_name, sizeof(h->kernel_name), "linear_generic<%s,%s>%s", dt_name(d.src_dt), dt_name(d.dst_dt), lut);
}

}  // namespace

extern "C" {

int dfx_linear_create(const dfx_linear_desc *desc, dfx_linear_t **out) {
  dfx_linear *h = nullptr;
  int cus = 0;
  const int rc = open_create("linear", desc, out, &h, [](const dfx_linear_desc &d) { return validated("linear", lin_validate, d); }, &cus, release);
  if (rc) return rc;
  const dfx_linear_desc &d = *desc;
  // AUTO RULE (include/dfx.h DFX_LINEAR_AUTO_NOTE)
  h->path = lin_path(d);
  const char *fb = tuning_value("DFX_LINEAR_BM");  // testing / tuning aid: 64 | 128, anything else is ignored
  h->bm = lin_bm(d, cus, fb ? atoi(fb) : 0);
  const long long cap = grid_cap("DFX_LINEAR_GRID");
  h->grid[h->path] = lin_grid(d, h->path, h->bm, cus, cap);
  h->grid[DFX_LINEAR_GENERIC] = lin_grid(d, DFX_LINEAR_GENERIC, h->bm, cus, cap);
  h->im = lin_image(d.n, d.k);
  const hipError_t e = hipMalloc((void **)&h->d_img, h->im.bytes);
  if (e != hipSuccess) {
    release(h);
    return fail(DFX_ERR_HIP, "linear_create: weight image: %s", hipGetErrorString(e));
  }
  LinArgs &a = h->args;
  a.wpk = h->d_img;
  a.comp = reinterpret_cast<const int *>(h->d_img + h->im.off_comp);
  a.bias = reinterpret_cast<const float *>(h->d_img + h->im.off_bias);
  a.scale = reinterpret_cast<const float *>(h->d_img + h->im.off_scale);
  a.lut = lin_has_table(d) ? h->d_img + h->im.off_table : nullptr;
  a.rows = d.rows; a.src_ld = d.src_ld; a.dst_ld = d.dst_ld;
  a.k = d.k; a.n = d.n; a.nks = lin_nslabs(d.k);
  a.a_u8 = d.src_dt == DFX_U8;
  a.req_dt = lin_requant_dt(d);
  a.lut_u8 = d.lut_in_dt == DFX_U8;
  a.relu = lin_relu(d) ? 1 : 0; a.rm = d.round_mode;
  a.mt = lin_mtiles(d.rows, h->bm); a.tiles = lin_tiles(d, h->bm);
  a.items = lin_items(d);
  set_name(h);
  *out = h;
  return DFX_OK;
}

int dfx_linear_set_weights(dfx_linear_t *h, const int8_t *wei, const void *bia, const float *scales) {
  if (!h || !wei || !scales) return fail(DFX_ERR_INVALID, "linear_set_weights: null argument");
  const dfx_linear_desc &d = h->d;
  if (d.bia_dt != DFX_UNDEF && !bia) return fail(DFX_ERR_INVALID, "linear_set_weights: null bias");
  std::vector<unsigned char> img;
  try {
    img.resize(h->im.off_table);
  } catch (const std::bad_alloc &) {
    return fail(DFX_ERR_HIP, "out of host memory");
  }
  const bool proven = lin_pack(d, wei, bia, scales, img.data());
  DeviceGuard dg(h->device);
  HIP_TRY(hipMemcpy(h->d_img, img.data(), img.size(), hipMemcpyHostToDevice));  // (the table section keeps what set_table put there)
  h->route = h->path == DFX_LINEAR_TILE && d.round_mode == DFX_ROUND_NEAREST && proven && fast_allowed() ? 1 : 0;
  h->weights_set.store(1);
  set_name(h);
  return DFX_OK;
}

int dfx_linear_set_table(dfx_linear_t *h, const uint8_t lut[256]) {
  if (!h || !lut) return fail(DFX_ERR_INVALID, "linear_set_table: null argument");
  if (!lin_has_table(h->d)) return fail(DFX_ERR_INVALID, "linear_set_table: the handle was created without a table (lut_in_dt)");
  DeviceGuard dg(h->device);
  HIP_TRY(hipMemcpy(h->d_img + h->im.off_table, lut, 256, hipMemcpyHostToDevice));
  h->table_set.store(1);
  return DFX_OK;
}

int dfx_linear_submit(dfx_linear_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s) {
  if (!h || !src_dev || !dst_dev) return fail(DFX_ERR_INVALID, "linear_submit: null argument");
  const dfx_linear_desc &d = h->d;
  if (!h->weights_set.load()) return fail(DFX_ERR_STATE, "linear_submit: dfx_linear_set_weights not called");
  if (lin_has_table(d) && !h->table_set.load()) return fail(DFX_ERR_STATE, "linear_submit: dfx_linear_set_table not called");
  const unsigned esz = (unsigned)plan_dt_size(d.dst_dt);
  const uintptr_t src = (uintptr_t)src_dev, dst = (uintptr_t)dst_dev;
  if (dst % esz) return fail(DFX_ERR_INVALID, "linear_submit: dst is not aligned to its element");
  if (plan_overlap(src, plan_extent(d.rows, d.src_ld, d.k, 1), dst, plan_extent(d.rows, d.dst_ld, d.n, (int)esz)))
    return fail(DFX_ERR_INVALID, "linear_submit: dst overlaps src");
  DeviceGuard dg(h->device);
  // 16-byte loads need an aligned src: others take the generic kernel for this submit, as lnorm and bmm do
  const int path = src % 16 == 0 ? h->path : DFX_LINEAR_GENERIC;
  LinArgs a = h->args;  // per launch: concurrent submits on several streams are independent
  a.src = (const unsigned char *)src_dev;
  a.dst = (unsigned char *)dst_dev;
  a.vec = dst % (4 * esz) == 0 && d.dst_ld % 4 == 0;
  const int rc = path == DFX_LINEAR_TILE ? launch_linear_tile(a, h->bm, h->grid[path], lin_lds_bytes(path, h->bm), (hipStream_t)s, h->route != 0)
                                         : launch_linear_generic(a, h->grid[path], (hipStream_t)s);
  return g_launches.launched("linear", rc, path);
}

int dfx_linear_submit_host(dfx_linear_t *h, const void *src_host, void *dst_host) {
  if (!h || !src_host || !dst_host) return fail(DFX_ERR_INVALID, "linear_submit_host: null argument");
  const dfx_linear_desc &d = h->d;
  if (!h->weights_set.load()) return fail(DFX_ERR_STATE, "linear_submit_host: dfx_linear_set_weights not called");
  if (lin_has_table(d) && !h->table_set.load()) return fail(DFX_ERR_STATE, "linear_submit_host: dfx_linear_set_table not called");
  if (d.src_ld != d.k || d.dst_ld != d.n) return fail(DFX_ERR_UNSUPPORTED, "linear_submit_host: densely packed operands only (src_ld == k, dst_ld == n)");
  DeviceGuard dg(h->device);
  return h->host.run(src_host, (size_t)d.rows * (size_t)d.k, dst_host, (size_t)d.rows * (size_t)d.n * (size_t)plan_dt_size(d.dst_dt),
                     [h](const void *sp, void *dp, dfx_stream_t st) { return dfx_linear_submit(h, sp, dp, st); });
}

// test hook: how many submits have launched each kernel so far (shows the per-submit fallback, which query cannot)
int dfx_debug_linear_launches(int64_t out[2]) { return g_launches.read("linear", out); }

// test hook: the requant route the last dfx_linear_set_weights proved (numbering of dfx_debug_conv_requant)
int dfx_debug_linear_requant(const dfx_linear_t *h, int32_t out[1]) {
  if (!h || !out) return fail(DFX_ERR_INVALID, "linear_requant: null argument");
  if (!h->weights_set.load()) return fail(DFX_ERR_STATE, "linear_requant: dfx_linear_set_weights not called");
  out[0] = h->route;
  return DFX_OK;
}

int dfx_linear_query(const dfx_linear_t *h, dfx_linear_info *info) {
  if (const int rc = open_query("linear", h, info)) return rc;
  info->grid = h->grid[h->path];
  info->block = LIN_THREADS;
  info->lds_bytes = lin_lds_bytes(h->path, h->bm);
  info->algorithmic_ops = lin_algorithmic_ops(h->d);
  info->algorithmic_bytes = lin_algorithmic_bytes(h->d);
  return DFX_OK;
}

int dfx_linear_destroy(dfx_linear_t *h) {
  release(h);
  return DFX_OK;
}

}  // extern "C"
