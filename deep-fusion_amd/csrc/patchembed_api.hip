// patchembed_api.hip -- host side of the int8 patch-embedding op (dfx_patchembed_* of include/dfx.h): descriptor validation,
// the path, the tile height and the grids (patchembed_plan.h, by linear_plan.h's rules), the device image and the requant
// route's proof (patchembed_pack.h over linear_pack.h), the overlap check and the choice of the kernel per submit, launches.
// The kernels are in patchembed.cuh / patchembed.hip.  The op has its own handle: weighted_op.h's skeleton has no table, no
// prefix and no token layout.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <new>
#include <vector>

#include "path_op.h"
#include "patchembed.cuh"
#include "patchembed_pack.h"
#include "patchembed_plan.h"

namespace dfx {
int launch_patchembed_tile(const PeArgs &a, int bm, int g, int grid, int lds, hipStream_t s, bool fast);
int launch_patchembed_generic(const PeArgs &a, int grid, hipStream_t s);
}
using namespace dfx;

struct dfx_patchembed {
  dfx_patchembed_desc d;
  int device = 0;
  int path = DFX_PATCHEMBED_GENERIC;
  int granule = 0;
  int bm = LIN_BM_MAX;           // tile kernel: rows per tile
  int grid[2] = {0, 0};          // per path; [path] and [DFX_PATCHEMBED_GENERIC] (the per-submit fallback) are used
  unsigned char *d_img = nullptr;  // packed weights | comp | bias | scale | K offsets | table | prefix
  PeImage im = {};
  PeArgs args = {};              // everything but src / dst / vec; copied per launch
  std::atomic<int> weights_set{0}, table_set{0}, prefix_set{0};
  int route = 0;                 // 0 exact, 1 fast (dfx_debug_conv_requant's numbering); tile path only
  // what the route is proved from, kept so that either setter can prove it again
  std::vector<int8_t> wperm;
  std::vector<unsigned char> bia;
  std::vector<float> scales, tmax;
  HostStaging host;
  char kernel_name[96] = "";
};

namespace {

void release(dfx_patchembed *h) {
  if (!h) return;
  DeviceGuard dg(h->device);
  h->host.release();
  (void)hipFree(h->d_img);
  delete h;
}

// launches since the library was loaded, by the kernel that ran; process-wide, because submit does not write to the
// handle (dfx_debug_patchembed_launches)
LaunchCounts<2> g_launches;

void set_name(dfx_patchembed *h) {
  const dfx_patchembed_desc &d = h->d;
  const char *tab = d.table ? " +table" : "";
  if (h->path == DFX_PATCHEMBED_TILE)
    snprintf(h->kernel_name, sizeof(h->kernel_name), "patchembed_tile<%s,%s,bm%d,g%d> %s%s", dt_name(d.src_dt), dt_name(d.dst_dt), h->bm, h->granule,
             !h->weights_set.load() ? "(no weights)" : h->route ? "fast" : "exact", tab);
  else
    snprintf(h->kernel_name, sizeof(h->kernel_name), "patchembed_generic<%s,%s>%s", dt_name(d.src_dt), dt_name(d.dst_dt), tab);
}

// packs everything below the table section from the handle's copies, uploads it and proves the route
int pack_and_prove(dfx_patchembed *h) {
  const dfx_patchembed_desc &d = h->d;
  std::vector<unsigned char> img;
  try {
    img.resize(h->im.off_table);
  } catch (const std::bad_alloc &) {
    return fail(DFX_ERR_HIP, "out of host memory");
  }
  const bool proven = pe_pack(d, h->wperm.data(), h->bia.empty() ? nullptr : h->bia.data(), h->scales.data(),
                              d.table && h->table_set.load() ? h->tmax.data() : nullptr, img.data());
  DeviceGuard dg(h->device);
  HIP_TRY(hipMemcpy(h->d_img, img.data(), img.size(), hipMemcpyHostToDevice));
  h->route = h->path == DFX_PATCHEMBED_TILE && d.round_mode == DFX_ROUND_NEAREST && proven && fast_allowed() ? 1 : 0;
  return DFX_OK;
}

}  // namespace

extern "C" {

int dfx_patchembed_create(const dfx_patchembed_desc *desc, dfx_patchembed_t **out) {
  dfx_patchembed *h = nullptr;
  int cus = 0;
  const int rc = open_create("patchembed", desc, out, &h, [](const dfx_patchembed_desc &d) { return validated("patchembed", pe_validate, d); }, &cus, release);
  if (rc) return rc;
  const dfx_patchembed_desc &d = *desc;
  // AUTO RULE (include/dfx.h DFX_PATCHEMBED_AUTO_NOTE)
  h->path = pe_path(d);
  h->granule = pe_granule(d);
  const char *fb = tuning_value("DFX_PATCHEMBED_BM");  // testing / tuning aid: 64 | 128, anything else is ignored
  h->bm = pe_bm(d, cus, fb ? atoi(fb) : 0);
  const long long cap = grid_cap("DFX_PATCHEMBED_GRID");
  h->grid[h->path] = pe_grid(d, h->path, h->bm, cus, cap);
  h->grid[DFX_PATCHEMBED_GENERIC] = pe_grid(d, DFX_PATCHEMBED_GENERIC, h->bm, cus, cap);
  h->im = pe_image(d);
  const hipError_t e = hipMalloc((void **)&h->d_img, h->im.bytes);
  if (e != hipSuccess) {
    release(h);
    return fail(DFX_ERR_HIP, "patchembed_create: device image: %s", hipGetErrorString(e));
  }
  try {
    h->tmax.assign((size_t)d.oc, 0.0f);
  } catch (const std::bad_alloc &) {
    release(h);
    return fail(DFX_ERR_HIP, "out of host memory");
  }
  const dfx_linear_desc g = pe_gemm(d, false);
  PeArgs &a = h->args;
  a.wpk = h->d_img;
  a.comp = reinterpret_cast<const int *>(h->d_img + h->im.lin.off_comp);
  a.bias = reinterpret_cast<const float *>(h->d_img + h->im.lin.off_bias);
  a.scale = reinterpret_cast<const float *>(h->d_img + h->im.lin.off_scale);
  a.ktab = reinterpret_cast<const int *>(h->d_img + h->im.off_ktab);
  a.table = d.table ? reinterpret_cast<const float *>(h->d_img + h->im.off_table) : nullptr;
  a.prefix = nullptr;
  a.rows = pe_rows(d); a.tokens = pe_tokens(d);
  a.img_rows = d.img_rows; a.dst_ld = d.dst_ld;
  a.img_bytes = (long long)d.ih * d.iw * d.ic; a.row_bytes = (long long)d.iw * d.ic;
  a.tw = d.tw; a.ph = d.ph; a.run = pe_run(d);
  a.k = g.k; a.n = d.oc; a.nks = lin_nslabs(g.k); a.tld = pe_table_ld(d.oc);
  a.t0 = d.tok_offset; a.bs = d.bs;
  a.a_u8 = d.src_dt == DFX_U8;
  a.dst_dt = d.dst_dt;
  a.relu = pe_relu(d) ? 1 : 0; a.rm = d.round_mode;
  a.mt = lin_mtiles(g.rows, h->bm); a.tiles = lin_tiles(g, h->bm);
  a.items = lin_items(g);
  a.pitems = 0;
  set_name(h);
  *out = h;
  return DFX_OK;
}

int dfx_patchembed_set_weights(dfx_patchembed_t *h, const int8_t *wei, const void *bia, const float *scales) {
  if (!h || !wei || !scales) return fail(DFX_ERR_INVALID, "patchembed_set_weights: null argument");
  const dfx_patchembed_desc &d = h->d;
  if (d.bia_dt != DFX_UNDEF && !bia) return fail(DFX_ERR_INVALID, "patchembed_set_weights: null bias");
  try {
    h->wperm.resize((size_t)d.oc * (size_t)pe_k(d));
    h->scales.assign(scales, scales + d.nscales);
    if (d.bia_dt != DFX_UNDEF) h->bia.assign((const unsigned char *)bia, (const unsigned char *)bia + (size_t)d.oc * (size_t)plan_dt_size(d.bia_dt));
  } catch (const std::bad_alloc &) {
    return fail(DFX_ERR_HIP, "out of host memory");
  }
  pe_permute(d, wei, h->wperm.data());
  const int rc = pack_and_prove(h);
  if (rc) return rc;
  h->weights_set.store(1);
  set_name(h);
  return DFX_OK;
}

int dfx_patchembed_set_table(dfx_patchembed_t *h, const float *table, int64_t ld) {
  if (!h || !table) return fail(DFX_ERR_INVALID, "patchembed_set_table: null argument");
  const dfx_patchembed_desc &d = h->d;
  if (!d.table) return fail(DFX_ERR_INVALID, "patchembed_set_table: the handle was created without a table");
  if (ld < d.oc) return fail(DFX_ERR_INVALID, "patchembed_set_table: ld below oc");
  std::vector<float> tmax;
  std::vector<unsigned char> img;
  try {
    tmax.resize((size_t)d.oc);
    img.resize(h->im.off_prefix - h->im.off_table);
  } catch (const std::bad_alloc &) {
    return fail(DFX_ERR_HIP, "out of host memory");
  }
  if (!pe_scan_table(d, table, ld, tmax.data())) return fail(DFX_ERR_INVALID, "patchembed_set_table: the table holds a non-finite entry");
  pe_pack_table(d, table, ld, reinterpret_cast<float *>(img.data()));
  {
    DeviceGuard dg(h->device);
    HIP_TRY(hipMemcpy(h->d_img + h->im.off_table, img.data(), img.size(), hipMemcpyHostToDevice));
  }
  h->tmax.swap(tmax);
  h->table_set.store(1);
  if (h->weights_set.load()) {  // the route rests on the table too
    const int rc = pack_and_prove(h);
    if (rc) return rc;
    set_name(h);
  }
  return DFX_OK;
}

int dfx_patchembed_set_prefix(dfx_patchembed_t *h, const void *rows) {
  if (!h || !rows) return fail(DFX_ERR_INVALID, "patchembed_set_prefix: null argument");
  const dfx_patchembed_desc &d = h->d;
  if (d.tok_offset < 1) return fail(DFX_ERR_INVALID, "patchembed_set_prefix: the handle has no prefix rows (tok_offset is 0)");
  DeviceGuard dg(h->device);
  HIP_TRY(hipMemcpy(h->d_img + h->im.off_prefix, rows, (size_t)d.tok_offset * (size_t)d.oc * (size_t)plan_dt_size(d.dst_dt), hipMemcpyHostToDevice));
  h->prefix_set.store(1);
  return DFX_OK;
}

int dfx_patchembed_submit(dfx_patchembed_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s) {
  if (!h || !src_dev || !dst_dev) return fail(DFX_ERR_INVALID, "patchembed_submit: null argument");
  const dfx_patchembed_desc &d = h->d;
  if (!h->weights_set.load()) return fail(DFX_ERR_STATE, "patchembed_submit: dfx_patchembed_set_weights not called");
  if (d.table && !h->table_set.load()) return fail(DFX_ERR_STATE, "patchembed_submit: dfx_patchembed_set_table not called");
  const unsigned esz = (unsigned)plan_dt_size(d.dst_dt);
  const uintptr_t src = (uintptr_t)src_dev, dst = (uintptr_t)dst_dev;
  if (dst % esz) return fail(DFX_ERR_INVALID, "patchembed_submit: dst is not aligned to its element");
  const unsigned long long first = (unsigned long long)(h->prefix_set.load() ? 0 : d.tok_offset) * d.dst_ld * esz;  // the first byte written
  if (plan_overlap(src, pe_src_extent(d), dst + first, pe_dst_extent(d) - first)) return fail(DFX_ERR_INVALID, "patchembed_submit: dst overlaps src");
  DeviceGuard dg(h->device);
  // the granule's loads need an aligned src: others take the generic kernel for this submit, as dfx_linear does
  const int path = h->granule && src % (unsigned)h->granule == 0 ? h->path : DFX_PATCHEMBED_GENERIC;
  PeArgs a = h->args;  // per launch: concurrent submits on several streams are independent
  a.src = (const unsigned char *)src_dev;
  a.dst = (unsigned char *)dst_dev;
  a.vec = dst % (4 * esz) == 0 && d.dst_ld % 4 == 0;
  if (h->prefix_set.load()) {
    a.prefix = h->d_img + h->im.off_prefix;
    a.pitems = (long long)d.bs * d.tok_offset * d.oc;
  }
  const int rc = path == DFX_PATCHEMBED_TILE
                     ? launch_patchembed_tile(a, h->bm, h->granule, h->grid[path], pe_lds_bytes(path, h->bm), (hipStream_t)s, h->route != 0)
                     : launch_patchembed_generic(a, h->grid[path], (hipStream_t)s);
  return g_launches.launched("patchembed", rc, path);
}

int dfx_patchembed_submit_host(dfx_patchembed_t *h, const void *src_host, void *dst_host) {
  if (!h || !src_host || !dst_host) return fail(DFX_ERR_INVALID, "patchembed_submit_host: null argument");
  const dfx_patchembed_desc &d = h->d;
  if (!h->weights_set.load()) return fail(DFX_ERR_STATE, "patchembed_submit_host: dfx_patchembed_set_weights not called");
  if (d.table && !h->table_set.load()) return fail(DFX_ERR_STATE, "patchembed_submit_host: dfx_patchembed_set_table not called");
  DeviceGuard dg(h->device);
  return h->host.run(src_host, (size_t)pe_src_extent(d), dst_host, (size_t)d.bs * (size_t)d.img_rows * (size_t)d.dst_ld * (size_t)plan_dt_size(d.dst_dt),
                     [h](const void *sp, void *dp, dfx_stream_t st) { return dfx_patchembed_submit(h, sp, dp, st); });
}

// test hook: how many submits have launched each kernel so far (shows the per-submit fallback, which query cannot)
int dfx_debug_patchembed_launches(int64_t out[2]) { return g_launches.read("patchembed", out); }

// test hook: the requant route as the handle's weights and table prove it (numbering of dfx_debug_conv_requant)
int dfx_debug_patchembed_requant(const dfx_patchembed_t *h, int32_t out[1]) {
  if (!h || !out) return fail(DFX_ERR_INVALID, "patchembed_requant: null argument");
  if (!h->weights_set.load()) return fail(DFX_ERR_STATE, "patchembed_requant: dfx_patchembed_set_weights not called");
  out[0] = h->route;
  return DFX_OK;
}

int dfx_patchembed_query(const dfx_patchembed_t *h, dfx_patchembed_info *info) {
  if (const int rc = open_query("patchembed", h, info)) return rc;
  info->grid = h->grid[h->path];
  info->block = LIN_THREADS;
  info->lds_bytes = pe_lds_bytes(h->path, h->bm);
  info->granule = h->granule;
  info->algorithmic_ops = pe_algorithmic_ops(h->d);
  info->algorithmic_bytes = pe_algorithmic_bytes(h->d, h->prefix_set.load() != 0);
  return DFX_OK;
}

int dfx_patchembed_destroy(dfx_patchembed_t *h) {
  release(h);
  return DFX_OK;
}

}  // extern "C"
