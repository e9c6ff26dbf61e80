// select_api.hip -- host side of the image-wide top-K with peak filter (dfx_select_* of include/dfx.h): descriptor
// validation, the chunk plan and the scratch layout (all in select_plan.h), the overlap check and the choice of the
// kernels per submit, the order of the submits that share the handle's scratch.  The kernels are in select.cuh.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "path_op.h"
#include "select.cuh"
#include "select_plan.h"

namespace dfx {
void launch_select_generic(const SelectArgs &a, int grid, hipStream_t s);
void launch_select_hist(const SelectArgs &a, int grid, hipStream_t s);
void launch_select_scan(const SelectArgs &a, int grid, hipStream_t s);
void launch_select_compact(const SelectArgs &a, int grid, hipStream_t s);
void launch_select_sort(const SelectArgs &a, int grid, hipStream_t s);
}
using namespace dfx;

struct dfx_select {
  dfx_select_desc d;
  int device = 0;
  int path = DFX_SELECT_GENERIC;
  SelectPlan plan = {};            // histogram path
  SelectScratch layout = {};
  unsigned char *d_scratch = nullptr;
  SelectArgs args = {};            // without the submit's pointers
  TwoLaunchOrder order;            // the launches of a histogram-path submit meet in d_scratch
  char kernel_name[96] = "";
};

namespace {

void release(dfx_select *h) {
  if (!h) return;
  DeviceGuard dg(h->device);
  (void)hipFree(h->d_scratch);
  h->order.destroy();
  delete h;
}

// submits since the library was loaded, by the path that ran (dfx_debug_select_launches)
LaunchCounts<2> g_launches;

}  // namespace

extern "C" {

int dfx_select_create(const dfx_select_desc *desc, dfx_select_t **out) {
  dfx_select *h = nullptr;
  const int rc = open_create("select", desc, out, &h, [](const dfx_select_desc &d) {
    if (const int bad = validated("select", select_validate, d)) return bad;
    if (d.force_path == DFX_SELECT_HIST && !select_hist_class(d))
      return fail(DFX_ERR_UNSUPPORTED, "select_create: descriptor outside the histogram path's class (src_ld a multiple of 16)");
    return (int)DFX_OK;
  });
  if (rc) return rc;
  const dfx_select_desc &d = *desc;
  // AUTO RULE (include/dfx.h DFX_SELECT_AUTO_NOTE)
  h->path = select_path(d);
  const long long px = (long long)d.h * d.w;
  SelectArgs &a = h->args;
  a.bs = d.bs; a.h = d.h; a.w = d.w; a.c = d.c; a.src_ld = d.src_ld; a.k = d.k; a.idx_ld = d.idx_ld;
  a.peak = d.peak; a.src_dt = d.src_dt;
  a.min_key = (int)select_key8((unsigned)d.min_val & 0xffu, d.src_dt);
  a.n_gather = d.n_gather;
  for (int i = 0; i < d.n_gather; ++i) {
    a.row_bytes[i] = d.row_bytes[i];
    a.pixel_stride[i] = d.pixel_stride_bytes[i];
  }
  a.chunks = 1;
  a.chunk_px = (int)std::min<long long>(px, 2147483647ll);
  a.items = d.bs;
  if (h->path == DFX_SELECT_HIST) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, h->device) != hipSuccess) {
      release(h);
      return fail(DFX_ERR_HIP, "select_create: cannot query the device");
    }
    long long forced = 0;
    if (const char *e = tuning_value("DFX_SELECT_CHUNK")) forced = std::max(1ll, atoll(e));  // testing / tuning aid: clamped by the planner
    h->plan = select_plan(d.bs, px, d.src_ld, std::max(1, prop.multiProcessorCount), forced);
    h->layout = select_scratch(d.bs, h->plan.chunks, d.k);
    hipError_t e = hipMalloc((void **)&h->d_scratch, h->layout.bytes);
    if (e == hipSuccess) e = h->order.create();
    if (e != hipSuccess) {
      release(h);
      return fail(DFX_ERR_HIP, "select_create: scratch: %s", hipGetErrorString(e));
    }
    a.chunks = h->plan.chunks;
    a.chunk_px = h->plan.chunk_px;
    a.items = h->plan.items;
    a.slab = (unsigned *)h->d_scratch;
    a.plan = (unsigned *)(h->d_scratch + h->layout.off_plan);
    a.cand = (unsigned long long *)(h->d_scratch + h->layout.off_cand);
  }
  snprintf(h->kernel_name, sizeof(h->kernel_name), "select_%s<%s,%s,k%d>", h->path == DFX_SELECT_HIST ? "hist" : "generic",
           d.peak == DFX_SELECT_PEAK3 ? "peak3" : "all", d.src_dt == DFX_S8 ? "s8" : "u8", d.k);
  *out = h;
  return DFX_OK;
}

int dfx_select_submit(dfx_select_t *h, const void *src_dev, void *idx_dev, void *val_or_null_dev, void *count_dev,
                      const void *const *gather_src_dev, void *const *gather_dst_dev, dfx_stream_t s) {
  if (!h || !src_dev || !idx_dev || !count_dev) return fail(DFX_ERR_INVALID, "select_submit: null argument");
  const dfx_select_desc &d = h->d;
  if (d.n_gather > 0 && (!gather_src_dev || !gather_dst_dev)) return fail(DFX_ERR_INVALID, "select_submit: null gather array");
  for (int i = 0; i < d.n_gather; ++i)
    if (!gather_src_dev[i] || !gather_dst_dev[i]) return fail(DFX_ERR_INVALID, "select_submit: null gather pointer");
  const uintptr_t src = (uintptr_t)src_dev, idx = (uintptr_t)idx_dev, val = (uintptr_t)val_or_null_dev, cnt = (uintptr_t)count_dev;
  if (idx % 4 || cnt % 4) return fail(DFX_ERR_INVALID, "select_submit: idx or count is not aligned to its element");
  // every output against every input and every other output
  uintptr_t in_p[1 + DFX_SELECT_MAX_GATHER], out_p[3 + DFX_SELECT_MAX_GATHER];
  unsigned long long in_n[1 + DFX_SELECT_MAX_GATHER], out_n[3 + DFX_SELECT_MAX_GATHER];
  int n_in = 0, n_out = 0;
  in_p[n_in] = src; in_n[n_in++] = select_src_extent(d);
  out_p[n_out] = idx; out_n[n_out++] = select_idx_extent(d, 4);
  out_p[n_out] = cnt; out_n[n_out++] = (unsigned long long)d.bs * 4;
  if (val) { out_p[n_out] = val; out_n[n_out++] = select_idx_extent(d, 1); }
  uintptr_t align = src | idx | val | cnt;
  for (int i = 0; i < d.n_gather; ++i) {
    in_p[n_in] = (uintptr_t)gather_src_dev[i]; in_n[n_in++] = select_gather_src_extent(d, i);
    out_p[n_out] = (uintptr_t)gather_dst_dev[i]; out_n[n_out++] = select_gather_dst_extent(d, i);
    align |= (uintptr_t)gather_dst_dev[i];
  }
  for (int o = 0; o < n_out; ++o) {
    for (int i = 0; i < n_in; ++i)
      if (plan_overlap(out_p[o], out_n[o], in_p[i], in_n[i])) return fail(DFX_ERR_INVALID, "select_submit: an output overlaps src or a gather source");
    for (int p = o + 1; p < n_out; ++p)
      if (plan_overlap(out_p[o], out_n[o], out_p[p], out_n[p])) return fail(DFX_ERR_INVALID, "select_submit: two outputs overlap");
  }
  DeviceGuard dg(h->device);
  const hipStream_t st = (hipStream_t)s;
  // 16-byte loads need aligned buffers: others take the generic kernel for this submit, as the head does
  const int path = align % 16 == 0 ? h->path : DFX_SELECT_GENERIC;
  SelectArgs a = h->args;  // per-launch copy
  a.src = (const unsigned char *)src_dev;
  a.idx = (int *)idx_dev;
  a.val = (unsigned char *)val_or_null_dev;
  a.count = (int *)count_dev;
  for (int i = 0; i < d.n_gather; ++i) {
    a.gsrc[i] = (const unsigned char *)gather_src_dev[i];
    a.gdst[i] = (unsigned char *)gather_dst_dev[i];
  }
  const int image_grid = select_image_grid(d.bs);
  if (path == DFX_SELECT_GENERIC) {  // one launch, nothing of the handle's: independent of every other submit
    launch_select_generic(a, image_grid, st);
    HIP_TRY(hipGetLastError());
    g_launches.hit(DFX_SELECT_GENERIC);
    return DFX_OK;
  }
  // four launches through the handle's scratch: serialised (dfx.h; TwoLaunchOrder in dfx_internal.h)
  std::lock_guard<std::mutex> lk(h->order.mu);
  int rc = h->order.enter(st);
  if (rc) return rc;
  launch_select_hist(a, h->plan.grid, st);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) {
    launch_select_scan(a, image_grid, st);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    launch_select_compact(a, h->plan.grid, st);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    launch_select_sort(a, image_grid, st);
    e = hipGetLastError();
  }
  // (once a launch is out the scratch has a writer in flight: every way out goes through leave())
  rc = h->order.leave(st);
  if (e != hipSuccess) return fail(DFX_ERR_HIP, "select_submit: %s", hipGetErrorString(e));
  if (rc == DFX_OK) g_launches.hit(DFX_SELECT_HIST);
  return rc;
}

// test hook: how many submits have run on each path so far (shows the per-submit fallback, which query cannot)
int dfx_debug_select_launches(int64_t out[2]) { return g_launches.read("select", out); }

int dfx_select_query(const dfx_select_t *h, dfx_select_info *info) {
  if (const int rc = open_query("select", h, info)) return rc;
  const bool hist = h->path == DFX_SELECT_HIST;
  info->chunks = h->args.chunks;
  info->chunk_pixels = h->args.chunk_px;
  info->grid = hist ? h->plan.grid : select_image_grid(h->d.bs);
  info->grid_image = select_image_grid(h->d.bs);
  info->block = hist ? SELECT_THREADS : SELECT_SORT_THREADS;
  info->block_image = SELECT_SORT_THREADS;
  info->lds_bytes = select_lds_bytes(h->path);
  info->launches = select_launches(h->path);
  info->scratch_bytes = hist ? h->layout.bytes : 0;
  info->algorithmic_bytes = select_algorithmic_bytes(h->d);
  return DFX_OK;
}

int dfx_select_destroy(dfx_select_t *h) {
  release(h);
  return DFX_OK;
}

}  // extern "C"
