// roialign_api.hip -- host side of RoIAlign (dfx_roialign_* of include/dfx.h): descriptor validation, the class test and
// the grid / split choice (all in roialign_plan.h), the pointer and overlap checks and the choice of the kernel per submit.
// The kernels are in roialign.cuh.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "path_op.h"
#include "roialign.cuh"
#include "roialign_plan.h"

namespace dfx {
void launch_roialign_generic(const RoiArgs &a, int dt, int grid, hipStream_t s);
void launch_roialign_tile(const RoiArgs &a, int dt, unsigned grid, hipStream_t s);
}
using namespace dfx;

struct dfx_roialign {
  dfx_roialign_desc d;
  int device = 0;
  int path = DFX_ROIALIGN_GENERIC;
  RoiArgs args = {};               // without the submit's pointers
  char kernel_name[96] = "";
};

namespace {

void release(dfx_roialign *h) {
  if (!h) return;
  DeviceGuard dg(h->device);
  delete h;
}

// submits since the library was loaded, by the kernel that ran (dfx_debug_roialign_launches)
LaunchCounts<2> g_launches;

}  // namespace

extern "C" {

int dfx_roialign_create(const dfx_roialign_desc *desc, dfx_roialign_t **out) {
  dfx_roialign *h = nullptr;
  const int rc = open_create("roialign", desc, out, &h, [](const dfx_roialign_desc &d) { return validated("roialign", roi_validate, d); });
  if (rc) return rc;
  const dfx_roialign_desc &d = *desc;
  // AUTO RULE (include/dfx.h DFX_ROIALIGN_AUTO_NOTE)
  h->path = roi_path(d);
  RoiArgs &a = h->args;
  for (int l = 0; l < 4; ++l) {
    const int u = l < d.levels ? l : 0;  // unused levels mirror level 0: never selected, never garbage
    a.h[l] = d.h[u]; a.w[l] = d.w[u]; a.ld[l] = d.src_ld[u]; a.scale[l] = d.spatial_scale[u];
  }
  for (int i = 0; i < 3; ++i) a.thr[i] = i + 1 < d.levels ? d.level_area_thr[i] : 0.0f;
  a.bs = d.bs; a.n = d.n; a.mode = d.mode; a.levels = d.levels; a.c = d.c; a.ph = d.ph; a.pw = d.pw; a.S = d.sampling_ratio;
  a.aligned = d.aligned; a.dst_ld = d.dst_ld;
  a.rows_per_group = roi_rows_per_group(d);
  a.splits = roi_splits(d);
  a.elements = roi_elements(d);
  snprintf(h->kernel_name, sizeof(h->kernel_name), "roialign_%s<%s,%dx%d,s%d,l%d>", h->path == DFX_ROIALIGN_TILE ? "tile" : "generic",
           d.dt == DFX_U8 ? "u8" : d.dt == DFX_S8 ? "s8" : "f32", d.ph, d.pw, d.sampling_ratio, d.levels);
  *out = h;
  return DFX_OK;
}

int dfx_roialign_submit(dfx_roialign_t *h, const dfx_roialign_io *io, dfx_stream_t s) {
  if (!h || !io) return fail(DFX_ERR_INVALID, "roialign_submit: null argument");
  const dfx_roialign_desc &d = h->d;
  const bool list = d.mode == DFX_ROI_LIST;
  if (!io->boxes || !io->dst) return fail(DFX_ERR_INVALID, "roialign_submit: null boxes or dst");
  if (list && !io->batch_idx) return fail(DFX_ERR_INVALID, "roialign_submit: null batch_idx");
  for (int l = 0; l < d.levels; ++l)
    if (!io->src[l]) return fail(DFX_ERR_INVALID, "roialign_submit: null level");
  // inputs the kernels read, with their extents
  uintptr_t in_p[6];
  unsigned long long in_n[6];
  int n_in = 0;
  uintptr_t four = (uintptr_t)io->boxes, align = (uintptr_t)io->boxes | (uintptr_t)io->dst;
  for (int l = 0; l < d.levels; ++l) {
    in_p[n_in] = (uintptr_t)io->src[l]; in_n[n_in++] = roi_level_extent(d, l);
    align |= (uintptr_t)io->src[l];
    if (d.dt == DFX_F32) four |= (uintptr_t)io->src[l];
  }
  in_p[n_in] = (uintptr_t)io->boxes; in_n[n_in++] = roi_boxes_extent(d);
  if (list) {
    in_p[n_in] = (uintptr_t)io->batch_idx; in_n[n_in++] = roi_rows(d) * 4;
    four |= (uintptr_t)io->batch_idx;
  } else if (io->count) {
    in_p[n_in] = (uintptr_t)io->count; in_n[n_in++] = (unsigned long long)d.bs * 4;
    four |= (uintptr_t)io->count;
  }
  if (d.dt == DFX_F32) four |= (uintptr_t)io->dst;
  if (four % 4) return fail(DFX_ERR_INVALID, "roialign_submit: a pointer to 4-byte elements is not 4-byte aligned");
  for (int i = 0; i < n_in; ++i)
    if (plan_overlap((uintptr_t)io->dst, roi_dst_extent(d), in_p[i], in_n[i])) return fail(DFX_ERR_INVALID, "roialign_submit: dst overlaps an input");
  DeviceGuard dg(h->device);
  const hipStream_t st = (hipStream_t)s;
  // 16-byte loads and stores need aligned buffers: others take the generic kernel for this submit, as in dfx_nms
  const int path = align % 16 == 0 ? h->path : DFX_ROIALIGN_GENERIC;
  RoiArgs a = h->args;  // per-launch copy
  for (int l = 0; l < 4; ++l) a.src[l] = io->src[l < d.levels ? l : 0];
  a.boxes = (const float *)io->boxes;
  a.count = list ? nullptr : (const int *)io->count;
  a.batch_idx = list ? (const int *)io->batch_idx : nullptr;
  a.dst = io->dst;
  if (path == DFX_ROIALIGN_TILE) launch_roialign_tile(a, d.dt, roi_tile_grid(d), st);
  else launch_roialign_generic(a, d.dt, roi_generic_grid(d), st);
  HIP_TRY(hipGetLastError());
  g_launches.hit(path);
  return DFX_OK;
}

// test hook: how many submits have launched each kernel so far (shows the per-submit fallback, which query cannot)
int dfx_debug_roialign_launches(int64_t out[2]) { return g_launches.read("roialign", out); }

int dfx_roialign_query(const dfx_roialign_t *h, dfx_roialign_info *info) {
  if (const int rc = open_query("roialign", h, info)) return rc;
  const dfx_roialign_desc &d = h->d;
  const bool tile = h->path == DFX_ROIALIGN_TILE;
  info->grid = roi_grid(d, h->path);
  info->block = ROI_THREADS;
  info->lds_bytes = roi_lds_bytes(h->path);
  info->launches = 1;
  info->rows_per_group = tile ? roi_rows_per_group(d) : 0;
  info->algorithmic_bytes = roi_algorithmic_bytes(d);
  return DFX_OK;
}

int dfx_roialign_destroy(dfx_roialign_t *h) {
  release(h);
  return DFX_OK;
}

}  // extern "C"
