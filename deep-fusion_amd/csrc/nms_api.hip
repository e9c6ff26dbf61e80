// nms_api.hip -- host side of the box decode + greedy NMS (dfx_nms_* of include/dfx.h): descriptor validation, the tile
// table and the scratch layout (all in nms_plan.h), the pointer and overlap checks and the choice of the kernels per submit,
// the order of the submits that share the handle's scratch.  The kernels are in nms.cuh.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "path_op.h"
#include "nms.cuh"
#include "nms_plan.h"

namespace dfx {
void launch_nms_generic(const NmsArgs &a, int grid, hipStream_t s);
void launch_nms_prep(const NmsArgs &a, int grid, hipStream_t s);
void launch_nms_mask(const NmsArgs &a, int grid, hipStream_t s);
void launch_nms_scan(const NmsArgs &a, int grid, hipStream_t s);
}
using namespace dfx;

struct dfx_nms {
  dfx_nms_desc d;
  int device = 0;
  int path = DFX_NMS_GENERIC;
  NmsScratch layout = {};
  unsigned char *d_scratch = nullptr;
  NmsArgs args = {};               // without the submit's pointers
  TwoLaunchOrder order;            // the launches of a mask-path submit meet in d_scratch
  char kernel_name[96] = "";
};

namespace {

void release(dfx_nms *h) {
  if (!h) return;
  DeviceGuard dg(h->device);
  (void)hipFree(h->d_scratch);
  h->order.destroy();
  delete h;
}

// submits since the library was loaded, by the path that ran (dfx_debug_nms_launches)
LaunchCounts<2> g_launches;

}  // namespace

extern "C" {

int dfx_nms_create(const dfx_nms_desc *desc, dfx_nms_t **out) {
  dfx_nms *h = nullptr;
  const int rc = open_create("nms", desc, out, &h, [](const dfx_nms_desc &d) { return validated("nms", nms_validate, d); });
  if (rc) return rc;
  const dfx_nms_desc &d = *desc;
  // AUTO RULE (include/dfx.h DFX_NMS_AUTO_NOTE)
  h->path = nms_path(d);
  NmsArgs &a = h->args;
  a.bs = d.bs; a.n = d.n; a.n64 = nms_blocks(d.n); a.max_out = d.max_out; a.keep_ld = d.keep_ld; a.mode = d.mode;
  a.per_class = d.per_class; a.classes = d.classes; a.apx = d.anchors_per_pixel; a.row_bytes = d.row_bytes; a.idx_ld = d.idx_ld;
  a.n_tiles = nms_tiles(d.n);
  a.n_entries = (long long)d.n_anchors * d.classes;
  a.iou_thr = d.iou_thr; a.clip_w = d.clip_w; a.clip_h = d.clip_h;
  if (h->path == DFX_NMS_MASK) {
    h->layout = nms_scratch(d.bs, d.n);
    std::vector<uint16_t> tiles((size_t)a.n_tiles);
    nms_enumerate_tiles(d.n, tiles.data());
    hipError_t e = hipMalloc((void **)&h->d_scratch, h->layout.bytes);
    if (e == hipSuccess) e = hipMemcpy(h->d_scratch + h->layout.off_tiles, tiles.data(), tiles.size() * 2, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = h->order.create();
    if (e != hipSuccess) {
      release(h);
      return fail(DFX_ERR_HIP, "nms_create: scratch: %s", hipGetErrorString(e));
    }
    a.box = (v4f *)h->d_scratch;
    a.lab = (int *)(h->d_scratch + h->layout.off_lab);
    a.mask = (unsigned long long *)(h->d_scratch + h->layout.off_mask);
    a.tiles = (const unsigned short *)(h->d_scratch + h->layout.off_tiles);
  }
  snprintf(h->kernel_name, sizeof(h->kernel_name), "nms_%s<%s,%s,n%d>", h->path == DFX_NMS_MASK ? "mask" : "generic",
           d.mode == DFX_NMS_DECODE ? "decode" : "boxes", d.per_class ? "perclass" : "agnostic", d.n);
  *out = h;
  return DFX_OK;
}

int dfx_nms_submit(dfx_nms_t *h, const dfx_nms_io *io, dfx_stream_t s) {
  if (!h || !io) return fail(DFX_ERR_INVALID, "nms_submit: null argument");
  const dfx_nms_desc &d = h->d;
  const bool decode = d.mode == DFX_NMS_DECODE, reads_idx = nms_reads_idx(d);
  if (!io->keep || !io->count) return fail(DFX_ERR_INVALID, "nms_submit: null keep or count");
  if (decode ? (!io->deltas || !io->anchors || !io->tab_c || !io->tab_s) : !io->boxes) return fail(DFX_ERR_INVALID, "nms_submit: null input of the mode");
  if (reads_idx && !io->idx) return fail(DFX_ERR_INVALID, "nms_submit: null idx");
  // inputs the kernels read, with their extents
  uintptr_t in_p[7], out_p[3];
  unsigned long long in_n[7], out_n[3];
  int n_in = 0, n_out = 0;
  uintptr_t four = 0, align = 0;  // pointers to 4-byte elements; pointers the mask path reads or writes 16 bytes at a time
  if (decode) {
    in_p[n_in] = (uintptr_t)io->deltas; in_n[n_in++] = nms_deltas_extent(d);
    in_p[n_in] = (uintptr_t)io->anchors; in_n[n_in++] = nms_anchors_extent(d);
    in_p[n_in] = (uintptr_t)io->tab_c; in_n[n_in++] = 1024;
    in_p[n_in] = (uintptr_t)io->tab_s; in_n[n_in++] = 1024;
    four |= (uintptr_t)io->anchors | (uintptr_t)io->tab_c | (uintptr_t)io->tab_s;
    align |= (uintptr_t)io->anchors;
  } else {
    in_p[n_in] = (uintptr_t)io->boxes; in_n[n_in++] = nms_boxes_extent(d);
    four |= (uintptr_t)io->boxes;
    align |= (uintptr_t)io->boxes;
  }
  if (reads_idx) {
    in_p[n_in] = (uintptr_t)io->idx; in_n[n_in++] = nms_idx_extent(d);
    four |= (uintptr_t)io->idx;
    align |= (uintptr_t)io->idx;
  }
  if (io->count_in) {
    in_p[n_in] = (uintptr_t)io->count_in; in_n[n_in++] = (unsigned long long)d.bs * 4;
    four |= (uintptr_t)io->count_in;
  }
  out_p[n_out] = (uintptr_t)io->keep; out_n[n_out++] = nms_keep_extent(d);
  out_p[n_out] = (uintptr_t)io->count; out_n[n_out++] = (unsigned long long)d.bs * 4;
  if (io->boxes_out) { out_p[n_out] = (uintptr_t)io->boxes_out; out_n[n_out++] = nms_boxes_out_extent(d); }
  four |= (uintptr_t)io->keep | (uintptr_t)io->count | (uintptr_t)io->boxes_out;
  align |= (uintptr_t)io->keep | (uintptr_t)io->count | (uintptr_t)io->boxes_out;
  if (four % 4) return fail(DFX_ERR_INVALID, "nms_submit: a pointer to 4-byte elements is not 4-byte aligned");
  for (int o = 0; o < n_out; ++o) {
    for (int i = 0; i < n_in; ++i)
      if (plan_overlap(out_p[o], out_n[o], in_p[i], in_n[i])) return fail(DFX_ERR_INVALID, "nms_submit: an output overlaps an input");
    for (int p = o + 1; p < n_out; ++p)
      if (plan_overlap(out_p[o], out_n[o], out_p[p], out_n[p])) return fail(DFX_ERR_INVALID, "nms_submit: two outputs overlap");
  }
  DeviceGuard dg(h->device);
  const hipStream_t st = (hipStream_t)s;
  // 16-byte loads and stores need aligned buffers: others take the generic kernel for this submit, as in dfx_select
  const int path = align % 16 == 0 ? h->path : DFX_NMS_GENERIC;
  NmsArgs a = h->args;  // per-launch copy
  a.boxes = (const float *)io->boxes;
  a.idx = reads_idx ? (const int *)io->idx : nullptr;
  a.deltas = (const unsigned char *)io->deltas;
  a.anchors = (const float *)io->anchors;
  a.tab_c = (const float *)io->tab_c;
  a.tab_s = (const float *)io->tab_s;
  a.count_in = (const int *)io->count_in;
  a.keep = (int *)io->keep;
  a.count = (int *)io->count;
  a.boxes_out = (float *)io->boxes_out;
  const int image_grid = nms_image_grid(d.bs);
  if (path == DFX_NMS_GENERIC) {  // one launch, nothing of the handle's: independent of every other submit
    launch_nms_generic(a, image_grid, st);
    HIP_TRY(hipGetLastError());
    g_launches.hit(DFX_NMS_GENERIC);
    return DFX_OK;
  }
  // three launches through the handle's scratch: serialised (dfx.h; TwoLaunchOrder in dfx_internal.h)
  std::lock_guard<std::mutex> lk(h->order.mu);
  int rc = h->order.enter(st);
  if (rc) return rc;
  launch_nms_prep(a, nms_prep_grid(d.bs, d.n), st);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) {
    launch_nms_mask(a, nms_mask_grid(d.bs, d.n), st);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    launch_nms_scan(a, image_grid, st);
    e = hipGetLastError();
  }
  // (once a launch is out the scratch has a writer in flight: every way out goes through leave())
  rc = h->order.leave(st);
  if (e != hipSuccess) return fail(DFX_ERR_HIP, "nms_submit: %s", hipGetErrorString(e));
  if (rc == DFX_OK) g_launches.hit(DFX_NMS_MASK);
  return rc;
}

// test hook: how many submits have run on each path so far (shows the per-submit fallback, which query cannot)
int dfx_debug_nms_launches(int64_t out[2]) { return g_launches.read("nms", out); }

int dfx_nms_query(const dfx_nms_t *h, dfx_nms_info *info) {
  if (const int rc = open_query("nms", h, info)) return rc;
  const bool mask = h->path == DFX_NMS_MASK;
  const dfx_nms_desc &d = h->d;
  info->tiles = mask ? nms_tiles(d.n) : 0;
  info->grid_prep = mask ? nms_prep_grid(d.bs, d.n) : 0;
  info->grid_mask = mask ? nms_mask_grid(d.bs, d.n) : 0;
  info->grid_scan = nms_image_grid(d.bs);
  info->block_prep = mask ? NMS_PREP_THREADS : 0;
  info->block_mask = mask ? NMS_MASK_THREADS : 0;
  info->block_scan = mask ? NMS_SCAN_THREADS : NMS_GENERIC_THREADS;
  info->lds_bytes = nms_lds_bytes(h->path);
  info->launches = nms_launches(h->path);
  info->scratch_bytes = mask ? h->layout.bytes : 0;
  info->algorithmic_bytes = nms_algorithmic_bytes(d);
  return DFX_OK;
}

int dfx_nms_destroy(dfx_nms_t *h) {
  release(h);
  return DFX_OK;
}

}  // extern "C"
