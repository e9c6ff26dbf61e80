// head_api.hip -- host side of the net head (dfx_head_* of include/dfx.h: channel top-k / argmax and softmax over a row
// matrix): descriptor validation, the device copy of the softmax table, the overlap check and the choice of the kernel
// per submit (all planned in head_plan.h), launches.  The kernels are in head.cuh.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>

#include "path_op.h"
#include "head.cuh"
#include "head_plan.h"

namespace dfx {
int launch_head(const HeadArgs &a, int path, bool softmax, int grid, hipStream_t s);
}
using namespace dfx;

struct dfx_head {
  dfx_head_desc d;
  int device = 0;
  int path = DFX_HEAD_GENERIC;
  int grid[3] = {0, 0, 0};           // per path; [path] and [DFX_HEAD_GENERIC] (the per-submit fallback) are used
  unsigned int *d_table = nullptr;   // SOFTMAX: 256 entries
  bool table_set = false;
  char kernel_name[96] = "";
};

namespace {

void release(dfx_head *h) {
  if (!h) return;
  DeviceGuard dg(h->device);
  (void)hipFree(h->d_table);
  delete h;
}

// launches since the library was loaded, by the kernel that ran; process-wide, because submit does not write to the
// handle (dfx_debug_head_launches)
LaunchCounts<3> g_launches;

}  // namespace

extern "C" {

int dfx_head_create(const dfx_head_desc *desc, dfx_head_t **out) {
  dfx_head *h = nullptr;
  const int rc = open_create("head", desc, out, &h, [](const dfx_head_desc &d) {
    if (const int bad = validated("head", head_validate, d)) return bad;
    if (d.force_path != -1 && !head_in_class(d, d.force_path))
      return fail(DFX_ERR_UNSUPPORTED, "head_create: descriptor outside the forced path's class (pixel: 1-byte src, k = 1 or softmax, "
                                       "src_ld a multiple of 16 up to 160; row: src_ld * element size a multiple of 16)");
    return (int)DFX_OK;
  });
  if (rc) return rc;
  const dfx_head_desc &d = *desc;
  // AUTO RULE (include/dfx.h DFX_HEAD_AUTO_NOTE)
  h->path = head_path(d);
  if (d.mode == DFX_HEAD_SOFTMAX) {
    const hipError_t e = hipMalloc((void **)&h->d_table, HEAD_TABLE_BYTES);
    if (e != hipSuccess) {
      release(h);
      return fail(DFX_ERR_HIP, "head_create: table: %s", hipGetErrorString(e));
    }
  }
  const long long cap = grid_cap("DFX_HEAD_GRID");
  h->grid[h->path] = head_grid(d.rows, h->path, cap);
  h->grid[DFX_HEAD_GENERIC] = head_grid(d.rows, DFX_HEAD_GENERIC, cap);
  std::string name = h->path == DFX_HEAD_PIXEL ? "head_pixel<" : h->path == DFX_HEAD_ROW ? "head_row<" : "head_generic<";
  name += d.mode == DFX_HEAD_SOFTMAX ? std::string("softmax") : "topk" + std::to_string(d.k);
  name += std::string(",") + dt_name(d.src_dt) + "->" + dt_name(d.dst_dt) + ">";
  snprintf(h->kernel_name, sizeof(h->kernel_name), "%s", name.c_str());
  *out = h;
  return DFX_OK;
}

int dfx_head_set_table(dfx_head_t *h, const uint32_t *table256) {
  if (!h || !table256) return fail(DFX_ERR_INVALID, "head_set_table: null argument");
  if (h->d.mode != DFX_HEAD_SOFTMAX) return fail(DFX_ERR_INVALID, "head_set_table: not a softmax handle");
  const char *why = "";
  const int rc = head_table_ok(table256, h->d.c, &why);
  if (rc) return fail(rc, "head_set_table: %s", why);
  DeviceGuard dg(h->device);
  HIP_TRY(hipMemcpy(h->d_table, table256, HEAD_TABLE_BYTES, hipMemcpyHostToDevice));
  h->table_set = true;
  return DFX_OK;
}

int dfx_head_submit(dfx_head_t *h, const void *src_dev, void *idx_or_dst_dev, void *val_or_null_dev, dfx_stream_t s) {
  if (!h || !src_dev || !idx_or_dst_dev) return fail(DFX_ERR_INVALID, "head_submit: null argument");
  const dfx_head_desc &d = h->d;
  const bool softmax = d.mode == DFX_HEAD_SOFTMAX;
  if (softmax && !h->table_set) return fail(DFX_ERR_STATE, "head_submit: dfx_head_set_table not called");
  if (softmax && val_or_null_dev) return fail(DFX_ERR_INVALID, "head_submit: a softmax has no val");
  const int ssz = plan_dt_size(d.src_dt), osz = plan_dt_size(d.dst_dt);
  const uintptr_t src = (uintptr_t)src_dev, out = (uintptr_t)idx_or_dst_dev, val = (uintptr_t)val_or_null_dev;
  if (src % ssz || out % osz || val % ssz) return fail(DFX_ERR_INVALID, "head_submit: a pointer is not aligned to its element");
  const unsigned long long sbytes = plan_extent(d.rows, d.src_ld, d.c, ssz);
  const unsigned long long obytes = plan_extent(d.rows, head_out_ld(d), head_out_cols(d), osz);
  const unsigned long long vbytes = val ? plan_extent(d.rows, d.idx_ld, d.k, ssz) : 0;
  if (plan_overlap(src, sbytes, out, obytes) || (val && (plan_overlap(src, sbytes, val, vbytes) || plan_overlap(out, obytes, val, vbytes))))
    return fail(DFX_ERR_INVALID, "head_submit: an output overlaps src or the other output");
  DeviceGuard dg(h->device);
  // 16-byte loads need aligned buffers: others take the generic kernel for this submit, as wsum does
  const int path = (src | out | val) % 16 == 0 ? h->path : DFX_HEAD_GENERIC;
  HeadArgs a = {};  // per launch: concurrent submits on several streams are independent
  a.src = (const unsigned char *)src_dev;
  a.out = (unsigned char *)idx_or_dst_dev;
  a.val = (unsigned char *)val_or_null_dev;
  a.table = h->d_table;
  a.rows = d.rows;
  a.c = d.c; a.src_ld = d.src_ld; a.out_ld = head_out_ld(d); a.k = softmax ? 0 : d.k;
  a.src_dt = d.src_dt; a.out_dt = d.dst_dt;
  a.out_vec = softmax && out % 16 == 0 && ((long long)d.dst_ld * osz) % 16 == 0;
  a.out_scale = d.out_scale;
  return g_launches.launched("head", launch_head(a, path, softmax, h->grid[path], (hipStream_t)s), path);
}

// test hook: how many submits have launched each kernel so far (shows the per-submit fallback, which query cannot)
int dfx_debug_head_launches(int64_t out[3]) { return g_launches.read("head", out); }

int dfx_head_query(const dfx_head_t *h, dfx_head_info *info) {
  if (const int rc = open_query("head", h, info)) return rc;
  info->grid = h->grid[h->path];
  info->block = HEAD_THREADS;
  info->lds_bytes = head_lds_bytes(h->d, h->path);
  info->algorithmic_bytes = head_algorithmic_bytes(h->d);
  return DFX_OK;
}

int dfx_head_destroy(dfx_head_t *h) {
  release(h);
  return DFX_OK;
}

}  // extern "C"
