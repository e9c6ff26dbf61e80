// head_api.hip -- host side of the net head (dfx_head_* of include/dfx.h: channel top-k / argmax and softmax over a row
// matrix): descriptor validation, the device copy of the softmax table, the overlap check and the choice of the kernel
// per submit (all planned in head_plan.h), launches.  The kernels are in head.cuh.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>

#include "dfx_internal.h"
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

// launches since the library was loaded, by the kernel that ran; process-wide, because submit does not write to the
// handle (dfx_debug_head_launches)
std::atomic<long long> g_launches[3];

const char *dt_name(int dt) { return dt == DFX_F32 ? "f32" : dt == DFX_S32 ? "s32" : dt == DFX_S8 ? "s8" : "u8"; }

long long grid_cap() {
  const char *e = tuning_value("DFX_HEAD_GRID");  // testing aid
  return e ? std::max(1ll, atoll(e)) : 0;
}

}  // namespace

extern "C" {

int dfx_head_create(const dfx_head_desc *desc, dfx_head_t **out) {
  if (!desc || !out) return fail(DFX_ERR_INVALID, "head_create: null argument");
  *out = nullptr;
  const dfx_head_desc &d = *desc;
  const char *why = "";
  int rc = head_validate(d, &why);
  if (rc) return fail(rc, "head: %s", why);
  if (d.force_path != -1 && !head_in_class(d, d.force_path))
    return fail(DFX_ERR_UNSUPPORTED, "head_create: descriptor outside the forced path's class (pixel: 1-byte src, k = 1 or softmax, "
                                     "src_ld a multiple of 16 up to 160; row: src_ld * element size a multiple of 16)");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(DFX_ERR_NO_DEVICE, "head_create: no HIP device (this library has no CPU path)");
  dfx_head *h = new (std::nothrow) dfx_head();
  if (!h) return fail(DFX_ERR_HIP, "out of host memory");
  h->d = d;
  if (hipGetDevice(&h->device) != hipSuccess) h->device = 0;
  // AUTO RULE (include/dfx.h DFX_HEAD_AUTO_NOTE)
  h->path = head_path(d);
  if (d.mode == DFX_HEAD_SOFTMAX) {
    const hipError_t e = hipMalloc((void **)&h->d_table, HEAD_TABLE_BYTES);
    if (e != hipSuccess) {
      delete h;
      return fail(DFX_ERR_HIP, "head_create: table: %s", hipGetErrorString(e));
    }
  }
  const long long cap = grid_cap();
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
  const int ssz = head_dt_size(d.src_dt), osz = head_dt_size(d.dst_dt);
  const uintptr_t src = (uintptr_t)src_dev, out = (uintptr_t)idx_or_dst_dev, val = (uintptr_t)val_or_null_dev;
  if (src % ssz || out % osz || val % ssz) return fail(DFX_ERR_INVALID, "head_submit: a pointer is not aligned to its element");
  const unsigned long long sbytes = head_extent(d.rows, d.src_ld, d.c, ssz);
  const unsigned long long obytes = head_extent(d.rows, head_out_ld(d), head_out_cols(d), osz);
  const unsigned long long vbytes = val ? head_extent(d.rows, d.idx_ld, d.k, ssz) : 0;
  if (head_overlap(src, sbytes, out, obytes) || (val && (head_overlap(src, sbytes, val, vbytes) || head_overlap(out, obytes, val, vbytes))))
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
  if (launch_head(a, path, softmax, h->grid[path], (hipStream_t)s) != 0) return fail(DFX_ERR_UNSUPPORTED, "head_submit: no kernel instance for this op");
  HIP_TRY(hipGetLastError());
  g_launches[path].fetch_add(1, std::memory_order_relaxed);
  return DFX_OK;
}

// test hook: how many submits have launched each kernel so far (shows the per-submit fallback, which query cannot)
int dfx_debug_head_launches(int64_t out[3]) {
  if (!out) return fail(DFX_ERR_INVALID, "debug_head_launches: null argument");
  for (int k = 0; k < 3; ++k) out[k] = g_launches[k].load(std::memory_order_relaxed);
  return DFX_OK;
}

int dfx_head_query(const dfx_head_t *h, dfx_head_info *info) {
  if (!h || !info) return fail(DFX_ERR_INVALID, "head_query: null argument");
  memset(info, 0, sizeof(*info));
  info->path = h->path;
  info->grid = h->grid[h->path];
  info->block = HEAD_THREADS;
  info->lds_bytes = head_lds_bytes(h->d, h->path);
  info->device = h->device;
  info->algorithmic_bytes = head_algorithmic_bytes(h->d);
  memcpy(info->kernel_name, h->kernel_name, sizeof(info->kernel_name));
  return DFX_OK;
}

int dfx_head_destroy(dfx_head_t *h) {
  if (!h) return DFX_OK;
  DeviceGuard dg(h->device);
  (void)hipFree(h->d_table);
  delete h;
  return DFX_OK;
}

}  // extern "C"
