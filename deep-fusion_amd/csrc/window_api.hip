// window_api.hip -- host side of the window partition / reverse op (dfx_window_* of include/dfx.h): descriptor validation,
// the row map and its device image, the overlap check and the choice of the kernel per submit (all planned in
// window_plan.h), launches.  The kernels are in window.cuh.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>
#include <vector>

#include "path_op.h"
#include "window.cuh"
#include "window_plan.h"

namespace dfx {
int launch_window(const WindowArgs &a, int path, int grid, hipStream_t s);
}
using namespace dfx;

struct dfx_window {
  dfx_window_desc d;
  int device = 0;
  int path = DFX_WINDOW_GENERIC;
  int grid[2] = {0, 0};              // per path; [path] and [DFX_WINDOW_GENERIC] (the per-submit fallback) are used
  int *d_map = nullptr;              // window_build_map's table: one entry per destination row of an image
  char kernel_name[96] = "";
};

namespace {

void release(dfx_window *h) {
  if (!h) return;
  DeviceGuard dg(h->device);
  (void)hipFree(h->d_map);
  delete h;
}

// launches since the library was loaded, by the kernel that ran; process-wide, because submit does not write to the
// handle (dfx_debug_window_launches)
LaunchCounts<2> g_launches;

void set_name(dfx_window *h) {
  const dfx_window_desc &d = h->d;
  std::string name = h->path == DFX_WINDOW_ROW ? "window_row<" : "window_generic<";
  name += d.dir == DFX_WINDOW_PARTITION ? "partition," : "reverse,";
  name += dt_name(d.dt);
  if (h->path == DFX_WINDOW_ROW) name += ",l" + std::to_string(window_lanes(d));
  name += ">";
  snprintf(h->kernel_name, sizeof(h->kernel_name), "%s", name.c_str());
}

}  // namespace

extern "C" {

int dfx_window_create(const dfx_window_desc *desc, dfx_window_t **out) {
  dfx_window *h = nullptr;
  const int rc = open_create("window", desc, out, &h, [](const dfx_window_desc &d) {
    if (const int bad = validated("window", window_validate, d)) return bad;
    if (d.force_path != -1 && !window_in_class(d, d.force_path))
      return fail(DFX_ERR_UNSUPPORTED, "window_create: descriptor outside the forced path's class (row: c, grid_ld and win_ld times the "
                                       "element size multiples of 16)");
    return (int)DFX_OK;
  });
  if (rc) return rc;
  const dfx_window_desc &d = *desc;
  // AUTO RULE (include/dfx.h DFX_WINDOW_AUTO_NOTE)
  h->path = window_path(d);
  std::vector<int32_t> map;
  window_build_map(d, map);
  hipError_t e = hipMalloc((void **)&h->d_map, map.size() * sizeof(int32_t));
  if (e == hipSuccess) e = hipMemcpy(h->d_map, map.data(), map.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    release(h);
    return fail(DFX_ERR_HIP, "window_create: row map: %s", hipGetErrorString(e));
  }
  const long long cap = grid_cap("DFX_WINDOW_GRID");
  h->grid[h->path] = window_grid(d, h->path, cap);
  h->grid[DFX_WINDOW_GENERIC] = window_grid(d, DFX_WINDOW_GENERIC, cap);
  set_name(h);
  *out = h;
  return DFX_OK;
}

int dfx_window_submit(dfx_window_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s) {
  if (!h || !src_dev || !dst_dev) return fail(DFX_ERR_INVALID, "window_submit: null argument");
  const dfx_window_desc &d = h->d;
  const int es = plan_dt_size(d.dt);
  const uintptr_t src = (uintptr_t)src_dev, dst = (uintptr_t)dst_dev;
  if ((src | dst) % es) return fail(DFX_ERR_INVALID, "window_submit: a 4-byte tensor is not 4-byte aligned");
  if (plan_overlap(src, window_src_extent(d), dst, window_dst_extent(d)))
    return fail(DFX_ERR_INVALID, "window_submit: dst overlaps src (a permutation cannot run in place)");
  DeviceGuard dg(h->device);
  // 16-byte loads and stores need aligned buffers: others take the generic kernel for this submit, as lnorm does
  const int path = (src | dst) % 16 == 0 ? h->path : DFX_WINDOW_GENERIC;
  WindowArgs a = {};  // per launch: concurrent submits on several streams are independent
  a.src = (const unsigned char *)src_dev;
  a.dst = (unsigned char *)dst_dev;
  a.map = h->d_map;
  a.rows = (long long)d.bs * window_dst_rows(d);
  a.src_img = window_src_rows(d);
  a.src_pitch = window_src_ld(d) * es;
  a.dst_pitch = window_dst_ld(d) * es;
  a.dst_img = (int)window_dst_rows(d);
  a.c = d.c;
  a.esize = es;
  a.lanes = path == DFX_WINDOW_ROW ? (int)window_lanes(d) : 0;
  a.pad = es == 1 ? (d.pad_value & 0xffu) * 0x01010101u : d.pad_value;
  return g_launches.launched("window", launch_window(a, path, h->grid[path], (hipStream_t)s), path);
}

// test hook: how many submits have launched each kernel so far (shows the per-submit fallback, which query cannot)
int dfx_debug_window_launches(int64_t out[2]) { return g_launches.read("window", out); }

int dfx_window_query(const dfx_window_t *h, dfx_window_info *info) {
  if (const int rc = open_query("window", h, info)) return rc;
  info->grid = h->grid[h->path];
  info->block = WINDOW_THREADS;
  info->algorithmic_bytes = window_algorithmic_bytes(h->d);
  return DFX_OK;
}

int dfx_window_destroy(dfx_window_t *h) {
  release(h);
  return DFX_OK;
}

}  // extern "C"
