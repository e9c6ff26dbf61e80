// lnorm_api.hip -- host side of the int8 layer norm / RMS norm (dfx_lnorm_* of include/dfx.h): descriptor validation, the
// device image of gamma / beta / shift, the overlap check and the choice of the kernel per submit (all planned in
// lnorm_plan.h), launches.  The kernels are in lnorm.cuh.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "path_op.h"
#include "lnorm.cuh"
#include "lnorm_plan.h"

namespace dfx {
int launch_lnorm(const LnormArgs &a, int path, int lanes, int grid, int lds, hipStream_t s);
}
using namespace dfx;

struct dfx_lnorm {
  dfx_lnorm_desc d;
  int device = 0;
  int path = DFX_LNORM_GENERIC;
  int lanes = 0;                     // row kernel: lanes per row
  int grid[2] = {0, 0};              // per path; [path] and [DFX_LNORM_GENERIC] (the per-submit fallback) are used
  unsigned char *d_params = nullptr; // gamma | beta | shift, whole 16-channel groups (lnorm_param_bytes)
  bool params_set = false, has_shift = false;
  char kernel_name[96] = "";
};

namespace {

void release(dfx_lnorm *h) {
  if (!h) return;
  DeviceGuard dg(h->device);
  (void)hipFree(h->d_params);
  delete h;
}

// launches since the library was loaded, by the kernel that ran; process-wide, because submit does not write to the
// handle (dfx_debug_lnorm_launches)
LaunchCounts<2> g_launches;

void set_name(dfx_lnorm *h) {
  const dfx_lnorm_desc &d = h->d;
  std::string name = h->path == DFX_LNORM_ROW ? "lnorm_row<" : "lnorm_generic<";
  name += d.mode == DFX_LNORM_LAYER ? "layer," : "rms,";
  name += std::string(dt_name(d.src_dt)) + "->" + dt_name(d.dst_dt);
  if (h->path == DFX_LNORM_ROW) name += ",w" + std::to_string(h->lanes);
  if (h->has_shift) name += ",shift";
  name += ">";
  snprintf(h->kernel_name, sizeof(h->kernel_name), "%s", name.c_str());
}

}  // namespace

extern "C" {

int dfx_lnorm_create(const dfx_lnorm_desc *desc, dfx_lnorm_t **out) {
  dfx_lnorm *h = nullptr;
  const int rc = open_create("lnorm", desc, out, &h, [](const dfx_lnorm_desc &d) {
    if (const int bad = validated("lnorm", lnorm_validate, d)) return bad;
    if (d.force_path != -1 && !lnorm_in_class(d, d.force_path))
      return fail(DFX_ERR_UNSUPPORTED, "lnorm_create: descriptor outside the forced path's class (row: src_ld and dst_ld * element size "
                                       "multiples of 16)");
    return (int)DFX_OK;
  });
  if (rc) return rc;
  const dfx_lnorm_desc &d = *desc;
  // AUTO RULE (include/dfx.h DFX_LNORM_AUTO_NOTE)
  h->path = lnorm_path(d);
  h->lanes = lnorm_lanes(d.c);
  const hipError_t e = hipMalloc((void **)&h->d_params, lnorm_param_bytes(d.c));
  if (e != hipSuccess) {
    release(h);
    return fail(DFX_ERR_HIP, "lnorm_create: parameters: %s", hipGetErrorString(e));
  }
  const long long cap = grid_cap("DFX_LNORM_GRID");
  h->grid[h->path] = lnorm_grid(d.rows, d.c, h->path, cap);
  h->grid[DFX_LNORM_GENERIC] = lnorm_grid(d.rows, d.c, DFX_LNORM_GENERIC, cap);
  set_name(h);
  *out = h;
  return DFX_OK;
}

int dfx_lnorm_set_params(dfx_lnorm_t *h, const float *gamma, const float *beta_or_null, const uint8_t *shift_or_null) {
  if (!h || !gamma) return fail(DFX_ERR_INVALID, "lnorm_set_params: null argument");
  const int c = h->d.c, cp = plan_up16(c);
  if (shift_or_null)
    for (int k = 0; k < c; ++k)
      if (shift_or_null[k] > DFX_LNORM_MAX_SHIFT) return fail(DFX_ERR_INVALID, "lnorm_set_params: shift[%d] = %d is above 7", k, (int)shift_or_null[k]);
  std::vector<unsigned char> image(lnorm_param_bytes(c), 0);
  memcpy(image.data(), gamma, (size_t)c * 4);
  if (beta_or_null) memcpy(image.data() + (size_t)cp * 4, beta_or_null, (size_t)c * 4);
  if (shift_or_null) memcpy(image.data() + (size_t)cp * 8, shift_or_null, (size_t)c);
  DeviceGuard dg(h->device);
  HIP_TRY(hipMemcpy(h->d_params, image.data(), image.size(), hipMemcpyHostToDevice));
  h->has_shift = shift_or_null != nullptr;
  h->params_set = true;
  set_name(h);
  return DFX_OK;
}

int dfx_lnorm_submit(dfx_lnorm_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s) {
  if (!h || !src_dev || !dst_dev) return fail(DFX_ERR_INVALID, "lnorm_submit: null argument");
  const dfx_lnorm_desc &d = h->d;
  if (!h->params_set) return fail(DFX_ERR_STATE, "lnorm_submit: dfx_lnorm_set_params not called");
  const int osz = plan_dt_size(d.dst_dt);
  const uintptr_t src = (uintptr_t)src_dev, dst = (uintptr_t)dst_dev;
  if (dst % osz) return fail(DFX_ERR_INVALID, "lnorm_submit: an f32 dst is not 4-byte aligned");
  if (plan_overlap(src, plan_extent(d.rows, d.src_ld, d.c, 1), dst, plan_extent(d.rows, d.dst_ld, d.c, osz)))
    return fail(DFX_ERR_INVALID, "lnorm_submit: dst overlaps src (in place is not built)");
  DeviceGuard dg(h->device);
  // 16-byte loads and stores need aligned buffers: others take the generic kernel for this submit, as head does
  const int path = (src | dst) % 16 == 0 ? h->path : DFX_LNORM_GENERIC;
  const int cp = plan_up16(d.c);
  LnormArgs a = {};  // per launch: concurrent submits on several streams are independent
  a.src = (const unsigned char *)src_dev;
  a.dst = (unsigned char *)dst_dev;
  a.gamma = reinterpret_cast<const float *>(h->d_params);
  a.beta = a.gamma + cp;
  a.shift = h->has_shift ? h->d_params + (size_t)cp * 8 : nullptr;
  a.rows = d.rows;
  a.c = d.c; a.src_ld = d.src_ld; a.dst_ld = d.dst_ld;
  a.mode = d.mode; a.src_dt = d.src_dt; a.dst_dt = d.dst_dt;
  const int lds = lnorm_lds_bytes(d, path);
  a.stage = lds > 0;
  a.eps = d.eps;
  return g_launches.launched("lnorm", launch_lnorm(a, path, h->lanes, h->grid[path], lds, (hipStream_t)s), path);
}

// test hook: how many submits have launched each kernel so far (shows the per-submit fallback, which query cannot)
int dfx_debug_lnorm_launches(int64_t out[2]) { return g_launches.read("lnorm", out); }

int dfx_lnorm_query(const dfx_lnorm_t *h, dfx_lnorm_info *info) {
  if (const int rc = open_query("lnorm", h, info)) return rc;
  info->grid = h->grid[h->path];
  info->block = LNORM_THREADS;
  info->lds_bytes = lnorm_lds_bytes(h->d, h->path);
  info->algorithmic_bytes = lnorm_algorithmic_bytes(h->d, h->has_shift);
  return DFX_OK;
}

int dfx_lnorm_destroy(dfx_lnorm_t *h) {
  release(h);
  return DFX_OK;
}

}  // extern "C"
