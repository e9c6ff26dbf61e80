// wsum_api.hip -- host side of the scaled element-wise sum (dfx_wsum_* of include/dfx.h): descriptor validation, the
// device image of the per-channel constants and the table, the aliasing check and the choice of the kernel per submit
// (all planned in wsum_plan.h), launches.  The kernels are in wsum.cuh.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "path_op.h"
#include "wsum.cuh"
#include "wsum_plan.h"

namespace dfx {
int launch_wsum_generic(const WsumArgs &a, int grid, hipStream_t s);
int launch_wsum_vec(const WsumArgs &a, int grid, hipStream_t s);
}
using namespace dfx;

struct dfx_wsum {
  dfx_wsum_desc d;
  int device = 0;
  int path = DFX_WSUM_GENERIC;
  WsumArgs args = {};              // without the buffer pointers and `total`; written by create and set_params only
  WsumImage img = {};
  int vec_grid = 0, generic_grid = 0;
  unsigned char *d_image = nullptr;
  bool params_set = false;
  HostStaging host;                // dfx_wsum_submit_host
  char kernel_name[96] = "";
};

namespace {

void release(dfx_wsum *h) {
  if (!h) return;
  DeviceGuard dg(h->device);
  (void)hipFree(h->d_image);
  h->host.release();
  delete h;
}

// launches since the library was loaded, by the kernel that ran ([DFX_WSUM_VEC], [DFX_WSUM_GENERIC]); process-wide,
// because submit does not write to the handle (dfx_debug_wsum_launches)
LaunchCounts<2> g_launches;

size_t tensor_bytes(const dfx_wsum_desc &d, int dt) { return (size_t)wsum_elems(d) * dt_size(dt); }

}  // namespace

extern "C" {

int dfx_wsum_create(const dfx_wsum_desc *desc, dfx_wsum_t **out) {
  dfx_wsum *h = nullptr;
  const int rc = open_create("wsum", desc, out, &h, [](const dfx_wsum_desc &d) {
    if (const int bad = validated("wsum", wsum_validate, d)) return bad;
    if (d.force_path == DFX_WSUM_VEC && !wsum_vec_class(d))
      return fail(DFX_ERR_UNSUPPORTED,
                  "wsum_create: shape outside the vec kernel's class (c a multiple of 16; per-channel constants and table within 64 KiB)");
    return (int)DFX_OK;
  });
  if (rc) return rc;
  const dfx_wsum_desc &d = *desc;
  for (int i = d.n_inputs; i < DFX_WSUM_MAX_INPUTS; ++i) h->d.src_dt[i] = h->d.nscales[i] = 0;
  // AUTO RULE (include/dfx.h DFX_WSUM_AUTO_NOTE)
  h->path = wsum_path(d);
  h->img = wsum_image(d);
  if (h->img.bytes) {
    const hipError_t e = hipMalloc((void **)&h->d_image, (size_t)h->img.bytes);
    if (e != hipSuccess) {
      release(h);
      return fail(DFX_ERR_HIP, "wsum_create: constants: %s", hipGetErrorString(e));
    }
  }
  WsumArgs &a = h->args;
  a.image = h->d_image;
  for (int i = 0; i < DFX_WSUM_MAX_INPUTS; ++i) {
    a.dt[i] = h->d.src_dt[i];
    a.slot[i] = h->img.slot[i];
  }
  a.bias_slot = h->img.bias_slot;
  a.has_bias = d.n_bias != 0;
  a.n = d.n_inputs; a.c = d.c; a.groups = d.c / 16;
  a.relu = d.post_relu; a.rm = d.round_mode; a.dst_dt = d.dst_dt; a.lut_in_dt = d.lut_in_dt;
  a.image_bytes = (int)h->img.bytes;
  a.lut_off = h->img.lut_off < 0 ? 0 : (int)h->img.lut_off;
  const long long cap = grid_cap("DFX_WSUM_GRID");
  h->generic_grid = wsum_grid(wsum_items(d, DFX_WSUM_GENERIC), cap);
  if (h->path == DFX_WSUM_VEC) h->vec_grid = wsum_grid(wsum_items(d, DFX_WSUM_VEC), cap);

  std::string name = h->path == DFX_WSUM_VEC ? "wsum_vec<" : "wsum_generic<";
  name += "n" + std::to_string(d.n_inputs) + ":";
  for (int i = 0; i < d.n_inputs; ++i) name += std::string(i ? "," : "") + dt_name(d.src_dt[i]);
  name += std::string("->") + dt_name(d.dst_dt);
  if (d.n_bias) name += ",bias";
  if (d.post_relu) name += ",relu";
  if (d.lut_in_dt != DFX_UNDEF) name += std::string(",lut_") + dt_name(d.lut_in_dt);
  if (d.round_mode == DFX_ROUND_DOWN && (d.dst_dt != DFX_F32)) name += ",down";
  name += ">";
  snprintf(h->kernel_name, sizeof(h->kernel_name), "%s", name.c_str());
  *out = h;
  return DFX_OK;
}

int dfx_wsum_set_params(dfx_wsum_t *h, const float *const *scales, const float *bias, const uint8_t *lut) {
  if (!h || !scales) return fail(DFX_ERR_INVALID, "wsum_set_params: null argument");
  const dfx_wsum_desc &d = h->d;
  for (int i = 0; i < d.n_inputs; ++i) {
    if (!scales[i]) return fail(DFX_ERR_INVALID, "wsum_set_params: null scales of input %d", i);
    for (int k = 0; k < d.nscales[i]; ++k)
      if (!std::isfinite(scales[i][k])) return fail(DFX_ERR_INVALID, "wsum_set_params: a scale of input %d is not finite", i);
  }
  if (d.n_bias && !bias) return fail(DFX_ERR_INVALID, "wsum_set_params: null bias");
  for (int k = 0; k < d.n_bias; ++k)
    if (!std::isfinite(bias[k])) return fail(DFX_ERR_INVALID, "wsum_set_params: a bias value is not finite");
  if (d.lut_in_dt != DFX_UNDEF && !lut) return fail(DFX_ERR_INVALID, "wsum_set_params: null table");
  std::vector<unsigned char> img((size_t)h->img.bytes, 0);
  float *f = reinterpret_cast<float *>(img.data());
  for (int i = 0; i < d.n_inputs; ++i) {
    if (h->img.slot[i] >= 0) memcpy(f + (size_t)h->img.slot[i] * d.c, scales[i], (size_t)d.c * 4);
    h->args.s1[i] = scales[i][0];
  }
  if (h->img.bias_slot >= 0) memcpy(f + (size_t)h->img.bias_slot * d.c, bias, (size_t)d.c * 4);
  h->args.b1 = d.n_bias ? bias[0] : 0.0f;
  if (h->img.lut_off >= 0) memcpy(img.data() + h->img.lut_off, lut, 256);
  if (h->img.bytes) {
    DeviceGuard dg(h->device);
    HIP_TRY(hipMemcpy(h->d_image, img.data(), img.size(), hipMemcpyHostToDevice));
  }
  h->params_set = true;
  return DFX_OK;
}

int dfx_wsum_submit(dfx_wsum_t *h, const void *const *srcs_dev, void *dst_dev, dfx_stream_t s) {
  if (!h || !srcs_dev || !dst_dev) return fail(DFX_ERR_INVALID, "wsum_submit: null argument");
  const dfx_wsum_desc &d = h->d;
  if (!h->params_set) return fail(DFX_ERR_STATE, "wsum_submit: dfx_wsum_set_params not called");
  uintptr_t src[DFX_WSUM_MAX_INPUTS], all = (uintptr_t)dst_dev;
  if ((uintptr_t)dst_dev % dt_size(d.dst_dt)) return fail(DFX_ERR_INVALID, "wsum_submit: dst not aligned to its element");
  for (int i = 0; i < d.n_inputs; ++i) {
    if (!srcs_dev[i]) return fail(DFX_ERR_INVALID, "wsum_submit: input %d is null", i);
    src[i] = (uintptr_t)srcs_dev[i];
    if (src[i] % dt_size(d.src_dt[i])) return fail(DFX_ERR_INVALID, "wsum_submit: input %d not aligned to its element", i);
    all |= src[i];
  }
  // a lane reads an element of every input before it writes that element: dst may BE an input of its own element size
  if (wsum_alias(d.n_inputs, src, d.src_dt, (uintptr_t)dst_dev, d.dst_dt, (unsigned long long)wsum_elems(d)) == WSUM_ALIAS_REFUSED)
    return fail(DFX_ERR_INVALID, "wsum_submit: dst overlaps an input without being an input of its own element size");
  DeviceGuard dg(h->device);
  // 16-byte accesses need aligned buffers: others take the per-element kernel for this submit, as resize does
  const bool vec = h->path == DFX_WSUM_VEC && all % 16 == 0;
  WsumArgs a = h->args;  // per-launch copy: concurrent submits on several streams are independent
  for (int i = 0; i < d.n_inputs; ++i) a.src[i] = (const unsigned char *)srcs_dev[i];
  a.dst = (unsigned char *)dst_dev;
  a.total = wsum_items(d, vec ? DFX_WSUM_VEC : DFX_WSUM_GENERIC);
  const int rc = vec ? launch_wsum_vec(a, h->vec_grid, (hipStream_t)s) : launch_wsum_generic(a, h->generic_grid, (hipStream_t)s);
  return g_launches.launched("wsum", rc, vec ? DFX_WSUM_VEC : DFX_WSUM_GENERIC);
}

// test hook: how many submits have launched each kernel so far (shows the per-submit fallback, which query cannot)
int dfx_debug_wsum_launches(int64_t out[2]) { return g_launches.read("wsum", out); }

int dfx_wsum_submit_host(dfx_wsum_t *h, const void *const *srcs_host, void *dst_host) {
  if (!h || !srcs_host || !dst_host) return fail(DFX_ERR_INVALID, "wsum_submit_host: null argument");
  if (!h->params_set) return fail(DFX_ERR_STATE, "wsum_submit_host: dfx_wsum_set_params not called");
  size_t bytes[DFX_WSUM_MAX_INPUTS];
  for (int i = 0; i < h->d.n_inputs; ++i) {
    if (!srcs_host[i]) return fail(DFX_ERR_INVALID, "wsum_submit_host: input %d is null", i);
    bytes[i] = tensor_bytes(h->d, h->d.src_dt[i]);
  }
  DeviceGuard dg(h->device);
  return h->host.run(h->d.n_inputs, srcs_host, bytes, dst_host, tensor_bytes(h->d, h->d.dst_dt),
                     [h](const void *const *sv, void *dv, dfx_stream_t st) { return dfx_wsum_submit(h, sv, dv, st); });
}

int dfx_wsum_query(const dfx_wsum_t *h, dfx_wsum_info *info) {
  if (const int rc = open_query("wsum", h, info)) return rc;
  const bool vec = h->path == DFX_WSUM_VEC;
  info->grid = vec ? h->vec_grid : h->generic_grid;
  info->block = WSUM_THREADS;
  info->lds_bytes = vec ? (int)h->img.bytes : 0;
  uint64_t bytes = tensor_bytes(h->d, h->d.dst_dt);
  for (int i = 0; i < h->d.n_inputs; ++i) bytes += tensor_bytes(h->d, h->d.src_dt[i]);
  info->algorithmic_bytes = bytes;
  return DFX_OK;
}

int dfx_wsum_destroy(dfx_wsum_t *h) {
  release(h);
  return DFX_OK;
}

}  // extern "C"
