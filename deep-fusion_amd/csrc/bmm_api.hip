// bmm_api.hip -- host side of the batched int8 matrix product (dfx_bmm_* of include/dfx.h): descriptor validation, the
// path and the grids (all planned in bmm_plan.h), the device copy of the scales with the requant route proved from the
// shape, the logit bias's device image (planned in bias_plan.h) and the route proved again with it, the overlap check and the
// choice of the kernel per submit, launches.  The kernels are in bmm.cuh / bmm.hip.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <new>
#include <vector>

#include "path_op.h"
#include "bmm.cuh"
#include "bmm_plan.h"
#include "bias_plan.h"

namespace dfx {
int launch_bmm_mfma(const BmmArgs &a, const BmmBiasArgs *bias, int grid, hipStream_t s, bool fast);
int launch_bmm_generic(const BmmArgs &a, const BmmBiasArgs *bias, int grid, hipStream_t s);
}
using namespace dfx;

struct dfx_bmm {
  dfx_bmm_desc d;
  int device = 0;
  int path = DFX_BMM_GENERIC;
  int grid[2] = {0, 0};        // per path; [path] and [DFX_BMM_GENERIC] (the per-submit fallback) are used
  BmmArgs args = {};           // everything but a / b / c; copied per launch
  float *d_scale = nullptr;    // [n rounded up to 32]
  int n_pad = 0;
  std::atomic<int> scales_set{0};
  int route = 0;               // 0 exact, 1 fast (dfx_debug_conv_requant's numbering); MFMA path only
  std::vector<float> scales;   // the host copy of the last set_scales: set_bias proves the route again from it
  // the logit bias: the device image and the biased kernels' second argument, its layout and what the scan of its entries found
  float *d_bias = nullptr;
  BmmBiasArgs bias_args = {};
  bool bias_set = false;
  dfx_logit_bias_desc bias = {};
  BiasScan bias_scan;
  char kernel_name[96] = "";
};

namespace {

void release(dfx_bmm *h) {
  if (!h) return;
  DeviceGuard dg(h->device);
  (void)hipFree(h->d_scale);
  (void)hipFree(h->d_bias);
  delete h;
}

// launches since the library was loaded, by the kernel that ran; process-wide, because submit does not write to the
// handle (dfx_debug_bmm_launches)
LaunchCounts<2> g_launches;

void set_name(dfx_bmm *h) {
  const dfx_bmm_desc &d = h->d;
  const char *form = d.trans_b ? "nt" : "nn";
  const char *bias = h->bias_set ? " +bias" : "";
  if (h->path == DFX_BMM_MFMA)
    snprintf(h->kernel_name, sizeof(h->kernel_name), "bmm_mfma<%s,%s,%s> %s%s", form, dt_name(d.a_dt), dt_name(d.dst_dt),
             !h->scales_set.load() ? "(no scales)" : h->route ? "fast" : "exact", bias);
  else
    snprintf(h->kernel_name, sizeof(h->kernel_name), "bmm_generic<%s,%s,%s> exact%s", form, dt_name(d.a_dt), dt_name(d.dst_dt), bias);
}

// the requant route from the shape, the scales and the bias as the handle holds them now: whichever setter came last
void prove_route(dfx_bmm *h) {
  if (!h->scales_set.load()) return;
  const bool ok = h->bias_set ? bmm_fast_ok_biased(h->d, h->scales.data(), h->bias_scan) : bmm_fast_ok(h->d, h->scales.data());
  h->route = h->path == DFX_BMM_MFMA && ok && fast_allowed() ? 1 : 0;
}

}  // namespace

extern "C" {

int dfx_bmm_create(const dfx_bmm_desc *desc, dfx_bmm_t **out) {
  dfx_bmm *h = nullptr;
  int cus = 0;
  const int rc = open_create("bmm", desc, out, &h, [](const dfx_bmm_desc &d) { return validated("bmm", bmm_validate, d); }, &cus, release);
  if (rc) return rc;
  const dfx_bmm_desc &d = *desc;
  // AUTO RULE (include/dfx.h DFX_BMM_AUTO_NOTE)
  h->path = bmm_path(d);
  const long long cap = grid_cap("DFX_BMM_GRID");
  h->grid[h->path] = bmm_grid(d, h->path, cus, cap);
  h->grid[DFX_BMM_GENERIC] = bmm_grid(d, DFX_BMM_GENERIC, cus, cap);
  h->n_pad = (int)(((long long)d.n + 31) / 32 * 32);  // (n <= 2^31 - 32: bmm_validate)
  const hipError_t e = hipMalloc((void **)&h->d_scale, (size_t)h->n_pad * sizeof(float));
  if (e != hipSuccess) {
    release(h);
    return fail(DFX_ERR_HIP, "bmm_create: scales: %s", hipGetErrorString(e));
  }
  BmmArgs &a = h->args;
  a.scale = h->d_scale;
  a.a_s0 = d.a_s0; a.a_s1 = d.a_s1; a.lda = d.lda;
  a.b_s0 = d.b_s0; a.b_s1 = d.b_s1; a.ldb = d.ldb;
  a.c_s0 = d.c_s0; a.c_s1 = d.c_s1; a.ldc = d.ldc;
  a.batch0 = d.batch0; a.batch1 = d.batch1; a.m = d.m; a.n = d.n; a.k = d.k;
  a.trans_b = d.trans_b; a.a_u8 = d.a_dt == DFX_U8; a.dst_dt = d.dst_dt;
  a.relu = (d.relu || d.dst_dt == DFX_U8) ? 1 : 0; a.rm = d.round_mode;
  a.mt = (int)bmm_mtiles(d); a.nt = (int)bmm_ntiles(d);
  a.tiles = bmm_tiles(d); a.units = bmm_units(d);
  a.items = bmm_items(d);
  set_name(h);
  *out = h;
  return DFX_OK;
}

int dfx_bmm_set_scales(dfx_bmm_t *h, const float *scales) {
  if (!h || !scales) return fail(DFX_ERR_INVALID, "bmm_set_scales: null argument");
  const dfx_bmm_desc &d = h->d;
  std::vector<float> img((size_t)h->n_pad, 0.0f);  // (the entries n .. n_pad - 1 stay 0)
  for (int i = 0; i < d.n; ++i) img[i] = scales[d.nscales == 1 ? 0 : i];
  DeviceGuard dg(h->device);
  HIP_TRY(hipMemcpy(h->d_scale, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice));
  h->scales.assign(scales, scales + d.nscales);
  h->scales_set.store(1);
  prove_route(h);
  set_name(h);
  return DFX_OK;
}

int dfx_bmm_set_bias(dfx_bmm_t *h, const dfx_logit_bias_desc *desc, const float *host_table) {
  if (!h) return fail(DFX_ERR_INVALID, "bmm_set_bias: null argument");
  DeviceGuard dg(h->device);
  if (!desc) {  // clear: the handle gives its former bits
    (void)hipFree(h->d_bias);
    h->d_bias = nullptr;
    h->bias_set = false;
    h->bias_args = BmmBiasArgs{};
    prove_route(h);
    set_name(h);
    return DFX_OK;
  }
  if (!host_table) return fail(DFX_ERR_INVALID, "bmm_set_bias: null table");
  const dfx_bmm_desc &d = h->d;
  const char *why = "";
  const int rc = bias_validate(d, *desc, &why);
  if (rc) return fail(rc, "bmm_set_bias: %s", why);
  BiasScan scan;
  if (bias_scan(d, *desc, host_table, &scan) != DFX_OK) return fail(DFX_ERR_INVALID, "bmm_set_bias: +inf or NaN in the table (finite values and -inf)");
  std::vector<float> img;
  try {
    img.resize((size_t)bias_image_elems(d, *desc));
  } catch (const std::bad_alloc &) {
    return fail(DFX_ERR_HIP, "out of host memory");
  }
  bias_fill_image(d, *desc, host_table, img.data());
  float *fresh = nullptr;  // the handle keeps its former bias if anything below fails
  hipError_t e = hipMalloc((void **)&fresh, img.size() * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(fresh, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(fresh);
    return fail(DFX_ERR_HIP, "bmm_set_bias: the table's image: %s", hipGetErrorString(e));
  }
  (void)hipFree(h->d_bias);
  h->d_bias = fresh;
  h->bias = *desc;
  h->bias_scan = scan;
  h->bias_set = true;
  h->bias_args = BmmBiasArgs{h->d_bias, desc->period0, desc->period1, (int)bias_rows(d, *desc), (int)bias_cols(d)};
  prove_route(h);
  set_name(h);
  return DFX_OK;
}

int dfx_bmm_submit(dfx_bmm_t *h, const void *a_dev, const void *b_dev, void *c_dev, dfx_stream_t s) {
  if (!h || !a_dev || !b_dev || !c_dev) return fail(DFX_ERR_INVALID, "bmm_submit: null argument");
  if (!h->scales_set.load()) return fail(DFX_ERR_STATE, "bmm_submit: dfx_bmm_set_scales not called");
  const dfx_bmm_desc &d = h->d;
  const unsigned esz = (unsigned)plan_dt_size(d.dst_dt);
  const uintptr_t pa = (uintptr_t)a_dev, pb = (uintptr_t)b_dev, pc = (uintptr_t)c_dev;
  if (pc % esz) return fail(DFX_ERR_INVALID, "bmm_submit: c is not aligned to its element");
  const unsigned long long abytes = bmm_a_elems(d), bbytes = bmm_b_elems(d), cbytes = bmm_c_elems(d) * esz;
  if (plan_overlap(pc, cbytes, pa, abytes) || plan_overlap(pc, cbytes, pb, bbytes))
    return fail(DFX_ERR_INVALID, "bmm_submit: c overlaps a or b");
  DeviceGuard dg(h->device);
  // 16-byte loads need aligned operands: others take the generic kernel for this submit, as resize and head do
  const int path = (pa | pb) % 16 == 0 ? h->path : DFX_BMM_GENERIC;
  BmmArgs a = h->args;  // per launch: concurrent submits on several streams are independent
  a.a = (const unsigned char *)a_dev;
  a.b = (const signed char *)b_dev;
  a.c = (unsigned char *)c_dev;
  a.c_vec = pc % (4 * esz) == 0 && d.ldc % 4 == 0 && d.c_s0 % 4 == 0 && d.c_s1 % 4 == 0;
  const BmmBiasArgs bias = h->bias_args;  // (a copy, like a)
  const BmmBiasArgs *const bp = h->bias_set ? &bias : nullptr;
  const int rc = path == DFX_BMM_MFMA ? launch_bmm_mfma(a, bp, h->grid[path], (hipStream_t)s, h->route != 0)
                                      : launch_bmm_generic(a, bp, h->grid[path], (hipStream_t)s);
  return g_launches.launched("bmm", rc, path);
}

// test hook: how many submits have launched each kernel so far (shows the per-submit fallback, which query cannot)
int dfx_debug_bmm_launches(int64_t out[2]) { return g_launches.read("bmm", out); }

// test hook: the requant route the last dfx_bmm_set_scales proved (numbering of dfx_debug_conv_requant)
int dfx_debug_bmm_requant(const dfx_bmm_t *h, int32_t out[1]) {
  if (!h || !out) return fail(DFX_ERR_INVALID, "bmm_requant: null argument");
  if (!h->scales_set.load()) return fail(DFX_ERR_STATE, "bmm_requant: dfx_bmm_set_scales not called");
  out[0] = h->route;
  return DFX_OK;
}

int dfx_bmm_query(const dfx_bmm_t *h, dfx_bmm_info *info) {
  if (const int rc = open_query("bmm", h, info)) return rc;
  info->grid = h->grid[h->path];
  info->block = BMM_THREADS;
  info->lds_bytes = bmm_lds_bytes(h->d, h->path);
  info->algorithmic_ops = bmm_algorithmic_ops(h->d);
  info->algorithmic_bytes = bmm_algorithmic_bytes(h->d) + (h->bias_set ? bias_distinct_bytes(h->d, h->bias) : 0);
  return DFX_OK;
}

int dfx_bmm_destroy(dfx_bmm_t *h) {
  release(h);
  return DFX_OK;
}

}  // extern "C"
