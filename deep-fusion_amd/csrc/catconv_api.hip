// catconv_api.hip -- host side of the concat + pointwise conv op (dfx_catconv_* of include/dfx.h): descriptor
// validation, choice of the path, the per-submit k-block table of the fused kernel (catconv_pw.cuh), and the
// two-launch path (dfx_concat_submit + dfx_conv_submit through a buffer the handle owns).
// The weights live in an ordinary conv handle of the equivalent pointwise conv on BOTH paths: its packed weight
// image, constants and requant-route proofs are read through conv_pw_view() (dfx_internal.h), never rebuilt here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "catconv_pw.cuh"
#include "dfx_device.cuh"
#include "dfx_internal.h"

namespace dfx {
int launch_catconv_pw(const ConvArgs &, const PwGeom &, const CatTab &, int, int, int, hipStream_t, int);
}
using namespace dfx;

struct dfx_catconv {
  dfx_catconv_desc d;
  std::vector<int> channels;
  int device = -1;
  int ic = 0;
  long long px = 0;
  int path = 0;
  dfx_conv_t *conv = nullptr;  // the equivalent pointwise conv: owns weights, constants, proofs (both paths)
  bool weights_set = false;
  // fused path
  int grid = 0, lds = 0;
  unsigned short kb_src[CAT_MAX_KB], kb_off[CAT_MAX_KB];  // k-block -> branch, byte offset inside its pixel row
  // two-launch path
  dfx_concat_t *concat = nullptr;
  void *d_cat = nullptr;  // the concatenated tensor: ONE buffer, so the submits are serialised
  TwoLaunchOrder order;
  HostStaging host;       // dfx_catconv_submit_host
  char kernel_name[96] = "";
};

namespace {

int validate_catconv(const dfx_catconv_desc &d, long long *ic_out) {
  if (d.n_inputs < 2 || d.n_inputs > 16) return fail(DFX_ERR_INVALID, "catconv: n_inputs must be 2 .. 16, not %d", d.n_inputs);
  if (d.bs <= 0 || d.h <= 0 || d.w <= 0 || d.oc <= 0) return fail(DFX_ERR_INVALID, "catconv: non-positive dimension");
  if (!d.channels) return fail(DFX_ERR_INVALID, "catconv: null channels");
  long long ic = 0;
  for (int i = 0; i < d.n_inputs; ++i) {
    if (d.channels[i] <= 0 || d.channels[i] % 16)
      return fail(DFX_ERR_INVALID, "catconv: channels of input %d (%d) not a positive multiple of 16", i, d.channels[i]);
    ic += d.channels[i];
  }
  if (ic >= (1ll << 31) || (long long)d.bs * d.h * d.w >= (1ll << 31))
    return fail(DFX_ERR_INVALID, "catconv: channel sum or pixel count beyond 2^31");
  if (d.dst_dt < DFX_F32 || d.dst_dt > DFX_U8) return fail(DFX_ERR_INVALID, "catconv: bad dst dtype");
  if (d.bia_dt != DFX_UNDEF && (d.bia_dt < DFX_F32 || d.bia_dt > DFX_U8)) return fail(DFX_ERR_INVALID, "catconv: bad bias dtype");
  if (d.round_mode != DFX_ROUND_NEAREST && d.round_mode != DFX_ROUND_DOWN) return fail(DFX_ERR_INVALID, "catconv: bad round mode");
  if (d.nscales != 1 && d.nscales != d.oc) return fail(DFX_ERR_INVALID, "catconv: scales count must be 1 or oc");
  if (d.force_path != -1 && d.force_path != DFX_CATCONV_FUSED && d.force_path != DFX_CATCONV_TWO_LAUNCH)
    return fail(DFX_ERR_INVALID, "catconv: bad force_path");
  *ic_out = ic;
  return DFX_OK;
}

// the shape class of catconv_pw.cuh (the conv handle must ALSO be served by conv_pw.cuh: checked at create)
bool fused_class(const dfx_catconv_desc &d, long long ic) {
  int widest = 0;
  for (int i = 0; i < d.n_inputs; ++i) {
    if (d.channels[i] % 32) return false;
    widest = std::max(widest, d.channels[i]);
  }
  const long long px = (long long)d.bs * d.h * d.w;
  return ic % 256 == 0 && (d.oc == 64 || d.oc == 128 || d.oc == 256) && (long long)d.oc * ic <= 98304 &&
         ic / 32 <= CAT_MAX_KB && px < (1ll << 31) - 64 && px * widest < (1ll << 31) - 64;
}

dfx_conv_desc equivalent_conv(const dfx_catconv_desc &d, int ic) {
  dfx_conv_desc c;
  memset(&c, 0, sizeof(c));
  c.bs = d.bs; c.ic = ic; c.ih = d.h; c.iw = d.w; c.oc = d.oc; c.oh = d.h; c.ow = d.w;
  c.kh = c.kw = c.sh = c.sw = 1;
  c.dst_dt = d.dst_dt; c.bia0_dt = d.bia_dt;
  c.conv0_relu = d.relu; c.conv0_round_mode = d.round_mode;
  c.conv0_nscales = d.nscales; c.conv1_nscales = 1;
  c.force_variant = -1;
  return c;
}

void release(dfx_catconv *h) {
  if (!h) return;
  DeviceGuard dg(h->device);
  if (h->conv) (void)dfx_conv_destroy(h->conv);
  if (h->concat) (void)dfx_concat_destroy(h->concat);
  (void)hipFree(h->d_cat);
  h->order.destroy();
  h->host.release();
  delete h;
}

size_t dst_bytes(const dfx_catconv *h) { return (size_t)h->px * h->d.oc * dt_size(h->d.dst_dt); }

}  // namespace

extern "C" {

int dfx_catconv_create(const dfx_catconv_desc *desc, dfx_catconv_t **out) {
  if (!desc || !out) return fail(DFX_ERR_INVALID, "catconv_create: null argument");
  *out = nullptr;
  const dfx_catconv_desc &d = *desc;
  long long ic = 0;
  int rc = validate_catconv(d, &ic);
  if (rc) return rc;
  const bool covered = fused_class(d, ic);
  dfx_catconv *h = new (std::nothrow) dfx_catconv();
  if (!h) return fail(DFX_ERR_HIP, "out of host memory");
  h->d = d;
  h->channels.assign(d.channels, d.channels + d.n_inputs);
  h->d.channels = h->channels.data();
  h->ic = (int)ic;
  h->px = (long long)d.bs * d.h * d.w;
  // whatever dfx_conv_create rejects for the equivalent pointwise conv is rejected here (before it touches a device)
  const dfx_conv_desc cd = equivalent_conv(d, h->ic);
  rc = dfx_conv_create(&cd, &h->conv);
  if (rc) { release(h); return rc; }
  if (hipGetDevice(&h->device) != hipSuccess) h->device = 0;
  ConvArgs ca;
  PwGeom pg;
  int lds = 0;
  const bool fused_ok = covered && conv_pw_view(h->conv, &ca, &pg, &lds);  // (DFX_STREAM_PW=0 leaves the class empty)
  if (d.force_path == DFX_CATCONV_FUSED && !fused_ok) {
    release(h);
    return fail(DFX_ERR_UNSUPPORTED, "catconv_create: shape outside the fused kernel's class (branches %% 32, ic %% 256, oc 64 / 128 / 256, oc * ic <= 96 KB)");
  }
  h->path = (fused_ok && d.force_path != DFX_CATCONV_TWO_LAUNCH) ? DFX_CATCONV_FUSED : DFX_CATCONV_TWO_LAUNCH;
  dfx_conv_info ci;
  rc = dfx_conv_query(h->conv, &ci);
  if (rc) { release(h); return rc; }
  if (h->path == DFX_CATCONV_FUSED) {
    int kb = 0;
    for (int i = 0; i < d.n_inputs; ++i)
      for (int off = 0; off < h->channels[i]; off += 32, ++kb) {
        h->kb_src[kb] = (unsigned short)i;
        h->kb_off[kb] = (unsigned short)off;
      }
    h->lds = lds;
    CatTab t;
    memset(&t, 0, sizeof(t));
    if (launch_catconv_pw(ca, pg, t, d.dst_dt, 0, lds, nullptr, 1) != 0) {
      release(h);
      return fail(DFX_ERR_HIP, "catconv_create: cannot raise dynamic LDS limit to %d bytes", lds);
    }
    int per_cu = launch_catconv_pw(ca, pg, t, d.dst_dt, 0, lds, nullptr, 2);
    if (per_cu < 1) per_cu = 1;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, h->device) != hipSuccess) {
      release(h);
      return fail(DFX_ERR_HIP, "catconv_create: cannot query the device");
    }
    // conv_pw.cuh's grid rule: one workgroup's worth of 32-pixel blocks per workgroup at most, all resident
    h->grid = std::min((pg.n_blocks + PW_THREADS / 64 - 1) / (PW_THREADS / 64), prop.multiProcessorCount * per_cu);
    snprintf(h->kernel_name, sizeof(h->kernel_name), "catconv_pw_kernel<%d,%d> %d branches", pg.ocb, d.dst_dt, d.n_inputs);
  } else {
    dfx_concat_desc cc;
    memset(&cc, 0, sizeof(cc));
    cc.n_inputs = d.n_inputs; cc.bs = d.bs; cc.h = d.h; cc.w = d.w; cc.dt = DFX_U8; cc.post_relu = 0;
    cc.channels = h->channels.data();
    rc = dfx_concat_create(&cc, &h->concat);
    if (rc) { release(h); return rc; }
    hipError_t e = hipMalloc(&h->d_cat, (size_t)h->px * h->ic);
    if (e == hipSuccess) e = h->order.create();
    if (e != hipSuccess) {
      release(h);
      return fail(DFX_ERR_HIP, "catconv_create: buffer of the concatenated tensor: %s", hipGetErrorString(e));
    }
    h->grid = ci.grid;
    h->lds = ci.lds_bytes;
    snprintf(h->kernel_name, sizeof(h->kernel_name), "%s", ci.kernel_name);
  }
  *out = h;
  return DFX_OK;
}

int dfx_catconv_set_weights(dfx_catconv_t *h, const int8_t *wei_blocked, const void *bia, const float *scales) {
  if (!h || !wei_blocked || !scales) return fail(DFX_ERR_INVALID, "catconv_set_weights: null argument");
  int rc = dfx_conv_set_weights(h->conv, wei_blocked, bia, scales, nullptr, nullptr, nullptr);
  if (rc) return rc;
  h->weights_set = true;
  return DFX_OK;
}

int dfx_catconv_submit(dfx_catconv_t *h, const void *const *srcs_dev, void *dst_dev, dfx_stream_t s) {
  if (!h || !srcs_dev || !dst_dev) return fail(DFX_ERR_INVALID, "catconv_submit: null argument");
  uintptr_t bits = (uintptr_t)dst_dev;
  for (int i = 0; i < h->d.n_inputs; ++i) {
    if (!srcs_dev[i]) return fail(DFX_ERR_INVALID, "catconv_submit: null input %d", i);
    bits |= (uintptr_t)srcs_dev[i];
  }
  if (bits % 16) return fail(DFX_ERR_INVALID, "catconv_submit: every branch and dst must be 16-byte aligned");
  if (!h->weights_set) return fail(DFX_ERR_STATE, "catconv_submit: dfx_catconv_set_weights not called");
  DeviceGuard dg(h->device);
  const hipStream_t st = (hipStream_t)s;
  if (h->path == DFX_CATCONV_FUSED) {
    // per-launch copies of everything: concurrent submits share only immutable state
    ConvArgs a;
    PwGeom g;
    int lds = 0;
    if (!conv_pw_view(h->conv, &a, &g, &lds)) return fail(DFX_ERR_STATE, "catconv_submit: internal: conv handle lost its pointwise kernel");
    a.src = nullptr;
    a.dst = dst_dev;
    CatTab t;
    memset(&t, 0, sizeof(t));
    for (int kb = 0; kb < g.icb; ++kb) {
      const int i = h->kb_src[kb];
      t.kb[kb].p = (const unsigned char *)srcs_dev[i] + h->kb_off[kb];
      t.kb[kb].pitch = (unsigned)h->channels[i];
    }
    if (launch_catconv_pw(a, g, t, h->d.dst_dt, h->grid, lds, st, 0) != 0)
      return fail(DFX_ERR_UNSUPPORTED, "catconv_submit: no kernel instance for this op");
    HIP_TRY(hipGetLastError());
    return DFX_OK;
  }
  // two launches through the handle's one buffer: serialised (dfx.h; TwoLaunchOrder in dfx_internal.h)
  std::lock_guard<std::mutex> lk(h->order.mu);
  int rc = h->order.enter(st);
  if (rc) return rc;
  rc = dfx_concat_submit(h->concat, srcs_dev, h->d_cat, s);
  if (rc) return rc;
  rc = dfx_conv_submit(h->conv, h->d_cat, dst_dev, s);
  if (rc) return rc;
  return h->order.leave(st);
}

int dfx_catconv_submit_host(dfx_catconv_t *h, const void *const *srcs_host, void *dst_host) {
  if (!h || !srcs_host || !dst_host) return fail(DFX_ERR_INVALID, "catconv_submit_host: null argument");
  for (int i = 0; i < h->d.n_inputs; ++i)
    if (!srcs_host[i]) return fail(DFX_ERR_INVALID, "catconv_submit_host: null input %d", i);
  if (!h->weights_set) return fail(DFX_ERR_STATE, "catconv_submit_host: dfx_catconv_set_weights not called");
  DeviceGuard dg(h->device);
  std::vector<size_t> sb;
  for (int c : h->channels) sb.push_back((size_t)h->px * c);
  return h->host.run(h->d.n_inputs, srcs_host, sb.data(), dst_host, dst_bytes(h),
                     [h](const void *const *s, void *d, dfx_stream_t st) { return dfx_catconv_submit(h, s, d, st); });
}

int dfx_catconv_query(const dfx_catconv_t *h, dfx_catconv_info *info) {
  if (!h || !info) return fail(DFX_ERR_INVALID, "catconv_query: null argument");
  memset(info, 0, sizeof(*info));
  info->path = h->path;
  info->grid = h->grid;
  info->block = PW_THREADS;
  if (h->path == DFX_CATCONV_TWO_LAUNCH) {
    dfx_conv_info ci;
    if (dfx_conv_query(h->conv, &ci) == DFX_OK) info->block = ci.block;
  }
  info->lds_bytes = h->lds;
  info->device = h->device;
  const uint64_t px = (uint64_t)h->px, ic = (uint64_t)h->ic, oc = (uint64_t)h->d.oc;
  info->algorithmic_ops = 2 * px * oc * ic;
  info->algorithmic_bytes = px * ic + oc * ic + px * oc * dt_size(h->d.dst_dt) +
                            (h->path == DFX_CATCONV_TWO_LAUNCH ? 2 * px * ic : 0);
  snprintf(info->kernel_name, sizeof(info->kernel_name), "%s", h->kernel_name);
  return DFX_OK;
}

// test hook: the requant route of the inner conv handle -- the fused kernel reads the same proofs (conv_pw_view)
int dfx_debug_catconv_requant(const dfx_catconv_t *h, int32_t out[2]) {
  if (!h || !out) return fail(DFX_ERR_INVALID, "catconv_requant: null argument");
  return dfx_debug_conv_requant(h->conv, out);
}

int dfx_catconv_destroy(dfx_catconv_t *h) {
  release(h);
  return DFX_OK;
}

}  // extern "C"
