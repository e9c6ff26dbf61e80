// dwpw_api.hip -- host side of the depthwise + pointwise conv op (dfx_dwpw_* of include/dfx.h): descriptor validation,
// choice of the path, the fused kernel's tile and LDS plan (dwpw.cuh), the packing and the requant-route proof of its
// stage 1, and the two-launch path (dfx_dwconv_submit + dfx_conv_submit through a buffer the handle owns).
// Stage 0 lives in an ordinary depthwise handle on BOTH paths: its packed weights, constants and proof are read through
// dwconv_window_view() (dfx_internal.h), never rebuilt here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "dfx_internal.h"
#include "dwpw.cuh"
#include "requant_host.h"

namespace dfx {
int launch_dwpw(const DwPwArgs &, int stride, int dst_dt, int grid, int lds, hipStream_t, int mode);
}
using namespace dfx;

struct dfx_dwpw {
  dfx_dwpw_desc d;
  int device = -1;
  int path = 0;
  dfx_dwconv_t *dw = nullptr;     // stage 0: owns its weights, constants and proof (both paths); launched on the two-launch path
  dfx_conv_t *conv = nullptr;     // two-launch path: the unfused pointwise conv
  bool weights_set = false;
  int route0 = 0, route1 = 0;
  // fused path
  int grid = 0, lds = 0;
  DwPwArgs args = {};             // everything but src / dst; copied per launch
  unsigned char *d_w1 = nullptr;  // [W0d | comp1 | bias1 | scale1]
  size_t w1_bytes = 0;
  // two-launch path
  void *d_mid = nullptr;          // the u8 tensor between the stages: ONE buffer, so the submits are serialised
  TwoLaunchOrder order;
  HostStaging host;               // dfx_dwpw_submit_host
  char kernel_name[96] = "";
};

namespace {

constexpr int LDS_MAX = 160 * 1024, LDS_PAIR = 80 * 1024;

int validate_dwpw(const dfx_dwpw_desc &d) {
  if (d.bs <= 0 || d.c <= 0 || d.ih <= 0 || d.iw <= 0 || d.oh <= 0 || d.ow <= 0 || d.oc <= 0)
    return fail(DFX_ERR_INVALID, "dwpw: non-positive dimension");
  if (d.kh <= 0 || d.kw <= 0 || d.kh > 255 || d.kw > 255)
    return fail(DFX_ERR_INVALID, "dwpw: window %d x %d outside 1 .. 255", d.kh, d.kw);
  if (d.sh <= 0 || d.sw <= 0) return fail(DFX_ERR_INVALID, "dwpw: non-positive stride");
  if (d.pad_t < 0 || d.pad_l < 0) return fail(DFX_ERR_INVALID, "dwpw: negative padding");
  if ((long long)(d.oh - 1) * d.sh - d.pad_t > d.ih - 1 || (long long)(d.ow - 1) * d.sw - d.pad_l > d.iw - 1)
    return fail(DFX_ERR_INVALID, "dwpw: the last output row / column's window starts outside the input");
  if ((long long)d.bs * d.ih * d.iw >= (1ll << 31) || (long long)d.bs * d.oh * d.ow >= (1ll << 31))
    return fail(DFX_ERR_INVALID, "dwpw: pixel count beyond 2^31");
  if (d.dst_dt < DFX_F32 || d.dst_dt > DFX_U8) return fail(DFX_ERR_INVALID, "dwpw: bad dst dtype");
  if (d.bia0_dt != DFX_UNDEF && (d.bia0_dt < DFX_F32 || d.bia0_dt > DFX_U8)) return fail(DFX_ERR_INVALID, "dwpw: bad stage-0 bias dtype");
  if (d.bia1_dt != DFX_UNDEF && (d.bia1_dt < DFX_F32 || d.bia1_dt > DFX_U8)) return fail(DFX_ERR_INVALID, "dwpw: bad stage-1 bias dtype");
  if ((d.round_mode0 != DFX_ROUND_NEAREST && d.round_mode0 != DFX_ROUND_DOWN) ||
      (d.round_mode1 != DFX_ROUND_NEAREST && d.round_mode1 != DFX_ROUND_DOWN))
    return fail(DFX_ERR_INVALID, "dwpw: bad round mode");
  if (d.nscales0 != 1 && d.nscales0 != d.c) return fail(DFX_ERR_INVALID, "dwpw: stage-0 scales count must be 1 or c");
  if (d.nscales1 != 1 && d.nscales1 != d.oc) return fail(DFX_ERR_INVALID, "dwpw: stage-1 scales count must be 1 or oc");
  if (d.force_path != -1 && d.force_path != DFX_DWPW_FUSED && d.force_path != DFX_DWPW_TWO_LAUNCH)
    return fail(DFX_ERR_INVALID, "dwpw: bad force_path");
  return DFX_OK;
}

// the shape class of dwpw.cuh
bool fused_class(const dfx_dwpw_desc &d) {
  const long long lim = (1ll << 31) - 64;
  return d.kh == 3 && d.kw == 3 && d.sh == d.sw && (d.sh == 1 || d.sh == 2) && d.c % 32 == 0 && d.c <= 256 &&
         (d.oc == 64 || d.oc == 128 || d.oc == 256) && (long long)d.c * d.oc <= 65536 &&
         (long long)d.ih * d.iw * d.c < lim && (long long)d.oh * d.ow * d.oc * (long long)dt_size(d.dst_dt) < lim &&
         (long long)d.oh * d.ow * d.c < lim;  // (the last clause keeps the owned depthwise handle, dst u8, on its window path)
}

// Auto sends a shape of the class to the fused path only where that path was measured faster than dfx_dwconv +
// dfx_conv by more than the +-4 % box spread.  No shape has such a measurement yet, so auto takes
// the two ops' kernels everywhere and the fused kernel is reached through force_path = DFX_DWPW_FUSED only.
bool fused_wins(const dfx_dwpw_desc &d) {
  (void)d;
  return false;
}

dfx_dwconv_desc stage0_desc(const dfx_dwpw_desc &d) {
  dfx_dwconv_desc s;
  memset(&s, 0, sizeof(s));
  s.bs = d.bs; s.c = d.c; s.ih = d.ih; s.iw = d.iw; s.oh = d.oh; s.ow = d.ow; s.kh = d.kh; s.kw = d.kw;
  s.sh = d.sh; s.sw = d.sw; s.pad_t = d.pad_t; s.pad_l = d.pad_l;
  s.dst_dt = DFX_U8; s.bia_dt = d.bia0_dt; s.relu = 1; s.round_mode = d.round_mode0; s.nscales = d.nscales0;
  s.force_path = -1;
  return s;
}

dfx_conv_desc stage1_desc(const dfx_dwpw_desc &d) {
  dfx_conv_desc c;
  memset(&c, 0, sizeof(c));
  c.bs = d.bs; c.ic = d.c; c.ih = d.oh; c.iw = d.ow; c.oc = d.oc; c.oh = d.oh; c.ow = d.ow;
  c.kh = c.kw = c.sh = c.sw = 1;
  c.dst_dt = d.dst_dt; c.bia0_dt = d.bia1_dt;
  c.conv0_relu = d.relu; c.conv0_round_mode = d.round_mode1;
  c.conv0_nscales = d.nscales1; c.conv1_nscales = 1;
  c.force_variant = -1;
  return c;
}

// LDS plan of dwpw.cuh for a tile height: [1x1 weights | stage-1 constants | mid | 4 staging areas]
struct Plan {
  int tw, nblk, off_cst, off_mid, off_stage, stage_bytes, total;
};
Plan lds_plan(const dfx_dwpw_desc &d, int th) {
  Plan p;
  p.tw = DWPW_THREADS / (d.c / 16);
  p.nblk = (th * p.tw + 31) / 32;
  p.off_cst = d.c * d.oc;
  p.off_mid = p.off_cst + 3 * d.oc * 4;
  p.off_stage = p.off_mid + p.nblk * 32 * (d.c + 16);
  p.stage_bytes = dt_size(d.dst_dt) == 1 ? 32 * (d.oc + 16) : 32 * 144;
  p.total = p.off_stage + (DWPW_THREADS / 64) * p.stage_bytes;
  return p;
}

const char *route_name(int r) { return r == 1 ? "fast" : r == 2 ? "magic" : r == 3 ? "fma" : "exact"; }

void set_name(dfx_dwpw *h) {
  const dfx_dwpw_desc &d = h->d;
  char routes[32];
  if (h->weights_set) snprintf(routes, sizeof(routes), "%s/%s", route_name(h->route0), route_name(h->route1));
  else snprintf(routes, sizeof(routes), "(no weights)");
  if (h->path == DFX_DWPW_FUSED)
    snprintf(h->kernel_name, sizeof(h->kernel_name), "dwpw_fused<%dx%d,s%d,c%d,oc%d,%s> th %d %s", d.kh, d.kw, d.sh, d.c,
             d.oc, dt_name(d.dst_dt), h->args.th, routes);
  else
    snprintf(h->kernel_name, sizeof(h->kernel_name), "dwpw_two_launch<%dx%d,s%dx%d,c%d,oc%d,%s> %s", d.kh, d.kw, d.sh,
             d.sw, d.c, d.oc, dt_name(d.dst_dt), routes);
}

void release(dfx_dwpw *h) {
  if (!h) return;
  DeviceGuard dg(h->device);
  if (h->dw) (void)dfx_dwconv_destroy(h->dw);
  if (h->conv) (void)dfx_conv_destroy(h->conv);
  (void)hipFree(h->d_w1);
  (void)hipFree(h->d_mid);
  h->order.destroy();
  h->host.release();
  delete h;
}

size_t src_bytes(const dfx_dwpw_desc &d) { return (size_t)d.bs * d.ih * d.iw * d.c; }
size_t mid_bytes(const dfx_dwpw_desc &d) { return (size_t)d.bs * d.oh * d.ow * d.c; }
size_t dst_bytes(const dfx_dwpw_desc &d) { return (size_t)d.bs * d.oh * d.ow * d.oc * dt_size(d.dst_dt); }

}  // namespace

extern "C" {

int dfx_dwpw_create(const dfx_dwpw_desc *desc, dfx_dwpw_t **out) {
  if (!desc || !out) return fail(DFX_ERR_INVALID, "dwpw_create: null argument");
  *out = nullptr;
  const dfx_dwpw_desc &d = *desc;
  int rc = validate_dwpw(d);
  if (rc) return rc;
  const bool covered = fused_class(d);
  if (d.force_path == DFX_DWPW_FUSED && !covered)
    return fail(DFX_ERR_UNSUPPORTED, "dwpw_create: shape outside the fused kernel's class (3x3, stride 1 or 2, c %% 32 == 0, c <= 256, oc 64 / 128 / 256, c * oc <= 64 KB, one image below 2^31 bytes)");
  dfx_dwpw *h = new (std::nothrow) dfx_dwpw();
  if (!h) return fail(DFX_ERR_HIP, "out of host memory");
  h->d = d;
  h->path = (covered && (d.force_path == DFX_DWPW_FUSED || (d.force_path == -1 && fused_wins(d)))) ? DFX_DWPW_FUSED
                                                                                                      : DFX_DWPW_TWO_LAUNCH;
  // whatever dfx_conv_create rejects for the pointwise conv is rejected here (before it touches a device)
  if (h->path == DFX_DWPW_TWO_LAUNCH) {
    const dfx_conv_desc cd = stage1_desc(d);
    rc = dfx_conv_create(&cd, &h->conv);
    if (rc) { release(h); return rc; }
  }
  const dfx_dwconv_desc sd = stage0_desc(d);
  rc = dfx_dwconv_create(&sd, &h->dw);
  if (rc) { release(h); return rc; }
  if (hipGetDevice(&h->device) != hipSuccess) h->device = 0;
  if (h->path == DFX_DWPW_FUSED) {
    DwPwArgs &a = h->args;
    a.oc = d.oc;  // (the launcher picks the instance by oc)
    // Tile height: the largest of 16 / 8 / 4 / 2 whose LDS plan fits the CU's 160 KB (2 always does: 64 KB of weights
    // + 3 KB + 9 KB + 35 KB).  Where the instance's registers let two workgroups share a CU (the occupancy query at an
    // 80 KB plan says >= 2: stride 2 with oc = 64, profiles/dwpw/isa_counts.txt), the largest whose plan fits 80 KB is
    // preferred, so that one workgroup's depthwise phase runs under the other's MFMAs; elsewhere that preference would
    // only shrink the tile.
    int th = 2, th_pair = 0;
    for (int t = 16; t >= 2; t /= 2)
      if (lds_plan(d, t).total <= LDS_MAX) { th = t; break; }
    for (int t = 16; t >= 2 && !th_pair; t /= 2)
      if (lds_plan(d, t).total <= LDS_PAIR) th_pair = t;
    if (launch_dwpw(a, d.sh, d.dst_dt, 0, LDS_MAX, nullptr, 1) != 0) {
      release(h);
      return fail(DFX_ERR_HIP, "dwpw_create: cannot raise dynamic LDS limit to %d bytes", LDS_MAX);
    }
    if (th_pair && th_pair != th && launch_dwpw(a, d.sh, d.dst_dt, 0, lds_plan(d, th_pair).total, nullptr, 2) >= 2) th = th_pair;
    if (const char *e = tuning_value("DFX_DWPW_TH")) {  // testing aid: a height of the list that fits
      const int t = atoi(e);
      if ((t == 2 || t == 4 || t == 8 || t == 16) && lds_plan(d, t).total <= LDS_MAX) th = t;
    }
    const Plan p = lds_plan(d, th);
    a.bs = d.bs; a.c = d.c; a.ih = d.ih; a.iw = d.iw; a.oh = d.oh; a.ow = d.ow; a.oc = d.oc; a.pt = d.pad_t; a.pl = d.pad_l;
    a.rm0 = d.round_mode0; a.relu1 = (d.relu || d.dst_dt == DFX_U8) ? 1 : 0; a.rm1 = d.round_mode1;
    a.groups = d.c / 16;
    a.th = th; a.tw = p.tw;
    a.ty = (d.oh + th - 1) / th; a.tx = (d.ow + p.tw - 1) / p.tw;
    const long long ntiles = (long long)d.bs * a.ty * a.tx;  // (< 2^31: bs * oh * ow is)
    a.ntiles = (int)ntiles;
    a.nblk = p.nblk;
    a.tw_magic = (1u << 20) / (unsigned)p.tw + 1;
    for (unsigned px = 0; px < (unsigned)p.nblk * 32; ++px)
      if (((px * a.tw_magic) >> 20) != px / (unsigned)p.tw) {
        release(h);
        return fail(DFX_ERR_HIP, "internal: dwpw tile-row division by %d inexact at %u", p.tw, px);
      }
    a.mid_pitch = d.c + 16;
    a.off_cst = p.off_cst; a.off_mid = p.off_mid; a.off_stage = p.off_stage; a.stage_bytes = p.stage_bytes;
    h->lds = p.total;
    h->w1_bytes = (size_t)d.c * d.oc + (size_t)3 * d.oc * 4;
    hipError_t e = hipMalloc((void **)&h->d_w1, h->w1_bytes);
    if (e != hipSuccess) {
      release(h);
      return fail(DFX_ERR_HIP, "dwpw_create: weight buffer: %s", hipGetErrorString(e));
    }
    a.w1 = h->d_w1;
    int per_cu = launch_dwpw(a, d.sh, d.dst_dt, 0, h->lds, nullptr, 2);
    if (per_cu < 1) per_cu = 1;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, h->device) != hipSuccess) {
      release(h);
      return fail(DFX_ERR_HIP, "dwpw_create: cannot query the device");
    }
    long long grid = std::min(ntiles, (long long)std::max(1, prop.multiProcessorCount) * per_cu);
    if (const char *e2 = tuning_value("DFX_DWPW_GRID")) grid = std::max(1ll, std::min(grid, (long long)atoi(e2)));  // testing aid
    h->grid = (int)grid;
  } else {
    hipError_t e = hipMalloc(&h->d_mid, mid_bytes(d));
    if (e == hipSuccess) e = h->order.create();
    if (e != hipSuccess) {
      release(h);
      return fail(DFX_ERR_HIP, "dwpw_create: buffer of the tensor between the stages: %s", hipGetErrorString(e));
    }
    dfx_conv_info ci;
    rc = dfx_conv_query(h->conv, &ci);
    if (rc) { release(h); return rc; }
    h->grid = ci.grid;
    h->lds = ci.lds_bytes;
  }
  set_name(h);
  *out = h;
  return DFX_OK;
}

int dfx_dwpw_set_weights(dfx_dwpw_t *h, const int8_t *wei_dw, const void *bia0, const float *scales0,
                         const int8_t *wei_pw, const void *bia1, const float *scales1) {
  if (!h || !wei_dw || !scales0 || !wei_pw || !scales1) return fail(DFX_ERR_INVALID, "dwpw_set_weights: null argument");
  const dfx_dwpw_desc &d = h->d;
  if ((d.bia0_dt != DFX_UNDEF && !bia0) || (d.bia1_dt != DFX_UNDEF && !bia1))
    return fail(DFX_ERR_INVALID, "dwpw_set_weights: null bias");
  int rc = dfx_dwconv_set_weights(h->dw, wei_dw, bia0, scales0);
  if (rc) return rc;
  int32_t r0[1] = {0};
  rc = dfx_debug_dwconv_requant(h->dw, r0);
  if (rc) return rc;
  if (h->path == DFX_DWPW_TWO_LAUNCH) {
    rc = dfx_conv_set_weights(h->conv, wei_pw, bia1, scales1, nullptr, nullptr, nullptr);
    if (rc) return rc;
    int32_t r1[2] = {0, -1};
    rc = dfx_debug_conv_requant(h->conv, r1);
    if (rc) return rc;
    h->route0 = r0[0];
    h->route1 = r1[0];
    h->weights_set = true;
    set_name(h);
    return DFX_OK;
  }
  // fused: stage 0 through the depthwise handle's view
  DwArgs da;
  if (!dwconv_window_view(h->dw, &da)) return fail(DFX_ERR_STATE, "dwpw_set_weights: internal: depthwise handle is not on the window path");
  // stage 1: conv_pw.cuh's one-tap W0d image, byte b of lane = W[oc = 32 ob + (lane & 31)][ic = 32 kb + 16 (lane >> 5) + b]
  const int OC = d.oc, IC = d.c, ocb = OC / 32, icb = IC / 32;
  std::vector<unsigned char> img(h->w1_bytes, 0);
  size_t o = 0;
  for (int ob = 0; ob < ocb; ++ob)
    for (int kb = 0; kb < icb; ++kb)
      for (int lane = 0; lane < 64; ++lane)
        for (int b = 0; b < 16; ++b, ++o)
          img[o] = (unsigned char)wei_pw[dfx_blocked_offset(32 * ob + (lane & 31), 32 * kb + 16 * (lane >> 5) + b, 0, 0, IC, 1, 1)];
  int32_t *comp = (int32_t *)(img.data() + (size_t)IC * OC);
  float *fb = (float *)(comp + OC), *fs = fb + OC;
  // (requant_host.h's clause over one output channel of the pointwise conv)
  const bool proven = requant_consts(OC, (size_t)IC, [&](int k, size_t i) { return wei_pw[dfx_blocked_offset(k, (int)i, 0, 0, IC, 1, 1)]; },
                                     bia1, d.bia1_dt, scales1, d.nscales1, comp, fb, fs);
  const bool fast1 = d.round_mode1 == DFX_ROUND_NEAREST && proven && fast_allowed();
  DeviceGuard dg(h->device);
  HIP_TRY(hipMemcpy(h->d_w1, img.data(), h->w1_bytes, hipMemcpyHostToDevice));
  DwPwArgs &a = h->args;
  a.wpk = da.wpk; a.comp0 = da.comp; a.bias0 = da.bias; a.scale0 = da.scale;
  a.fast0 = da.fast;
  a.fast1 = fast1 ? 1 : 0;
  h->route0 = r0[0];
  h->route1 = a.fast1;
  h->weights_set = true;
  set_name(h);
  return DFX_OK;
}

int dfx_dwpw_submit(dfx_dwpw_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s) {
  if (!h || !src_dev || !dst_dev) return fail(DFX_ERR_INVALID, "dwpw_submit: null argument");
  if (((uintptr_t)src_dev | (uintptr_t)dst_dev) % 16)
    return fail(DFX_ERR_INVALID, "dwpw_submit: src and dst must be 16-byte aligned");
  if (!h->weights_set) return fail(DFX_ERR_STATE, "dwpw_submit: dfx_dwpw_set_weights not called");
  DeviceGuard dg(h->device);
  const hipStream_t st = (hipStream_t)s;
  if (h->path == DFX_DWPW_FUSED) {
    DwPwArgs a = h->args;  // per-launch copy: concurrent submits on several streams are independent
    a.src = (const unsigned char *)src_dev;
    a.dst = (unsigned char *)dst_dev;
    if (launch_dwpw(a, h->d.sh, h->d.dst_dt, h->grid, h->lds, st, 0) != 0)
      return fail(DFX_ERR_UNSUPPORTED, "dwpw_submit: no kernel instance for this op");
    HIP_TRY(hipGetLastError());
    return DFX_OK;
  }
  // two launches through the handle's one buffer: serialised (dfx.h; TwoLaunchOrder in dfx_internal.h)
  std::lock_guard<std::mutex> lk(h->order.mu);
  int rc = h->order.enter(st);
  if (rc) return rc;
  rc = dfx_dwconv_submit(h->dw, src_dev, h->d_mid, s);
  if (rc) return rc;
  rc = dfx_conv_submit(h->conv, h->d_mid, dst_dev, s);
  if (rc) return rc;
  return h->order.leave(st);
}

int dfx_dwpw_submit_host(dfx_dwpw_t *h, const void *src_host, void *dst_host) {
  if (!h || !src_host || !dst_host) return fail(DFX_ERR_INVALID, "dwpw_submit_host: null argument");
  if (!h->weights_set) return fail(DFX_ERR_STATE, "dwpw_submit_host: dfx_dwpw_set_weights not called");
  DeviceGuard dg(h->device);
  return h->host.run(src_host, src_bytes(h->d), dst_host, dst_bytes(h->d),
                     [h](const void *s, void *d, dfx_stream_t st) { return dfx_dwpw_submit(h, s, d, st); });
}

int dfx_dwpw_query(const dfx_dwpw_t *h, dfx_dwpw_info *info) {
  if (!h || !info) return fail(DFX_ERR_INVALID, "dwpw_query: null argument");
  memset(info, 0, sizeof(*info));
  info->path = h->path;
  info->grid = h->grid;
  info->block = DWPW_THREADS;
  if (h->path == DFX_DWPW_TWO_LAUNCH) {
    dfx_conv_info ci;
    if (dfx_conv_query(h->conv, &ci) == DFX_OK) info->block = ci.block;
  }
  info->lds_bytes = h->lds;
  info->device = h->device;
  const dfx_dwpw_desc &d = h->d;
  const uint64_t px = (uint64_t)d.bs * d.oh * d.ow;
  info->algorithmic_ops = 2 * px * d.c * d.kh * d.kw + 2 * px * (uint64_t)d.c * d.oc;
  info->algorithmic_bytes = (uint64_t)src_bytes(d) + (uint64_t)d.c * d.kh * d.kw + (uint64_t)d.c * d.oc + (uint64_t)dst_bytes(d) +
                            (h->path == DFX_DWPW_TWO_LAUNCH ? 2 * (uint64_t)mid_bytes(d) : 0);
  memcpy(info->kernel_name, h->kernel_name, sizeof(info->kernel_name));
  return DFX_OK;
}

// test hook: the requant routes the last dfx_dwpw_set_weights proved (numbering of dfx_debug_conv_requant)
int dfx_debug_dwpw_requant(const dfx_dwpw_t *h, int32_t out[2]) {
  if (!h || !out) return fail(DFX_ERR_INVALID, "dwpw_requant: null argument");
  if (!h->weights_set) return fail(DFX_ERR_STATE, "dwpw_requant: dfx_dwpw_set_weights not called");
  out[0] = h->route0;
  out[1] = h->route1;
  return DFX_OK;
}

int dfx_dwpw_destroy(dfx_dwpw_t *h) {
  release(h);
  return DFX_OK;
}

}  // extern "C"
