// reorder_api.hip -- host side of the activation reorder (dfx_reorder_* of include/dfx.h): descriptor
// validation, choice of the kernel path and its tiling, launches.  The kernels are in reorder.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "dfx_device.cuh"
#include "dfx_internal.h"
#include "requant_host.h"

namespace dfx {
int launch_reorder(const ReorderArgs &a, hipStream_t s);
}
using namespace dfx;

struct dfx_reorder {
  dfx_reorder_desc d;
  int device = 0;
  ReorderArgs args = {};
  float *d_scales = nullptr;
  HostStaging host;  // dfx_reorder_submit_host
  char kernel_name[96] = "";
};

namespace {

constexpr int kLdsBudget = 48 * 1024;  // whole-depth tiles: three workgroups per CU and more
constexpr int kMaxBlocks = 256 * 8;    // grid-stride kernels: 8 workgroups per CU

int validate_reorder(const dfx_reorder_desc &d, const float *scales) {
  if (d.bs <= 0 || d.h <= 0 || d.w <= 0 || d.src_c <= 0 || d.dst_c <= 0)
    return fail(DFX_ERR_INVALID, "reorder: non-positive dimension");
  if ((d.src_fmt != DFX_FMT_NHWC && d.src_fmt != DFX_FMT_NCHW) || (d.dst_fmt != DFX_FMT_NHWC && d.dst_fmt != DFX_FMT_NCHW))
    return fail(DFX_ERR_INVALID, "reorder: bad format (NHWC and NCHW only)");
  if (d.src_dt < DFX_F32 || d.src_dt > DFX_U8 || d.dst_dt < DFX_F32 || d.dst_dt > DFX_U8)
    return fail(DFX_ERR_INVALID, "reorder: bad dtype");
  if (d.round_mode != DFX_ROUND_NEAREST && d.round_mode != DFX_ROUND_DOWN)
    return fail(DFX_ERR_INVALID, "reorder: bad round mode");
  if (d.n_scales != 0 && d.n_scales != 1 && d.n_scales != d.src_c)
    return fail(DFX_ERR_INVALID, "reorder: n_scales must be 0, 1 or src_c (%d), not %d", d.src_c, d.n_scales);
  if (d.n_scales > 0 && !scales) return fail(DFX_ERR_INVALID, "reorder: n_scales %d without scales", d.n_scales);
  for (int i = 0; i < d.n_scales; ++i)
    if (!std::isfinite(scales[i])) return fail(DFX_ERR_INVALID, "reorder: scale %d is not finite", i);
  if (d.dst_dt == DFX_S32) return fail(DFX_ERR_UNSUPPORTED, "reorder: s32 destination");
  const long long hw = (long long)d.h * d.w;
  if (hw * d.src_c >= (1ll << 31) || hw * d.dst_c >= (1ll << 31))
    return fail(DFX_ERR_UNSUPPORTED, "reorder: one image has 2^31 elements or more");
  return DFX_OK;
}

// fills everything of `a` but the buffer pointers
int plan_reorder(const dfx_reorder_desc &d, ReorderArgs &a, char *name, size_t name_len) {
  memset(&a, 0, sizeof(a));
  a.bs = d.bs; a.hw = d.h * d.w; a.src_c = d.src_c; a.dst_c = d.dst_c;
  a.src_fmt = d.src_fmt; a.dst_fmt = d.dst_fmt; a.src_dt = d.src_dt; a.dst_dt = d.dst_dt;
  a.rm = d.round_mode;
  a.uniform_scale = d.n_scales <= 1;
  const int es = (int)dt_size(d.src_dt), ed = (int)dt_size(d.dst_dt);
  const long long px = (long long)d.bs * a.hw;
  long long blocks = 0;
  if (d.src_fmt == d.dst_fmt && d.src_c == d.dst_c) {
    a.path = REORDER_FLAT;
    a.total = px * d.src_c;
    a.inner = d.src_fmt == DFX_FMT_NHWC ? 1 : a.hw;
    const int v = 16 / (es > ed ? es : ed);
    blocks = (a.total + 256 * v - 1) / (256 * v);
    if (blocks > kMaxBlocks) blocks = kMaxBlocks;
    snprintf(name, name_len, "reorder_flat<%s,%s> %d elements per lane", dt_name(d.src_dt), dt_name(d.dst_dt), v);
  } else if (d.src_fmt == d.dst_fmt) {
    a.path = REORDER_GENERIC;
    a.total = px * d.dst_c;
    blocks = (a.total + 255) / 256;
    if (blocks > 2 * kMaxBlocks) blocks = 2 * kMaxBlocks;
    snprintf(name, name_len, "reorder_generic<%s,%s>", dt_name(d.src_dt), dt_name(d.dst_dt));
  } else if (d.src_fmt == DFX_FMT_NCHW && d.src_c <= 4 && d.dst_c <= 16) {
    a.path = REORDER_SMALLC;
    a.ptiles = (a.hw + SMALLC_PX - 1) / SMALLC_PX;
    blocks = (long long)d.bs * a.ptiles;
    snprintf(name, name_len, "reorder_smallc<%s,%s> %d->%d", dt_name(d.src_dt), dt_name(d.dst_dt), d.src_c, d.dst_c);
  } else {
    a.path = REORDER_TRANSPOSE;
    const bool to_nhwc = d.dst_fmt == DFX_FMT_NHWC;
    const int cl = d.src_c < d.dst_c ? d.src_c : d.dst_c;
    const int cmax = d.src_c > d.dst_c ? d.src_c : d.dst_c;
    // the NCHW side is the plane side, the NHWC side the pixel side
    const int e_plane = to_nhwc ? es : ed, e_pixel = to_nhwc ? ed : es, c_pixel = to_nhwc ? d.dst_c : d.src_c;
    // Tiling (measured): small tiles -- 64 pixels x 128 bytes (4-byte types) or 64 bytes (1-byte
    // types) of pixel-side channels, 8 - 16 KiB of LDS, 8 workgroups per CU -- beat deep ones, and pixel rows
    // indexed per row beat the same bytes indexed as one span.  The block is the whole depth, its pixel side ONE
    // span, only where channel blocks could not use 16-byte accesses on the pixel side (c * elsize % 16 != 0)
    // and the whole depth fits in LDS.
    const int cb_pref = e_pixel == 4 ? 32 : 64;
    const bool rows_vec = ((long long)c_pixel * e_pixel) % 16 == 0;
    a.tp = a.hw > 32 ? 64 : 32;
    a.cb = cb_pref;
    if (!rows_vec && (long long)cl * (a.tp + 1) * 4 <= kLdsBudget) { a.cb = cmax; a.flat_pixel = 1; }
    else if (!rows_vec && (long long)cl * 33 * 4 <= kLdsBudget) { a.tp = 32; a.cb = cmax; a.flat_pixel = 1; }
    a.cblocks = a.flat_pixel ? 1 : (d.dst_c + a.cb - 1) / a.cb;
    a.ptiles = (a.hw + a.tp - 1) / a.tp;
    a.lds_bytes = (cl < a.cb ? cl : a.cb) * (a.tp + 1) * 4;
    // 16-byte accesses where every tile is aligned (a tile starts at a multiple of 32 pixels)
    a.vec_plane = ((long long)a.hw * e_plane) % 16 == 0;
    a.vec_pixel = a.flat_pixel ? ((long long)a.hw * c_pixel * e_pixel) % 16 == 0 : ((long long)c_pixel * e_pixel) % 16 == 0;
    blocks = (long long)d.bs * a.ptiles * a.cblocks;
    snprintf(name, name_len, "reorder_transpose<%s,%s,%s> tile %dpx x %dch%s%s", dt_name(d.src_dt), dt_name(d.dst_dt),
             to_nhwc ? "to_nhwc" : "to_nchw", a.tp, cl < a.cb ? cl : a.cb, a.vec_plane ? "" : " narrow-plane",
             a.vec_pixel ? "" : " narrow-pixel");
  }
  if (blocks >= (1ll << 31)) return fail(DFX_ERR_UNSUPPORTED, "reorder: more than 2^31 workgroups");
  a.grid = (int)blocks;
  return DFX_OK;
}

size_t src_bytes(const dfx_reorder_desc &d) { return (size_t)d.bs * d.h * d.w * d.src_c * dt_size(d.src_dt); }
size_t dst_bytes(const dfx_reorder_desc &d) { return (size_t)d.bs * d.h * d.w * d.dst_c * dt_size(d.dst_dt); }

}  // namespace

extern "C" {

int dfx_reorder_create(const dfx_reorder_desc *desc, const float *scales_host, dfx_reorder_t **out) {
  if (!desc || !out) return fail(DFX_ERR_INVALID, "reorder_create: null argument");
  *out = nullptr;
  const dfx_reorder_desc &d = *desc;
  int rc = validate_reorder(d, scales_host);
  if (rc) return rc;
  ReorderArgs a;
  char name[96];
  rc = plan_reorder(d, a, name, sizeof(name));
  if (rc) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(DFX_ERR_NO_DEVICE, "reorder_create: no HIP device (this library has no CPU path)");
  dfx_reorder *h = new (std::nothrow) dfx_reorder();
  if (!h) return fail(DFX_ERR_HIP, "out of host memory");
  h->d = d;
  if (hipGetDevice(&h->device) != hipSuccess) h->device = 0;
  h->args = a;
  memcpy(h->kernel_name, name, sizeof(name));
  // the kernels index one scale per source channel: expand "none" (1.0f) and "one"
  std::vector<float> sc((size_t)d.src_c, 1.0f);
  for (int k = 0; k < d.src_c && d.n_scales > 0; ++k) sc[k] = scales_host[d.n_scales == 1 ? 0 : k];
  hipError_t e = hipMalloc((void **)&h->d_scales, sc.size() * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(h->d_scales, sc.data(), sc.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(h->d_scales);
    delete h;
    return fail(DFX_ERR_HIP, "reorder_create: scales upload: %s", hipGetErrorString(e));
  }
  h->args.scales = h->d_scales;
  *out = h;
  return DFX_OK;
}

int dfx_reorder_submit(dfx_reorder_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s) {
  if (!h || !src_dev || !dst_dev) return fail(DFX_ERR_INVALID, "reorder_submit: null argument");
  if (((uintptr_t)src_dev | (uintptr_t)dst_dev) % 16)
    return fail(DFX_ERR_INVALID, "reorder_submit: src and dst must be 16-byte aligned");
  DeviceGuard dg(h->device);
  ReorderArgs a = h->args;  // per-launch copy: concurrent submits on several streams are independent
  a.src = (const unsigned char *)src_dev;
  a.dst = (unsigned char *)dst_dev;
  if (launch_reorder(a, (hipStream_t)s) != 0) return fail(DFX_ERR_INVALID, "reorder_submit: bad dtype");
  HIP_TRY(hipGetLastError());
  return DFX_OK;
}

int dfx_reorder_submit_host(dfx_reorder_t *h, const void *src_host, void *dst_host) {
  if (!h || !src_host || !dst_host) return fail(DFX_ERR_INVALID, "reorder_submit_host: null argument");
  DeviceGuard dg(h->device);
  return h->host.run(src_host, src_bytes(h->d), dst_host, dst_bytes(h->d),
                     [h](const void *s, void *d, dfx_stream_t st) { return dfx_reorder_submit(h, s, d, st); });
}

int dfx_reorder_query(const dfx_reorder_t *h, dfx_reorder_info *info) {
  if (!h || !info) return fail(DFX_ERR_INVALID, "reorder_query: null argument");
  memset(info, 0, sizeof(*info));
  const ReorderArgs &a = h->args;
  info->path = a.path;
  info->grid = a.grid;
  info->block = 256;
  info->lds_bytes = a.lds_bytes;
  info->device = h->device;
  info->tile_pixels = a.tp;
  info->channel_block = a.path == REORDER_TRANSPOSE ? (a.cb < a.dst_c ? a.cb : a.dst_c) : 0;
  info->vec_plane = a.vec_plane;
  info->vec_pixel = a.vec_pixel;
  const int cl = a.src_c < a.dst_c ? a.src_c : a.dst_c;
  info->algorithmic_bytes = (uint64_t)a.bs * a.hw * ((uint64_t)cl * dt_size(a.src_dt) + (uint64_t)a.dst_c * dt_size(a.dst_dt));
  memcpy(info->kernel_name, h->kernel_name, sizeof(info->kernel_name));
  return DFX_OK;
}

int dfx_reorder_destroy(dfx_reorder_t *h) {
  if (!h) return DFX_OK;
  DeviceGuard dg(h->device);
  (void)hipFree(h->d_scales);
  h->host.release();
  delete h;
  return DFX_OK;
}

}  // extern "C"
