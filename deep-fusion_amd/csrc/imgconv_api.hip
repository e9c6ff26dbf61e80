// imgconv_api.hip -- host side of the first-layer conv op (dfx_imgconv_* of include/dfx.h): descriptor validation,
// choice of the path and of the launch geometry, weight packing for the MFMA kernel (imgconv.cuh, imgconv_pack.h), and
// the requant route's proof from the actual weights, bias and scales (requant_host.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "dfx_internal.h"
#include "imgconv.cuh"
#include "imgconv_pack.h"
#include "requant_host.h"

namespace dfx {
int launch_imgconv_mfma(const IcArgs &, int grid, int lds, hipStream_t, int mode, bool fast);
int launch_imgconv_generic(const IcArgs &, int grid, hipStream_t);
}
using namespace dfx;

struct dfx_imgconv {
  dfx_imgconv_desc d;
  int device = 0;
  int path = 0;
  int grid = 0, block = 0, lds = 0;
  IcArgs args = {};                // everything but src / dst; copied per launch
  unsigned char *d_buf = nullptr;  // packed weights | raw weights | comp | bias | scale
  size_t off_wraw = 0, off_comp = 0, off_bias = 0, off_scale = 0, buf_bytes = 0;
  bool weights_set = false;
  int route = 0;                   // 0 exact, 1 fast (dfx_debug_conv_requant's numbering)
  HostStaging host;                // dfx_imgconv_submit_host
  char kernel_name[96] = "";
};

namespace {

int validate_imgconv(const dfx_imgconv_desc &d) {
  if (d.bs <= 0 || d.ic <= 0 || d.ih <= 0 || d.iw <= 0 || d.oc <= 0 || d.oh <= 0 || d.ow <= 0 || d.kh <= 0 || d.kw <= 0)
    return fail(DFX_ERR_INVALID, "imgconv: non-positive dimension");
  if (d.ic > 4) return fail(DFX_ERR_INVALID, "imgconv: ic %d beyond 4 (an image has 1 to 4 channels; dfx_conv / dfx_gconv take more)", d.ic);
  if (d.kh > 255 || d.kw > 255) return fail(DFX_ERR_INVALID, "imgconv: window beyond 255");
  if (d.sh <= 0 || d.sw <= 0) return fail(DFX_ERR_INVALID, "imgconv: non-positive stride");
  if (d.pad_t < 0 || d.pad_l < 0) return fail(DFX_ERR_INVALID, "imgconv: negative padding");
  if ((long long)d.kh * d.kw * d.ic > 65025)
    return fail(DFX_ERR_INVALID, "imgconv: kh * kw * ic beyond 65025 (the accumulator could leave s32)");
  if ((long long)(d.oh - 1) * d.sh - d.pad_t > d.ih - 1 || (long long)(d.ow - 1) * d.sw - d.pad_l > d.iw - 1)
    return fail(DFX_ERR_INVALID, "imgconv: the last output row / column's window starts outside the input");
  if ((long long)d.bs * d.ih * d.iw >= (1ll << 31) || (long long)d.bs * d.oh * d.ow >= (1ll << 31))
    return fail(DFX_ERR_INVALID, "imgconv: pixel count beyond 2^31");
  if (d.dst_dt < DFX_F32 || d.dst_dt > DFX_U8) return fail(DFX_ERR_INVALID, "imgconv: bad dst dtype");
  if (d.bia_dt != DFX_UNDEF && (d.bia_dt < DFX_F32 || d.bia_dt > DFX_U8)) return fail(DFX_ERR_INVALID, "imgconv: bad bias dtype");
  if (d.round_mode != DFX_ROUND_NEAREST && d.round_mode != DFX_ROUND_DOWN) return fail(DFX_ERR_INVALID, "imgconv: bad round mode");
  if (d.nscales != 1 && d.nscales != d.oc) return fail(DFX_ERR_INVALID, "imgconv: scales count must be 1 or oc");
  if (d.force_path != -1 && d.force_path != DFX_IMGCONV_MFMA && d.force_path != DFX_IMGCONV_GENERIC)
    return fail(DFX_ERR_INVALID, "imgconv: bad force_path");
  return DFX_OK;
}

// the shape class of imgconv.cuh
bool mfma_class(const dfx_imgconv_desc &d) {
  const long long lim = 1ll << 31;  // one image below 2^31 bytes on either side (the kernel's offsets are 64-bit)
  const bool window = d.kh == d.kw && d.sh == d.sw && ((d.kh == 7 && d.sh == 2) || (d.kh == 3 && (d.sh == 1 || d.sh == 2)));
  return window && (d.ic == 3 || d.ic == 4) && d.pad_t <= d.kh - 1 && d.pad_l <= d.kw - 1 && d.oc % 32 == 0 &&
         d.oc <= 32 * IC_MAX_BLOCKS && (long long)d.ih * d.iw * d.ic < lim &&
         (long long)d.oh * d.ow * d.oc * (long long)dt_size(d.dst_dt) < lim;
}

void set_name(dfx_imgconv *h) {
  const dfx_imgconv_desc &d = h->d;
  if (h->path == DFX_IMGCONV_MFMA)
    snprintf(h->kernel_name, sizeof(h->kernel_name), "imgconv_mfma<%dx%d,s%d,ic%d,oc%d,%s> %s", d.kh, d.kw, d.sh, d.ic, d.oc,
             dt_name(d.dst_dt), !h->weights_set ? "(no weights)" : h->route ? "fast" : "exact");
  else
    snprintf(h->kernel_name, sizeof(h->kernel_name), "imgconv_generic<%dx%d,s%dx%d,ic%d,oc%d,%s> %s", d.kh, d.kw, d.sh, d.sw, d.ic,
             d.oc, dt_name(d.dst_dt), !h->weights_set ? "(no weights)" : "exact");
}

void release(dfx_imgconv *h) {
  if (!h) return;
  DeviceGuard dg(h->device);
  (void)hipFree(h->d_buf);
  h->host.release();
  delete h;
}

size_t src_bytes(const dfx_imgconv_desc &d) { return (size_t)d.bs * d.ih * d.iw * d.ic; }
size_t dst_bytes(const dfx_imgconv_desc &d) { return (size_t)d.bs * d.oh * d.ow * d.oc * dt_size(d.dst_dt); }
size_t wei_count(const dfx_imgconv_desc &d) { return (size_t)d.oc * d.ic * d.kh * d.kw; }

}  // namespace

extern "C" {

int dfx_imgconv_create(const dfx_imgconv_desc *desc, dfx_imgconv_t **out) {
  if (!desc || !out) return fail(DFX_ERR_INVALID, "imgconv_create: null argument");
  *out = nullptr;
  const dfx_imgconv_desc &d = *desc;
  int rc = validate_imgconv(d);
  if (rc) return rc;
  const bool covered = mfma_class(d);
  if (d.force_path == DFX_IMGCONV_MFMA && !covered)
    return fail(DFX_ERR_UNSUPPORTED, "imgconv_create: shape outside the MFMA kernel's class (ic 3 or 4, window / stride 7x7 / 2, 3x3 / 1 or 3x3 / 2, padding at most k - 1, oc a multiple of 32 up to 128, one image below 2^31 bytes)");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(DFX_ERR_NO_DEVICE, "imgconv_create: no HIP device (this library has no CPU path)");
  dfx_imgconv *h = new (std::nothrow) dfx_imgconv();
  if (!h) return fail(DFX_ERR_HIP, "out of host memory");
  h->d = d;
  if (hipGetDevice(&h->device) != hipSuccess) h->device = 0;
  h->path = (covered && d.force_path != DFX_IMGCONV_GENERIC) ? DFX_IMGCONV_MFMA : DFX_IMGCONV_GENERIC;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, h->device) != hipSuccess) {
    release(h);
    return fail(DFX_ERR_HIP, "imgconv_create: cannot query the device");
  }
  const int cus = std::max(1, prop.multiProcessorCount);
  IcArgs &a = h->args;
  a.bs = d.bs; a.ic = d.ic; a.ih = d.ih; a.iw = d.iw; a.oc = d.oc; a.oh = d.oh; a.ow = d.ow;
  a.kh = d.kh; a.kw = d.kw; a.sh = d.sh; a.sw = d.sw; a.pt = d.pad_t; a.pl = d.pad_l;
  a.dst_dt = d.dst_dt; a.relu = (d.relu || d.dst_dt == DFX_U8) ? 1 : 0; a.rm = d.round_mode;
  a.src_total = (long long)src_bytes(d);
  size_t wpk_bytes = 0;
  if (h->path == DFX_IMGCONV_MFMA) {
    const int K = d.kh, S = d.sh;
    a.cblocks = d.oc / 32;
    wpk_bytes = imgconv_pack_bytes(d.oc, K);
    h->block = IC_THREADS;
    const int fixed = (int)wpk_bytes + 3 * 32 * IC_MAX_BLOCKS * 4 + (IC_THREADS / 64) * GC_STAGE_BYTES;
    // An item is a band of tr output rows x a block of tc <= 64 output columns of one image, about 512 pixels (two
    // strips per wave), the columns of a row split evenly; its halo is ir rows of icp pixels (the lanes of the last
    // column read 4 pixels from kernel column 4 (7x7) or 0 (3x3) on, rounded up to whole groups of 4), kept below 48 KB.
    const int ncb = (d.ow + 63) / 64, tc = (d.ow + ncb - 1) / ncb;
    const int icp = (((tc - 1) * S + (K == 7 ? 8 : 4)) + 3) & ~3;
    auto halo = [&](int tr) { return (long long)((tr - 1) * S + K) * icp * 4; };
    int tr = std::max(1, std::min(d.oh, 512 / tc));
    while (tr > 1 && halo(tr) > 48 * 1024) --tr;
    a.t_tr = tr; a.t_tc = tc; a.t_ir = (tr - 1) * S + K; a.t_icp = icp;
    a.t_nbands = (d.oh + tr - 1) / tr; a.t_ncb = ncb;
    const long long items = (long long)d.bs * a.t_nbands * ncb;  // <= bs * oh * ow < 2^31
    a.t_items = (int)items;
    h->lds = fixed + (int)halo(tr);
    // Launch: the workgroups that are resident at once (by LDS, at most 4 of 512 threads per CU); fewer workgroups
    // than items (small devices, DFX_IMGCONV_GRID) make the workgroups loop over the items.
    long long grid = std::min<long long>(items, (long long)cus * std::min(4, std::max(1, 160 * 1024 / h->lds)));
    if (const char *e = tuning_value("DFX_IMGCONV_GRID")) grid = std::max(1ll, std::min(grid, (long long)atoi(e)));  // testing aid
    h->grid = (int)grid;
    // both routes' instances: set_weights may switch between them later
    if (launch_imgconv_mfma(a, h->grid, h->lds, nullptr, 1, false) != 0 || launch_imgconv_mfma(a, h->grid, h->lds, nullptr, 1, true) != 0) {
      release(h);
      return fail(DFX_ERR_HIP, "imgconv_create: cannot reserve %d bytes of LDS", h->lds);
    }
  } else {
    a.items = (long long)d.bs * d.oh * d.ow * d.oc;
    h->block = 256;
    h->lds = 0;
    h->grid = (int)std::min((a.items + 255) / 256, (long long)cus * 8);
  }
  h->off_wraw = round16(wpk_bytes);
  h->off_comp = h->off_wraw + round16(wei_count(d));
  h->off_bias = h->off_comp + round16((size_t)d.oc * 4);
  h->off_scale = h->off_bias + round16((size_t)d.oc * 4);
  h->buf_bytes = h->off_scale + round16((size_t)d.oc * 4);
  hipError_t e = hipMalloc((void **)&h->d_buf, h->buf_bytes);
  if (e != hipSuccess) {
    release(h);
    return fail(DFX_ERR_HIP, "imgconv_create: weight buffer: %s", hipGetErrorString(e));
  }
  a.wpk = h->d_buf;
  a.wraw = (const signed char *)(h->d_buf + h->off_wraw);
  a.comp = (const int *)(h->d_buf + h->off_comp);
  a.bias = (const float *)(h->d_buf + h->off_bias);
  a.scale = (const float *)(h->d_buf + h->off_scale);
  set_name(h);
  *out = h;
  return DFX_OK;
}

int dfx_imgconv_set_weights(dfx_imgconv_t *h, const int8_t *wei, const void *bia, const float *scales) {
  if (!h || !wei || !scales) return fail(DFX_ERR_INVALID, "imgconv_set_weights: null argument");
  const dfx_imgconv_desc &d = h->d;
  if (d.bia_dt != DFX_UNDEF && !bia) return fail(DFX_ERR_INVALID, "imgconv_set_weights: null bias");
  const size_t taps = (size_t)d.ic * d.kh * d.kw;  // of one output channel
  std::vector<unsigned char> img(h->buf_bytes, 0);
  int *comp = (int *)(img.data() + h->off_comp);
  float *fb = (float *)(img.data() + h->off_bias), *fs = (float *)(img.data() + h->off_scale);
  memcpy(img.data() + h->off_wraw, wei, wei_count(d));
  const bool proven = requant_consts(d.oc, taps, [&](int k, size_t i) { return wei[(size_t)k * taps + i]; }, bia, d.bia_dt, scales,
                                     d.nscales, comp, fb, fs);
  const bool fast = h->path == DFX_IMGCONV_MFMA && d.round_mode == DFX_ROUND_NEAREST && proven && fast_allowed();
  if (h->path == DFX_IMGCONV_MFMA) imgconv_pack(wei, d.oc, d.ic, d.kh, img.data());
  DeviceGuard dg(h->device);
  HIP_TRY(hipMemcpy(h->d_buf, img.data(), h->buf_bytes, hipMemcpyHostToDevice));
  h->route = fast ? 1 : 0;
  h->args.fast = h->route;
  h->weights_set = true;
  set_name(h);
  return DFX_OK;
}

int dfx_imgconv_submit(dfx_imgconv_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s) {
  if (!h || !src_dev || !dst_dev) return fail(DFX_ERR_INVALID, "imgconv_submit: null argument");
  if ((uintptr_t)dst_dev % 16) return fail(DFX_ERR_INVALID, "imgconv_submit: dst must be 16-byte aligned");
  if (!h->weights_set) return fail(DFX_ERR_STATE, "imgconv_submit: dfx_imgconv_set_weights not called");
  DeviceGuard dg(h->device);
  IcArgs a = h->args;  // per-launch copy: concurrent submits on several streams are independent
  a.src = (const unsigned char *)src_dev;
  a.dst = (unsigned char *)dst_dev;
  const int rc = h->path == DFX_IMGCONV_MFMA ? launch_imgconv_mfma(a, h->grid, h->lds, (hipStream_t)s, 0, a.fast != 0)
                                             : launch_imgconv_generic(a, h->grid, (hipStream_t)s);
  if (rc != 0) return fail(DFX_ERR_UNSUPPORTED, "imgconv_submit: no kernel instance for this op");
  HIP_TRY(hipGetLastError());
  return DFX_OK;
}

int dfx_imgconv_submit_host(dfx_imgconv_t *h, const void *src_host, void *dst_host) {
  if (!h || !src_host || !dst_host) return fail(DFX_ERR_INVALID, "imgconv_submit_host: null argument");
  if (!h->weights_set) return fail(DFX_ERR_STATE, "imgconv_submit_host: dfx_imgconv_set_weights not called");
  DeviceGuard dg(h->device);
  return h->host.run(src_host, src_bytes(h->d), dst_host, dst_bytes(h->d),
                     [h](const void *s, void *d, dfx_stream_t st) { return dfx_imgconv_submit(h, s, d, st); });
}

int dfx_imgconv_query(const dfx_imgconv_t *h, dfx_imgconv_info *info) {
  if (!h || !info) return fail(DFX_ERR_INVALID, "imgconv_query: null argument");
  memset(info, 0, sizeof(*info));
  info->path = h->path;
  info->grid = h->grid;
  info->block = h->block;
  info->lds_bytes = h->lds;
  info->device = h->device;
  const dfx_imgconv_desc &d = h->d;
  const uint64_t outs = (uint64_t)d.bs * d.oh * d.ow * d.oc;
  info->algorithmic_ops = 2 * outs * d.kh * d.kw * d.ic;
  info->algorithmic_bytes = (uint64_t)src_bytes(d) + (uint64_t)wei_count(d) + (uint64_t)dst_bytes(d);
  memcpy(info->kernel_name, h->kernel_name, sizeof(info->kernel_name));
  return DFX_OK;
}

// test hook: the requant route the last dfx_imgconv_set_weights proved (numbering of dfx_debug_conv_requant)
int dfx_debug_imgconv_requant(const dfx_imgconv_t *h, int32_t out[1]) {
  if (!h || !out) return fail(DFX_ERR_INVALID, "imgconv_requant: null argument");
  if (!h->weights_set) return fail(DFX_ERR_STATE, "imgconv_requant: dfx_imgconv_set_weights not called");
  out[0] = h->route;
  return DFX_OK;
}

int dfx_imgconv_destroy(dfx_imgconv_t *h) {
  release(h);
  return DFX_OK;
}

}  // extern "C"
