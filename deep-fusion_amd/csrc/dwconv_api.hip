// dwconv_api.hip -- host side of the depthwise conv op (dfx_dwconv_* of include/dfx.h): descriptor validation, choice
// of the path and of the launch geometry, weight packing for the sliding-window kernel (dwconv.cuh), and the requant
// route's proof from the actual weights, bias and scales.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "dfx_internal.h"
#include "dwconv.cuh"
#include "requant_host.h"

namespace dfx {
int launch_dwconv_window(const DwArgs &, int grid, int block, int lds, hipStream_t);
int launch_dwconv_generic(const DwArgs &, int grid, hipStream_t);
}
using namespace dfx;

struct dfx_dwconv {
  dfx_dwconv_desc d;
  int device = 0;
  int path = 0;
  int grid = 0, block = 0, lds = 0;
  DwArgs args = {};                // everything but src / dst; copied per launch
  unsigned char *d_buf = nullptr;  // packed weights | raw weights | comp | bias | scale
  size_t off_wraw = 0, off_comp = 0, off_bias = 0, off_scale = 0, buf_bytes = 0;
  bool weights_set = false;
  int route = 0;                   // 0 exact, 1 fast (dfx_debug_conv_requant's numbering)
  HostStaging host;                // dfx_dwconv_submit_host
  char kernel_name[96] = "";
};

namespace {

int validate_dwconv(const dfx_dwconv_desc &d) {
  if (d.bs <= 0 || d.c <= 0 || d.ih <= 0 || d.iw <= 0 || d.oh <= 0 || d.ow <= 0)
    return fail(DFX_ERR_INVALID, "dwconv: non-positive dimension");
  if (d.kh <= 0 || d.kw <= 0 || d.kh > 255 || d.kw > 255)
    return fail(DFX_ERR_INVALID, "dwconv: window %d x %d outside 1 .. 255", d.kh, d.kw);
  if (d.sh <= 0 || d.sw <= 0) return fail(DFX_ERR_INVALID, "dwconv: non-positive stride");
  if (d.pad_t < 0 || d.pad_l < 0) return fail(DFX_ERR_INVALID, "dwconv: negative padding");
  if ((long long)(d.oh - 1) * d.sh - d.pad_t > d.ih - 1 || (long long)(d.ow - 1) * d.sw - d.pad_l > d.iw - 1)
    return fail(DFX_ERR_INVALID, "dwconv: the last output row / column's window starts outside the input");
  if ((long long)d.bs * d.ih * d.iw >= (1ll << 31) || (long long)d.bs * d.oh * d.ow >= (1ll << 31))
    return fail(DFX_ERR_INVALID, "dwconv: pixel count beyond 2^31");
  if (d.dst_dt < DFX_F32 || d.dst_dt > DFX_U8) return fail(DFX_ERR_INVALID, "dwconv: bad dst dtype");
  if (d.bia_dt != DFX_UNDEF && (d.bia_dt < DFX_F32 || d.bia_dt > DFX_U8)) return fail(DFX_ERR_INVALID, "dwconv: bad bias dtype");
  if (d.round_mode != DFX_ROUND_NEAREST && d.round_mode != DFX_ROUND_DOWN) return fail(DFX_ERR_INVALID, "dwconv: bad round mode");
  if (d.nscales != 1 && d.nscales != d.c) return fail(DFX_ERR_INVALID, "dwconv: scales count must be 1 or c");
  if (d.force_path != -1 && d.force_path != DFX_DWCONV_WINDOW && d.force_path != DFX_DWCONV_GENERIC)
    return fail(DFX_ERR_INVALID, "dwconv: bad force_path");
  return DFX_OK;
}

// the shape class of dwconv.cuh
bool window_class(const dfx_dwconv_desc &d) {
  const long long lim = (1ll << 31) - 64;
  return d.kh == d.kw && (d.kh == 3 || d.kh == 5) && d.sh == d.sw && (d.sh == 1 || d.sh == 2) && d.c % 16 == 0 &&
         (long long)d.ih * d.iw * d.c < lim && (long long)d.oh * d.ow * d.c * (long long)dt_size(d.dst_dt) < lim;
}

void set_name(dfx_dwconv *h) {
  const dfx_dwconv_desc &d = h->d;
  if (h->path == DFX_DWCONV_WINDOW)
    snprintf(h->kernel_name, sizeof(h->kernel_name), "dwconv_window<%dx%d,s%d,%s> band %d %s", d.kh, d.kw, d.sh,
             dt_name(d.dst_dt), h->args.band, !h->weights_set ? "(no weights)" : h->route ? "fast" : "exact");
  else
    snprintf(h->kernel_name, sizeof(h->kernel_name), "dwconv_generic<%dx%d,s%dx%d,%s> exact", d.kh, d.kw, d.sh, d.sw,
             dt_name(d.dst_dt));
}

void release(dfx_dwconv *h) {
  if (!h) return;
  DeviceGuard dg(h->device);
  (void)hipFree(h->d_buf);
  h->host.release();
  delete h;
}

size_t src_bytes(const dfx_dwconv_desc &d) { return (size_t)d.bs * d.ih * d.iw * d.c; }
size_t dst_bytes(const dfx_dwconv_desc &d) { return (size_t)d.bs * d.oh * d.ow * d.c * dt_size(d.dst_dt); }

}  // namespace

bool dfx::dwconv_window_view(const dfx_dwconv *h, DwArgs *args) {  // (declared in dfx_internal.h)
  if (!h || h->path != DFX_DWCONV_WINDOW || !h->weights_set) return false;
  *args = h->args;
  return true;
}

extern "C" {

int dfx_dwconv_create(const dfx_dwconv_desc *desc, dfx_dwconv_t **out) {
  if (!desc || !out) return fail(DFX_ERR_INVALID, "dwconv_create: null argument");
  *out = nullptr;
  const dfx_dwconv_desc &d = *desc;
  int rc = validate_dwconv(d);
  if (rc) return rc;
  const bool covered = window_class(d);
  if (d.force_path == DFX_DWCONV_WINDOW && !covered)
    return fail(DFX_ERR_UNSUPPORTED, "dwconv_create: shape outside the window kernel's class (3x3 or 5x5, stride 1 or 2, c %% 16 == 0, one image below 2^31 bytes)");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(DFX_ERR_NO_DEVICE, "dwconv_create: no HIP device (this library has no CPU path)");
  dfx_dwconv *h = new (std::nothrow) dfx_dwconv();
  if (!h) return fail(DFX_ERR_HIP, "out of host memory");
  h->d = d;
  if (hipGetDevice(&h->device) != hipSuccess) h->device = 0;
  h->path = (covered && d.force_path != DFX_DWCONV_GENERIC) ? DFX_DWCONV_WINDOW : DFX_DWCONV_GENERIC;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, h->device) != hipSuccess) {
    release(h);
    return fail(DFX_ERR_HIP, "dwconv_create: cannot query the device");
  }
  const int cus = std::max(1, prop.multiProcessorCount);
  DwArgs &a = h->args;
  a.bs = d.bs; a.c = d.c; a.ih = d.ih; a.iw = d.iw; a.oh = d.oh; a.ow = d.ow; a.kh = d.kh; a.kw = d.kw;
  a.sh = d.sh; a.sw = d.sw; a.pt = d.pad_t; a.pl = d.pad_l;
  a.dst_dt = d.dst_dt; a.relu = (d.relu || d.dst_dt == DFX_U8) ? 1 : 0; a.rm = d.round_mode;
  const size_t taps = (size_t)d.kh * d.kw;
  size_t wpk_bytes = 0;
  if (h->path == DFX_DWCONV_WINDOW) {
    const int K = d.kh, ndw = K == 3 ? 1 : 2;
    a.groups = d.c / 16;
    // Launch: at most 4 workgroups of 256 lanes per CU (two are resident at the kernel's register count), lanes loop
    // over their work items.  Band: the output rows one lane slides over.  The K - S halo rows of a band are read
    // again by the band below, (K - S) / (band * S) of the input: 1/8 at 16 rows (3x3 stride 1), 1/4 at 8, 1/2 at
    // 4.  The largest band that still gives every lane of the launch a work item; 4 for tensors too small for that.
    const long long cap_blocks = (long long)cus * 4;
    int band = 16;
    while (band > 4 && (long long)d.bs * ((d.oh + band - 1) / band) * d.ow * a.groups < cap_blocks * DW_THREADS) band /= 2;
    if (const char *e = tuning_value("DFX_DWCONV_BAND")) band = std::max(1, std::min(atoi(e), 1 << 20));  // testing aid
    // (a band beyond oh is harmless: nbands is then 1, so the kernel's oy0 = band index * band is 0 and its nrows is
    // cut to oh - oy0; band itself never enters a product that could leave an int)
    a.band = band;
    a.nbands = (d.oh + band - 1) / band;
    a.items = (long long)d.bs * a.nbands * d.ow;
    // 5x5: weights and constants in LDS, one slot per channel group where a block's lanes share groups
    h->block = DW_THREADS;
    if (K == 5) {
      a.slot_by_group = a.groups <= 64;
      if (!a.slot_by_group) h->block = 64;
      h->lds = DW_LDS_ROWS * (a.slot_by_group ? a.groups : 64) * 16;
    } else {
      h->lds = 0;
    }
    // lanes: one per (item, group) at most, a multiple of groups, at least one item's
    const long long lanes = a.items * a.groups;
    long long blocks = std::min((lanes + h->block - 1) / h->block, cap_blocks * (DW_THREADS / h->block));
    if (const char *e = tuning_value("DFX_DWCONV_GRID")) blocks = std::max(1ll, std::min(blocks, (long long)atoi(e)));  // testing aid
    blocks = std::max(blocks, ((long long)a.groups + h->block - 1) / h->block);
    h->grid = (int)blocks;
    a.threads = std::min(lanes, blocks * h->block / a.groups * a.groups);
    wpk_bytes = (size_t)a.groups * K * ndw * 16 * 4;
  } else {
    a.items = (long long)d.bs * d.oh * d.ow * d.c;
    h->block = 256;
    h->lds = 0;
    h->grid = (int)std::min((a.items + 255) / 256, (long long)cus * 8);
  }
  h->off_wraw = round16(wpk_bytes);
  h->off_comp = h->off_wraw + round16((size_t)d.c * taps);
  h->off_bias = h->off_comp + round16((size_t)d.c * 4);
  h->off_scale = h->off_bias + round16((size_t)d.c * 4);
  h->buf_bytes = h->off_scale + round16((size_t)d.c * 4);
  hipError_t e = hipMalloc((void **)&h->d_buf, h->buf_bytes);
  if (e != hipSuccess) {
    release(h);
    return fail(DFX_ERR_HIP, "dwconv_create: weight buffer: %s", hipGetErrorString(e));
  }
  a.wpk = (const unsigned *)h->d_buf;
  a.wraw = (const signed char *)(h->d_buf + h->off_wraw);
  a.comp = (const int *)(h->d_buf + h->off_comp);
  a.bias = (const float *)(h->d_buf + h->off_bias);
  a.scale = (const float *)(h->d_buf + h->off_scale);
  set_name(h);
  *out = h;
  return DFX_OK;
}

int dfx_dwconv_set_weights(dfx_dwconv_t *h, const int8_t *wei, const void *bia, const float *scales) {
  if (!h || !wei || !scales) return fail(DFX_ERR_INVALID, "dwconv_set_weights: null argument");
  const dfx_dwconv_desc &d = h->d;
  if (d.bia_dt != DFX_UNDEF && !bia) return fail(DFX_ERR_INVALID, "dwconv_set_weights: null bias");
  const int taps = d.kh * d.kw;
  std::vector<unsigned char> img(h->buf_bytes, 0);
  int *comp = (int *)(img.data() + h->off_comp);
  float *fb = (float *)(img.data() + h->off_bias), *fs = (float *)(img.data() + h->off_scale);
  memcpy(img.data() + h->off_wraw, wei, (size_t)d.c * taps);
  const bool proven = requant_consts(d.c, taps, [&](int k, size_t i) { return wei[(size_t)k * taps + i]; }, bia, d.bia_dt, scales,
                                     d.nscales, comp, fb, fs);
  const bool fast = h->path == DFX_DWCONV_WINDOW && d.round_mode == DFX_ROUND_NEAREST && proven && fast_allowed();
  if (h->path == DFX_DWCONV_WINDOW) {
    // [group][ky][dword of the row][channel of the group]: bytes = the row's taps kx = 4 * dword .. + 3, zero past K
    const int K = d.kh, ndw = K == 3 ? 1 : 2;
    unsigned *wpk = (unsigned *)img.data();
    for (int k = 0; k < d.c; ++k)
      for (int ky = 0; ky < K; ++ky)
        for (int j = 0; j < ndw; ++j) {
          unsigned v = 0;
          for (int b = 0; b < 4; ++b) {
            const int kx = 4 * j + b;
            if (kx < K) v |= (unsigned)(uint8_t)wei[((size_t)k * K + ky) * K + kx] << (8 * b);
          }
          wpk[(((size_t)(k / 16) * K + ky) * ndw + j) * 16 + k % 16] = v;
        }
  }
  DeviceGuard dg(h->device);
  HIP_TRY(hipMemcpy(h->d_buf, img.data(), h->buf_bytes, hipMemcpyHostToDevice));
  h->route = fast ? 1 : 0;
  h->args.fast = h->route;
  h->weights_set = true;
  set_name(h);
  return DFX_OK;
}

int dfx_dwconv_submit(dfx_dwconv_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s) {
  if (!h || !src_dev || !dst_dev) return fail(DFX_ERR_INVALID, "dwconv_submit: null argument");
  if (((uintptr_t)src_dev | (uintptr_t)dst_dev) % 16)
    return fail(DFX_ERR_INVALID, "dwconv_submit: src and dst must be 16-byte aligned");
  if (!h->weights_set) return fail(DFX_ERR_STATE, "dwconv_submit: dfx_dwconv_set_weights not called");
  DeviceGuard dg(h->device);
  DwArgs a = h->args;  // per-launch copy: concurrent submits on several streams are independent
  a.src = (const unsigned char *)src_dev;
  a.dst = (unsigned char *)dst_dev;
  const int rc = h->path == DFX_DWCONV_WINDOW ? launch_dwconv_window(a, h->grid, h->block, h->lds, (hipStream_t)s)
                                              : launch_dwconv_generic(a, h->grid, (hipStream_t)s);
  if (rc != 0) return fail(DFX_ERR_UNSUPPORTED, "dwconv_submit: no kernel instance for this op");
  HIP_TRY(hipGetLastError());
  return DFX_OK;
}

int dfx_dwconv_submit_host(dfx_dwconv_t *h, const void *src_host, void *dst_host) {
  if (!h || !src_host || !dst_host) return fail(DFX_ERR_INVALID, "dwconv_submit_host: null argument");
  if (!h->weights_set) return fail(DFX_ERR_STATE, "dwconv_submit_host: dfx_dwconv_set_weights not called");
  DeviceGuard dg(h->device);
  return h->host.run(src_host, src_bytes(h->d), dst_host, dst_bytes(h->d),
                     [h](const void *s, void *d, dfx_stream_t st) { return dfx_dwconv_submit(h, s, d, st); });
}

int dfx_dwconv_query(const dfx_dwconv_t *h, dfx_dwconv_info *info) {
  if (!h || !info) return fail(DFX_ERR_INVALID, "dwconv_query: null argument");
  memset(info, 0, sizeof(*info));
  info->path = h->path;
  info->grid = h->grid;
  info->block = h->block;
  info->lds_bytes = h->lds;
  info->device = h->device;
  const dfx_dwconv_desc &d = h->d;
  const uint64_t outs = (uint64_t)d.bs * d.oh * d.ow * d.c;
  info->algorithmic_ops = 2 * outs * d.kh * d.kw;
  info->algorithmic_bytes = (uint64_t)src_bytes(d) + (uint64_t)d.c * d.kh * d.kw + (uint64_t)dst_bytes(d);
  memcpy(info->kernel_name, h->kernel_name, sizeof(info->kernel_name));
  return DFX_OK;
}

// test hook: the requant route the last dfx_dwconv_set_weights proved (numbering of dfx_debug_conv_requant)
int dfx_debug_dwconv_requant(const dfx_dwconv_t *h, int32_t out[1]) {
  if (!h || !out) return fail(DFX_ERR_INVALID, "dwconv_requant: null argument");
  if (!h->weights_set) return fail(DFX_ERR_STATE, "dwconv_requant: dfx_dwconv_set_weights not called");
  out[0] = h->route;
  return DFX_OK;
}

int dfx_dwconv_destroy(dfx_dwconv_t *h) {
  release(h);
  return DFX_OK;
}

}  // extern "C"
