// gconv_api.hip -- host side of the grouped conv op (dfx_gconv_* of include/dfx.h): descriptor validation, choice of
// the path and of the launch geometry, weight packing for the MFMA kernel (gconv.cuh, gconv_pack.h), and the requant
// route's proof from the actual weights, bias and scales.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "dfx_internal.h"
#include "gconv.cuh"
#include "gconv_pack.h"
#include "requant_host.h"

namespace dfx {
int launch_gconv_mfma(const GcArgs &, int grid, int lds, hipStream_t, int mode, bool fast);
int launch_gconv_generic(const GcArgs &, int grid, hipStream_t);
}
using namespace dfx;

struct dfx_gconv {
  dfx_gconv_desc d;
  int device = 0;
  int path = 0;
  int grid = 0, block = 0, lds = 0;
  GcArgs args = {};                // everything but src / dst; copied per launch
  unsigned char *d_buf = nullptr;  // packed weights | raw weights | comp | bias | scale
  size_t off_wraw = 0, off_comp = 0, off_bias = 0, off_scale = 0, buf_bytes = 0;
  bool weights_set = false;
  int route = 0;                   // 0 exact, 1 fast (dfx_debug_conv_requant's numbering)
  HostStaging host;                // dfx_gconv_submit_host
  char kernel_name[96] = "";
};

namespace {

int validate_gconv(const dfx_gconv_desc &d) {
  if (d.bs <= 0 || d.ic <= 0 || d.ih <= 0 || d.iw <= 0 || d.oc <= 0 || d.oh <= 0 || d.ow <= 0 || d.kh <= 0 || d.kw <= 0)
    return fail(DFX_ERR_INVALID, "gconv: non-positive dimension");
  if (d.sh <= 0 || d.sw <= 0) return fail(DFX_ERR_INVALID, "gconv: non-positive stride");
  if (d.pad_t < 0 || d.pad_l < 0) return fail(DFX_ERR_INVALID, "gconv: negative padding");
  if (d.groups < 1) return fail(DFX_ERR_INVALID, "gconv: groups must be at least 1");
  if (d.ic % d.groups || d.oc % d.groups)
    return fail(DFX_ERR_INVALID, "gconv: ic %d and oc %d must be divisible by groups %d", d.ic, d.oc, d.groups);
  if ((long long)d.kh * d.kw * (d.ic / d.groups) > 65025)
    return fail(DFX_ERR_INVALID, "gconv: kh * kw * ic / groups beyond 65025 (the accumulator could leave s32)");
  if ((long long)(d.oh - 1) * d.sh - d.pad_t > d.ih - 1 || (long long)(d.ow - 1) * d.sw - d.pad_l > d.iw - 1)
    return fail(DFX_ERR_INVALID, "gconv: the last output row / column's window starts outside the input");
  if ((long long)d.bs * d.ih * d.iw >= (1ll << 31) || (long long)d.bs * d.oh * d.ow >= (1ll << 31))
    return fail(DFX_ERR_INVALID, "gconv: pixel count beyond 2^31");
  if (d.dst_dt < DFX_F32 || d.dst_dt > DFX_U8) return fail(DFX_ERR_INVALID, "gconv: bad dst dtype");
  if (d.bia_dt != DFX_UNDEF && (d.bia_dt < DFX_F32 || d.bia_dt > DFX_U8)) return fail(DFX_ERR_INVALID, "gconv: bad bias dtype");
  if (d.round_mode != DFX_ROUND_NEAREST && d.round_mode != DFX_ROUND_DOWN) return fail(DFX_ERR_INVALID, "gconv: bad round mode");
  if (d.nscales != 1 && d.nscales != d.oc) return fail(DFX_ERR_INVALID, "gconv: scales count must be 1 or oc");
  if (d.force_path != -1 && d.force_path != DFX_GCONV_MFMA && d.force_path != DFX_GCONV_GENERIC)
    return fail(DFX_ERR_INVALID, "gconv: bad force_path");
  return DFX_OK;
}

// the shape class of gconv.cuh
bool mfma_class(const dfx_gconv_desc &d) {
  const long long lim = 1ll << 31;  // one image below 2^31 bytes on either side (the kernel's offsets are 64-bit)
  const int cpg = d.ic / d.groups;
  return d.kh == 3 && d.kw == 3 && d.sh == d.sw && (d.sh == 1 || d.sh == 2) && d.ic == d.oc && d.ic % 32 == 0 &&
         (cpg == 4 || cpg == 8 || cpg == 16 || cpg == 32 || cpg == 64) && (long long)d.ih * d.iw * d.ic < lim &&
         (long long)d.oh * d.ow * d.oc * (long long)dt_size(d.dst_dt) < lim;
}

void set_name(dfx_gconv *h) {
  const dfx_gconv_desc &d = h->d;
  if (h->path == DFX_GCONV_MFMA)
    snprintf(h->kernel_name, sizeof(h->kernel_name), "gconv_mfma%s<%dx%d,s%d,cpg%d,%s> %s", h->args.t_tr > 0 ? "_tile" : "", d.kh,
             d.kw, d.sh, d.ic / d.groups, dt_name(d.dst_dt), !h->weights_set ? "(no weights)" : h->route ? "fast" : "exact");
  else
    snprintf(h->kernel_name, sizeof(h->kernel_name), "gconv_generic<%dx%d,s%dx%d,cpg%d,%s> exact", d.kh, d.kw, d.sh, d.sw,
             d.ic / d.groups, dt_name(d.dst_dt));
}

void release(dfx_gconv *h) {
  if (!h) return;
  DeviceGuard dg(h->device);
  (void)hipFree(h->d_buf);
  h->host.release();
  delete h;
}

size_t src_bytes(const dfx_gconv_desc &d) { return (size_t)d.bs * d.ih * d.iw * d.ic; }
size_t dst_bytes(const dfx_gconv_desc &d) { return (size_t)d.bs * d.oh * d.ow * d.oc * dt_size(d.dst_dt); }
size_t wei_count(const dfx_gconv_desc &d) { return (size_t)d.oc * (d.ic / d.groups) * d.kh * d.kw; }

}  // namespace

extern "C" {

int dfx_gconv_create(const dfx_gconv_desc *desc, dfx_gconv_t **out) {
  if (!desc || !out) return fail(DFX_ERR_INVALID, "gconv_create: null argument");
  *out = nullptr;
  const dfx_gconv_desc &d = *desc;
  int rc = validate_gconv(d);
  if (rc) return rc;
  const bool covered = mfma_class(d);
  if (d.force_path == DFX_GCONV_MFMA && !covered)
    return fail(DFX_ERR_UNSUPPORTED, "gconv_create: shape outside the MFMA kernel's class (3x3, stride (1,1) or (2,2), ic == oc a multiple of 32, ic / groups in {4, 8, 16, 32, 64}, one image below 2^31 bytes)");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(DFX_ERR_NO_DEVICE, "gconv_create: no HIP device (this library has no CPU path)");
  dfx_gconv *h = new (std::nothrow) dfx_gconv();
  if (!h) return fail(DFX_ERR_HIP, "out of host memory");
  h->d = d;
  if (hipGetDevice(&h->device) != hipSuccess) h->device = 0;
  h->path = (covered && d.force_path != DFX_GCONV_GENERIC) ? DFX_GCONV_MFMA : DFX_GCONV_GENERIC;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, h->device) != hipSuccess) {
    release(h);
    return fail(DFX_ERR_HIP, "gconv_create: cannot query the device");
  }
  const int cus = std::max(1, prop.multiProcessorCount);
  GcArgs &a = h->args;
  a.bs = d.bs; a.ic = d.ic; a.ih = d.ih; a.iw = d.iw; a.oc = d.oc; a.oh = d.oh; a.ow = d.ow; a.groups = d.groups;
  a.kh = d.kh; a.kw = d.kw; a.sh = d.sh; a.sw = d.sw; a.pt = d.pad_t; a.pl = d.pad_l;
  a.dst_dt = d.dst_dt; a.relu = (d.relu || d.dst_dt == DFX_U8) ? 1 : 0; a.rm = d.round_mode;
  a.px_total = (int)((long long)d.bs * d.oh * d.ow);
  size_t wpk_bytes = 0;
  if (h->path == DFX_GCONV_MFMA) {
    const int cpg = d.ic / d.groups, nib = gconv_pack_nib(cpg);
    a.cblocks = d.oc / 32;
    a.nchunks = (a.cblocks + GC_CHUNK - 1) / GC_CHUNK;
    a.wblocks = std::min(GC_CHUNK, a.cblocks);
    a.strips = (a.px_total + 31) / 32;
    wpk_bytes = gconv_pack_bytes(d.oc, cpg);
    h->block = GC_THREADS;
    h->lds = a.wblocks * 9 * nib * 1024 + 3 * 32 * GC_CHUNK * 4 + (GC_THREADS / 64) * GC_STAGE_BYTES;
    // Launch: the workgroups that are resident at once (LDS: two per CU, one at cpg 64), a multiple of the chunk count;
    // a workgroup keeps its chunk's weights in LDS and its 8 waves stride over the strips.  Fewer workgroups than
    // (chunk, slot) units (tiny devices, DFX_GCONV_GRID) make the workgroups loop over the units.
    const int wg_strips = GC_THREADS / 64;
    const long long cap = (long long)cus * (nib == 2 ? 1 : 2);
    long long slots = std::min<long long>((a.strips + wg_strips - 1) / wg_strips, std::max<long long>(1, cap / a.nchunks));
    long long grid = slots * a.nchunks;
    if (const char *e = tuning_value("DFX_GCONV_TILE"); e && atoi(e) != 0) {
      // The variant that stages the input in LDS (gconv_mfma_tile_kernel), kept for the A/B of DESIGN 4.9.  An item is
      // a band of tr output rows x a block of tc <= 64 output columns of one image, about 256 pixels (one strip per
      // wave), shrunk until its halo fits in what a CU's 160 KB of LDS leave (4 KB kept free).
      const int S = d.sh, pp = 32 * a.wblocks + 16;
      const long long room = 156 * 1024 - h->lds;
      auto halo = [&](int tr, int tc) { return (long long)((tr - 1) * S + 3) * ((tc - 1) * S + 3) * pp; };
      int tc = std::min(d.ow, 64);
      while (tc > 1 && halo(1, tc) > room) tc = (tc + 1) / 2;
      int tr = std::max(1, std::min(d.oh, 256 / tc));
      while (tr > 1 && halo(tr, tc) > room) --tr;
      if (halo(tr, tc) <= room) {
        a.t_tr = tr; a.t_tc = tc; a.t_ir = (tr - 1) * S + 3; a.t_ic = (tc - 1) * S + 3; a.t_pp = pp;
        a.t_nbands = (d.oh + tr - 1) / tr; a.t_ncb = (d.ow + tc - 1) / tc;
        a.t_items = (int)((long long)d.bs * a.t_nbands * a.t_ncb);  // <= bs * oh * ow
        h->lds += (int)halo(tr, tc);
        const long long cap_t = (long long)cus * std::max(1, 160 * 1024 / h->lds);
        slots = std::min<long long>(a.t_items, std::max<long long>(1, cap_t / a.nchunks));
        grid = slots * a.nchunks;
      }
    }
    if (const char *e = tuning_value("DFX_GCONV_GRID")) {  // testing aid
      grid = std::max(1ll, std::min(grid, (long long)atoi(e)));
      slots = (grid + a.nchunks - 1) / a.nchunks;
    }
    a.slots = (int)slots;
    h->grid = (int)grid;
    // both routes' instances: set_weights may switch between them later
    if (launch_gconv_mfma(a, h->grid, h->lds, nullptr, 1, false) != 0 || launch_gconv_mfma(a, h->grid, h->lds, nullptr, 1, true) != 0) {
      release(h);
      return fail(DFX_ERR_HIP, "gconv_create: cannot reserve %d bytes of LDS", h->lds);
    }
  } else {
    a.items = (long long)a.px_total * d.oc;
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
    return fail(DFX_ERR_HIP, "gconv_create: weight buffer: %s", hipGetErrorString(e));
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

int dfx_gconv_set_weights(dfx_gconv_t *h, const int8_t *wei, const void *bia, const float *scales) {
  if (!h || !wei || !scales) return fail(DFX_ERR_INVALID, "gconv_set_weights: null argument");
  const dfx_gconv_desc &d = h->d;
  if (d.bia_dt != DFX_UNDEF && !bia) return fail(DFX_ERR_INVALID, "gconv_set_weights: null bias");
  const size_t taps = (size_t)(d.ic / d.groups) * d.kh * d.kw;  // of one output channel
  std::vector<unsigned char> img(h->buf_bytes, 0);
  int *comp = (int *)(img.data() + h->off_comp);
  float *fb = (float *)(img.data() + h->off_bias), *fs = (float *)(img.data() + h->off_scale);
  memcpy(img.data() + h->off_wraw, wei, wei_count(d));
  const bool proven = requant_consts(d.oc, taps, [&](int k, size_t i) { return wei[(size_t)k * taps + i]; }, bia, d.bia_dt, scales,
                                     d.nscales, comp, fb, fs);
  const bool fast = h->path == DFX_GCONV_MFMA && d.round_mode == DFX_ROUND_NEAREST && proven && fast_allowed();
  if (h->path == DFX_GCONV_MFMA) gconv_pack(wei, d.oc, d.ic / d.groups, img.data());
  DeviceGuard dg(h->device);
  HIP_TRY(hipMemcpy(h->d_buf, img.data(), h->buf_bytes, hipMemcpyHostToDevice));
  h->route = fast ? 1 : 0;
  h->args.fast = h->route;
  h->weights_set = true;
  set_name(h);
  return DFX_OK;
}

int dfx_gconv_submit(dfx_gconv_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s) {
  if (!h || !src_dev || !dst_dev) return fail(DFX_ERR_INVALID, "gconv_submit: null argument");
  if (((uintptr_t)src_dev | (uintptr_t)dst_dev) % 16)
    return fail(DFX_ERR_INVALID, "gconv_submit: src and dst must be 16-byte aligned");
  if (!h->weights_set) return fail(DFX_ERR_STATE, "gconv_submit: dfx_gconv_set_weights not called");
  DeviceGuard dg(h->device);
  GcArgs a = h->args;  // per-launch copy: concurrent submits on several streams are independent
  a.src = (const unsigned char *)src_dev;
  a.dst = (unsigned char *)dst_dev;
  const int rc = h->path == DFX_GCONV_MFMA ? launch_gconv_mfma(a, h->grid, h->lds, (hipStream_t)s, 0, a.fast != 0)
                                           : launch_gconv_generic(a, h->grid, (hipStream_t)s);
  if (rc != 0) return fail(DFX_ERR_UNSUPPORTED, "gconv_submit: no kernel instance for this op");
  HIP_TRY(hipGetLastError());
  return DFX_OK;
}

int dfx_gconv_submit_host(dfx_gconv_t *h, const void *src_host, void *dst_host) {
  if (!h || !src_host || !dst_host) return fail(DFX_ERR_INVALID, "gconv_submit_host: null argument");
  if (!h->weights_set) return fail(DFX_ERR_STATE, "gconv_submit_host: dfx_gconv_set_weights not called");
  DeviceGuard dg(h->device);
  return h->host.run(src_host, src_bytes(h->d), dst_host, dst_bytes(h->d),
                     [h](const void *s, void *d, dfx_stream_t st) { return dfx_gconv_submit(h, s, d, st); });
}

int dfx_gconv_query(const dfx_gconv_t *h, dfx_gconv_info *info) {
  if (!h || !info) return fail(DFX_ERR_INVALID, "gconv_query: null argument");
  memset(info, 0, sizeof(*info));
  info->path = h->path;
  info->grid = h->grid;
  info->block = h->block;
  info->lds_bytes = h->lds;
  info->device = h->device;
  const dfx_gconv_desc &d = h->d;
  const uint64_t outs = (uint64_t)d.bs * d.oh * d.ow * d.oc;
  info->algorithmic_ops = 2 * outs * d.kh * d.kw * (d.ic / d.groups);
  info->algorithmic_bytes = (uint64_t)src_bytes(d) + (uint64_t)wei_count(d) + (uint64_t)dst_bytes(d);
  memcpy(info->kernel_name, h->kernel_name, sizeof(info->kernel_name));
  return DFX_OK;
}

// test hook: the requant route the last dfx_gconv_set_weights proved (numbering of dfx_debug_conv_requant)
int dfx_debug_gconv_requant(const dfx_gconv_t *h, int32_t out[1]) {
  if (!h || !out) return fail(DFX_ERR_INVALID, "gconv_requant: null argument");
  if (!h->weights_set) return fail(DFX_ERR_STATE, "gconv_requant: dfx_gconv_set_weights not called");
  out[0] = h->route;
  return DFX_OK;
}

int dfx_gconv_destroy(dfx_gconv_t *h) {
  release(h);
  return DFX_OK;
}

}  // extern "C"
