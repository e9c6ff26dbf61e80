// dilconv_api.hip -- host side of the dilated conv op (dfx_dilconv_* of include/dfx.h): descriptor validation, choice of
// the path, of the LDS plan (K-steps per weight slab, one or two slab buffers) and of the launch geometry, weight packing
// for the MFMA kernel (dilconv.cuh, dilconv_pack.h), and the requant route's proof from the actual weights, bias and
// scales (requant_host.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "dfx_internal.h"
#include "dilconv.cuh"
#include "dilconv_pack.h"
#include "requant_host.h"

namespace dfx {
int launch_dilconv_mfma(const DlArgs &, int grid, int lds, hipStream_t, int mode, bool fast);
int launch_dilconv_generic(const DlArgs &, int grid, hipStream_t);
}
using namespace dfx;

static_assert(DL_CHUNK == DL_PACK_CHUNK, "the kernel and the packer must agree on the chunk");

struct dfx_dilconv {
  dfx_dilconv_desc d;
  int device = 0;
  int path = 0;
  int grid = 0, block = 0, lds = 0;
  DlArgs args = {};                // everything but src / dst; copied per launch
  unsigned char *d_buf = nullptr;  // packed weights | raw weights | comp | bias | scale
  size_t off_wraw = 0, off_comp = 0, off_bias = 0, off_scale = 0, buf_bytes = 0;
  bool weights_set = false;
  int route = 0;                   // 0 exact, 1 fast (dfx_debug_conv_requant's numbering)
  HostStaging host;                // dfx_dilconv_submit_host
  char kernel_name[96] = "";
};

namespace {

constexpr int LDS_LIMIT = 160 * 1024;
constexpr int DEFAULT_SLAB = 3;    // K-steps per slab and strips per wave: DESIGN.md section 4.13, profiles/dilconv/
constexpr int DEFAULT_STRIPS = 1;

int validate_dilconv(const dfx_dilconv_desc &d) {
  if (d.bs <= 0 || d.ic <= 0 || d.ih <= 0 || d.iw <= 0 || d.oc <= 0 || d.oh <= 0 || d.ow <= 0 || d.kh <= 0 || d.kw <= 0)
    return fail(DFX_ERR_INVALID, "dilconv: non-positive dimension");
  if (d.kh > 255 || d.kw > 255) return fail(DFX_ERR_INVALID, "dilconv: window beyond 255");
  if (d.sh <= 0 || d.sw <= 0 || d.sh > 255 || d.sw > 255) return fail(DFX_ERR_INVALID, "dilconv: stride outside 1 .. 255");
  if (d.dh <= 0 || d.dw <= 0 || d.dh > 255 || d.dw > 255) return fail(DFX_ERR_INVALID, "dilconv: dilation outside 1 .. 255");
  if (d.pad_t < 0 || d.pad_l < 0) return fail(DFX_ERR_INVALID, "dilconv: negative padding");
  if (d.pad_t > (d.kh - 1) * d.dh || d.pad_l > (d.kw - 1) * d.dw) return fail(DFX_ERR_INVALID, "dilconv: padding beyond (k - 1) * dilation");
  if ((long long)d.kh * d.kw * d.ic > 65025)
    return fail(DFX_ERR_INVALID, "dilconv: kh * kw * ic beyond 65025 (the accumulator could leave s32)");
  if (((long long)d.oh - 1) * d.sh - d.pad_t > (long long)d.ih - 1 || ((long long)d.ow - 1) * d.sw - d.pad_l > (long long)d.iw - 1)
    return fail(DFX_ERR_INVALID, "dilconv: an output row / column starts below / right of the input");
  if ((long long)d.bs * d.ih * d.iw >= (1ll << 31) || (long long)d.bs * d.oh * d.ow >= (1ll << 31))
    return fail(DFX_ERR_INVALID, "dilconv: pixel count beyond 2^31");
  if (d.dst_dt < DFX_F32 || d.dst_dt > DFX_U8) return fail(DFX_ERR_INVALID, "dilconv: bad dst dtype");
  if (d.bia_dt != DFX_UNDEF && (d.bia_dt < DFX_F32 || d.bia_dt > DFX_U8)) return fail(DFX_ERR_INVALID, "dilconv: bad bias dtype");
  if (d.round_mode != DFX_ROUND_NEAREST && d.round_mode != DFX_ROUND_DOWN) return fail(DFX_ERR_INVALID, "dilconv: bad round mode");
  if (d.nscales != 1 && d.nscales != d.oc) return fail(DFX_ERR_INVALID, "dilconv: scales count must be 1 or oc");
  if (d.force_path != -1 && d.force_path != DFX_DILCONV_MFMA && d.force_path != DFX_DILCONV_GENERIC)
    return fail(DFX_ERR_INVALID, "dilconv: bad force_path");
  return DFX_OK;
}

// the shape class of dilconv.cuh: nothing in it depends on how large ic is
bool mfma_class(const dfx_dilconv_desc &d) {
  const long long lim = 1ll << 31;  // one image below 2^31 bytes on either side (the kernel's offsets are 64-bit)
  if (d.kh != 3 || d.kw != 3 || d.sh != 1 || d.sw != 1 || d.ic % 32 || d.oc % 32) return false;
  return (long long)d.ih * d.iw * d.ic < lim && (long long)d.oh * d.ow * d.oc * (long long)dt_size(d.dst_dt) < lim;
}

void set_name(dfx_dilconv *h) {
  const dfx_dilconv_desc &d = h->d;
  if (h->path == DFX_DILCONV_MFMA)
    snprintf(h->kernel_name, sizeof(h->kernel_name), "dilconv_mfma<3x3,d%dx%d,ic%d,oc%d,%s,slab%dx%d,r%d> %s", d.dh, d.dw, d.ic, d.oc,
             dt_name(d.dst_dt), h->args.slab, h->args.nbuf, h->args.rstrips, !h->weights_set ? "(no weights)" : h->route ? "fast" : "exact");
  else
    snprintf(h->kernel_name, sizeof(h->kernel_name), "dilconv_generic<%dx%d,s%dx%d,d%dx%d,ic%d,oc%d,%s> %s", d.kh, d.kw, d.sh, d.sw,
             d.dh, d.dw, d.ic, d.oc, dt_name(d.dst_dt), !h->weights_set ? "(no weights)" : "exact");
}

void release(dfx_dilconv *h) {
  if (!h) return;
  DeviceGuard dg(h->device);
  (void)hipFree(h->d_buf);
  h->host.release();
  delete h;
}

size_t src_bytes(const dfx_dilconv_desc &d) { return (size_t)d.bs * d.ih * d.iw * d.ic; }
size_t dst_bytes(const dfx_dilconv_desc &d) { return (size_t)d.bs * d.oh * d.ow * d.oc * dt_size(d.dst_dt); }
size_t wei_count(const dfx_dilconv_desc &d) { return (size_t)d.oc * d.ic * d.kh * d.kw; }

}  // namespace

extern "C" {

int dfx_dilconv_create(const dfx_dilconv_desc *desc, dfx_dilconv_t **out) {
  if (!desc || !out) return fail(DFX_ERR_INVALID, "dilconv_create: null argument");
  *out = nullptr;
  const dfx_dilconv_desc &d = *desc;
  int rc = validate_dilconv(d);
  if (rc) return rc;
  const bool covered = mfma_class(d);
  if (d.force_path == DFX_DILCONV_MFMA && !covered)
    return fail(DFX_ERR_UNSUPPORTED, "dilconv_create: shape outside the MFMA kernel's class (3x3 window; stride (1,1); ic and oc multiples of 32; one image below 2^31 bytes)");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(DFX_ERR_NO_DEVICE, "dilconv_create: no HIP device (this library has no CPU path)");
  dfx_dilconv *h = new (std::nothrow) dfx_dilconv();
  if (!h) return fail(DFX_ERR_HIP, "out of host memory");
  h->d = d;
  if (hipGetDevice(&h->device) != hipSuccess) h->device = 0;
  // AUTO RULE (include/dfx.h): the MFMA kernel everywhere in its class
  h->path = (covered && d.force_path != DFX_DILCONV_GENERIC) ? DFX_DILCONV_MFMA : DFX_DILCONV_GENERIC;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, h->device) != hipSuccess) {
    release(h);
    return fail(DFX_ERR_HIP, "dilconv_create: cannot query the device");
  }
  const int cus = std::max(1, prop.multiProcessorCount);
  DlArgs &a = h->args;
  a.bs = d.bs; a.ic = d.ic; a.ih = d.ih; a.iw = d.iw; a.oc = d.oc; a.oh = d.oh; a.ow = d.ow;
  a.kh = d.kh; a.kw = d.kw; a.sh = d.sh; a.sw = d.sw; a.dh = d.dh; a.dw = d.dw; a.pt = d.pad_t; a.pl = d.pad_l;
  a.dst_dt = d.dst_dt; a.relu = (d.relu || d.dst_dt == DFX_U8) ? 1 : 0; a.rm = d.round_mode;
  a.px_total = (int)((long long)d.bs * d.oh * d.ow);
  size_t wpk_bytes = 0;
  if (h->path == DFX_DILCONV_MFMA) {
    a.cblocks = d.oc / 32;
    a.ksteps = d.ic / 32;
    a.wblocks = std::min(DL_CHUNK, a.cblocks);
    a.nchunks = (a.cblocks + DL_CHUNK - 1) / DL_CHUNK;
    a.strips = (a.px_total + 31) / 32;
    // LDS plan: slab K-steps of the chunk per buffer; what LDS holds does not depend on ic (36 KB per K-step at 4
    // blocks: 3 K-steps at most).  A second buffer where two fit and there is more than one slab to stream.
    const int kstep_bytes = a.wblocks * DL_KSTEP;
    const int slab_max = (LDS_LIMIT - DL_FIXED_LDS) / kstep_bytes;  // >= 3
    int slab = DEFAULT_SLAB;
    if (const char *e = tuning_value("DFX_DILCONV_SLAB")) slab = atoi(e);
    a.slab = std::min(std::max(1, std::min(slab, slab_max)), a.ksteps);
    // ... and a thread's DL_WREG registers of 16 bytes hold its share of a slab (dilconv.cuh)
    a.nbuf = (a.slab < a.ksteps && 2 * a.slab * kstep_bytes + DL_FIXED_LDS <= LDS_LIMIT &&
              a.slab * kstep_bytes <= DL_WREG * DL_THREADS * 16) ? 2 : 1;
    a.rstrips = DEFAULT_STRIPS;
    if (const char *e = tuning_value("DFX_DILCONV_STRIPS")) a.rstrips = std::min(std::max(1, atoi(e)), DL_MAX_STRIPS);  // A/B aid
    wpk_bytes = dilconv_pack_bytes(d.oc, d.ic);
    h->block = DL_THREADS;
    h->lds = a.nbuf * a.slab * kstep_bytes + DL_FIXED_LDS;
    // Launch: the workgroups that are resident at once (by LDS, at most 4 per CU), a multiple of the chunk count; a
    // workgroup (a "slot" of its chunk) takes DL_WAVES * rstrips strips per pass over the chunk's weights and strides
    // over the strips.  Fewer workgroups than (chunk, slot) units (tiny devices, DFX_DILCONV_GRID) make the workgroups
    // loop over the units.
    const int wg_strips = DL_WAVES * a.rstrips;
    const long long cap = (long long)cus * std::min(4, std::max(1, LDS_LIMIT / h->lds));
    long long slots = std::min<long long>((a.strips + wg_strips - 1) / wg_strips, std::max<long long>(1, cap / a.nchunks));
    long long grid = slots * a.nchunks;
    if (const char *e = tuning_value("DFX_DILCONV_GRID")) {  // testing aid
      grid = std::max(1ll, std::min(grid, (long long)atoi(e)));
      slots = (grid + a.nchunks - 1) / a.nchunks;
    }
    a.slots = (int)slots;
    h->grid = (int)grid;
    // both routes' instances: set_weights may switch between them later
    if (launch_dilconv_mfma(a, h->grid, h->lds, nullptr, 1, false) != 0 || launch_dilconv_mfma(a, h->grid, h->lds, nullptr, 1, true) != 0) {
      release(h);
      return fail(DFX_ERR_HIP, "dilconv_create: cannot reserve %d bytes of LDS", h->lds);
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
    return fail(DFX_ERR_HIP, "dilconv_create: weight buffer: %s", hipGetErrorString(e));
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

int dfx_dilconv_set_weights(dfx_dilconv_t *h, const int8_t *wei, const void *bia, const float *scales) {
  if (!h || !wei || !scales) return fail(DFX_ERR_INVALID, "dilconv_set_weights: null argument");
  const dfx_dilconv_desc &d = h->d;
  if (d.bia_dt != DFX_UNDEF && !bia) return fail(DFX_ERR_INVALID, "dilconv_set_weights: null bias");
  const size_t taps = (size_t)d.ic * d.kh * d.kw;  // of one output channel
  std::vector<unsigned char> img(h->buf_bytes, 0);
  int *comp = (int *)(img.data() + h->off_comp);
  float *fb = (float *)(img.data() + h->off_bias), *fs = (float *)(img.data() + h->off_scale);
  memcpy(img.data() + h->off_wraw, wei, wei_count(d));
  // comp[k] = 128 * sum of the channel's weights: the MFMA kernel's start value (a skipped tap is the activation 0,
  // i.e. the s8 operand -128, for EVERY pixel, so the compensation is one number per channel)
  const bool proven = requant_consts(d.oc, taps, [&](int k, size_t i) { return wei[(size_t)k * taps + i]; }, bia, d.bia_dt, scales,
                                     d.nscales, comp, fb, fs);
  const bool fast = h->path == DFX_DILCONV_MFMA && d.round_mode == DFX_ROUND_NEAREST && proven && fast_allowed();
  if (h->path == DFX_DILCONV_MFMA) dilconv_pack(wei, d.oc, d.ic, img.data());
  DeviceGuard dg(h->device);
  HIP_TRY(hipMemcpy(h->d_buf, img.data(), h->buf_bytes, hipMemcpyHostToDevice));
  h->route = fast ? 1 : 0;
  h->args.fast = h->route;
  h->weights_set = true;
  set_name(h);
  return DFX_OK;
}

int dfx_dilconv_submit(dfx_dilconv_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s) {
  if (!h || !src_dev || !dst_dev) return fail(DFX_ERR_INVALID, "dilconv_submit: null argument");
  if (h->path == DFX_DILCONV_MFMA) {
    if (((uintptr_t)src_dev | (uintptr_t)dst_dev) % 16) return fail(DFX_ERR_INVALID, "dilconv_submit: src and dst must be 16-byte aligned");
  } else if ((uintptr_t)dst_dev % dt_size(h->d.dst_dt)) {
    return fail(DFX_ERR_INVALID, "dilconv_submit: dst must be aligned to its element");
  }
  if (!h->weights_set) return fail(DFX_ERR_STATE, "dilconv_submit: dfx_dilconv_set_weights not called");
  DeviceGuard dg(h->device);
  DlArgs a = h->args;  // per-launch copy: concurrent submits on several streams are independent
  a.src = (const unsigned char *)src_dev;
  a.dst = (unsigned char *)dst_dev;
  const int rc = h->path == DFX_DILCONV_MFMA ? launch_dilconv_mfma(a, h->grid, h->lds, (hipStream_t)s, 0, a.fast != 0)
                                             : launch_dilconv_generic(a, h->grid, (hipStream_t)s);
  if (rc != 0) return fail(DFX_ERR_UNSUPPORTED, "dilconv_submit: no kernel instance for this op");
  HIP_TRY(hipGetLastError());
  return DFX_OK;
}

int dfx_dilconv_submit_host(dfx_dilconv_t *h, const void *src_host, void *dst_host) {
  if (!h || !src_host || !dst_host) return fail(DFX_ERR_INVALID, "dilconv_submit_host: null argument");
  if (!h->weights_set) return fail(DFX_ERR_STATE, "dilconv_submit_host: dfx_dilconv_set_weights not called");
  DeviceGuard dg(h->device);
  return h->host.run(src_host, src_bytes(h->d), dst_host, dst_bytes(h->d),
                     [h](const void *s, void *d, dfx_stream_t st) { return dfx_dilconv_submit(h, s, d, st); });
}

int dfx_dilconv_query(const dfx_dilconv_t *h, dfx_dilconv_info *info) {
  if (!h || !info) return fail(DFX_ERR_INVALID, "dilconv_query: null argument");
  memset(info, 0, sizeof(*info));
  info->path = h->path;
  info->grid = h->grid;
  info->block = h->block;
  info->lds_bytes = h->lds;
  info->device = h->device;
  const dfx_dilconv_desc &d = h->d;
  // the kh * kw taps of the un-stuffed window, per output value
  info->algorithmic_ops = 2ull * d.bs * d.oh * d.ow * d.oc * d.ic * d.kh * d.kw;
  info->algorithmic_bytes = (uint64_t)src_bytes(d) + (uint64_t)wei_count(d) + (uint64_t)dst_bytes(d);
  memcpy(info->kernel_name, h->kernel_name, sizeof(info->kernel_name));
  return DFX_OK;
}

// test hook: the requant route the last dfx_dilconv_set_weights proved (numbering of dfx_debug_conv_requant)
int dfx_debug_dilconv_requant(const dfx_dilconv_t *h, int32_t out[1]) {
  if (!h || !out) return fail(DFX_ERR_INVALID, "dilconv_requant: null argument");
  if (!h->weights_set) return fail(DFX_ERR_STATE, "dilconv_requant: dfx_dilconv_set_weights not called");
  out[0] = h->route;
  return DFX_OK;
}

int dfx_dilconv_destroy(dfx_dilconv_t *h) {
  release(h);
  return DFX_OK;
}

}  // extern "C"
