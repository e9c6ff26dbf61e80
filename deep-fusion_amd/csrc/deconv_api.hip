// deconv_api.hip -- host side of the transposed conv op (dfx_deconv_* of include/dfx.h): descriptor validation, choice of
// the path and of the launch geometry, weight packing for the MFMA kernel (deconv.cuh, deconv_pack.h), and the requant
// route's proof from the actual weights, bias and scales (requant_host.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "deconv.cuh"
#include "deconv_pack.h"
#include "dfx_internal.h"
#include "requant_host.h"

namespace dfx {
int launch_deconv_mfma(const DcArgs &, int grid, int lds, hipStream_t, int mode, bool fast);
int launch_deconv_generic(const DcArgs &, int grid, hipStream_t);
}
using namespace dfx;

struct dfx_deconv {
  dfx_deconv_desc d;
  int device = 0;
  int path = 0;
  int grid = 0, block = 0, lds = 0;
  DcArgs args = {};                // everything but src / dst; copied per launch
  unsigned char *d_buf = nullptr;  // packed weights | raw weights | comp (4 parities) | bias | scale
  size_t off_wraw = 0, off_comp = 0, off_bias = 0, off_scale = 0, buf_bytes = 0;
  bool weights_set = false;
  int route = 0;                   // 0 exact, 1 fast (dfx_debug_conv_requant's numbering)
  HostStaging host;                // dfx_deconv_submit_host
  char kernel_name[96] = "";
};

namespace {

constexpr int LDS_LIMIT = 160 * 1024;

int validate_deconv(const dfx_deconv_desc &d) {
  if (d.bs <= 0 || d.ic <= 0 || d.ih <= 0 || d.iw <= 0 || d.oc <= 0 || d.oh <= 0 || d.ow <= 0 || d.kh <= 0 || d.kw <= 0)
    return fail(DFX_ERR_INVALID, "deconv: non-positive dimension");
  if (d.kh > 255 || d.kw > 255) return fail(DFX_ERR_INVALID, "deconv: window beyond 255");
  if (d.sh <= 0 || d.sw <= 0 || d.sh > 255 || d.sw > 255) return fail(DFX_ERR_INVALID, "deconv: stride outside 1 .. 255");
  if (d.pad_t < 0 || d.pad_l < 0) return fail(DFX_ERR_INVALID, "deconv: negative padding");
  if (d.pad_t > d.kh - 1 || d.pad_l > d.kw - 1) return fail(DFX_ERR_INVALID, "deconv: padding beyond k - 1");
  if ((long long)d.kh * d.kw * d.ic > 65025)
    return fail(DFX_ERR_INVALID, "deconv: kh * kw * ic beyond 65025 (the accumulator could leave s32)");
  if (d.oh > ((long long)d.ih - 1) * d.sh + d.kh - d.pad_t || d.ow > ((long long)d.iw - 1) * d.sw + d.kw - d.pad_l)
    return fail(DFX_ERR_INVALID, "deconv: output size beyond (in - 1) * stride + k - pad");
  if ((long long)d.bs * d.ih * d.iw >= (1ll << 31) || (long long)d.bs * d.oh * d.ow >= (1ll << 31))
    return fail(DFX_ERR_INVALID, "deconv: pixel count beyond 2^31");
  if (d.dst_dt < DFX_F32 || d.dst_dt > DFX_U8) return fail(DFX_ERR_INVALID, "deconv: bad dst dtype");
  if (d.bia_dt != DFX_UNDEF && (d.bia_dt < DFX_F32 || d.bia_dt > DFX_U8)) return fail(DFX_ERR_INVALID, "deconv: bad bias dtype");
  if (d.round_mode != DFX_ROUND_NEAREST && d.round_mode != DFX_ROUND_DOWN) return fail(DFX_ERR_INVALID, "deconv: bad round mode");
  if (d.nscales != 1 && d.nscales != d.oc) return fail(DFX_ERR_INVALID, "deconv: scales count must be 1 or oc");
  if (d.force_path != -1 && d.force_path != DFX_DECONV_MFMA && d.force_path != DFX_DECONV_GENERIC)
    return fail(DFX_ERR_INVALID, "deconv: bad force_path");
  return DFX_OK;
}

// the shape class of deconv.cuh
bool mfma_class(const dfx_deconv_desc &d) {
  const long long lim = 1ll << 31;  // one image below 2^31 bytes on either side (the kernel's offsets are 64-bit)
  const bool window = d.kh == d.kw && d.sh == 2 && d.sw == 2 && ((d.kh == 2 && d.pad_t == 0 && d.pad_l == 0) || d.kh == 3 || d.kh == 4);
  if (!window || d.ic % 32 || d.oc % 32) return false;
  if ((long long)deconv_pack_block_bytes(d.ic, d.kh) + DC_FIXED_LDS > LDS_LIMIT) return false;  // one block's fragments must fit
  return (long long)d.ih * d.iw * d.ic < lim && (long long)d.oh * d.ow * d.oc * (long long)dt_size(d.dst_dt) < lim;
}

void set_name(dfx_deconv *h) {
  const dfx_deconv_desc &d = h->d;
  if (h->path == DFX_DECONV_MFMA)
    snprintf(h->kernel_name, sizeof(h->kernel_name), "deconv_mfma<%dx%d,s2,ic%d,oc%d,%s> %s", d.kh, d.kw, d.ic, d.oc, dt_name(d.dst_dt),
             !h->weights_set ? "(no weights)" : h->route ? "fast" : "exact");
  else
    snprintf(h->kernel_name, sizeof(h->kernel_name), "deconv_generic<%dx%d,s%dx%d,ic%d,oc%d,%s> %s", d.kh, d.kw, d.sh, d.sw, d.ic,
             d.oc, dt_name(d.dst_dt), !h->weights_set ? "(no weights)" : "exact");
}

void release(dfx_deconv *h) {
  if (!h) return;
  DeviceGuard dg(h->device);
  (void)hipFree(h->d_buf);
  h->host.release();
  delete h;
}

size_t src_bytes(const dfx_deconv_desc &d) { return (size_t)d.bs * d.ih * d.iw * d.ic; }
size_t dst_bytes(const dfx_deconv_desc &d) { return (size_t)d.bs * d.oh * d.ow * d.oc * dt_size(d.dst_dt); }
size_t wei_count(const dfx_deconv_desc &d) { return (size_t)d.oc * d.ic * d.kh * d.kw; }

// sum over the outputs o < on of the taps k < kn that reach o: (o + pad - k) a multiple of `s` whose quotient is below `in`
unsigned long long taps_along(int in, int on, int kn, int s, int pad) {
  unsigned long long n = 0;
  for (int k = 0; k < kn; ++k) {  // o = i * s + k - pad in [0, on)
    const long long lo = std::max(0ll, ((long long)pad - k + s - 1) / s);  // pad - k <= pad <= kn - 1: the ceiling of a value > -s
    const long long hi = std::min<long long>(in - 1, ((long long)on - 1 + pad - k) >= 0 ? ((long long)on - 1 + pad - k) / s : -1);
    if (hi >= lo) n += (unsigned long long)(hi - lo + 1);
  }
  return n;
}

}  // namespace

extern "C" {

int dfx_deconv_create(const dfx_deconv_desc *desc, dfx_deconv_t **out) {
  if (!desc || !out) return fail(DFX_ERR_INVALID, "deconv_create: null argument");
  *out = nullptr;
  const dfx_deconv_desc &d = *desc;
  int rc = validate_deconv(d);
  if (rc) return rc;
  const bool covered = mfma_class(d);
  if (d.force_path == DFX_DECONV_MFMA && !covered)
    return fail(DFX_ERR_UNSUPPORTED, "deconv_create: shape outside the MFMA kernel's class (stride (2,2); window 2x2 with pad 0, 3x3 or 4x4; ic and oc multiples of 32; one output block's fragments within 160 KB of LDS; one image below 2^31 bytes)");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(DFX_ERR_NO_DEVICE, "deconv_create: no HIP device (this library has no CPU path)");
  dfx_deconv *h = new (std::nothrow) dfx_deconv();
  if (!h) return fail(DFX_ERR_HIP, "out of host memory");
  h->d = d;
  if (hipGetDevice(&h->device) != hipSuccess) h->device = 0;
  // AUTO RULE (include/dfx.h): the MFMA kernel everywhere in its class -- on every layer of
  // profiles/deconv/ inside it, it beats the generic kernel and conv() on the pre-stuffed tensor
  h->path = (covered && d.force_path != DFX_DECONV_GENERIC) ? DFX_DECONV_MFMA : DFX_DECONV_GENERIC;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, h->device) != hipSuccess) {
    release(h);
    return fail(DFX_ERR_HIP, "deconv_create: cannot query the device");
  }
  const int cus = std::max(1, prop.multiProcessorCount);
  DcArgs &a = h->args;
  a.bs = d.bs; a.ic = d.ic; a.ih = d.ih; a.iw = d.iw; a.oc = d.oc; a.oh = d.oh; a.ow = d.ow;
  a.kh = d.kh; a.kw = d.kw; a.sh = d.sh; a.sw = d.sw; a.pt = d.pad_t; a.pl = d.pad_l;
  a.dst_dt = d.dst_dt; a.relu = (d.relu || d.dst_dt == DFX_U8) ? 1 : 0; a.rm = d.round_mode;
  size_t wpk_bytes = 0;
  if (h->path == DFX_DECONV_MFMA) {
    const int wblk = (int)deconv_pack_block_bytes(d.ic, d.kh);
    a.cblocks = d.oc / 32;
    a.ksteps = d.ic / 32;
    a.wblocks = std::min({DC_CHUNK, a.cblocks, (LDS_LIMIT - DC_FIXED_LDS) / wblk});  // >= 1 inside the class
    a.nchunks = (a.cblocks + a.wblocks - 1) / a.wblocks;
    // base grid: output row oy = 2 yb + a - pad_t, yb = (oy + pad_t) / 2 over oy < oh (YB <= oh, XB <= ow)
    a.yb0 = d.pad_t / 2; a.YB = (d.oh - 1 + d.pad_t) / 2 - a.yb0 + 1;
    a.xb0 = d.pad_l / 2; a.XB = (d.ow - 1 + d.pad_l) / 2 - a.xb0 + 1;
    a.bp_total = (int)((long long)d.bs * a.YB * a.XB);
    a.strips = (a.bp_total + 31) / 32;
    wpk_bytes = deconv_pack_bytes(d.oc, d.ic, d.kh);
    h->block = DC_THREADS;
    h->lds = a.wblocks * wblk + DC_FIXED_LDS;
    // Launch: the workgroups that are resident at once (by LDS, at most 4 per CU), a multiple of the chunk count; a
    // workgroup keeps its chunk's weights in LDS and its waves stride over the strips.  Fewer workgroups than
    // (chunk, slot) units (tiny devices, DFX_DECONV_GRID) make the workgroups loop over the units.
    const int wg_strips = DC_THREADS / 64;
    const long long cap = (long long)cus * std::min(4, std::max(1, LDS_LIMIT / h->lds));
    long long slots = std::min<long long>((a.strips + wg_strips - 1) / wg_strips, std::max<long long>(1, cap / a.nchunks));
    long long grid = slots * a.nchunks;
    if (const char *e = tuning_value("DFX_DECONV_GRID")) {  // testing aid
      grid = std::max(1ll, std::min(grid, (long long)atoi(e)));
      slots = (grid + a.nchunks - 1) / a.nchunks;
    }
    a.slots = (int)slots;
    h->grid = (int)grid;
    // both routes' instances: set_weights may switch between them later
    if (launch_deconv_mfma(a, h->grid, h->lds, nullptr, 1, false) != 0 || launch_deconv_mfma(a, h->grid, h->lds, nullptr, 1, true) != 0) {
      release(h);
      return fail(DFX_ERR_HIP, "deconv_create: cannot reserve %d bytes of LDS", h->lds);
    }
  } else {
    a.items = (long long)d.bs * d.oh * d.ow * d.oc;
    h->block = 256;
    h->lds = 0;
    h->grid = (int)std::min((a.items + 255) / 256, (long long)cus * 8);
  }
  h->off_wraw = round16(wpk_bytes);
  h->off_comp = h->off_wraw + round16(wei_count(d));
  h->off_bias = h->off_comp + round16((size_t)d.oc * 4 * 4);
  h->off_scale = h->off_bias + round16((size_t)d.oc * 4);
  h->buf_bytes = h->off_scale + round16((size_t)d.oc * 4);
  hipError_t e = hipMalloc((void **)&h->d_buf, h->buf_bytes);
  if (e != hipSuccess) {
    release(h);
    return fail(DFX_ERR_HIP, "deconv_create: weight buffer: %s", hipGetErrorString(e));
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

int dfx_deconv_set_weights(dfx_deconv_t *h, const int8_t *wei, const void *bia, const float *scales) {
  if (!h || !wei || !scales) return fail(DFX_ERR_INVALID, "deconv_set_weights: null argument");
  const dfx_deconv_desc &d = h->d;
  if (d.bia_dt != DFX_UNDEF && !bia) return fail(DFX_ERR_INVALID, "deconv_set_weights: null bias");
  const size_t taps = (size_t)d.ic * d.kh * d.kw;  // of one output channel
  std::vector<unsigned char> img(h->buf_bytes, 0);
  int *comp = (int *)(img.data() + h->off_comp);
  float *fb = (float *)(img.data() + h->off_bias), *fs = (float *)(img.data() + h->off_scale);
  memcpy(img.data() + h->off_wraw, wei, wei_count(d));
  // the proof runs over ALL taps of a channel: every output sums a subset of them, so |acc| <= 255 * max(P, N) holds
  std::vector<int32_t> comp_all((size_t)d.oc);
  const bool proven = requant_consts(d.oc, taps, [&](int k, size_t i) { return wei[(size_t)k * taps + i]; }, bia, d.bia_dt, scales,
                                     d.nscales, comp_all.data(), fb, fs);
  const bool fast = h->path == DFX_DECONV_MFMA && d.round_mode == DFX_ROUND_NEAREST && proven && fast_allowed();
  if (h->path == DFX_DECONV_MFMA) {
    deconv_pack(wei, d.oc, d.ic, d.kh, img.data());
    // the start value of parity (a, b): 128 * the sum of ITS taps (ky % 2 == a, kx % 2 == b)
    for (int k = 0; k < d.oc; ++k)
      for (int i = 0; i < d.ic; ++i)
        for (int ky = 0; ky < d.kh; ++ky)
          for (int kx = 0; kx < d.kw; ++kx)
            comp[(size_t)((ky & 1) * 2 + (kx & 1)) * d.oc + k] += 128 * (int)wei[(((size_t)k * d.ic + i) * d.kh + ky) * d.kw + kx];
  }
  DeviceGuard dg(h->device);
  HIP_TRY(hipMemcpy(h->d_buf, img.data(), h->buf_bytes, hipMemcpyHostToDevice));
  h->route = fast ? 1 : 0;
  h->args.fast = h->route;
  h->weights_set = true;
  set_name(h);
  return DFX_OK;
}

int dfx_deconv_submit(dfx_deconv_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s) {
  if (!h || !src_dev || !dst_dev) return fail(DFX_ERR_INVALID, "deconv_submit: null argument");
  if (h->path == DFX_DECONV_MFMA) {
    if (((uintptr_t)src_dev | (uintptr_t)dst_dev) % 16) return fail(DFX_ERR_INVALID, "deconv_submit: src and dst must be 16-byte aligned");
  } else if ((uintptr_t)dst_dev % dt_size(h->d.dst_dt)) {
    return fail(DFX_ERR_INVALID, "deconv_submit: dst must be aligned to its element");
  }
  if (!h->weights_set) return fail(DFX_ERR_STATE, "deconv_submit: dfx_deconv_set_weights not called");
  DeviceGuard dg(h->device);
  DcArgs a = h->args;  // per-launch copy: concurrent submits on several streams are independent
  a.src = (const unsigned char *)src_dev;
  a.dst = (unsigned char *)dst_dev;
  const int rc = h->path == DFX_DECONV_MFMA ? launch_deconv_mfma(a, h->grid, h->lds, (hipStream_t)s, 0, a.fast != 0)
                                            : launch_deconv_generic(a, h->grid, (hipStream_t)s);
  if (rc != 0) return fail(DFX_ERR_UNSUPPORTED, "deconv_submit: no kernel instance for this op");
  HIP_TRY(hipGetLastError());
  return DFX_OK;
}

int dfx_deconv_submit_host(dfx_deconv_t *h, const void *src_host, void *dst_host) {
  if (!h || !src_host || !dst_host) return fail(DFX_ERR_INVALID, "deconv_submit_host: null argument");
  if (!h->weights_set) return fail(DFX_ERR_STATE, "deconv_submit_host: dfx_deconv_set_weights not called");
  DeviceGuard dg(h->device);
  return h->host.run(src_host, src_bytes(h->d), dst_host, dst_bytes(h->d),
                     [h](const void *s, void *d, dfx_stream_t st) { return dfx_deconv_submit(h, s, d, st); });
}

int dfx_deconv_query(const dfx_deconv_t *h, dfx_deconv_info *info) {
  if (!h || !info) return fail(DFX_ERR_INVALID, "deconv_query: null argument");
  memset(info, 0, sizeof(*info));
  info->path = h->path;
  info->grid = h->grid;
  info->block = h->block;
  info->lds_bytes = h->lds;
  info->device = h->device;
  const dfx_deconv_desc &d = h->d;
  // the taps that exist: the (oy, ky) pairs times the (ox, kx) pairs, per image, input and output channel
  info->algorithmic_ops = 2ull * d.bs * d.ic * d.oc * taps_along(d.ih, d.oh, d.kh, d.sh, d.pad_t) * taps_along(d.iw, d.ow, d.kw, d.sw, d.pad_l);
  info->algorithmic_bytes = (uint64_t)src_bytes(d) + (uint64_t)wei_count(d) + (uint64_t)dst_bytes(d);
  memcpy(info->kernel_name, h->kernel_name, sizeof(info->kernel_name));
  return DFX_OK;
}

// test hook: the requant route the last dfx_deconv_set_weights proved (numbering of dfx_debug_conv_requant)
int dfx_debug_deconv_requant(const dfx_deconv_t *h, int32_t out[1]) {
  if (!h || !out) return fail(DFX_ERR_INVALID, "deconv_requant: null argument");
  if (!h->weights_set) return fail(DFX_ERR_STATE, "deconv_requant: dfx_deconv_set_weights not called");
  out[0] = h->route;
  return DFX_OK;
}

int dfx_deconv_destroy(dfx_deconv_t *h) {
  release(h);
  return DFX_OK;
}

}  // extern "C"
