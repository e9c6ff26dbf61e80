// fc_api.hip -- host side of the fully-connected op (dfx_fc_* of include/dfx.h): descriptor validation, choice of the
// path, the split-K plan, weight packing for the MFMA kernel (fc.cuh, fc_pack.h), the requant route's proof from the
// actual weights, bias and scales, and the order of the submits that share the handle's slab of partial sums.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "dfx_internal.h"
#include "fc.cuh"
#include "fc_pack.h"
#include "requant_host.h"

namespace dfx {
int launch_fc_mfma(const FcArgs &, int grid, int lds, hipStream_t, int mode);
int launch_fc_epilogue(const FcArgs &, int grid, hipStream_t, bool fast);
int launch_fc_generic(const FcArgs &, int grid, hipStream_t);
}
using namespace dfx;

struct dfx_fc {
  dfx_fc_desc d;
  int device = 0;
  int path = 0;
  int grid = 0, block = 0, lds = 0;
  int ep_grid = 0;                 // of the epilogue kernel
  FcArgs args = {};                // everything but src / dst; copied per launch
  unsigned char *d_buf = nullptr;  // packed weights (MFMA) | raw weights (generic) | comp | bias | scale
  int *d_slab = nullptr;           // MFMA: [splitk][n_pad][oc_pad]
  size_t off_comp = 0, off_bias = 0, off_scale = 0, buf_bytes = 0;
  bool weights_set = false;
  int route = 0;                   // 0 exact, 1 fast (dfx_debug_conv_requant's numbering)
  TwoLaunchOrder order;            // MFMA: the two launches meet in d_slab
  HostStaging host;                // dfx_fc_submit_host
  char kernel_name[96] = "";
};

namespace {

// Split-K plan (from tools/bench_fc's sweep).  A slab slice is n_pad * oc_pad * 4 bytes; the slab is
// capped at FC_SLAB_CAP.  K is split until there is one unit per CU, but into no more slices than staged tiles of
// FC_KT k-steps: slices of whole tiles run the kernel's branch-free path only.
constexpr size_t FC_SLAB_CAP = 64u << 20;

long long k_of(const dfx_fc_desc &d) { return (long long)d.ih * d.iw * d.ic; }

int validate_fc(const dfx_fc_desc &d) {
  if (d.bs <= 0 || d.ic <= 0 || d.ih <= 0 || d.iw <= 0 || d.oc <= 0) return fail(DFX_ERR_INVALID, "fc: non-positive dimension");
  if ((long long)d.ih * d.iw > 65025 || k_of(d) > 65025)
    return fail(DFX_ERR_INVALID, "fc: ih * iw * ic beyond 65025 (the accumulator could leave s32)");
  if ((long long)d.bs * d.oc >= (1ll << 31)) return fail(DFX_ERR_INVALID, "fc: bs * oc beyond 2^31");
  if (d.bs > INT32_MAX - 31) return fail(DFX_ERR_INVALID, "fc: bs beyond 2^31 - 32 (bs rounded up to 32 must fit an int)");
  if (d.dst_dt < DFX_F32 || d.dst_dt > DFX_U8) return fail(DFX_ERR_INVALID, "fc: bad dst dtype");
  if (d.bia_dt != DFX_UNDEF && (d.bia_dt < DFX_F32 || d.bia_dt > DFX_U8)) return fail(DFX_ERR_INVALID, "fc: bad bias dtype");
  if (d.round_mode != DFX_ROUND_NEAREST && d.round_mode != DFX_ROUND_DOWN) return fail(DFX_ERR_INVALID, "fc: bad round mode");
  if (d.nscales != 1 && d.nscales != d.oc) return fail(DFX_ERR_INVALID, "fc: scales count must be 1 or oc");
  if (d.force_path != -1 && d.force_path != DFX_FC_MFMA && d.force_path != DFX_FC_GENERIC)
    return fail(DFX_ERR_INVALID, "fc: bad force_path");
  return DFX_OK;
}

void set_name(dfx_fc *h) {
  if (h->path == DFX_FC_MFMA)
    snprintf(h->kernel_name, sizeof(h->kernel_name), "fc_mfma<k%d,%s,sk%d> %s", h->args.k, dt_name(h->d.dst_dt), h->args.splitk,
             !h->weights_set ? "(no weights)" : h->route ? "fast" : "exact");
  else
    snprintf(h->kernel_name, sizeof(h->kernel_name), "fc_generic<%s> exact", dt_name(h->d.dst_dt));
}

void release(dfx_fc *h) {
  if (!h) return;
  DeviceGuard dg(h->device);
  (void)hipFree(h->d_buf);
  (void)hipFree(h->d_slab);
  h->order.destroy();
  h->host.release();
  delete h;
}

size_t src_bytes(const dfx_fc_desc &d) { return (size_t)d.bs * (size_t)k_of(d); }
size_t dst_bytes(const dfx_fc_desc &d) { return (size_t)d.bs * d.oc * dt_size(d.dst_dt); }
size_t wei_count(const dfx_fc_desc &d) { return (size_t)d.oc * (size_t)k_of(d); }

}  // namespace

extern "C" {

int dfx_fc_create(const dfx_fc_desc *desc, dfx_fc_t **out) {
  if (!desc || !out) return fail(DFX_ERR_INVALID, "fc_create: null argument");
  *out = nullptr;
  const dfx_fc_desc &d = *desc;
  int rc = validate_fc(d);
  if (rc) return rc;
  const int K = (int)k_of(d);
  const bool covered = K % 64 == 0;
  if (d.force_path == DFX_FC_MFMA && !covered)
    return fail(DFX_ERR_UNSUPPORTED, "fc_create: shape outside the MFMA kernel's class (ih * iw * ic a multiple of 64)");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(DFX_ERR_NO_DEVICE, "fc_create: no HIP device (this library has no CPU path)");
  dfx_fc *h = new (std::nothrow) dfx_fc();
  if (!h) return fail(DFX_ERR_HIP, "out of host memory");
  h->d = d;
  if (hipGetDevice(&h->device) != hipSuccess) h->device = 0;
  h->path = (covered && d.force_path != DFX_FC_GENERIC) ? DFX_FC_MFMA : DFX_FC_GENERIC;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, h->device) != hipSuccess) {
    release(h);
    return fail(DFX_ERR_HIP, "fc_create: cannot query the device");
  }
  const int cus = std::max(1, prop.multiProcessorCount);
  FcArgs &a = h->args;
  a.bs = d.bs; a.k = K; a.oc = d.oc; a.ic = d.ic; a.ih = d.ih; a.iw = d.iw;
  a.dst_dt = d.dst_dt; a.relu = (d.relu || d.dst_dt == DFX_U8) ? 1 : 0; a.rm = d.round_mode;
  a.ocb = fc_pack_blocks(d.oc);
  a.oc_pad = 32 * a.ocb;
  a.n_pad = (int)(((long long)d.bs + 31) / 32 * 32);
  a.splitk = 1;
  size_t w_bytes;
  if (h->path == DFX_FC_MFMA) {
    a.nks = K / 64;
    a.ocg = (a.ocb + FC_WAVES - 1) / FC_WAVES;
    a.chunks = (d.bs + FC_CHUNK - 1) / FC_CHUNK;
    // Split K until there is a unit per CU, within one slice per tile and the slab cap; never more slices than
    // k-steps.  Slices are cut at whole tiles (the last one takes the partial tile); a forced splitk beyond the tile
    // count is cut at k-steps and may be uneven.
    const long long base = (long long)a.ocg * a.chunks;
    const size_t slice_bytes = (size_t)a.n_pad * a.oc_pad * 4;
    const int tiles = (a.nks + FC_KT - 1) / FC_KT;
    long long sk = std::max<long long>(1, cus / base);
    sk = std::min<long long>(sk, std::max<long long>(1, (long long)(FC_SLAB_CAP / slice_bytes)));
    sk = std::min<long long>(sk, tiles);
    if (const char *e = tuning_value("DFX_FC_SPLITK")) sk = atoi(e);  // testing / tuning aid: forced, clamped below
    a.splitk = (int)std::max<long long>(1, std::min<long long>(sk, a.nks));
    a.cut = a.splitk <= tiles ? FC_KT : 1;
    const long long units = base * a.splitk;
    if (units >= (1ll << 31)) {
      release(h);
      return fail(DFX_ERR_INVALID, "fc_create: too many work units");
    }
    a.units = (int)units;
    long long grid = std::min<long long>(units, (long long)cus * 8);
    if (const char *e = tuning_value("DFX_FC_GRID")) grid = std::max(1ll, std::min(grid, (long long)atoi(e)));  // testing aid
    h->grid = (int)grid;
    h->block = FC_THREADS;
    h->lds = 32 * std::min(FC_CHUNK / 32, a.n_pad / 32) * FC_PITCH;
    const long long ep_items = (long long)d.bs * ((d.oc + 3) / 4);
    h->ep_grid = (int)std::min<long long>((ep_items + 255) / 256, (long long)cus * 8);
    w_bytes = fc_pack_bytes(d.oc, K);
    hipError_t e = hipMalloc((void **)&h->d_slab, slice_bytes * a.splitk);
    if (e == hipSuccess) e = h->order.create();
    if (e != hipSuccess) {
      release(h);
      return fail(DFX_ERR_HIP, "fc_create: slab of partial sums: %s", hipGetErrorString(e));
    }
    a.slab = h->d_slab;
    if (launch_fc_mfma(a, h->grid, h->lds, nullptr, 1) != 0) {
      release(h);
      return fail(DFX_ERR_HIP, "fc_create: cannot reserve %d bytes of LDS", h->lds);
    }
  } else {
    a.items = (long long)d.bs * d.oc;
    h->block = 256;
    h->lds = 0;
    h->grid = (int)std::min((a.items + 255) / 256, (long long)cus * 8);
    w_bytes = wei_count(d);
  }
  h->off_comp = round16(w_bytes);
  h->off_bias = h->off_comp + round16((size_t)a.oc_pad * 4);
  h->off_scale = h->off_bias + round16((size_t)a.oc_pad * 4);
  h->buf_bytes = h->off_scale + round16((size_t)a.oc_pad * 4);
  hipError_t e = hipMalloc((void **)&h->d_buf, h->buf_bytes);
  if (e != hipSuccess) {
    release(h);
    return fail(DFX_ERR_HIP, "fc_create: weight buffer: %s", hipGetErrorString(e));
  }
  a.wpk = h->d_buf;
  a.wraw = (const signed char *)h->d_buf;
  a.comp = (const int *)(h->d_buf + h->off_comp);
  a.bias = (const float *)(h->d_buf + h->off_bias);
  a.scale = (const float *)(h->d_buf + h->off_scale);
  set_name(h);
  *out = h;
  return DFX_OK;
}

int dfx_fc_set_weights(dfx_fc_t *h, const int8_t *wei, const void *bia, const float *scales) {
  if (!h || !wei || !scales) return fail(DFX_ERR_INVALID, "fc_set_weights: null argument");
  const dfx_fc_desc &d = h->d;
  if (d.bia_dt != DFX_UNDEF && !bia) return fail(DFX_ERR_INVALID, "fc_set_weights: null bias");
  const size_t taps = (size_t)h->args.k;  // of one output channel
  std::vector<unsigned char> img(h->buf_bytes, 0);  // (the entries oc .. oc_pad - 1 of the constants stay 0)
  int *comp = (int *)(img.data() + h->off_comp);
  float *fb = (float *)(img.data() + h->off_bias), *fs = (float *)(img.data() + h->off_scale);
  const bool proven = requant_consts(d.oc, taps, [&](int k, size_t i) { return wei[(size_t)k * taps + i]; }, bia, d.bia_dt, scales,
                                     d.nscales, comp, fb, fs);
  const bool fast = h->path == DFX_FC_MFMA && d.round_mode == DFX_ROUND_NEAREST && proven && fast_allowed();
  if (h->path == DFX_FC_MFMA) fc_pack(wei, d.oc, d.ic, d.ih, d.iw, img.data());
  else memcpy(img.data(), wei, wei_count(d));
  DeviceGuard dg(h->device);
  HIP_TRY(hipMemcpy(h->d_buf, img.data(), h->buf_bytes, hipMemcpyHostToDevice));
  h->route = fast ? 1 : 0;
  h->args.fast = h->route;
  h->weights_set = true;
  set_name(h);
  return DFX_OK;
}

int dfx_fc_submit(dfx_fc_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s) {
  if (!h || !src_dev || !dst_dev) return fail(DFX_ERR_INVALID, "fc_submit: null argument");
  if (((uintptr_t)src_dev | (uintptr_t)dst_dev) % 16) return fail(DFX_ERR_INVALID, "fc_submit: src and dst must be 16-byte aligned");
  if (!h->weights_set) return fail(DFX_ERR_STATE, "fc_submit: dfx_fc_set_weights not called");
  DeviceGuard dg(h->device);
  const hipStream_t st = (hipStream_t)s;
  FcArgs a = h->args;  // per-launch copy
  a.src = (const unsigned char *)src_dev;
  a.dst = (unsigned char *)dst_dev;
  if (h->path == DFX_FC_GENERIC) {
    launch_fc_generic(a, h->grid, st);
    HIP_TRY(hipGetLastError());
    return DFX_OK;
  }
  // two launches through the handle's one slab: serialised (dfx.h; TwoLaunchOrder in dfx_internal.h)
  std::lock_guard<std::mutex> lk(h->order.mu);
  int rc = h->order.enter(st);
  if (rc) return rc;
  // (once the first launch is out the slab has a writer in flight: every way out goes through leave(), so that a
  //  submit on another stream still waits for it)
  rc = launch_fc_mfma(a, h->grid, h->lds, st, 0) != 0 ? fail(DFX_ERR_UNSUPPORTED, "fc_submit: no kernel instance for this op") : DFX_OK;
  if (rc) return rc;  // nothing was launched
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) {
    if (launch_fc_epilogue(a, h->ep_grid, st, a.fast != 0) != 0) rc = fail(DFX_ERR_UNSUPPORTED, "fc_submit: no kernel instance for this op");
    else e = hipGetLastError();
  }
  if (e != hipSuccess) rc = fail(DFX_ERR_HIP, "fc_submit: %s", hipGetErrorString(e));
  if (rc) {
    (void)h->order.leave(st);
    return rc;
  }
  return h->order.leave(st);
}

int dfx_fc_submit_host(dfx_fc_t *h, const void *src_host, void *dst_host) {
  if (!h || !src_host || !dst_host) return fail(DFX_ERR_INVALID, "fc_submit_host: null argument");
  if (!h->weights_set) return fail(DFX_ERR_STATE, "fc_submit_host: dfx_fc_set_weights not called");
  DeviceGuard dg(h->device);
  return h->host.run(src_host, src_bytes(h->d), dst_host, dst_bytes(h->d),
                     [h](const void *s, void *d, dfx_stream_t st) { return dfx_fc_submit(h, s, d, st); });
}

int dfx_fc_query(const dfx_fc_t *h, dfx_fc_info *info) {
  if (!h || !info) return fail(DFX_ERR_INVALID, "fc_query: null argument");
  memset(info, 0, sizeof(*info));
  info->path = h->path;
  info->splitk = h->args.splitk;
  info->grid = h->grid;
  info->block = h->block;
  info->lds_bytes = h->lds;
  info->device = h->device;
  const dfx_fc_desc &d = h->d;
  info->algorithmic_ops = 2 * (uint64_t)d.bs * (uint64_t)h->args.k * (uint64_t)d.oc;
  info->algorithmic_bytes = (uint64_t)src_bytes(d) + (uint64_t)wei_count(d) + (uint64_t)dst_bytes(d);
  memcpy(info->kernel_name, h->kernel_name, sizeof(info->kernel_name));
  return DFX_OK;
}

// test hook: the requant route the last dfx_fc_set_weights proved (numbering of dfx_debug_conv_requant)
int dfx_debug_fc_requant(const dfx_fc_t *h, int32_t out[1]) {
  if (!h || !out) return fail(DFX_ERR_INVALID, "fc_requant: null argument");
  if (!h->weights_set) return fail(DFX_ERR_STATE, "fc_requant: dfx_fc_set_weights not called");
  out[0] = h->route;
  return DFX_OK;
}

int dfx_fc_destroy(dfx_fc_t *h) {
  release(h);
  return DFX_OK;
}

}  // extern "C"
