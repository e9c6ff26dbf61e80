// se_api.hip -- host side of the squeeze-and-excitation op (dfx_se_* of include/dfx.h): descriptor validation, the
// squeeze kernel's plan (se_plan.h), the device image of the two weight matrices with their requant constants, the gate
// table and the output scales, and the order of the submits that share the handle's scratch (the slab of partial sums
// and the gate).  The kernels are in se.cuh.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "dfx_internal.h"
#include "requant_host.h"
#include "se.cuh"
#include "se_plan.h"

namespace dfx {
int launch_se_squeeze(const SeArgs &a, int grid, hipStream_t s);
int launch_se_squeeze_generic(const SeArgs &a, int grid, hipStream_t s);
int launch_se_excite(const SeArgs &a, int grid, int block, int lds, hipStream_t s);
int launch_se_scale(const SeArgs &a, int grid, hipStream_t s);
int launch_se_scale_generic(const SeArgs &a, int grid, hipStream_t s);
int se_squeeze_lds_bytes();
}
using namespace dfx;

struct dfx_se {
  dfx_se_desc d;
  int device = 0;
  int path = DFX_SE_GENERIC;
  SeArgs band = {}, generic = {};  // without src / dst; `band` only on the band path
  int sq_grid = 0, sq_grid_generic = 0, ex_grid = 0, ex_block = 0, ex_lds = 0, sc_grid = 0, sc_grid_generic = 0;
  unsigned char *d_buf = nullptr;  // w1 | w2 | comp1 bias1 scale1 | comp2 bias2 scale2 | out_scale | lut
  int *d_slab = nullptr;           // [bs][slices][c] partial sums
  unsigned char *d_gate = nullptr; // [bs][c]
  size_t off_w2 = 0, off_c1 = 0, off_b1 = 0, off_s1 = 0, off_c2 = 0, off_b2 = 0, off_s2 = 0, off_os = 0, off_lut = 0, buf_bytes = 0;
  bool weights_set = false;
  TwoLaunchOrder order;            // the launches of a submit meet in d_slab and d_gate
  HostStaging host;                // dfx_se_submit_host
  char kernel_name[96] = "";
};

namespace {

constexpr int kMaxBlocks = 256 * 8;  // grid-stride kernels: 8 workgroups per CU
constexpr int kScaleRows = 8;        // pixels a lane of the scale kernel walks, halved while the launch would have fewer
constexpr int kFillBlocks = 512;     // than kFillBlocks workgroups
constexpr long long kMaxElems = 1ll << 40;
constexpr long long kWideLayer = 8192;  // c * cr above which the excite kernel runs 1024 lanes

const char *mode_name(int m) { return m == DFX_SE_SCALE ? "scale" : m == DFX_SE_GATE ? "gate" : "squeeze"; }

bool bias_dt_ok(int dt) { return dt == DFX_UNDEF || (dt >= DFX_F32 && dt <= DFX_U8); }

int validate_se(const dfx_se_desc &d) {
  if (d.bs < 1 || d.c < 1 || d.ih < 1 || d.iw < 1 || d.cr < 1) return fail(DFX_ERR_INVALID, "se: bs, c, ih, iw and cr must be at least 1");
  if ((long long)d.ih * d.iw > SE_MAX_PX) return fail(DFX_ERR_INVALID, "se: ih * iw beyond 2^23 (a channel's sum could leave s32)");
  if (d.c > SE_MAX_C || d.cr > SE_MAX_C) return fail(DFX_ERR_INVALID, "se: c or cr beyond %d (the accumulators could leave s32)", SE_MAX_C);
  // ih * iw <= 2^23 and c <= 2^14: one image is at most 2^37 elements, and no product is formed before it is known to fit
  if (d.bs > (kMaxElems - 1) / ((long long)d.ih * d.iw * d.c)) return fail(DFX_ERR_INVALID, "se: a tensor of 2^40 elements or more");
  if (d.mode != DFX_SE_SCALE && d.mode != DFX_SE_GATE && d.mode != DFX_SE_SQUEEZE) return fail(DFX_ERR_INVALID, "se: bad mode");
  if (!bias_dt_ok(d.bia1_dt) || !bias_dt_ok(d.bia2_dt)) return fail(DFX_ERR_INVALID, "se: bad bias dtype");
  if (d.round_mode != DFX_ROUND_NEAREST && d.round_mode != DFX_ROUND_DOWN) return fail(DFX_ERR_INVALID, "se: bad round mode");
  if (d.nscales1 != 1 && d.nscales1 != d.cr) return fail(DFX_ERR_INVALID, "se: nscales1 must be 1 or cr");
  if (d.nscales2 != 1 && d.nscales2 != d.c) return fail(DFX_ERR_INVALID, "se: nscales2 must be 1 or c");
  if (d.nscales_out != 1 && d.nscales_out != d.c) return fail(DFX_ERR_INVALID, "se: nscales_out must be 1 or c");
  if (d.force_path != -1 && d.force_path != DFX_SE_BAND && d.force_path != DFX_SE_GENERIC) return fail(DFX_ERR_INVALID, "se: bad force_path");
  return DFX_OK;
}

bool band_class(const dfx_se_desc &d) { return d.c % 16 == 0 && (long long)d.ih * d.iw * d.c < (1ll << 31); }

size_t src_bytes(const dfx_se_desc &d) { return (size_t)d.bs * d.ih * d.iw * d.c; }
size_t dst_bytes(const dfx_se_desc &d) { return d.mode == DFX_SE_SCALE ? src_bytes(d) : (size_t)d.bs * d.c; }

int capped_grid(long long blocks) {
  blocks = std::max(1ll, std::min<long long>(blocks, kMaxBlocks));
  if (const char *e = tuning_value("DFX_SE_GRID")) blocks = std::max(1ll, std::min(blocks, (long long)atoi(e)));  // testing aid
  return (int)blocks;
}

void release(dfx_se *h) {
  if (!h) return;
  DeviceGuard dg(h->device);
  (void)hipFree(h->d_buf);
  (void)hipFree(h->d_slab);
  (void)hipFree(h->d_gate);
  h->order.destroy();
  h->host.release();
  delete h;
}

}  // namespace

extern "C" {

int dfx_se_create(const dfx_se_desc *desc, dfx_se_t **out) {
  if (!desc || !out) return fail(DFX_ERR_INVALID, "se_create: null argument");
  *out = nullptr;
  const dfx_se_desc &d = *desc;
  int rc = validate_se(d);
  if (rc) return rc;
  const bool covered = band_class(d);
  if (d.force_path == DFX_SE_BAND && !covered)
    return fail(DFX_ERR_UNSUPPORTED, "se_create: shape outside the band kernels' class (c a multiple of 16; one image below 2^31 bytes)");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(DFX_ERR_NO_DEVICE, "se_create: no HIP device (this library has no CPU path)");
  dfx_se *h = new (std::nothrow) dfx_se();
  if (!h) return fail(DFX_ERR_HIP, "out of host memory");
  h->d = d;
  if (hipGetDevice(&h->device) != hipSuccess) h->device = 0;
  // AUTO RULE (include/dfx.h): the band kernels everywhere in their class
  h->path = (covered && d.force_path != DFX_SE_GENERIC) ? DFX_SE_BAND : DFX_SE_GENERIC;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, h->device) != hipSuccess) {
    release(h);
    return fail(DFX_ERR_HIP, "se_create: cannot query the device");
  }
  const int cus = std::max(1, prop.multiProcessorCount);
  const int px = d.ih * d.iw;
  const bool weights = d.mode != DFX_SE_SQUEEZE;

  SeArgs a = {};
  a.bs = d.bs; a.c = d.c; a.cr = d.cr; a.px = px; a.mode = d.mode; a.rm = d.round_mode;
  a.cpad = (int)round16((size_t)d.c);
  a.crpad = (int)round16((size_t)d.cr);
  a.ex_parts = 1;
  a.slices = 1; a.groups = 0; a.gl = 1; a.gchunks = 1; a.pln = 1; a.parts = 1;
  a.sq_items = (long long)d.bs * d.c;
  a.cols = px;
  a.sc_total = (long long)d.bs * px * d.c;
  h->generic = a;
  h->sq_grid_generic = capped_grid((a.sq_items + 255) / 256);
  h->sc_grid_generic = capped_grid((a.sc_total + 255) / 256);
  h->ex_grid = capped_grid(d.bs);
  // the excite kernel: one workgroup per image, 1024 lanes where the two layers are wide (measured)
  h->ex_block = weights && (long long)d.c * d.cr > kWideLayer ? SE_EXCITE_MAX_THREADS : SE_THREADS;
  h->ex_lds = a.cpad + a.crpad + 4 * h->ex_block;
  if (h->path == DFX_SE_BAND) {
    long long forced = 0;
    if (const char *e = tuning_value("DFX_SE_SLICES")) forced = std::max(1ll, atoll(e));  // testing / tuning aid: clamped by the planner
    const SePlan p = se_plan(d.bs, px, d.c, cus, forced);
    a.slices = p.slices; a.groups = p.groups; a.gl = p.gl; a.gchunks = p.gchunks; a.pln = p.pln; a.parts = p.parts;
    a.sq_items = p.items;
    a.ex_parts = std::max(1, std::min(p.slices, h->ex_block / d.c));
    h->sq_grid = capped_grid(p.items);
    int rows = kScaleRows;
    while (rows > 1 && (long long)d.bs * ((px + rows - 1) / rows) * p.groups < 256ll * kFillBlocks) rows /= 2;
    a.cols = (px + rows - 1) / rows;
    a.sc_total = (long long)d.bs * a.cols * p.groups;
    h->sc_grid = capped_grid((a.sc_total + 255) / 256);
    h->band = a;
    snprintf(h->kernel_name, sizeof(h->kernel_name), "se_band<%s> c%d cr%d slices%d", mode_name(d.mode), d.c, d.cr, p.slices);
  } else {
    snprintf(h->kernel_name, sizeof(h->kernel_name), "se_generic<%s> c%d cr%d", mode_name(d.mode), d.c, d.cr);
  }

  // scratch: the slab for the larger of the two plans' slice counts, the gate
  hipError_t e = hipMalloc((void **)&h->d_slab, (size_t)d.bs * a.slices * d.c * 4);
  if (e == hipSuccess && d.mode == DFX_SE_SCALE) e = hipMalloc((void **)&h->d_gate, round16((size_t)d.bs * d.c));
  if (e == hipSuccess) e = h->order.create();
  if (e == hipSuccess && weights) {
    const size_t cr = (size_t)d.cr, c = (size_t)d.c;
    h->off_w2 = round16(cr * a.cpad);
    h->off_c1 = h->off_w2 + round16(c * a.crpad);
    h->off_b1 = h->off_c1 + round16(cr * 4);
    h->off_s1 = h->off_b1 + round16(cr * 4);
    h->off_c2 = h->off_s1 + round16(cr * 4);
    h->off_b2 = h->off_c2 + round16(c * 4);
    h->off_s2 = h->off_b2 + round16(c * 4);
    h->off_os = h->off_s2 + round16(c * 4);
    h->off_lut = h->off_os + round16(c * 4);
    h->buf_bytes = h->off_lut + 256;
    e = hipMalloc((void **)&h->d_buf, h->buf_bytes);
  }
  if (e != hipSuccess) {
    release(h);
    return fail(DFX_ERR_HIP, "se_create: scratch and weight buffers: %s", hipGetErrorString(e));
  }
  for (SeArgs *p : {&h->band, &h->generic}) {
    p->slab = h->d_slab;
    p->gate = h->d_gate;
    if (!weights) continue;
    p->w1 = (const signed char *)h->d_buf;
    p->w2 = (const signed char *)(h->d_buf + h->off_w2);
    p->comp1 = (const int *)(h->d_buf + h->off_c1);
    p->bias1 = (const float *)(h->d_buf + h->off_b1);
    p->scale1 = (const float *)(h->d_buf + h->off_s1);
    p->comp2 = (const int *)(h->d_buf + h->off_c2);
    p->bias2 = (const float *)(h->d_buf + h->off_b2);
    p->scale2 = (const float *)(h->d_buf + h->off_s2);
    p->out_scale = (const float *)(h->d_buf + h->off_os);
    p->lut = h->d_buf + h->off_lut;
  }
  *out = h;
  return DFX_OK;
}

int dfx_se_set_weights(dfx_se_t *h, const int8_t *w1, const void *bia1, const float *scales1, const int8_t *w2, const void *bia2,
                       const float *scales2, const uint8_t *lut, const float *out_scales) {
  if (!h) return fail(DFX_ERR_INVALID, "se_set_weights: null handle");
  const dfx_se_desc &d = h->d;
  if (d.mode == DFX_SE_SQUEEZE) return fail(DFX_ERR_INVALID, "se_set_weights: DFX_SE_SQUEEZE takes no weights");
  if (!w1 || !scales1 || !w2 || !scales2 || !lut || !out_scales) return fail(DFX_ERR_INVALID, "se_set_weights: null argument");
  if ((d.bia1_dt != DFX_UNDEF && !bia1) || (d.bia2_dt != DFX_UNDEF && !bia2)) return fail(DFX_ERR_INVALID, "se_set_weights: null bias");
  const int cpad = h->generic.cpad, crpad = h->generic.crpad;
  std::vector<unsigned char> img(h->buf_bytes, 0);  // (the rows' padding stays 0)
  signed char *p1 = (signed char *)img.data(), *p2 = (signed char *)(img.data() + h->off_w2);
  for (int j = 0; j < d.cr; ++j) memcpy(p1 + (size_t)j * cpad, w1 + (size_t)j * d.c, (size_t)d.c);
  for (int k = 0; k < d.c; ++k) memcpy(p2 + (size_t)k * crpad, w2 + (size_t)k * d.cr, (size_t)d.cr);
  // the kernel reads activations as u8 - 128: the compensation 128 * sum of the row puts the 128 back
  requant_consts(d.cr, (size_t)d.c, [&](int j, size_t i) { return w1[(size_t)j * d.c + i]; }, bia1, d.bia1_dt, scales1, d.nscales1,
                 (int32_t *)(img.data() + h->off_c1), (float *)(img.data() + h->off_b1), (float *)(img.data() + h->off_s1));
  requant_consts(d.c, (size_t)d.cr, [&](int k, size_t i) { return w2[(size_t)k * d.cr + i]; }, bia2, d.bia2_dt, scales2, d.nscales2,
                 (int32_t *)(img.data() + h->off_c2), (float *)(img.data() + h->off_b2), (float *)(img.data() + h->off_s2));
  float *os = (float *)(img.data() + h->off_os);
  for (int k = 0; k < d.c; ++k) os[k] = out_scales[d.nscales_out == 1 ? 0 : k];
  memcpy(img.data() + h->off_lut, lut, 256);
  DeviceGuard dg(h->device);
  HIP_TRY(hipMemcpy(h->d_buf, img.data(), h->buf_bytes, hipMemcpyHostToDevice));
  h->weights_set = true;
  return DFX_OK;
}

int dfx_se_submit(dfx_se_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s) {
  if (!h || !src_dev || !dst_dev) return fail(DFX_ERR_INVALID, "se_submit: null argument");
  const dfx_se_desc &d = h->d;
  if (d.mode != DFX_SE_SQUEEZE && !h->weights_set) return fail(DFX_ERR_STATE, "se_submit: dfx_se_set_weights not called");
  const uintptr_t s0 = (uintptr_t)src_dev, d0 = (uintptr_t)dst_dev;
  // the scale kernel reads a byte where it then writes it, so dst may BE src; any other overlap would race.  The
  // {bs,c} result of the other modes has another shape than src and must lie apart from it.
  if (!(d.mode == DFX_SE_SCALE && s0 == d0) && s0 < d0 + dst_bytes(d) && d0 < s0 + src_bytes(d))
    return fail(DFX_ERR_INVALID, "se_submit: dst overlaps src without being src");
  DeviceGuard dg(h->device);
  const hipStream_t st = (hipStream_t)s;
  // 16-byte accesses need aligned buffers: others take the generic kernels for this submit, as pooling does
  const bool band = h->path == DFX_SE_BAND && (s0 | d0) % 16 == 0;
  SeArgs a = band ? h->band : h->generic;  // per-launch copy
  a.src = (const unsigned char *)src_dev;
  a.dst = (unsigned char *)dst_dev;
  // two or three launches through the handle's scratch: serialised (dfx.h; TwoLaunchOrder in dfx_internal.h)
  std::lock_guard<std::mutex> lk(h->order.mu);
  int rc = h->order.enter(st);
  if (rc) return rc;
  if (band) launch_se_squeeze(a, h->sq_grid, st);
  else launch_se_squeeze_generic(a, h->sq_grid_generic, st);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) {
    launch_se_excite(a, h->ex_grid, h->ex_block, h->ex_lds, st);
    e = hipGetLastError();
  }
  if (e == hipSuccess && d.mode == DFX_SE_SCALE) {
    if (band) launch_se_scale(a, h->sc_grid, st);
    else launch_se_scale_generic(a, h->sc_grid_generic, st);
    e = hipGetLastError();
  }
  // (once a launch is out the scratch has a writer in flight: every way out goes through leave())
  rc = h->order.leave(st);
  if (e != hipSuccess) return fail(DFX_ERR_HIP, "se_submit: %s", hipGetErrorString(e));
  return rc;
}

int dfx_se_submit_host(dfx_se_t *h, const void *src_host, void *dst_host) {
  if (!h || !src_host || !dst_host) return fail(DFX_ERR_INVALID, "se_submit_host: null argument");
  if (h->d.mode != DFX_SE_SQUEEZE && !h->weights_set) return fail(DFX_ERR_STATE, "se_submit_host: dfx_se_set_weights not called");
  DeviceGuard dg(h->device);
  return h->host.run(src_host, src_bytes(h->d), dst_host, dst_bytes(h->d),
                     [h](const void *s, void *d, dfx_stream_t st) { return dfx_se_submit(h, s, d, st); });
}

int dfx_se_query(const dfx_se_t *h, dfx_se_info *info) {
  if (!h || !info) return fail(DFX_ERR_INVALID, "se_query: null argument");
  memset(info, 0, sizeof(*info));
  const bool band = h->path == DFX_SE_BAND;
  info->path = h->path;
  info->slices = band ? h->band.slices : 1;
  info->grid = band ? h->sq_grid : h->sq_grid_generic;
  info->block = 256;
  info->lds_bytes = band ? se_squeeze_lds_bytes() : 0;
  info->device = h->device;
  info->algorithmic_bytes = (uint64_t)src_bytes(h->d) * (h->d.mode == DFX_SE_SCALE ? 2 : 1) + (uint64_t)dst_bytes(h->d);
  memcpy(info->kernel_name, h->kernel_name, sizeof(info->kernel_name));
  return DFX_OK;
}

int dfx_se_destroy(dfx_se_t *h) {
  release(h);
  return DFX_OK;
}

}  // extern "C"
