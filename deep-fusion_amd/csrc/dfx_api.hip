// dfx_api.hip -- host side of the C ABI declared in include/dfx.h.
//
// Host-side counterparts of the reference's op drivers:
//   validation        op_conv<T>::init_conf + jit_conv_kernel::init_conf
//                     (/root/reference/src/op_conv.cc:262-365, src/jit_conv_kernel.cc:512-673): conv_plan.h, which also
//                     decides kernel family, unit geometry, LDS layout and grid of a conv op (no HIP in there)
//   workspace/buffers op_conv<T>::op_conv (src/op_conv.h:70-95), util/memory.cc:21-40
//   dispatch          op_conv<T>::infer (src/op_conv.cc:22-29) -> ONE kernel launch
//   concat            op_concat<T> (src/op_concat.h:28-61), jit_concat_kernel::init_conf
//                     (src/jit_concat_kernel.cc:130-197)
// No CPU compute path exists here: without a usable HIP device every compute
// entry point returns an error.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "conv_mfma.cuh"
#include "conv_stream.cuh"
#include "conv_direct.cuh"
#include "conv_pw.cuh"
#include "conv_mfma_roles.cuh"
#include "dfx_device.cuh"
#include "dfx_internal.h"
#include "requant_host.h"
#pragma GCC visibility push(hidden)  // (the planner's inline functions are no part of the library's exported symbols)
#include "conv_plan.h"
#pragma GCC visibility pop

namespace dfx {
int launch_conv_generic(const ConvArgs &a, hipStream_t s, int *grid_out, int *lds_out);
#define DFX_DECL(n) \
  int launch_conv_mfma_##n(const ConvArgs &, const MfmaGeom &, int, int, int, int, int, hipStream_t, int)
DFX_DECL(f32);
DFX_DECL(s32);
DFX_DECL(s8);
DFX_DECL(u8);
#undef DFX_DECL
int launch_conv_mfma_roles_u8(const ConvArgs &, const MfmaGeom &, int, int, int, int, int, hipStream_t, int);
int launch_conv_mfma_roles_s8(const ConvArgs &, const MfmaGeom &, int, int, int, int, int, hipStream_t, int);
#define DFX_DECL(n) \
  int launch_conv_mfma_##n##_unfused(const ConvArgs &, const MfmaGeom &, int, int, int, int, hipStream_t, int)
DFX_DECL(f32);
DFX_DECL(s32);
DFX_DECL(s8);
DFX_DECL(u8);
#undef DFX_DECL

#define DFX_DECL(n) \
  int launch_conv_stream_##n(const ConvArgs &, const StreamGeom &, int, int, int, int, int, int, hipStream_t, int)
DFX_DECL(f32);
DFX_DECL(s32);
DFX_DECL(s8);
DFX_DECL(u8);
#undef DFX_DECL

#define DFX_DECL(n) \
  int launch_conv_direct_##n(const ConvArgs &, const DirectGeom &, int, int, int, int, int, int, hipStream_t, int)
DFX_DECL(f32);
DFX_DECL(s32);
DFX_DECL(s8);
DFX_DECL(u8);
#undef DFX_DECL

int launch_concat(const ConcatArgs &a, hipStream_t s);
int launch_pool(const PoolArgs &a, hipStream_t s);
int launch_eltwise(const EltwiseArgs &a, hipStream_t s);
}  // namespace dfx

using namespace dfx;

static thread_local char g_err[512] = "";

int dfx::fail(int code, const char *fmt, ...) {  // (declared in dfx_internal.h)
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

// ---- testing / tuning switches.  The environment is read ONCE, when the
//      library is first used; tests flip a switch afterwards with dfx_debug_set_tuning(). ----
namespace {
const char *const kTuningKeys[] = {"DFX_MAX_TH", "DFX_FORCE_GEOM", "DFX_UNIT_PX", "DFX_STATIC_ROUNDS", "DFX_NO_FAST", "DFX_NO_MAGIC", "DFX_NO_LAZY", "DFX_HALF_UNITS", "DFX_NO_ROLES", "DFX_STORE_BOUND_BYTES",
                                   "DFX_STREAM_PXB", "DFX_STREAM_BLOCKING", "DFX_STREAM_PLANES", "DFX_STREAM_OCC_PAR",
                                   "DFX_STREAM_DIRECT", "DFX_STREAM_PW", "DFX_DIRECT_NPB", "DFX_DIRECT_NW", "DFX_DIRECT_WO1", "DFX_STREAM_GRID", "DFX_DEBUG_PTRS", "DFX_DWCONV_GRID", "DFX_DWCONV_BAND", "DFX_DWPW_GRID", "DFX_DWPW_TH", "DFX_GCONV_GRID", "DFX_GCONV_TILE", "DFX_FC_SPLITK", "DFX_FC_GRID", "DFX_IMGCONV_GRID", "DFX_DECONV_GRID", "DFX_DILCONV_GRID", "DFX_DILCONV_SLAB", "DFX_DILCONV_STRIPS", "DFX_RESIZE_ROWS", "DFX_RESIZE_MAX_GRID", "DFX_SE_SLICES", "DFX_SE_GRID", "DFX_WSUM_GRID", "DFX_HEAD_GRID", "DFX_SELECT_CHUNK", "DFX_BMM_GRID", "DFX_ATTN_GRID", "DFX_LNORM_GRID", "DFX_LINEAR_GRID", "DFX_LINEAR_BM",
                                   "DEEPFUSION_PROFILE"};
struct Tuning {
  std::mutex mu;
  std::map<std::string, std::string> kv;
  Tuning() {
    for (const char *k : kTuningKeys)
      if (const char *v = getenv(k)) kv[k] = v;
  }
};
Tuning &tuning() {
  static Tuning t;
  return t;
}
// value of a switch or nullptr; the returned pointer stays valid until the switch is set again
// (thread_local copy: callers use it immediately)
const char *tune(const char *key) {
  static thread_local std::string held;
  Tuning &t = tuning();
  std::lock_guard<std::mutex> lk(t.mu);
  auto it = t.kv.find(key);
  if (it == t.kv.end()) return nullptr;
  held = it->second;
  return held.c_str();
}
// Streams made by dfx_stream_create that are still alive, each with a serial number that is never reused.  A conv
// handle remembers the serial of the first stream it was submitted on, so that it never hands the runtime a
// stream that dfx_stream_destroy has destroyed since (hipEventRecord on such a handle crashes: the runtime
// looks into the stream object before it validates it).  Streams made elsewhere have serial 0: not tracked.
struct StreamRegistry {
  std::mutex mu;
  std::map<hipStream_t, unsigned long long> live;
  unsigned long long next = 1;
};
StreamRegistry &streams() {
  static StreamRegistry r;
  return r;
}
unsigned long long stream_serial(hipStream_t st) {
  StreamRegistry &r = streams();
  std::lock_guard<std::mutex> lk(r.mu);
  auto it = r.live.find(st);
  return it == r.live.end() ? 0ull : it->second;
}
}  // namespace

unsigned long long dfx::stream_serial_of(hipStream_t st) { return stream_serial(st); }  // (declared in dfx_internal.h)
const char *dfx::tuning_value(const char *key) { return tune(key); }                     // (declared in dfx_internal.h)

// launches of one MFMA-variant handle that may be in flight at the same time (any streams)
constexpr unsigned DFX_QUEUE_RING = 16;

struct dfx_conv : ConvPlan {  // (the plan: kernel family, geometry, grid, LDS, kernel name -- conv_plan.h)
  int device;  // ordinal the handle lives on (current device at dfx_conv_create)
  dfx_conv_desc d;
  ConvArgs args;
  // role-specialised fused kernel (conv_mfma_roles.cuh): roles_ok (ConvPlan) = the SHAPE fits it, roles = the WEIGHTS
  // allow its requant modes (decided by dfx_conv_set_weights); otherwise the op runs on conv_mfma.cuh's kernel
  bool roles;
  void *d_wei, *d_wei1, *d_consts;
  int *d_queue;  // MFMA variant: ring of DFX_QUEUE_RING x {next unit, finished loaders}, one slot per launch in flight
  unsigned launch_seq;
  // In-flight guard of the queue ring.  Launches on ONE stream are ordered by the stream; as soon as a handle
  // has been submitted on a second stream every launch records its slot's event, and a launch that finds its
  // slot last used on another stream first waits (on the device) for that launch: a 17th concurrent launch
  // queues up behind the 1st instead of sharing its queue words.  The launches made while there was one stream
  // only carry no events of their own: when the second stream appears, ONE event recorded on first_stream
  // (first_ev, owned by the handle, shared by their slots) stands for all of them, so that a third, fourth ...
  // stream that reuses one of those slots waits as well.
  std::mutex *ring_mu;
  hipEvent_t slot_ev[DFX_QUEUE_RING];
  hipStream_t slot_stream[DFX_QUEUE_RING];
  unsigned char slot_state[DFX_QUEUE_RING];  // 0 never used, 1 used (no event recorded), 2 used + event recorded
  bool multi_stream;
  hipStream_t first_stream;
  unsigned long long first_serial;  // stream_serial(first_stream) at the first launch (0: not one of dfx_stream_create's)
  hipEvent_t first_ev;  // see above; slot_ev[i] == first_ev marks a slot that borrows it (never destroyed per slot)
  int ring_waits;       // hipStreamWaitEvent calls the guard has issued so far (dfx_debug_conv_sched)
  int *trace_host;  // DFX_TRACE builds only
  unsigned long long *d_prof;  // DFX_STAMPS builds only
  bool weights_set;
  HostStaging host;  // dfx_conv_submit_host
};

struct dfx_concat {
  int device;
  dfx_concat_desc d;
  std::vector<int> channels;
  ConcatArgs args;
  HostStaging host;  // dfx_concat_submit_host
};

extern "C" {

int dfx_version(void) { return DFX_VERSION; }
const char *dfx_last_error(void) { return g_err; }

int dfx_device_count(int *count) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) n = 0;
  if (count) *count = n;
  return DFX_OK;
}

int dfx_set_device(int ordinal) {
  HIP_TRY(hipSetDevice(ordinal));
  return DFX_OK;
}

int dfx_device_name(char *buf, size_t len) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  hipDeviceProp_t p;
  HIP_TRY(hipGetDeviceProperties(&p, dev));
  snprintf(buf, len, "%s (%s, %d CUs)", p.name, p.gcnArchName, p.multiProcessorCount);
  return DFX_OK;
}

int dfx_mem_alloc_host(void **p, size_t bytes) {
  HIP_TRY(hipHostMalloc(p, bytes ? bytes : 1, hipHostMallocDefault));
  return DFX_OK;
}
int dfx_mem_free_host(void *p) {
  if (p) HIP_TRY(hipHostFree(p));
  return DFX_OK;
}
int dfx_mem_alloc_device(void **p, size_t bytes) {
  HIP_TRY(hipMalloc(p, bytes ? bytes : 1));
  return DFX_OK;
}
int dfx_mem_free_device(void *p) {
  if (p) HIP_TRY(hipFree(p));
  return DFX_OK;
}
int dfx_memcpy_h2d(void *dst, const void *src, size_t bytes, dfx_stream_t s) {
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)s));
  return DFX_OK;
}
int dfx_memcpy_d2h(void *dst, const void *src, size_t bytes, dfx_stream_t s) {
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)s));
  return DFX_OK;
}
int dfx_memset_device(void *dst, int value, size_t bytes, dfx_stream_t s) {
  HIP_TRY(hipMemsetAsync(dst, value, bytes, (hipStream_t)s));
  return DFX_OK;
}
int dfx_stream_create(dfx_stream_t *s) {
  hipStream_t st;
  HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  {
    StreamRegistry &r = streams();
    std::lock_guard<std::mutex> lk(r.mu);
    r.live[st] = r.next++;
  }
  *s = st;
  return DFX_OK;
}
int dfx_stream_destroy(dfx_stream_t s) {
  if (!s) return DFX_OK;
  {
    StreamRegistry &r = streams();
    std::lock_guard<std::mutex> lk(r.mu);
    r.live.erase((hipStream_t)s);
  }
  HIP_TRY(hipStreamDestroy((hipStream_t)s));
  return DFX_OK;
}
int dfx_stream_sync(dfx_stream_t s) {
  HIP_TRY(hipStreamSynchronize((hipStream_t)s));
  return DFX_OK;
}
int dfx_stream_wait_stream(dfx_stream_t waiter, dfx_stream_t producer) {
  if (waiter == producer) return DFX_OK;
  // the event must live on the PRODUCER stream's device (the streams of a multi-device pipeline differ)
  int cur = -1, pdev = -1;
  (void)hipGetDevice(&cur);
  if (producer && hipStreamGetDevice((hipStream_t)producer, &pdev) != hipSuccess) pdev = -1;
  if (pdev >= 0 && pdev != cur) (void)hipSetDevice(pdev);
  hipEvent_t e = nullptr;
  hipError_t r = hipEventCreateWithFlags(&e, hipEventDisableTiming);
  if (r == hipSuccess) r = hipEventRecord(e, (hipStream_t)producer);
  if (pdev >= 0 && pdev != cur) (void)hipSetDevice(cur);
  if (r == hipSuccess) r = hipStreamWaitEvent((hipStream_t)waiter, e, 0);
  if (e) (void)hipEventDestroy(e);  // (released once the recorded work has completed)
  HIP_TRY(r);
  return DFX_OK;
}
int dfx_event_create(dfx_event_t *e) {
  hipEvent_t ev;
  HIP_TRY(hipEventCreate(&ev));
  *e = ev;
  return DFX_OK;
}
int dfx_event_record(dfx_event_t e, dfx_stream_t s) {
  HIP_TRY(hipEventRecord((hipEvent_t)e, (hipStream_t)s));
  return DFX_OK;
}
int dfx_event_elapsed_ms(dfx_event_t start, dfx_event_t stop, float *ms) {
  HIP_TRY(hipEventSynchronize((hipEvent_t)stop));
  HIP_TRY(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
  return DFX_OK;
}
int dfx_event_destroy(dfx_event_t e) {
  if (e) HIP_TRY(hipEventDestroy((hipEvent_t)e));
  return DFX_OK;
}

size_t dfx_blocked_offset(int o, int i, int kh, int kw, int I, int KH, int KW) {
  // [o/16][i/16][kh][kw][(i%16)/4][o%16][i%4], jit_conv_kernel.cc:333-338
  const size_t nb_ic = (size_t)I / 16;
  return ((((size_t)(o / 16) * nb_ic + (size_t)(i / 16)) * KH + kh) * KW + kw) * 256 +
         (size_t)((i % 16) / 4) * 64 + (size_t)(o % 16) * 4 + (size_t)(i % 4);
}

int dfx_reorder_oihw_to_blocked(const int8_t *oihw, int8_t *blocked, int O, int I, int KH,
                                int KW) {
  if (!oihw || !blocked || O <= 0 || I <= 0 || O % 16 || I % 16 || KH <= 0 || KW <= 0)
    return fail(DFX_ERR_INVALID, "reorder: O and I must be positive multiples of 16");
  for (int o = 0; o < O; ++o)
    for (int i = 0; i < I; ++i)
      for (int h = 0; h < KH; ++h)
        for (int w = 0; w < KW; ++w)
          blocked[dfx_blocked_offset(o, i, h, w, I, KH, KW)] =
              oihw[(((size_t)o * I + i) * KH + h) * KW + w];
  return DFX_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// conv
// ---------------------------------------------------------------------------

namespace dfx { int launch_conv_pw(const ConvArgs &, const PwGeom &, int, int, int, hipStream_t, int); }

static int direct_dispatch(dfx_conv *h, const ConvArgs &a, hipStream_t s, int mode) {
  if (h->pw) {  // pointwise unfused conv (conv_pw.cuh); the requant proofs live in dgeom (set_weights_direct)
    PwGeom pg = h->pwgeom;
    pg.fast = h->dgeom.fast;
    pg.m0 = h->dgeom.m0;
    return dfx::launch_conv_pw(a, pg, h->d.dst_dt, h->grid, h->lds, s, mode);
  }
  switch (h->d.dst_dt) {
    case DFX_F32: return launch_conv_direct_f32(a, h->dgeom, h->nw, h->wo, h->G, h->wo1, h->grid, h->lds, s, mode);
    case DFX_S32: return launch_conv_direct_s32(a, h->dgeom, h->nw, h->wo, h->G, h->wo1, h->grid, h->lds, s, mode);
    case DFX_S8: return launch_conv_direct_s8(a, h->dgeom, h->nw, h->wo, h->G, h->wo1, h->grid, h->lds, s, mode);
    case DFX_U8: return launch_conv_direct_u8(a, h->dgeom, h->nw, h->wo, h->G, h->wo1, h->grid, h->lds, s, mode);
  }
  return -1;
}

bool dfx::conv_pw_view(const dfx_conv *h, ConvArgs *args, PwGeom *geom, int *lds) {  // (declared in dfx_internal.h)
  if (!h || !h->pw || h->variant != DFX_VARIANT_MFMA_STREAM) return false;
  *args = h->args;
  *geom = h->pwgeom;
  geom->fast = h->dgeom.fast;
  geom->m0 = h->dgeom.m0;
  *lds = h->lds;
  return true;
}

static int stream_dispatch(dfx_conv *h, const ConvArgs &a, hipStream_t s, int mode) {
  const int fused = h->d.oc1x1 > 0;
  switch (h->d.dst_dt) {
    case DFX_F32: return launch_conv_stream_f32(a, h->sgeom, h->occ, h->G, h->pxb, fused, h->grid, h->lds, s, mode);
    case DFX_S32: return launch_conv_stream_s32(a, h->sgeom, h->occ, h->G, h->pxb, fused, h->grid, h->lds, s, mode);
    case DFX_S8: return launch_conv_stream_s8(a, h->sgeom, h->occ, h->G, h->pxb, fused, h->grid, h->lds, s, mode);
    case DFX_U8: return launch_conv_stream_u8(a, h->sgeom, h->occ, h->G, h->pxb, fused, h->grid, h->lds, s, mode);
  }
  return -1;
}

// `a` and `g` are per-launch copies (src/dst pointers, queue slot): submits of one handle do not
// share mutable host state
static int mfma_dispatch(dfx_conv *h, const ConvArgs &a, const MfmaGeom &g, hipStream_t s, int mode) {
  if (h->variant == DFX_VARIANT_MFMA_STREAM) return h->direct ? direct_dispatch(h, a, s, mode) : stream_dispatch(h, a, s, mode);
  if (h->variant == DFX_VARIANT_MFMA_CONV) {
    switch (h->d.dst_dt) {
      case DFX_F32: return launch_conv_mfma_f32_unfused(a, g, h->icb, h->ocb, h->grid, h->lds, s, mode);
      case DFX_S32: return launch_conv_mfma_s32_unfused(a, g, h->icb, h->ocb, h->grid, h->lds, s, mode);
      case DFX_S8: return launch_conv_mfma_s8_unfused(a, g, h->icb, h->ocb, h->grid, h->lds, s, mode);
      case DFX_U8: return launch_conv_mfma_u8_unfused(a, g, h->icb, h->ocb, h->grid, h->lds, s, mode);
    }
    return -1;
  }
  if (h->roles_ok && (mode == 1 || h->roles)) {
    const int ncb = h->d.oc1x1 / 32;
    const int rc = h->d.dst_dt == DFX_U8 ? launch_conv_mfma_roles_u8(a, g, h->icb, h->ocb, ncb, h->grid, h->lds, s, mode)
                                         : launch_conv_mfma_roles_s8(a, g, h->icb, h->ocb, ncb, h->grid, h->lds, s, mode);
    if (mode != 1 || rc != 0) return rc;  // (mode 1 raises the LDS limit of BOTH kernels)
  }
  switch (h->d.dst_dt) {
    case DFX_F32: return launch_conv_mfma_f32(a, g, h->icb, h->ocb, h->G, h->grid, h->lds, s, mode);
    case DFX_S32: return launch_conv_mfma_s32(a, g, h->icb, h->ocb, h->G, h->grid, h->lds, s, mode);
    case DFX_S8: return launch_conv_mfma_s8(a, g, h->icb, h->ocb, h->G, h->grid, h->lds, s, mode);
    case DFX_U8: return launch_conv_mfma_u8(a, g, h->icb, h->ocb, h->G, h->grid, h->lds, s, mode);
  }
  return -1;
}

// releases everything a conv handle owns (also used on dfx_conv_create's failure paths)
static void conv_release(dfx_conv *h) {
  if (!h) return;
  DeviceGuard dg(h->device);
  h->host.release();
  (void)hipFree(h->d_wei); (void)hipFree(h->d_wei1); (void)hipFree(h->d_consts);
  (void)hipFree(h->d_queue);
  (void)hipFree(h->d_prof);
  for (unsigned i = 0; i < DFX_QUEUE_RING; ++i)
    if (h->slot_ev[i] && h->slot_ev[i] != h->first_ev) (void)hipEventDestroy(h->slot_ev[i]);
  if (h->first_ev) (void)hipEventDestroy(h->first_ev);
  delete h->ring_mu;
  delete h;
}

// dfx_conv_create behind the descriptor and device checks: plans the op (conv_plan.h), allocates what the plan calls
// for and raises the kernel's LDS limit.  On failure the caller releases the handle.
static int conv_build(dfx_conv *h) {
  const dfx_conv_desc &d = h->d;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, h->device) != hipSuccess) return fail(DFX_ERR_HIP, "conv_create: cannot query the device");
  ConvEnv env;
  env.ncu = prop.multiProcessorCount;
  env.tune = tune;
  env.ctx = h;  // (the plan being made is the handle's base: the launchers' modes 1 and 2 see it as it stands)
  env.wg_per_cu = [](void *ctx, const ConvPlan &) {
    dfx_conv *hh = static_cast<dfx_conv *>(ctx);
    return mfma_dispatch(hh, hh->args, hh->geom, nullptr, 1) != 0 ? -1 : mfma_dispatch(hh, hh->args, hh->geom, nullptr, 2);
  };
  const char *why = "";
  const int rc = conv_plan(d, env, h, &why);
  if (rc) return fail(rc, "%s", why);
  h->args.rows_per_unit = h->rows_per_unit;
  h->args.units_per_image = h->units_per_image;
  const bool resident = h->variant == DFX_VARIANT_MFMA_FUSED || h->variant == DFX_VARIANT_MFMA_CONV;
  [[maybe_unused]] const bool direct = h->variant == DFX_VARIANT_MFMA_STREAM && h->direct;  // conv_direct.cuh, conv_pw.cuh
  if (resident) {
    if (hipMalloc((void **)&h->d_queue, 8 * DFX_QUEUE_RING) != hipSuccess ||
        hipMemset(h->d_queue, 0, 8 * DFX_QUEUE_RING) != hipSuccess)
      return fail(DFX_ERR_HIP, "conv_create: cannot allocate the unit queue");
    h->geom.queue = h->d_queue;
    h->ring_mu = new (std::nothrow) std::mutex();
    if (!h->ring_mu) return fail(DFX_ERR_HIP, "out of host memory");
  }
#ifdef DFX_STAMPS
  if (h->variant != DFX_VARIANT_GENERIC) {
    // resident: [grid][16 waves][16] sums, then [grid][16 waves][8 events][4] timeline words
    const size_t bytes = resident ? (size_t)h->grid * 768 * 8 : direct ? (size_t)h->grid * h->nw * 16 * 8 : (size_t)h->grid * 96 * 8;
    if (hipMalloc((void **)&h->d_prof, bytes) != hipSuccess || hipMemset(h->d_prof, 0, bytes) != hipSuccess)
      return fail(DFX_ERR_HIP, "conv_create: cannot allocate the stamp buffer");
    (resident ? h->geom.prof : direct ? h->dgeom.prof : h->sgeom.prof) = h->d_prof;
  }
#endif
#ifdef DK_DEBUG
  if (direct) {
    if (hipMalloc((void **)&h->d_prof, 64 * 8) != hipSuccess || hipMemset(h->d_prof, 0xff, 64 * 8) != hipSuccess)
      return fail(DFX_ERR_HIP, "conv_create: cannot allocate the debug buffer");
    h->dgeom.dbg = (long long *)h->d_prof;
    h->dgeom.src_bytes = (long long)d.bs * d.ih * d.iw * d.ic;
    h->dgeom.dst_bytes = (long long)d.bs * d.oh * d.ow * (d.oc1x1 ? d.oc1x1 : d.oc) * (long long)dt_size(d.dst_dt);
  }
#endif
#ifdef DFX_TRACE
  if (resident) {
    void *hp = nullptr, *dp = nullptr;
    if (hipHostMalloc(&hp, (size_t)h->grid * 16 * 4 * 4, hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer(&dp, hp, 0) != hipSuccess)
      return fail(DFX_ERR_HIP, "conv_create: cannot allocate the trace buffer");
    memset(hp, 0, (size_t)h->grid * 16 * 4 * 4);
    h->trace_host = (int *)hp;
    h->geom.trace = (int *)dp;
  }
#endif
  if (h->variant != DFX_VARIANT_GENERIC && mfma_dispatch(h, h->args, h->geom, nullptr, 1) != 0)
    return fail(DFX_ERR_HIP, "conv_create: cannot raise dynamic LDS limit to %d bytes", h->lds);
  return DFX_OK;
}

extern "C" {

int dfx_conv_create(const dfx_conv_desc *desc, dfx_conv_t **out) {
  if (!desc || !out) return fail(DFX_ERR_INVALID, "conv_create: null argument");
  *out = nullptr;
  const char *why = "";
  int rc = conv_validate(*desc, &why);
  if (rc) return fail(rc, "%s", why);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(DFX_ERR_NO_DEVICE, "conv_create: no HIP device (this library has no CPU path)");

  dfx_conv *h = new (std::nothrow) dfx_conv();  // (value-initialised: every plain field starts as zero)
  if (!h) return fail(DFX_ERR_HIP, "out of host memory");
  h->d = *desc;
  if (hipGetDevice(&h->device) != hipSuccess) h->device = 0;
  const dfx_conv_desc &d = h->d;

  ConvArgs &a = h->args;
  a.bs = d.bs; a.ic = d.ic; a.ih = d.ih; a.iw = d.iw; a.oc = d.oc; a.oh = d.oh; a.ow = d.ow;
  a.kh = d.kh; a.kw = d.kw; a.sh = d.sh; a.sw = d.sw; a.pt = d.pad_t; a.pl = d.pad_l;
  a.oc1 = d.oc1x1; a.dst_dt = d.dst_dt; a.relu0 = d.conv0_relu; a.relu1 = d.conv1_relu;
  a.rm0 = d.conv0_round_mode; a.rm1 = d.conv1_round_mode;

  rc = conv_build(h);
  if (rc) {
    conv_release(h);  // (the message is recorded: releasing does not touch it)
    return rc;
  }
  *out = h;
  return DFX_OK;
}

// One channel's precondition of the fast requant path (conv_mfma.cuh store_group<FAST>):
// amax bounds |true accumulator|; comp + bias must fold into ONE exact f32 add (bias
// integer-valued, |comp + bias| < 2^24, |acc + bias| < 2^24) and nothing may reach +-2^31.
static bool fast_ok_channel(double amax, double comp, float bias, float scale) {
  if (!std::isfinite(bias) || !std::isfinite(scale)) return false;
  const double b = bias;
  if (b != std::floor(b)) return false;
  const double lim = 16777216.0;  // 2^24
  if (std::fabs(comp + b) >= lim || amax + std::fabs(b) >= lim || std::fabs(comp) + amax >= lim) return false;
  return (amax + std::fabs(b)) * std::fabs((double)scale) * 1.0001 + 2.0 < 2147480000.0;
}

// The constants of conv_stream.cuh and conv_direct.cuh: comp0 (s32) bias0 scale0 [OCP each] comp1 (s32) bias1 scale1
// [OC1P each]; padding channels are all-zero (their intermediate is 0 and meets zero 1x1 weights).  fb0 / fb1: the
// biases as f32.  Returns whether the fast requant path is proven for every channel of both stages; the bias slots
// then hold comp + bias.
static bool stream_consts(const dfx_conv_desc &d, int OCP, int OC1P, const int8_t *wei, const void *bia0, const float *scales0,
                          const int8_t *wei1, const void *bia1, const float *scales1, std::vector<int32_t> &cst,
                          std::vector<float> &fb0, std::vector<float> &fb1) {
  const int OC = d.oc, IC = d.ic, OC1 = d.oc1x1, ntap = d.kh * d.kw;
  cst.assign((size_t)3 * (OCP + OC1P), 0);
  auto put_f = [&](size_t idx, float v) { memcpy(&cst[idx], &v, 4); };
  bool fast = d.conv0_round_mode == DFX_ROUND_NEAREST && (OC1 == 0 || d.conv1_round_mode == DFX_ROUND_NEAREST);
  fb0.assign(OC, 0.0f);
  fb1.assign(OC1 ? OC1 : 1, 0.0f);
  for (int c = 0; c < OC; ++c) {
    int32_t sum = 0, pos = 0, neg = 0;
    for (int ic = 0; ic < IC; ++ic)
      for (int tap = 0; tap < ntap; ++tap) {
        const int w = wei[dfx_blocked_offset(c, ic, tap / d.kw, tap % d.kw, IC, d.kh, d.kw)];
        sum += w;
        (w > 0 ? pos : neg) += w;
      }
    cst[c] = 128 * sum;
    fb0[c] = d.bia0_dt == DFX_UNDEF ? 0.0f : bias_to_f32(bia0, d.bia0_dt, c);
    const float sc = scales0[d.conv0_nscales > 1 ? c : 0];
    put_f((size_t)OCP + c, fb0[c]);
    put_f((size_t)2 * OCP + c, sc);
    fast = fast && fast_ok_channel(255.0 * std::max(pos, -neg), 128.0 * sum, fb0[c], sc);
  }
  for (int c = 0; c < OC1; ++c) {
    int32_t sum = 0, pos = 0, neg = 0;
    for (int oc = 0; oc < OC; ++oc) {
      const int w = wei1[dfx_blocked_offset(c, oc, 0, 0, OC, 1, 1)];
      sum += w;
      (w > 0 ? pos : neg) += w;
    }
    cst[(size_t)3 * OCP + c] = 128 * sum;
    fb1[c] = d.bia1_dt == DFX_UNDEF ? 0.0f : bias_to_f32(bia1, d.bia1_dt, c);
    const float sc = scales1[d.conv1_nscales > 1 ? c : 0];
    put_f((size_t)3 * OCP + OC1P + c, fb1[c]);
    put_f((size_t)3 * OCP + 2 * OC1P + c, sc);
    fast = fast && fast_ok_channel(255.0 * std::max(pos, -neg), 128.0 * sum, fb1[c], sc);
  }
  fast = fast && fast_allowed();
  if (fast) {  // the fast path reads comp + bias (an exact f32) from the bias slot
    for (int c = 0; c < OC; ++c) put_f((size_t)OCP + c, (float)((double)cst[c] + (double)fb0[c]));
    for (int c = 0; c < OC1; ++c)
      put_f((size_t)3 * OCP + OC1P + c, (float)((double)cst[(size_t)3 * OCP + c] + (double)fb1[c]));
  }
  return fast;
}

// Packs weights for conv_stream.cuh: ONE device buffer
//   [conv0 steps | conv1 steps | consts], a step = 2 k-blocks x (OCC | G) fragments of 1 KB,
// in the exact order the kernel walks them (oc chunk, ic chunk, step; 1x1 group, step).
static int set_weights_direct(dfx_conv_t *h, const int8_t *wei, const void *bia0, const float *scales0,
                              const int8_t *wei1, const void *bia1, const float *scales1);

static int set_weights_stream(dfx_conv_t *h, const int8_t *wei, const void *bia0, const float *scales0,
                              const int8_t *wei1, const void *bia1, const float *scales1) {
  if (h->direct) return set_weights_direct(h, wei, bia0, scales0, wei1, bia1, scales1);
  const dfx_conv_desc &d = h->d;
  const StreamGeom &g = h->sgeom;
  const bool fused = d.oc1x1 > 0;
  const int OCC = h->occ, G = h->G, OC = d.oc, IC = d.ic, OC1 = d.oc1x1;
  const int OCP = 32 * g.ocb, OC1P = fused ? 32 * G * g.n_g1 : 0;
  const size_t n0 = (size_t)g.s0_steps * 2 * OCC * 1024;
  const size_t n1 = fused ? (size_t)g.n_g1 * g.ks2 * 2 * G * 1024 : 0;
  std::vector<int8_t> pk(n0 + n1, 0);
  const int ntap = d.kh * d.kw;
  size_t o = 0;
  for (int occ = 0; occ < g.n_occ; ++occ)
    for (int icc = 0; icc < g.n_icc; ++icc) {
      const int kbn = std::min(2, g.icb - 2 * icc), ns = ntap * kbn;
      for (int s2 = 0; s2 < (ns + 1) / 2; ++s2)
        for (int j = 0; j < 2; ++j)
          for (int r = 0; r < OCC; ++r)
            for (int lane = 0; lane < 64; ++lane)
              for (int b = 0; b < 16; ++b, ++o) {
                const int s = 2 * s2 + j;
                if (s >= ns) continue;  // padding k-block: zero weights
                const int tap = s / kbn, icbl = s % kbn;
                // fused: A operand, row = channel 32*(occ*OCC + r) + rho.  unfused: B operand with
                // the store stage's channel permutation: column lam of block r = 32*OCC*occ + OCC*lam + r
                const int oc = fused ? 32 * (occ * OCC + r) + (lane & 31) : 32 * OCC * occ + OCC * (lane & 31) + r;
                const int ic = 64 * icc + 32 * icbl + 16 * (lane >> 5) + b;
                if (oc < OC && ic < IC) pk[o] = wei[dfx_blocked_offset(oc, ic, tap / d.kw, tap % d.kw, IC, d.kh, d.kw)];
              }
    }
  if (o != n0) return fail(DFX_ERR_HIP, "internal: conv0 pack size mismatch");
  for (int g1 = 0; g1 < g.n_g1; ++g1)
    for (int s2 = 0; s2 < g.ks2; ++s2)
      for (int j = 0; j < 2; ++j)
        for (int cc = 0; cc < G; ++cc)
          for (int lane = 0; lane < 64; ++lane)
            for (int b = 0; b < 16; ++b, ++o) {
              const int blk = 2 * s2 + j;
              if (blk >= g.ocb) continue;
              const int oc1 = 32 * G * g1 + G * (lane & 31) + cc;
              const int oc = 32 * blk + 8 * (b >> 2) + 4 * (lane >> 5) + (b & 3);  // mid's k order
              if (oc1 < OC1 && oc < OC) pk[o] = wei1[dfx_blocked_offset(oc1, oc, 0, 0, OC, 1, 1)];
            }
  std::vector<int32_t> cst;
  std::vector<float> fb0, fb1;
  const bool fast = stream_consts(d, OCP, OC1P, wei, bia0, scales0, wei1, bia1, scales1, cst, fb0, fb1);
  h->sgeom.fast = fast ? 1 : 0;
  if (!h->d_wei) HIP_TRY(hipMalloc(&h->d_wei, pk.size() + cst.size() * 4));
  char *base = (char *)h->d_wei;
  HIP_TRY(hipMemcpy(base, pk.data(), pk.size(), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(base + pk.size(), cst.data(), cst.size() * 4, hipMemcpyHostToDevice));
  h->args.wei = (const int8_t *)base;
  h->args.wei1 = (const int8_t *)(base + n0);
  h->args.consts = (const float *)(base + pk.size());
  h->weights_set = true;
  return DFX_OK;
}

// Packs weights for conv_direct.cuh: ONE device buffer [W0d | W1d | consts].
//   W0d[ob][kb = icb * ntap + tap][lane][16]: byte b of lane = W0[oc = 32 ob + (lane & 31)][ic = 32 icb + 16 (lane >> 5) + b][tap]
//   W1d[g1][blk][cc][lane][16]: byte b = W1[oc1 = 32 G g1 + G (lane & 31) + cc][oc = 32 blk + 8 (b >> 2) + 4 (lane >> 5) + (b & 3)]
static int set_weights_direct(dfx_conv_t *h, const int8_t *wei, const void *bia0, const float *scales0,
                              const int8_t *wei1, const void *bia1, const float *scales1) {
  const dfx_conv_desc &d = h->d;
  const DirectGeom &g = h->dgeom;
  const int G = h->G, OC = d.oc, IC = d.ic, OC1 = d.oc1x1;
  const int OCP = 32 * g.ocb, OC1P = 32 * G * g.n_g1;
  const int ntap = d.kh * d.kw, nkb0 = g.icb * ntap;
  const size_t n0 = (size_t)g.ocb * nkb0 * 1024, n1 = (size_t)g.n_g1 * g.ocb * G * 1024;
  std::vector<int8_t> pk(n0 + n1, 0);
  size_t o = 0;
  for (int ob = 0; ob < g.ocb; ++ob)
    for (int icb = 0; icb < g.icb; ++icb)
      for (int tap = 0; tap < ntap; ++tap)
        for (int lane = 0; lane < 64; ++lane)
          for (int b = 0; b < 16; ++b, ++o) {
            const int oc = 32 * ob + (lane & 31), ic = 32 * icb + 16 * (lane >> 5) + b;
            if (oc < OC && ic < IC) pk[o] = wei[dfx_blocked_offset(oc, ic, tap / d.kw, tap % d.kw, IC, d.kh, d.kw)];
          }
  for (int g1 = 0; g1 < g.n_g1; ++g1)
    for (int blk = 0; blk < g.ocb; ++blk)
      for (int cc = 0; cc < G; ++cc)
        for (int lane = 0; lane < 64; ++lane)
          for (int b = 0; b < 16; ++b, ++o) {
            const int oc1 = 32 * G * g1 + G * (lane & 31) + cc;
            const int oc = 32 * blk + 8 * (b >> 2) + 4 * (lane >> 5) + (b & 3);
            if (oc1 < OC1 && oc < OC) pk[o] = wei1[dfx_blocked_offset(oc1, oc, 0, 0, OC, 1, 1)];
          }
  if (o != n0 + n1) return fail(DFX_ERR_HIP, "internal: direct pack size mismatch");
  std::vector<int32_t> cst;
  std::vector<float> fb0, fb1;
  const bool fast = stream_consts(d, OCP, OC1P, wei, bia0, scales0, wei1, bia1, scales1, cst, fb0, fb1);
  auto put_f = [&](size_t idx, float v) { memcpy(&cst[idx], &v, 4); };
  h->dgeom.fast = fast ? 1 : 0;
  // Requant without int -> float conversions (conv_direct.cuh, round 3), proven per channel from the actual
  // weights like the modes of the resident kernels: with activations stored as u8 - 128 the raw accumulator lies
  // in [-(128 P + 127 N), 127 P + 128 N] (P / N = sums of the positive / negative weights' magnitudes).
  //   m0  stage 0 "fma": start value bits(2^23) + comp + bias, t = acc + bias inside (-2^23, 2^23), bias
  //       integer-valued, scale >= 0: comp slot <- start bits, bias slot <- -2^23 * scale
  //   m1  stage 1 "magic" (u8 output through the 16-byte store path only): start 1/(2 pi), conditions of
  //       magic1_ok; bias slot <- (comp + bias - 2^23 - 0x22F983) * 2^-26, scale slot <- scale * 2^26 (m1 = 2),
  //       or bias slot <- (comp + bias - 2^23 - 0x22F983) * scale where that product is exact for every channel:
  //       one fma (m1 = 3)
  h->dgeom.m0 = h->dgeom.m1 = 0;
  const bool no_magic = tune("DFX_NO_MAGIC") && atoi(tune("DFX_NO_MAGIC")) != 0;
  if (fast && !no_magic) {
    auto pn = [&](bool stage1, int c, double &P, double &N) {
      P = N = 0;
      if (!stage1) {
        for (int ic = 0; ic < IC; ++ic)
          for (int tap = 0; tap < ntap; ++tap) {
            const int w = wei[dfx_blocked_offset(c, ic, tap / d.kw, tap % d.kw, IC, d.kh, d.kw)];
            (w > 0 ? P : N) += std::abs(w);
          }
      } else {
        for (int oc = 0; oc < OC; ++oc) {
          const int w = wei1[dfx_blocked_offset(c, oc, 0, 0, OC, 1, 1)];
          (w > 0 ? P : N) += std::abs(w);
        }
      }
    };
    // (stage 0's "fma" route relies on the unsigned saturation of a u8 result: the fused intermediate, or a u8 dst)
    bool m0 = OC1 > 0 || d.dst_dt == DFX_U8;
    for (int c = 0; c < OC && m0; ++c) {
      double P, N;
      pn(false, c, P, N);
      const float sc = scales0[d.conv0_nscales > 1 ? c : 0];
      const double b = fb0[c], cb = 128.0 * (P - N) + b;
      m0 = b == std::floor(b) && sc >= 0.0f && std::isfinite(sc * 8388608.0f) &&
           -(128.0 * P + 127.0 * N) + cb > -8388608.0 && 127.0 * P + 128.0 * N + cb < 8388608.0;
    }
    if (m0) {
      for (int c = 0; c < OC; ++c) {
        const float sc = scales0[d.conv0_nscales > 1 ? c : 0];
        cst[c] = MAGIC3_BITS + cst[c] + (int32_t)fb0[c];
        put_f((size_t)OCP + c, -8388608.0f * sc);
      }
      h->dgeom.m0 = 1;
    }
    bool m1 = d.dst_dt == DFX_U8 && G == 4 && OC1 > 0, fma1 = true;
    for (int c = 0; c < OC1 && m1; ++c) {
      double P, N;
      pn(true, c, P, N);
      const float sc = scales1[d.conv1_nscales > 1 ? c : 0];
      const double b = fb1[c], cb = 128.0 * (P - N) + b, lo = -(128.0 * P + 127.0 * N), hi = 127.0 * P + 128.0 * N;
      const double k = cb - 8388608.0 - (double)0x22F983;
      m1 = b == std::floor(b) && lo >= (double)MAGIC1_LO && hi <= (double)MAGIC1_HI && std::fabs(k) < 16777216.0 &&
           std::fabs(lo + cb) < 16777216.0 && std::fabs(hi + cb) < 16777216.0 && std::isfinite(sc * 67108864.0f);
      const double prod = k * (double)sc;
      fma1 = fma1 && std::isfinite(prod) && (double)(float)prod == prod;
    }
    m1 = m1 && m0;  // (the kernels specialise on "both stages without conversions": conv_direct.cuh, QM)
    if (m1) {
      for (int c = 0; c < OC1; ++c) {
        const float sc = scales1[d.conv1_nscales > 1 ? c : 0];
        const double k = (double)cst[(size_t)3 * OCP + c] + (double)fb1[c] - 8388608.0 - (double)0x22F983;
        put_f((size_t)3 * OCP + OC1P + c, fma1 ? (float)(k * (double)sc) : (float)k * 1.4901161193847656e-08f);
        put_f((size_t)3 * OCP + 2 * OC1P + c, sc * 67108864.0f);
      }
      h->dgeom.m1 = fma1 ? 3 : 2;
    }
  }
#ifdef DK_DEBUG
  h->dgeom.wei_bytes = (long long)n0; h->dgeom.wei1_bytes = (long long)n1; h->dgeom.cst_bytes = (long long)cst.size() * 4;
#endif
  if (!h->d_wei) HIP_TRY(hipMalloc(&h->d_wei, pk.size() + cst.size() * 4));
  char *base = (char *)h->d_wei;
  HIP_TRY(hipMemcpy(base, pk.data(), pk.size(), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(base + pk.size(), cst.data(), cst.size() * 4, hipMemcpyHostToDevice));
  h->args.wei = (const int8_t *)base;
  h->args.wei1 = (const int8_t *)(base + n0);
  h->args.consts = (const float *)(base + pk.size());
  h->weights_set = true;
  if (tune("DFX_DEBUG_PTRS")) fprintf(stderr, "[dfx] direct weights %p..%p (W0 %zu, W1 %zu, consts %zu bytes)\n", (void *)base, (void *)(base + pk.size() + cst.size() * 4), n0, n1, cst.size() * 4);
  return DFX_OK;
}

int dfx_conv_set_weights(dfx_conv_t *h, const int8_t *wei, const void *bia0, const float *scales0,
                         const int8_t *wei1, const void *bia1, const float *scales1) {
  if (!h || !wei || !scales0) return fail(DFX_ERR_INVALID, "set_weights: null argument");
  DeviceGuard dg(h->device);
  const dfx_conv_desc &d = h->d;
  const bool fused = d.oc1x1 > 0;
  if (fused && (!wei1 || !scales1)) return fail(DFX_ERR_INVALID, "set_weights: fused op needs wei1x1 and scales1");
  if ((d.bia0_dt != DFX_UNDEF && !bia0) || (fused && d.bia1_dt != DFX_UNDEF && !bia1))
    return fail(DFX_ERR_INVALID, "set_weights: bias dtype set but pointer is null");

  const int OC = d.oc, OC1 = d.oc1x1, IC = d.ic;
  const size_t nw0 = (size_t)OC * IC * d.kh * d.kw, nw1 = (size_t)OC1 * OC;
  std::vector<int8_t> p0(nw0), p1(nw1 ? nw1 : 1);
  std::vector<float> cst((size_t)3 * (OC + OC1), 0.0f);
  float *comp0 = cst.data();  // f32: exact, |comp| < 2^24 for K <= 1023
  float *b0 = cst.data() + OC, *s0 = cst.data() + 2 * OC;
  float *comp1 = cst.data() + 3 * OC;
  float *b1 = cst.data() + 3 * OC + OC1, *s1 = cst.data() + 3 * OC + 2 * OC1;
  for (int c = 0; c < OC; ++c) {
    b0[c] = d.bia0_dt == DFX_UNDEF ? 0.0f : bias_to_f32(bia0, d.bia0_dt, c);
    s0[c] = scales0[d.conv0_nscales > 1 ? c : 0];  // count 1 = broadcast (intended semantics)
  }
  for (int c = 0; c < OC1; ++c) {
    b1[c] = d.bia1_dt == DFX_UNDEF ? 0.0f : bias_to_f32(bia1, d.bia1_dt, c);
    s1[c] = scales1[d.conv1_nscales > 1 ? c : 0];
  }

  if (h->variant == DFX_VARIANT_MFMA_STREAM) return set_weights_stream(h, wei, bia0, scales0, wei1, bia1, scales1);

  if (h->variant != DFX_VARIANT_GENERIC) {
    const int ICB = h->icb, OCB = h->ocb, G = h->G, NCB = OC1 / 32;
    // W0 fragments [r][tap][c][lane][16]: lane (rho = lane&31, hh = lane>>5), byte j
    //   = W0[oc = 32r + rho][ic = 32c + 16hh + j][tap]
    for (int r = 0; r < OCB; ++r)
      for (int tap = 0; tap < 9; ++tap)
        for (int c = 0; c < ICB; ++c)
          for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < 16; ++j) {
              // fused: A operand, row = oc 32r + rho.  unfused: B operand with the channel
              // permutation of the store stage (G == OCB): column lam of block r = oc G*lam + r
              const int oc = fused ? 32 * r + (lane & 31) : G * (lane & 31) + r;
              const int ic = 32 * c + 16 * (lane >> 5) + j;
              p0[((((size_t)r * 9 + tap) * ICB + c) * 64 + lane) * 16 + j] =
                  wei[dfx_blocked_offset(oc, ic, tap / 3, tap % 3, IC, 3, 3)];
            }
    // W1 fragments [cb][r][lane][16]: cb = cg*G + cc; lane (lam, hh); byte j = 4q + i
    //   = W1[oc1 = 32G*cg + G*lam + cc][oc = 32r + 8q + 4hh + i]
    for (int cb = 0; cb < NCB; ++cb)
      for (int r = 0; r < OCB; ++r)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 16; ++j) {
            const int cg = cb / G, cc = cb % G, lam = lane & 31, hh = lane >> 5;
            const int oc1 = 32 * G * cg + G * lam + cc;
            const int oc = 32 * r + 8 * (j >> 2) + 4 * hh + (j & 3);
            p1[(((size_t)cb * OCB + r) * 64 + lane) * 16 + j] =
                wei1[dfx_blocked_offset(oc1, oc, 0, 0, OC, 1, 1)];
          }
    // ---- constants and requant mode per stage (conv_mfma.cuh header; emit_group) ----
    // Per channel, from the ACTUAL weights: P = sum of positive weights, N = -sum of negative
    // ones.  With activations stored as u8 - 128 in [-128, 127] the raw MFMA accumulator lies in
    // [-(128 P + 127 N), 127 P + 128 N]; comp = 128 * (P - N) turns it into the reference's s32
    // accumulator, |true acc| <= 255 * max(P, N).
    struct Ch { double P, N; };
    std::vector<Ch> c0(OC), c1(OC1 ? OC1 : 1);
    for (int oc = 0; oc < OC; ++oc) {
      double P = 0, N = 0;
      for (int ic = 0; ic < IC; ++ic)
        for (int tap = 0; tap < 9; ++tap) {
          const int w = wei[dfx_blocked_offset(oc, ic, tap / 3, tap % 3, IC, 3, 3)];
          (w > 0 ? P : N) += std::abs(w);
        }
      c0[oc] = {P, N};
    }
    for (int o1 = 0; o1 < OC1; ++o1) {
      double P = 0, N = 0;
      for (int oc = 0; oc < OC; ++oc) {
        const int w = wei1[dfx_blocked_offset(o1, oc, 0, 0, OC, 1, 1)];
        (w > 0 ? P : N) += std::abs(w);
      }
      c1[o1] = {P, N};
    }
    // "fast": rounding to nearest-even (the caller checks the round mode), every value finite and
    // |f| < 2^31 so the x86 overflow / NaN results of vcvtps2dq cannot occur
    auto fast_ok = [](const Ch &c, float bias, float scale) {
      if (!std::isfinite(bias) || !std::isfinite(scale)) return false;
      const double amax = 255.0 * std::max(c.P, c.N);
      return (amax + std::fabs((double)bias)) * std::fabs((double)scale) * 1.0001 + 2.0 < 2147480000.0;
    };
    // "magic", accumulator started from bits(1.5 * 2^23) + comp + bias (stage 0 of a fused op):
    // bias integer-valued and raw + comp + bias inside the binade, i.e. |.| < 2^22
    auto magic0_ok = [](const Ch &c, float bias) {
      const double b = bias, cb = 128.0 * (c.P - c.N) + b;
      if (b != std::floor(b)) return false;
      return -(128.0 * c.P + 127.0 * c.N) + cb > -4194304.0 && 127.0 * c.P + 128.0 * c.N + cb < 4194304.0;
    };
    // "magic", accumulator started from the inline constant 1/(2 pi) = 0x3E22F983 (ulp 2^-26):
    // raw within the mantissa's room; k = (comp + bias - 2^23 - 0x22F983) exactly representable;
    // |acc + bias| < 2^24; scale * 2^26 finite
    auto magic1_ok = [](const Ch &c, float bias, float scale) {
      const double b = bias, cb = 128.0 * (c.P - c.N) + b;
      if (b != std::floor(b)) return false;
      const double lo = -(128.0 * c.P + 127.0 * c.N), hi = 127.0 * c.P + 128.0 * c.N;
      if (lo < (double)MAGIC1_LO || hi > (double)MAGIC1_HI) return false;
      if (std::fabs(cb - 8388608.0 - (double)0x22F983) >= 16777216.0) return false;
      if (std::fabs(lo + cb) >= 16777216.0 || std::fabs(hi + cb) >= 16777216.0) return false;
      return std::isfinite(scale * 67108864.0f);
    };
    const bool no_fast = tune("DFX_NO_FAST") && atoi(tune("DFX_NO_FAST")) != 0;     // testing aid: exact paths
    const bool no_magic = tune("DFX_NO_MAGIC") && atoi(tune("DFX_NO_MAGIC")) != 0;  // testing aid: no magic paths
    int mode0 = (d.conv0_round_mode == DFX_ROUND_NEAREST && !no_fast) ? 2 : 0;
    for (int oc = 0; oc < OC && mode0; ++oc) {
      if (!fast_ok(c0[oc], b0[oc], s0[oc])) mode0 = 0;
      else if (mode0 == 2 && !(fused ? magic0_ok(c0[oc], b0[oc]) : magic1_ok(c0[oc], b0[oc], s0[oc]))) mode0 = 1;
    }
    int mode1 = (fused && d.conv1_round_mode == DFX_ROUND_NEAREST && !no_fast) ? 2 : 0;
    for (int o1 = 0; o1 < OC1 && mode1; ++o1) {
      if (!fast_ok(c1[o1], b1[o1], s1[o1])) mode1 = 0;
      else if (mode1 == 2 && !magic1_ok(c1[o1], b1[o1], s1[o1])) mode1 = 1;
    }
    if (no_magic) { mode0 = std::min(mode0, 1); mode1 = std::min(mode1, 1); }
    // "fma" (stage 0 of the role-specialised kernel, conv_mfma_roles.cuh): accumulator started from
    // bits(2^23) + comp + bias.  t = acc + bias must stay inside (-2^23, 2^23): non-negative t then reads as the
    // float 2^23 + t, negative t as 2^23 - |t|/2; fma(x, s, -2^23 s) = t * s with one rounding (2^23 s is exact)
    // or something negative that the stage's ReLU + u8 saturation turn into 0 like the reference's negative
    // product -- which needs s >= 0.  bias integer-valued; |acc| <= 2^24 follows (0 is a possible acc).
    auto fma0_ok = [](const Ch &c, float bias, float scale) {
      const double b = bias, cb = 128.0 * (c.P - c.N) + b;
      if (b != std::floor(b) || !(scale >= 0.0f) || !std::isfinite(scale * 8388608.0f)) return false;
      return -(128.0 * c.P + 127.0 * c.N) + cb > -8388608.0 && 127.0 * c.P + 128.0 * c.N + cb < 8388608.0;
    };
    bool roles = h->roles_ok && fused && mode1 == 2 && d.conv0_round_mode == DFX_ROUND_NEAREST && !no_fast && !no_magic;
    for (int oc = 0; oc < OC && roles; ++oc)
      if (!fast_ok(c0[oc], b0[oc], s0[oc]) || !fma0_ok(c0[oc], b0[oc], s0[oc])) roles = false;
    if (roles) mode0 = 3;
    h->roles = roles;
    // "fma" for stage 1 (role-specialised kernel only): (x + B) * C = fma(x, C, B * C) with one rounding when
    // the addend B * C = (comp + bias - 2^23 - 0x22F983) * scale is exactly representable -- power-of-two scales
    // and a few others; checked per channel in double (a 24-bit integer times a 24-bit mantissa is exact there)
    if (roles) {
      bool fma1 = true;
      for (int o1 = 0; o1 < OC1 && fma1; ++o1) {
        const double k = 128.0 * (c1[o1].P - c1[o1].N) + (double)b1[o1] - 8388608.0 - (double)0x22F983;
        const double prod = k * (double)s1[o1];
        fma1 = std::isfinite(prod) && (double)(float)prod == prod;
      }
      if (fma1) mode1 = 3;
    }
    if (h->variant == DFX_VARIANT_MFMA_FUSED) {
      // (the suffix names stage 1's requant route: "fma" = one v_fma_f32 per value, admitted where the addend is exactly
      //  representable -- power-of-two scales and a few others; "magic" = v_add_f32 + v_mul_f32)
      if (roles) snprintf(h->kernel_name, sizeof(h->kernel_name), "conv_mfma_roles_kernel<%d,%d,%d,%d>/%s", ICB, OCB, NCB, d.dst_dt,
                          mode1 == 3 ? "fma" : "magic");
      else snprintf(h->kernel_name, sizeof(h->kernel_name), "conv_mfma_fused_kernel<%d,%d,%d,%d>", ICB, OCB, G, d.dst_dt);
      h->block = roles ? RL_THREADS : MFMA_THREADS;
    }
    // slot A is an integer (bit copy into the f32 array), B and C are floats
    auto put_i = [](float *dst, int32_t v) { memcpy(dst, &v, 4); };
    auto inline_stage = [&](int mode, const Ch &c, float bias, float scale, float *A, float *B, float *C) {
      const int32_t comp = (int32_t)(128.0 * (c.P - c.N));
      put_i(A, comp - MAGIC1_BITS);  // acc bits + A = the reference's s32 accumulator
      if (mode == 3) {  // fma(x, C, B): B = (comp + bias - 2^23 - 0x22F983) * scale (proven exact), C = scale * 2^26
        *B = (float)(((double)comp + (double)bias - 8388608.0 - (double)0x22F983) * (double)scale);
        *C = scale * 67108864.0f;
      } else if (mode == 2) {
        *B = (float)((double)comp + (double)bias - 8388608.0 - (double)0x22F983) * 1.4901161193847656e-08f;  // * 2^-26, exact
        *C = scale * 67108864.0f;                                                                           // * 2^26, exact
      } else {
        *B = bias;
        *C = scale;
      }
    };
    for (int oc = 0; oc < OC; ++oc) {
      if (fused) {
        const int32_t comp = (int32_t)(128.0 * (c0[oc].P - c0[oc].N));
        put_i(comp0 + oc, mode0 == 3 ? MAGIC3_BITS + comp + (int32_t)b0[oc]
                        : mode0 == 2 ? MAGIC0_BITS + comp + (int32_t)b0[oc] : comp);  // accumulator start value
        if (mode0 == 3) b0[oc] = -8388608.0f * s0[oc];  // the fma's addend -2^23 * scale (exact)
      } else {
        float A, B, C;
        inline_stage(mode0, c0[oc], b0[oc], s0[oc], &A, &B, &C);
        comp0[oc] = A; b0[oc] = B; s0[oc] = C;
      }
    }
    for (int o1 = 0; o1 < OC1; ++o1) {
      float A, B, C;
      inline_stage(mode1, c1[o1], b1[o1], s1[o1], &A, &B, &C);
      comp1[o1] = A; b1[o1] = B; s1[o1] = C;
    }
    h->geom.mode0 = mode0;
    h->geom.mode1 = mode1;
    h->geom.s0_uniform = (fused && d.conv0_nscales == 1) ? 1 : 0;
    h->geom.s0_value = scales0[0];
  } else {
    memcpy(p0.data(), wei, nw0);
    if (fused) memcpy(p1.data(), wei1, nw1);
  }

  if (h->variant != DFX_VARIANT_GENERIC) {
    // constants in the kernel's layout: the storing stage's B and C as pairs {k, k} (conv_mfma.cuh,
    // mfma_cst_floats)
    {
      std::vector<float> lay((size_t)mfma_cst_floats(OC, OC1), 0.0f);
      if (fused) {
        memcpy(lay.data(), cst.data(), (size_t)(3 * OC + OC1) * 4);  // A0 B0 C0 A1
        for (int c = 0; c < OC1; ++c) {
          lay[(size_t)3 * OC + OC1 + 2 * c] = lay[(size_t)3 * OC + OC1 + 2 * c + 1] = b1[c];
          lay[(size_t)3 * OC + 3 * OC1 + 2 * c] = lay[(size_t)3 * OC + 3 * OC1 + 2 * c + 1] = s1[c];
        }
      } else {
        memcpy(lay.data(), cst.data(), (size_t)OC * 4);  // A0
        for (int c = 0; c < OC; ++c) {
          lay[(size_t)OC + 2 * c] = lay[(size_t)OC + 2 * c + 1] = b0[c];
          lay[(size_t)3 * OC + 2 * c] = lay[(size_t)3 * OC + 2 * c + 1] = s0[c];
        }
      }
      cst.swap(lay);
    }
    // one buffer in LDS-image order: [W0 fragments | W1 fragments | constants]
    const size_t cbytes = round16(cst.size() * 4);
    if (!h->d_wei) HIP_TRY(hipMalloc(&h->d_wei, nw0 + nw1 + cbytes));
    char *base = (char *)h->d_wei;
    HIP_TRY(hipMemcpy(base, p0.data(), nw0, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(base + nw0, p1.data(), nw1, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(base + nw0 + nw1, cst.data(), cst.size() * 4, hipMemcpyHostToDevice));
    h->args.wei = (const int8_t *)base;
    h->args.wei1 = (const int8_t *)(base + nw0);
    h->args.consts = (const float *)(base + nw0 + nw1);
  } else {
    if (!h->d_wei) {
      HIP_TRY(hipMalloc(&h->d_wei, nw0));
      HIP_TRY(hipMalloc(&h->d_wei1, nw1 ? nw1 : 16));
      HIP_TRY(hipMalloc(&h->d_consts, cst.size() * 4));
    }
    HIP_TRY(hipMemcpy(h->d_wei, p0.data(), nw0, hipMemcpyHostToDevice));
    if (nw1) HIP_TRY(hipMemcpy(h->d_wei1, p1.data(), nw1, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->d_consts, cst.data(), cst.size() * 4, hipMemcpyHostToDevice));
    h->args.wei = (const int8_t *)h->d_wei;
    h->args.wei1 = (const int8_t *)h->d_wei1;
    h->args.consts = (const float *)h->d_consts;
  }
  h->weights_set = true;
  return DFX_OK;
}

int dfx_conv_submit(dfx_conv_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s) {
  if (!h || !src_dev || !dst_dev) return fail(DFX_ERR_INVALID, "conv_submit: null argument");
  if (!h->weights_set) return fail(DFX_ERR_STATE, "conv_submit: dfx_conv_set_weights not called");
  DeviceGuard dg(h->device);
  // per-launch copies: concurrent submits of one handle (other host threads, other streams) share
  // only immutable state and each takes its own unit-queue slot of the ring
  ConvArgs a = h->args;
  a.src = (const uint8_t *)src_dev;
  a.dst = dst_dev;
  MfmaGeom g = h->geom;
  if (g.queue) {
    // one queue-ring slot per launch in flight; see struct dfx_conv for the guard
    const hipStream_t st = (hipStream_t)s;
    std::lock_guard<std::mutex> lk(*h->ring_mu);
    const unsigned slot = h->launch_seq++ % DFX_QUEUE_RING;
    if (h->launch_seq == 1) {
      h->first_stream = st;
      h->first_serial = stream_serial(st);
    }
    if (!h->multi_stream && st != h->first_stream) {
      // second stream seen: the launches so far (all on first_stream, no events) are covered by ONE event
      // recorded there now -- a stream event stands for everything submitted before it.  This stream waits for
      // it here; the slots of those launches keep it, so that any OTHER stream that reuses one waits too.
      h->multi_stream = true;
      hipEvent_t e0 = nullptr;
      HIP_TRY(hipEventCreateWithFlags(&e0, hipEventDisableTiming));
      // (a first stream of dfx_stream_create's that dfx_stream_destroy has destroyed since must not be touched)
      const bool gone = h->first_serial != 0 && stream_serial(h->first_stream) != h->first_serial;
      hipError_t r = gone ? hipErrorContextIsDestroyed : hipEventRecord(e0, h->first_stream);
      if (r == hipSuccess) r = hipStreamWaitEvent(st, e0, 0);
      if (r == hipSuccess) {
        ++h->ring_waits;
        h->first_ev = e0;
        for (unsigned i = 0; i < DFX_QUEUE_RING; ++i)
          if (h->slot_state[i] == 1) {
            h->slot_state[i] = 2;
            h->slot_stream[i] = h->first_stream;
            h->slot_ev[i] = e0;
          }
      } else {  // first_stream already destroyed by the caller: nothing to record on, wait for the device instead
        (void)hipEventDestroy(e0);
        if (!gone) (void)hipGetLastError();
        HIP_TRY(hipDeviceSynchronize());
        for (unsigned i = 0; i < DFX_QUEUE_RING; ++i)
          if (h->slot_state[i] == 1) h->slot_state[i] = 0;  // their launches have finished
      }
    }
    if (h->slot_state[slot] == 2 && h->slot_stream[slot] != st) {
      HIP_TRY(hipStreamWaitEvent(st, h->slot_ev[slot], 0));
      ++h->ring_waits;
    }
    g.queue += 2 * slot;
    if (mfma_dispatch(h, a, g, st, 0) != 0) return fail(DFX_ERR_UNSUPPORTED, "conv_submit: no kernel instance for this op");
    HIP_TRY(hipGetLastError());
    h->slot_stream[slot] = st;
    h->slot_state[slot] = 1;
    if (h->multi_stream) {
      if (h->slot_ev[slot] == h->first_ev) h->slot_ev[slot] = nullptr;  // (borrowed: this launch needs its own)
      if (!h->slot_ev[slot]) HIP_TRY(hipEventCreateWithFlags(&h->slot_ev[slot], hipEventDisableTiming));
      HIP_TRY(hipEventRecord(h->slot_ev[slot], st));
      h->slot_state[slot] = 2;
    }
    return DFX_OK;
  }
  int rc;
  if (h->variant != DFX_VARIANT_GENERIC)
    rc = mfma_dispatch(h, a, g, (hipStream_t)s, 0);
  else
    rc = launch_conv_generic(a, (hipStream_t)s, nullptr, nullptr);
  if (rc != 0) return fail(DFX_ERR_UNSUPPORTED, "conv_submit: no kernel instance for this op");
  HIP_TRY(hipGetLastError());
  return DFX_OK;
}

static size_t conv_src_bytes(const dfx_conv_desc &d) { return (size_t)d.bs * d.ih * d.iw * d.ic; }
static size_t conv_dst_bytes(const dfx_conv_desc &d) {
  const size_t px = d.fuse_pool ? (size_t)(d.oh / 2) * (d.ow / 2) : (size_t)d.oh * d.ow;
  return (size_t)d.bs * px * (d.oc1x1 ? d.oc1x1 : d.oc) * dt_size(d.dst_dt);
}

int dfx_conv_submit_host(dfx_conv_t *h, const void *src_host, void *dst_host) {
  if (!h || !src_host || !dst_host) return fail(DFX_ERR_INVALID, "conv_submit_host: null argument");
  DeviceGuard dg(h->device);
  return h->host.run(src_host, conv_src_bytes(h->d), dst_host, conv_dst_bytes(h->d),
                     [h](const void *s, void *d, dfx_stream_t st) { return dfx_conv_submit(h, s, d, st); });
}

int dfx_conv_query(const dfx_conv_t *h, dfx_conv_info *info) {
  if (!h || !info) return fail(DFX_ERR_INVALID, "conv_query: null argument");
  const dfx_conv_desc &d = h->d;
  memset(info, 0, sizeof(*info));
  info->variant = h->variant;
  info->grid = h->grid; info->block = h->block; info->lds_bytes = h->lds;
  info->rows_per_unit = h->args.rows_per_unit;
  info->device = h->device;
  const uint64_t px = (uint64_t)d.bs * d.oh * d.ow;
  const uint64_t mac = px * ((uint64_t)d.oc * d.ic * d.kh * d.kw + (uint64_t)d.oc1x1 * d.oc);
  info->algorithmic_ops = 2 * mac;
  info->algorithmic_bytes = conv_src_bytes(d) + conv_dst_bytes(d) +
                            (uint64_t)d.oc * d.ic * d.kh * d.kw + (uint64_t)d.oc1x1 * d.oc;
  snprintf(info->kernel_name, sizeof(info->kernel_name), "%s", h->kernel_name);
  return DFX_OK;
}

// test hook: the unit hand-out of a resident-weight op as the host decided it (include/dfx.h lists the order)
int dfx_debug_conv_sched(const dfx_conv_t *h, int32_t *out, int n) {
  if (!h || !out || n < 0) return fail(DFX_ERR_INVALID, "conv_sched: null argument");
  if (!h->geom.queue) return fail(DFX_ERR_UNSUPPORTED, "conv_sched: this op has no unit queue (%s)", h->kernel_name);
  const MfmaGeom &g = h->geom;
  int waits;
  {
    std::lock_guard<std::mutex> lk(*h->ring_mu);
    waits = h->ring_waits;
  }
  const int32_t v[13] = {g.th, g.tw, g.linear, g.uy, g.ux, g.total_units, g.half_from, g.static_rounds, g.lazy_queue,
                         g.pool, h->grid * MFMA_TEAMS, (h->roles_ok && h->roles) ? 1 : 0, waits};
  for (int i = 0; i < n && i < 13; ++i) out[i] = v[i];
  return DFX_OK;
}

// test hook: pixels per pixel-run unit of a resident-weight op (MfmaGeom::upx), 0 = row / column units or another
// kernel family.  Launches nothing.
int dfx_debug_conv_unit_px(const dfx_conv_t *h) {
  if (!h) return fail(DFX_ERR_INVALID, "conv_unit_px: null argument");
  return h->geom.queue ? h->geom.upx : 0;
}

// test hook: the requant route dfx_conv_set_weights proved for each stage, in ONE numbering for every kernel family
// (include/dfx.h): 0 exact, 1 fast, 2 magic, 3 fma, -1 no such stage.  Launches nothing.
int dfx_debug_conv_requant(const dfx_conv_t *h, int32_t out[2]) {
  if (!h || !out) return fail(DFX_ERR_INVALID, "conv_requant: null argument");
  if (!h->weights_set) return fail(DFX_ERR_STATE, "conv_requant: dfx_conv_set_weights not called");
  const bool fused = h->d.oc1x1 > 0;
  if (h->variant == DFX_VARIANT_MFMA_STREAM && h->direct) {  // conv_direct.cuh, conv_pw.cuh (and catconv_pw.cuh through conv_pw_view)
    const DirectGeom &g = h->dgeom;
    out[0] = g.m0 ? 3 : g.fast ? 1 : 0;
    out[1] = !fused ? -1 : g.m1 ? g.m1 : g.fast ? 1 : 0;
  } else if (h->variant == DFX_VARIANT_MFMA_STREAM) {  // conv_stream.cuh: one switch for both stages
    out[0] = h->sgeom.fast ? 1 : 0;
    out[1] = fused ? out[0] : -1;
  } else if (h->variant != DFX_VARIANT_GENERIC) {  // conv_mfma.cuh, conv_mfma_roles.cuh
    out[0] = h->geom.mode0;
    out[1] = fused ? h->geom.mode1 : -1;
  } else {  // the scalar kernel follows the reference's arithmetic step by step
    out[0] = 0;
    out[1] = fused ? 0 : -1;
  }
  return DFX_OK;
}

#ifdef DK_DEBUG
// bounds-checking diagnostic build of conv_direct.cuh: 32 x {offset, size} of the first violation per tag (-1 = none)
int dfx_debug_read_bounds(dfx_conv_t *h, long long *out) {
  if (!h || !h->d_prof) return fail(DFX_ERR_STATE, "no debug buffer");
  HIP_TRY(hipMemcpy(out, h->d_prof, 64 * 8, hipMemcpyDeviceToHost));
  return DFX_OK;
}
#endif

#ifdef DFX_TRACE
// diagnostic build only (make trace): host pointer to the [grid][16 waves][4] progress words
int *dfx_debug_trace(dfx_conv_t *h) { return h ? h->trace_host : nullptr; }
#endif

#ifdef DFX_STAMPS
// diagnostic build only: copies the [grid][8 waves][8] stamp sums of the last launch
int dfx_debug_read_stamps(dfx_conv_t *h, unsigned long long *out, int max_entries) {
  if (!h || !h->d_prof) return fail(DFX_ERR_STATE, "no stamps");
  int n = h->grid * (h->variant == DFX_VARIANT_MFMA_STREAM ? (h->direct ? h->nw * 16 : 96) : 768);
  if (n > max_entries) n = max_entries;
  HIP_TRY(hipMemcpy(out, h->d_prof, (size_t)n * 8, hipMemcpyDeviceToHost));
  return n;
}
#endif

int dfx_conv_destroy(dfx_conv_t *h) {
  conv_release(h);
  return DFX_OK;
}

// test hook: set (value != NULL) or clear one of the testing / tuning switches of DESIGN.md
// section 9 after the environment has been read; affects handles created afterwards
int dfx_debug_set_tuning(const char *key, const char *value) {
  if (!key) return fail(DFX_ERR_INVALID, "set_tuning: null key");
  bool known = false;
  for (const char *k : kTuningKeys) known = known || strcmp(k, key) == 0;
  if (!known) return fail(DFX_ERR_INVALID, "set_tuning: unknown switch %s", key);
  Tuning &t = tuning();
  std::lock_guard<std::mutex> lk(t.mu);
  if (value) t.kv[key] = value;
  else t.kv.erase(key);
  return DFX_OK;
}

// ---------------------------------------------------------------------------
// concat
// ---------------------------------------------------------------------------

int dfx_concat_create(const dfx_concat_desc *desc, dfx_concat_t **out) {
  if (!desc || !out || !desc->channels) return fail(DFX_ERR_INVALID, "concat_create: null argument");
  *out = nullptr;
  const dfx_concat_desc &d = *desc;
  if (d.n_inputs <= 0 || d.bs <= 0 || d.h <= 0 || d.w <= 0)
    return fail(DFX_ERR_INVALID, "concat: non-positive dimension");
  if (d.dt < DFX_F32 || d.dt > DFX_U8) return fail(DFX_ERR_INVALID, "concat: bad dtype");
  if (d.n_inputs > CONCAT_MAX_INPUTS)
    return fail(DFX_ERR_UNSUPPORTED, "concat: more than %d inputs", CONCAT_MAX_INPUTS);
  const int blk = dt_size(d.dt) == 1 ? 16 : 4;  // jit_concat_kernel.cc:155-196
  for (int i = 0; i < d.n_inputs; ++i)
    if (d.channels[i] <= 0 || d.channels[i] % blk)
      return fail(DFX_ERR_INVALID, "concat: channels of input %d not a multiple of %d", i, blk);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(DFX_ERR_NO_DEVICE, "concat_create: no HIP device (this library has no CPU path)");
  dfx_concat *h = new (std::nothrow) dfx_concat();
  if (!h) return fail(DFX_ERR_HIP, "out of host memory");
  h->d = d;
  if (hipGetDevice(&h->device) != hipSuccess) h->device = 0;
  h->channels.assign(d.channels, d.channels + d.n_inputs);
  h->d.channels = h->channels.data();
  ConcatArgs &a = h->args;
  memset(&a, 0, sizeof(a));
  const int per_chunk = 16 / (int)dt_size(d.dt);
  int end = 0;
  for (int i = 0; i < d.n_inputs; ++i) {
    end += d.channels[i] / per_chunk;
    a.chunk_end[i] = end;
  }
  a.n_inputs = d.n_inputs;
  a.chunks_per_px = end;
  a.total_chunks = (long long)d.bs * d.h * d.w * end;
  a.dt = d.dt;
  a.relu = d.post_relu;
  *out = h;
  return DFX_OK;
}

int dfx_concat_submit(dfx_concat_t *h, const void *const *srcs_dev, void *dst_dev, dfx_stream_t s) {
  if (!h || !srcs_dev || !dst_dev) return fail(DFX_ERR_INVALID, "concat_submit: null argument");
  DeviceGuard dg(h->device);
  ConcatArgs a = h->args;  // per-launch copy: h->args is written at create only, so submits on several
                           // streams and from several host threads never see each other's pointers
  for (int i = 0; i < a.n_inputs; ++i) {
    if (!srcs_dev[i]) return fail(DFX_ERR_INVALID, "concat_submit: null input %d", i);
    if ((uintptr_t)srcs_dev[i] % 16) return fail(DFX_ERR_INVALID, "concat_submit: input %d not 16-byte aligned", i);
    a.src[i] = (const unsigned char *)srcs_dev[i];
  }
  if ((uintptr_t)dst_dev % 16) return fail(DFX_ERR_INVALID, "concat_submit: dst not 16-byte aligned");
  a.dst = (unsigned char *)dst_dev;
  launch_concat(a, (hipStream_t)s);
  HIP_TRY(hipGetLastError());
  return DFX_OK;
}

int dfx_concat_submit_gathered(dfx_concat_t *h, const void *gathered_dev, const uint64_t *offsets,
                               void *dst_dev, dfx_stream_t s) {
  if (!h || !gathered_dev || !offsets || !dst_dev)
    return fail(DFX_ERR_INVALID, "concat_submit_gathered: null argument");
  if ((uintptr_t)gathered_dev % 16)
    return fail(DFX_ERR_INVALID, "concat_submit_gathered: base not 16-byte aligned");
  const void *ptrs[CONCAT_MAX_INPUTS];
  for (int i = 0; i < h->d.n_inputs; ++i) {
    if (offsets[i] % 16) return fail(DFX_ERR_INVALID, "concat_submit_gathered: offset %d not 16-byte aligned", i);
    ptrs[i] = (const unsigned char *)gathered_dev + offsets[i];
  }
  return dfx_concat_submit(h, ptrs, dst_dev, s);
}

int dfx_concat_submit_host(dfx_concat_t *h, const void *const *srcs_host, void *dst_host) {
  if (!h || !srcs_host || !dst_host) return fail(DFX_ERR_INVALID, "concat_submit_host: null argument");
  DeviceGuard dg(h->device);
  const size_t px = (size_t)h->d.bs * h->d.h * h->d.w, es = dt_size(h->d.dt);
  size_t oc = 0;
  std::vector<size_t> sb;
  for (int c : h->channels) {
    oc += c;
    sb.push_back(px * c * es);
  }
  return h->host.run(h->d.n_inputs, srcs_host, sb.data(), dst_host, px * oc * es,
                     [h](const void *const *s, void *d, dfx_stream_t st) { return dfx_concat_submit(h, s, d, st); });
}

int dfx_concat_destroy(dfx_concat_t *h) {
  if (!h) return DFX_OK;
  DeviceGuard dg(h->device);
  h->host.release();
  delete h;
  return DFX_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// pooling stage of conv+relu+pool, eltwise-sum (+relu): the reference's roadmap ops
// (README.md:64-65; semantics of the MKL-DNN pipeline in test/test_conv_relu_pooling.cc:30-235)
// ---------------------------------------------------------------------------

struct dfx_pool {
  dfx_pool_desc d;
  int device;
  PoolArgs args;
};
struct dfx_eltwise {
  dfx_eltwise_desc d;
  int device;
  EltwiseArgs args;
};

int dfx_pool_create(const dfx_pool_desc *desc, dfx_pool_t **out) {
  if (!desc || !out) return fail(DFX_ERR_INVALID, "pool_create: null argument");
  *out = nullptr;
  const dfx_pool_desc &d = *desc;
  if (d.bs <= 0 || d.c <= 0 || d.ih <= 0 || d.iw <= 0 || d.oh <= 0 || d.ow <= 0 || d.kh <= 0 || d.kw <= 0 ||
      d.sh <= 0 || d.sw <= 0 || d.pad_t < 0 || d.pad_l < 0)
    return fail(DFX_ERR_INVALID, "pool: bad dimension");
  if (d.dt < DFX_F32 || d.dt > DFX_U8) return fail(DFX_ERR_INVALID, "pool: bad dtype");
  if (d.algo < DFX_POOL_MAX || d.algo > DFX_POOL_AVG_EXCLUDE_PADDING) return fail(DFX_ERR_INVALID, "pool: bad algorithm");
  // every output window must contain at least one input position (as MKL-DNN requires)
  if (d.pad_t >= d.kh || d.pad_l >= d.kw || (long long)(d.oh - 1) * d.sh - d.pad_t >= d.ih ||
      (long long)(d.ow - 1) * d.sw - d.pad_l >= d.iw)
    return fail(DFX_ERR_INVALID, "pool: an output window lies entirely in the padding");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(DFX_ERR_NO_DEVICE, "pool_create: no HIP device (this library has no CPU path)");
  dfx_pool *h = new (std::nothrow) dfx_pool();
  if (!h) return fail(DFX_ERR_HIP, "out of host memory");
  h->d = d;
  if (hipGetDevice(&h->device) != hipSuccess) h->device = 0;
  PoolArgs &a = h->args;
  memset(&a, 0, sizeof(a));
  a.bs = d.bs; a.c = d.c; a.ih = d.ih; a.iw = d.iw; a.oh = d.oh; a.ow = d.ow;
  a.kh = d.kh; a.kw = d.kw; a.sh = d.sh; a.sw = d.sw; a.pad_t = d.pad_t; a.pad_l = d.pad_l; a.dt = d.dt;
  a.algo = d.algo;
  const size_t es = dt_size(d.dt);
  a.vec = ((size_t)d.c * es) % 16 == 0;
  a.groups = a.vec ? (int)((size_t)d.c * es / 16) : d.c;
  a.total = (long long)d.bs * d.oh * d.ow * a.groups;
  *out = h;
  return DFX_OK;
}

int dfx_pool_submit(dfx_pool_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s) {
  if (!h || !src_dev || !dst_dev) return fail(DFX_ERR_INVALID, "pool_submit: null argument");
  DeviceGuard dg(h->device);
  PoolArgs a = h->args;  // per-launch copy: concurrent submits on several streams are independent
  a.src = (const unsigned char *)src_dev;
  a.dst = (unsigned char *)dst_dev;
  if (((uintptr_t)src_dev | (uintptr_t)dst_dev) % dt_size(a.dt))
    return fail(DFX_ERR_INVALID, "pool_submit: src or dst not aligned to the element size (%d bytes)",
                (int)dt_size(a.dt));
  if (a.vec && (((uintptr_t)src_dev | (uintptr_t)dst_dev) % 16)) {  // 16-byte vector path needs aligned buffers:
    a.vec = 0;                                                       // misaligned ones take the per-channel path
    a.groups = a.c;
    a.total = (long long)a.bs * a.oh * a.ow * a.groups;
  }
  if (launch_pool(a, (hipStream_t)s) != 0) return fail(DFX_ERR_INVALID, "pool_submit: bad dtype");
  HIP_TRY(hipGetLastError());
  return DFX_OK;
}

int dfx_pool_destroy(dfx_pool_t *h) {
  delete h;
  return DFX_OK;
}

int dfx_eltwise_create(const dfx_eltwise_desc *desc, dfx_eltwise_t **out) {
  if (!desc || !out) return fail(DFX_ERR_INVALID, "eltwise_create: null argument");
  *out = nullptr;
  const dfx_eltwise_desc &d = *desc;
  if (d.n_inputs < 2 || d.n_inputs > ELTWISE_MAX_INPUTS)
    return fail(DFX_ERR_UNSUPPORTED, "eltwise: 2..%d inputs", ELTWISE_MAX_INPUTS);
  if (d.elems <= 0) return fail(DFX_ERR_INVALID, "eltwise: non-positive size");
  if (d.dt < DFX_F32 || d.dt > DFX_U8) return fail(DFX_ERR_INVALID, "eltwise: bad dtype");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(DFX_ERR_NO_DEVICE, "eltwise_create: no HIP device (this library has no CPU path)");
  dfx_eltwise *h = new (std::nothrow) dfx_eltwise();
  if (!h) return fail(DFX_ERR_HIP, "out of host memory");
  h->d = d;
  if (hipGetDevice(&h->device) != hipSuccess) h->device = 0;
  memset(&h->args, 0, sizeof(h->args));
  h->args.n_inputs = d.n_inputs;
  h->args.dt = d.dt;
  h->args.relu = d.post_relu;
  h->args.elems = d.elems;
  *out = h;
  return DFX_OK;
}

int dfx_eltwise_submit(dfx_eltwise_t *h, const void *const *srcs_dev, void *dst_dev, dfx_stream_t s) {
  if (!h || !srcs_dev || !dst_dev) return fail(DFX_ERR_INVALID, "eltwise_submit: null argument");
  DeviceGuard dg(h->device);
  EltwiseArgs a = h->args;
  for (int i = 0; i < a.n_inputs; ++i) {
    if (!srcs_dev[i]) return fail(DFX_ERR_INVALID, "eltwise_submit: null input %d", i);
    if ((uintptr_t)srcs_dev[i] % 16) return fail(DFX_ERR_INVALID, "eltwise_submit: input %d not 16-byte aligned", i);
    a.src[i] = (const unsigned char *)srcs_dev[i];
  }
  if ((uintptr_t)dst_dev % 16) return fail(DFX_ERR_INVALID, "eltwise_submit: dst not 16-byte aligned");
  a.dst = (unsigned char *)dst_dev;
  if (launch_eltwise(a, (hipStream_t)s) != 0) return fail(DFX_ERR_INVALID, "eltwise_submit: bad dtype");
  HIP_TRY(hipGetLastError());
  return DFX_OK;
}

int dfx_eltwise_destroy(dfx_eltwise_t *h) {
  delete h;
  return DFX_OK;
}
