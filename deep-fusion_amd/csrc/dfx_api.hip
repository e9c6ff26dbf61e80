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
#pragma GCC visibility push(hidden)  // (the planner's and packer's inline functions are no part of the library's exported symbols)
#include "conv_plan.h"
#include "conv_weights.h"
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
                                   "DFX_STREAM_DIRECT", "DFX_STREAM_PW", "DFX_DIRECT_NPB", "DFX_DIRECT_NW", "DFX_DIRECT_WO1", "DFX_STREAM_GRID", "DFX_DEBUG_PTRS", "DFX_DWCONV_GRID", "DFX_DWCONV_BAND", "DFX_DWPW_GRID", "DFX_DWPW_TH", "DFX_GCONV_GRID", "DFX_GCONV_TILE", "DFX_FC_SPLITK", "DFX_FC_GRID", "DFX_IMGCONV_GRID", "DFX_DECONV_GRID", "DFX_DILCONV_GRID", "DFX_DILCONV_SLAB", "DFX_DILCONV_STRIPS", "DFX_RESIZE_ROWS", "DFX_RESIZE_MAX_GRID", "DFX_SE_SLICES", "DFX_SE_GRID", "DFX_WSUM_GRID", "DFX_HEAD_GRID", "DFX_SELECT_CHUNK", "DFX_BMM_GRID", "DFX_ATTN_GRID", "DFX_LNORM_GRID", "DFX_LINEAR_GRID", "DFX_LINEAR_BM", "DFX_PATCHEMBED_GRID", "DFX_PATCHEMBED_BM", "DFX_WINDOW_GRID",
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
  void *d_wei;  // ONE buffer [W0 | W1 | constants] (conv_weights.h), allocated by the first dfx_conv_set_weights
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
  return blocked_offset(o, i, kh, kw, I, KH, KW);  // (conv_weights.h)
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
  if (h->pw) {  // pointwise unfused conv (conv_pw.cuh); the requant proofs live in dgeom (conv_weights.h, pack_streamed)
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
  (void)hipFree(h->d_wei);
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

// Weight images and requant-route proofs are conv_weights.h's (no HIP in there); here: the argument checks and the upload
// of the ONE buffer [W0 | W1 | constants] a handle owns.
int dfx_conv_set_weights(dfx_conv_t *h, const int8_t *wei, const void *bia0, const float *scales0,
                         const int8_t *wei1, const void *bia1, const float *scales1) {
  if (!h || !wei || !scales0) return fail(DFX_ERR_INVALID, "set_weights: null argument");
  DeviceGuard dg(h->device);
  const dfx_conv_desc &d = h->d;
  const bool fused = d.oc1x1 > 0;
  if (fused && (!wei1 || !scales1)) return fail(DFX_ERR_INVALID, "set_weights: fused op needs wei1x1 and scales1");
  if ((d.bia0_dt != DFX_UNDEF && !bia0) || (fused && d.bia1_dt != DFX_UNDEF && !bia1))
    return fail(DFX_ERR_INVALID, "set_weights: bias dtype set but pointer is null");

  ConvWeights w;
  const char *why = "";
  const int rc = conv_pack_weights(d, *h, tune, wei, bia0, scales0, wei1, bia1, scales1, &w, &why);
  if (rc) return fail(rc, "%s", why);

  if (!h->d_wei) HIP_TRY(hipMalloc(&h->d_wei, w.image.size()));  // (the size depends on the plan alone: once per handle)
  char *base = (char *)h->d_wei;
  HIP_TRY(hipMemcpy(base, w.image.data(), w.image.size(), hipMemcpyHostToDevice));
  h->args.wei = (const int8_t *)base;
  h->args.wei1 = (const int8_t *)(base + w.off_w1);
  h->args.consts = (const float *)(base + w.off_cst);
  if (h->variant == DFX_VARIANT_MFMA_STREAM && h->direct) {  // conv_direct.cuh, conv_pw.cuh
    h->dgeom.fast = w.fast;
    h->dgeom.m0 = w.m0;
    h->dgeom.m1 = w.m1;
#ifdef DK_DEBUG
    h->dgeom.wei_bytes = (long long)w.n_w0; h->dgeom.wei1_bytes = (long long)w.n_w1; h->dgeom.cst_bytes = (long long)w.n_cst;
#endif
  } else if (h->variant == DFX_VARIANT_MFMA_STREAM) {  // conv_stream.cuh
    h->sgeom.fast = w.fast;
  } else if (h->variant != DFX_VARIANT_GENERIC) {  // conv_mfma.cuh, conv_mfma_roles.cuh
    h->geom.mode0 = w.mode0;
    h->geom.mode1 = w.mode1;
    h->geom.s0_uniform = w.s0_uniform;
    h->geom.s0_value = w.s0_value;
  }
  // (only the fused resident variant's roles decision changes these three; everywhere else they are the plan's again)
  h->roles = w.roles;
  snprintf(h->kernel_name, sizeof(h->kernel_name), "%s", w.kernel_name);
  h->block = w.block;
  h->weights_set = true;
  if (h->direct && tune("DFX_DEBUG_PTRS")) fprintf(stderr, "[dfx] direct weights %p..%p (W0 %zu, W1 %zu, consts %zu bytes)\n", (void *)base, (void *)(base + w.image.size()), w.n_w0, w.n_w1, w.n_cst);
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
