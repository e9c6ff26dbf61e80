// dfx_internal.h -- the few host-side helpers the translation units behind include/dfx.h share (every *_api.hip includes
// it, directly or through weighted_op.h or path_op.h).  Not installed, not part of the C ABI.  What needs no HIP is in
// requant_host.h and plan_common.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdlib.h>

#include <mutex>
#include <vector>

#include "../../include/dfx.h"

#define HIP_TRY(expr)                                                                        \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      return dfx::fail(e_ == hipErrorNoDevice ? DFX_ERR_NO_DEVICE : DFX_ERR_HIP, "%s: %s",   \
                       #expr, hipGetErrorString(e_));                                        \
  } while (0)

namespace dfx {

// records the thread's dfx_last_error() message and returns `code` (defined in dfx_api.hip)
__attribute__((visibility("hidden"))) int fail(int code, const char *fmt, ...);

// The pointwise kernel's view of a conv handle (defined in dfx_api.hip): its kernel arguments without src / dst (packed
// weight image, constants, flags), its geometry with the requant-route proofs of the last dfx_conv_set_weights (fast,
// m0) and its LDS size.  false when the handle is not served by conv_pw.cuh.  catconv_api.hip launches its own kernel
// on these, so that neither the packing nor the proofs exist twice.
struct ConvArgs;
struct PwGeom;
__attribute__((visibility("hidden"))) bool conv_pw_view(const dfx_conv *h, ConvArgs *args, PwGeom *geom, int *lds);

// The window kernel's view of a depthwise handle (defined in dwconv_api.hip): its kernel arguments without src / dst
// (packed weights, compensation, bias, scale) with the requant-route proof of the last dfx_dwconv_set_weights (fast).
// false when the handle is not on the window path or has no weights yet.  dwpw_api.hip launches its fused kernel on
// these, so that neither the packing nor the proof exist twice.
struct DwArgs;
__attribute__((visibility("hidden"))) bool dwconv_window_view(const dfx_dwconv *h, DwArgs *args);

// serial number of a live stream of dfx_stream_create's (never reused), 0 for any other stream: how a handle that
// remembers a stream finds out that dfx_stream_destroy has destroyed it since (defined in dfx_api.hip)
__attribute__((visibility("hidden"))) unsigned long long stream_serial_of(hipStream_t st);

// value of a testing / tuning switch or nullptr; use it at once (defined in dfx_api.hip)
__attribute__((visibility("hidden"))) const char *tuning_value(const char *key);

inline size_t dt_size(int dt) { return (dt == DFX_F32 || dt == DFX_S32) ? 4 : 1; }

// every entry point that takes a handle runs on the device the handle was created on
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (dev >= 0 && dev != prev) (void)hipSetDevice(dev);
    else prev = -1;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// testing aid: DFX_NO_FAST set to a non-zero value forces the exact requant route of whatever set_weights proves next
inline bool fast_allowed() {
  const char *e = tuning_value("DFX_NO_FAST");
  return !e || atoi(e) == 0;
}

// Order of the submits of a two-launch op (catconv_api.hip, dwpw_api.hip, fc_api.hip), whose two kernels meet in ONE buffer the
// handle owns, so that its submits are SERIALISED on the device.  Submits on ONE stream are ordered by the stream and
// cost nothing extra (an event record behind every submit measured + 3 us per submit).  When a second stream appears,
// one event recorded on the first stream stands for everything submitted so far; from then on every submit records `ev`
// behind its second launch and a submit on another stream than the previous one's first waits for it.
struct TwoLaunchOrder {
  std::mutex mu;  // held from enter() to the end of the submit: guards the buffer's hand-over and the fields below
  hipEvent_t ev = nullptr;
  hipStream_t first_stream = nullptr, last_stream = nullptr;
  unsigned long long first_serial = 0;  // stream_serial_of(first_stream) at the first submit
  bool have_last = false, multi_stream = false;

  hipError_t create() { return hipEventCreateWithFlags(&ev, hipEventDisableTiming); }
  void destroy() {
    if (ev) (void)hipEventDestroy(ev);
  }
  // before the first launch, with mu held
  int enter(hipStream_t st) {
    if (!have_last) {
      first_stream = st;
      first_serial = stream_serial_of(st);
    } else if (!multi_stream && st != first_stream) {
      multi_stream = true;
      // (a first stream of dfx_stream_create's that dfx_stream_destroy has destroyed since must not be touched)
      const bool gone = first_serial != 0 && stream_serial_of(first_stream) != first_serial;
      hipError_t r = gone ? hipErrorContextIsDestroyed : hipEventRecord(ev, first_stream);
      if (r == hipSuccess) r = hipStreamWaitEvent(st, ev, 0);
      if (r != hipSuccess) {  // nothing to record on: wait for the device instead
        if (!gone) (void)hipGetLastError();
        HIP_TRY(hipDeviceSynchronize());
      }
    } else if (multi_stream && st != last_stream) {
      HIP_TRY(hipStreamWaitEvent(st, ev, 0));
    }
    return DFX_OK;
  }
  // behind the second launch, with mu held
  int leave(hipStream_t st) {
    if (multi_stream) HIP_TRY(hipEventRecord(ev, st));
    last_stream = st;
    have_last = true;
    return DFX_OK;
  }
};

// What every dfx_*_submit_host works through: device copies of the op's sources and of its destination and a
// non-blocking stream, made at the first call and kept until the handle goes.  Calls on one handle take turns (mu).
struct HostStaging {
  std::mutex mu;
  std::vector<void *> d_src;
  void *d_dst = nullptr;
  hipStream_t stream = nullptr;

  // Each piece on its own: a call that failed half way leaves nothing the next one would take for complete.
  int ensure(int n, const size_t *src_bytes, size_t dst_bytes) {
    d_src.resize((size_t)n, nullptr);
    for (int i = 0; i < n; ++i)
      if (!d_src[i]) HIP_TRY(hipMalloc(&d_src[i], src_bytes[i]));
    if (!d_dst) HIP_TRY(hipMalloc(&d_dst, dst_bytes));
    if (!stream) HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    return DFX_OK;
  }
  void release() {
    for (void *p : d_src) (void)hipFree(p);
    (void)hipFree(d_dst);
    if (stream) (void)hipStreamDestroy(stream);
  }
  // the n sources to the device, submit(device sources, device destination, stream), the destination back, all on the
  // staging stream, which is drained before the call returns
  template <class Submit>
  int run(int n, const void *const *srcs_host, const size_t *src_bytes, void *dst_host, size_t dst_bytes, Submit submit) {
    std::lock_guard<std::mutex> lk(mu);
    int rc = ensure(n, src_bytes, dst_bytes);
    if (rc) return rc;
    for (int i = 0; i < n; ++i) HIP_TRY(hipMemcpyAsync(d_src[i], srcs_host[i], src_bytes[i], hipMemcpyHostToDevice, stream));
    rc = submit((const void *const *)d_src.data(), d_dst, (dfx_stream_t)stream);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(dst_host, d_dst, dst_bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return DFX_OK;
  }
  // (one source)
  template <class Submit>
  int run(const void *src_host, size_t src_bytes, void *dst_host, size_t dst_bytes, Submit submit) {
    return run(1, &src_host, &src_bytes, dst_host, dst_bytes,
               [&](const void *const *s, void *d, dfx_stream_t st) { return submit(s[0], d, st); });
  }
};

}  // namespace dfx
