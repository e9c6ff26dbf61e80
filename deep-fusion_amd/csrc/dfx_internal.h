// dfx_internal.h -- the few host-side helpers the translation units behind include/dfx.h share
// (dfx_api.hip, reorder_api.hip, catconv_api.hip, dwconv_api.hip, gconv_api.hip).  Not installed, not part of the C ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/dfx.h"

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

}  // namespace dfx

#define HIP_TRY(expr)                                                                        \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      return dfx::fail(e_ == hipErrorNoDevice ? DFX_ERR_NO_DEVICE : DFX_ERR_HIP, "%s: %s",   \
                       #expr, hipGetErrorString(e_));                                        \
  } while (0)
