// dfx_internal.h -- the few host-side helpers the translation units behind include/dfx.h share
// (dfx_api.hip, reorder_api.hip).  Not installed, not part of the C ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/dfx.h"

namespace dfx {

// records the thread's dfx_last_error() message and returns `code` (defined in dfx_api.hip)
__attribute__((visibility("hidden"))) int fail(int code, const char *fmt, ...);

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
