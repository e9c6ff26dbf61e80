// path_op.h -- what the host sides of the ops that plan a fast path and a generic one at create and fall back to the generic
// kernel per submit repeat word for word (resize, wsum, head, select, nms, roialign, bmm, attn, lnorm, linear, patchembed,
// window): the opening of create, the launch counters behind dfx_debug_X_launches, the DFX_X_GRID cap, the tail of a
// one-launch submit and the head of query.  Plain helpers, no skeleton: below this frame the ops differ (one to N inputs,
// one to four launches, tables, scales, a bias, TwoLaunchOrder), so each *_api.hip keeps its `struct dfx_X`, its extern "C"
// entry points and every line of its own, and calls these where it would repeat itself.  Not installed, not part of the
// C ABI.
//
// A handle is `struct dfx_X { dfx_X_desc d; int device; int path; char kernel_name[96]; ... }`, and its file has ONE
// `void release(dfx_X *h)`: under DeviceGuard(h->device) it gives back everything the handle can own, tolerating members
// that are still null (and a null h), and deletes it.  Every failure path of create and destroy go through it.
#pragma once

#include <algorithm>
#include <atomic>
#include <cstring>
#include <new>

#include "dfx_internal.h"
#include "requant_host.h"  // dt_name

#pragma GCC visibility push(hidden)
namespace dfx {

// The opening of dfx_X_create: null check, *out = nullptr, `refuse(desc)` (the op's validation and then its forced-path
// refusal; each has called fail() when it returns non-zero), the device count, the handle with `d` and `device` filled
// and, where the plan needs it, the device's CU count (`cus` with the op's `release`).  DFX_OK with *hp set, or the code
// with nothing left behind.
template <class H, class Desc, class Refuse>
int open_create(const char *op, const Desc *desc, H **out, H **hp, Refuse refuse, int *cus = nullptr, void (*release)(H *) = nullptr) {
  if (!desc || !out) return fail(DFX_ERR_INVALID, "%s_create: null argument", op);
  *out = nullptr;
  if (const int rc = refuse(*desc)) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(DFX_ERR_NO_DEVICE, "%s_create: no HIP device (this library has no CPU path)", op);
  H *h = new (std::nothrow) H();
  if (!h) return fail(DFX_ERR_HIP, "out of host memory");
  h->d = *desc;
  if (hipGetDevice(&h->device) != hipSuccess) h->device = 0;
  if (cus) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, h->device) != hipSuccess) {
      release(h);
      return fail(DFX_ERR_HIP, "%s_create: cannot query the device", op);
    }
    *cus = std::max(1, prop.multiProcessorCount);
  }
  *hp = h;
  return DFX_OK;
}

// what a plan header's X_validate(d, &why) becomes in create: its code, with "X: why" recorded
template <class Desc>
int validated(const char *op, int (*validate)(const Desc &, const char **), const Desc &d) {
  const char *why = "";
  const int rc = validate(d, &why);
  return rc ? fail(rc, "%s: %s", op, why) : DFX_OK;
}

// Launches (select, nms, attn: submits) since the library was loaded, by the path that ran: one static instance per op
// file, process-wide, because submit does not write to the handle.  Relaxed: a count, not a synchronisation.
template <int N>
struct LaunchCounts {
  std::atomic<long long> n[N];

  void hit(int path) { n[path].fetch_add(1, std::memory_order_relaxed); }

  // dfx_debug_X_launches: shows the per-submit fallback, which query cannot
  int read(const char *op, int64_t *out) const {
    if (!out) return fail(DFX_ERR_INVALID, "debug_%s_launches: null argument", op);
    for (int k = 0; k < N; ++k) out[k] = n[k].load(std::memory_order_relaxed);
    return DFX_OK;
  }

  // what a submit returns behind its one launch, `launch_rc` being what the op's launcher returned: counted once the
  // launch is known to be out
  int launched(const char *op, int launch_rc, int path) {
    if (launch_rc != 0) return fail(DFX_ERR_UNSUPPORTED, "%s_submit: no kernel instance for this op", op);
    HIP_TRY(hipGetLastError());
    hit(path);
    return DFX_OK;
  }
};

// testing aid: the cap DFX_X_GRID puts on a grid, 0 for none; read at every create
inline long long grid_cap(const char *key) {
  const char *e = tuning_value(key);
  return e ? std::max(1ll, atoll(e)) : 0;
}

// The head of dfx_X_query: null check, a zeroed info with path, device and kernel_name; the op fills in the rest.
template <class H, class Info>
int open_query(const char *op, const H *h, Info *info) {
  if (!h || !info) return fail(DFX_ERR_INVALID, "%s_query: null argument", op);
  memset(info, 0, sizeof(*info));
  info->path = h->path;
  info->device = h->device;
  memcpy(info->kernel_name, h->kernel_name, sizeof(info->kernel_name));
  return DFX_OK;
}

}  // namespace dfx
#pragma GCC visibility pop
