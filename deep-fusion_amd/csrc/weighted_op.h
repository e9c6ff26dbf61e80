// weighted_op.h -- the host-side skeleton of the ops that own ONE set of weights and choose between a fast kernel for a
// shape class and a generic kernel for everything else (dwconv, gconv, imgconv, deconv, dilconv, fc): the handle, and
// what create / set_weights / submit / submit_host / query / the requant hook / destroy do the same way for all of
// them.  Not installed, not part of the C ABI: the extern "C" entry points stay in the op's *_api.hip and forward here.
//
// An op supplies a traits struct `Op` (in its file's unnamed namespace; everything static, all dispatch at compile time):
//   using H                      the handle, `struct dfx_X : WeightedHandle<dfx_X_desc, XArgs>`
//   name, channels_name          "gconv"; what the descriptor calls the channels that carry a scale ("oc", dwconv: "c")
//   FAST, GENERIC, class_text    the two path ids; the fast kernel and its class, for the refusal of a forced path
//   raw_beside_packed            the image of the fast path carries the raw weights as well (all but fc)
//   validate_shape(d)            the op's own descriptor clauses; validate_tail() follows
//   in_class(d)                  the fast kernel's shape class
//   channels(d), taps(d)         weights are {channels, taps}; one scale, bias and compensation per channel
//   src_bytes(d), dst_elems(d)   tensor sizes
//   packed_bytes(d)              the fast path's weight image
//   comp_count(d), const_count(d)  entries of the image's compensation section and of its bias / scale sections
//   fill_args(d, a)              the descriptor's fields into the kernel arguments
//   plan_fast(h, cus) -> rc      the fast path's launch plan (a failure has called fail(); create releases the handle)
//   pack(h, wei, image)          what the image holds beyond raw weights and per-channel constants: the fast path's
//                                packed weights (called on either path; deconv's compensation is not per channel)
//   check_ptrs(h, src, dst) -> rc  the alignment the path's kernel needs
//   launch(h, a, stream) -> rc   the launch(es) of one submit, through launched()
//   set_name(h)                  kernel_name from the plan and the route
//   algorithmic_ops(d)
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "dfx_internal.h"
#include "requant_host.h"

#pragma GCC visibility push(hidden)
namespace dfx {

template <class Desc, class Args>
struct WeightedHandle {
  Desc d;
  int device = 0;
  int path = 0;
  int grid = 0, block = 0, lds = 0;
  Args args = {};                  // everything but src / dst; copied per launch
  unsigned char *d_buf = nullptr;  // packed weights | raw weights | comp | bias | scale
  size_t off_wraw = 0, off_comp = 0, off_bias = 0, off_scale = 0, buf_bytes = 0;
  bool weights_set = false;
  int route = 0;                   // 0 exact, 1 fast (dfx_debug_conv_requant's numbering)
  HostStaging host;                // dfx_*_submit_host
  char kernel_name[96] = "";
};

// the handle's destructor, if it has one, runs on the handle's device
template <class H>
void weighted_release(H *h) {
  if (!h) return;
  DeviceGuard dg(h->device);
  (void)hipFree(h->d_buf);
  h->host.release();
  delete h;
}

template <class Op, class Desc>
int validate_tail(const Desc &d) {
  if (d.dst_dt < DFX_F32 || d.dst_dt > DFX_U8) return fail(DFX_ERR_INVALID, "%s: bad dst dtype", Op::name);
  if (d.bia_dt != DFX_UNDEF && (d.bia_dt < DFX_F32 || d.bia_dt > DFX_U8)) return fail(DFX_ERR_INVALID, "%s: bad bias dtype", Op::name);
  if (d.round_mode != DFX_ROUND_NEAREST && d.round_mode != DFX_ROUND_DOWN) return fail(DFX_ERR_INVALID, "%s: bad round mode", Op::name);
  if (d.nscales != 1 && d.nscales != Op::channels(d))
    return fail(DFX_ERR_INVALID, "%s: scales count must be 1 or %s", Op::name, Op::channels_name);
  if (d.force_path != -1 && d.force_path != Op::FAST && d.force_path != Op::GENERIC) return fail(DFX_ERR_INVALID, "%s: bad force_path", Op::name);
  return DFX_OK;
}

// bytes of raw weights in the handle's image
template <class Op>
size_t weighted_raw_bytes(const typename Op::H *h) {
  return (h->path == Op::FAST && !Op::raw_beside_packed) ? 0 : (size_t)Op::channels(h->d) * Op::taps(h->d);
}

template <class Op, class Desc>
int weighted_create(const Desc *desc, typename Op::H **out) {
  using H = typename Op::H;
  if (!desc || !out) return fail(DFX_ERR_INVALID, "%s_create: null argument", Op::name);
  *out = nullptr;
  const Desc &d = *desc;
  int rc = Op::validate_shape(d);
  if (!rc) rc = validate_tail<Op>(d);
  if (rc) return rc;
  const bool covered = Op::in_class(d);
  if (d.force_path == Op::FAST && !covered)
    return fail(DFX_ERR_UNSUPPORTED, "%s_create: shape outside the %s", Op::name, Op::class_text);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(DFX_ERR_NO_DEVICE, "%s_create: no HIP device (this library has no CPU path)", Op::name);
  H *h = new (std::nothrow) H();
  if (!h) return fail(DFX_ERR_HIP, "out of host memory");
  h->d = d;
  if (hipGetDevice(&h->device) != hipSuccess) h->device = 0;
  // AUTO RULE (include/dfx.h): the fast kernel everywhere in its class
  h->path = (covered && d.force_path != Op::GENERIC) ? Op::FAST : Op::GENERIC;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, h->device) != hipSuccess) {
    weighted_release(h);
    return fail(DFX_ERR_HIP, "%s_create: cannot query the device", Op::name);
  }
  const int cus = std::max(1, prop.multiProcessorCount);
  auto &a = h->args;
  Op::fill_args(d, a);
  a.dst_dt = d.dst_dt; a.relu = (d.relu || d.dst_dt == DFX_U8) ? 1 : 0; a.rm = d.round_mode;
  if (h->path == Op::FAST) {
    rc = Op::plan_fast(h, cus);
    if (rc) {
      weighted_release(h);
      return rc;
    }
  } else {  // one thread per dst element, looping where the tensor is larger than the launch
    a.items = (long long)Op::dst_elems(d);
    h->block = 256;
    h->lds = 0;
    h->grid = (int)std::min((a.items + 255) / 256, (long long)cus * 8);
  }
  h->off_wraw = round16(h->path == Op::FAST ? Op::packed_bytes(d) : 0);
  h->off_comp = h->off_wraw + round16(weighted_raw_bytes<Op>(h));
  h->off_bias = h->off_comp + round16((size_t)Op::comp_count(d) * 4);
  h->off_scale = h->off_bias + round16((size_t)Op::const_count(d) * 4);
  h->buf_bytes = h->off_scale + round16((size_t)Op::const_count(d) * 4);
  hipError_t e = hipMalloc((void **)&h->d_buf, h->buf_bytes);
  if (e != hipSuccess) {
    weighted_release(h);
    return fail(DFX_ERR_HIP, "%s_create: weight buffer: %s", Op::name, hipGetErrorString(e));
  }
  a.wpk = reinterpret_cast<decltype(a.wpk)>(h->d_buf);
  a.wraw = (const signed char *)(h->d_buf + h->off_wraw);
  a.comp = (const int *)(h->d_buf + h->off_comp);
  a.bias = (const float *)(h->d_buf + h->off_bias);
  a.scale = (const float *)(h->d_buf + h->off_scale);
  Op::set_name(h);
  *out = h;
  return DFX_OK;
}

// Builds the image on the host (whatever the op does not write stays 0), proves the requant route from the actual
// weights, bias and scales (requant_host.h) and uploads.
template <class Op>
int weighted_set_weights(typename Op::H *h, const int8_t *wei, const void *bia, const float *scales) {
  if (!h || !wei || !scales) return fail(DFX_ERR_INVALID, "%s_set_weights: null argument", Op::name);
  const auto &d = h->d;
  if (d.bia_dt != DFX_UNDEF && !bia) return fail(DFX_ERR_INVALID, "%s_set_weights: null bias", Op::name);
  const size_t taps = (size_t)Op::taps(d);  // of one channel
  std::vector<unsigned char> img(h->buf_bytes, 0);
  int *comp = (int *)(img.data() + h->off_comp);
  float *fb = (float *)(img.data() + h->off_bias), *fs = (float *)(img.data() + h->off_scale);
  memcpy(img.data() + h->off_wraw, wei, weighted_raw_bytes<Op>(h));
  // comp[k] = 128 * the sum of the channel's weights: the start value of a kernel that reads activations as s8
  const bool proven = requant_consts(Op::channels(d), taps, [&](int k, size_t i) { return wei[(size_t)k * taps + i]; }, bia, d.bia_dt,
                                     scales, d.nscales, comp, fb, fs);
  const bool fast = h->path == Op::FAST && d.round_mode == DFX_ROUND_NEAREST && proven && fast_allowed();
  Op::pack(h, wei, img.data());
  DeviceGuard dg(h->device);
  HIP_TRY(hipMemcpy(h->d_buf, img.data(), h->buf_bytes, hipMemcpyHostToDevice));
  h->route = fast ? 1 : 0;
  h->args.fast = h->route;
  h->weights_set = true;
  Op::set_name(h);
  return DFX_OK;
}

// the alignment rules of check_ptrs
template <class Op>
int need_16_bytes(const void *src, const void *dst) {
  if (((uintptr_t)src | (uintptr_t)dst) % 16) return fail(DFX_ERR_INVALID, "%s_submit: src and dst must be 16-byte aligned", Op::name);
  return DFX_OK;
}
// (the MFMA kernels of deconv and dilconv move 16 bytes per lane, their generic kernels one element)
template <class Op>
int need_16_bytes_on_fast_path(const typename Op::H *h, const void *src, const void *dst) {
  if (h->path == Op::FAST) return need_16_bytes<Op>(src, dst);
  if ((uintptr_t)dst % dt_size(h->d.dst_dt)) return fail(DFX_ERR_INVALID, "%s_submit: dst must be aligned to its element", Op::name);
  return DFX_OK;
}

// what a submit returns behind its one launch, `launch_rc` being what the op's launcher returned
template <class Op>
int launched(int launch_rc) {
  if (launch_rc != 0) return fail(DFX_ERR_UNSUPPORTED, "%s_submit: no kernel instance for this op", Op::name);
  HIP_TRY(hipGetLastError());
  return DFX_OK;
}

template <class Op>
int weighted_submit(typename Op::H *h, const void *src_dev, void *dst_dev, dfx_stream_t s) {
  if (!h || !src_dev || !dst_dev) return fail(DFX_ERR_INVALID, "%s_submit: null argument", Op::name);
  if (int rc = Op::check_ptrs(h, src_dev, dst_dev)) return rc;
  if (!h->weights_set) return fail(DFX_ERR_STATE, "%s_submit: dfx_%s_set_weights not called", Op::name, Op::name);
  DeviceGuard dg(h->device);
  auto a = h->args;  // per-launch copy: concurrent submits on several streams are independent
  a.src = (const unsigned char *)src_dev;
  a.dst = (unsigned char *)dst_dev;
  return Op::launch(h, a, (hipStream_t)s);
}

template <class Op>
int weighted_submit_host(typename Op::H *h, const void *src_host, void *dst_host) {
  if (!h || !src_host || !dst_host) return fail(DFX_ERR_INVALID, "%s_submit_host: null argument", Op::name);
  if (!h->weights_set) return fail(DFX_ERR_STATE, "%s_submit_host: dfx_%s_set_weights not called", Op::name, Op::name);
  DeviceGuard dg(h->device);
  return h->host.run(src_host, Op::src_bytes(h->d), dst_host, Op::dst_elems(h->d) * dt_size(h->d.dst_dt),
                     [h](const void *s, void *d, dfx_stream_t st) { return weighted_submit<Op>(h, s, d, st); });
}

template <class Op, class Info>
int weighted_query(const typename Op::H *h, Info *info) {
  if (!h || !info) return fail(DFX_ERR_INVALID, "%s_query: null argument", Op::name);
  memset(info, 0, sizeof(*info));
  info->path = h->path;
  info->grid = h->grid;
  info->block = h->block;
  info->lds_bytes = h->lds;
  info->device = h->device;
  const auto &d = h->d;
  info->algorithmic_ops = Op::algorithmic_ops(d);
  info->algorithmic_bytes = (uint64_t)Op::src_bytes(d) + (uint64_t)Op::channels(d) * Op::taps(d) + (uint64_t)Op::dst_elems(d) * dt_size(d.dst_dt);
  memcpy(info->kernel_name, h->kernel_name, sizeof(info->kernel_name));
  return DFX_OK;
}

// test hook: the requant route the last set_weights proved (numbering of dfx_debug_conv_requant)
template <class Op>
int weighted_requant(const typename Op::H *h, int32_t out[1]) {
  if (!h || !out) return fail(DFX_ERR_INVALID, "%s_requant: null argument", Op::name);
  if (!h->weights_set) return fail(DFX_ERR_STATE, "%s_requant: dfx_%s_set_weights not called", Op::name, Op::name);
  out[0] = h->route;
  return DFX_OK;
}

}  // namespace dfx
#pragma GCC visibility pop
