// fc_api.hip -- host side of the fully-connected op (dfx_fc_* of include/dfx.h): descriptor validation, choice of the
// path, the split-K plan, weight packing for the MFMA kernel (fc.cuh, fc_pack.h), the requant route's proof from the
// actual weights, bias and scales, and the order of the submits that share the handle's slab of partial sums.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "fc.cuh"
#include "fc_pack.h"
#include "weighted_op.h"

namespace dfx {
int launch_fc_mfma(const FcArgs &, int grid, int lds, hipStream_t, int mode);
int launch_fc_epilogue(const FcArgs &, int grid, hipStream_t, bool fast);
int launch_fc_generic(const FcArgs &, int grid, hipStream_t);
}
using namespace dfx;

// (the image has one weight section: packed weights (MFMA) or raw weights (generic), then comp | bias | scale)
struct dfx_fc : WeightedHandle<dfx_fc_desc, FcArgs> {
  int ep_grid = 0;        // of the epilogue kernel
  int *d_slab = nullptr;  // MFMA: [splitk][n_pad][oc_pad]
  TwoLaunchOrder order;   // MFMA: the two launches meet in d_slab
  ~dfx_fc() {             // (weighted_release() deletes the handle on its device)
    (void)hipFree(d_slab);
    order.destroy();
  }
};

namespace {

// Split-K plan (from tools/bench_fc's sweep).  A slab slice is n_pad * oc_pad * 4 bytes; the slab is
// capped at FC_SLAB_CAP.  K is split until there is one unit per CU, but into no more slices than staged tiles of
// FC_KT k-steps: slices of whole tiles run the kernel's branch-free path only.
constexpr size_t FC_SLAB_CAP = 64u << 20;

long long k_of(const dfx_fc_desc &d) { return (long long)d.ih * d.iw * d.ic; }

struct Fc {  // the op's part of weighted_op.h's skeleton
  using H = dfx_fc;
  static constexpr const char *name = "fc", *channels_name = "oc";
  static constexpr int FAST = DFX_FC_MFMA, GENERIC = DFX_FC_GENERIC;
  static constexpr const char *class_text = "MFMA kernel's class (ih * iw * ic a multiple of 64)";
  static constexpr bool raw_beside_packed = false;

  static int validate_shape(const dfx_fc_desc &d) {
    if (d.bs <= 0 || d.ic <= 0 || d.ih <= 0 || d.iw <= 0 || d.oc <= 0) return fail(DFX_ERR_INVALID, "fc: non-positive dimension");
    if ((long long)d.ih * d.iw > 65025 || k_of(d) > 65025)
      return fail(DFX_ERR_INVALID, "fc: ih * iw * ic beyond 65025 (the accumulator could leave s32)");
    if ((long long)d.bs * d.oc >= (1ll << 31)) return fail(DFX_ERR_INVALID, "fc: bs * oc beyond 2^31");
    if (d.bs > INT32_MAX - 31) return fail(DFX_ERR_INVALID, "fc: bs beyond 2^31 - 32 (bs rounded up to 32 must fit an int)");
    return DFX_OK;
  }

  static bool in_class(const dfx_fc_desc &d) { return k_of(d) % 64 == 0; }

  static int channels(const dfx_fc_desc &d) { return d.oc; }
  static size_t taps(const dfx_fc_desc &d) { return (size_t)k_of(d); }
  static size_t src_bytes(const dfx_fc_desc &d) { return (size_t)d.bs * (size_t)k_of(d); }
  static size_t dst_elems(const dfx_fc_desc &d) { return (size_t)d.bs * d.oc; }
  static size_t packed_bytes(const dfx_fc_desc &d) { return fc_pack_bytes(d.oc, (int)k_of(d)); }
  // the constants are padded to the MFMA kernel's blocks of 32 channels; the entries oc .. oc_pad - 1 stay 0
  static int comp_count(const dfx_fc_desc &d) { return 32 * fc_pack_blocks(d.oc); }
  static int const_count(const dfx_fc_desc &d) { return comp_count(d); }
  static uint64_t algorithmic_ops(const dfx_fc_desc &d) { return 2 * (uint64_t)d.bs * (uint64_t)k_of(d) * (uint64_t)d.oc; }

  static void fill_args(const dfx_fc_desc &d, FcArgs &a) {
    a.bs = d.bs; a.k = (int)k_of(d); a.oc = d.oc; a.ic = d.ic; a.ih = d.ih; a.iw = d.iw;
    a.ocb = fc_pack_blocks(d.oc);
    a.oc_pad = 32 * a.ocb;
    a.n_pad = (int)(((long long)d.bs + 31) / 32 * 32);
    a.splitk = 1;
  }

  static int plan_fast(dfx_fc *h, int cus) {
    const dfx_fc_desc &d = h->d;
    FcArgs &a = h->args;
    a.nks = a.k / 64;
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
    if (units >= (1ll << 31)) return fail(DFX_ERR_INVALID, "fc_create: too many work units");
    a.units = (int)units;
    long long grid = std::min<long long>(units, (long long)cus * 8);
    if (const char *e = tuning_value("DFX_FC_GRID")) grid = std::max(1ll, std::min(grid, (long long)atoi(e)));  // testing aid
    h->grid = (int)grid;
    h->block = FC_THREADS;
    h->lds = 32 * std::min(FC_CHUNK / 32, a.n_pad / 32) * FC_PITCH;
    const long long ep_items = (long long)d.bs * ((d.oc + 3) / 4);
    h->ep_grid = (int)std::min<long long>((ep_items + 255) / 256, (long long)cus * 8);
    hipError_t e = hipMalloc((void **)&h->d_slab, slice_bytes * a.splitk);
    if (e == hipSuccess) e = h->order.create();
    if (e != hipSuccess) return fail(DFX_ERR_HIP, "fc_create: slab of partial sums: %s", hipGetErrorString(e));
    a.slab = h->d_slab;
    if (launch_fc_mfma(a, h->grid, h->lds, nullptr, 1) != 0) return fail(DFX_ERR_HIP, "fc_create: cannot reserve %d bytes of LDS", h->lds);
    return DFX_OK;
  }

  static void pack(const dfx_fc *h, const int8_t *wei, unsigned char *img) {
    if (h->path == DFX_FC_MFMA) fc_pack(wei, h->d.oc, h->d.ic, h->d.ih, h->d.iw, img);
  }

  static int check_ptrs(const dfx_fc *, const void *src, const void *dst) { return need_16_bytes<Fc>(src, dst); }

  static int launch(dfx_fc *h, const FcArgs &a, hipStream_t st) {
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

  static void set_name(dfx_fc *h) {
    if (h->path == DFX_FC_MFMA)
      snprintf(h->kernel_name, sizeof(h->kernel_name), "fc_mfma<k%d,%s,sk%d> %s", h->args.k, dt_name(h->d.dst_dt), h->args.splitk,
               !h->weights_set ? "(no weights)" : h->route ? "fast" : "exact");
    else
      snprintf(h->kernel_name, sizeof(h->kernel_name), "fc_generic<%s> exact", dt_name(h->d.dst_dt));
  }
};

}  // namespace

extern "C" {

int dfx_fc_create(const dfx_fc_desc *desc, dfx_fc_t **out) { return weighted_create<Fc>(desc, out); }
int dfx_fc_set_weights(dfx_fc_t *h, const int8_t *wei, const void *bia, const float *scales) { return weighted_set_weights<Fc>(h, wei, bia, scales); }
int dfx_fc_submit(dfx_fc_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s) { return weighted_submit<Fc>(h, src_dev, dst_dev, s); }
int dfx_fc_submit_host(dfx_fc_t *h, const void *src_host, void *dst_host) { return weighted_submit_host<Fc>(h, src_host, dst_host); }
int dfx_fc_query(const dfx_fc_t *h, dfx_fc_info *info) {
  const int rc = weighted_query<Fc>(h, info);
  if (rc == DFX_OK) info->splitk = h->args.splitk;
  return rc;
}
int dfx_debug_fc_requant(const dfx_fc_t *h, int32_t out[1]) { return weighted_requant<Fc>(h, out); }
int dfx_fc_destroy(dfx_fc_t *h) {
  weighted_release(h);
  return DFX_OK;
}

}  // extern "C"
