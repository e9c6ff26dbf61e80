// imgconv_api.hip -- host side of the first-layer conv op (dfx_imgconv_* of include/dfx.h): descriptor validation,
// choice of the path and of the launch geometry, weight packing for the MFMA kernel (imgconv.cuh, imgconv_pack.h), and
// the requant route's proof from the actual weights, bias and scales (requant_host.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "imgconv.cuh"
#include "imgconv_pack.h"
#include "weighted_op.h"

namespace dfx {
int launch_imgconv_mfma(const IcArgs &, int grid, int lds, hipStream_t, int mode, bool fast);
int launch_imgconv_generic(const IcArgs &, int grid, hipStream_t);
}
using namespace dfx;

struct dfx_imgconv : WeightedHandle<dfx_imgconv_desc, IcArgs> {};

namespace {

struct Imgconv {  // the op's part of weighted_op.h's skeleton
  using H = dfx_imgconv;
  static constexpr const char *name = "imgconv", *channels_name = "oc";
  static constexpr int FAST = DFX_IMGCONV_MFMA, GENERIC = DFX_IMGCONV_GENERIC;
  static constexpr const char *class_text = "MFMA kernel's class (ic 3 or 4, window / stride 7x7 / 2, 3x3 / 1 or 3x3 / 2, padding at most k - 1, oc a multiple of 32 up to 128, one image below 2^31 bytes)";
  static constexpr bool raw_beside_packed = true;

  static int validate_shape(const dfx_imgconv_desc &d) {
    if (d.bs <= 0 || d.ic <= 0 || d.ih <= 0 || d.iw <= 0 || d.oc <= 0 || d.oh <= 0 || d.ow <= 0 || d.kh <= 0 || d.kw <= 0)
      return fail(DFX_ERR_INVALID, "imgconv: non-positive dimension");
    if (d.ic > 4) return fail(DFX_ERR_INVALID, "imgconv: ic %d beyond 4 (an image has 1 to 4 channels; dfx_conv / dfx_gconv take more)", d.ic);
    if (d.kh > 255 || d.kw > 255) return fail(DFX_ERR_INVALID, "imgconv: window beyond 255");
    if (d.sh <= 0 || d.sw <= 0) return fail(DFX_ERR_INVALID, "imgconv: non-positive stride");
    if (d.pad_t < 0 || d.pad_l < 0) return fail(DFX_ERR_INVALID, "imgconv: negative padding");
    if ((long long)d.kh * d.kw * d.ic > 65025)
      return fail(DFX_ERR_INVALID, "imgconv: kh * kw * ic beyond 65025 (the accumulator could leave s32)");
    if ((long long)(d.oh - 1) * d.sh - d.pad_t > d.ih - 1 || (long long)(d.ow - 1) * d.sw - d.pad_l > d.iw - 1)
      return fail(DFX_ERR_INVALID, "imgconv: the last output row / column's window starts outside the input");
    if ((long long)d.bs * d.ih * d.iw >= (1ll << 31) || (long long)d.bs * d.oh * d.ow >= (1ll << 31))
      return fail(DFX_ERR_INVALID, "imgconv: pixel count beyond 2^31");
    return DFX_OK;
  }

  // the shape class of imgconv.cuh
  static bool in_class(const dfx_imgconv_desc &d) {
    const long long lim = 1ll << 31;  // one image below 2^31 bytes on either side (the kernel's offsets are 64-bit)
    const bool window = d.kh == d.kw && d.sh == d.sw && ((d.kh == 7 && d.sh == 2) || (d.kh == 3 && (d.sh == 1 || d.sh == 2)));
    return window && (d.ic == 3 || d.ic == 4) && d.pad_t <= d.kh - 1 && d.pad_l <= d.kw - 1 && d.oc % 32 == 0 &&
           d.oc <= 32 * IC_MAX_BLOCKS && (long long)d.ih * d.iw * d.ic < lim &&
           (long long)d.oh * d.ow * d.oc * (long long)dt_size(d.dst_dt) < lim;
  }

  static int channels(const dfx_imgconv_desc &d) { return d.oc; }
  static size_t taps(const dfx_imgconv_desc &d) { return (size_t)d.ic * d.kh * d.kw; }
  static size_t src_bytes(const dfx_imgconv_desc &d) { return (size_t)d.bs * d.ih * d.iw * d.ic; }
  static size_t dst_elems(const dfx_imgconv_desc &d) { return (size_t)d.bs * d.oh * d.ow * d.oc; }
  static size_t packed_bytes(const dfx_imgconv_desc &d) { return imgconv_pack_bytes(d.oc, d.kh); }
  static int comp_count(const dfx_imgconv_desc &d) { return d.oc; }
  static int const_count(const dfx_imgconv_desc &d) { return d.oc; }
  static uint64_t algorithmic_ops(const dfx_imgconv_desc &d) { return 2 * (uint64_t)dst_elems(d) * d.kh * d.kw * d.ic; }

  static void fill_args(const dfx_imgconv_desc &d, IcArgs &a) {
    a.bs = d.bs; a.ic = d.ic; a.ih = d.ih; a.iw = d.iw; a.oc = d.oc; a.oh = d.oh; a.ow = d.ow;
    a.kh = d.kh; a.kw = d.kw; a.sh = d.sh; a.sw = d.sw; a.pt = d.pad_t; a.pl = d.pad_l;
    a.src_total = (long long)src_bytes(d);
  }

  static int plan_fast(dfx_imgconv *h, int cus) {
    const dfx_imgconv_desc &d = h->d;
    IcArgs &a = h->args;
    const int K = d.kh, S = d.sh;
    a.cblocks = d.oc / 32;
    h->block = IC_THREADS;
    const int fixed = (int)packed_bytes(d) + 3 * 32 * IC_MAX_BLOCKS * 4 + (IC_THREADS / 64) * GC_STAGE_BYTES;
    // An item is a band of tr output rows x a block of tc <= 64 output columns of one image, about 512 pixels (two
    // strips per wave), the columns of a row split evenly; its halo is ir rows of icp pixels (the lanes of the last
    // column read 4 pixels from kernel column 4 (7x7) or 0 (3x3) on, rounded up to whole groups of 4), kept below 48 KB.
    const int ncb = (d.ow + 63) / 64, tc = (d.ow + ncb - 1) / ncb;
    const int icp = (((tc - 1) * S + (K == 7 ? 8 : 4)) + 3) & ~3;
    auto halo = [&](int tr) { return (long long)((tr - 1) * S + K) * icp * 4; };
    int tr = std::max(1, std::min(d.oh, 512 / tc));
    while (tr > 1 && halo(tr) > 48 * 1024) --tr;
    a.t_tr = tr; a.t_tc = tc; a.t_ir = (tr - 1) * S + K; a.t_icp = icp;
    a.t_nbands = (d.oh + tr - 1) / tr; a.t_ncb = ncb;
    const long long items = (long long)d.bs * a.t_nbands * ncb;  // <= bs * oh * ow < 2^31
    a.t_items = (int)items;
    h->lds = fixed + (int)halo(tr);
    // Launch: the workgroups that are resident at once (by LDS, at most 4 of 512 threads per CU); fewer workgroups
    // than items (small devices, DFX_IMGCONV_GRID) make the workgroups loop over the items.
    long long grid = std::min<long long>(items, (long long)cus * std::min(4, std::max(1, 160 * 1024 / h->lds)));
    if (const char *e = tuning_value("DFX_IMGCONV_GRID")) grid = std::max(1ll, std::min(grid, (long long)atoi(e)));  // testing aid
    h->grid = (int)grid;
    // both routes' instances: set_weights may switch between them later
    if (launch_imgconv_mfma(a, h->grid, h->lds, nullptr, 1, false) != 0 || launch_imgconv_mfma(a, h->grid, h->lds, nullptr, 1, true) != 0)
      return fail(DFX_ERR_HIP, "imgconv_create: cannot reserve %d bytes of LDS", h->lds);
    return DFX_OK;
  }

  static void pack(const dfx_imgconv *h, const int8_t *wei, unsigned char *img) {
    if (h->path == DFX_IMGCONV_MFMA) imgconv_pack(wei, h->d.oc, h->d.ic, h->d.kh, img);
  }

  static int check_ptrs(const dfx_imgconv *, const void *, const void *dst) {
    if ((uintptr_t)dst % 16) return fail(DFX_ERR_INVALID, "imgconv_submit: dst must be 16-byte aligned");
    return DFX_OK;
  }

  static int launch(const dfx_imgconv *h, const IcArgs &a, hipStream_t st) {
    return launched<Imgconv>(h->path == DFX_IMGCONV_MFMA ? launch_imgconv_mfma(a, h->grid, h->lds, st, 0, a.fast != 0)
                                                         : launch_imgconv_generic(a, h->grid, st));
  }

  static void set_name(dfx_imgconv *h) {
    const dfx_imgconv_desc &d = h->d;
    if (h->path == DFX_IMGCONV_MFMA)
      snprintf(h->kernel_name, sizeof(h->kernel_name), "imgconv_mfma<%dx%d,s%d,ic%d,oc%d,%s> %s", d.kh, d.kw, d.sh, d.ic, d.oc,
               dt_name(d.dst_dt), !h->weights_set ? "(no weights)" : h->route ? "fast" : "exact");
    else
      snprintf(h->kernel_name, sizeof(h->kernel_name), "imgconv_generic<%dx%d,s%dx%d,ic%d,oc%d,%s> %s", d.kh, d.kw, d.sh, d.sw, d.ic,
               d.oc, dt_name(d.dst_dt), !h->weights_set ? "(no weights)" : "exact");
  }
};

}  // namespace

extern "C" {

int dfx_imgconv_create(const dfx_imgconv_desc *desc, dfx_imgconv_t **out) { return weighted_create<Imgconv>(desc, out); }
int dfx_imgconv_set_weights(dfx_imgconv_t *h, const int8_t *wei, const void *bia, const float *scales) { return weighted_set_weights<Imgconv>(h, wei, bia, scales); }
int dfx_imgconv_submit(dfx_imgconv_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s) { return weighted_submit<Imgconv>(h, src_dev, dst_dev, s); }
int dfx_imgconv_submit_host(dfx_imgconv_t *h, const void *src_host, void *dst_host) { return weighted_submit_host<Imgconv>(h, src_host, dst_host); }
int dfx_imgconv_query(const dfx_imgconv_t *h, dfx_imgconv_info *info) { return weighted_query<Imgconv>(h, info); }
int dfx_debug_imgconv_requant(const dfx_imgconv_t *h, int32_t out[1]) { return weighted_requant<Imgconv>(h, out); }
int dfx_imgconv_destroy(dfx_imgconv_t *h) {
  weighted_release(h);
  return DFX_OK;
}

}  // extern "C"
