// gconv_api.hip -- host side of the grouped conv op (dfx_gconv_* of include/dfx.h): descriptor validation, choice of
// the path and of the launch geometry, weight packing for the MFMA kernel (gconv.cuh, gconv_pack.h), and the requant
// route's proof from the actual weights, bias and scales.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "gconv.cuh"
#include "gconv_pack.h"
#include "weighted_op.h"

namespace dfx {
int launch_gconv_mfma(const GcArgs &, int grid, int lds, hipStream_t, int mode, bool fast);
int launch_gconv_generic(const GcArgs &, int grid, hipStream_t);
}
using namespace dfx;

struct dfx_gconv : WeightedHandle<dfx_gconv_desc, GcArgs> {};

namespace {

struct Gconv {  // the op's part of weighted_op.h's skeleton
  using H = dfx_gconv;
  static constexpr const char *name = "gconv", *channels_name = "oc";
  static constexpr int FAST = DFX_GCONV_MFMA, GENERIC = DFX_GCONV_GENERIC;
  static constexpr const char *class_text = "MFMA kernel's class (3x3, stride (1,1) or (2,2), ic == oc a multiple of 32, ic / groups in {4, 8, 16, 32, 64}, one image below 2^31 bytes)";
  static constexpr bool raw_beside_packed = true;

  static int validate_shape(const dfx_gconv_desc &d) {
    if (d.bs <= 0 || d.ic <= 0 || d.ih <= 0 || d.iw <= 0 || d.oc <= 0 || d.oh <= 0 || d.ow <= 0 || d.kh <= 0 || d.kw <= 0)
      return fail(DFX_ERR_INVALID, "gconv: non-positive dimension");
    if (d.sh <= 0 || d.sw <= 0) return fail(DFX_ERR_INVALID, "gconv: non-positive stride");
    if (d.pad_t < 0 || d.pad_l < 0) return fail(DFX_ERR_INVALID, "gconv: negative padding");
    if (d.groups < 1) return fail(DFX_ERR_INVALID, "gconv: groups must be at least 1");
    if (d.ic % d.groups || d.oc % d.groups)
      return fail(DFX_ERR_INVALID, "gconv: ic %d and oc %d must be divisible by groups %d", d.ic, d.oc, d.groups);
    if ((long long)d.kh * d.kw * (d.ic / d.groups) > 65025)
      return fail(DFX_ERR_INVALID, "gconv: kh * kw * ic / groups beyond 65025 (the accumulator could leave s32)");
    if ((long long)(d.oh - 1) * d.sh - d.pad_t > d.ih - 1 || (long long)(d.ow - 1) * d.sw - d.pad_l > d.iw - 1)
      return fail(DFX_ERR_INVALID, "gconv: the last output row / column's window starts outside the input");
    if ((long long)d.bs * d.ih * d.iw >= (1ll << 31) || (long long)d.bs * d.oh * d.ow >= (1ll << 31))
      return fail(DFX_ERR_INVALID, "gconv: pixel count beyond 2^31");
    return DFX_OK;
  }

  // the shape class of gconv.cuh
  static bool in_class(const dfx_gconv_desc &d) {
    const long long lim = 1ll << 31;  // one image below 2^31 bytes on either side (the kernel's offsets are 64-bit)
    const int cpg = d.ic / d.groups;
    return d.kh == 3 && d.kw == 3 && d.sh == d.sw && (d.sh == 1 || d.sh == 2) && d.ic == d.oc && d.ic % 32 == 0 &&
           (cpg == 4 || cpg == 8 || cpg == 16 || cpg == 32 || cpg == 64) && (long long)d.ih * d.iw * d.ic < lim &&
           (long long)d.oh * d.ow * d.oc * (long long)dt_size(d.dst_dt) < lim;
  }

  static int channels(const dfx_gconv_desc &d) { return d.oc; }
  static size_t taps(const dfx_gconv_desc &d) { return (size_t)(d.ic / d.groups) * d.kh * d.kw; }
  static size_t src_bytes(const dfx_gconv_desc &d) { return (size_t)d.bs * d.ih * d.iw * d.ic; }
  static size_t dst_elems(const dfx_gconv_desc &d) { return (size_t)d.bs * d.oh * d.ow * d.oc; }
  static size_t packed_bytes(const dfx_gconv_desc &d) { return gconv_pack_bytes(d.oc, d.ic / d.groups); }
  static int comp_count(const dfx_gconv_desc &d) { return d.oc; }
  static int const_count(const dfx_gconv_desc &d) { return d.oc; }
  static uint64_t algorithmic_ops(const dfx_gconv_desc &d) { return 2 * (uint64_t)dst_elems(d) * d.kh * d.kw * (d.ic / d.groups); }

  static void fill_args(const dfx_gconv_desc &d, GcArgs &a) {
    a.bs = d.bs; a.ic = d.ic; a.ih = d.ih; a.iw = d.iw; a.oc = d.oc; a.oh = d.oh; a.ow = d.ow; a.groups = d.groups;
    a.kh = d.kh; a.kw = d.kw; a.sh = d.sh; a.sw = d.sw; a.pt = d.pad_t; a.pl = d.pad_l;
    a.px_total = (int)((long long)d.bs * d.oh * d.ow);
  }

  static int plan_fast(dfx_gconv *h, int cus) {
    const dfx_gconv_desc &d = h->d;
    GcArgs &a = h->args;
    const int cpg = d.ic / d.groups, nib = gconv_pack_nib(cpg);
    a.cblocks = d.oc / 32;
    a.nchunks = (a.cblocks + GC_CHUNK - 1) / GC_CHUNK;
    a.wblocks = std::min(GC_CHUNK, a.cblocks);
    a.strips = (a.px_total + 31) / 32;
    h->block = GC_THREADS;
    h->lds = a.wblocks * 9 * nib * 1024 + 3 * 32 * GC_CHUNK * 4 + (GC_THREADS / 64) * GC_STAGE_BYTES;
    // Launch: the workgroups that are resident at once (LDS: two per CU, one at cpg 64), a multiple of the chunk count;
    // a workgroup keeps its chunk's weights in LDS and its 8 waves stride over the strips.  Fewer workgroups than
    // (chunk, slot) units (tiny devices, DFX_GCONV_GRID) make the workgroups loop over the units.
    const int wg_strips = GC_THREADS / 64;
    const long long cap = (long long)cus * (nib == 2 ? 1 : 2);
    long long slots = std::min<long long>((a.strips + wg_strips - 1) / wg_strips, std::max<long long>(1, cap / a.nchunks));
    long long grid = slots * a.nchunks;
    if (const char *e = tuning_value("DFX_GCONV_TILE"); e && atoi(e) != 0) {
      // The variant that stages the input in LDS (gconv_mfma_tile_kernel), kept for the A/B of DESIGN 4.9.  An item is
      // a band of tr output rows x a block of tc <= 64 output columns of one image, about 256 pixels (one strip per
      // wave), shrunk until its halo fits in what a CU's 160 KB of LDS leave (4 KB kept free).
      const int S = d.sh, pp = 32 * a.wblocks + 16;
      const long long room = 156 * 1024 - h->lds;
      auto halo = [&](int tr, int tc) { return (long long)((tr - 1) * S + 3) * ((tc - 1) * S + 3) * pp; };
      int tc = std::min(d.ow, 64);
      while (tc > 1 && halo(1, tc) > room) tc = (tc + 1) / 2;
      int tr = std::max(1, std::min(d.oh, 256 / tc));
      while (tr > 1 && halo(tr, tc) > room) --tr;
      if (halo(tr, tc) <= room) {
        a.t_tr = tr; a.t_tc = tc; a.t_ir = (tr - 1) * S + 3; a.t_ic = (tc - 1) * S + 3; a.t_pp = pp;
        a.t_nbands = (d.oh + tr - 1) / tr; a.t_ncb = (d.ow + tc - 1) / tc;
        a.t_items = (int)((long long)d.bs * a.t_nbands * a.t_ncb);  // <= bs * oh * ow
        h->lds += (int)halo(tr, tc);
        const long long cap_t = (long long)cus * std::max(1, 160 * 1024 / h->lds);
        slots = std::min<long long>(a.t_items, std::max<long long>(1, cap_t / a.nchunks));
        grid = slots * a.nchunks;
      }
    }
    if (const char *e = tuning_value("DFX_GCONV_GRID")) {  // testing aid
      grid = std::max(1ll, std::min(grid, (long long)atoi(e)));
      slots = (grid + a.nchunks - 1) / a.nchunks;
    }
    a.slots = (int)slots;
    h->grid = (int)grid;
    // both routes' instances: set_weights may switch between them later
    if (launch_gconv_mfma(a, h->grid, h->lds, nullptr, 1, false) != 0 || launch_gconv_mfma(a, h->grid, h->lds, nullptr, 1, true) != 0)
      return fail(DFX_ERR_HIP, "gconv_create: cannot reserve %d bytes of LDS", h->lds);
    return DFX_OK;
  }

  static void pack(const dfx_gconv *h, const int8_t *wei, unsigned char *img) {
    if (h->path == DFX_GCONV_MFMA) gconv_pack(wei, h->d.oc, h->d.ic / h->d.groups, img);
  }

  static int check_ptrs(const dfx_gconv *, const void *src, const void *dst) { return need_16_bytes<Gconv>(src, dst); }

  static int launch(const dfx_gconv *h, const GcArgs &a, hipStream_t st) {
    return launched<Gconv>(h->path == DFX_GCONV_MFMA ? launch_gconv_mfma(a, h->grid, h->lds, st, 0, a.fast != 0)
                                                     : launch_gconv_generic(a, h->grid, st));
  }

  static void set_name(dfx_gconv *h) {
    const dfx_gconv_desc &d = h->d;
    if (h->path == DFX_GCONV_MFMA)
      snprintf(h->kernel_name, sizeof(h->kernel_name), "gconv_mfma%s<%dx%d,s%d,cpg%d,%s> %s", h->args.t_tr > 0 ? "_tile" : "", d.kh,
               d.kw, d.sh, d.ic / d.groups, dt_name(d.dst_dt), !h->weights_set ? "(no weights)" : h->route ? "fast" : "exact");
    else
      snprintf(h->kernel_name, sizeof(h->kernel_name), "gconv_generic<%dx%d,s%dx%d,cpg%d,%s> exact", d.kh, d.kw, d.sh, d.sw,
               d.ic / d.groups, dt_name(d.dst_dt));
  }
};

}  // namespace

extern "C" {

int dfx_gconv_create(const dfx_gconv_desc *desc, dfx_gconv_t **out) { return weighted_create<Gconv>(desc, out); }
int dfx_gconv_set_weights(dfx_gconv_t *h, const int8_t *wei, const void *bia, const float *scales) { return weighted_set_weights<Gconv>(h, wei, bia, scales); }
int dfx_gconv_submit(dfx_gconv_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s) { return weighted_submit<Gconv>(h, src_dev, dst_dev, s); }
int dfx_gconv_submit_host(dfx_gconv_t *h, const void *src_host, void *dst_host) { return weighted_submit_host<Gconv>(h, src_host, dst_host); }
int dfx_gconv_query(const dfx_gconv_t *h, dfx_gconv_info *info) { return weighted_query<Gconv>(h, info); }
int dfx_debug_gconv_requant(const dfx_gconv_t *h, int32_t out[1]) { return weighted_requant<Gconv>(h, out); }
int dfx_gconv_destroy(dfx_gconv_t *h) {
  weighted_release(h);
  return DFX_OK;
}

}  // extern "C"
