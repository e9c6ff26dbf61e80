// dilconv_api.hip -- host side of the dilated conv op (dfx_dilconv_* of include/dfx.h): descriptor validation, choice of
// the path, of the LDS plan (K-steps per weight slab, one or two slab buffers) and of the launch geometry, weight packing
// for the MFMA kernel (dilconv.cuh, dilconv_pack.h), and the requant route's proof from the actual weights, bias and
// scales (requant_host.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "dilconv.cuh"
#include "dilconv_pack.h"
#include "weighted_op.h"

namespace dfx {
int launch_dilconv_mfma(const DlArgs &, int grid, int lds, hipStream_t, int mode, bool fast);
int launch_dilconv_generic(const DlArgs &, int grid, hipStream_t);
}
using namespace dfx;

static_assert(DL_CHUNK == DL_PACK_CHUNK, "the kernel and the packer must agree on the chunk");

struct dfx_dilconv : WeightedHandle<dfx_dilconv_desc, DlArgs> {};

namespace {

constexpr int LDS_LIMIT = 160 * 1024;
constexpr int DEFAULT_SLAB = 3;    // K-steps per slab and strips per wave: DESIGN.md section 4.13, profiles/dilconv/
constexpr int DEFAULT_STRIPS = 1;

struct Dilconv {  // the op's part of weighted_op.h's skeleton
  using H = dfx_dilconv;
  static constexpr const char *name = "dilconv", *channels_name = "oc";
  static constexpr int FAST = DFX_DILCONV_MFMA, GENERIC = DFX_DILCONV_GENERIC;  // AUTO RULE: DESIGN.md section 4.13
  static constexpr const char *class_text = "MFMA kernel's class (3x3 window; stride (1,1); ic and oc multiples of 32; one image below 2^31 bytes)";
  static constexpr bool raw_beside_packed = true;

  static int validate_shape(const dfx_dilconv_desc &d) {
    if (d.bs <= 0 || d.ic <= 0 || d.ih <= 0 || d.iw <= 0 || d.oc <= 0 || d.oh <= 0 || d.ow <= 0 || d.kh <= 0 || d.kw <= 0)
      return fail(DFX_ERR_INVALID, "dilconv: non-positive dimension");
    if (d.kh > 255 || d.kw > 255) return fail(DFX_ERR_INVALID, "dilconv: window beyond 255");
    if (d.sh <= 0 || d.sw <= 0 || d.sh > 255 || d.sw > 255) return fail(DFX_ERR_INVALID, "dilconv: stride outside 1 .. 255");
    if (d.dh <= 0 || d.dw <= 0 || d.dh > 255 || d.dw > 255) return fail(DFX_ERR_INVALID, "dilconv: dilation outside 1 .. 255");
    if (d.pad_t < 0 || d.pad_l < 0) return fail(DFX_ERR_INVALID, "dilconv: negative padding");
    if (d.pad_t > (d.kh - 1) * d.dh || d.pad_l > (d.kw - 1) * d.dw) return fail(DFX_ERR_INVALID, "dilconv: padding beyond (k - 1) * dilation");
    if ((long long)d.kh * d.kw * d.ic > 65025)
      return fail(DFX_ERR_INVALID, "dilconv: kh * kw * ic beyond 65025 (the accumulator could leave s32)");
    if (((long long)d.oh - 1) * d.sh - d.pad_t > (long long)d.ih - 1 || ((long long)d.ow - 1) * d.sw - d.pad_l > (long long)d.iw - 1)
      return fail(DFX_ERR_INVALID, "dilconv: an output row / column starts below / right of the input");
    if ((long long)d.bs * d.ih * d.iw >= (1ll << 31) || (long long)d.bs * d.oh * d.ow >= (1ll << 31))
      return fail(DFX_ERR_INVALID, "dilconv: pixel count beyond 2^31");
    return DFX_OK;
  }

  // the shape class of dilconv.cuh: nothing in it depends on how large ic is
  static bool in_class(const dfx_dilconv_desc &d) {
    const long long lim = 1ll << 31;  // one image below 2^31 bytes on either side (the kernel's offsets are 64-bit)
    if (d.kh != 3 || d.kw != 3 || d.sh != 1 || d.sw != 1 || d.ic % 32 || d.oc % 32) return false;
    return (long long)d.ih * d.iw * d.ic < lim && (long long)d.oh * d.ow * d.oc * (long long)dt_size(d.dst_dt) < lim;
  }

  static int channels(const dfx_dilconv_desc &d) { return d.oc; }
  static size_t taps(const dfx_dilconv_desc &d) { return (size_t)d.ic * d.kh * d.kw; }
  static size_t src_bytes(const dfx_dilconv_desc &d) { return (size_t)d.bs * d.ih * d.iw * d.ic; }
  static size_t dst_elems(const dfx_dilconv_desc &d) { return (size_t)d.bs * d.oh * d.ow * d.oc; }
  static size_t packed_bytes(const dfx_dilconv_desc &d) { return dilconv_pack_bytes(d.oc, d.ic); }
  // comp[k] = 128 * sum of the channel's weights is the MFMA kernel's start value: a skipped tap is the activation 0,
  // i.e. the s8 operand -128, for EVERY pixel, so the compensation is one number per channel
  static int comp_count(const dfx_dilconv_desc &d) { return d.oc; }
  static int const_count(const dfx_dilconv_desc &d) { return d.oc; }
  // the kh * kw taps of the un-stuffed window, per output value
  static uint64_t algorithmic_ops(const dfx_dilconv_desc &d) { return 2ull * d.bs * d.oh * d.ow * d.oc * d.ic * d.kh * d.kw; }

  static void fill_args(const dfx_dilconv_desc &d, DlArgs &a) {
    a.bs = d.bs; a.ic = d.ic; a.ih = d.ih; a.iw = d.iw; a.oc = d.oc; a.oh = d.oh; a.ow = d.ow;
    a.kh = d.kh; a.kw = d.kw; a.sh = d.sh; a.sw = d.sw; a.dh = d.dh; a.dw = d.dw; a.pt = d.pad_t; a.pl = d.pad_l;
    a.px_total = (int)((long long)d.bs * d.oh * d.ow);
  }

  static int plan_fast(dfx_dilconv *h, int cus) {
    const dfx_dilconv_desc &d = h->d;
    DlArgs &a = h->args;
    a.cblocks = d.oc / 32;
    a.ksteps = d.ic / 32;
    a.wblocks = std::min(DL_CHUNK, a.cblocks);
    a.nchunks = (a.cblocks + DL_CHUNK - 1) / DL_CHUNK;
    a.strips = (a.px_total + 31) / 32;
    // LDS plan: slab K-steps of the chunk per buffer; what LDS holds does not depend on ic (36 KB per K-step at 4
    // blocks: 3 K-steps at most).  A second buffer where two fit and there is more than one slab to stream.
    const int kstep_bytes = a.wblocks * DL_KSTEP;
    const int slab_max = (LDS_LIMIT - DL_FIXED_LDS) / kstep_bytes;  // >= 3
    int slab = DEFAULT_SLAB;
    if (const char *e = tuning_value("DFX_DILCONV_SLAB")) slab = atoi(e);
    a.slab = std::min(std::max(1, std::min(slab, slab_max)), a.ksteps);
    // ... and a thread's DL_WREG registers of 16 bytes hold its share of a slab (dilconv.cuh)
    a.nbuf = (a.slab < a.ksteps && 2 * a.slab * kstep_bytes + DL_FIXED_LDS <= LDS_LIMIT &&
              a.slab * kstep_bytes <= DL_WREG * DL_THREADS * 16) ? 2 : 1;
    a.rstrips = DEFAULT_STRIPS;
    if (const char *e = tuning_value("DFX_DILCONV_STRIPS")) a.rstrips = std::min(std::max(1, atoi(e)), DL_MAX_STRIPS);  // A/B aid
    h->block = DL_THREADS;
    h->lds = a.nbuf * a.slab * kstep_bytes + DL_FIXED_LDS;
    // Launch: the workgroups that are resident at once (by LDS, at most 4 per CU), a multiple of the chunk count; a
    // workgroup (a "slot" of its chunk) takes DL_WAVES * rstrips strips per pass over the chunk's weights and strides
    // over the strips.  Fewer workgroups than (chunk, slot) units (tiny devices, DFX_DILCONV_GRID) make the workgroups
    // loop over the units.
    const int wg_strips = DL_WAVES * a.rstrips;
    const long long cap = (long long)cus * std::min(4, std::max(1, LDS_LIMIT / h->lds));
    long long slots = std::min<long long>((a.strips + wg_strips - 1) / wg_strips, std::max<long long>(1, cap / a.nchunks));
    long long grid = slots * a.nchunks;
    if (const char *e = tuning_value("DFX_DILCONV_GRID")) {  // testing aid
      grid = std::max(1ll, std::min(grid, (long long)atoi(e)));
      slots = (grid + a.nchunks - 1) / a.nchunks;
    }
    a.slots = (int)slots;
    h->grid = (int)grid;
    // both routes' instances: set_weights may switch between them later
    if (launch_dilconv_mfma(a, h->grid, h->lds, nullptr, 1, false) != 0 || launch_dilconv_mfma(a, h->grid, h->lds, nullptr, 1, true) != 0)
      return fail(DFX_ERR_HIP, "dilconv_create: cannot reserve %d bytes of LDS", h->lds);
    return DFX_OK;
  }

  static void pack(const dfx_dilconv *h, const int8_t *wei, unsigned char *img) {
    if (h->path == DFX_DILCONV_MFMA) dilconv_pack(wei, h->d.oc, h->d.ic, img);
  }

  static int check_ptrs(const dfx_dilconv *h, const void *src, const void *dst) { return need_16_bytes_on_fast_path<Dilconv>(h, src, dst); }

  static int launch(const dfx_dilconv *h, const DlArgs &a, hipStream_t st) {
    return launched<Dilconv>(h->path == DFX_DILCONV_MFMA ? launch_dilconv_mfma(a, h->grid, h->lds, st, 0, a.fast != 0)
                                                         : launch_dilconv_generic(a, h->grid, st));
  }

  static void set_name(dfx_dilconv *h) {
    const dfx_dilconv_desc &d = h->d;
    if (h->path == DFX_DILCONV_MFMA)
      snprintf(h->kernel_name, sizeof(h->kernel_name), "dilconv_mfma<3x3,d%dx%d,ic%d,oc%d,%s,slab%dx%d,r%d> %s", d.dh, d.dw, d.ic, d.oc,
               dt_name(d.dst_dt), h->args.slab, h->args.nbuf, h->args.rstrips, !h->weights_set ? "(no weights)" : h->route ? "fast" : "exact");
    else
      snprintf(h->kernel_name, sizeof(h->kernel_name), "dilconv_generic<%dx%d,s%dx%d,d%dx%d,ic%d,oc%d,%s> %s", d.kh, d.kw, d.sh, d.sw,
               d.dh, d.dw, d.ic, d.oc, dt_name(d.dst_dt), !h->weights_set ? "(no weights)" : "exact");
  }
};

}  // namespace

extern "C" {

int dfx_dilconv_create(const dfx_dilconv_desc *desc, dfx_dilconv_t **out) { return weighted_create<Dilconv>(desc, out); }
int dfx_dilconv_set_weights(dfx_dilconv_t *h, const int8_t *wei, const void *bia, const float *scales) { return weighted_set_weights<Dilconv>(h, wei, bia, scales); }
int dfx_dilconv_submit(dfx_dilconv_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s) { return weighted_submit<Dilconv>(h, src_dev, dst_dev, s); }
int dfx_dilconv_submit_host(dfx_dilconv_t *h, const void *src_host, void *dst_host) { return weighted_submit_host<Dilconv>(h, src_host, dst_host); }
int dfx_dilconv_query(const dfx_dilconv_t *h, dfx_dilconv_info *info) { return weighted_query<Dilconv>(h, info); }
int dfx_debug_dilconv_requant(const dfx_dilconv_t *h, int32_t out[1]) { return weighted_requant<Dilconv>(h, out); }
int dfx_dilconv_destroy(dfx_dilconv_t *h) {
  weighted_release(h);
  return DFX_OK;
}

}  // extern "C"
