// deconv_api.hip -- host side of the transposed conv op (dfx_deconv_* of include/dfx.h): descriptor validation, choice of
// the path and of the launch geometry, weight packing for the MFMA kernel (deconv.cuh, deconv_pack.h), and the requant
// route's proof from the actual weights, bias and scales (requant_host.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "deconv.cuh"
#include "deconv_pack.h"
#include "weighted_op.h"

namespace dfx {
int launch_deconv_mfma(const DcArgs &, int grid, int lds, hipStream_t, int mode, bool fast);
int launch_deconv_generic(const DcArgs &, int grid, hipStream_t);
}
using namespace dfx;

struct dfx_deconv : WeightedHandle<dfx_deconv_desc, DcArgs> {};  // (the image's comp section: 4 parities)

namespace {

constexpr int LDS_LIMIT = 160 * 1024;

// sum over the outputs o < on of the taps k < kn that reach o: (o + pad - k) a multiple of `s` whose quotient is below `in`
unsigned long long taps_along(int in, int on, int kn, int s, int pad) {
  unsigned long long n = 0;
  for (int k = 0; k < kn; ++k) {  // o = i * s + k - pad in [0, on)
    const long long lo = std::max(0ll, ((long long)pad - k + s - 1) / s);  // pad - k <= pad <= kn - 1: the ceiling of a value > -s
    const long long hi = std::min<long long>(in - 1, ((long long)on - 1 + pad - k) >= 0 ? ((long long)on - 1 + pad - k) / s : -1);
    if (hi >= lo) n += (unsigned long long)(hi - lo + 1);
  }
  return n;
}

struct Deconv {  // the op's part of weighted_op.h's skeleton
  using H = dfx_deconv;
  static constexpr const char *name = "deconv", *channels_name = "oc";
  static constexpr int FAST = DFX_DECONV_MFMA, GENERIC = DFX_DECONV_GENERIC;  // AUTO RULE: DESIGN.md section 4.12
  static constexpr const char *class_text = "MFMA kernel's class (stride (2,2); window 2x2 with pad 0, 3x3 or 4x4; ic and oc multiples of 32; one output block's fragments within 160 KB of LDS; one image below 2^31 bytes)";
  static constexpr bool raw_beside_packed = true;

  static int validate_shape(const dfx_deconv_desc &d) {
    if (d.bs <= 0 || d.ic <= 0 || d.ih <= 0 || d.iw <= 0 || d.oc <= 0 || d.oh <= 0 || d.ow <= 0 || d.kh <= 0 || d.kw <= 0)
      return fail(DFX_ERR_INVALID, "deconv: non-positive dimension");
    if (d.kh > 255 || d.kw > 255) return fail(DFX_ERR_INVALID, "deconv: window beyond 255");
    if (d.sh <= 0 || d.sw <= 0 || d.sh > 255 || d.sw > 255) return fail(DFX_ERR_INVALID, "deconv: stride outside 1 .. 255");
    if (d.pad_t < 0 || d.pad_l < 0) return fail(DFX_ERR_INVALID, "deconv: negative padding");
    if (d.pad_t > d.kh - 1 || d.pad_l > d.kw - 1) return fail(DFX_ERR_INVALID, "deconv: padding beyond k - 1");
    if ((long long)d.kh * d.kw * d.ic > 65025)
      return fail(DFX_ERR_INVALID, "deconv: kh * kw * ic beyond 65025 (the accumulator could leave s32)");
    if (d.oh > ((long long)d.ih - 1) * d.sh + d.kh - d.pad_t || d.ow > ((long long)d.iw - 1) * d.sw + d.kw - d.pad_l)
      return fail(DFX_ERR_INVALID, "deconv: output size beyond (in - 1) * stride + k - pad");
    if ((long long)d.bs * d.ih * d.iw >= (1ll << 31) || (long long)d.bs * d.oh * d.ow >= (1ll << 31))
      return fail(DFX_ERR_INVALID, "deconv: pixel count beyond 2^31");
    return DFX_OK;
  }

  // the shape class of deconv.cuh
  static bool in_class(const dfx_deconv_desc &d) {
    const long long lim = 1ll << 31;  // one image below 2^31 bytes on either side (the kernel's offsets are 64-bit)
    const bool window = d.kh == d.kw && d.sh == 2 && d.sw == 2 && ((d.kh == 2 && d.pad_t == 0 && d.pad_l == 0) || d.kh == 3 || d.kh == 4);
    if (!window || d.ic % 32 || d.oc % 32) return false;
    if ((long long)deconv_pack_block_bytes(d.ic, d.kh) + DC_FIXED_LDS > LDS_LIMIT) return false;  // one block's fragments must fit
    return (long long)d.ih * d.iw * d.ic < lim && (long long)d.oh * d.ow * d.oc * (long long)dt_size(d.dst_dt) < lim;
  }

  static int channels(const dfx_deconv_desc &d) { return d.oc; }
  static size_t taps(const dfx_deconv_desc &d) { return (size_t)d.ic * d.kh * d.kw; }
  static size_t src_bytes(const dfx_deconv_desc &d) { return (size_t)d.bs * d.ih * d.iw * d.ic; }
  static size_t dst_elems(const dfx_deconv_desc &d) { return (size_t)d.bs * d.oh * d.ow * d.oc; }
  static size_t packed_bytes(const dfx_deconv_desc &d) { return deconv_pack_bytes(d.oc, d.ic, d.kh); }
  static int comp_count(const dfx_deconv_desc &d) { return 4 * d.oc; }
  static int const_count(const dfx_deconv_desc &d) { return d.oc; }
  // the taps that exist: the (oy, ky) pairs times the (ox, kx) pairs, per image, input and output channel
  static uint64_t algorithmic_ops(const dfx_deconv_desc &d) {
    return 2ull * d.bs * d.ic * d.oc * taps_along(d.ih, d.oh, d.kh, d.sh, d.pad_t) * taps_along(d.iw, d.ow, d.kw, d.sw, d.pad_l);
  }

  static void fill_args(const dfx_deconv_desc &d, DcArgs &a) {
    a.bs = d.bs; a.ic = d.ic; a.ih = d.ih; a.iw = d.iw; a.oc = d.oc; a.oh = d.oh; a.ow = d.ow;
    a.kh = d.kh; a.kw = d.kw; a.sh = d.sh; a.sw = d.sw; a.pt = d.pad_t; a.pl = d.pad_l;
  }

  static int plan_fast(dfx_deconv *h, int cus) {
    const dfx_deconv_desc &d = h->d;
    DcArgs &a = h->args;
    const int wblk = (int)deconv_pack_block_bytes(d.ic, d.kh);
    a.cblocks = d.oc / 32;
    a.ksteps = d.ic / 32;
    a.wblocks = std::min({DC_CHUNK, a.cblocks, (LDS_LIMIT - DC_FIXED_LDS) / wblk});  // >= 1 inside the class
    a.nchunks = (a.cblocks + a.wblocks - 1) / a.wblocks;
    // base grid: output row oy = 2 yb + a - pad_t, yb = (oy + pad_t) / 2 over oy < oh (YB <= oh, XB <= ow)
    a.yb0 = d.pad_t / 2; a.YB = (d.oh - 1 + d.pad_t) / 2 - a.yb0 + 1;
    a.xb0 = d.pad_l / 2; a.XB = (d.ow - 1 + d.pad_l) / 2 - a.xb0 + 1;
    a.bp_total = (int)((long long)d.bs * a.YB * a.XB);
    a.strips = (a.bp_total + 31) / 32;
    h->block = DC_THREADS;
    h->lds = a.wblocks * wblk + DC_FIXED_LDS;
    // Launch: the workgroups that are resident at once (by LDS, at most 4 per CU), a multiple of the chunk count; a
    // workgroup keeps its chunk's weights in LDS and its waves stride over the strips.  Fewer workgroups than
    // (chunk, slot) units (tiny devices, DFX_DECONV_GRID) make the workgroups loop over the units.
    const int wg_strips = DC_THREADS / 64;
    const long long cap = (long long)cus * std::min(4, std::max(1, LDS_LIMIT / h->lds));
    long long slots = std::min<long long>((a.strips + wg_strips - 1) / wg_strips, std::max<long long>(1, cap / a.nchunks));
    long long grid = slots * a.nchunks;
    if (const char *e = tuning_value("DFX_DECONV_GRID")) {  // testing aid
      grid = std::max(1ll, std::min(grid, (long long)atoi(e)));
      slots = (grid + a.nchunks - 1) / a.nchunks;
    }
    a.slots = (int)slots;
    h->grid = (int)grid;
    // both routes' instances: set_weights may switch between them later
    if (launch_deconv_mfma(a, h->grid, h->lds, nullptr, 1, false) != 0 || launch_deconv_mfma(a, h->grid, h->lds, nullptr, 1, true) != 0)
      return fail(DFX_ERR_HIP, "deconv_create: cannot reserve %d bytes of LDS", h->lds);
    return DFX_OK;
  }

  // The skeleton's compensation runs over ALL taps of a channel, which is what the proof needs: every output sums a
  // subset of them, so |acc| <= 255 * max(P, N) holds.  No kernel starts from it: the generic one takes none, the
  // MFMA one the start value of parity (a, b), 128 * the sum of ITS taps (ky % 2 == a, kx % 2 == b).
  static void pack(const dfx_deconv *h, const int8_t *wei, unsigned char *img) {
    const dfx_deconv_desc &d = h->d;
    int *comp = (int *)(img + h->off_comp);
    memset(comp, 0, (size_t)d.oc * 4);
    if (h->path != DFX_DECONV_MFMA) return;
    deconv_pack(wei, d.oc, d.ic, d.kh, img);
    for (int k = 0; k < d.oc; ++k)
      for (int i = 0; i < d.ic; ++i)
        for (int ky = 0; ky < d.kh; ++ky)
          for (int kx = 0; kx < d.kw; ++kx)
            comp[(size_t)((ky & 1) * 2 + (kx & 1)) * d.oc + k] += 128 * (int)wei[(((size_t)k * d.ic + i) * d.kh + ky) * d.kw + kx];
  }

  static int check_ptrs(const dfx_deconv *h, const void *src, const void *dst) { return need_16_bytes_on_fast_path<Deconv>(h, src, dst); }

  static int launch(const dfx_deconv *h, const DcArgs &a, hipStream_t st) {
    return launched<Deconv>(h->path == DFX_DECONV_MFMA ? launch_deconv_mfma(a, h->grid, h->lds, st, 0, a.fast != 0)
                                                       : launch_deconv_generic(a, h->grid, st));
  }

  static void set_name(dfx_deconv *h) {
    const dfx_deconv_desc &d = h->d;
    if (h->path == DFX_DECONV_MFMA)
      snprintf(h->kernel_name, sizeof(h->kernel_name), "deconv_mfma<%dx%d,s2,ic%d,oc%d,%s> %s", d.kh, d.kw, d.ic, d.oc, dt_name(d.dst_dt),
               !h->weights_set ? "(no weights)" : h->route ? "fast" : "exact");
    else
      snprintf(h->kernel_name, sizeof(h->kernel_name), "deconv_generic<%dx%d,s%dx%d,ic%d,oc%d,%s> %s", d.kh, d.kw, d.sh, d.sw, d.ic,
               d.oc, dt_name(d.dst_dt), !h->weights_set ? "(no weights)" : "exact");
  }
};

}  // namespace

extern "C" {

int dfx_deconv_create(const dfx_deconv_desc *desc, dfx_deconv_t **out) { return weighted_create<Deconv>(desc, out); }
int dfx_deconv_set_weights(dfx_deconv_t *h, const int8_t *wei, const void *bia, const float *scales) { return weighted_set_weights<Deconv>(h, wei, bia, scales); }
int dfx_deconv_submit(dfx_deconv_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s) { return weighted_submit<Deconv>(h, src_dev, dst_dev, s); }
int dfx_deconv_submit_host(dfx_deconv_t *h, const void *src_host, void *dst_host) { return weighted_submit_host<Deconv>(h, src_host, dst_host); }
int dfx_deconv_query(const dfx_deconv_t *h, dfx_deconv_info *info) { return weighted_query<Deconv>(h, info); }
int dfx_debug_deconv_requant(const dfx_deconv_t *h, int32_t out[1]) { return weighted_requant<Deconv>(h, out); }
int dfx_deconv_destroy(dfx_deconv_t *h) {
  weighted_release(h);
  return DFX_OK;
}

}  // extern "C"
