// dwconv_api.hip -- host side of the depthwise conv op (dfx_dwconv_* of include/dfx.h): descriptor validation, choice
// of the path and of the launch geometry, weight packing for the sliding-window kernel (dwconv.cuh), and the requant
// route's proof from the actual weights, bias and scales.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "dwconv.cuh"
#include "weighted_op.h"

namespace dfx {
int launch_dwconv_window(const DwArgs &, int grid, int block, int lds, hipStream_t);
int launch_dwconv_generic(const DwArgs &, int grid, hipStream_t);
}
using namespace dfx;

struct dfx_dwconv : WeightedHandle<dfx_dwconv_desc, DwArgs> {};

namespace {

struct Dwconv {  // the op's part of weighted_op.h's skeleton
  using H = dfx_dwconv;
  static constexpr const char *name = "dwconv", *channels_name = "c";
  static constexpr int FAST = DFX_DWCONV_WINDOW, GENERIC = DFX_DWCONV_GENERIC;
  static constexpr const char *class_text = "window kernel's class (3x3 or 5x5, stride 1 or 2, c % 16 == 0, one image below 2^31 bytes)";
  static constexpr bool raw_beside_packed = true;

  static int validate_shape(const dfx_dwconv_desc &d) {
    if (d.bs <= 0 || d.c <= 0 || d.ih <= 0 || d.iw <= 0 || d.oh <= 0 || d.ow <= 0)
      return fail(DFX_ERR_INVALID, "dwconv: non-positive dimension");
    if (d.kh <= 0 || d.kw <= 0 || d.kh > 255 || d.kw > 255)
      return fail(DFX_ERR_INVALID, "dwconv: window %d x %d outside 1 .. 255", d.kh, d.kw);
    if (d.sh <= 0 || d.sw <= 0) return fail(DFX_ERR_INVALID, "dwconv: non-positive stride");
    if (d.pad_t < 0 || d.pad_l < 0) return fail(DFX_ERR_INVALID, "dwconv: negative padding");
    if ((long long)(d.oh - 1) * d.sh - d.pad_t > d.ih - 1 || (long long)(d.ow - 1) * d.sw - d.pad_l > d.iw - 1)
      return fail(DFX_ERR_INVALID, "dwconv: the last output row / column's window starts outside the input");
    if ((long long)d.bs * d.ih * d.iw >= (1ll << 31) || (long long)d.bs * d.oh * d.ow >= (1ll << 31))
      return fail(DFX_ERR_INVALID, "dwconv: pixel count beyond 2^31");
    return DFX_OK;
  }

  // the shape class of dwconv.cuh
  static bool in_class(const dfx_dwconv_desc &d) {
    const long long lim = (1ll << 31) - 64;
    return d.kh == d.kw && (d.kh == 3 || d.kh == 5) && d.sh == d.sw && (d.sh == 1 || d.sh == 2) && d.c % 16 == 0 &&
           (long long)d.ih * d.iw * d.c < lim && (long long)d.oh * d.ow * d.c * (long long)dt_size(d.dst_dt) < lim;
  }

  static int channels(const dfx_dwconv_desc &d) { return d.c; }
  static size_t taps(const dfx_dwconv_desc &d) { return (size_t)d.kh * d.kw; }
  static size_t src_bytes(const dfx_dwconv_desc &d) { return (size_t)d.bs * d.ih * d.iw * d.c; }
  static size_t dst_elems(const dfx_dwconv_desc &d) { return (size_t)d.bs * d.oh * d.ow * d.c; }
  // [group][ky][dword of the row][channel of the group]: bytes = the row's taps kx = 4 * dword .. + 3, zero past K
  static size_t packed_bytes(const dfx_dwconv_desc &d) { return (size_t)(d.c / 16) * d.kh * (d.kh == 3 ? 1 : 2) * 16 * 4; }
  static int comp_count(const dfx_dwconv_desc &d) { return d.c; }
  static int const_count(const dfx_dwconv_desc &d) { return d.c; }
  static uint64_t algorithmic_ops(const dfx_dwconv_desc &d) { return 2 * (uint64_t)dst_elems(d) * d.kh * d.kw; }

  static void fill_args(const dfx_dwconv_desc &d, DwArgs &a) {
    a.bs = d.bs; a.c = d.c; a.ih = d.ih; a.iw = d.iw; a.oh = d.oh; a.ow = d.ow; a.kh = d.kh; a.kw = d.kw;
    a.sh = d.sh; a.sw = d.sw; a.pt = d.pad_t; a.pl = d.pad_l;
  }

  static int plan_fast(dfx_dwconv *h, int cus) {
    const dfx_dwconv_desc &d = h->d;
    DwArgs &a = h->args;
    a.groups = d.c / 16;
    // Launch: at most 4 workgroups of 256 lanes per CU (two are resident at the kernel's register count), lanes loop
    // over their work items.  Band: the output rows one lane slides over.  The K - S halo rows of a band are read
    // again by the band below, (K - S) / (band * S) of the input: 1/8 at 16 rows (3x3 stride 1), 1/4 at 8, 1/2 at
    // 4.  The largest band that still gives every lane of the launch a work item; 4 for tensors too small for that.
    const long long cap_blocks = (long long)cus * 4;
    int band = 16;
    while (band > 4 && (long long)d.bs * ((d.oh + band - 1) / band) * d.ow * a.groups < cap_blocks * DW_THREADS) band /= 2;
    if (const char *e = tuning_value("DFX_DWCONV_BAND")) band = std::max(1, std::min(atoi(e), 1 << 20));  // testing aid
    // (a band beyond oh is harmless: nbands is then 1, so the kernel's oy0 = band index * band is 0 and its nrows is
    // cut to oh - oy0; band itself never enters a product that could leave an int)
    a.band = band;
    a.nbands = (d.oh + band - 1) / band;
    a.items = (long long)d.bs * a.nbands * d.ow;
    // 5x5: weights and constants in LDS, one slot per channel group where a block's lanes share groups
    h->block = DW_THREADS;
    if (d.kh == 5) {
      a.slot_by_group = a.groups <= 64;
      if (!a.slot_by_group) h->block = 64;
      h->lds = DW_LDS_ROWS * (a.slot_by_group ? a.groups : 64) * 16;
    } else {
      h->lds = 0;
    }
    // lanes: one per (item, group) at most, a multiple of groups, at least one item's
    const long long lanes = a.items * a.groups;
    long long blocks = std::min((lanes + h->block - 1) / h->block, cap_blocks * (DW_THREADS / h->block));
    if (const char *e = tuning_value("DFX_DWCONV_GRID")) blocks = std::max(1ll, std::min(blocks, (long long)atoi(e)));  // testing aid
    blocks = std::max(blocks, ((long long)a.groups + h->block - 1) / h->block);
    h->grid = (int)blocks;
    a.threads = std::min(lanes, blocks * h->block / a.groups * a.groups);
    return DFX_OK;
  }

  static void pack(const dfx_dwconv *h, const int8_t *wei, unsigned char *img) {
    if (h->path != DFX_DWCONV_WINDOW) return;
    const dfx_dwconv_desc &d = h->d;
    const int K = d.kh, ndw = K == 3 ? 1 : 2;
    unsigned *wpk = (unsigned *)img;  // packed_bytes' layout
    for (int k = 0; k < d.c; ++k)
      for (int ky = 0; ky < K; ++ky)
        for (int j = 0; j < ndw; ++j) {
          unsigned v = 0;
          for (int b = 0; b < 4; ++b) {
            const int kx = 4 * j + b;
            if (kx < K) v |= (unsigned)(uint8_t)wei[((size_t)k * K + ky) * K + kx] << (8 * b);
          }
          wpk[(((size_t)(k / 16) * K + ky) * ndw + j) * 16 + k % 16] = v;
        }
  }

  static int check_ptrs(const dfx_dwconv *, const void *src, const void *dst) { return need_16_bytes<Dwconv>(src, dst); }

  static int launch(const dfx_dwconv *h, const DwArgs &a, hipStream_t st) {
    return launched<Dwconv>(h->path == DFX_DWCONV_WINDOW ? launch_dwconv_window(a, h->grid, h->block, h->lds, st)
                                                         : launch_dwconv_generic(a, h->grid, st));
  }

  static void set_name(dfx_dwconv *h) {
    const dfx_dwconv_desc &d = h->d;
    if (h->path == DFX_DWCONV_WINDOW)
      snprintf(h->kernel_name, sizeof(h->kernel_name), "dwconv_window<%dx%d,s%d,%s> band %d %s", d.kh, d.kw, d.sh,
               dt_name(d.dst_dt), h->args.band, !h->weights_set ? "(no weights)" : h->route ? "fast" : "exact");
    else
      snprintf(h->kernel_name, sizeof(h->kernel_name), "dwconv_generic<%dx%d,s%dx%d,%s> exact", d.kh, d.kw, d.sh, d.sw,
               dt_name(d.dst_dt));
  }
};

}  // namespace

bool dfx::dwconv_window_view(const dfx_dwconv *h, DwArgs *args) {  // (declared in dfx_internal.h)
  if (!h || h->path != DFX_DWCONV_WINDOW || !h->weights_set) return false;
  *args = h->args;
  return true;
}

extern "C" {

int dfx_dwconv_create(const dfx_dwconv_desc *desc, dfx_dwconv_t **out) { return weighted_create<Dwconv>(desc, out); }
int dfx_dwconv_set_weights(dfx_dwconv_t *h, const int8_t *wei, const void *bia, const float *scales) { return weighted_set_weights<Dwconv>(h, wei, bia, scales); }
int dfx_dwconv_submit(dfx_dwconv_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s) { return weighted_submit<Dwconv>(h, src_dev, dst_dev, s); }
int dfx_dwconv_submit_host(dfx_dwconv_t *h, const void *src_host, void *dst_host) { return weighted_submit_host<Dwconv>(h, src_host, dst_host); }
int dfx_dwconv_query(const dfx_dwconv_t *h, dfx_dwconv_info *info) { return weighted_query<Dwconv>(h, info); }
int dfx_debug_dwconv_requant(const dfx_dwconv_t *h, int32_t out[1]) { return weighted_requant<Dwconv>(h, out); }
int dfx_dwconv_destroy(dfx_dwconv_t *h) {
  weighted_release(h);
  return DFX_OK;
}

}  // extern "C"
