// patchembed_plan.h -- host-only, plain C++: what the int8 patch-embedding op (dfx_patchembed_* of include/dfx.h) decides
// before a kernel runs: the descriptor's validation in the order the header documents, the tile kernel's class (its granule),
// the auto rule, the GEMM the op is (linear_plan.h's descriptor: rows = bs * th * tw, k = ph * pw * ic, n = oc), from which
// the tile height, the tile count, the grids and the LDS size follow by linear_plan.h's own rules, the sections of the device
// image, the K offset table and the algorithmic counts.  No HIP in here, so that it can be built and run on its own
// (tools/patchembed_plan_check.cc, under the host sanitizers).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "linear_plan.h"
#include "plan_common.h"

namespace dfx {

constexpr long long PE_MAX_ELEMS = 1ll << 40;     // bs * ih * iw * ic and bs * img_rows * dst_ld
constexpr size_t PE_TABLE_MAX_BYTES = (size_t)1 << 30;

inline long long pe_tokens(const dfx_patchembed_desc &d) { return (long long)d.th * d.tw; }  // per image
inline long long pe_rows(const dfx_patchembed_desc &d) { return (long long)d.bs * pe_tokens(d); }
inline int pe_run(const dfx_patchembed_desc &d) { return d.pw * d.ic; }                      // L: contiguous bytes of a patch row
inline int pe_k(const dfx_patchembed_desc &d) { return d.ph * d.pw * d.ic; }
inline bool pe_relu(const dfx_patchembed_desc &d) { return d.relu != 0 || d.dst_dt == DFX_U8; }
inline int pe_table_ld(int oc) { return (int)(((long long)oc + 3) / 4 * 4); }                 // floats per row of the table's image

// the granule of the tile kernel's loads: 16, 4, or 0 outside its class (the alignment of src is checked per submit)
inline int pe_granule(const dfx_patchembed_desc &d) {
  const long long l = (long long)d.pw * d.ic, row = (long long)d.iw * d.ic;
  if (l % 16 == 0 && row % 16 == 0) return 16;
  if (l % 4 == 0 && row % 4 == 0) return 4;
  return 0;
}
inline bool pe_tile_class(const dfx_patchembed_desc &d) { return pe_granule(d) != 0; }

// DFX_OK, or the code dfx_patchembed_create returns with *why set to the reason.  Everything DFX_ERR_INVALID is found before
// the one DFX_ERR_UNSUPPORTED.
inline int pe_validate(const dfx_patchembed_desc &d, const char **why) {
  const char *dummy;
  if (!why) why = &dummy;
  *why = "";
  if (d.bs < 1 || d.ih < 1 || d.iw < 1 || d.ic < 1) return *why = "bs, ih, iw, ic below 1", DFX_ERR_INVALID;
  if (d.ph < 1 || d.ph > 255 || d.pw < 1 || d.pw > 255) return *why = "ph, pw must lie in 1 .. 255", DFX_ERR_INVALID;
  if (d.th < 1 || d.th > d.ih / d.ph) return *why = "th must lie in 1 .. ih / ph", DFX_ERR_INVALID;
  if (d.tw < 1 || d.tw > d.iw / d.pw) return *why = "tw must lie in 1 .. iw / pw", DFX_ERR_INVALID;
  if ((long long)d.ph * d.pw * d.ic > LIN_KMAX) return *why = "ph * pw * ic beyond 65025 (the accumulator could leave s32)", DFX_ERR_INVALID;
  if (d.oc < 1 || d.oc > LIN_NMAX) return *why = "oc must lie in 1 .. 2^31 - 128", DFX_ERR_INVALID;
  if (d.src_dt != DFX_U8 && d.src_dt != DFX_S8) return *why = "bad src dtype (u8 or s8)", DFX_ERR_INVALID;
  if (!lin_dt_ok(d.dst_dt)) return *why = "bad dst dtype", DFX_ERR_INVALID;
  if (d.bia_dt != DFX_UNDEF && !lin_dt_ok(d.bia_dt)) return *why = "bad bias dtype", DFX_ERR_INVALID;
  if (d.round_mode != DFX_ROUND_NEAREST && d.round_mode != DFX_ROUND_DOWN) return *why = "bad round mode", DFX_ERR_INVALID;
  if (d.nscales != 1 && d.nscales != d.oc) return *why = "scales count must be 1 or oc", DFX_ERR_INVALID;
  if (d.table != 0 && d.table != 1) return *why = "table must be 0 or 1", DFX_ERR_INVALID;
  if (d.table && d.bia_dt != DFX_UNDEF) return *why = "a table and a bias (fold the bias into the table)", DFX_ERR_INVALID;
  if (d.tok_offset < 0) return *why = "tok_offset below 0", DFX_ERR_INVALID;
  if (d.force_path != -1 && d.force_path != DFX_PATCHEMBED_TILE && d.force_path != DFX_PATCHEMBED_GENERIC) return *why = "bad force_path", DFX_ERR_INVALID;
  if (d.img_rows < (long long)d.tok_offset + pe_tokens(d)) return *why = "img_rows below tok_offset + th * tw", DFX_ERR_INVALID;
  if (d.dst_ld < d.oc) return *why = "dst_ld below oc", DFX_ERR_INVALID;
  if ((unsigned __int128)d.bs * (unsigned __int128)d.ih * (unsigned __int128)((long long)d.iw * d.ic) > (unsigned __int128)PE_MAX_ELEMS)
    return *why = "bs * ih * iw * ic beyond 2^40", DFX_ERR_INVALID;
  if ((long long)d.ph * ((long long)d.iw * d.ic) >= (1ll << 31)) return *why = "ph * iw * ic reaches 2^31 (a patch's byte offsets leave s32)", DFX_ERR_INVALID;
  if ((unsigned __int128)d.bs * (unsigned __int128)d.img_rows * (unsigned __int128)d.dst_ld > (unsigned __int128)PE_MAX_ELEMS)
    return *why = "bs * img_rows * dst_ld beyond 2^40", DFX_ERR_INVALID;
  if (d.table && (unsigned __int128)pe_tokens(d) * (unsigned)pe_table_ld(d.oc) * 4 > (unsigned __int128)PE_TABLE_MAX_BYTES)
    return *why = "the table's device image {th * tw, up4(oc)} f32 exceeds 2^30 bytes", DFX_ERR_INVALID;
  if (d.force_path == DFX_PATCHEMBED_TILE && !pe_tile_class(d))
    return *why = "descriptor outside the tile kernel's class (pw * ic and iw * ic multiples of 4)", DFX_ERR_UNSUPPORTED;
  return DFX_OK;
}

// AUTO RULE (include/dfx.h DFX_PATCHEMBED_AUTO_NOTE, DESIGN.md section 4.25, measured in profiles/patchembed/): the tile kernel in its
// class from the smallest of each size at which tools/bench_patchembed timed it and it beat both the generic kernel and dfx_imgconv
// on auto on the same image: rows >= 49 (ViT-B/32 bs 1), oc >= 96 and K >= 48 (the Swin-T stem) and 3136 * 96 * 48 multiply-adds
// (the Swin-T stem at bs 1).  It won at all 21 measured points, by 2.3x at the least; nothing smaller was timed, so everything
// smaller stays generic and reaches the tile kernel with force_path.
constexpr long long PE_AUTO_MIN_ROWS = 49, PE_AUTO_MIN_MACS = 3136ll * 96 * 48;
constexpr int PE_AUTO_MIN_OC = 96, PE_AUTO_MIN_K = 48;
inline bool pe_tile_auto(const dfx_patchembed_desc &d) {
  if (pe_rows(d) < PE_AUTO_MIN_ROWS || d.oc < PE_AUTO_MIN_OC || pe_k(d) < PE_AUTO_MIN_K) return false;
  return (unsigned __int128)pe_rows(d) * (unsigned __int128)((long long)d.oc * pe_k(d)) >= (unsigned __int128)PE_AUTO_MIN_MACS;
}
inline int pe_path(const dfx_patchembed_desc &d) {
  if (d.force_path != -1) return d.force_path;
  return pe_tile_class(d) && pe_tile_auto(d) ? DFX_PATCHEMBED_TILE : DFX_PATCHEMBED_GENERIC;
}

// The GEMM the op is, as linear_plan.h's descriptor: lin_bm, lin_tiles, lin_mtiles, lin_grid, lin_lds_bytes, lin_image and
// linear_pack.h's lin_pack take it as it is.  bias_f32: the packer is handed an f32 vector (the bias converted, or the
// table's per-channel maximum for the route's proof).
inline dfx_linear_desc pe_gemm(const dfx_patchembed_desc &d, bool bias_f32) {
  dfx_linear_desc g;
  g.rows = pe_rows(d);
  g.k = pe_k(d);
  g.n = d.oc;
  g.src_dt = d.src_dt;
  g.dst_dt = d.dst_dt;
  g.bia_dt = bias_f32 ? (int32_t)DFX_F32 : d.bia_dt;
  g.relu = d.relu;
  g.round_mode = d.round_mode;
  g.nscales = d.nscales;
  g.lut_in_dt = DFX_UNDEF;
  g.force_path = d.force_path;
  g.src_ld = g.k;
  g.dst_ld = d.dst_ld;
  return g;
}
inline int pe_bm(const dfx_patchembed_desc &d, int cus, int forced) { return lin_bm(pe_gemm(d, false), cus, forced); }
inline int pe_grid(const dfx_patchembed_desc &d, int path, int bm, int cus, long long cap) { return lin_grid(pe_gemm(d, false), path, bm, cus, cap); }
// tile kernel: linear_plan.h's LDS plan without the byte table
inline int pe_lds_bytes(int path, int bm) { return path == DFX_PATCHEMBED_TILE ? lin_lds_bytes(DFX_LINEAR_TILE, bm) - 256 : 0; }

// The K offset table: entry g is the byte offset, from a patch's first byte, of granule g of its K bytes in the order
// (ky, kx, i): (g G / L) * iw * ic + (g G % L), L = pw * ic.  In the class L % G == 0, so no granule straddles two runs.  It
// has an entry for every granule of the slabs (entries at or beyond K are 0 and never used).  Outside the class G = 1 would
// be the only granule; the generic kernel walks the runs itself and the table is empty.
inline size_t pe_ktab_entries(const dfx_patchembed_desc &d) {
  const int g = pe_granule(d);
  return g ? (size_t)lin_nslabs(pe_k(d)) * (size_t)(LIN_KS / g) : 0;
}
inline void pe_fill_ktab(const dfx_patchembed_desc &d, int32_t *tab) {
  const int g = pe_granule(d), l = pe_run(d), k = pe_k(d);
  const size_t n = pe_ktab_entries(d);
  const long long row = (long long)d.iw * d.ic;
  for (size_t e = 0; e < n; ++e) {
    const long long c = (long long)e * g;
    tab[e] = c < k ? (int32_t)((c / l) * row + c % l) : 0;
  }
}

// The device image: linear_pack.h's image up to its table section (packed weights | comp | bias | scale) | K offset table |
// token table {th * tw, up4(oc)} f32 | prefix rows {tok_offset, oc} of dst's dtype.  Every section starts at a multiple of 16.
struct PeImage {
  LinImage lin;
  size_t off_ktab, off_table, off_prefix, bytes;
};
inline PeImage pe_image(const dfx_patchembed_desc &d) {
  PeImage im;
  im.lin = lin_image(d.oc, pe_k(d));
  im.off_ktab = im.lin.off_table;
  im.off_table = im.off_ktab + plan_up16(pe_ktab_entries(d) * 4);
  im.off_prefix = im.off_table + (d.table ? (size_t)pe_tokens(d) * (size_t)pe_table_ld(d.oc) * 4 : 0);
  im.bytes = im.off_prefix + plan_up16((size_t)d.tok_offset * (size_t)d.oc * (size_t)plan_dt_size(d.dst_dt));
  if (im.bytes == 0) im.bytes = 16;
  return im;
}

inline unsigned long long pe_algorithmic_ops(const dfx_patchembed_desc &d) {
  return 2ull * (unsigned long long)pe_rows(d) * (unsigned long long)d.oc * (unsigned long long)pe_k(d);
}
inline unsigned long long pe_algorithmic_bytes(const dfx_patchembed_desc &d, bool prefix) {
  const unsigned esz = (unsigned)plan_dt_size(d.dst_dt);
  return (unsigned long long)pe_rows(d) * pe_k(d) + (unsigned long long)d.oc * pe_k(d) + (unsigned long long)pe_rows(d) * d.oc * esz +
         (d.table ? 4ull * pe_tokens(d) * d.oc : d.bia_dt != DFX_UNDEF ? 4ull * d.oc : 0) + 4ull * d.nscales +
         (prefix ? (unsigned long long)d.bs * d.tok_offset * d.oc * esz : 0);
}

// bytes from an operand's first to one past its last byte the op may touch
inline unsigned long long pe_src_extent(const dfx_patchembed_desc &d) {
  return (unsigned long long)d.bs * d.ih * ((unsigned long long)d.iw * d.ic);
}
inline unsigned long long pe_dst_extent(const dfx_patchembed_desc &d) {
  const unsigned long long last = (unsigned long long)(d.bs - 1) * d.img_rows + d.tok_offset + pe_tokens(d) - 1;  // the last token's row
  return (last * d.dst_ld + d.oc) * (unsigned)plan_dt_size(d.dst_dt);
}

}  // namespace dfx
