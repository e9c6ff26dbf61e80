// conv_plan.h -- host-only, plain C++: everything dfx_conv_create decides before it allocates anything: the descriptor's
// validation, the kernel family (resident / role-specialised / streamed / direct / pointwise / scalar), each family's unit
// geometry and LDS layout, the candidate search of the direct kernel, the unit hand-out of the resident kernel, grid, block
// and the kernel's name.  What comes from outside arrives in a ConvEnv: the CU count, the tuning switches and the answer
// to "how many workgroups of this kernel fit a CU".  No HIP in here, so that it can be built, run, dumped and diffed on
// its own (tools/conv_plan_check.cc, under the host sanitizers; tests/golden/conv_plans.json holds recorded plans).
#pragma once

#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <initializer_list>
#include <vector>

#include "../../include/dfx.h"
#include "conv_geom.h"
#include "requant_host.h"

namespace dfx {

struct ConvPlan {
  int variant;
  MfmaGeom geom;
  StreamGeom sgeom;  // DFX_VARIANT_MFMA_STREAM
  DirectGeom dgeom;  // DFX_VARIANT_MFMA_STREAM served by conv_direct.cuh (fused ops): direct != 0
  int direct, nw, wo, wo1;
  int pw;            // DFX_VARIANT_MFMA_STREAM served by conv_pw.cuh (pointwise unfused): direct != 0 too (weights packed as for conv_direct.cuh)
  PwGeom pwgeom;
  int occ, pxb;      // stream variant: conv0 output blocks per chunk, pixel blocks per wave
  int icb, ocb, G, grid, block, lds;
  // role-specialised fused kernel (conv_mfma_roles.cuh): roles_ok = the SHAPE fits it (LDS is then sized for its larger
  // control block); whether the WEIGHTS allow its requant modes is dfx_conv_set_weights' business
  bool roles_ok;
  int rows_per_unit, units_per_image;  // what ConvArgs carries of the plan
  char kernel_name[96];
};

typedef const char *(*ConvTune)(const char *key);

// the only facts planning takes from outside
struct ConvEnv {
  int ncu;         // compute units of the device
  ConvTune tune;   // value of a testing / tuning switch or nullptr
  // Workgroups per CU of the kernel `p` names so far (variant, direct / pw, block and the template parameters), at p.lds
  // bytes of LDS.  The library answers with the launchers' mode 2 after mode 1 has raised the LDS limit.  < 1 counts as 1.
  int (*wg_per_cu)(void *ctx, const ConvPlan &p);
  void *ctx;
};

inline size_t conv_dt_size(int dt) { return (dt == DFX_F32 || dt == DFX_S32) ? 4 : 1; }

// DFX_OK, or the code dfx_conv_create returns with *why set to the message
inline int conv_validate(const dfx_conv_desc &d, const char **why) {
  const char *dummy;
  if (!why) why = &dummy;
  *why = "";
  auto is_dt = [](int v) { return v >= DFX_F32 && v <= DFX_U8; };
  if (d.bs <= 0 || d.ic <= 0 || d.oc <= 0 || d.ih <= 0 || d.iw <= 0 || d.kh <= 0 || d.kw <= 0 ||
      d.sh <= 0 || d.sw <= 0 || d.pad_t < 0 || d.pad_l < 0 || d.oc1x1 < 0)
    return *why = "conv: non-positive dimension", DFX_ERR_INVALID;
  if (!is_dt(d.dst_dt)) return *why = "conv: bad dst dtype", DFX_ERR_INVALID;  // jit_conv_kernel.cc:536-540
  if (d.bia0_dt != DFX_UNDEF && !is_dt(d.bia0_dt)) return *why = "conv: bad bias dtype", DFX_ERR_INVALID;
  if (d.bia1_dt != DFX_UNDEF && !is_dt(d.bia1_dt)) return *why = "conv: bad bias1x1 dtype", DFX_ERR_INVALID;
  if (d.ic % 16 || d.oc % 16)  // jit_conv_kernel.cc:590-592
    return *why = "conv: ic and oc must be multiples of 16", DFX_ERR_INVALID;
  if (d.oh != (d.ih + 2 * d.pad_t - d.kh) / d.sh + 1 || d.ow != (d.iw + 2 * d.pad_l - d.kw) / d.sw + 1 ||
      d.oh <= 0 || d.ow <= 0)  // op_conv.cc:290-297
    return *why = "conv: output image size do not match", DFX_ERR_INVALID;
  if (d.conv0_nscales != 1 && d.conv0_nscales != d.oc)  // op_conv.cc:311-313, :342-345
    return *why = "conv: conv0 scales count must be 1 or oc", DFX_ERR_INVALID;
  if (d.oc1x1) {
    if (d.oc1x1 % 16) return *why = "conv: oc1x1 must be a multiple of 16", DFX_ERR_INVALID;  // :619-621
    if (d.conv1_nscales != 1 && d.conv1_nscales != d.oc1x1)
      return *why = "conv: conv1 scales count must be 1 or oc1x1", DFX_ERR_INVALID;
  }
  if (d.conv0_round_mode < 0 || d.conv0_round_mode > 1 || d.conv1_round_mode < 0 || d.conv1_round_mode > 1)
    return *why = "conv: bad round mode", DFX_ERR_INVALID;
  return DFX_OK;
}

// output bytes per pixel from which an op counts as bound by its output stream (finer units, lazy queue)
inline size_t store_bound_bytes(ConvTune tune) {
  if (const char *e = tune("DFX_STORE_BOUND_BYTES")) return (size_t)std::max(1, atoi(e));  // tuning aid
  return 512;
}

inline bool mfma_eligible(const dfx_conv_desc &d) {  // fused or unfused (oc1x1 == 0)
  if ((long long)d.bs * d.oh * d.ow >= (1LL << 31) - 64) return false;  // (pixel indices are 32-bit in the kernel)
  return d.kh == 3 && d.kw == 3 && d.sh == 1 && d.sw == 1 && d.pad_t <= 1 && d.pad_l <= 1 &&
         (d.ic == 32 || d.ic == 64) && (d.oc == 32 || d.oc == 64) && d.oc1x1 % 32 == 0;
}

// the role-specialised kernel (conv_mfma_roles.cuh): fused, 1-byte output, output channels in groups of 128 (<= 4)
inline bool roles_eligible(const dfx_conv_desc &d, ConvTune tune) {
  if (tune("DFX_NO_ROLES") && atoi(tune("DFX_NO_ROLES")) != 0) return false;  // testing aid: conv_mfma.cuh's kernel
  // (this IS the list of shapes the library can launch: it must mirror DFX_FOR_EACH_ROLES_SHAPE in
  //  conv_mfma_roles_inst.inc: with oc = 64 only oc1x1 <= 256 is built -- admitting 384 / 512 here made dfx_conv_create
  //  fail for those ops, found by profiles/debug/soak_resident.py)
  return mfma_eligible(d) && d.oc1x1 > 0 && !d.fuse_pool && (d.dst_dt == DFX_U8 || d.dst_dt == DFX_S8) &&
         d.oc1x1 % 128 == 0 && d.oc1x1 / 128 <= (d.oc == 64 ? 2 : 4);
}

// pixels per pixel-run unit of a store-bound op (0: row units), see pick_geometry; DFX_UNIT_PX overrides it.
// Chosen by measurement on the s32 headline (profiles/ab_unit_px.txt): runs of 96 pixels -- three full tiles, 33
// units per 56 x 56 image, 5 halo rows -- 75.8 us against 78.1 us for 2-row units; 128 (4 tiles, 6 halo rows) 78.1,
// 160 80.2: the lazy queue's granule and the halo rows a loader stages per unit weigh more than the tile count.
constexpr int kDefaultUnitPx = 96;

// Pick the unit decomposition of the MFMA variant: TH output rows x TW output
// columns per unit, either full-width rows (linear pixel numbering) or TW a
// multiple of 32.  Scored by how full a unit's 32-pixel tiles are (tiles rotate over
// the compute waves, so the tile count per unit need not match the wave count), how
// little halo it re-reads, whether the loader wave can hold the whole halo tile in
// registers, and -- for HBM-bound outputs -- how fine the dynamic hand-out is.
// false if nothing fits LDS.
inline bool pick_geometry(const dfx_conv_desc &d, ConvTune tune, MfmaGeom &g, int &lds, int ctrl_bytes = MFMA_CTRL_BYTES) {
  const int ICB = d.ic / 32, OCB = d.oc / 32, NCB = d.oc1x1 / 32;
  const size_t fixed = (size_t)OCB * 9 * ICB * 1024 + (size_t)NCB * OCB * 1024 +
                       round16((size_t)mfma_cst_floats(d.oc, d.oc1x1) * 4) + (size_t)ctrl_bytes;
  const size_t lds_max = 163840;  // one workgroup per CU owns the whole LDS
  if (fixed + 4 * 1024 > lds_max) return false;
  const size_t tile_max = (lds_max - fixed) / MFMA_NB;  // ring of MFMA_NB tile slots
  // rows per unit wanted for parallelism: aim for >= ~3 units per team (512 teams)
  int th_par = (int)(((long long)d.bs * d.oh) / 1536);
  if (th_par < 1) th_par = 1;
  if (th_par < 2 && (long long)d.bs * d.oh / 2 >= 512) th_par = 2;
  if (th_par > 16) th_par = 16;
  if (const char *e = tune("DFX_MAX_TH")) th_par = std::max(1, std::min(th_par, atoi(e)));  // tuning aid
  const bool hbm_bound_dst = d.dst_dt == DFX_S32 || d.dst_dt == DFX_F32;
  double best = -1.0;
  for (int mode = 0; mode < 2; ++mode)
    for (int tw = (mode == 0 ? d.ow : 32); tw <= (mode == 0 ? d.ow : std::min(d.ow, 256)); tw += 32) {
      if (mode == 1 && tw >= d.ow) break;  // full width is mode 0
      for (int th = 1; th <= std::min(d.oh, th_par); ++th) {
        // a tile slot holds whole 1 KB pieces (64 granules of 16 bytes: one write per loader lane) + a dump piece
        const size_t tile = ((size_t)(th + 2) * (tw + 2) * (d.ic / 16) + 63) / 64 * 1024 + 1024;
        if (tile > tile_max) break;
        const int npx = th * tw;
        const int ntiles = mode == 0 ? (npx + 31) / 32 : th * (tw / 32);
        const double px_eff = (double)npx / (32.0 * ntiles);
        const double halo_eff = (double)npx / ((th + 2.0) * (tw + 2.0));
        // edge units are partial: fraction of the covered area that is real output
        const double cover = ((double)d.oh * d.ow) /
                             ((double)((d.oh + th - 1) / th * th) * ((d.ow + tw - 1) / tw * tw));
        const bool oversize = (tile - 1024) / 16 > (size_t)64 * MFMA_LC;
        double score = px_eff * cover * (0.75 + 0.25 * halo_eff) * (oversize ? 0.9 : 1.0);
        // The 14 compute waves of a CU claim tiles from the units in the 4-slot LDS ring: a unit should
        // bring >= 7 tiles so that two units in flight keep every wave busy while two more are staged
        // (measured at config 3, s32: 2-row units of 4 tiles 124 us, 4-row units of 7 tiles 97 us)
        const bool store_bound = hbm_bound_dst && (size_t)(d.oc1x1 > 0 ? d.oc1x1 : d.oc) * 4 >= store_bound_bytes(tune);
        score *= 0.5 + 0.5 * std::min(1.0, ntiles / (store_bound ? 4.0 : 7.0));
        // Store-bound ops (>= 512 output bytes per pixel): workgroups drain at very different rates and
        // the lazy queue (conv_mfma.cuh) can only even that out with enough units per loader -- >= 6
        // (s32 headline, same box: 2-row units / 7 per loader 84.1 us, 4-row units / 3.5 per loader 86.5 us)
        if (store_bound) {
          if (mode == 1) score *= 0.9;  // column-split units end in partial tiles (the slower store form)
          const double units = (double)d.bs * ((d.oh + th - 1) / th) * ((d.ow + tw - 1) / tw);
          score *= 0.5 + 0.5 * std::min(1.0, units / (6.0 * 512.0));
        }
        if (score > best) {
          best = score;
          g.th = th; g.tw = tw; g.linear = mode == 0;
        }
      }
    }
  if (best < 0) return false;
  if (const char *e = tune("DFX_FORCE_GEOM")) {  // tuning aid: "th,tw" (must fit LDS)
    int fth = 0, ftw = 0;
    if (sscanf(e, "%d,%d", &fth, &ftw) == 2 && fth >= 1 && (ftw == d.ow || (ftw % 32 == 0 && ftw < d.ow)) &&
        ((size_t)(fth + 2) * (ftw + 2) * (d.ic / 16) + 63) / 64 * 1024 + 1024 <= tile_max) {
      g.th = fth; g.tw = ftw; g.linear = ftw == d.ow;
    }
  }
  g.pool = d.fuse_pool ? 1 : 0;
  if (g.pool) {
    // pooled ops: the scored unit (full-width rows, or a 32-multiple of columns) with an even number of rows
    // (a tile is 2 rows x 16 columns): the largest even th <= the scored one whose tile fits, at least 2
    auto tile_of = [&](int th, int tw) { return ((size_t)(th + 2) * (tw + 2) * (d.ic / 16) + 63) / 64 * 1024 + 1024; };
    int th = std::max(2, g.th & ~1);
    while (th > 2 && tile_of(th, g.tw) > tile_max) th -= 2;
    if (tile_of(th, g.tw) > tile_max) {  // rows of this width do not fit even in pairs: split the columns
      g.tw = 32 * std::max(1, std::min(d.ow / 32, 4));
      g.linear = g.tw == d.ow;
      while (g.tw > 32 && tile_of(th, g.tw) > tile_max) g.tw -= 32;
      if (tile_of(th, g.tw) > tile_max) return false;
    }
    g.th = th;
  }
  // Pixel-run units (MfmaGeom::upx): a unit is a run of U consecutive pixels of one image in
  // row-major order, U a multiple of 32, instead of th whole rows.  Every 32-pixel tile is then full except the last
  // one of an image (2-row units of a 56-wide image are 3.5 tiles: every fourth tile ran its MFMAs and requant
  // arithmetic for 16 pixels nobody stores).  For store-bound ops whose row units end in a partial tile; never with
  // fused pooling, a forced geometry, or a shape the role-specialised kernel could take (conv_mfma_roles.cuh has
  // no decode for these units, and which kernel runs is only known once the weights are -- see half_from below).
  // A unit that starts anywhere in a row touches at most rmax = ceil((ow - 1 + U) / ow) output rows; its halo tile
  // is always rmax + 2 full-width rows, which must fit a ring slot and -- for the default rule, a matter of speed --
  // the loader's registers (no oversize path; a forced U may take it: write_rest decodes these units like any other).
  // The fields below are reported as th = rmax, tw = ow, uy = units per image, ux = 1.
  g.upx = 0;
  {
    const bool store_bound = hbm_bound_dst && (size_t)(d.oc1x1 > 0 ? d.oc1x1 : d.oc) * 4 >= store_bound_bytes(tune);
    int U = store_bound ? kDefaultUnitPx : 0;
    bool forced = false;
    if (const char *e = tune("DFX_UNIT_PX")) {  // tuning aid: 0 = off, N = U wherever it is legal (store-bound or not)
      U = atoi(e);
      forced = true;
    }
    const long long opx = (long long)d.oh * d.ow;
    // (U < 2^15: the unit record packs pixels << 16; opx * ow < 2^31: pixel / ow by multiply-high with tw_magic)
    if (U >= 32 && U % 32 == 0 && U < 32768 && g.linear && (g.th * g.tw) % 32 != 0 && !g.pool && !roles_eligible(d, tune) &&
        !tune("DFX_FORCE_GEOM") && d.ow >= 2 && d.ow < 65536 && opx * d.ow < (1LL << 31)) {
      const int rmax = (d.ow - 1 + U + d.ow - 1) / d.ow;
      const size_t chunks = (size_t)(rmax + 2) * (d.ow + 2) * (d.ic / 16);
      if ((chunks + 63) / 64 * 1024 + 1024 <= tile_max && (forced || chunks <= (size_t)64 * MFMA_LC)) {
        g.upx = U;
        g.th = rmax;
        g.tw = d.ow;
      }
    }
  }
  g.uy = g.upx ? (int)(((long long)d.oh * d.ow + g.upx - 1) / g.upx) : (d.oh + g.th - 1) / g.th;
  g.ux = (d.ow + g.tw - 1) / g.tw;
  g.total_units = d.bs * g.uy * g.ux;
  g.row_chunks = (g.tw + 2) * (d.ic / 16);
  g.tile_chunks = (g.th + 2) * g.row_chunks;
  g.row_magic = (unsigned)(((1ull << 32) + g.row_chunks - 1) / g.row_chunks);
  g.tile_stride = (g.tile_chunks + 63) / 64 * 1024 + 1024;  // + the loader's dump piece
  g.tw_magic = (unsigned)(((1ull << 32) + g.tw - 1) / g.tw);
  g.upi_magic = g.uy * g.ux > 1 ? (unsigned)(((1ull << 32) + g.uy * g.ux - 1) / (g.uy * g.ux)) : 0u;
  g.ux_magic = g.ux > 1 ? (unsigned)(((1ull << 32) + g.ux - 1) / g.ux) : 0u;
  g.ntu = g.pool ? (g.th / 2) * ((g.tw + 15) / 16)
          : g.upx ? g.upx / 32
                  : g.linear ? (g.th * g.tw + 31) / 32 : g.th * (g.tw / 32);  // tile claims per unit
  g.ntu_magic = (unsigned)(((1ull << 32) + g.ntu - 1) / g.ntu);
  g.claim_limit = (int)std::min<long long>(0x7ffffff0LL, (long long)g.ntu * ((long long)g.total_units + 4));
  lds = (int)(fixed + (size_t)MFMA_NB * g.tile_stride);
  return true;
}

// ---- direct-weight fused kernel (conv_direct.cuh) ----
inline bool pick_direct_geometry(const dfx_conv_desc &d, int NW, int WO, int G, int npb, DirectGeom &g, int &lds) {
  const int M = 32 * npb;  // pixel slots per unit
  g.npb = npb;
  g.m0 = g.m1 = 0;
  const int ocb_real = (d.oc + 31) / 32;
  g.icb = (d.ic + 31) / 32;
  g.n_planes = (g.icb + 1) / 2;
  if (g.n_planes > 16) return false;  // (plane index 0..15: 4 bits in the staging table)
  g.ocb = (ocb_real + WO - 1) / WO * WO;
  g.n_g1 = ((d.oc1x1 + 31) / 32 + G - 1) / G;
  g.mid_stride = 32 * g.ocb + 16;
  const size_t cst_bytes = round16((size_t)3 * 32 * (g.ocb + G * g.n_g1) * 4);  // both stages' constants
  const size_t stage_bytes = (G == 4 && conv_dt_size(d.dst_dt) == 1) ? (size_t)NW * DK_STAGE : 0;
  // (`mid`: the u8 intermediate / the 1-byte output rows; an unfused op with 4-byte output stages 32 px x 128 B per wave there)
  const size_t mid_bytes = std::max((size_t)M * g.mid_stride, (d.oc1x1 == 0 && conv_dt_size(d.dst_dt) == 4) ? (size_t)NW * 32 * 144 : (size_t)0);
  const size_t fixed = 8 * M + mid_bytes + cst_bytes;  // (8 M: the slot tables pxoff and fboff)
  const size_t lds_max = 163840;
  g.unfused = d.oc1x1 == 0 ? 1 : 0;
  if ((long long)d.bs * d.oh * d.ow * (d.oc1x1 ? d.oc1x1 : d.oc) * (long long)conv_dt_size(d.dst_dt) >= (1LL << 32) - 16 ||
      (long long)d.bs * d.oh * d.ow >= (1LL << 31) || (long long)d.ih * d.iw * d.ic * M >= (1LL << 31))
    return false;
  double best = -1.0;
  auto consider = [&](int ni, int thv, int twv) {
    const int lh = (thv - 1) * d.sh + d.kh, lw = (twv - 1) * d.sw + d.kw;
    if (lh >= 1024 || lw >= 1024 || ni >= 256) return;
    const long long npos = (long long)ni * lh * lw;
    // (+ 240 bytes per row and per image: the bank-spreading pads of the pitches, chosen below)
    const size_t tile = std::max((size_t)((long long)g.n_planes * ni * ((long long)lh * (lw * DK_POS + 240) + 240) + 16), stage_bytes);
    if (fixed + tile > lds_max) return;
    const double groups = (double)((d.bs + ni - 1) / ni);
    const double units = groups * ((d.oh + thv - 1) / thv) * ((d.ow + twv - 1) / twv);
    const double util = (double)d.bs * d.oh * d.ow / (units * M);
    const double halo = (double)thv * d.sh * twv * d.sw / ((double)lh * lw);
    const double two = fixed + tile <= 81920 ? 1.0 : 0.8;  // two workgroups per CU
    const double score = util * (0.8 + 0.2 * std::min(1.0, halo)) * two;
    if (score > best) {
      best = score;
      g.ni = ni; g.thv = thv; g.twv = twv; g.lh = lh; g.lw = lw; g.npos = (int)npos;
    }
  };
  if (d.oh * d.ow <= M) {
    for (int ni = std::min(d.bs, M / (d.oh * d.ow)); ni >= 1; --ni) consider(ni, d.oh, d.ow);
  } else {
    for (int twv = 1; twv <= std::min(d.ow, M); ++twv) consider(1, std::min(d.oh, M / twv), twv);
  }
  if (best < 0) return false;
  g.uy = (d.oh + g.thv - 1) / g.thv;
  g.ux = (d.ow + g.twv - 1) / g.twv;
  g.total_units = (d.bs + g.ni - 1) / g.ni * g.uy * g.ux;
  // Pitches: 16 c / 16 c' bytes of padding per tile row / image so that the 16 lanes of each ds_read_b128 lane
  // group ({0-3,12-15,20-27}, {4-11,16-19,28-31} of either half wave) read 16 different 16-byte bank columns --
  // brute force over c, c', cost = extra LDS cycles summed over the unit's pixel blocks (0 = conflict-free).
  {
    const int px_img = g.thv * g.twv, npx = g.ni * px_img;
    static const int grp[2][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                   {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31}};
    long long best_cost = -1;
    int best_c = 0, best_ci = 0;
    for (int ci = 0; ci < (g.ni > 1 ? 16 : 1); ++ci)
      for (int c = 0; c < 16; ++c) {
        const long long rp = (long long)g.lw * DK_POS + 16 * c, ip = (long long)g.lh * rp + 16 * ci;
        long long cost = 0;
        for (int b = 0; b < npb; ++b)
          for (int gi = 0; gi < 2; ++gi) {
            int cnt[16] = {0};
            long long seen[16][16];
            for (int k = 0; k < 16; ++k) {
              const int pc = std::min(32 * b + grp[gi][k], npx - 1);
              const int img = pc / px_img, r = pc % px_img, ty = r / g.twv, tx = r % g.twv;
              const long long addr = img * ip + (long long)ty * d.sh * rp + (long long)tx * d.sw * DK_POS;
              const int col = (int)((addr / 16) % 16);
              bool dup = false;  // identical addresses broadcast
              for (int j = 0; j < cnt[col]; ++j) dup = dup || seen[col][j] == addr;
              if (!dup) seen[col][cnt[col]++] = addr;
            }
            int worst = 1;
            for (int k = 0; k < 16; ++k) worst = std::max(worst, cnt[k]);
            cost += worst - 1;
          }
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best_c = c; best_ci = ci; }
      }
    g.row_pitch = g.lw * DK_POS + 16 * best_c;
    g.img_pitch = g.lh * g.row_pitch + 16 * best_ci;
  }
  g.plane_bytes = g.ni * g.img_pitch;
  g.off_pxoff = (int)round16(std::max((size_t)g.n_planes * (size_t)g.plane_bytes + 16, stage_bytes));
  g.off_mid = g.off_pxoff + 8 * M;
  g.off_cst = g.off_mid + (int)round16(mid_bytes);
  lds = g.off_cst + (int)cst_bytes;
  g.fast = 0;
  return true;
}

// ---- streamed-weight variant (conv_stream.cuh) ----
// blocks per chunk / group: the largest of {4,2,1} that pads the block count by <= 1/3
inline int pick_blocking(int nblocks) {
  for (int x : {4, 2, 1}) {
    const int padded = (nblocks + x - 1) / x * x;
    if (3 * padded <= 4 * nblocks) return x;
  }
  return 1;
}

// chunk_par: the op will hand out (unit, output chunk) items (one output chunk per item)
inline bool pick_stream_geometry(const dfx_conv_desc &d, ConvTune tune, int OCC, int G, int PXB, bool chunk_par, StreamGeom &g,
                                 int &lds) {
  const int M = ST_M * PXB;  // pixel slots per unit
  const bool fused = d.oc1x1 > 0;
  const int icb = (d.ic + 31) / 32, ocb_real = (d.oc + 31) / 32;
  g.icb = icb;
  g.n_icc = (icb + 1) / 2;
  g.n_occ = (ocb_real + OCC - 1) / OCC;
  g.ocb = g.n_occ * OCC;
  g.n_g1 = fused ? ((d.oc1x1 + 31) / 32 + G - 1) / G : 0;
  g.ks2 = (g.ocb + 1) / 2;
  g.mid_stride = 32 * g.ocb + 16;
  int s0 = 0;
  for (int c = 0; c < g.n_icc; ++c) s0 += (d.kh * d.kw * std::min(2, icb - 2 * c) + 1) / 2;
  g.s0_steps = s0 * g.n_occ;
  const int WB = fused ? std::max(OCC, G) : OCC;
  const size_t cst_bytes = fused ? round16((size_t)3 * 32 * g.ocb * 4) : 0;
  // 1-byte store staging, 4 waves (fused: 4-block groups; unfused: chunks of >= 2 blocks)
  const size_t stage_bytes = (conv_dt_size(d.dst_dt) == 1 && (fused ? G == 4 : OCC >= 2)) ? (size_t)4 * ST_STAGE : 0;
  const size_t fixed = (size_t)3 * 2 * WB * 1024 + 4 * M + (fused ? (size_t)M * g.mid_stride : 0) + cst_bytes;
  const size_t lds_max = 163840;
  // index ranges the kernel keeps in 32 bits / packed fields
  // (dst byte offsets are 32-bit in the kernel's pixel table)
  if ((long long)d.bs * d.oh * d.ow * (d.oc1x1 ? d.oc1x1 : d.oc) * (long long)conv_dt_size(d.dst_dt) >= (1LL << 32) - 16 ||
      (long long)d.bs * d.oh * d.ow >= (1LL << 31) || (long long)d.ih * d.iw * d.ic * M >= (1LL << 31)) return false;
  double best = -1.0;
  auto consider = [&](int ni, int thv, int twv) {
    const int lh = (thv - 1) * d.sh + d.kh, lw = (twv - 1) * d.sw + d.kw;
    if (lh >= 1024 || lw >= 1024) return;
    const long long npos = (long long)ni * lh * lw;
    if (fixed + std::max((size_t)npos * ST_POS + 16, stage_bytes) > lds_max) return;
    const double groups = (double)((d.bs + ni - 1) / ni);
    const double units = groups * ((d.oh + thv - 1) / thv) * ((d.ow + twv - 1) / twv);
    const double util = (double)d.bs * d.oh * d.ow / (units * M);           // filled pixel slots
    const double halo = (double)thv * d.sh * twv * d.sw / ((double)lh * lw);  // input re-read
    const double score = util * (0.8 + 0.2 * std::min(1.0, halo));
    if (score > best) {
      best = score;
      g.ni = ni; g.thv = thv; g.twv = twv; g.lh = lh; g.lw = lw; g.npos = (int)npos;
    }
  };
  if (d.oh * d.ow <= M) {
    for (int ni = std::min(d.bs, M / (d.oh * d.ow)); ni >= 1; --ni) consider(ni, d.oh, d.ow);
  } else {
    for (int twv = 1; twv <= std::min(d.ow, M); ++twv) consider(1, std::min(d.oh, M / twv), twv);
  }
  if (best < 0) return false;
  g.uy = (d.oh + g.thv - 1) / g.thv;
  g.ux = (d.ow + g.twv - 1) / g.twv;
  g.total_units = (d.bs + g.ni - 1) / g.ni * g.uy * g.ux;
  g.off_tile = 3 * 2 * WB * 1024;  // three weight buffers
  // All input chunks resident in LDS (staged once per work item, without register prefetch)
  // instead of one chunk at a time (prefetched): pays when a work item would otherwise stage
  // every chunk once per output chunk, or when a chunk has too few steps to hide the next
  // fetch (1x1 kernels) -- if that still leaves room for two workgroups per CU.
  g.planes = 1;
  const bool restaged = !chunk_par && g.n_occ > 1;
  const bool short_chunks = d.kh * d.kw <= 2;
  if (g.n_icc > 1 && (restaged || short_chunks) &&
      fixed + std::max((size_t)g.n_icc * g.npos * ST_POS + 16, stage_bytes) <= 81920)
    g.planes = g.n_icc;
  if (const char *e = tune("DFX_STREAM_PLANES"))  // testing aid: 0 = never, 1 = whenever it fits LDS at all
    g.planes = (atoi(e) && g.n_icc > 1 && fixed + std::max((size_t)g.n_icc * g.npos * ST_POS + 16, stage_bytes) <= lds_max) ? g.n_icc : 1;
  {
    auto magic = [](long long x) { return (unsigned)(((1ull << 32) + (unsigned long long)x - 1) / (unsigned long long)x); };
    g.mg_g4 = magic(4 * g.planes); g.mg_lhw = magic((long long)g.lh * g.lw); g.mg_lw = magic(g.lw);
  }
  // +16: the staging dump slot; the 1-byte store staging areas alias the tile
  g.off_pxoff = (int)round16((size_t)g.off_tile + std::max((size_t)g.planes * g.npos * ST_POS + 16, stage_bytes));
  g.off_mid = g.off_pxoff + 4 * M;
  g.off_cst = g.off_mid + (fused ? M * g.mid_stride : 0);
  g.off_stage = g.off_tile;
  lds = g.off_cst + (int)cst_bytes;
  return true;
}

// conv_stream.cuh's blocking, pixel blocks per wave and geometry; false where no unit of it fits the shape
inline bool plan_stream(const dfx_conv_desc &d, const ConvEnv &env, ConvPlan *p) {
  const ConvTune tune = env.tune;
  p->occ = pick_blocking((d.oc + 31) / 32);
  p->G = d.oc1x1 ? pick_blocking((d.oc1x1 + 31) / 32) : p->occ;
  if (const char *e = tune("DFX_STREAM_BLOCKING")) {  // tuning aid: "occ,g" from {1,2,4}
    int o = 0, gg = 0;
    if (sscanf(e, "%d,%d", &o, &gg) == 2 && (o == 1 || o == 2 || o == 4) && (gg == 1 || gg == 2 || gg == 4)) {
      p->occ = o;
      p->G = d.oc1x1 ? gg : o;
    }
  }
  // Two pixel blocks per wave halve the LDS fragment traffic per MFMA but double the unit:
  // taken when the units still fill the machine twice over and two workgroups still share a CU.
  p->pxb = 2;
  if (const char *e = tune("DFX_STREAM_PXB")) p->pxb = atoi(e) == 1 ? 1 : 2;  // tuning aid
  bool ok = p->pxb == 2 && pick_stream_geometry(d, tune, p->occ, p->G, 2, false, p->sgeom, p->lds) &&
            ((p->sgeom.total_units >= 4 * env.ncu && p->lds <= 81920) || tune("DFX_STREAM_PXB"));
  if (!ok) {
    p->pxb = 1;
    ok = pick_stream_geometry(d, tune, p->occ, p->G, 1, false, p->sgeom, p->lds);
  }
  return ok;
}

// conv_pw.cuh: no unit geometry, the weights' LDS image and a staging area per wave
inline void plan_pw(const dfx_conv_desc &d, ConvPlan *p) {
  memset(&p->dgeom, 0, sizeof(p->dgeom));
  p->dgeom.icb = d.ic / 32;
  p->dgeom.ocb = d.oc / 32;
  p->dgeom.n_g1 = 0;
  p->dgeom.unfused = 1;
  p->dgeom.npb = 1;
  p->G = 4;
  p->pw = 1;
  p->direct = 1;
  p->nw = PW_THREADS / 64;
  p->pwgeom.icb = p->dgeom.icb;
  p->pwgeom.ocb = p->dgeom.ocb;
  p->pwgeom.px_total = d.bs * d.oh * d.ow;
  p->pwgeom.n_blocks = (p->pwgeom.px_total + 31) / 32;
  p->pwgeom.off_cst = d.oc * d.ic;
  p->pwgeom.fast = p->pwgeom.m0 = 0;
  p->pwgeom.off_stage = (int)round16((size_t)d.oc * d.ic + (size_t)3 * d.oc * 4);
  p->pwgeom.stage_bytes = (int)round16(conv_dt_size(d.dst_dt) == 1 ? (size_t)32 * (d.oc + 16) : (size_t)32 * 144);
  p->lds = p->pwgeom.off_stage + p->nw * p->pwgeom.stage_bytes;
  p->dgeom.total_units = (p->pwgeom.n_blocks + p->nw - 1) / p->nw;  // (workgroups' worth of blocks: the grid's upper bound)
  p->dgeom.thv = 0; p->dgeom.uy = p->dgeom.ux = 1;
}

// conv_direct.cuh: the candidate search; leaves p->direct == 0 where no instance takes the shape
inline void plan_direct(const dfx_conv_desc &d, const ConvEnv &env, bool direct_unfused, ConvPlan *p) {
  const ConvTune tune = env.tune;
  const int ocb2 = ((d.oc + 31) / 32 + 1) / 2 * 2;
  const int ncb1 = (d.oc1x1 + 31) / 32;
  const int G = direct_unfused ? 4 : (ncb1 >= 3 ? 4 : 2);  // (unfused: the instances with G = 4 and no 1x1 groups)
  // Pixel blocks per unit: the largest of 4, 2, 1 whose units still fill three quarters of the workgroup slots
  // (two per CU).  Smaller units re-stream the weights more often, larger ones leave CUs (res4: 196 units of
  // 128 pixels for 512 slots, res5: 64) or SIMDs empty.  With fewer than 4 blocks the four waves split the
  // output blocks of BOTH stages four ways (WO = WO1 = 4).  DFX_DIRECT_NPB forces one (testing aid).
  const int ncu2 = 2 * env.ncu;
  int forced = 0, forced_nw = 0, forced_wo1 = 0;
  if (const char *e = tune("DFX_DIRECT_NPB")) forced = atoi(e);
  if (const char *e = tune("DFX_DIRECT_NW")) forced_nw = atoi(e);
  if (const char *e = tune("DFX_DIRECT_WO1")) forced_wo1 = atoi(e);
  const int ocb_real = (d.oc + 31) / 32, n_g1 = (ncb1 + G - 1) / G;
  // candidates in order of preference (instances: conv_direct_inst.inc):
  //  * four waves, 128-pixel units, where those fill three quarters of the workgroup slots (two per CU);
  //  * eight waves (one workgroup per CU, two waves per SIMD, each weight byte fetched once or twice per
  //    unit) with the largest unit that still fills three quarters of the CUs;
  //  * four waves with smaller units.
  struct Cand { int nw, wo, wo1, npb, min_units; };
  std::vector<Cand> cands;
  const int wo4 = ocb2 % 4 == 0 ? 4 : 2;
  const int wo1_4 = (G == 4 && wo4 == 4 && n_g1 % 4 == 0 && !direct_unfused) ? 4 : 1;
  cands.push_back({4, wo4, wo1_4, 4, 3 * ncu2 / 4});
  if (wo1_4 == 4) cands.push_back({4, wo4, 1, 4, 3 * ncu2 / 4});
  if (G == 4 && ocb_real % 8 == 0) {
    // (a pointwise conv's units are short -- one tap -- and 64-pixel units measured better than 128: tried first)
    if (direct_unfused && d.kh * d.kw == 1) cands.push_back({8, 8, 8, 2, 3 * ncu2 / 8});
    for (int npb : {4, 2, 1}) cands.push_back({8, 8, 8, npb, npb == 1 ? 0 : 3 * ncu2 / 8});
  }
  for (int npb : {2, 1}) cands.push_back({4, 4, 4, npb, npb == 1 ? 0 : 3 * ncu2 / 4});
  // first pass: four-wave candidates must also leave room for two workgroups per CU (80 KB of LDS each; a
  // stride-2 layer's 128-pixel halo tile does not: res3s2 72 us with 128-pixel units, 45 us with 64)
  // ... and every candidate must fill its pixel slots: where the LDS only admits a sliver of a patch (512 input
  // channels at 14 x 14: 14 x 3 pixels of a 128-slot unit) the next smaller unit is the better kernel (vgg5
  // unfused: 95 us with 128-slot units, 39 us with 64).  Passes: 0 = all rules, 1 = without the LDS rule,
  // 2 = anything that fits.
  for (int pass = 0; pass < 3 && !p->direct; ++pass)
    for (const Cand &c : cands) {
      if (forced && c.npb != forced) continue;
      if (forced_nw && c.nw != forced_nw) continue;
      if (forced_wo1 && c.wo1 != forced_wo1) continue;
      DirectGeom dg;
      memset(&dg, 0, sizeof(dg));
      int lds = 0;
      if (!pick_direct_geometry(d, c.nw, c.wo, G, c.npb, dg, lds)) continue;
      if (!forced && dg.total_units < c.min_units) continue;  // too few units: try the next candidate
      if (!forced && pass == 0 && c.nw == 4 && lds > 81920) continue;
      const double util = (double)d.bs * d.oh * d.ow / ((double)dg.total_units * 32.0 * c.npb);
      if (!forced && pass < 2 && util < 0.7) continue;
      if (tune("DFX_DEBUG_PTRS"))
        fprintf(stderr, "[dfx] direct candidate nw%d wo%d wo1 %d npb%d: ni %d th %d tw %d units %d (min %d) lds %d pass %d\n", c.nw, c.wo, c.wo1,
                c.npb, dg.ni, dg.thv, dg.twv, dg.total_units, c.min_units, lds, pass);
      p->dgeom = dg;
      p->direct = 1;
      p->G = G;
      p->nw = c.nw;
      p->wo = c.wo;
      p->wo1 = c.wo1;
      p->lds = lds;
      break;
    }
}

// the resident kernel's unit hand-out (geom and grid are set): static rounds, lazy queue, half units
inline void plan_handout(const dfx_conv_desc &d, ConvTune tune, ConvPlan *p) {
  MfmaGeom &g = p->geom;
  const int teams = p->grid * MFMA_TEAMS;
  // Few units per loader (the headline block: 3.5): the queue's granularity -- a whole unit, half a
  // round of the 14 compute waves -- makes workgroups end up with 6..8 units and the slowest sets the
  // kernel time (measured spread of workgroup lifetimes: 30 %).  A static split (stream-major, see
  // stream_id in conv_mfma.cuh) gives every workgroup the same count +- 1 unit.  Many units per
  // loader: three static rounds, then the queue evens out speed differences between CUs.
  // (Also for the store-bound s32 headline, whose XCDs finish 40 % apart: static 82.5 us median,
  // two static rounds + queue 88.5 us, profiles/r02/ab_s32.txt.)
  const int rounds = (g.total_units + teams - 1) / teams;
  g.static_rounds = rounds <= 8 ? rounds : 3;
  // store-bound op (>= 512 output bytes per pixel): two static rounds (staged before the barrier),
  // then the queue with lazy draws -- see the loader in conv_mfma.cuh
  const size_t out_px_bytes = (size_t)(d.oc1x1 > 0 ? d.oc1x1 : d.oc) * conv_dt_size(d.dst_dt);
  g.lazy_queue = 0;
  if (out_px_bytes >= store_bound_bytes(tune) && rounds > 2 && !tune("DFX_NO_LAZY")) {
    g.lazy_queue = 1;
    g.static_rounds = 2;
  }
  if (const char *e = tune("DFX_STATIC_ROUNDS")) g.static_rounds = std::min(rounds, std::max(0, atoi(e)));  // tuning aid
  // Store-bound ops, the tail: a loader stream works through a unit in ~1/7 of the launch (headline: 10.7 us)
  // and a workgroup still holds up to four when the queue runs dry, so workgroups finish up to ~20 us apart
  // (stamps: a CU is idle 8.4 us = 10.5 % of the span before the kernel ends).  Handing out the last units as
  // two half units each (ids >= half_from, MfmaGeom::half_from: the same tiles, the same bytes, half the
  // granule) pays only where a HALF unit still brings >= 7 tiles for the 14 compute waves: VGG conv1_2 f32
  // (224-pixel rows) 325.5-325.9 us with the last 2048 units split against 327.2-328.6; the headline's
  // half units have 2 tiles and cost it 0.3 % (256 units split) to 13 % (2048): profiles/r03/ab_half_units.txt.
  // DFX_HALF_UNITS = number of units to split (0: none) overrides the rule.
  // Only conv_mfma.cuh decodes half-unit ids: conv_mfma_roles.cuh would take an id >= the real unit count for a
  // whole unit of an image behind the batch.  Which of the two kernels runs is decided by the weights
  // (dfx_conv_set_weights), after total_units is fixed, so every op whose SHAPE fits the role-specialised
  // kernel goes without half units, also where it later falls back to conv_mfma.cuh.
  g.half_from = 0x7fffffff;
  if (g.lazy_queue && !g.pool && g.th % 2 == 0 && !p->roles_ok && !g.upx) {  // (pixel-run units have no halves)
    const int half_tiles = g.linear ? ((g.th / 2) * g.tw + 31) / 32 : (g.th / 2) * (g.tw / 32);
    long long nh = half_tiles >= 7 ? 4LL * teams : 0;
    if (const char *e = tune("DFX_HALF_UNITS")) nh = std::max(0, atoi(e));
    nh = std::min<long long>(nh, (long long)g.total_units - (long long)(g.static_rounds + 1) * teams);
    if (nh > 0) {
      g.half_from = g.total_units - (int)nh;
      g.total_units += (int)nh;
      g.claim_limit = (int)std::min<long long>(0x7ffffff0LL, (long long)g.ntu * ((long long)g.total_units + 4));
    }
  }
}

// The plan of a validated descriptor into *p, which the caller has zeroed.  DFX_OK, or the code dfx_conv_create returns
// with *why set to the message.
inline int conv_plan(const dfx_conv_desc &d, const ConvEnv &env, ConvPlan *p, const char **why) {
  const ConvTune tune = env.tune;
  *why = "";
  bool want_mfma = mfma_eligible(d) && d.force_variant != DFX_VARIANT_GENERIC &&
                   d.force_variant != DFX_VARIANT_MFMA_STREAM;
  if (d.fuse_pool) {  // fused 2x2/2 max pooling: the resident-weight kernel's unfused form only
    if (d.fuse_pool != 2 || d.oc1x1 != 0 || !want_mfma || (d.oh & 1) || (d.ow & 1))
      return *why = "conv_create: fused pooling needs an unfused 3x3 stride-1 conv with 32/64 channels and even output size", DFX_ERR_UNSUPPORTED;
  }
  if ((d.force_variant == DFX_VARIANT_MFMA_FUSED || d.force_variant == DFX_VARIANT_MFMA_CONV) && !mfma_eligible(d))
    return *why = "conv_create: shape not covered by the MFMA variant", DFX_ERR_UNSUPPORTED;
  const bool want_stream = !want_mfma && d.force_variant != DFX_VARIANT_GENERIC;
  const bool stream_ok = want_stream && plan_stream(d, env, p);
  if (want_stream && !stream_ok && d.force_variant == DFX_VARIANT_MFMA_STREAM)
    return *why = "conv_create: shape does not fit the streamed MFMA variant", DFX_ERR_UNSUPPORTED;
  // The direct-weight kernel (conv_direct.cuh) serves fused ops with >= 64 channels on both sides wherever one of
  // its instances fits (N=128, u8 out, against conv_stream.cuh: res3 37 vs 50 us, res4 31 vs 53, res5 43 vs 79
  // in two launches, res3s2 45 vs 63: profiles/r03/direct_sweep_*.txt).  DFX_STREAM_DIRECT=0 turns it off.
  // Unfused ops (late round 3): the same kernel without its 1x1 stage (DirectGeom::unfused), for convs with a window
  // (kh * kw > 1) and >= 64 channels on both sides -- VGG conv3 / conv5-style layers.  Pointwise convs stay on
  // conv_stream.cuh (HBM-bound by their input; pw256 measured here 55 us against 42, profiles/r03/unfused_pointwise.txt).
  const bool direct_fused = d.oc1x1 > 0 && d.oc >= 64 && d.oc1x1 >= 64;
  // ... except deep ones whose weights do not fit conv_pw.cuh's LDS image (ic >= 512: res4 / res5 reduce convs, 1024 ->
  // 256 at 14 x 14: 26.8 us here against 31.3, profiles/r03/unfused_pointwise.txt).
  const bool direct_unfused = d.oc1x1 == 0 && d.oc >= 64 && d.ic >= 64 && (d.kh * d.kw > 1 || d.ic >= 512) && !d.fuse_pool;
  // Pointwise unfused convs whose weights fit LDS: conv_pw.cuh (pixel fragments straight from global memory into the
  // MFMA operands, no input tile).  DFX_STREAM_PW=0 turns it off (those shapes then run on conv_stream.cuh).
  bool want_pw = stream_ok && d.oc1x1 == 0 && d.kh == 1 && d.kw == 1 && d.sh == 1 && d.sw == 1 && d.pad_t == 0 && d.pad_l == 0 &&
                 !d.fuse_pool && d.ic % 256 == 0 && (d.oc == 64 || d.oc == 128 || d.oc == 256) && (long long)d.oc * d.ic <= 98304 &&
                 (long long)d.bs * d.oh * d.ow < (1LL << 31) - 64;
  if (const char *e = tune("DFX_STREAM_PW")) want_pw = want_pw && atoi(e) != 0;
  if (want_pw) plan_pw(d, p);
  bool want_direct = stream_ok && !p->pw && (direct_fused || direct_unfused);
  if (const char *e = tune("DFX_STREAM_DIRECT")) want_direct = want_direct && atoi(e) != 0;
  if (want_direct) plan_direct(d, env, direct_unfused, p);
  if (stream_ok) {  // conv_direct.cuh / conv_pw.cuh (direct != 0) or conv_stream.cuh
    p->variant = DFX_VARIANT_MFMA_STREAM;
    p->block = p->direct ? 64 * p->nw : ST_THREADS;
    int per_cu = env.wg_per_cu(env.ctx, *p);
    if (per_cu < 1) per_cu = 1;
    const int capacity = env.ncu * per_cu;  // resident workgroups
    int items = p->dgeom.total_units;
    if (!p->direct) {
      StreamGeom &sg = p->sgeom;
      // unfused op whose units leave workgroup slots empty: hand out (unit, output chunk) items
      sg.occ_par = (d.oc1x1 == 0 && sg.n_occ > 1 && sg.total_units < 2 * capacity) ? 1 : 0;
      if (const char *e = tune("DFX_STREAM_OCC_PAR")) sg.occ_par = (d.oc1x1 == 0 && sg.n_occ > 1 && atoi(e)) ? 1 : 0;  // testing aid
      if (sg.occ_par) {  // lay LDS out again for one output chunk per item (same units)
        const int units = sg.total_units;
        if (!pick_stream_geometry(d, tune, p->occ, p->G, p->pxb, true, sg, p->lds) || sg.total_units != units)
          return *why = "conv_create: internal: chunk-parallel layout failed", DFX_ERR_HIP;
        sg.occ_par = 1;
      }
      items = sg.total_units * (sg.occ_par ? sg.n_occ : 1);
    }
    p->grid = std::min(items, capacity);
    // (Until round 3 a fused op with too few units to fill the machine ran as two launches through an
    // intermediate in global memory; conv_direct.cuh's one-launch kernel replaced that path: res5 79 -> 43 us.)
    if (const char *e = tune("DFX_STREAM_GRID")) p->grid = std::max(1, std::min(p->grid, atoi(e)));  // testing aid
    p->rows_per_unit = p->direct ? p->dgeom.thv : p->sgeom.thv;
    p->units_per_image = p->direct ? p->dgeom.uy * p->dgeom.ux : p->sgeom.uy * p->sgeom.ux;
    if (p->pw)
      snprintf(p->kernel_name, sizeof(p->kernel_name), "conv_pw_kernel<%d,%d>", p->dgeom.ocb, d.dst_dt);
    else if (p->direct)
      snprintf(p->kernel_name, sizeof(p->kernel_name), "conv_direct_kernel<nw%d,%d,%d,%d,%d,%snpb%d>", p->nw, p->wo, p->G, p->wo1, d.dst_dt,
               p->dgeom.unfused ? "unfused," : "", p->dgeom.npb);
    else
      snprintf(p->kernel_name, sizeof(p->kernel_name), "conv_stream_kernel<%d,%d,%d,%d,%s%s>", p->occ, p->G, p->pxb,
               d.dst_dt, d.oc1x1 ? "fused" : "unfused", p->sgeom.occ_par ? ",occ_par" : "");
  } else if (d.fuse_pool && !(want_mfma && pick_geometry(d, tune, p->geom, p->lds))) {
    // (no other kernel knows about the pooled destination)
    return *why = "conv_create: no unit geometry of the resident-weight kernel fits fused pooling here", DFX_ERR_UNSUPPORTED;
  } else if (want_mfma && pick_geometry(d, tune, p->geom, p->lds, roles_eligible(d, tune) ? RL_CTRL_BYTES : MFMA_CTRL_BYTES)) {
    const bool fused = d.oc1x1 > 0;
    p->roles_ok = roles_eligible(d, tune);
    p->variant = fused ? DFX_VARIANT_MFMA_FUSED : DFX_VARIANT_MFMA_CONV;
    p->icb = d.ic / 32; p->ocb = d.oc / 32;
    const int ncb = d.oc1x1 / 32;
    p->G = fused ? ((ncb % 4 == 0) ? 4 : (ncb % 2 == 0 ? 2 : 1)) : p->ocb;
    p->grid = env.ncu;  // one persistent workgroup (two teams) per CU
    const int want = (p->geom.total_units + MFMA_TEAMS - 1) / MFMA_TEAMS;
    if (p->grid > want) p->grid = want;
    p->block = MFMA_THREADS;
    p->geom.mode0 = p->geom.mode1 = 0;
    plan_handout(d, tune, p);
    p->rows_per_unit = p->geom.th;
    p->units_per_image = p->geom.uy * p->geom.ux;
    snprintf(p->kernel_name, sizeof(p->kernel_name), "conv_mfma_fused_kernel<%d,%d,%d,%d%s>", p->icb,
             p->ocb, p->G, d.dst_dt, fused ? "" : ",unfused");
  } else {
    const long long total_px = (long long)d.bs * d.oh * d.ow;
    p->variant = DFX_VARIANT_GENERIC;
    p->block = GEN_THREADS;
    p->grid = (int)((total_px + GEN_TP - 1) / GEN_TP);
    p->lds = d.oc1x1 > 0 ? GEN_TP * d.oc : 0;
    p->rows_per_unit = 0;
    // The streamed- and direct-weight MFMA kernels hold dst offsets in 32 bits: an op whose dst reaches 4 GiB
    // runs on the scalar kernel, and its name says why (dfx_conv_query).
    const bool big_dst = total_px * (d.oc1x1 ? d.oc1x1 : d.oc) * (long long)conv_dt_size(d.dst_dt) >= (1LL << 32) - 16;
    snprintf(p->kernel_name, sizeof(p->kernel_name), "conv_generic_kernel<dt=%d>%s", d.dst_dt,
             big_dst && d.force_variant != DFX_VARIANT_GENERIC ? " [dst >= 4 GiB: no MFMA kernel (32-bit dst offsets)]" : "");
  }
  return DFX_OK;
}

}  // namespace dfx
