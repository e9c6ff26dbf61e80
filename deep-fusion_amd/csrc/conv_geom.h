// conv_geom.h -- plain C++, no HIP: what the host-side planner of the conv op (conv_plan.h) and the conv kernels share: the
// geometry structs the kernels take as arguments (their field order, types and #ifdef members ARE the kernel-argument
// layouts) and the constants that size workgroups and LDS.  Each kernel's header (conv_mfma.cuh, conv_mfma_roles.cuh,
// conv_stream.cuh, conv_direct.cuh, conv_pw.cuh, conv_generic.hip) includes it and explains what the fields mean to it.
#pragma once

#ifdef __HIPCC__
#define DFX_GEOM_HD __host__ __device__
#else
#define DFX_GEOM_HD
#endif

namespace dfx {

// ---- conv_mfma.cuh: the resident-weight kernel
constexpr int MFMA_THREADS = 1024;  // 16 waves: 14 compute + 2 loaders (waves 7 and 15)
constexpr int MFMA_TEAMS = 2;       // loader waves = unit streams per CU
constexpr int MFMA_NB = 4;          // input-tile ring slots in LDS (2 per loader)
#ifndef DFX_STAMPS
constexpr int MFMA_CTRL_BYTES = 128; // LDS control block, see CTL_* in conv_mfma.cuh
#else
constexpr int MFMA_CTRL_BYTES = 128 + 16 * 8 * 4; // + the stamps build's per-wave cycle sums ([16 waves][8] ints)
#endif
constexpr int MFMA_LC = 22;         // 16-byte chunks the loader wave holds per lane (88 VGPRs)

// Constant area (floats): per conv0 channel A0 | B0 | C0, per 1x1 channel A1 | B1 | C1 (see emit_pair).
// The B and C of the STORING stage (stage 1 of a fused op, stage 0 of an unfused one) are kept as
// PAIRS {k, k}: v_pk_add_f32 / v_pk_mul_f32 then take them as plain 64-bit operands.  Broadcasting
// one 32-bit constant with op_sel instead is not safe on this hardware: the form that takes the HIGH
// half of a source pair for the low lane (op_sel:[0,1]) returned wrong low results in the last 16
// lanes of a wave about once per 1e4 epilogue executions (tools/probe/probe_pk_opsel.hip reproduces it
// in isolation; the form op_sel_hi:[1,0] and scalar arithmetic never did).
DFX_GEOM_HD constexpr int mfma_cst_floats(int oc, int oc1) { return oc1 ? 3 * oc + 5 * oc1 : 5 * oc; }

// requant start values (see conv_mfma.cuh's header): bit patterns the accumulators start from
constexpr int MAGIC0_BITS = 0x4B400000;   // 1.5 * 2^23: ulp 1, room for +-2^22
constexpr int MAGIC1_BITS = 0x3E22F983;   // 1/(2*pi), an inline constant: ulp 2^-26, mantissa 0x22F983
constexpr int MAGIC1_LO = -0x22F983;      // most negative / positive integer it can absorb
constexpr int MAGIC1_HI = 0x7FFFFF - 0x22F983;

struct MfmaGeom {  // unit decomposition chosen by the host (conv_plan.h: pick_geometry, plan_handout)
  int th, tw;      // unit size in output rows / columns
  int uy, ux;      // units per image along y / x
  int linear;      // 1: tw == ow, pixels of a unit are numbered linearly across rows
                   // 0: tw % 32 == 0, every 32-pixel tile lies inside one row
  int total_units;
  int row_chunks;   // (tw + 2) * (ic / 16)
  int tile_chunks;  // (th + 2) * row_chunks
  unsigned row_magic;  // ceil(2^32 / row_chunks): q / row_chunks == umulhi(q, row_magic)
  unsigned tw_magic;   // ceil(2^32 / tw)
  unsigned upi_magic, ux_magic;  // ceil(2^32 / (uy * ux)), ceil(2^32 / ux); 0 where the divisor is 1
  int ntu;             // tile claims per unit = tiles of a full unit
  unsigned ntu_magic;  // ceil(2^32 / ntu) (unused when ntu == 1)
  int claim_limit;     // ntu * (total_units + 4): no CU can legitimately claim more tiles
  int mode0, mode1;    // requant mode of stage 0 / stage 1: 0 exact, 1 fast, 2 magic (see header)
  int s0_uniform;      // fused op with ONE conv0 scale (count 1, op_conv.cc:311-313): s0_value, no per-channel reads
  float s0_value;
  int tile_stride;     // bytes between the MFMA_NB input-tile slots in LDS
  int static_rounds;   // units a loader owns statically before it turns to the queue
  int pool;            // unfused ops only: 1 = 2x2 stride-2 max pooling fused into the store stage.  Units are
                       // full-width row groups (th even); a tile is 2 rows x 16 columns, so that a pooling
                       // window is accumulator registers e, e+1, e+8, e+9 of one lane; dst has oh/2 x ow/2 pixels
  int lazy_queue;      // 1: a loader draws its next unit only when the slot for it is free (store-bound ops)
  int half_from;       // unit ids >= half_from denote HALF units (th / 2 rows): id half_from + 2 i + j is half j of unit
                       // half_from + i; total_units counts them.  INT_MAX: none.  The tail of a store-bound op: the
                       // queue's granule is what a workgroup still holds when the queue runs dry (conv_plan.h)
  int upx;             // > 0: PIXEL-RUN units (conv_mfma.cuh only; store-bound ops whose row units end in a partial tile).
                       // Unit u of an image is its pixels [u * upx, min((u + 1) * upx, oh * ow)) in row-major order, upx a
                       // multiple of 32: every tile is full except the last of an image.  linear == 1, tw == ow, ux == 1,
                       // uy = units per image, ntu = upx / 32, no half units; th = the most output rows a run touches,
                       // ceil((ow - 1 + upx) / ow): the halo tile is always th + 2 full-width rows from the run's first row
                       // and the run's start column travels in the unit record.  0: row / column units as above
  int *queue;          // [0] next unit, [1] finished loaders; both 0 between launches
#ifdef DFX_STAMPS
  unsigned long long *prof;  // diagnostic build only: [workgroup][wave][16] cycle sums
#endif
#ifdef DFX_TRACE
  int *trace;  // diagnostic build only (make trace): host-visible [workgroup][wave][4] progress words
#endif
};

// ---- conv_mfma_roles.cuh: the role-specialised resident kernel
constexpr int RL_CTRL_BYTES = 512;                   // control block: the words of conv_mfma.cuh + the mid ring's
#ifndef RL_NA
#define RL_NA 6
#endif
#ifndef RL_NB
#define RL_NB 8
#endif
constexpr int RL_A = RL_NA;                          // conv0 waves
constexpr int RL_B = RL_NB;                          // conv1 + store waves
constexpr int RL_C = RL_A + RL_B;                    // waves that stage the weights
constexpr int RL_WAVES = RL_C + MFMA_TEAMS;          // + 2 loaders
constexpr int RL_THREADS = 64 * RL_WAVES;            // 1024
constexpr int MAGIC3_BITS = 0x4B000000;              // 2^23: stage-0 accumulator start of the "fma" mode

// ---- conv_stream.cuh: the streamed-weight kernel
constexpr int ST_THREADS = 256;
constexpr int ST_M = 128;  // pixel slots per unit and PXB
constexpr int ST_POS = 64;  // LDS bytes per halo-tile position (16-byte chunks XOR-swizzled by position)
constexpr int ST_STAGE = 32 * 144;  // per wave: 32 pixels x 128 output bytes (+16 pad), 1-byte outputs;
                                   // the four staging areas alias the input tile (dead during the 1x1 stage)

struct StreamGeom {
  int ni, thv, twv;     // unit = ni whole images (ni > 1 only if thv == oh && twv == ow) x thv x twv px
  int uy, ux;           // units per image (group) along y / x
  int total_units;
  int lh, lw, npos;     // halo tile rows / cols per image; LDS positions = ni * lh * lw
  int n_icc;            // 64-channel input chunks
  int icb;              // 32-channel input blocks (ic rounded up)
  int n_occ;            // conv0 output chunks of OCC blocks
  int ocb;              // = n_occ * OCC: padded conv0 output blocks
  int n_g1, ks2;        // conv1: groups of G column blocks; k-steps (pairs of oc blocks)
  int s0_steps;         // conv0 steps per unit
  int mid_stride;       // bytes per slot of the intermediate (32 * ocb + 16)
  int off_tile, off_pxoff, off_mid, off_cst, off_stage;  // LDS byte offsets (weight buffers at 0)
  int fast;             // 1: the fast requant path is valid (host proof, see conv_mfma.cuh store_group)
  int planes;           // 1: one 64-channel input chunk in LDS at a time; n_icc: all chunks resident (staged once per item)
  unsigned mg_g4, mg_lhw, mg_lw;  // ceil(2^32 / x) for x = 4 * planes, lh * lw, lw (resident-chunk staging)
  int occ_par;          // unfused only: 1 = a work item is (unit, output chunk) instead of a whole unit
#ifdef DFX_STAMPS
  unsigned long long *prof;  // diagnostic build only: [workgroup][wave][16] cycle sums
#endif
};

// ---- conv_direct.cuh: the direct-weight kernel
constexpr int DK_POS = 80;   // LDS bytes per halo-tile position and plane (64 + 16 pad)
constexpr int DK_STAGE = 32 * 144;  // per wave: 1-byte store staging (aliases the dead tile)

struct DirectGeom {
  int ni, thv, twv;     // unit = ni whole images (ni > 1 only if thv == oh && twv == ow) x thv x twv px
  int uy, ux, total_units;
  int lh, lw, npos;     // halo tile rows / cols per image; positions = ni * lh * lw
  int icb;              // 32-channel input blocks
  int n_planes;         // 64-channel planes of the tile = (icb + 1) / 2
  int plane_bytes;      // ni * img_pitch
  // byte pitches of the tile: position (img, ly, lx) of a plane sits at img * img_pitch + ly * row_pitch + lx *
  // DK_POS.  row_pitch = lw * DK_POS + 16 c, img_pitch = lh * row_pitch + 16 c': the host picks c, c' (0..15) so
  // that the 16 lanes of every ds_read_b128 lane group of a pixel fragment fall into 16 different 16-byte bank
  // columns.  (With the plain pitches consecutive slots of one output row are conflict-free -- DK_POS is 5 x 16 --
  // but a 32-slot block wraps over 2-5 output rows and the row gap broke the pattern: 47 % of the LDS cycles at
  // res4 were bank conflicts, profiles/r03/final pmc.)
  int row_pitch, img_pitch;
  // unfused != 0: no 1x1 stage (oc1x1 == 0).  conv0's requantised result IS the output: 4-byte outputs are stored
  // straight from the accumulators (a lane holds 4 consecutive channels of its pixel per q: one 16-byte store),
  // 1-byte outputs are collected in `mid` in natural channel order and leave as whole pixel rows (16-byte stores).
  int unfused;
  int ocb;              // conv0 output blocks, padded to a multiple of WO
  int n_g1;             // conv1 groups of G column blocks
  int mid_stride;       // 32 * ocb + 16
  int off_pxoff, off_mid, off_cst;  // LDS byte offsets (tile and the aliased staging at 0)
  int fast;             // 1: fast requant path valid (host proof)
  int m0, m1;           // host-proven requant without conversions: m0 = 1 stage-0 "fma"; m1 = 2 / 3 stage-1 "magic" / "fma"
  int npb;              // 32-pixel blocks per unit (1, 2 or 4)
#ifdef DFX_STAMPS
  unsigned long long *prof;  // diagnostic build only: [workgroup][wave][16] cycle sums
#endif
#ifdef DK_DEBUG
  // bounds-checking diagnostic build: every global access is checked against these sizes; the
  // first violation per tag is recorded in dbg[2 tag] (offset) / dbg[2 tag + 1] (size) and the
  // access is redirected to offset 0
  long long src_bytes, dst_bytes, wei_bytes, wei1_bytes, cst_bytes;
  long long *dbg;
#endif
};

// ---- conv_pw.cuh: the pointwise kernel
constexpr int PW_THREADS = 256;

struct PwGeom {
  int icb, ocb;      // 32-channel blocks
  int px_total;      // bs * oh * ow (< 2^31 / ic: byte offsets of pixel rows stay in 32 bits per lane pair ... see host)
  int n_blocks;      // ceil(px_total / 32)
  int off_cst;       // LDS byte offset of the constants (behind the weights)
  int off_stage;     // ... of the waves' store staging (behind the constants), stage_bytes per wave
  int stage_bytes;
  int fast, m0;      // host proofs: fast requant route valid; stage-0 "fma" route (u8 dst)
};

// ---- conv_generic.hip: the scalar kernel
constexpr int GEN_TP = 32;       // pixels per workgroup
constexpr int GEN_THREADS = 256;

}  // namespace dfx
