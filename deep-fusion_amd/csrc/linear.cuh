// linear.cuh -- the int8 token linear op's kernels (dfx_linear_* of include/dfx.h; gfx950): dst = requant(src . W^T) over a
// row matrix of u8 / s8 tokens and a weight image the host packed (linear_pack.h), one launch.
//
// linear_generic_kernel: one thread per dst element, grid-stride, any pitch and alignment, the exact route.  It reads the
// same packed image (lin_wei_offset restated) and defines the bits.
//
// linear_tile_kernel<BM>: v_mfma_i32_32x32x32_i8 on operands that are fetched from global memory ONCE per workgroup.
//   * 256 lanes = 4 waves own a BM x 128 tile of dst, BM in {128, 64}; wave w owns rows (w & 1) * BM / 2 .. and columns
//     (w >> 1) * 64 .. of it as BM / 64 x 2 accumulators of 32 x 32.  K runs in slabs of 64 (two MFMA steps).
//   * A slab of the weight block is 8 KB of the image, already in fragment order: the workgroup copies it to LDS with two
//     aligned 16-byte loads and stores per lane.  A slab of the tokens is BM rows x 4 pieces of 16 bytes: lane t loads
//     piece t & 3 of row t >> 2 (a row's 64 bytes by four adjacent lanes) and stores it in the SAME fragment order, piece p
//     of row r at ((r >> 5) * 4 + p) * 512 + (r & 31) * 16: a 32-row block's operand of step j is the 1 KB at
//     ((block * 2 + j) * 64 + lane) * 16.  Every fragment of either operand is one ds_read_b128 at lane * 16 from a 1 KB
//     aligned base: the 16 lanes of each of the instruction's lane groups cover the 16 slots of 16 bytes of the 256-byte
//     bank row once: no conflict.
//   * Two slab buffers, one barrier per slab: the slab's registers go to buffer ks & 1, barrier, the global loads of slab
//     ks + 1 are issued, then the slab's 8 (BM 64: 6) fragment reads and 8 (4) MFMAs run.  A writer of buffer b at slab
//     ks + 2 is behind the barrier of slab ks + 1, which every reader of slab ks has reached.
//   * Rows at or beyond `rows` load the last valid row (no address outside src is formed) and store nothing.  A piece that
//     starts at or beyond k is never loaded (zero); the piece k falls into is loaded whole -- it ends at most at k rounded
//     up to 16 <= src_ld -- and its tail meets the image's zero pad, whatever src's pad columns hold.  u8 tokens are stored
//     as a ^ 0x80; the compensation 128 * sum(w) comes from the image.
//   * N is on the MFMA's row operand (fc.cuh's lane map): a lane ends with 4 x 4 adjacent n of ITS row m per accumulator.
//     comp / bias / scale of the tile's 128 columns and the table are in LDS; a quad leaves as one dword (1-byte dst) or
//     one dfx_store16 (4-byte dst) where dst's alignment allows, element by element otherwise.
//   * Workgroups loop over tiles, m fastest inside an n-block, so the workgroups in flight share a weight block in L2.
#pragma once

#include "gconv.cuh"  // gc_mfma, gc_quarter

#include "linear_plan.h"

namespace dfx {

struct LinArgs {
  const unsigned char *src;
  unsigned char *dst;
  const unsigned char *wpk;  // linear_pack.h's weight section
  const int *comp;           // [nblocks * 128] 128 * sum of the channel's weights
  const float *bias;         // [nblocks * 128] f32 (0 without bias)
  const float *scale;        // [nblocks * 128] (a single scale is expanded by the host)
  const unsigned char *lut;  // 256 bytes, or nullptr
  long long rows, src_ld, dst_ld;
  int k, n, nks;
  int a_u8;                  // src is u8
  int req_dt;                // the type the requant produces: dst's, or the table's index type
  int lut_u8;                // the table is indexed by t (1) or by t + 128 (0)
  int relu, rm;
  int vec;                   // tile: 4 adjacent n leave as one store (dst and dst_ld allow it)
  long long mt, tiles;       // tile: m tiles per n-block, tiles in all
  long long items;           // generic: dst elements
};

// the four bytes of a packed dword through the table
__device__ __forceinline__ unsigned lin_lut4(const unsigned char *lut, unsigned pk, unsigned flip) {
  pk ^= flip;  // s8 index type: t + 128 is t ^ 0x80 on the byte
  return (unsigned)lut[pk & 0xffu] | ((unsigned)lut[(pk >> 8) & 0xffu] << 8) | ((unsigned)lut[(pk >> 16) & 0xffu] << 16) |
         ((unsigned)lut[pk >> 24] << 24);
}

// LDS: [2][BM * 64 tokens | 8 KB weights] | comp[128] | bias[128] | scale[128] | lut[256]   (lin_lds_bytes)
template <int BM, int DST, bool FAST>
__global__ __launch_bounds__(LIN_THREADS, 2) void linear_tile_kernel(LinArgs a) {
  constexpr int ESZ = (DST == DFX_F32 || DST == DFX_S32) ? 4 : 1;
  constexpr int MB = BM / 64;                     // 32-row blocks per wave
  constexpr int AP = BM * 4 / LIN_THREADS;        // token pieces per lane per slab
  constexpr int ABYTES = BM * LIN_KS, BUF = ABYTES + LIN_WBLOCK;
  extern __shared__ __attribute__((aligned(16))) unsigned char lin_lds[];
  int *const l_comp = reinterpret_cast<int *>(lin_lds + 2 * BUF);
  float *const l_bias = reinterpret_cast<float *>(l_comp + LIN_BN);
  float *const l_scale = l_bias + LIN_BN;
  unsigned char *const l_lut = reinterpret_cast<unsigned char *>(l_scale + LIN_BN);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, h = lane >> 5;
  const int wm = wave & 1, wn = wave >> 1;
  const v4i zero4 = v4i{0, 0, 0, 0};
  const int axor = a.a_u8 ? (int)0x80808080 : 0;
  const v4i x80 = v4i{axor, axor, axor, axor};
  const bool relu = a.relu != 0;
  const bool lut = a.lut != nullptr;  // (uniform)
  const unsigned flip = a.lut_u8 ? 0u : 0x80808080u;

  if (lut && tid < 16) reinterpret_cast<v4i *>(l_lut)[tid] = reinterpret_cast<const v4i *>(a.lut)[tid];  // behind the first barrier below

  for (long long t = blockIdx.x; t < a.tiles; t += gridDim.x) {  // uniform over the workgroup: so are the barriers
    const long long nb = t / a.mt, mi = t - nb * a.mt;
    const long long m0 = mi * BM;
    const int n0 = (int)nb * LIN_BN;
    if (tid < LIN_BN) {  // the tile's constants (the image has 128 entries per n-block)
      l_comp[tid] = a.comp[n0 + tid];
      l_bias[tid] = a.bias[n0 + tid];
      l_scale[tid] = a.scale[n0 + tid];
    }
    // this lane's token pieces: piece p of row `row`, clamped into src
    const unsigned char *arow[AP];
    int aoff[AP], apc[AP];
#pragma unroll
    for (int i = 0; i < AP; ++i) {
      const int pi = tid + LIN_THREADS * i, row = pi >> 2, p = pi & 3;
      const long long m = m0 + row < a.rows ? m0 + row : a.rows - 1;
      arow[i] = a.src + (size_t)m * (size_t)a.src_ld + 16 * p;
      aoff[i] = ((row >> 5) * 4 + p) * 512 + (row & 31) * 16;
      apc[i] = 16 * p;
    }
    const unsigned char *const wblk = a.wpk + (size_t)nb * (size_t)a.nks * LIN_WBLOCK + (size_t)tid * 16;

    v4i ra[AP], rb[2];
    auto load = [&](int ks) {
#pragma unroll
      for (int i = 0; i < AP; ++i) ra[i] = (LIN_KS * ks + apc[i] < a.k) ? *reinterpret_cast<const v4i *>(arow[i] + (size_t)LIN_KS * ks) : zero4;
#pragma unroll
      for (int i = 0; i < 2; ++i) rb[i] = *reinterpret_cast<const v4i *>(wblk + (size_t)ks * LIN_WBLOCK + (size_t)i * (LIN_THREADS * 16));
    };

    v16i acc[MB][2];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
      for (int nn = 0; nn < 2; ++nn)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[mb][nn][i] = 0;

    load(0);
    for (int ks = 0; ks < a.nks; ++ks) {
      unsigned char *const buf = lin_lds + (ks & 1) * BUF;
#pragma unroll
      for (int i = 0; i < AP; ++i) *reinterpret_cast<v4i *>(buf + aoff[i]) = ra[i] ^ x80;
#pragma unroll
      for (int i = 0; i < 2; ++i) *reinterpret_cast<v4i *>(buf + ABYTES + tid * 16 + i * (LIN_THREADS * 16)) = rb[i];
      __syncthreads();
      if (ks + 1 < a.nks) load(ks + 1);  // in flight under this slab's MFMAs
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        v4i fa[MB], fb[2];
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) fa[mb] = *reinterpret_cast<const v4i *>(buf + (((wm * MB + mb) * 2 + j) * 64 + lane) * 16);
#pragma unroll
        for (int nn = 0; nn < 2; ++nn) fb[nn] = *reinterpret_cast<const v4i *>(buf + ABYTES + (((wn * 2 + nn) * 2 + j) * 64 + lane) * 16);
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
          for (int nn = 0; nn < 2; ++nn) acc[mb][nn] = gc_mfma(fb[nn], fa[mb], acc[mb][nn]);  // D[n][m]
      }
    }

    // register 4 q + j of accumulator (mb, nn) is row m = .. + l31, column n = .. + 8 q + 4 h + j
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      const long long m = m0 + wm * (BM / 2) + mb * 32 + l31;
#pragma unroll
      for (int nn = 0; nn < 2; ++nn)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int nl = wn * 64 + nn * 32 + 8 * q + 4 * h;  // within the tile
          const int n = n0 + nl;
          if (m >= a.rows || n >= a.n) continue;
          int a4[4] = {acc[mb][nn][4 * q], acc[mb][nn][4 * q + 1], acc[mb][nn][4 * q + 2], acc[mb][nn][4 * q + 3]};
          if (a.a_u8) {  // (uniform)
            const v4i c4 = *reinterpret_cast<const v4i *>(l_comp + nl);
#pragma unroll
            for (int j = 0; j < 4; ++j) a4[j] += c4[j];
          }
          v4i out = gc_quarter<DST, FAST>(a4, *reinterpret_cast<const v4f *>(l_bias + nl), *reinterpret_cast<const v4f *>(l_scale + nl), relu, a.rm);
          const int left = min(4, a.n - n);
          const size_t at = (size_t)m * (size_t)a.dst_ld + (size_t)n;
          if constexpr (ESZ == 1) {
            if (lut) out[0] = (int)lin_lut4(l_lut, (unsigned)out[0], flip);
            unsigned char *const p = a.dst + at;
            if (a.vec && left == 4) *reinterpret_cast<int *>(p) = out[0];
            else
#pragma unroll
              for (int j = 0; j < 4; ++j)
                if (j < left) p[j] = (unsigned char)((unsigned)out[0] >> (8 * j));
          } else {
            int *const p = reinterpret_cast<int *>(a.dst) + at;
            if (a.vec && left == 4) dfx_store16(reinterpret_cast<v4i *>(p), out);
            else
#pragma unroll
              for (int j = 0; j < 4; ++j)
                if (j < left) p[j] = out[j];
          }
        }
    }
    __syncthreads();  // the next tile rewrites the constants and buffer 0, which the last slab may still be read from
  }
}

}  // namespace dfx
