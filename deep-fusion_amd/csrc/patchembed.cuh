// patchembed.cuh -- the int8 patch-embedding op's kernels (dfx_patchembed_* of include/dfx.h; gfx950): a non-overlapping
// conv as one GEMM over the image in place, dst a token matrix, one launch.
//
// patchembed_generic_kernel (patchembed.hip): one thread per dst element, grid-stride, any shape and alignment, the exact
// route.  It reads the same packed image through linear_pack.h's lin_wei_offset and defines the bits.
//
// patchembed_tile_kernel<BM, DST, FAST, G>: linear_tile_kernel's scheme (linear.cuh) -- 256 lanes own a
// BM x 128 tile, K in slabs of 64 through two LDS buffers with one barrier per slab, both operands in LDS in fragment order so
// that every MFMA operand is one conflict-free ds_read_b128, gc_quarter's epilogue -- with three differences:
//   * The A loader GATHERS.  Row m of a tile is token (b, ty, tx); its patch starts at src + ((b ih + ty ph) iw + tx pw) ic,
//     computed once per tile in 64 bits.  Lane t owns piece p = t & 3 of row t >> 2 (and of row 64 + (t >> 2) at BM 128), so
//     the K offsets of its piece are the same for all its rows: ktab[(64 ks + 16 p) / G + j], j < 16 / G, one entry (G 16:
//     one 16-byte load) or four (G 4: four dword loads).  The entries of slab ks + 1 are fetched while slab ks is loaded, so
//     no load waits for its address.  A granule at or beyond K is not loaded and stays zero; K is a multiple of G, and a
//     granule lies within one run of pw * ic bytes, so no address outside the patch's rows is formed.  Tokens at or beyond
//     bs * th * tw clamp to the last valid token and store nothing.
//   * With a table the epilogue adds table[t][n .. n + 3] -- one aligned 16-byte global load per quad from rows of up4(oc)
//     floats -- instead of the per-n bias (wave-uniform branch).
//   * The dst row of m is b * img_rows + t0 + t; the prefix rows are stored behind the tile loop, grid-stride, an element once.
#pragma once

// lin_wei_offset (and lin_nslabs under it) are plain inline host functions of HIP-free headers; the generic kernel calls
// them on the device, so they are declared for both sides here, before anything else includes those headers.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <cmath>
#include <vector>
#pragma clang force_cuda_host_device begin
#include "linear_plan.h"
#include "linear_pack.h"
#pragma clang force_cuda_host_device end

#include "gconv.cuh"  // gc_mfma, gc_quarter

#include "patchembed_plan.h"

namespace dfx {

struct PeArgs {
  const unsigned char *src;
  unsigned char *dst;
  const unsigned char *wpk;  // linear_pack.h's weight section
  const int *comp;           // [nblocks * 128]
  const float *bias;         // [nblocks * 128] f32 (0 without bias, and with a table)
  const float *scale;        // [nblocks * 128]
  const int *ktab;           // K offset table (tile class only)
  const float *table;        // {tokens, tld} f32, or nullptr
  const unsigned char *prefix;  // {t0, oc} of dst's dtype, or nullptr
  long long rows;            // bs * tokens
  long long tokens;          // th * tw
  long long img_rows, dst_ld;
  long long img_bytes, row_bytes;  // ih * iw * ic, iw * ic
  int tw, ph, run;           // run = pw * ic
  int k, n, nks, tld;
  int t0, bs;
  int a_u8, dst_dt, relu, rm;
  int vec;                   // tile: 4 adjacent n leave as one store
  long long mt, tiles;       // tile: m tiles per n-block, tiles in all
  long long items;           // generic: dst elements of the tokens
  long long pitems;          // prefix elements in all: bs * t0 * oc (0 without a prefix)
};

// the prefix rows: element e of {bs, t0, oc}, each written by exactly one thread of the launch
template <int ESZ>
__device__ __forceinline__ void pe_store_prefix(const PeArgs &a) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long per = (long long)a.t0 * a.n;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < a.pitems; e += stride) {
    const long long b = e / per, r = e - b * per;
    const long long row = r / a.n;
    const int o = (int)(r - row * a.n);
    const size_t at = (size_t)(b * a.img_rows + row) * (size_t)a.dst_ld + (size_t)o;
    if (ESZ == 1) a.dst[at] = a.prefix[r];
    else reinterpret_cast<int *>(a.dst)[at] = reinterpret_cast<const int *>(a.prefix)[r];
  }
}

// LDS: [2][BM * 64 tokens | 8 KB weights] | comp[128] | bias[128] | scale[128]   (pe_lds_bytes)
template <int BM, int DST, bool FAST, int G>
__global__ __launch_bounds__(LIN_THREADS, 2) void patchembed_tile_kernel(PeArgs a) {
  constexpr int ESZ = (DST == DFX_F32 || DST == DFX_S32) ? 4 : 1;
  constexpr int MB = BM / 64;                     // 32-row blocks per wave
  constexpr int AP = BM * 4 / LIN_THREADS;        // token pieces per lane per slab
  constexpr int GP = 16 / G;                      // granules per piece
  constexpr int ABYTES = BM * LIN_KS, BUF = ABYTES + LIN_WBLOCK;
  extern __shared__ __attribute__((aligned(16))) unsigned char pe_lds[];
  int *const l_comp = reinterpret_cast<int *>(pe_lds + 2 * BUF);
  float *const l_bias = reinterpret_cast<float *>(l_comp + LIN_BN);
  float *const l_scale = l_bias + LIN_BN;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, h = lane >> 5;
  const int wm = wave & 1, wn = wave >> 1;
  const v4i zero4 = v4i{0, 0, 0, 0};
  const int axor = a.a_u8 ? (int)0x80808080 : 0;
  const v4i x80 = v4i{axor, axor, axor, axor};
  const bool relu = a.relu != 0;
  const bool tab = a.table != nullptr;  // (uniform)
  const int p = tid & 3;                // this lane's piece of every row it loads
  const int *const ktab = a.ktab + p * GP;

  for (long long t = blockIdx.x; t < a.tiles; t += gridDim.x) {  // uniform over the workgroup: so are the barriers
    const long long nb = t / a.mt, mi = t - nb * a.mt;
    const long long m0 = mi * BM;
    const int n0 = (int)nb * LIN_BN;
    if (tid < LIN_BN) {  // the tile's constants (the image has 128 entries per n-block)
      l_comp[tid] = a.comp[n0 + tid];
      l_bias[tid] = a.bias[n0 + tid];
      l_scale[tid] = a.scale[n0 + tid];
    }
    // this lane's rows: the first byte of the token's patch, clamped into the valid tokens
    const unsigned char *abase[AP];
    int aoff[AP];
#pragma unroll
    for (int i = 0; i < AP; ++i) {
      const int row = (tid >> 2) + (LIN_THREADS / 4) * i;
      const long long m = m0 + row < a.rows ? m0 + row : a.rows - 1;
      const long long b = m / a.tokens, tk = m - b * a.tokens;
      const long long ty = tk / a.tw, tx = tk - ty * a.tw;
      abase[i] = a.src + (size_t)b * (size_t)a.img_bytes + (size_t)(ty * a.ph) * (size_t)a.row_bytes + (size_t)tx * (size_t)a.run;
      aoff[i] = ((row >> 5) * 4 + p) * 512 + (row & 31) * 16;
    }
    const unsigned char *const wblk = a.wpk + (size_t)nb * (size_t)a.nks * LIN_WBLOCK + (size_t)tid * 16;

    int koff[GP];  // the offsets of this lane's granules of the slab that is loaded next
    auto offsets = [&](int ks) {
#pragma unroll
      for (int j = 0; j < GP; ++j) koff[j] = ktab[ks * (LIN_KS / G) + j];
    };
    v4i ra[AP], rb[2];
    auto load = [&](int ks) {
      const int c0 = LIN_KS * ks + 16 * p;
#pragma unroll
      for (int i = 0; i < AP; ++i) {
        if constexpr (G == 16) {
          ra[i] = c0 < a.k ? *reinterpret_cast<const v4i *>(abase[i] + koff[0]) : zero4;
        } else {
#pragma unroll
          for (int j = 0; j < GP; ++j) ra[i][j] = c0 + 4 * j < a.k ? *reinterpret_cast<const int *>(abase[i] + koff[j]) : 0;
        }
      }
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

    offsets(0);
    load(0);
    if (a.nks > 1) offsets(1);
    for (int ks = 0; ks < a.nks; ++ks) {
      unsigned char *const buf = pe_lds + (ks & 1) * BUF;
#pragma unroll
      for (int i = 0; i < AP; ++i) *reinterpret_cast<v4i *>(buf + aoff[i]) = ra[i] ^ x80;
#pragma unroll
      for (int i = 0; i < 2; ++i) *reinterpret_cast<v4i *>(buf + ABYTES + tid * 16 + i * (LIN_THREADS * 16)) = rb[i];
      __syncthreads();
      if (ks + 1 < a.nks) {
        load(ks + 1);  // in flight under this slab's MFMAs
        if (ks + 2 < a.nks) offsets(ks + 2);
      }
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
      if (m < a.rows) {
        const long long b = m / a.tokens, tk = m - b * a.tokens;
        const size_t drow = (size_t)(b * a.img_rows + a.t0 + tk) * (size_t)a.dst_ld;
        const float *const trow = tab ? a.table + (size_t)tk * (size_t)a.tld : nullptr;
#pragma unroll
        for (int nn = 0; nn < 2; ++nn)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int nl = wn * 64 + nn * 32 + 8 * q + 4 * h;  // within the tile
            const int n = n0 + nl;
            if (n >= a.n) continue;
            int a4[4] = {acc[mb][nn][4 * q], acc[mb][nn][4 * q + 1], acc[mb][nn][4 * q + 2], acc[mb][nn][4 * q + 3]};
            if (a.a_u8) {  // (uniform)
              const v4i c4 = *reinterpret_cast<const v4i *>(l_comp + nl);
#pragma unroll
              for (int j = 0; j < 4; ++j) a4[j] += c4[j];
            }
            const v4f add4 = tab ? *reinterpret_cast<const v4f *>(trow + n) : *reinterpret_cast<const v4f *>(l_bias + nl);
            v4i out = gc_quarter<DST, FAST>(a4, add4, *reinterpret_cast<const v4f *>(l_scale + nl), relu, a.rm);
            const int left = min(4, a.n - n);
            const size_t at = drow + (size_t)n;
            if constexpr (ESZ == 1) {
              unsigned char *const pd = a.dst + at;
              if (a.vec && left == 4) *reinterpret_cast<int *>(pd) = out[0];
              else
#pragma unroll
                for (int j = 0; j < 4; ++j)
                  if (j < left) pd[j] = (unsigned char)((unsigned)out[0] >> (8 * j));
            } else {
              int *const pd = reinterpret_cast<int *>(a.dst) + at;
              if (a.vec && left == 4) dfx_store16(reinterpret_cast<v4i *>(pd), out);
              else
#pragma unroll
                for (int j = 0; j < 4; ++j)
                  if (j < left) pd[j] = out[j];
            }
          }
      }
    }
    __syncthreads();  // the next tile rewrites the constants and buffer 0, which the last slab may still be read from
  }
  pe_store_prefix<ESZ>(a);
}

}  // namespace dfx
