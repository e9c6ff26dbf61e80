// bmm.cuh -- the batched int8 matrix product's kernels (dfx_bmm_* of include/dfx.h; gfx950): C[g] = requant(A[g] . B[g](^T))
// over two DEVICE tensors with their own strides, one launch.
//
// bmm_generic_kernel: one thread per C element, grid-stride, any strides and alignment, the exact route.  It defines the bits.
//
// bmm_mfma_kernel: v_mfma_i32_32x32x32_i8, no LDS in the NT form, no scratch, the requant in the epilogue.
//   * A wave owns one 32 x 32 tile of C of one matrix g; the four waves of a workgroup own four consecutive tiles (n tile
//     fastest, then m tile, then g), so that they share rows of A in L2.  A workgroup loops over units of four tiles
//     (DFX_BMM_GRID caps the grid); a wave whose tile lies beyond the last one computes the last tile again and stores nothing,
//     so the barriers of the NN form are uniform.
//   * N is carried by the MFMA's A operand (rows), M by its B operand (columns): D[n][m].  With fc.cuh's lane map -- lane l,
//     r = l & 31, h = l >> 5, holds 16 consecutive k of row / column r starting at 16 h of a 32-k step; D is column l & 31, row
//     (reg & 3) + 8 (reg >> 2) + 4 h -- a lane ends up with 4 x 4 ADJACENT n of ITS row m: each quad leaves as one dword
//     (1-byte dst) or one dfx_store16 (4-byte dst) where C's alignment allows, element by element otherwise.
//   * NT form (B is {N,K}): both fragments are one aligned 16-byte global load per lane per 32-k step, straight into the
//     operand registers; the next step's loads are issued before the current step's MFMA.
//   * NN form (B is {K,N}): the 32 k x 32 n block of a step is loaded as 64 aligned 16-byte pieces (lane l: k row l >> 1,
//     n piece l & 1), written byte by byte TRANSPOSED into the wave's own LDS image T[n][k] (pitch 48, two buffers, one
//     barrier per step), and read back as one 16-byte k-contiguous fragment per lane.
//   * K tails: a piece of B that starts at or beyond K is never loaded (zero); in the piece K falls into, the bytes beyond K
//     are zeroed by a byte mask (NT) / the rows k >= K are zero pieces (NN).  A's tail then multiplies zeros, whatever its pad
//     holds.  M / N tails: rows beyond M / N load from the last valid row (fc_tile's clamp: no address outside the operand is
//     formed) and are never stored; an NN piece that starts at or beyond N is not loaded.
//   * u8 A is staged as a ^ 0x80 (a - 128 as s8).  The compensation 128 * sum_k B[g,n,k] is computed from the B fragments the
//     lane already holds (v_dot4_i32_i8 against 0x01010101), the two lane halves are combined once per tile, and the epilogue
//     fetches the value of ITS n with a lane shuffle and adds it as an integer before the requant.
#pragma once

#include "gconv.cuh"  // gc_mfma, gc_quarter

#include "bmm_plan.h"

namespace dfx {

struct BmmArgs {
  const unsigned char *a;
  const signed char *b;
  unsigned char *c;
  const float *scale;        // [n rounded up to 32] (a single scale is expanded by the host)
  long long a_s0, a_s1, lda, b_s0, b_s1, ldb, c_s0, c_s1, ldc;
  int batch0, batch1, m, n, k;
  int trans_b, a_u8, dst_dt, relu, rm;
  int mt, nt;                // tiles of 32 along m and n
  long long tiles, units;    // MFMA: tiles = G * mt * nt, units of BMM_WAVES tiles
  int c_vec;                 // MFMA: 4 adjacent n leave as one store (c, ldc and C's batch strides allow it)
  long long items;           // generic: C elements
};

// the logit bias (bias_plan.h): the handle's device image {p0 * p1, rows, cols} f32
struct BmmBiasArgs {
  const float *img;
  int p0, p1;                // periods over batch0 / batch1
  int rows, cols;            // m, or 1 (one row broadcast over m); n rounded up to 32
};
// The argument of the BIASED instances of both kernels.  The kernels are templates over their argument type: the unbiased
// instances take BmmArgs itself, so their argument segment and their code are what they were before the bias existed (the
// hidden grid size stays in the segment's third 64-byte line: one line more to fetch showed as 2.4 % at the ViT-B bs 8 P.V
// point of tools/bench_bmm when the bias's fields sat in BmmArgs).
struct BmmBiasedArgs : BmmArgs {
  BmmBiasArgs bias;
};
template <class ARGS>
struct bmm_biased { static constexpr bool value = false; };
template <>
struct bmm_biased<BmmBiasedArgs> { static constexpr bool value = true; };

// bias_plan.h's image index: the row of matrix (b0, b1)'s table that C's row m uses (m < the operand's rows).  b0 < batch0 and
// b1 < batch1 fit an int: the two remainders are 32-bit ones
__device__ __forceinline__ const float *bmm_bias_row(const float *img, int p0, int p1, int rows, int cols, long long b0, long long b1, int m) {
  const long long t = (long long)((unsigned)b0 % (unsigned)p0) * p1 + (long long)((unsigned)b1 % (unsigned)p1);
  return img + (size_t)((t * rows + (rows == 1 ? 0 : m)) * cols);
}

// bytes >= nv of a 16-byte piece zeroed (0 <= nv <= 16)
__device__ __forceinline__ v4i bmm_mask16(v4i v, int nv) {
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const int left = nv - 4 * d;  // valid bytes of this dword
    const unsigned mk = left >= 4 ? 0xffffffffu : left <= 0 ? 0u : ((1u << (8 * left)) - 1u);
    v[d] = (int)((unsigned)v[d] & mk);
  }
  return v;
}

// sum of the 16 signed bytes of a piece
__device__ __forceinline__ int bmm_bytesum(v4i v) {
  int s = 0;
#pragma unroll
  for (int d = 0; d < 4; ++d) s = __builtin_amdgcn_sdot4(v[d], 0x01010101, s, false);
  return s;
}

// the NN form's transposed images of B: two per wave.  Declared in the NN instances only.
template <bool NT>
__device__ __forceinline__ unsigned char *bmm_nn_images() {
  if constexpr (NT) {
    return nullptr;
  } else {
    __shared__ __attribute__((aligned(16))) unsigned char images[BMM_NN_LDS];
    return images;
  }
}

// ARGS: BmmArgs, or BmmBiasedArgs: the epilogue's requant then adds the logit bias's entry
template <bool NT, int DST, bool FAST, class ARGS>
__global__ __launch_bounds__(BMM_THREADS) void bmm_mfma_kernel(ARGS a) {
  constexpr bool BIAS = bmm_biased<ARGS>::value;
  constexpr int ESZ = (DST == DFX_F32 || DST == DFX_S32) ? 4 : 1;
  unsigned char *const bmm_lds = bmm_nn_images<NT>();  // (the NT instances have no LDS at all)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, h = lane >> 5;
  const v4i zero4 = v4i{0, 0, 0, 0};
  const int axor = a.a_u8 ? (int)0x80808080 : 0;
  const v4i x80 = v4i{axor, axor, axor, axor};
  const int nks = (a.k + 31) / 32;
  const bool relu = a.relu != 0;
  unsigned char *const tw = NT ? nullptr : bmm_lds + wave * 2 * 32 * BMM_NN_PITCH;  // NN: this wave's two images

  for (long long u = blockIdx.x; u < a.units; u += gridDim.x) {  // uniform over the workgroup: so are the barriers below
    const long long t_raw = u * BMM_WAVES + wave;
    const bool live = t_raw < a.tiles;                           // (wave-uniform)
    const long long t = live ? t_raw : a.tiles - 1;
    const int ntile = (int)(t % a.nt);
    const long long r0 = t / a.nt;
    const int mtile = (int)(r0 % a.mt);
    const long long g = r0 / a.mt;
    const long long b0 = g / a.batch1, b1 = g % a.batch1;
    const int m0 = 32 * mtile, n0 = 32 * ntile;
    const unsigned char *const ag = a.a + (size_t)(b0 * a.a_s0 + b1 * a.a_s1);
    const signed char *const bg = a.b + (size_t)(b0 * a.b_s0 + b1 * a.b_s1);
    // this lane's row of A (the MFMA's column m) and, NT, its row of B (the MFMA's row n), clamped into the operand
    const unsigned char *const arow = ag + (size_t)min(m0 + l31, a.m - 1) * (size_t)a.lda + 16 * h;
    const signed char *const brow = bg + (size_t)min(n0 + l31, a.n - 1) * (size_t)a.ldb + 16 * h;
    // NN: this lane's piece of a step's block: k row l >> 1, n piece l & 1
    const int kk = lane >> 1, np = n0 + 16 * (lane & 1);
    const bool np_in = np < a.n;  // (pieces start at multiples of 16 <= ldb - 16 when they start below n)

    auto load_a = [&](int ks) -> v4i {
      const int kp = 32 * ks + 16 * h;
      return kp < a.k ? *reinterpret_cast<const v4i *>(arow + 32 * ks) : zero4;
    };
    auto load_b = [&](int ks) -> v4i {
      if (NT) {
        const int kp = 32 * ks + 16 * h;
        if (kp >= a.k) return zero4;
        const v4i v = *reinterpret_cast<const v4i *>(brow + 32 * ks);
        return a.k - kp < 16 ? bmm_mask16(v, a.k - kp) : v;
      } else {
        const int kr = 32 * ks + kk;
        return (kr < a.k && np_in) ? *reinterpret_cast<const v4i *>(bg + (size_t)kr * (size_t)a.ldb + np) : zero4;
      }
    };

    // the lane's four quads of bias, n0 + 8 q + 4 h .. + 3 of its row m, issued ahead of the K loop (the row clamped as A's is;
    // n0 + 31 < up32(n) = bias_cols: inside the padded image row, 16-byte aligned)
    v4f bq[4];
    if constexpr (BIAS) {
      const float *const brw = bmm_bias_row(a.bias.img, a.bias.p0, a.bias.p1, a.bias.rows, a.bias.cols, b0, b1, min(m0 + l31, a.m - 1)) + n0 + 4 * h;
#pragma unroll
      for (int q = 0; q < 4; ++q) bq[q] = *reinterpret_cast<const v4f *>(brw + 8 * q);
    }

    v16i acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0;
    int bsum = 0;  // sum of the B bytes this lane has fed: row n = l31, its half of every step
    v4i fa = load_a(0), fb = load_b(0);
    for (int ks = 0; ks < nks; ++ks) {
      v4i na = zero4, nb = zero4;
      if (ks + 1 < nks) {
        na = load_a(ks + 1);
        nb = load_b(ks + 1);
      }
      v4i bf = fb;
      if (!NT) {
        unsigned char *const img = tw + (ks & 1) * 32 * BMM_NN_PITCH;
        unsigned char *const col = img + (16 * (lane & 1)) * BMM_NN_PITCH + kk;  // T[16 p + i][kk] = byte i of the piece
#pragma unroll
        for (int i = 0; i < 16; ++i) col[i * BMM_NN_PITCH] = (unsigned char)((unsigned)fb[i >> 2] >> (8 * (i & 3)));
        __syncthreads();  // (the image is the wave's own; the barrier orders its writes before its reads.  The other image's
                          //  readers of the previous step are behind the previous barrier.)
        bf = *reinterpret_cast<const v4i *>(img + l31 * BMM_NN_PITCH + 16 * h);
      }
      bsum += bmm_bytesum(bf);
      acc = gc_mfma(bf, fa ^ x80, acc);  // D[n][m]
      fa = na;
      fb = nb;
    }
    if (!NT) __syncthreads();  // the next unit's first write goes to image 0, which step nks - 1 may still read when nks is odd

    // compensation of the xor: sum_k (a - 128) b = sum a b - 128 sum b.  Both halves of row n, then on every lane.
    // The lane holds n0 + 8 q + 4 h + j in register 4 q + j and fetches that row's value from lane 8 q + 4 h + j; every lane
    // takes part in every shuffle (nothing has diverged yet).
    if (a.a_u8) {  // (uniform)
      const int comp_tot = 128 * (bsum + __shfl_xor(bsum, 32));
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] += __shfl(comp_tot, 8 * (i >> 2) + 4 * h + (i & 3));
    }

    const int mrow = m0 + l31;
    const size_t cbase = (size_t)(b0 * a.c_s0 + b1 * a.c_s1) + (size_t)mrow * (size_t)a.ldc;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int nl = 8 * q + 4 * h;  // the lane holds n0 + nl .. + 3 of its row m
      const int a4[4] = {acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
      const int n = n0 + nl;
      if (!live || mrow >= a.m || n >= a.n) continue;
      v4f bias4 = v4f{0.0f, 0.0f, 0.0f, 0.0f};
      if constexpr (BIAS) bias4 = bq[q];
      const v4i out = gc_quarter<DST, FAST>(a4, bias4, *reinterpret_cast<const v4f *>(a.scale + n), relu, a.rm);
      const int left = min(4, a.n - n);
      if constexpr (ESZ == 1) {
        unsigned char *const p = a.c + cbase + n;
        if (a.c_vec && left == 4) *reinterpret_cast<int *>(p) = out[0];
        else
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (j < left) p[j] = (unsigned char)((unsigned)out[0] >> (8 * j));
      } else {
        int *const p = reinterpret_cast<int *>(a.c) + cbase + n;
        if (a.c_vec && left == 4) dfx_store16(reinterpret_cast<v4i *>(p), out);
        else
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (j < left) p[j] = out[j];
      }
    }
  }
}

}  // namespace dfx
