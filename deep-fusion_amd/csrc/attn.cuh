// attn.cuh -- the fused int8 attention's kernel (dfx_attn_* of include/dfx.h, DFX_ATTN_FUSED; gfx950): Q.K^T, the table
// softmax and P.V in ONE launch, the logits and the probabilities never leaving the CU.  Bit-identical to the chain of
// dfx_bmm, dfx_head and dfx_bmm it is defined by: the products are exact s32 sums, the requants are gc_quarter's, the softmax
// is head.cuh's head_prob / head_cvt_u8 on an exact u32 sum.
//
// attn_fused_kernel: a workgroup of four waves owns a strip of 32 query rows of one matrix g and loops over strips
// (DFX_ATTN_GRID caps the grid).  LDS: [table E: 1 KB][strip: 32 rows of `pitch` = up16(tk) + 16 bytes][the waves' V images].
//   1 LOGITS.  bmm.cuh's NT form and lane map: D[n][m], the keys on the MFMA's rows, the queries on its columns.  The strip's
//     Q fragments (d <= 256: 8 steps, 32 VGPRs; u8 Q as q ^ 0x80) are loaded once; the waves take the 32-key tiles in turn with
//     K fragments straight from global (rows beyond tk clamped, the d tail masked, the u8 compensation from the K fragments).
//     gc_quarter<DFX_S8> with logit_scale; a lane's 4 adjacent n go as one dword into L[m][n].
//   2 SOFTMAX in LDS, in place.  A wave owns 8 rows and works on all of them at once, 8 lanes per row: a lane scans the 16-byte
//     groups sub, sub + 8, ... of its row; row maximum and the exact u32 sum through head.cuh's reductions over the row's 8 lanes
//     (a wave per row would leave 51 of 64 lanes idle at tk 197 and 60 at tk 49); the u8 probability overwrites the s8 logit
//     byte it came from.
//   3 CONTEXT.  bmm.cuh's NN form: V {tk, dv} goes through the wave's own transposed LDS image, rows n >= tk are zero pieces, so
//     P's pad bytes (and whatever the strip holds up to the next multiple of 32) multiply zeros.  P fragments are 16-byte
//     k-contiguous reads of the strip, staged as p ^ 0x80 with the compensation 128 * sum_n V[n,j] from the V fragments.  A work
//     item is (column tile of 32, key part); where there are fewer column tiles than waves the key range is split over
//     4 / tiles waves and the s32 partial sums meet through LDS (integer sums: the order does not change the bits).  Every wave
//     runs the same number of steps -- steps beyond the key range feed zeros -- so every barrier is uniform.
#pragma once

#include "bmm.cuh"   // gc_mfma, gc_quarter, bmm_mask16, bmm_bytesum, BMM_NN_PITCH
#include "head.cuh"  // head_key8, head_byte, head_prob, head_cvt_u8, the wave reductions

#include "attn_plan.h"

namespace dfx {

struct AttnArgs {
  const unsigned char *q;
  const signed char *k, *v;
  unsigned char *o;
  const unsigned int *table;   // the handle's device copy of E
  const float *oscale;         // [dv rounded up to 32] (a single scale is expanded by the host)
  float logit_scale, prob_scale;
  long long q_s0, q_s1, ldq, k_s0, k_s1, ldk, v_s0, v_s1, ldv, o_s0, o_s1, ldo;
  int batch1, tq, tk, d, dv;
  int q_u8, dst_dt, relu, rm;
  int mt;                      // strips per matrix
  long long strips;            // G * mt
  int pitch;                   // bytes per strip row
  int vtiles, kparts;          // context: column tiles of 32, key parts (attn_plan.h)
  int o_vec;                   // 4 adjacent j leave as one store (o, ldo and O's batch strides allow it)
  // the logit bias (bias_plan.h): the handle's device image {bias_p0 * bias_p1, bias_rows, bias_cols} f32, or nullptr
  const float *bias;
  int bias_p0, bias_p1;        // periods over batch0 / batch1
  int bias_rows, bias_cols;    // tq, or 1 (one row broadcast over tq); tk rounded up to 32
};

// BIAS: the logits' requant adds the logit bias's entry (a.bias is set), as dfx_bmm's epilogue does; the instances without
// it are the kernel as it was before the bias existed.
// amdgpu_waves_per_eu: the unbiased instances take 164 or 168 VGPRs (AGPRs included), three waves per SIMD; the 16 VGPRs of the
// tile's bias quads took the biased ones to 184 - 200, TWO waves per SIMD, i.e. two workgroups per CU instead of three, and every
// point with more than 512 strips paid for it (ViT-B bs 8: 672 strips, 1.50x the unbiased time; bs 64: 1.28x).  Asked for three
// waves the compiler fits the biased instances into 157 - 161 VGPRs without scratch.  The argument depends on BIAS so that
// the unbiased instances stay as they were (1 is the default's lower bound: profiles/attn/bias_codegen.txt).
template <int DST, bool FL, bool FO, bool BIAS>
__global__ __launch_bounds__(ATTN_THREADS) __attribute__((amdgpu_waves_per_eu(BIAS ? 3 : 1))) void attn_fused_kernel(AttnArgs a) {
  constexpr int ESZ = (DST == DFX_F32 || DST == DFX_S32) ? 4 : 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char attn_lds[];
  unsigned *const tab = reinterpret_cast<unsigned *>(attn_lds);
  unsigned char *const strip = attn_lds + HEAD_TABLE_BYTES;
  unsigned char *const vimg = strip + ATTN_STRIP * a.pitch;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, h = lane >> 5;
  const v4i zero4 = v4i{0, 0, 0, 0};
  const int qxor = a.q_u8 ? (int)0x80808080 : 0;
  const v4i qx80 = v4i{qxor, qxor, qxor, qxor};
  const v4i px80 = v4i{(int)0x80808080, (int)0x80808080, (int)0x80808080, (int)0x80808080};
  const int nds = (a.d + 31) / 32;                       // steps over d, <= 8
  const int nkt = (a.tk + 31) / 32;                      // key tiles = steps over tk
  const int spp = (nkt + a.kparts - 1) / a.kparts;       // steps per key part
  const int items = a.vtiles * a.kparts, passes = (items + ATTN_WAVES - 1) / ATTN_WAVES;
  const int groups = (a.tk + 15) / 16;
  const bool relu = a.relu != 0;
  const v4f ls4 = v4f{a.logit_scale, a.logit_scale, a.logit_scale, a.logit_scale};
  unsigned char *const tw = vimg + wave * 2 * 32 * BMM_NN_PITCH;  // this wave's two V images
  int *const red = reinterpret_cast<int *>(vimg);                // the split-key sums (the same bytes, between barriers)

  tab[tid] = a.table[tid];  // (published by the barrier behind the first strip's logits)

  for (long long u = blockIdx.x; u < a.strips; u += gridDim.x) {  // uniform over the workgroup: so are the barriers below
    const int mtile = (int)(u % a.mt);
    const long long g = u / a.mt;
    const long long b0 = g / a.batch1, b1 = g % a.batch1;
    const int m0 = ATTN_STRIP * mtile;
    const unsigned char *const qg = a.q + (size_t)(b0 * a.q_s0 + b1 * a.q_s1);
    const signed char *const kg = a.k + (size_t)(b0 * a.k_s0 + b1 * a.k_s1);
    const signed char *const vg = a.v + (size_t)(b0 * a.v_s0 + b1 * a.v_s1);

    // ---- 1: logits -------------------------------------------------------------------------------------------------------
    // this lane's row of Q (the MFMA's column m), clamped into the operand; pieces at or beyond d are zero (K's are too)
    const unsigned char *const qrow = qg + (size_t)min(m0 + l31, a.tq - 1) * (size_t)a.ldq + 16 * h;
    v4i qf[ATTN_D_MAX / 32];
#pragma unroll
    for (int s = 0; s < ATTN_D_MAX / 32; ++s) {
      qf[s] = zero4;
      if (s < nds && 32 * s + 16 * h < a.d) qf[s] = *reinterpret_cast<const v4i *>(qrow + 32 * s) ^ qx80;
    }
    // this lane's row of the bias: the strip's clamped query row, as Q's is
    const float *biasrow = nullptr;
    if constexpr (BIAS) biasrow = bmm_bias_row(a.bias, a.bias_p0, a.bias_p1, a.bias_rows, a.bias_cols, b0, b1, min(m0 + l31, a.tq - 1)) + 4 * h;
    for (int kt = wave; kt < nkt; kt += ATTN_WAVES) {
      const int n0 = 32 * kt;
      const signed char *const krow = kg + (size_t)min(n0 + l31, a.tk - 1) * (size_t)a.ldk + 16 * h;
      // the tile's four quads of bias, n0 + 8 q + 4 h .. + 3, issued ahead of the MFMA loop (n0 + 31 < up32(tk) = bias_cols:
      // inside the padded image row, 16-byte aligned)
      v4f bq[4];
      if constexpr (BIAS) {
#pragma unroll
        for (int q = 0; q < 4; ++q) bq[q] = *reinterpret_cast<const v4f *>(biasrow + n0 + 8 * q);
      }
      v16i acc;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0;
      int bsum = 0;  // sum of the K bytes this lane has fed: row n = l31, its half of every step
#pragma unroll
      for (int s = 0; s < ATTN_D_MAX / 32; ++s) {
        if (s < nds) {  // (uniform)
          const int kp = 32 * s + 16 * h;
          v4i kf = zero4;
          if (kp < a.d) {
            kf = *reinterpret_cast<const v4i *>(krow + 32 * s);
            if (a.d - kp < 16) kf = bmm_mask16(kf, a.d - kp);
          }
          bsum += bmm_bytesum(kf);
          acc = gc_mfma(kf, qf[s], acc);  // D[n][m]
        }
      }
      if (a.q_u8) {  // (uniform) bmm.cuh's compensation of the xor
        const int comp_tot = 128 * (bsum + __shfl_xor(bsum, 32));
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] += __shfl(comp_tot, 8 * (i >> 2) + 4 * h + (i & 3));
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int a4[4] = {acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
        v4f bias4 = v4f{0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (BIAS) bias4 = bq[q];
        const v4i out = gc_quarter<DFX_S8, FL>(a4, bias4, ls4, false, a.rm);
        // (n0 + 31 < up32(tk) <= pitch: inside the row)
        *reinterpret_cast<int *>(strip + l31 * a.pitch + n0 + 8 * q + 4 * h) = out[0];
      }
    }
    __syncthreads();

    // ---- 2: softmax, in place -----------------------------------------------------------------------------------------------
    {
      // a wave owns 8 rows and works on all of them at once: 8 lanes per row (row = lane >> 3), a lane scans the groups
      // sub, sub + 8, ... of its row; the 8 lanes of a row meet through shuffles over their aligned group of lanes
      constexpr int LPR = 64 / (ATTN_STRIP / ATTN_WAVES);  // lanes per row: 8
      const int sub = lane & (LPR - 1);
      v4i *const p = reinterpret_cast<v4i *>(strip + ((ATTN_STRIP / ATTN_WAVES) * wave + lane / LPR) * a.pitch);
      unsigned m = 0;
      for (int gi = sub; gi < groups; gi += LPR) {
        const v4i raw = p[gi];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const unsigned key = head_key8(head_byte(raw, e), DFX_S8);
          if (gi * 16 + e < a.tk) m = key > m ? key : m;
        }
      }
      m = head_lanes_max<LPR>(m);
      unsigned sum = 0;
      for (int gi = sub; gi < groups; gi += LPR) {
        const v4i raw = p[gi];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const unsigned key = head_key8(head_byte(raw, e), DFX_S8);
          if (gi * 16 + e < a.tk) sum += tab[m - key];
        }
      }
      const float fs = __uint2float_rn(head_lanes_sum<LPR>(sum));
      for (int gi = sub; gi < groups; gi += LPR) {  // (a lane rewrites the groups it reads and no others)
        const v4i raw = p[gi];
        v4i o = zero4;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const unsigned key = head_key8(head_byte(raw, e), DFX_S8);
          const float pr = head_prob(tab[gi * 16 + e < a.tk ? m - key : 0], fs);  // (a pad byte may exceed the maximum)
          o[e >> 2] |= head_cvt_u8(pr, a.prob_scale) << (8 * (e & 3));
        }
        p[gi] = o;
      }
    }
    __syncthreads();

    // ---- 3: context ---------------------------------------------------------------------------------------------------------
    for (int pass = 0; pass < passes; ++pass) {  // (uniform)
      const int item_raw = pass * ATTN_WAVES + wave;
      const bool live = item_raw < items;  // (wave-uniform) a wave beyond the last item repeats it and stores nothing
      const int item = live ? item_raw : items - 1;
      const int jt = item / a.kparts, part = item % a.kparts;
      const int n0 = 32 * jt, ks0 = part * spp;
      // this lane's piece of a step's block of V: key row l >> 1, column piece l & 1
      const int kk = lane >> 1, np = n0 + 16 * (lane & 1);
      const bool np_in = np < a.dv;  // (pieces start at multiples of 16 <= ldv - 16 when they start below dv)
      auto load_v = [&](int ks) -> v4i {
        const int kr = 32 * ks + kk;
        return (ks < nkt && kr < a.tk && np_in) ? *reinterpret_cast<const v4i *>(vg + (size_t)kr * (size_t)a.ldv + np) : zero4;
      };
      v16i acc;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0;
      int bsum = 0;  // sum of the V bytes this lane has fed: column j = l31, its half of every step
      v4i fv = load_v(ks0);
      for (int i = 0; i < spp; ++i) {  // (the same trip count on every wave)
        const int ks = ks0 + i;
        const v4i nv = i + 1 < spp ? load_v(ks + 1) : zero4;
        unsigned char *const img = tw + (i & 1) * 32 * BMM_NN_PITCH;
        unsigned char *const col = img + (16 * (lane & 1)) * BMM_NN_PITCH + kk;  // T[16 p + e][kk] = byte e of the piece
#pragma unroll
        for (int e = 0; e < 16; ++e) col[e * BMM_NN_PITCH] = (unsigned char)((unsigned)fv[e >> 2] >> (8 * (e & 3)));
        __syncthreads();  // (the image is the wave's own: as in bmm.cuh)
        const v4i vf = *reinterpret_cast<const v4i *>(img + l31 * BMM_NN_PITCH + 16 * h);
        // (32 ks + 16 h + 16 <= up32(tk) <= pitch when ks < nkt; steps beyond the key range feed nothing)
        const v4i pf = ks < nkt ? *reinterpret_cast<const v4i *>(strip + l31 * a.pitch + 32 * ks + 16 * h) : px80;
        bsum += bmm_bytesum(vf);
        acc = gc_mfma(vf, pf ^ px80, acc);  // D[j][m]
        fv = nv;
      }
      __syncthreads();  // the images are free: the sums below and the next pass's first image reuse their bytes
      {                 // compensation of the xor over the keys this wave has fed (the parts add up to the whole sum)
        const int comp_tot = 128 * (bsum + __shfl_xor(bsum, 32));
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] += __shfl(comp_tot, 8 * (i >> 2) + 4 * h + (i & 3));
      }
      if (a.kparts > 1) {  // (uniform; then items <= 4: one pass, every wave live)
        if (part > 0) {
          int *const mine = red + ((jt * (a.kparts - 1) + part - 1) * 16) * 64 + lane;
#pragma unroll
          for (int i = 0; i < 16; ++i) mine[i * 64] = acc[i];
        }
        __syncthreads();
        if (part == 0) {
          for (int pp = 1; pp < a.kparts; ++pp) {
            const int *const other = red + ((jt * (a.kparts - 1) + pp - 1) * 16) * 64 + lane;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] += other[i * 64];
          }
        }
        __syncthreads();
      }

      const int mrow = m0 + l31;
      const size_t obase = (size_t)(b0 * a.o_s0 + b1 * a.o_s1) + (size_t)mrow * (size_t)a.ldo;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int a4[4] = {acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
        const int n = n0 + 8 * q + 4 * h;  // the lane holds columns n .. n + 3 of its row m
        if (!live || part != 0 || mrow >= a.tq || n >= a.dv) continue;
        const v4i out = gc_quarter<DST, FO>(a4, v4f{0.0f, 0.0f, 0.0f, 0.0f}, *reinterpret_cast<const v4f *>(a.oscale + n), relu, a.rm);
        const int left = min(4, a.dv - n);
        if constexpr (ESZ == 1) {
          unsigned char *const p = a.o + obase + n;
          if (a.o_vec && left == 4) *reinterpret_cast<int *>(p) = out[0];
          else
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (j < left) p[j] = (unsigned char)((unsigned)out[0] >> (8 * j));
        } else {
          int *const p = reinterpret_cast<int *>(a.o) + obase + n;
          if (a.o_vec && left == 4) dfx_store16(reinterpret_cast<v4i *>(p), out);
          else
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (j < left) p[j] = out[j];
        }
      }
    }
    __syncthreads();  // the next strip's logits overwrite the strip this one's context has read
  }
}

}  // namespace dfx
