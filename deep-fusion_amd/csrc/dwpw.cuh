// dwpw.cuh -- depthwise 3x3 conv + pointwise 1x1 conv in ONE launch (dfx_dwpw_* of include/dfx.h; gfx950): the
// block of MobileNet / EfficientNet / Xception with the u8 tensor between its two convs kept in LDS.
//
// A workgroup of 256 lanes owns tiles of TH output rows x TW output columns of one image, tile = blockIdx.x +
// j * gridDim.x.  TW = 256 / (c / 16): every lane has one (column, 16-channel group), as in dwconv.cuh.
//   entry    the 1x1 weights (conv_pw.cuh's one-tap W0d image [oc/32][c/32][lane][16 B]) and the stage-1 constants
//            (comp | bias | scale) go to LDS by LDS-DMA and stay there for the whole launch.
//   phase A  dwconv.cuh's row loop for K = 3 (v_perm_b32 packing, v_dot4_i32_i8, clamped addresses, next row
//            prefetched); the lane's 16 requantised u8 bytes go with one ds_write_b128 into the `mid` tile
//            [tile pixel = row * TW + column][c], row pitch c + 16 bytes (an odd multiple of 16: the ds_read_b128 of
//            phase B, 32 pixels x 2 k-halves, is conflict-free).  The lane's depthwise weights and constants are
//            re-read from global memory (L1 / L2) at the start of every tile, so that they do not stay in registers
//            across phase B, whose accumulators need them.
//   barrier
//   phase B  conv_pw.cuh's MFMA loop and epilogue per block of 32 tile pixels, blocks dealt to the 4 waves: the B
//            fragment is a ds_read_b128 of `mid` ^ 0x80808080, A is the weight image, the accumulators start from the
//            integer compensation 128 * sum(w), so both requant routes add the plain f32 bias.  Rows are assembled in
//            a wave-private staging area and leave as 16 bytes per lane through DFX_STORE16.
//   barrier  before the next tile's phase A overwrites `mid`.
// The only synchronisation is the workgroup barrier, and every wave passes the same number of them: the tile loop's
// trip count depends on blockIdx alone, no lane returns early.  Lanes without a column (c = 96: 252 of 256 lanes
// work), columns beyond ow and the tile pixels of rows beyond oh compute on clamped addresses (or stale LDS) and are
// masked at the LDS write / the global store.
#pragma once

#include "conv_pw.cuh"
#include "dwconv.cuh"

namespace dfx {

constexpr int DWPW_THREADS = 256;

struct DwPwArgs {
  const unsigned char *src;
  unsigned char *dst;
  // stage 0 (the owned depthwise handle's buffers, dwconv_api.hip)
  const unsigned *wpk;   // [c/16][3][16] dwords
  const int *comp0;      // [c]
  const float *bias0, *scale0;
  // stage 1: [W0d | comp1[oc] | bias1[oc] | scale1[oc]], contiguous
  const unsigned char *w1;
  int bs, c, ih, iw, oh, ow, oc, pt, pl;
  int rm0, fast0;
  int relu1, rm1, fast1;
  int groups;            // c / 16
  int th, tw;            // tile
  int ty, tx;            // tiles per image along y / x
  int ntiles;            // bs * ty * tx
  int nblk;              // ceil(th * tw / 32): 32-pixel blocks of a tile
  unsigned tw_magic;     // floor(2^20 / tw) + 1: p / tw == (p * tw_magic) >> 20 for p < 2^11 (checked by the host)
  int mid_pitch;         // c + 16
  int off_cst, off_mid, off_stage, stage_bytes;  // LDS byte offsets
};

// dw_store's u8 branch, value for value, returning the 16 bytes instead of storing them
template <bool FAST>
__device__ __forceinline__ v4i dwpw_mid16(const int (&acc)[16], const float (&bias)[16], const float (&scale)[16], int rm) {
  v4i pk4;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    unsigned pk = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ch = 4 * g + j;
      const float f = __fmul_rn(__fadd_rn(__int2float_rn(acc[ch]), bias[ch]), scale[ch]);
      if (FAST) {
        pk = __builtin_amdgcn_cvt_pk_u8_f32(f, j, pk);  // nearest even, [0, 255]: subsumes the ReLU
      } else {
        pk |= sat_u8_bits(cvt_x86_rt(relu_x86(f), rm)) << (8 * j);
      }
    }
    pk4[g] = (int)pk;
  }
  return pk4;
}

template <int S, int OCB, int DST>
__global__ __launch_bounds__(DWPW_THREADS) void dwpw_kernel(DwPwArgs a) {
  constexpr int K = 3;
  constexpr int NA = (K + S - 1) / S;
  constexpr int U = NA * S;
  constexpr int ESZ = (DST == DFX_F32 || DST == DFX_S32) ? 4 : 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char *const w_lds = smem;
  const float *const cst = reinterpret_cast<const float *>(smem + a.off_cst);
  unsigned char *const mid = smem + a.off_mid;
  const int OC = 32 * OCB;
  const int *comp1 = reinterpret_cast<const int *>(cst);
  const float *bias1 = cst + OC, *scale1 = cst + 2 * OC;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, h = lane >> 5;
  const int icb = a.c >> 5;

  {  // 1x1 weights + constants -> LDS by LDS-DMA (1 KB per wave instruction), as conv_pw.cuh
    typedef __attribute__((address_space(3))) void lds_void;
    typedef __attribute__((address_space(1))) const void global_void;
    const int total16 = OCB * icb * 64 + 3 * OC / 4;  // 16-byte chunks
    const v4i *ws = reinterpret_cast<const v4i *>(a.w1);
    v4i *wd = reinterpret_cast<v4i *>(smem);
    for (int j = wave; 64 * j < total16; j += DWPW_THREADS / 64) {
      const int q = 64 * j + lane;
      if (q < total16) __builtin_amdgcn_global_load_lds((global_void *)(ws + q), (lds_void *)(wd + 64 * j), 16, 0, 0);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // phase A's lane: column xl of the tile, channel group g
  const int g = tid % a.groups;
  const int xl_raw = tid / a.groups;
  const bool has_col = xl_raw < a.tw;
  const int xl = has_col ? xl_raw : a.tw - 1;
  const int row_pitch = a.iw * a.c;  // one image is below 2^31 bytes (the class)
  const bool relu1 = a.relu1 != 0 || DST == DFX_U8;
  const v4i x80 = v4i{(int)0x80808080, (int)0x80808080, (int)0x80808080, (int)0x80808080};
  const unsigned row_bytes = (unsigned)OC * ESZ;
  unsigned char *const stg = smem + a.off_stage + wave * a.stage_bytes;
  const int tp_all = a.th * a.tw;

  // (unsigned: ntiles is below 2^31 and the grid far below that, so tile + gridDim.x cannot wrap)
  for (unsigned utile = blockIdx.x; utile < (unsigned)a.ntiles; utile += gridDim.x) {
    const int tile = (int)utile;
    const int n = tile / (a.ty * a.tx);
    const int trem = tile - n * (a.ty * a.tx);
    const int tyi = trem / a.tx, txi = trem - tyi * a.tx;
    const int oy0 = tyi * a.th, ox0 = txi * a.tw;
    const int nrows = min(a.th, a.oh - oy0);  // >= 1, the same for every lane of the workgroup

    {  // ---- phase A
      unsigned w[K][16];
      int comp[16];
      float bias[16], scale[16];
      {
        const v4i *wp = reinterpret_cast<const v4i *>(a.wpk) + (size_t)g * K * 4;
#pragma unroll
        for (int ky = 0; ky < K; ++ky)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const v4i v = wp[ky * 4 + q];
            w[ky][4 * q + 0] = (unsigned)v[0]; w[ky][4 * q + 1] = (unsigned)v[1];
            w[ky][4 * q + 2] = (unsigned)v[2]; w[ky][4 * q + 3] = (unsigned)v[3];
          }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const v4i cv = reinterpret_cast<const v4i *>(a.comp0)[(size_t)g * 4 + q];
          const v4f bv = reinterpret_cast<const v4f *>(a.bias0)[(size_t)g * 4 + q];
          const v4f sv = reinterpret_cast<const v4f *>(a.scale0)[(size_t)g * 4 + q];
#pragma unroll
          for (int j = 0; j < 4; ++j) { comp[4 * q + j] = cv[j]; bias[4 * q + j] = bv[j]; scale[4 * q + j] = sv[j]; }
        }
      }
      const int ox = min(ox0 + xl, a.ow - 1);  // a column beyond ow computes its neighbour's values; masked at the store
      const int iy0 = oy0 * S - a.pt, ix0 = ox * S - a.pl;
      DwPack<K> pk;
      bool valid[K];
      int xoff[K];
#pragma unroll
      for (int kx = 0; kx < K; ++kx) {
        const int ix = ix0 + kx;
        valid[kx] = ix >= 0 && ix < a.iw;
        xoff[kx] = min(max(ix, 0), a.iw - 1) * a.c;  // clamped: the address stays inside the image
      }
      pk.set(valid);
      const unsigned char *img = a.src + (size_t)n * a.ih * row_pitch + (size_t)g * 16;
      unsigned char *mid_lane = mid + xl * a.mid_pitch + 16 * g;
      const int mid_row = a.tw * a.mid_pitch;

      int acc[NA][16];
      v4i raw[K];
      auto load_row = [&](int r) {
        const unsigned char *rowp = img + min(max(iy0 + r, 0), a.ih - 1) * row_pitch;  // clamped
#pragma unroll
        for (int kx = 0; kx < K; ++kx) raw[kx] = *reinterpret_cast<const v4i *>(rowp + xoff[kx]);
      };
      const int rlast = (nrows - 1) * S + K - 1;
      load_row(0);
      for (int rb = 0; rb <= rlast; rb += U) {
        dw_static_for<U>([&](auto uc) {
          constexpr int u = decltype(uc)::value;
          const int r = rb + u;
          if (r > rlast) return;
          unsigned P[16];
          pk.pack(raw, iy0 + r >= 0 && iy0 + r < a.ih, P);
          load_row(r + 1);  // (clamped address: harmless past the tile's last row)
          dw_static_for<K>([&](auto kc) {
            constexpr int ky = decltype(kc)::value;
            if constexpr (dw_fmod(u - ky, S) == 0) {
              constexpr int d = dw_fdiv(u - ky, S);
              constexpr int set = dw_fmod(d, NA);
#pragma unroll
              for (int ch = 0; ch < 16; ++ch)
                acc[set][ch] = __builtin_amdgcn_sdot4((int)P[ch], (int)w[ky][ch], ky == 0 ? comp[ch] : acc[set][ch], false);
              if constexpr (ky == K - 1) {
                const int tt = rb / S + d;
                if (tt >= 0 && tt < nrows) {
                  const v4i m16 = a.fast0 ? dwpw_mid16<true>(acc[set], bias, scale, a.rm0)
                                          : dwpw_mid16<false>(acc[set], bias, scale, a.rm0);
                  if (has_col) *reinterpret_cast<v4i *>(mid_lane + tt * mid_row) = m16;
                }
              }
            }
          });
        });
      }
    }
    __syncthreads();

    // ---- phase B: 32-pixel blocks of the tile, dealt to the waves
    for (int blk = wave; blk < a.nblk; blk += DWPW_THREADS / 64) {
      v16i acc[OCB];
#pragma unroll
      for (int ob = 0; ob < OCB; ++ob)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const v4i iv = *reinterpret_cast<const v4i *>(comp1 + ob * 32 + 8 * q + 4 * h);
          acc[ob][4 * q + 0] = iv[0]; acc[ob][4 * q + 1] = iv[1]; acc[ob][4 * q + 2] = iv[2]; acc[ob][4 * q + 3] = iv[3];
        }
      // (the mid image is allocated for nblk * 32 pixels: the last block's tail reads stale LDS, masked below)
      const unsigned char *mp = mid + (32 * blk + l31) * a.mid_pitch + 16 * h;
      const unsigned char *wp = w_lds + lane * 16;
      for (int kb = 0; kb < icb; ++kb) {
        const v4i bfrag = *reinterpret_cast<const v4i *>(mp + 32 * kb) ^ x80;  // u8 -> s8
#pragma unroll
        for (int ob = 0; ob < OCB; ++ob) {
          const v4i wfrag = *reinterpret_cast<const v4i *>(wp + (ob * icb + kb) * 1024);
          acc[ob] = mfma_i8(wfrag, bfrag, acc[ob]);  // D[oc][px]
        }
      }
      // requant + store.  Lane = tile pixel 32 blk + l31; per output block and quarter q it holds channels
      // 8 q + 4 h .. + 3 (conv_pw.cuh).  cp4 = 0: the compensation is in the accumulator already.
      auto quarter = [&](int ob, int q) -> v4i {
        const int ch = ob * 32 + 8 * q + 4 * h;
        const v4f bs4 = *reinterpret_cast<const v4f *>(bias1 + ch);
        const v4f sc4 = *reinterpret_cast<const v4f *>(scale1 + ch);
        const v4i cp4 = {0, 0, 0, 0};
        int a4[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a4[i] = acc[ob][4 * q + i];
        return a.fast1 ? pw_quarter<DST, true>(a4, cp4, bs4, sc4, relu1, a.rm1, false)
                       : pw_quarter<DST, false>(a4, cp4, bs4, sc4, relu1, a.rm1, false);
      };
      // dst row of the tile pixel p of this block, or nullptr outside the image / the tile
      auto dst_row = [&](int p) -> unsigned char * {
        const int tp = 32 * blk + p;
        const int r = (int)(((unsigned)tp * a.tw_magic) >> 20), xx = tp - r * a.tw;
        if (tp >= tp_all || r >= nrows || ox0 + xx >= a.ow) return nullptr;
        return a.dst + (((size_t)n * a.oh + oy0 + r) * a.ow + ox0 + xx) * row_bytes;
      };
      if constexpr (ESZ == 1) {
        const int pitch = OC + 16;
#pragma unroll
        for (int ob = 0; ob < OCB; ++ob)
#pragma unroll
          for (int q = 0; q < 4; ++q)
            *reinterpret_cast<int *>(stg + l31 * pitch + ob * 32 + 8 * q + 4 * h) = quarter(ob, q)[0];
        constexpr int c16n = OC >> 4;  // 16-byte chunks per pixel row: 4, 8 or 16
        constexpr int sh = c16n == 4 ? 2 : c16n == 8 ? 3 : 4;
#pragma unroll
        for (int ck0 = 0; ck0 < 32 * c16n; ck0 += 64) {
          const int ck = ck0 + lane, row = ck >> sh, c16 = ck & (c16n - 1);
          const v4i val = *reinterpret_cast<const v4i *>(stg + row * pitch + 16 * c16);
          unsigned char *dp = dst_row(row);
          if (dp) DFX_STORE16(reinterpret_cast<v4i *>(dp + 16 * c16), val);
        }
      } else {
#pragma unroll
        for (int ob = 0; ob < OCB; ++ob) {
#pragma unroll
          for (int q = 0; q < 4; ++q) *reinterpret_cast<v4i *>(stg + l31 * 144 + 32 * q + 16 * h) = quarter(ob, q);
#pragma unroll
          for (int k = 0; k < 4; ++k) {  // 32 rows x 128 bytes = 256 chunks
            const int ck = lane + 64 * k, row = ck >> 3, c16 = ck & 7;
            const v4i val = *reinterpret_cast<const v4i *>(stg + row * 144 + 16 * c16);
            unsigned char *dp = dst_row(row);
            if (dp) DFX_STORE16(reinterpret_cast<v4i *>(dp + ob * 128 + 16 * c16), val);
          }
        }
      }
    }
    __syncthreads();  // the next tile's phase A overwrites mid
  }
}

}  // namespace dfx
