// catconv_pw.cuh -- channel concat + POINTWISE conv in one launch (dfx_catconv_*): conv_pw.cuh's kernel with the
// concat folded into its address computation (gfx950 / CDNA4).  The concatenated tensor never exists.
//
// conv_pw.cuh needs no input tile: lane (pixel p, k half h) loads its 16 bytes of every 32-channel k-block straight
// from global memory into the MFMA B operand.  Nothing there needs a pixel's channels to be contiguous in ONE buffer,
// only the pointer arithmetic assumes it.  Here k-block kb of the concatenated channel axis lives in branch s(kb), at
// byte offset off(kb) of that branch's pixel rows of channels[s(kb)] bytes; the lane's address is
//     src[s(kb)] + off(kb) + px * channels[s(kb)] + 16 h
// The HOST resolves the first two terms and the row pitch per k-block, once per submit, into a table of
// {pointer, pitch} that travels in the kernel arguments (CatTab, <= 48 entries of 16 bytes): the kernel never sees a
// branch index.  A k-block's entry is wave-uniform -- one scalar 16-byte load from the kernel-argument segment -- and
// the lane's address is one 32-bit multiply-add on top of it.  The entries of the chunk that is fetched NEXT are read
// and multiplied before the MFMA group of the current chunk, so neither the scalar loads nor the multiplies sit
// between the MFMAs and the global loads they feed.
// Kept from conv_pw.cuh, line for line: weights + constants resident in LDS by LDS-DMA, a wave owns 32-pixel blocks
// b = wave id, + #waves, ..., a ring of two 4-k-block chunks in flight across block ends (past its last block a wave
// re-reads ITS OWN block), the requant routes (pw_quarter) and the row assembly in a wave-private LDS area with
// 16-byte stores.  Given up: the immediate offsets 0 / 32 / 64 / 96 of a chunk's four loads (each load has its own
// address register pair here, 8 VGPRs per ring set).
// Covered: every branch a multiple of 32 channels (a pixel's two lanes read one whole 32-byte sector), and conv_pw.cuh's
// limits for the sum: ic a multiple of 256, oc in {64, 128, 256}, oc * ic <= 96 KB; px * pitch < 2^31 per branch.
#pragma once

#include "conv_pw.cuh"

namespace dfx {

constexpr int CAT_MAX_KB = 48;  // k-blocks of the concatenated axis: 96 KB / (64 oc * 32)

struct CatKb {
  const unsigned char *p;  // branch base + byte offset of this k-block inside a pixel row
  unsigned pitch;          // bytes per pixel row of that branch
  unsigned pad_;
};
struct CatTab {
  CatKb kb[CAT_MAX_KB];
};

template <int OCB, int DST>
__global__ __launch_bounds__(PW_THREADS, 2) void catconv_pw_kernel(ConvArgs a, PwGeom g, CatTab t) {
  constexpr int ESZ = (DST == DFX_F32 || DST == DFX_S32) ? 4 : 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char *const w_lds = smem;                                   // W0d[ob][kb][lane][16]
  const float *const cst = reinterpret_cast<const float *>(smem + g.off_cst);
  const int OCP = 32 * g.ocb;
  const int *comp0 = reinterpret_cast<const int *>(cst);
  const float *bias0 = cst + OCP, *scale0 = cst + 2 * OCP;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, h = lane >> 5;

  {  // weights + constants -> LDS by LDS-DMA (1 KB per wave instruction); [W0d | consts] is contiguous in global memory
    typedef __attribute__((address_space(3))) void lds_void;
    typedef __attribute__((address_space(1))) const void global_void;
    const int wq = g.ocb * g.icb * 64;                  // 16-byte chunks of weights
    const int total16 = wq + 3 * OCP / 4;
    const v4i *ws = reinterpret_cast<const v4i *>(a.wei);
    const v4i *cs = reinterpret_cast<const v4i *>(a.consts);
    v4i *wd = reinterpret_cast<v4i *>(smem);
    for (int j = wave; 64 * j < total16; j += PW_THREADS / 64) {
      const int q = 64 * j + lane;
      if (q < wq) __builtin_amdgcn_global_load_lds((global_void *)(ws + q), (lds_void *)(wd + 64 * j), 16, 0, 0);
      else if (q < total16) __builtin_amdgcn_global_load_lds((global_void *)(cs + (q - wq)), (lds_void *)(wd + 64 * j), 16, 0, 0);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const int gw = blockIdx.x * (PW_THREADS / 64) + wave, GW = gridDim.x * (PW_THREADS / 64);
  const int nch = g.icb / PW_CH;  // chunks per block (even: ic is a multiple of 256)
  const bool relu0 = a.relu0 != 0 || DST == DFX_U8;
  const bool fast = g.fast != 0, fma0 = DST == DFX_U8 && g.m0 != 0;
  const v4i x80 = v4i{(int)0x80808080, (int)0x80808080, (int)0x80808080, (int)0x80808080};
  const v16i zero16 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  unsigned char *const dst_b = reinterpret_cast<unsigned char *>(a.dst);
  const unsigned row_bytes = (unsigned)a.oc * ESZ;
  int wa[OCB];
#pragma unroll
  for (int ob = 0; ob < OCB; ++ob) wa[ob] = lane * 16 + ob * g.icb * 1024;

  auto pixel = [&](int b) -> unsigned {  // this lane's pixel of block b (clamped to the last pixel)
    return (unsigned)min(32 * b + l31, g.px_total - 1);
  };
  // the four addresses of chunk `c` for pixel `px`: table entry + px * pitch + 16 h (32-bit offset, checked by the host)
  const unsigned char *ad[PW_CH];
  auto address = [&](unsigned px, int c) {
#pragma unroll
    for (int j = 0; j < PW_CH; ++j) {
      const CatKb e = t.kb[c * PW_CH + j];
      ad[j] = e.p + (px * e.pitch + 16u * (unsigned)h);
    }
  };
  v4i fx[2][PW_CH];
  auto fetch = [&](int set) {
#pragma unroll
    for (int j = 0; j < PW_CH; ++j) fx[set][j] = *reinterpret_cast<const v4i *>(ad[j]);
  };
  if (gw >= g.n_blocks) return;
  unsigned xp = pixel(gw);
  address(xp, 0);
  fetch(0);
  address(xp, 1);
  fetch(1);
  for (int b = gw; b < g.n_blocks; b += GW) {
    // (past the wave's last block: a harmless re-read of ITS OWN block, as in conv_pw.cuh)
    const unsigned xn = pixel(b + GW < g.n_blocks ? b + GW : b);
    v16i acc[OCB];
    if (fma0) {  // "fma": start from bits(2^23) + comp + bias of this lane's 16 channels (comp slot of the constants)
#pragma unroll
      for (int ob = 0; ob < OCB; ++ob)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const v4i iv = *reinterpret_cast<const v4i *>(comp0 + ob * 32 + 8 * q + 4 * h);
          acc[ob][4 * q + 0] = iv[0]; acc[ob][4 * q + 1] = iv[1]; acc[ob][4 * q + 2] = iv[2]; acc[ob][4 * q + 3] = iv[3];
        }
    } else {
#pragma unroll
      for (int ob = 0; ob < OCB; ++ob) acc[ob] = zero16;
    }
    for (int c = 0; c < nch; c += 2) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int cc = c + s;  // this chunk; its ring set is s (nch is even)
        // addresses of the chunk two ahead (of this block, or the first two of the wave's next block): ahead of the MFMAs
        const int ca = cc + 2;
        if (ca < nch) address(xp, ca);
        else address(xn, ca - nch);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < PW_CH; ++j) {
          const v4i bfrag = fx[s][j] ^ x80;  // u8 -> s8 (the exact compensation 128 * sum(w) is in comp0)
#pragma unroll
          for (int ob = 0; ob < OCB; ++ob) {
            const v4i wfrag = *reinterpret_cast<const v4i *>(w_lds + wa[ob] + (cc * PW_CH + j) * 1024);
            acc[ob] = mfma_i8(wfrag, bfrag, acc[ob]);  // D[oc][px]
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        fetch(s);  // refill this set
      }
    }
    // ---- requant + store: conv_pw.cuh's epilogue (rows assembled in a wave-private LDS area, 16 bytes per lane out)
    unsigned char *stg = smem + g.off_stage + wave * g.stage_bytes;
    const int nvalid = min(32, g.px_total - 32 * b);
    unsigned char *dst_blk = dst_b + (size_t)(32 * b) * row_bytes;
    auto quarter = [&](int ob, int q) -> v4i {
      const int ch = ob * 32 + 8 * q + 4 * h;
      const v4f bs4 = *reinterpret_cast<const v4f *>(bias0 + ch);
      const v4f sc4 = *reinterpret_cast<const v4f *>(scale0 + ch);
      v4i cp4 = {0, 0, 0, 0};
      if (!fast) cp4 = *reinterpret_cast<const v4i *>(comp0 + ch);
      int a4[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a4[i] = acc[ob][4 * q + i];
      return fast ? pw_quarter<DST, true>(a4, cp4, bs4, sc4, relu0, a.rm0, fma0) : pw_quarter<DST, false>(a4, cp4, bs4, sc4, relu0, a.rm0, fma0);
    };
    if constexpr (ESZ == 1) {
      const int pitch = a.oc + 16;  // (row pitch of the staging: odd multiple of 16 for oc = 64 / 128 / 256)
#pragma unroll
      for (int ob = 0; ob < OCB; ++ob)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          *reinterpret_cast<int *>(stg + l31 * pitch + ob * 32 + 8 * q + 4 * h) = quarter(ob, q)[0];
      const int c16n = a.oc >> 4;  // 16-byte chunks per pixel row: 4, 8 or 16 (a power of two)
      const int sh = c16n == 4 ? 2 : c16n == 8 ? 3 : 4;
      for (int ck = lane; ck < 32 * c16n; ck += 64) {
        const int row = ck >> sh, c16 = ck & (c16n - 1);
        const v4i val = *reinterpret_cast<const v4i *>(stg + row * pitch + 16 * c16);
        if (row < nvalid) DFX_STORE16(reinterpret_cast<v4i *>(dst_blk + (size_t)row * row_bytes + 16 * c16), val);
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
          if (row < nvalid) DFX_STORE16(reinterpret_cast<v4i *>(dst_blk + (size_t)row * row_bytes + ob * 128 + 16 * c16), val);
        }
      }
    }
    xp = xn;
  }
}

}  // namespace dfx
