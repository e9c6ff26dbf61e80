// imgconv.cuh -- the first-layer int8 conv's MFMA kernel (dfx_imgconv_* of include/dfx.h; gfx950): a 3- or 4-channel u8
// NHWC image, window / stride 7x7 / 2, 3x3 / 1 or 3x3 / 2, oc a multiple of 32 up to 128 -- conv1 of ResNet / ResNeXt /
// DenseNet, VGG's conv1_1 and the MobileNet / EfficientNet / RegNet / Inception stems.
//
// The contraction is v_mfma_i32_32x32x32_i8 over K-steps of 8 input pixels x 4 bytes (imgconv_pack.h): a 7x7 window is
// 7 steps (one kernel row each: 7 taps and one zero-weight tap), a 3x3 window 2 steps (rows 0 and 1 in the two lane
// halves, then row 2 and zeros).  Activations are u8 xor 0x80; the compensation 128 * sum(w) is the accumulator's start
// value (gconv.cuh).  The 4th byte of a 3-channel pixel and every position outside the image hold 0x80 -- the
// activation 0 -- or meet a zero weight, so neither contributes.
//   * Work item = (image, band of t_tr output rows, block of t_tc <= 64 output columns).  The workgroup first copies
//     the item's halo -- t_ir input rows x t_icp pixels -- into LDS, repacked to 4 bytes per pixel and already xor 0x80.
//     A thread copies 4 pixels: the 12 or 16 source bytes start at ANY byte address (a 3-byte-pixel row is not dword
//     aligned, src itself need not be), so it loads the aligned dwords that cover them and shifts; where those dwords
//     would reach outside [src, src + bytes) -- the first and last bytes of the tensor -- it loads byte by byte,
//     bounds-checked.  No lane reads outside the tensor.
//   * After a barrier the 8 waves take the item's output pixels 32 at a time.  Lane (pixel p = lane & 31, half h) reads
//     per K-step the 16 LDS bytes of its 4 input pixels.  They start at byte 8 ox (+ 16) with stride 2 and 4 ox with
//     stride 1: 8- resp. 4-byte aligned only, so they are read as 2 x 8 resp. 4 x 4 bytes (a 16-byte LDS read off its
//     alignment is replayed).  The B fragments are loaded once per strip and serve every 32-channel block of oc.
//   * The weight fragments of all of oc (at most 4 blocks x 7 KB) and the constants sit in LDS for the whole launch.
//   * Epilogue, requant and stores are gconv.cuh's: rows are assembled in a wave-private LDS area and leave as 16 bytes
//     per lane through dfx_store16_nt, whole lines where oc allows.
#pragma once

#include "gconv.cuh"

namespace dfx {

constexpr int IC_THREADS = 512;
constexpr int IC_MAX_BLOCKS = 4;  // oc <= 128

struct IcArgs {
  const unsigned char *src;
  unsigned char *dst;
  const unsigned char *wpk;  // MFMA path: imgconv_pack.h's image
  const signed char *wraw;   // generic path: {oc, ic, kh, kw} as given
  const int *comp;           // [oc] 128 * sum of the channel's weights
  const float *bias;         // [oc] f32 (0 without bias)
  const float *scale;        // [oc] (a single scale is expanded by the host)
  int bs, ic, ih, iw, oc, oh, ow, kh, kw, sh, sw, pt, pl;
  int dst_dt, relu, rm;
  int fast;                  // requant route (0 exact, 1 fast)
  int cblocks;               // MFMA: 32-channel blocks of oc
  // MFMA: an item is (image, band of t_tr output rows, block of t_tc output columns); its halo is t_ir rows of t_icp
  // pixels (a multiple of 4) of 4 bytes each; t_items items in all
  int t_tr, t_tc, t_ir, t_icp, t_nbands, t_ncb, t_items;
  long long src_total;       // bytes of src
  long long items;           // generic: dst elements
};

typedef int v2i __attribute__((ext_vector_type(2)));

// 4 consecutive pixels of IC bytes each, starting `off` bytes into src (any alignment; off may lie outside the tensor
// for the pixels the caller masks), as 4 dwords with the pixel's channels in the low IC bytes.
template <int IC>
__device__ __forceinline__ v4i ic_load4(const unsigned char *src, long long off, long long total) {
  unsigned d[4] = {0, 0, 0, 0};  // the 4 * IC bytes, little endian (d[3] unused for IC == 3)
  const int mis = (int)(((long long)reinterpret_cast<uintptr_t>(src) + off) & 3);
  const long long lo = off - mis;
  if (lo >= 0 && lo + 4 * (IC + 1) <= total) {
    const unsigned *p = reinterpret_cast<const unsigned *>(src + lo);  // 4-byte aligned
    unsigned w[IC + 1];
#pragma unroll
    for (int i = 0; i <= IC; ++i) w[i] = p[i];
#pragma unroll
    for (int i = 0; i < IC; ++i) d[i] = (unsigned)(((((unsigned long long)w[i + 1]) << 32) | w[i]) >> (8 * mis));
  } else {
#pragma unroll
    for (int b = 0; b < 4 * IC; ++b) {
      const long long o = off + b;
      const unsigned v = (o >= 0 && o < total) ? src[o] : 0u;
      d[b >> 2] |= v << (8 * (b & 3));
    }
  }
  v4i px;
  if (IC == 4) {
    px = v4i{(int)d[0], (int)d[1], (int)d[2], (int)d[3]};
  } else {
    px[0] = (int)(d[0] & 0xffffffu);
    px[1] = (int)(((d[0] >> 24) | (d[1] << 8)) & 0xffffffu);
    px[2] = (int)(((d[1] >> 16) | (d[2] << 16)) & 0xffffffu);
    px[3] = (int)(d[2] >> 8);
  }
  return px;
}

// K: window (7 | 3).  S: stride (1 | 2).
// LDS: [weights: cblocks * NT KB][comp | bias | scale: 3 * 128 dwords][8 waves' staging][tile: t_ir * t_icp * 4 bytes].
template <int K, int S, int DST, bool FAST>
__global__ __launch_bounds__(IC_THREADS) void imgconv_mfma_kernel(IcArgs a) {
  constexpr int ESZ = (DST == DFX_F32 || DST == DFX_S32) ? 4 : 1;
  constexpr int NT = K == 7 ? 7 : 2;  // imgconv_pack_steps
  extern __shared__ __attribute__((aligned(16))) unsigned char ic_lds[];
  unsigned char *const w_lds = ic_lds;
  int *const comp_l = reinterpret_cast<int *>(ic_lds + a.cblocks * NT * 1024);
  float *const bias_l = reinterpret_cast<float *>(comp_l + 32 * IC_MAX_BLOCKS);
  float *const scale_l = bias_l + 32 * IC_MAX_BLOCKS;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  unsigned char *const stg0 = reinterpret_cast<unsigned char *>(scale_l + 32 * IC_MAX_BLOCKS);
  unsigned char *const stg = stg0 + wave * GC_STAGE_BYTES;
  unsigned char *const tile = stg0 + (IC_THREADS / 64) * GC_STAGE_BYTES;
  const int l31 = lane & 31, h = lane >> 5;
  const bool relu = a.relu != 0;
  const v4i x80 = v4i{(int)0x80808080, (int)0x80808080, (int)0x80808080, (int)0x80808080};
  const size_t row_bytes = (size_t)a.oc * ESZ;
  const int nb = a.cblocks, c16n = 2 * nb;  // 16-byte pieces per pixel of a 1-byte dst
  const int gpr = a.t_icp >> 2;             // 4-pixel groups per tile row

  {  // the whole op's weights and constants, once per workgroup (published by the first item's barrier)
    const v4i *ws = reinterpret_cast<const v4i *>(a.wpk);
    v4i *wd = reinterpret_cast<v4i *>(w_lds);
    for (int q = tid; q < nb * NT * 64; q += IC_THREADS) wd[q] = ws[q];
    for (int q = tid; q < 32 * nb; q += IC_THREADS) {
      comp_l[q] = a.comp[q];
      bias_l[q] = a.bias[q];
      scale_l[q] = a.scale[q];
    }
  }
  for (int it = blockIdx.x; it < a.t_items; it += gridDim.x) {  // uniform over the workgroup
    const int cbk = it % a.t_ncb, t2 = it / a.t_ncb;
    const int band = t2 % a.t_nbands, n = t2 / a.t_nbands;
    const int oy0 = band * a.t_tr, ox0 = cbk * a.t_tc;
    const int tc = min(a.t_tc, a.ow - ox0), npx = min(a.t_tr, a.oh - oy0) * tc;
    const int iyb = oy0 * S - a.pt, ixb = ox0 * S - a.pl;
    __syncthreads();  // the previous item's readers are done with the tile
    for (int q = tid; q < a.t_ir * gpr; q += IC_THREADS) {
      const int row = q / gpr, g = q - row * gpr;
      const int iy = iyb + row, ix = ixb + 4 * g;
      v4i v = v4i{0, 0, 0, 0};  // outside the image: the byte 0x00 before the xor, the activation 0
      if (iy >= 0 && iy < a.ih && ix + 3 >= 0 && ix < a.iw) {
        const long long off = (((long long)n * a.ih + iy) * a.iw + ix) * a.ic;
        const v4i ld = a.ic == 4 ? ic_load4<4>(a.src, off, a.src_total) : ic_load4<3>(a.src, off, a.src_total);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (ix + j >= 0 && ix + j < a.iw) ? ld[j] : 0;
      }
      *reinterpret_cast<v4i *>(tile + (size_t)(row * a.t_icp + 4 * g) * 4) = v ^ x80;
    }
    __syncthreads();  // the tile (and, for the first item, the weights) are in place

    // byte offset in dst of item pixel p's first byte
    auto dst_off = [&](int p) -> size_t {
      const int r = p / tc, cx = p - r * tc;
      return (((size_t)n * a.oh + oy0 + r) * a.ow + ox0 + cx) * row_bytes;
    };
    for (int strip = wave; 32 * strip < npx; strip += IC_THREADS / 64) {
      const int p = min(32 * strip + l31, npx - 1);  // clamped: reads stay inside the tile, its rows are not stored
      const int r = p / tc, cx = p - r * tc;
      const int nvalid = min(32, npx - 32 * strip);
      v4i fx[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int ky = K == 7 ? t : (t == 0 ? h : 2), kx0 = K == 7 ? 4 * h : 0;  // imgconv_pack_tap
        const unsigned char *tp = tile + (size_t)((r * S + ky) * a.t_icp + cx * S + kx0) * 4;
        if constexpr (S == 2) {  // 8-byte aligned
          const v2i lo = *reinterpret_cast<const v2i *>(tp), hi = *reinterpret_cast<const v2i *>(tp + 8);
          fx[t] = v4i{lo[0], lo[1], hi[0], hi[1]};
        } else {                 // 4-byte aligned
          const int *ip = reinterpret_cast<const int *>(tp);
          fx[t] = v4i{ip[0], ip[1], ip[2], ip[3]};
        }
      }
      for (int obl = 0; obl < nb; ++obl) {
        v16i acc;
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // start value: the compensation of this lane's 16 channels
          const v4i cv = *reinterpret_cast<const v4i *>(comp_l + obl * 32 + 8 * q + 4 * h);
          acc[4 * q + 0] = cv[0]; acc[4 * q + 1] = cv[1]; acc[4 * q + 2] = cv[2]; acc[4 * q + 3] = cv[3];
        }
        const unsigned char *wl = w_lds + obl * NT * 1024 + lane * 16;
#pragma unroll
        for (int t = 0; t < NT; ++t) acc = gc_mfma(*reinterpret_cast<const v4i *>(wl + t * 1024), fx[t], acc);  // D[oc][px]

        auto quarter = [&](int q) -> v4i {
          const int ch = obl * 32 + 8 * q + 4 * h;
          const v4f bs4 = *reinterpret_cast<const v4f *>(bias_l + ch);
          const v4f sc4 = *reinterpret_cast<const v4f *>(scale_l + ch);
          const int a4[4] = {acc[4 * q + 0], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
          return gc_quarter<DST, FAST>(a4, bs4, sc4, relu, a.rm);
        };
        if constexpr (ESZ == 1) {
#pragma unroll
          for (int q = 0; q < 4; ++q) *reinterpret_cast<int *>(stg + l31 * GC_STAGE_PITCH + obl * 32 + 8 * q + 4 * h) = quarter(q)[0];
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) *reinterpret_cast<v4i *>(stg + l31 * GC_STAGE_PITCH + 32 * q + 16 * h) = quarter(q);
#pragma unroll
          for (int k = 0; k < 4; ++k) {  // 32 rows x 128 bytes = 256 chunks of 16
            const int ck = lane + 64 * k, row = ck >> 3, c16 = ck & 7;
            const v4i val = *reinterpret_cast<const v4i *>(stg + row * GC_STAGE_PITCH + 16 * c16);
            if (row < nvalid) dfx_store16_nt(reinterpret_cast<v4i *>(a.dst + dst_off(32 * strip + row) + obl * 128 + 16 * c16), val);
          }
        }
      }
      if constexpr (ESZ == 1) {
        for (int ck = lane; ck < 32 * c16n; ck += 64) {
          const int row = ck / c16n, c16 = ck - row * c16n;
          const v4i val = *reinterpret_cast<const v4i *>(stg + row * GC_STAGE_PITCH + 16 * c16);
          if (row < nvalid) dfx_store16_nt(reinterpret_cast<v4i *>(a.dst + dst_off(32 * strip + row) + 16 * c16), val);
        }
      }
    }
  }
}

}  // namespace dfx
