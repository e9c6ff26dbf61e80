// gconv.cuh -- the grouped int8 conv's MFMA kernel (dfx_gconv_* of include/dfx.h; gfx950): 3x3, stride 1 or 2,
// ic == oc a multiple of 32, ic / groups in {4, 8, 16, 32, 64} -- the 3x3 of a ResNeXt / RegNet block.
//
// One v_mfma_i32_32x32x32_i8 contracts a 32-channel block of inputs into a 32-channel block of outputs.  For
// cpg = ic / groups <= 32 every output block reads exactly ONE input block (its own) through a block-diagonal 32 x 32
// weight tile per tap, whose off-group bytes the host packs as zero: 9 MFMAs per 32 pixels x 32 channels whatever cpg
// is.  For cpg = 64 output block b reads input blocks 2 (b / 2) and 2 (b / 2) + 1: 18 MFMAs.  Per 1 KB of u8 in and
// 1 KB out that is 288 matrix cycles on one SIMD: the op is meant to be an HBM stream, not a matrix-bound kernel.
//   * Work item = (strip of 32 consecutive output pixels of the flattened {bs, oh, ow}, chunk of up to 4 channel
//     blocks).  128 channels make a pixel's u8 output one whole 128-byte line; chunks of one pixel read disjoint source
//     bytes, so chunking costs no re-reads.  A wave owns a strip; the 8 waves of a workgroup share the chunk, whose
//     fragments (36 KB, 72 KB at cpg 64) and constants are copied to LDS once per (workgroup, chunk).
//   * Lane (pixel p = lane & 31, half h = lane >> 5) loads, per tap, its 16 channel bytes of the tap's input pixel with
//     one global_load_dwordx4 (conv_pw.cuh's B operand), xors them to s8 and feeds the MFMA.  A tap outside the input
//     is the byte 0x00 BEFORE the xor -- the activation 0 -- so the compensation 128 * sum(w), the accumulator's start
//     value, is the same for every pixel.  Addresses are clamped into the tensor first: no lane forms one outside.
//   * The epilogue is conv_pw.cuh's: the lane holds, per quarter q of a block, channels 8 q + 4 h .. + 3 of its pixel;
//     rows are assembled in a wave-private LDS area and leave as 16 bytes per lane, whole lines (u8 / s8: the chunk's
//     128 bytes per pixel; 4-byte types: one block's 128 bytes per pixel at a time).
//   * Requant: the depthwise op's chain (dwconv.cuh dw_store), value for value; FAST swaps only the conversion.
#pragma once

#include "dfx_device.cuh"

namespace dfx {

constexpr int GC_THREADS = 512;             // 8 waves share a chunk's LDS image: two workgroups per CU at cpg <= 32
constexpr int GC_CHUNK = 4;            // channel blocks per chunk
constexpr int GC_STAGE_PITCH = 144;    // bytes per staged pixel row: 128 + 16 (odd multiple of 16: conflict-free rows)
constexpr int GC_STAGE_BYTES = 32 * GC_STAGE_PITCH;

struct GcArgs {
  const unsigned char *src;
  unsigned char *dst;
  const unsigned char *wpk;  // MFMA path: [ob][tap][input block of ob (1 | 2)][lane][16]: byte b of lane =
                             // W[oc = 32 ob + (lane & 31)][ic = 32 ib + 16 (lane >> 5) + b][tap], 0 outside oc's group
  const signed char *wraw;   // generic path: {oc, ic / groups, kh, kw} as given
  const int *comp;           // [oc] 128 * sum of the channel's weights
  const float *bias;         // [oc] f32 (0 without bias)
  const float *scale;        // [oc] (a single scale is expanded by the host)
  int bs, ic, ih, iw, oc, oh, ow, groups, kh, kw, sh, sw, pt, pl;
  int dst_dt, relu, rm;
  int fast;                  // requant route (0 exact, 1 fast)
  int cblocks, nchunks;      // MFMA: 32-channel blocks, chunks of GC_CHUNK of them
  int wblocks;               // MFMA: blocks the LDS image has room for: min(GC_CHUNK, cblocks)
  int strips, slots;         // MFMA: 32-pixel strips; workgroup slots per chunk (a slot's 8 waves stride over the strips)
  int px_total;              // bs * oh * ow
  // tile variant (gconv_mfma_tile_kernel; all 0 otherwise): an item is (image, band of t_tr output rows, block of t_tc
  // output columns); its input halo is t_ir x t_ic pixels of t_pp bytes each in LDS; t_items items per chunk
  int t_tr, t_tc, t_ir, t_ic, t_pp, t_nbands, t_ncb, t_items;
  long long items;           // generic: dst elements
};

__device__ __forceinline__ v16i gc_mfma(v4i a, v4i b, v16i c) { return __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, c, 0, 0, 0); }

// 4 consecutive channels of one pixel after requant: the packed dword (1-byte outputs, in [0]) or the four 4-byte bit
// patterns.  dwconv.cuh's dw_store, value for value.
template <int DST, bool FAST>
__device__ __forceinline__ v4i gc_quarter(const int (&acc)[4], const v4f bias, const v4f scale, bool relu, int rm) {
  v4i out = {0, 0, 0, 0};
  if (DST == DFX_U8 || DST == DFX_S8) {
    unsigned pk = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float f = __fmul_rn(__fadd_rn(__int2float_rn(acc[j]), bias[j]), scale[j]);
      if (FAST && DST == DFX_U8) {
        pk = __builtin_amdgcn_cvt_pk_u8_f32(f, j, pk);  // nearest even, [0, 255]: subsumes the ReLU
      } else if (FAST && relu) {                        // s8 with ReLU: [0, 127]
        pk = __builtin_amdgcn_cvt_pk_u8_f32(__builtin_amdgcn_fmed3f(f, 0.0f, 127.0f), j, pk);
      } else {
        const float fr = relu ? relu_x86(f) : f;
        const int v = FAST ? (int)__builtin_rintf(fr) : cvt_x86_rt(fr, rm);
        const unsigned b = (DST == DFX_U8) ? sat_u8_bits(v) : ((unsigned)sat_s8(v) & 0xffu);
        pk |= b << (8 * j);
      }
    }
    out[0] = (int)pk;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float f = __fmul_rn(__fadd_rn(__int2float_rn(acc[j]), bias[j]), scale[j]);
      f = relu ? relu_x86(f) : f;
      if (DST == DFX_F32) out[j] = __float_as_int(f);
      else out[j] = FAST ? (int)__builtin_rintf(f) : cvt_x86_rt(f, rm);
    }
  }
  return out;
}

// S: stride (1 | 2).  NIB: input blocks per output block (1: cpg <= 32, 2: cpg = 64).
// LDS: [weights of the chunk: wblocks * 9 * NIB KB][comp | bias | scale: 3 * 128 dwords][8 waves' staging].
template <int S, int NIB, int DST, bool FAST>
__global__ __launch_bounds__(GC_THREADS) void gconv_mfma_kernel(GcArgs a) {
  constexpr int ESZ = (DST == DFX_F32 || DST == DFX_S32) ? 4 : 1;
  constexpr int WBLK = 9 * NIB * 1024;  // bytes of one output block's fragments
  extern __shared__ __attribute__((aligned(16))) unsigned char gc_lds[];
  unsigned char *const w_lds = gc_lds;
  int *const comp_l = reinterpret_cast<int *>(gc_lds + a.wblocks * WBLK);
  float *const bias_l = reinterpret_cast<float *>(comp_l + 32 * GC_CHUNK);
  float *const scale_l = bias_l + 32 * GC_CHUNK;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  unsigned char *const stg = reinterpret_cast<unsigned char *>(scale_l + 32 * GC_CHUNK) + wave * GC_STAGE_BYTES;
  const int l31 = lane & 31, h = lane >> 5;
  const bool relu = a.relu != 0;
  const v4i x80 = v4i{(int)0x80808080, (int)0x80808080, (int)0x80808080, (int)0x80808080};
  const v4i zero4 = v4i{0, 0, 0, 0};
  const size_t row_bytes = (size_t)a.oc * ESZ;

  const int units = a.nchunks * a.slots;  // the same for every workgroup: the barriers below are uniform
  for (int u = blockIdx.x; u < units; u += gridDim.x) {
    const int chunk = u % a.nchunks, slot = u / a.nchunks;
    const int cb0 = chunk * GC_CHUNK, nb = min(GC_CHUNK, a.cblocks - cb0);
    __syncthreads();  // the previous unit's readers are done with the LDS image
    {
      const v4i *ws = reinterpret_cast<const v4i *>(a.wpk + (size_t)cb0 * WBLK);
      v4i *wd = reinterpret_cast<v4i *>(w_lds);
      const int n16 = nb * (WBLK / 16);
      for (int q = tid; q < n16; q += GC_THREADS) wd[q] = ws[q];
      for (int q = tid; q < 32 * nb; q += GC_THREADS) {
        comp_l[q] = a.comp[32 * cb0 + q];
        bias_l[q] = a.bias[32 * cb0 + q];
        scale_l[q] = a.scale[32 * cb0 + q];
      }
    }
    __syncthreads();

    for (int strip = slot * (GC_THREADS / 64) + wave; strip < a.strips; strip += a.slots * (GC_THREADS / 64)) {
      // this lane's output pixel (clamped to the last one: its loads stay inside the tensor, its rows are not stored).
      // int holds it: px_total <= 2^31 - 1 (validated), so strip <= 2^26 - 1 and 32 * strip + 31 <= 2^31 - 1.
      const int px = min(32 * strip + l31, a.px_total - 1);
      const int r = px / a.ow, ox = px - r * a.ow;
      const int n = r / a.oh, oy = r - n * a.oh;
      const int iy0 = oy * S - a.pt, ix0 = ox * S - a.pl;
      bool ok[9];
      size_t off[9];  // byte offset of the tap's pixel (clamped into the image), this lane's half of input block 0
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int iy = iy0 + ky, ix = ix0 + kx;
          ok[3 * ky + kx] = iy >= 0 && iy < a.ih && ix >= 0 && ix < a.iw;
          const int cy = min(max(iy, 0), a.ih - 1), cx = min(max(ix, 0), a.iw - 1);
          off[3 * ky + kx] = (((size_t)n * a.ih + cy) * a.iw + cx) * (size_t)a.ic + 16 * h;
        }
      const int nvalid = min(32, a.px_total - 32 * strip);
      unsigned char *const dst_strip = a.dst + (size_t)(32 * strip) * row_bytes + (size_t)cb0 * 32 * ESZ;

      for (int obl = 0; obl < nb; ++obl) {
        const int ib0 = (NIB == 2) ? ((cb0 + obl) & ~1) : (cb0 + obl);  // first input block of this output block
        v4i fx[9 * NIB];
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
          for (int j = 0; j < NIB; ++j) {
            const v4i v = *reinterpret_cast<const v4i *>(a.src + off[t] + (size_t)(ib0 + j) * 32);
            fx[t * NIB + j] = (ok[t] ? v : zero4) ^ x80;  // u8 -> s8; a skipped tap is the activation 0
          }
        v16i acc;
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // start value: the compensation of this lane's 16 channels
          const v4i cv = *reinterpret_cast<const v4i *>(comp_l + obl * 32 + 8 * q + 4 * h);
          acc[4 * q + 0] = cv[0]; acc[4 * q + 1] = cv[1]; acc[4 * q + 2] = cv[2]; acc[4 * q + 3] = cv[3];
        }
        const unsigned char *wl = w_lds + obl * WBLK + lane * 16;
#pragma unroll
        for (int t = 0; t < 9 * NIB; ++t) acc = gc_mfma(*reinterpret_cast<const v4i *>(wl + t * 1024), fx[t], acc);  // D[oc][px]

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
            if (row < nvalid) dfx_store16_nt(reinterpret_cast<v4i *>(dst_strip + (size_t)row * row_bytes + obl * 128 + 16 * c16), val);
          }
        }
      }
      if constexpr (ESZ == 1) {
        const int c16n = 2 * nb;  // 16-byte pieces per pixel of this chunk: 2, 4, 6 or 8
        for (int ck = lane; ck < 32 * c16n; ck += 64) {
          const int row = ck / c16n, c16 = ck - row * c16n;
          const v4i val = *reinterpret_cast<const v4i *>(stg + row * GC_STAGE_PITCH + 16 * c16);
          if (row < nvalid) dfx_store16_nt(reinterpret_cast<v4i *>(dst_strip + (size_t)row * row_bytes + 16 * c16), val);
        }
      }
    }
  }
}

// ---- the variant with the input staged in LDS (DFX_GCONV_TILE=1; DESIGN 4.9 "LDS tile versus direct load") ----------
// Same contraction, weights, requant and stores as gconv_mfma_kernel.  The difference is the input: a work item is
// (image, band of t_tr output rows, block of t_tc output columns) of one chunk; the workgroup first copies the item's
// halo -- t_ir x t_ic input pixels, the chunk's nb * 32 channel bytes of each, whole lines from global memory, already
// xor 0x80, positions outside the image as the byte 0x80 (the activation 0) -- into LDS, and after a barrier its waves
// take the item's output pixels 32 at a time and read every tap's B fragment from that tile with one 16-byte LDS load
// per lane.  Every source byte of the chunk is requested once per item (plus the halo) instead of once per tap.
// LDS: [weights][comp | bias | scale][8 waves' staging][tile: t_ir * t_ic * t_pp bytes].
template <int S, int NIB, int DST, bool FAST>
__global__ __launch_bounds__(GC_THREADS) void gconv_mfma_tile_kernel(GcArgs a) {
  constexpr int ESZ = (DST == DFX_F32 || DST == DFX_S32) ? 4 : 1;
  constexpr int WBLK = 9 * NIB * 1024;
  extern __shared__ __attribute__((aligned(16))) unsigned char gc_lds[];
  unsigned char *const w_lds = gc_lds;
  int *const comp_l = reinterpret_cast<int *>(gc_lds + a.wblocks * WBLK);
  float *const bias_l = reinterpret_cast<float *>(comp_l + 32 * GC_CHUNK);
  float *const scale_l = bias_l + 32 * GC_CHUNK;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  unsigned char *const stg0 = reinterpret_cast<unsigned char *>(scale_l + 32 * GC_CHUNK);
  unsigned char *const stg = stg0 + wave * GC_STAGE_BYTES;
  unsigned char *const tile = stg0 + (GC_THREADS / 64) * GC_STAGE_BYTES;
  const int l31 = lane & 31, h = lane >> 5;
  const bool relu = a.relu != 0;
  const v4i x80 = v4i{(int)0x80808080, (int)0x80808080, (int)0x80808080, (int)0x80808080};
  const size_t row_bytes = (size_t)a.oc * ESZ;

  const int units = a.nchunks * a.slots;  // the same for every workgroup: the barriers below are uniform
  for (int u = blockIdx.x; u < units; u += gridDim.x) {
    const int chunk = u % a.nchunks, slot = u / a.nchunks;
    const int cb0 = chunk * GC_CHUNK, nb = min(GC_CHUNK, a.cblocks - cb0);
    const int c16n = 2 * nb;  // 16-byte pieces per pixel of this chunk
    __syncthreads();  // the previous unit's readers are done with the LDS image
    {
      const v4i *ws = reinterpret_cast<const v4i *>(a.wpk + (size_t)cb0 * WBLK);
      v4i *wd = reinterpret_cast<v4i *>(w_lds);
      const int n16 = nb * (WBLK / 16);
      for (int q = tid; q < n16; q += GC_THREADS) wd[q] = ws[q];
      for (int q = tid; q < 32 * nb; q += GC_THREADS) {
        comp_l[q] = a.comp[32 * cb0 + q];
        bias_l[q] = a.bias[32 * cb0 + q];
        scale_l[q] = a.scale[32 * cb0 + q];
      }
    }
    for (int it = slot; it < a.t_items; it += a.slots) {  // uniform over the workgroup
      const int cbk = it % a.t_ncb, t2 = it / a.t_ncb;
      const int band = t2 % a.t_nbands, n = t2 / a.t_nbands;
      const int oy0 = band * a.t_tr, ox0 = cbk * a.t_tc;
      const int tc = min(a.t_tc, a.ow - ox0), npx = min(a.t_tr, a.oh - oy0) * tc;
      const int iyb = oy0 * S - a.pt, ixb = ox0 * S - a.pl;
      __syncthreads();  // the previous item's readers are done with the tile
      const int npiece = a.t_ir * a.t_ic * c16n;
      for (int q = tid; q < npiece; q += GC_THREADS) {
        const int pix = q / c16n, pc = q - pix * c16n;
        const int row = pix / a.t_ic, col = pix - row * a.t_ic;
        const int iy = iyb + row, ix = ixb + col;
        v4i v = v4i{0, 0, 0, 0};
        if (iy >= 0 && iy < a.ih && ix >= 0 && ix < a.iw)
          v = *reinterpret_cast<const v4i *>(a.src + (((size_t)n * a.ih + iy) * a.iw + ix) * (size_t)a.ic + (size_t)cb0 * 32 + 16 * pc);
        *reinterpret_cast<v4i *>(tile + pix * a.t_pp + 16 * pc) = v ^ x80;
      }
      __syncthreads();  // the tile (and, for the unit's first item, the weights) are in place

      // byte offset in dst of item pixel p's first byte of this chunk
      auto dst_off = [&](int p) -> size_t {
        const int r = p / tc, cx = p - r * tc;
        return ((((size_t)n * a.oh + oy0 + r) * a.ow + ox0 + cx) * row_bytes) + (size_t)cb0 * 32 * ESZ;
      };
      for (int strip = wave; 32 * strip < npx; strip += GC_THREADS / 64) {
        const int p = min(32 * strip + l31, npx - 1);  // clamped: reads stay inside the tile, its rows are not stored
        const int r = p / tc, cx = p - r * tc;
        const unsigned char *const tp = tile + ((r * S) * a.t_ic + cx * S) * a.t_pp + 16 * h;
        const int nvalid = min(32, npx - 32 * strip);

        for (int obl = 0; obl < nb; ++obl) {
          const int lb = (NIB == 2) ? (obl & ~1) : obl;  // first input block of this output block, within the chunk
          v4i fx[9 * NIB];
#pragma unroll
          for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
#pragma unroll
              for (int j = 0; j < NIB; ++j)
                fx[(3 * ky + kx) * NIB + j] = *reinterpret_cast<const v4i *>(tp + (ky * a.t_ic + kx) * a.t_pp + (lb + j) * 32);
          v16i acc;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const v4i cv = *reinterpret_cast<const v4i *>(comp_l + obl * 32 + 8 * q + 4 * h);
            acc[4 * q + 0] = cv[0]; acc[4 * q + 1] = cv[1]; acc[4 * q + 2] = cv[2]; acc[4 * q + 3] = cv[3];
          }
          const unsigned char *wl = w_lds + obl * WBLK + lane * 16;
#pragma unroll
          for (int t = 0; t < 9 * NIB; ++t) acc = gc_mfma(*reinterpret_cast<const v4i *>(wl + t * 1024), fx[t], acc);

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
            for (int k = 0; k < 4; ++k) {
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
}

}  // namespace dfx
