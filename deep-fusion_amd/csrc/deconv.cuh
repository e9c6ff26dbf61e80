// deconv.cuh -- the int8 transposed conv's MFMA kernel (dfx_deconv_* of include/dfx.h; gfx950): stride 2, window 2x2
// (pad 0), 4x4 (pad <= 3) or 3x3 (pad <= 2, packed as a 4x4 window whose last row and column are zero), ic and oc
// multiples of 32 -- the up-conv of a U-Net, a pose head or a DCGAN generator.
//
// Sub-pixel decomposition.  Write an output row as oy = 2 yb + a - pad_t with the "base" row yb = (oy + pad_t) / 2 and
// the parity a = (oy + pad_t) % 2, likewise ox = 2 xb + b - pad_l.  The taps that reach (oy, ox) are ky = a + 2 j,
// kx = b + 2 l with j, l < T (T = 1 for 2x2, 2 for 4x4), from the input pixel (yb - j, xb - l).  So base pixel (yb, xb)
// owns a 2 x 2 quad of output pixels, all four computed from the SAME T x T input pixels, each with its own sub-kernel
// w[:, :, a + 2 j, b + 2 l]: four dense T x T convs of the un-stuffed input.  No zero is multiplied, nothing is stuffed.
//   * Work item = (strip of 32 consecutive base pixels of the flattened {bs, YB, XB} base grid, chunk of up to DC_CHUNK
//     32-channel output blocks).  A wave owns a strip; the waves of a workgroup share the chunk, whose fragments -- all
//     four parities, every K-step -- and constants are copied to LDS once per (workgroup, chunk).
//   * Lane (pixel p = lane & 31, half h = lane >> 5) loads, per K-step of 32 input channels, its 16 channel bytes of
//     each of the T x T input pixels with one 16-byte load from global memory (a pixel is a multiple of 32 bytes, so
//     the shifted loads stay aligned), xors them to s8 and feeds them to the 4 T^2 MFMAs of the four parities: every
//     loaded fragment is used by every parity.  A pixel outside the input is the byte 0x00 BEFORE the xor -- the
//     activation 0 -- so the compensation 128 * sum(w over the parity's taps), the accumulator's start value, is the
//     same for every pixel.  Addresses are clamped into the tensor first: no lane forms one outside.
//   * Epilogue, per (block, parity): gconv.cuh's -- rows are assembled in a wave-private LDS area and leave as 16 bytes
//     per lane, 32 (1-byte dst) or 128 (4-byte dst) contiguous bytes per pixel; the two x-parities of a row, stored back
//     to back, are adjacent output pixels.  Quad members outside {oh, ow} (pad, odd / cropped sizes) are not stored.
//   * Requant: gconv.cuh's gc_quarter, value for value; FAST swaps only the conversion.
//   * Every loop over work is grid-stride; no flags, spin-waits or atomics.
#pragma once

#include "gconv.cuh"

namespace dfx {

constexpr int DC_THREADS = 256;  // 4 waves share a chunk's LDS image
constexpr int DC_CHUNK = 4;      // output-channel blocks per chunk at most (fewer where the LDS plan has no room)
constexpr int DC_FIXED_LDS = 6 * 32 * DC_CHUNK * 4 + (DC_THREADS / 64) * GC_STAGE_BYTES;  // constants + staging

struct DcArgs {
  const unsigned char *src;
  unsigned char *dst;
  const unsigned char *wpk;  // MFMA path: deconv_pack.h's image
  const signed char *wraw;   // generic path: {oc, ic, kh, kw} as given
  const int *comp;           // MFMA path: [4 parities a * 2 + b][oc] 128 * sum of the parity's weights of the channel
  const float *bias;         // [oc] f32 (0 without bias)
  const float *scale;        // [oc] (a single scale is expanded by the host)
  int bs, ic, ih, iw, oc, oh, ow, kh, kw, sh, sw, pt, pl;
  int dst_dt, relu, rm;
  int fast;                  // requant route (0 exact, 1 fast)
  int cblocks, nchunks;      // MFMA: 32-channel output blocks; chunks of wblocks of them
  int wblocks;               // MFMA: blocks the LDS image has room for
  int ksteps;                // MFMA: ic / 32
  int yb0, xb0, YB, XB;      // MFMA: first base row / column, base rows / columns
  int bp_total;              // MFMA: bs * YB * XB base pixels
  int strips, slots;         // MFMA: 32-pixel strips; workgroup slots per chunk (a slot's waves stride over the strips)
  long long items;           // generic: dst elements
};

// T: taps per axis and parity (1: 2x2 window, 2: 4x4).
// LDS: [weights of the chunk: wblocks * ksteps * 4 T^2 KB][comp: 4 x 128 dwords | bias | scale: 128 dwords each][staging].
template <int T, int DST, bool FAST>
__global__ __launch_bounds__(DC_THREADS) void deconv_mfma_kernel(DcArgs a) {
  constexpr int ESZ = (DST == DFX_F32 || DST == DFX_S32) ? 4 : 1;
  constexpr int KSTEP = 4 * T * T * 1024;  // bytes of one K-step's fragments of one output block
  extern __shared__ __attribute__((aligned(16))) unsigned char dc_lds[];
  const int wblk = a.ksteps * KSTEP;
  unsigned char *const w_lds = dc_lds;
  int *const comp_l = reinterpret_cast<int *>(dc_lds + (size_t)a.wblocks * wblk);  // [parity][32 * DC_CHUNK]
  float *const bias_l = reinterpret_cast<float *>(comp_l + 4 * 32 * DC_CHUNK);
  float *const scale_l = bias_l + 32 * DC_CHUNK;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  unsigned char *const stg = reinterpret_cast<unsigned char *>(scale_l + 32 * DC_CHUNK) + wave * GC_STAGE_BYTES;
  const int l31 = lane & 31, h = lane >> 5;
  const bool relu = a.relu != 0;
  const v4i x80 = v4i{(int)0x80808080, (int)0x80808080, (int)0x80808080, (int)0x80808080};
  const v4i zero4 = v4i{0, 0, 0, 0};
  const long long row_bytes = (long long)a.oc * ESZ;

  const int units = a.nchunks * a.slots;  // the same for every workgroup: the barriers below are uniform
  for (int u = blockIdx.x; u < units; u += gridDim.x) {
    const int chunk = u % a.nchunks, slot = u / a.nchunks;
    const int cb0 = chunk * a.wblocks, nb = min(a.wblocks, a.cblocks - cb0);
    __syncthreads();  // the previous unit's readers are done with the LDS image
    {
      const v4i *ws = reinterpret_cast<const v4i *>(a.wpk + (size_t)cb0 * wblk);
      v4i *wd = reinterpret_cast<v4i *>(w_lds);
      const int n16 = nb * (wblk / 16);
      for (int q = tid; q < n16; q += DC_THREADS) wd[q] = ws[q];
      for (int q = tid; q < 32 * nb; q += DC_THREADS) {
#pragma unroll
        for (int par = 0; par < 4; ++par) comp_l[par * 32 * DC_CHUNK + q] = a.comp[(size_t)par * a.oc + 32 * cb0 + q];
        bias_l[q] = a.bias[32 * cb0 + q];
        scale_l[q] = a.scale[32 * cb0 + q];
      }
    }
    __syncthreads();

    for (int strip = slot * (DC_THREADS / 64) + wave; strip < a.strips; strip += a.slots * (DC_THREADS / 64)) {
      // this lane's base pixel (clamped to the last one: its loads stay inside the tensor, its quad is not stored).
      // int holds it: bp_total <= bs * oh * ow <= 2^31 - 1 (validated).
      const bool lane_live = 32 * strip + l31 < a.bp_total;
      const int bp = min(32 * strip + l31, a.bp_total - 1);
      const int r = bp / a.XB, xb = bp - r * a.XB + a.xb0;
      const int n = r / a.YB, yb = r - n * a.YB + a.yb0;
      bool ok[T * T];
      size_t off[T * T];  // byte offset of the tap's input pixel (clamped into the image), this lane's half of K-step 0
#pragma unroll
      for (int j = 0; j < T; ++j)
#pragma unroll
        for (int l = 0; l < T; ++l) {
          const int iy = yb - j, ix = xb - l;
          ok[j * T + l] = iy >= 0 && iy < a.ih && ix >= 0 && ix < a.iw;
          const int cy = min(max(iy, 0), a.ih - 1), cx = min(max(ix, 0), a.iw - 1);
          off[j * T + l] = (((size_t)n * a.ih + cy) * a.iw + cx) * (size_t)a.ic + 16 * h;
        }
      // the quad: output pixel (2 yb - pt + a, 2 xb - pl + b); bit a * 2 + b of `live`: it exists and is this lane's
      const int oy0 = 2 * yb - a.pt, ox0 = 2 * xb - a.pl;
      const long long obase = (((long long)n * a.oh + oy0) * a.ow + ox0) * row_bytes;  // may lie outside: used with `live` only
      int live = 0;
#pragma unroll
      for (int par = 0; par < 4; ++par) {
        const int oy = oy0 + (par >> 1), ox = ox0 + (par & 1);
        if (lane_live && oy >= 0 && oy < a.oh && ox >= 0 && ox < a.ow) live |= 1 << par;
      }
      const int ob_lo = (int)(unsigned)(obase & 0xffffffffll), ob_hi = (int)(obase >> 32);

      for (int obl = 0; obl < nb; ++obl) {
        v16i acc[4];
#pragma unroll
        for (int par = 0; par < 4; ++par)
#pragma unroll
          for (int q = 0; q < 4; ++q) {  // start value: the parity's compensation of this lane's 16 channels
            const v4i cv = *reinterpret_cast<const v4i *>(comp_l + par * 32 * DC_CHUNK + obl * 32 + 8 * q + 4 * h);
            acc[par][4 * q + 0] = cv[0]; acc[par][4 * q + 1] = cv[1]; acc[par][4 * q + 2] = cv[2]; acc[par][4 * q + 3] = cv[3];
          }
        const unsigned char *wl = w_lds + (size_t)obl * wblk + lane * 16;
        for (int s = 0; s < a.ksteps; ++s) {
          v4i fx[T * T];
#pragma unroll
          for (int t = 0; t < T * T; ++t) {
            const v4i v = *reinterpret_cast<const v4i *>(a.src + off[t] + (size_t)s * 32);
            fx[t] = (ok[t] ? v : zero4) ^ x80;  // u8 -> s8; a skipped tap is the activation 0
          }
#pragma unroll
          for (int par = 0; par < 4; ++par)
#pragma unroll
            for (int t = 0; t < T * T; ++t)
              acc[par] = gc_mfma(*reinterpret_cast<const v4i *>(wl + (size_t)s * KSTEP + (par * T * T + t) * 1024), fx[t], acc[par]);  // D[oc][px]
        }

#pragma unroll
        for (int par = 0; par < 4; ++par) {
          auto quarter = [&](int q) -> v4i {
            const int ch = obl * 32 + 8 * q + 4 * h;
            const v4f bs4 = *reinterpret_cast<const v4f *>(bias_l + ch);
            const v4f sc4 = *reinterpret_cast<const v4f *>(scale_l + ch);
            const int a4[4] = {acc[par][4 * q + 0], acc[par][4 * q + 1], acc[par][4 * q + 2], acc[par][4 * q + 3]};
            return gc_quarter<DST, FAST>(a4, bs4, sc4, relu, a.rm);
          };
          const long long par_off = ((long long)(par >> 1) * a.ow + (par & 1)) * row_bytes + (long long)(cb0 + obl) * 32 * ESZ;
          if constexpr (ESZ == 1) {
#pragma unroll
            for (int q = 0; q < 4; ++q) *reinterpret_cast<int *>(stg + l31 * GC_STAGE_PITCH + 8 * q + 4 * h) = quarter(q)[0];
            // 32 rows x 32 bytes = 64 pieces of 16
            const int row = lane >> 1, c16 = lane & 1;
            const v4i val = *reinterpret_cast<const v4i *>(stg + row * GC_STAGE_PITCH + 16 * c16);
            const int rl = __shfl(live, row), lo = __shfl(ob_lo, row), hi = __shfl(ob_hi, row);
            const long long ob = ((long long)hi << 32) | (unsigned)lo;
            if ((rl >> par) & 1) dfx_store16_nt(reinterpret_cast<v4i *>(a.dst + ob + par_off + 16 * c16), val);
          } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) *reinterpret_cast<v4i *>(stg + l31 * GC_STAGE_PITCH + 32 * q + 16 * h) = quarter(q);
#pragma unroll
            for (int k = 0; k < 4; ++k) {  // 32 rows x 128 bytes = 256 pieces of 16
              const int ck = lane + 64 * k, row = ck >> 3, c16 = ck & 7;
              const v4i val = *reinterpret_cast<const v4i *>(stg + row * GC_STAGE_PITCH + 16 * c16);
              const int rl = __shfl(live, row), lo = __shfl(ob_lo, row), hi = __shfl(ob_hi, row);
              const long long ob = ((long long)hi << 32) | (unsigned)lo;
              if ((rl >> par) & 1) dfx_store16_nt(reinterpret_cast<v4i *>(a.dst + ob + par_off + 16 * c16), val);
            }
          }
        }
      }
    }
  }
}

}  // namespace dfx
