// dilconv.cuh -- the int8 dilated conv's MFMA kernel (dfx_dilconv_* of include/dfx.h; gfx950): 3x3 window, stride 1, any
// dilation (dh, dw), ic and oc multiples of 32 with no cap on ic -- the 3x3 of a DeepLab ASPP branch (d = 6 .. 36 on
// 2048 or 320 channels) or of a dilated ResNet's res4 / res5.
//
//   * Work item = (R strips of 32 consecutive output pixels of the flattened {bs, oh, ow} per wave, chunk of up to
//     DL_CHUNK 32-channel output blocks).  The DL_WAVES waves of a workgroup share the chunk.
//   * Lane (pixel p = lane & 31, half h = lane >> 5) loads, per K-step of 32 input channels, its 16 channel bytes of each
//     of the 9 taps with one 16-byte load from global memory.  Dilation is only an address offset -- which is why the
//     activations come straight from global memory and not from a halo tile in LDS: at d = 18 such a tile would be 37
//     rows tall.  A tap outside the image is the byte 0x00 BEFORE the xor -- the activation 0 -- so the compensation
//     128 * sum(w), the accumulator's start value, is the same for every pixel.  Addresses are clamped into the tensor
//     first: no lane forms one outside.
//   * Every loaded fragment feeds the MFMAs of all nb blocks of the chunk: 9 nb MFMAs per 9 loads.  The accumulators of
//     all nb blocks of all R strips stay in registers over the whole contraction (64 R VGPRs).
//   * Weights: deconv.cuh keeps a chunk's fragments in LDS for the whole unit, which caps ic.  Here they move through
//     LDS in K-slabs -- S K-steps x 9 taps x nb KB (dilconv_pack.h's pieces) -- in one buffer or, where the plan has
//     room, two.  With two, a slab costs ONE barrier and nothing waits for memory in between: after the barrier a
//     thread issues the global loads of its share of the next slab into registers and of the next K-step's
//     activations, runs the MFMAs of the slab in LDS, and only then writes the registers to the other buffer.  The
//     plan does not depend on ic.
//   * The epilogue and stores are gconv.cuh's: a wave-private LDS staging area, 16 bytes per lane, nontemporal.
//   * Requant: gconv.cuh's gc_quarter, value for value; FAST swaps only the conversion.
//   * Every loop over work is grid-stride; no flags, spin-waits or atomics.
#pragma once

#include "gconv.cuh"

namespace dfx {

#ifndef DFX_DL_WAVES
#define DFX_DL_WAVES 8  // waves per workgroup: 8 from the A/B of DESIGN.md section 4.13 (-DDFX_DL_WAVES=4 builds the other leg)
#endif
constexpr int DL_WAVES = DFX_DL_WAVES;
constexpr int DL_THREADS = 64 * DL_WAVES;
constexpr int DL_CHUNK = 4;            // output-channel blocks per chunk (dilconv_pack.h's DL_PACK_CHUNK)
constexpr int DL_KSTEP = 9 * 1024;     // bytes of one K-step's fragments of one output block
constexpr int DL_FIXED_LDS = 3 * 32 * DL_CHUNK * 4 + DL_WAVES * GC_STAGE_BYTES;  // constants + staging
// 16-byte pieces of a slab a thread carries in registers (two-buffer plan): one K-step of a full chunk, 5 at 8 waves
constexpr int DL_WREG = (DL_CHUNK * DL_KSTEP / 16 + DL_THREADS - 1) / DL_THREADS;
// strips a wave may contract at once.  2 needs 128 accumulator registers and 72 of activations in flight: it fits the
// 512 registers of a 4-wave workgroup's waves, not the 256 of an 8-wave one's, so only the 4-wave build has the instance
constexpr int DL_MAX_STRIPS = DL_WAVES <= 4 ? 2 : 1;

struct DlArgs {
  const unsigned char *src;
  unsigned char *dst;
  const unsigned char *wpk;  // MFMA path: dilconv_pack.h's image
  const signed char *wraw;   // generic path: {oc, ic, kh, kw} as given
  const int *comp;           // MFMA path: [oc] 128 * sum of the channel's weights
  const float *bias;         // [oc] f32 (0 without bias)
  const float *scale;        // [oc] (a single scale is expanded by the host)
  int bs, ic, ih, iw, oc, oh, ow, kh, kw, sh, sw, dh, dw, pt, pl;
  int dst_dt, relu, rm;
  int fast;                  // requant route (0 exact, 1 fast)
  int cblocks, nchunks;      // MFMA: 32-channel output blocks; chunks of DL_CHUNK of them
  int wblocks;               // MFMA: min(DL_CHUNK, cblocks): the blocks a slab buffer has room for
  int ksteps;                // MFMA: ic / 32
  int slab, nbuf;            // MFMA: K-steps per slab; slab buffers (1 | 2)
  int rstrips;               // MFMA: strips a wave contracts at once (the kernel's R)
  int strips, slots;         // MFMA: 32-pixel strips; workgroup slots per chunk
  int px_total;              // bs * oh * ow
  long long items;           // generic: dst elements
};

// R: strips per wave.  LDS: [nbuf slab buffers of slab * 9 * wblocks KB][comp | bias | scale: 128 dwords each][staging].
template <int R, int DST, bool FAST>
__global__ __launch_bounds__(DL_THREADS) void dilconv_mfma_kernel(DlArgs a) {
  constexpr int ESZ = (DST == DFX_F32 || DST == DFX_S32) ? 4 : 1;
  constexpr int WR = DL_WAVES * R;  // strips of a workgroup's pass
  extern __shared__ __attribute__((aligned(16))) unsigned char dl_lds[];
  const int buf_bytes = a.slab * a.wblocks * DL_KSTEP;
  unsigned char *const w_lds = dl_lds;
  int *const comp_l = reinterpret_cast<int *>(dl_lds + (size_t)a.nbuf * buf_bytes);
  float *const bias_l = reinterpret_cast<float *>(comp_l + 32 * DL_CHUNK);
  float *const scale_l = bias_l + 32 * DL_CHUNK;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  unsigned char *const stg = reinterpret_cast<unsigned char *>(scale_l + 32 * DL_CHUNK) + wave * GC_STAGE_BYTES;
  const int l31 = lane & 31, h = lane >> 5;
  const bool relu = a.relu != 0;
  const v4i x80 = v4i{(int)0x80808080, (int)0x80808080, (int)0x80808080, (int)0x80808080};
  const v4i zero4 = v4i{0, 0, 0, 0};
  const size_t row_bytes = (size_t)a.oc * ESZ;
  const int nslabs = (a.ksteps + a.slab - 1) / a.slab;

  // BARRIERS.  Every __syncthreads() below sits in code whose control flow depends only on kernel arguments,
  // blockIdx / gridDim and the loop counters u, base and j derived from them -- never on tid, wave, lane or a strip
  // being live:
  //   - `units` and the unit loop's bounds are the same for every thread of a workgroup;
  //   - the pass loop runs while base < a.strips with base = (slot + n * slots) * WR: slot is the workgroup's, so all its
  //     waves make the same number of passes, also the waves whose strips base + wave * R + r lie beyond the last one.
  //     Those compute the LAST strip again (clamped: every address stays inside the tensors) and store nothing
  //     (nvalid = 0);
  //   - the slab loop runs j = 0 .. nslabs - 1 with nslabs from the arguments, and the choices inside it (nbuf, j + 1 <
  //     nslabs) are uniform too.
  // No `continue`, `break` or `return` precedes any barrier.  So all DL_THREADS threads reach the same sequence of
  // barriers, and a workgroup never waits for a wave that has left.
  const int units = a.nchunks * a.slots;
  for (int u = blockIdx.x; u < units; u += gridDim.x) {
    const int chunk = u % a.nchunks, slot = u / a.nchunks;
    const int cb0 = chunk * DL_CHUNK, nb = min(DL_CHUNK, a.cblocks - cb0);
    const int kbytes = nb * DL_KSTEP;  // one K-step of the chunk
    const unsigned char *const wchunk = a.wpk + (size_t)cb0 * a.ksteps * DL_KSTEP;
    __syncthreads();  // the previous unit's readers are done with the constants
    for (int q = tid; q < 32 * nb; q += DL_THREADS) {
      comp_l[q] = a.comp[32 * cb0 + q];
      bias_l[q] = a.bias[32 * cb0 + q];
      scale_l[q] = a.scale[32 * cb0 + q];
    }
    __syncthreads();

    // copies slab j of the chunk into buffer b (whole workgroup)
    auto copy_slab = [&](int j, int b) {
      const int ns = min(a.slab, a.ksteps - j * a.slab);
      const v4i *ws = reinterpret_cast<const v4i *>(wchunk + (size_t)j * a.slab * kbytes);
      v4i *wd = reinterpret_cast<v4i *>(w_lds + (size_t)b * buf_bytes);
      const int n16 = ns * (kbytes / 16);
      for (int q = tid; q < n16; q += DL_THREADS) wd[q] = ws[q];
    };
    // the same copy in two halves, for the plan with two buffers: global memory -> registers before the MFMAs of the
    // slab in use, registers -> LDS after them (the host admits two buffers only where DL_WREG pieces per thread hold
    // a slab: slab * wblocks <= DL_WREG * DL_THREADS / 576)
    auto slab_to_regs = [&](int j, v4i (&wreg)[DL_WREG]) {
      const int ns = min(a.slab, a.ksteps - j * a.slab);
      const v4i *ws = reinterpret_cast<const v4i *>(wchunk + (size_t)j * a.slab * kbytes);
      const int n16 = ns * (kbytes / 16);
#pragma unroll
      for (int i = 0; i < DL_WREG; ++i)
        if (tid + i * DL_THREADS < n16) wreg[i] = ws[tid + i * DL_THREADS];
    };
    auto regs_to_slab = [&](int j, int b, const v4i (&wreg)[DL_WREG]) {
      const int ns = min(a.slab, a.ksteps - j * a.slab);
      v4i *wd = reinterpret_cast<v4i *>(w_lds + (size_t)b * buf_bytes);
      const int n16 = ns * (kbytes / 16);
#pragma unroll
      for (int i = 0; i < DL_WREG; ++i)
        if (tid + i * DL_THREADS < n16) wd[tid + i * DL_THREADS] = wreg[i];
    };

    for (int base = slot * WR; base < a.strips; base += a.slots * WR) {
      bool ok[R][9];
      size_t off[R][9];  // byte offset of the tap's pixel (clamped into the image), this lane's half of K-step 0
      int nvalid[R], strip_c[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int strip = base + wave * R + r;
        strip_c[r] = min(strip, a.strips - 1);
        nvalid[r] = strip < a.strips ? min(32, a.px_total - 32 * strip) : 0;
        // this lane's output pixel (clamped to the last one).  int holds it: px_total <= 2^31 - 1 (validated).
        const int px = min(32 * strip_c[r] + l31, a.px_total - 1);
        const int q = px / a.ow, ox = px - q * a.ow;
        const int n = q / a.oh, oy = q - n * a.oh;
        const int iy0 = oy - a.pt, ix0 = ox - a.pl;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const int iy = iy0 + ky * a.dh, ix = ix0 + kx * a.dw;
            ok[r][3 * ky + kx] = iy >= 0 && iy < a.ih && ix >= 0 && ix < a.iw;
            const int cy = min(max(iy, 0), a.ih - 1), cx = min(max(ix, 0), a.iw - 1);
            off[r][3 * ky + kx] = (((size_t)n * a.ih + cy) * a.iw + cx) * (size_t)a.ic + 16 * h;
          }
      }
      v16i acc[R][DL_CHUNK];
#pragma unroll
      for (int obl = 0; obl < DL_CHUNK; ++obl)
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // start value: the compensation of this lane's 16 channels (obl >= nb: unused)
          const v4i cv = *reinterpret_cast<const v4i *>(comp_l + obl * 32 + 8 * q + 4 * h);
#pragma unroll
          for (int r = 0; r < R; ++r) {
            acc[r][obl][4 * q + 0] = cv[0]; acc[r][obl][4 * q + 1] = cv[1]; acc[r][obl][4 * q + 2] = cv[2]; acc[r][obl][4 * q + 3] = cv[3];
          }
        }

      // this lane's 16 bytes of the nine taps of K-step k, as loaded (the xor and the zero of a skipped tap come at use)
      auto load_acts = [&](int k, v4i (&fx)[R][9]) {
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int t = 0; t < 9; ++t) fx[r][t] = *reinterpret_cast<const v4i *>(a.src + off[r][t] + (size_t)k * 32);
      };

      __syncthreads();  // the previous pass's readers are done with every slab buffer
      copy_slab(0, 0);
      v4i fx[R][9];  // the NEXT K-step's activations: loaded while the MFMAs of this one run
      load_acts(0, fx);
      for (int j = 0; j < nslabs; ++j) {
        // slab j is in place, and (two buffers) every wave is done with slab j - 1, whose buffer slab j + 1 goes to
        __syncthreads();
        const bool ahead = a.nbuf == 2 && j + 1 < nslabs;  // uniform
        const unsigned char *wl = w_lds + (size_t)(a.nbuf == 2 ? (j & 1) : 0) * buf_bytes + lane * 16;
        const int ns = min(a.slab, a.ksteps - j * a.slab);
        v4i wreg[DL_WREG];  // two buffers: this thread's share of slab j + 1, in flight from global memory during the MFMAs
        for (int s = 0; s < ns; ++s) {
          const int k = j * a.slab + s;
          v4i cur[R][9];
#pragma unroll
          for (int r = 0; r < R; ++r)
#pragma unroll
            for (int t = 0; t < 9; ++t) cur[r][t] = (ok[r][t] ? fx[r][t] : zero4) ^ x80;  // u8 -> s8; a skipped tap is the activation 0
          if (ahead && s == 0) slab_to_regs(j + 1, wreg);
          if (k + 1 < a.ksteps) load_acts(k + 1, fx);
          const unsigned char *ws = wl + (size_t)s * kbytes;
#pragma unroll
          for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int obl = 0; obl < DL_CHUNK; ++obl)
              if (obl < nb) {
                const v4i wf = *reinterpret_cast<const v4i *>(ws + (t * nb + obl) * 1024);
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r][obl] = gc_mfma(wf, cur[r][t], acc[r][obl]);  // D[oc][px]
              }
        }
        if (ahead) regs_to_slab(j + 1, (j + 1) & 1, wreg);
        if (a.nbuf == 1) {
          __syncthreads();  // every wave is done with slab j
          if (j + 1 < nslabs) copy_slab(j + 1, 0);
        }
      }

#pragma unroll
      for (int r = 0; r < R; ++r) {
        unsigned char *const dst_strip = a.dst + (size_t)(32 * strip_c[r]) * row_bytes + (size_t)cb0 * 32 * ESZ;
#pragma unroll
        for (int obl = 0; obl < DL_CHUNK; ++obl)
          if (obl < nb) {
            auto quarter = [&](int q) -> v4i {
              const int ch = obl * 32 + 8 * q + 4 * h;
              const v4f bs4 = *reinterpret_cast<const v4f *>(bias_l + ch);
              const v4f sc4 = *reinterpret_cast<const v4f *>(scale_l + ch);
              const int a4[4] = {acc[r][obl][4 * q + 0], acc[r][obl][4 * q + 1], acc[r][obl][4 * q + 2], acc[r][obl][4 * q + 3]};
              return gc_quarter<DST, FAST>(a4, bs4, sc4, relu, a.rm);
            };
            if constexpr (ESZ == 1) {
#pragma unroll
              for (int q = 0; q < 4; ++q) *reinterpret_cast<int *>(stg + l31 * GC_STAGE_PITCH + obl * 32 + 8 * q + 4 * h) = quarter(q)[0];
            } else {
#pragma unroll
              for (int q = 0; q < 4; ++q) *reinterpret_cast<v4i *>(stg + l31 * GC_STAGE_PITCH + 32 * q + 16 * h) = quarter(q);
#pragma unroll
              for (int k = 0; k < 4; ++k) {  // 32 rows x 128 bytes = 256 pieces of 16
                const int ck = lane + 64 * k, row = ck >> 3, c16 = ck & 7;
                const v4i val = *reinterpret_cast<const v4i *>(stg + row * GC_STAGE_PITCH + 16 * c16);
                if (row < nvalid[r]) dfx_store16_nt(reinterpret_cast<v4i *>(dst_strip + (size_t)row * row_bytes + obl * 128 + 16 * c16), val);
              }
            }
          }
        if constexpr (ESZ == 1) {
          const int c16n = 2 * nb;  // 16-byte pieces per pixel of this chunk: 2, 4, 6 or 8
          for (int ck = lane; ck < 32 * c16n; ck += 64) {
            const int row = ck / c16n, c16 = ck - row * c16n;
            const v4i val = *reinterpret_cast<const v4i *>(stg + row * GC_STAGE_PITCH + 16 * c16);
            if (row < nvalid[r]) dfx_store16_nt(reinterpret_cast<v4i *>(dst_strip + (size_t)row * row_bytes + 16 * c16), val);
          }
        }
      }
    }
  }
}

}  // namespace dfx
