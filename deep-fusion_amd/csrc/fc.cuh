// fc.cuh -- the int8 fully-connected op's kernels (dfx_fc_* of include/dfx.h; gfx950): a split-K GEMM on
// v_mfma_i32_32x32x32_i8 that writes raw s32 partial sums, and the vector epilogue that adds them up and requantises.
//
// The op is bound by its weight stream (every weight byte is used once per batch), so parallelism comes from
// oc x K, not from the batch:
//   * A operand = weights, 32 output channels per block; B operand = the batch, 32 images per column block.  The host
//     packs the weights as [oc block][k-step of 64][2 fragments][lane][16 B] in src's (y, x, c) order (fc_pack.h): every
//     fragment is one contiguous, aligned 1 KB that goes global -> VGPR with one 16-byte load per lane, no LDS.
//   * Unit = (group of FC_WAVES oc blocks, K slice, batch chunk of <= FC_CHUNK images).  The chunk's slice of the
//     activations is staged in LDS FC_KT k-steps at a time -- whole 128-byte lines, stored as u8 - 128 (xor 0x80),
//     16-byte pieces XOR-swizzled by the image index's low three bits (see fc_tile) --
//     and every wave of the workgroup owns another oc block over it.  A wave issues the weight loads of a whole tile
//     (up to 16 KB) before the staging barrier, so they are in flight while the tile is staged.
//   * Images n >= bs of the last column block are staged from image bs - 1 (no address outside src is formed); their
//     columns are never stored.
//   * The unit's result goes, without compensation, bias or scale, into slab[slice][image][oc rounded up to 32] with
//     plain 16-byte stores.  fc_epilogue_kernel sums the slices as integers (every splitk gives the same bits), adds
//     the compensation 128 * sum(w) once, and runs gconv.cuh's requant chain on four adjacent channels per thread.
// No workgroup waits on another one.
#pragma once

#include "gconv.cuh"  // gc_mfma, gc_quarter

namespace dfx {

constexpr int FC_THREADS = 256;
constexpr int FC_WAVES = FC_THREADS / 64;  // oc blocks per unit
constexpr int FC_CHUNK = 128;              // images per unit: 4 column blocks
constexpr int FC_KT = 8;                   // k-steps of 64 per staged tile
constexpr int FC_PITCH = 64 * FC_KT;       // bytes per staged image: 32 pieces of 16 bytes

struct FcArgs {
  const unsigned char *src;
  unsigned char *dst;
  const unsigned char *wpk;  // MFMA path: fc_pack.h's image
  const signed char *wraw;   // generic path: {oc, ic, ih, iw} as given
  int *slab;                 // MFMA path: [splitk][n_pad][oc_pad] partial sums
  const int *comp;           // [oc_pad] 128 * sum of the channel's weights
  const float *bias;         // [oc_pad] f32 (0 without bias)
  const float *scale;        // [oc_pad] (a single scale is expanded by the host)
  int bs, k, oc, ic, ih, iw;
  int dst_dt, relu, rm;
  int fast;                  // requant route (0 exact, 1 fast)
  int nks;                   // k-steps of 64
  int ocb, ocg;              // oc blocks of 32, groups of FC_WAVES of them
  int chunks;                // batch chunks of FC_CHUNK
  int splitk, units;         // K slices; units = ocg * splitk * chunks
  int cut;                   // slices are cut at multiples of `cut` k-steps: FC_KT (whole tiles) or 1 (splitk > tiles)
  int n_pad, oc_pad;         // bs, oc rounded up to 32
  long long items;           // generic: dst elements
};

// One staged tile of a unit: FC_KT k-steps (FULL) or the nst < FC_KT that end a slice.  Every thread first issues its
// 4 * NCB staging loads (32 * NCB images x 32 pieces over 256 threads; images beyond the batch are image bs - 1), then its
// wave's 16 weight-fragment loads; the staging loads are the older ones, so the LDS image is written while the weights
// are still in flight, and each MFMA pair waits for its own fragment only.  FULL has no conditionals at all; WHOLE (the
// chunk has all its 32 * NCB images) needs no clamp, so the staging addresses are one lane offset plus uniform steps.
// Swizzle: piece p of image n sits at piece p ^ (n & 7) of its row: the 8 lanes of a B-fragment read that go together
// hit 8 different 16-byte columns, and both sides address with one or four lane offsets plus immediates.
template <int NCB, bool FULL, bool WHOLE>
__device__ __forceinline__ void fc_tile(const FcArgs &a, unsigned char *lds, const unsigned char *wl, int kt, int nst, int n0,
                                        int tid, int l31, int h, v16i (&acc)[NCB]) {
  constexpr int NIT = 4 * NCB;
  const v4i x80 = v4i{(int)0x80808080, (int)0x80808080, (int)0x80808080, (int)0x80808080};
  const v4i zero4 = v4i{0, 0, 0, 0};
  const int piece = tid & 31, row0 = tid >> 5;  // this thread's 16-byte piece of rows row0, row0 + 8, ...
  const bool mine = FULL || piece < 4 * nst;
  // (uniform 64-bit bases and 32-bit lane offsets: an image of the chunk is at most 127 * 65025 bytes from its first)
  const unsigned char *const sb = a.src + (size_t)n0 * a.k + (size_t)kt * 64;
  const int nlast = a.bs - 1 - n0;
  v4i sv[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    sv[it] = zero4;
    if (WHOLE) {
      if (mine) sv[it] = *reinterpret_cast<const v4i *>(sb + (size_t)(8 * it) * a.k + ((unsigned)row0 * (unsigned)a.k + (unsigned)(piece * 16)));
    } else {
      const unsigned off = (unsigned)min(row0 + 8 * it, nlast) * (unsigned)a.k + (unsigned)(piece * 16);
      if (mine) sv[it] = *reinterpret_cast<const v4i *>(sb + off);
    }
  }
  __builtin_amdgcn_sched_barrier(0);  // keep the staging loads the older ones: vmcnt counts in issue order
  const unsigned char *const wt = wl + (size_t)kt * 2048;
  const unsigned lane16 = (unsigned)(tid & 63) * 16;
  v4i wf[2 * FC_KT];
#pragma unroll
  for (int i = 0; i < 2 * FC_KT; ++i) {
    wf[i] = zero4;
    if (FULL || i < 2 * nst) wf[i] = *reinterpret_cast<const v4i *>(wt + (lane16 + (unsigned)i * 1024));
  }
  __builtin_amdgcn_sched_barrier(0);  // every load of the tile is issued before anything waits for one
  __syncthreads();  // the previous tile's readers are done with the LDS image
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    // ((row0 + 8 it) & 7 == row0)
    *reinterpret_cast<v4i *>(lds + (row0 * FC_PITCH + ((piece ^ row0) << 4)) + it * 8 * FC_PITCH) = sv[it] ^ x80;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2 * FC_KT; ++i)
    if (FULL || i < 2 * nst) {
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        // piece 2 i + h of row cb * 32 + l31: bits 3, 4 of 2 i pass the xor with l31 & 7 unchanged
        const v4i b = *reinterpret_cast<const v4i *>(lds + (l31 * FC_PITCH + ((((2 * i) & 6) ^ h ^ (l31 & 7)) << 4)) +
                                                     (cb * 32 * FC_PITCH + (((2 * i) & 24) << 4)));
        acc[cb] = gc_mfma(wf[i], b, acc[cb]);  // D[oc][image]
      }
    }
}

// NCB: column blocks of a full chunk, min(4, n_pad / 32): a batch of <= 32 images keeps 16 accumulator registers, not 64.
// A chunk with fewer images and a wave beyond the last oc block compute like the others (on image bs - 1 / on the last
// block's weights) and store nothing: the kernel has no conditional around its loads and MFMAs.
// LDS: [32 * NCB][FC_PITCH] bytes.
template <int NCB>
__global__ __launch_bounds__(FC_THREADS, 2) void fc_mfma_kernel(FcArgs a) {  // two waves per SIMD: two workgroups per CU
  extern __shared__ __attribute__((aligned(16))) unsigned char fc_lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, h = lane >> 5;

  for (int u = blockIdx.x; u < a.units; u += gridDim.x) {  // uniform over the workgroup: so are the barriers of fc_tile
    const int g = u % a.ocg, r = u / a.ocg;
    const int s = r % a.splitk, chunk = r / a.splitk;
    const long long ncut = (a.nks + a.cut - 1) / a.cut;  // slice s: granules [s ncut / splitk, (s + 1) ncut / splitk)
    const int ks0 = min(a.nks, a.cut * (int)(s * ncut / a.splitk)), ks1 = min(a.nks, a.cut * (int)((s + 1) * ncut / a.splitk));
    const int n0 = chunk * FC_CHUNK;
    const int ob = g * FC_WAVES + wave;  // (wave-uniform) the last group may have fewer than FC_WAVES blocks
    const unsigned char *const wl = a.wpk + (size_t)min(ob, a.ocb - 1) * a.nks * 2048;  // (uniform)
    v16i acc[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[cb][i] = 0;

    int kt = ks0;
    if (n0 + 32 * NCB <= a.bs) {  // (uniform)
      for (; kt + FC_KT <= ks1; kt += FC_KT) fc_tile<NCB, true, true>(a, fc_lds, wl, kt, FC_KT, n0, tid, l31, h, acc);
      if (kt < ks1) fc_tile<NCB, false, true>(a, fc_lds, wl, kt, ks1 - kt, n0, tid, l31, h, acc);
    } else {
      for (; kt + FC_KT <= ks1; kt += FC_KT) fc_tile<NCB, true, false>(a, fc_lds, wl, kt, FC_KT, n0, tid, l31, h, acc);
      if (kt < ks1) fc_tile<NCB, false, false>(a, fc_lds, wl, kt, ks1 - kt, n0, tid, l31, h, acc);
    }

    if (ob < a.ocb) {
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        const int n = n0 + cb * 32 + l31;
        if (n < a.bs) {
          int *const row = a.slab + ((size_t)s * a.n_pad + n) * a.oc_pad + ob * 32 + 4 * h;
#pragma unroll
          for (int q = 0; q < 4; ++q)  // the lane holds channels 8 q + 4 h .. + 3 of its image
            dfx_store16(reinterpret_cast<v4i *>(row + 8 * q), v4i{acc[cb][4 * q], acc[cb][4 * q + 1], acc[cb][4 * q + 2], acc[cb][4 * q + 3]});
        }
      }
    }
  }
}

// One thread per (image, four adjacent output channels).  Rows of dst are oc elements apart: with oc no multiple of 4
// they are not aligned, and the values leave one by one.
template <int DST, bool FAST>
__global__ __launch_bounds__(256) void fc_epilogue_kernel(FcArgs a) {
  constexpr int ESZ = (DST == DFX_F32 || DST == DFX_S32) ? 4 : 1;
  const int o4n = (a.oc + 3) / 4;
  const long long total = (long long)a.bs * o4n, stride = (long long)gridDim.x * blockDim.x;
  const bool vec = (a.oc & 3) == 0;
  for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += stride) {
    const int n = (int)(id / o4n), o = 4 * (int)(id % o4n);
    v4i sum = *reinterpret_cast<const v4i *>(a.comp + o);  // (comp, bias and scale have oc_pad entries)
    for (int s = 0; s < a.splitk; ++s) sum += *reinterpret_cast<const v4i *>(a.slab + ((size_t)s * a.n_pad + n) * a.oc_pad + o);
    const int a4[4] = {sum[0], sum[1], sum[2], sum[3]};
    const v4i out = gc_quarter<DST, FAST>(a4, *reinterpret_cast<const v4f *>(a.bias + o), *reinterpret_cast<const v4f *>(a.scale + o),
                                          a.relu != 0, a.rm);
    const int left = min(4, a.oc - o);
    if constexpr (ESZ == 1) {
      unsigned char *const p = a.dst + (size_t)n * a.oc + o;
      if (vec) *reinterpret_cast<int *>(p) = out[0];
      else
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < left) p[j] = (unsigned char)((unsigned)out[0] >> (8 * j));
    } else {
      int *const p = reinterpret_cast<int *>(a.dst) + (size_t)n * a.oc + o;
      if (vec) dfx_store16(reinterpret_cast<v4i *>(p), out);
      else
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < left) p[j] = out[j];
    }
  }
}

}  // namespace dfx
