// dwconv.cuh -- the depthwise int8 conv's sliding-window kernel (dfx_dwconv_* of include/dfx.h; gfx950).
//
// There is no matrix form, so no MFMA: the design quantity is VECTOR INSTRUCTIONS PER OUTPUT VALUE (DESIGN.md 4.7:
// one wave64 vector instruction per 4 cycles per SIMD makes every instruction per value ~1.3 us at N=128 56x56x128,
// ten of them the HBM floor).  Formulation: tap-transposed dot4.
//   * A lane owns 16 channels (one dwordx4 per pixel) of ONE output column and slides down a band of output rows.
//     Consecutive lanes hold consecutive channel groups, then consecutive columns: a wave's loads and stores are
//     contiguous.  The K loads of one input row overlap between neighbouring lanes and are served by L1; the K - S
//     halo rows two neighbouring bands share come from L2: (K - S) / (band * S) of the input is read twice.
//   * Each input row is turned ONCE, per channel, into dwords that hold the row's K taps of the x axis
//     [t0 t1 t2 0] (K = 5: [t0 t1 t2 t3] [t4 0 0 0]) by v_perm_b32, 6 (12) per 4 channels, then xor 0x80808080
//     (u8 -> s8 - 128), and added to every output row it is a tap row of: ceil(K / S) accumulator sets are in
//     flight, indexed statically (the row loop is unrolled over the bookkeeping's period).
//   * Each output is K (2K) v_dot4_i32_i8 against per-channel weight dwords packed the same way by the host, started
//     from 128 * sum(w): a tap outside the input is the byte 0x00 before the xor, i.e. the activation 0, so the
//     compensation is the same for every pixel.  3x3 weights live in registers (48), 5x5 weights (160 dwords) in LDS.
//   * Edges cost nothing in the loop: a column outside the input only changes the lane's v_perm selectors (selector
//     byte 0x0c yields 0x00), computed once per work item; a row outside the input swaps the last-level selectors
//     for 0x0c0c0c0c.  Addresses are CLAMPED to the image first: no lane ever forms an address outside the tensors.
//   * The loads of the next input row are issued before the current row is computed.
// Counted from the ISA: 3x3 stride 1, u8 out, fast route: 2.5 (pack) + 3 (dot4) + 1 (start value) + 4
// (convert, add, multiply, v_cvt_pk_u8_f32) + 1.1 (selects, addresses) = 11.65 vector instructions per value.
#pragma once

#include <type_traits>
#include <utility>

#include "dfx_device.cuh"

namespace dfx {

constexpr int DW_THREADS = 256;
constexpr int DW_LDS_ROWS = 53;  // 5x5: 40 + 12 rows of 16 bytes per slot, + 1

struct DwArgs {
  const unsigned char *src;
  unsigned char *dst;
  const unsigned *wpk;      // window path: [c/16][K][NDW][16] dwords, the row's taps of one channel per dword
  const signed char *wraw;  // generic path: {c, kh, kw} as given
  const int *comp;          // [c] 128 * sum of the channel's weights
  const float *bias;        // [c] f32 (0 without bias)
  const float *scale;       // [c] (a single scale is expanded by the host)
  int bs, c, ih, iw, oh, ow, kh, kw, sh, sw, pt, pl;
  int dst_dt, relu, rm;
  int fast;                 // requant route (0 exact, 1 fast)
  int groups;               // c / 16
  int band, nbands;         // output rows per work item, work items per image column
  long long items;          // window: bs * nbands * ow pixel items (x groups lanes each); generic: dst elements
  long long threads;        // window: lanes that take part, a multiple of groups; a lane's step is threads / groups items
  int slot_by_group;        // window, weights in LDS: a lane's slot of the block's LDS image is its group (1) or thread (0)
};

__device__ __forceinline__ unsigned dw_sel(unsigned base, unsigned mask, bool valid) {
  return valid ? base : ((base & ~mask) | (0x0c0c0c0cu & mask));
}
// v_perm_b32: selector bytes 0-3 take bytes of `lo`, 4-7 bytes of `hi`, 0x0c gives 0x00
__device__ __forceinline__ unsigned dw_perm(unsigned hi, unsigned lo, unsigned sel) { return __builtin_amdgcn_perm(hi, lo, sel); }

template <int K> struct DwPack;

template <> struct DwPack<3> {
  static constexpr int NDW = 1;
  unsigned s[6];
  __device__ __forceinline__ void set(const bool (&v)[3]) {
    s[0] = dw_sel(dw_sel(0x05010400u, 0x00ff00ffu, v[0]), 0xff00ff00u, v[1]);  // [p0.c0 p1.c0 p0.c1 p1.c1]
    s[1] = dw_sel(dw_sel(0x07030602u, 0x00ff00ffu, v[0]), 0xff00ff00u, v[1]);  // [p0.c2 p1.c2 p0.c3 p1.c3]
    s[2] = dw_sel(0x0c040100u, 0x00ff0000u, v[2]);                             // [t.b0 t.b1 p2.c0 0]
    s[3] = dw_sel(0x0c050302u, 0x00ff0000u, v[2]);                             // [t.b2 t.b3 p2.c1 0]
    s[4] = dw_sel(0x0c060100u, 0x00ff0000u, v[2]);
    s[5] = dw_sel(0x0c070302u, 0x00ff0000u, v[2]);
  }
  __device__ __forceinline__ void pack(const v4i (&p)[3], bool row_ok, unsigned (&out)[16]) const {
    const unsigned z = 0x0c0c0c0cu;
    const unsigned s2 = row_ok ? s[2] : z, s3 = row_ok ? s[3] : z, s4 = row_ok ? s[4] : z, s5 = row_ok ? s[5] : z;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const unsigned t01 = dw_perm((unsigned)p[1][q], (unsigned)p[0][q], s[0]);
      const unsigned t23 = dw_perm((unsigned)p[1][q], (unsigned)p[0][q], s[1]);
      out[4 * q + 0] = dw_perm((unsigned)p[2][q], t01, s2) ^ 0x80808080u;
      out[4 * q + 1] = dw_perm((unsigned)p[2][q], t01, s3) ^ 0x80808080u;
      out[4 * q + 2] = dw_perm((unsigned)p[2][q], t23, s4) ^ 0x80808080u;
      out[4 * q + 3] = dw_perm((unsigned)p[2][q], t23, s5) ^ 0x80808080u;
    }
  }
};

template <> struct DwPack<5> {
  static constexpr int NDW = 2;
  unsigned s[8];
  __device__ __forceinline__ void set(const bool (&v)[5]) {
    s[0] = dw_sel(dw_sel(0x05010400u, 0x00ff00ffu, v[0]), 0xff00ff00u, v[1]);
    s[1] = dw_sel(dw_sel(0x07030602u, 0x00ff00ffu, v[0]), 0xff00ff00u, v[1]);
    s[2] = dw_sel(dw_sel(0x05010400u, 0x00ff00ffu, v[2]), 0xff00ff00u, v[3]);
    s[3] = dw_sel(dw_sel(0x07030602u, 0x00ff00ffu, v[2]), 0xff00ff00u, v[3]);
#pragma unroll
    for (int j = 0; j < 4; ++j) s[4 + j] = v[4] ? (0x0c0c0c00u | (unsigned)j) : 0x0c0c0c0cu;  // [p4.cj 0 0 0]
  }
  // out[2 * ch] = [t0 t1 t2 t3], out[2 * ch + 1] = [t4 0 0 0]
  __device__ __forceinline__ void pack(const v4i (&p)[5], bool row_ok, unsigned (&out)[32]) const {
    const unsigned z = 0x0c0c0c0cu;
    const unsigned sa = row_ok ? 0x05040100u : z, sb = row_ok ? 0x07060302u : z;
    unsigned st[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) st[j] = row_ok ? s[4 + j] : z;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const unsigned a01 = dw_perm((unsigned)p[1][q], (unsigned)p[0][q], s[0]);
      const unsigned b01 = dw_perm((unsigned)p[1][q], (unsigned)p[0][q], s[1]);
      const unsigned a23 = dw_perm((unsigned)p[3][q], (unsigned)p[2][q], s[2]);
      const unsigned b23 = dw_perm((unsigned)p[3][q], (unsigned)p[2][q], s[3]);
      out[8 * q + 0] = dw_perm(a23, a01, sa) ^ 0x80808080u;
      out[8 * q + 2] = dw_perm(a23, a01, sb) ^ 0x80808080u;
      out[8 * q + 4] = dw_perm(b23, b01, sa) ^ 0x80808080u;
      out[8 * q + 6] = dw_perm(b23, b01, sb) ^ 0x80808080u;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        out[8 * q + 2 * j + 1] = dw_perm(0u, (unsigned)p[4][q], st[j]) ^ 0x80808080u;
    }
  }
};

// one output pixel's 16 channels: requantisation and store.  FAST: host-proven (dwconv_api.hip): bias and scale finite,
// round to nearest, nothing within reach of +-2^31 -- the add and the multiply are the exact route's, only the
// conversion is the hardware's.
template <int DST, bool FAST>
__device__ __forceinline__ void dw_store(unsigned char *q, const int (&acc)[16], const float (&bias)[16],
                                         const float (&scale)[16], bool relu, int rm) {
  if (DST == DFX_U8 || DST == DFX_S8) {
    v4i pk4;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      unsigned pk = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int ch = 4 * g + j;
        float f = __fmul_rn(__fadd_rn(__int2float_rn(acc[ch]), bias[ch]), scale[ch]);
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
      pk4[g] = (int)pk;
    }
    dfx_store16_nt(reinterpret_cast<v4i *>(q), pk4);
  } else {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float f[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int ch = 4 * g + j;
        f[j] = __fmul_rn(__fadd_rn(__int2float_rn(acc[ch]), bias[ch]), scale[ch]);
        f[j] = relu ? relu_x86(f[j]) : f[j];
      }
      if (DST == DFX_F32) {
        dfx_store16_nt(reinterpret_cast<v4f *>(q) + g, v4f{f[0], f[1], f[2], f[3]});
      } else {
        v4i v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = FAST ? (int)__builtin_rintf(f[j]) : cvt_x86_rt(f[j], rm);
        dfx_store16_nt(reinterpret_cast<v4i *>(q) + g, v);
      }
    }
  }
}

// compile-time loop: f(std::integral_constant<int, 0>) ... f(std::integral_constant<int, N - 1>)
template <class F, int... I>
__device__ __forceinline__ void dw_static_for_impl(F &&f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void dw_static_for(F &&f) {
  dw_static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// floor division / modulo for the static row bookkeeping (operands may be negative)
constexpr int dw_fdiv(int x, int y) { return (x >= 0) ? x / y : -((-x + y - 1) / y); }
constexpr int dw_fmod(int x, int y) { return x - dw_fdiv(x, y) * y; }

// WLDS: the lane's weight dwords are read from LDS for every use instead of living in registers (K = 5: 160 dwords).
// LDS layout: v4i [slots][DW_LDS_ROWS]: K * NDW * 4 rows of weights, 4 of compensation, 4 of bias, 4 of scale, padded
// to an odd count so that 16 lanes' 16-byte reads of one row fall into 64 different banks and every read has a constant
// offset from the lane's base.  A lane's slot is its channel group where the block's lanes share groups
// (a.slot_by_group), else its thread index.
template <int K, int S, int DST, bool FAST, bool WLDS>
__global__ __launch_bounds__(DW_THREADS) void dwconv_window_kernel(DwArgs a) {
  constexpr int NDW = DwPack<K>::NDW;
  constexpr int NA = (K + S - 1) / S;  // output rows in flight
  constexpr int U = NA * S;            // input rows after which the static bookkeeping repeats
  extern __shared__ v4i dw_lds[];
  // (32-bit: the host keeps threads and items below 2^31; 64-bit divisions would cost as much as an output row)
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = t < (unsigned)a.threads;
  const int g = active ? (int)(t % (unsigned)a.groups) : 0;
  const unsigned step = (unsigned)a.threads / (unsigned)a.groups, items = (unsigned)a.items;

  // this lane's 16 channels: weights, compensation, bias, scale -- loaded once, the lane keeps its channel group
  unsigned w[WLDS ? 1 : K][NDW][16];
  v4i *wl = dw_lds + (a.slot_by_group ? g : (int)threadIdx.x) * DW_LDS_ROWS;
  {
    const v4i *wp = reinterpret_cast<const v4i *>(a.wpk) + (size_t)g * K * NDW * 4;
#pragma unroll
    for (int ky = 0; ky < K; ++ky)
#pragma unroll
      for (int j = 0; j < NDW; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const v4i v = wp[(ky * NDW + j) * 4 + q];
          if (WLDS) {
            wl[(ky * NDW + j) * 4 + q] = v;
          } else {
            w[ky][j][4 * q + 0] = (unsigned)v[0]; w[ky][j][4 * q + 1] = (unsigned)v[1];
            w[ky][j][4 * q + 2] = (unsigned)v[2]; w[ky][j][4 * q + 3] = (unsigned)v[3];
          }
        }
  }
  // compensation, bias, scale: registers (48), or behind the weights in LDS
  constexpr int NW = K * NDW * 4;  // v4i rows of the weights
  int comp[16];
  float bias[16], scale[16];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const v4i cv = reinterpret_cast<const v4i *>(a.comp)[(size_t)g * 4 + q];
    const v4f bv = reinterpret_cast<const v4f *>(a.bias)[(size_t)g * 4 + q];
    const v4f sv = reinterpret_cast<const v4f *>(a.scale)[(size_t)g * 4 + q];
    if (WLDS) {
      wl[NW + q] = cv;
      wl[NW + 4 + q] = v4i{__float_as_int(bv[0]), __float_as_int(bv[1]), __float_as_int(bv[2]), __float_as_int(bv[3])};
      wl[NW + 8 + q] = v4i{__float_as_int(sv[0]), __float_as_int(sv[1]), __float_as_int(sv[2]), __float_as_int(sv[3])};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) { comp[4 * q + j] = cv[j]; bias[4 * q + j] = bv[j]; scale[4 * q + j] = sv[j]; }
    }
  }
  if (WLDS) __syncthreads();  // (lanes that share a group wrote the same values)
  if (!active) return;
  const size_t es = (DST == DFX_F32 || DST == DFX_S32) ? 4 : 1;
  const int row_pitch = a.iw * a.c;  // one image is below 2^31 bytes (the class): offsets inside an image fit an int

  for (unsigned item = t / (unsigned)a.groups; item < items; item += step) {
    const unsigned r0 = item / (unsigned)a.ow;
    const int ox = (int)(item - r0 * (unsigned)a.ow);
    const int n = (int)(r0 / (unsigned)a.nbands), band = (int)(r0 - (unsigned)n * (unsigned)a.nbands);
    const int oy0 = band * a.band;
    const int nrows = min(a.band, a.oh - oy0);  // >= 1
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
    unsigned char *out = a.dst + (((size_t)n * a.oh + oy0) * a.ow + ox) * a.c * es + (size_t)g * 16 * es;
    const size_t out_pitch = (size_t)a.ow * a.c * es;

    // Input row r (relative to iy0) is tap row ky = r - tt * S of output row tt (relative to oy0): the NA output rows
    // in flight own one accumulator set each, output tt the set tt % NA.  r = rb + u with rb a multiple of U, so the
    // set and the tap row of every (u, ky) pair are static.  Sets of output rows outside 0 .. nrows-1 collect
    // rubbish that is never stored: a set is started afresh at its ky = 0.
    int acc[NA][16];
    v4i raw[K];  // the row in flight
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
        // (opaque offset: or the weight reads, loop-invariant, are hoisted back into 160 registers)
        int opq = 0;
        if (WLDS) asm volatile("" : "+v"(opq));
        const v4i *wls = wl + opq;
        unsigned P[16 * NDW];
        pk.pack(raw, iy0 + r >= 0 && iy0 + r < a.ih, P);
        load_row(r + 1);  // (clamped address: harmless past the band's last row)
        dw_static_for<K>([&](auto kc) {
          constexpr int ky = decltype(kc)::value;
          if constexpr (dw_fmod(u - ky, S) == 0) {
            constexpr int d = dw_fdiv(u - ky, S);  // output row rb / S + d
            constexpr int set = dw_fmod(d, NA);
#pragma unroll
            for (int j = 0; j < NDW; ++j)
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                v4i wq, cq;
                if constexpr (WLDS) {
                  wq = wls[(ky * NDW + j) * 4 + q];
                  if (ky == 0 && j == 0) cq = wls[NW + q];
                } else {
#pragma unroll
                  for (int e = 0; e < 4; ++e) { wq[e] = (int)w[ky][j][4 * q + e]; cq[e] = comp[4 * q + e]; }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                  const int ch = 4 * q + e;
                  acc[set][ch] = __builtin_amdgcn_sdot4((int)P[ch * NDW + j], wq[e], (ky == 0 && j == 0) ? cq[e] : acc[set][ch], false);
                }
              }
            if constexpr (ky == K - 1) {
              const int tt = rb / S + d;
              if (tt >= 0 && tt < nrows) {
                if constexpr (WLDS) {
                  float bl[16], sl[16];
#pragma unroll
                  for (int q = 0; q < 4; ++q) {
                    const v4i bv = wls[NW + 4 + q], sv = wls[NW + 8 + q];
#pragma unroll
                    for (int e = 0; e < 4; ++e) { bl[4 * q + e] = __int_as_float(bv[e]); sl[4 * q + e] = __int_as_float(sv[e]); }
                  }
                  dw_store<DST, FAST>(out + (size_t)tt * out_pitch, acc[set], bl, sl, a.relu != 0, a.rm);
                } else {
                  dw_store<DST, FAST>(out + (size_t)tt * out_pitch, acc[set], bias, scale, a.relu != 0, a.rm);
                }
              }
            }
          }
        });
      });
    }
  }
}

}  // namespace dfx
