// linear.hip -- the token linear op's kernels: the instances of the LDS-tiled MFMA kernel (linear.cuh) and the generic
// backstop (one thread per output value, any k, pitch and alignment, the exact requant route).
#include "linear.cuh"

namespace dfx {

__global__ __launch_bounds__(LIN_THREADS) void linear_generic_kernel(LinArgs a) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < a.items; id += stride) {
    const int o = (int)(id % a.n);
    const long long m = id / a.n;
    const unsigned char *sp = a.src + (size_t)m * (size_t)a.src_ld;
    // linear_pack.h's lin_wei_offset: row o's 16-byte piece kp = c / 16 of the image
    const signed char *wp = reinterpret_cast<const signed char *>(a.wpk) + (size_t)(o / LIN_BN) * (size_t)a.nks * LIN_WBLOCK +
                            (size_t)(((o % LIN_BN) / 32) * 2048 + (o % 32) * 16);
    int acc = 0;
    for (int c = 0; c < a.k; ++c) {
      const int kp = c >> 4;
      const int w = wp[(size_t)(kp >> 2) * LIN_WBLOCK + (size_t)(((kp >> 1) & 1) * 1024 + (kp & 1) * 512 + (c & 15))];
      const int x = a.a_u8 ? (int)sp[c] : (int)(signed char)sp[c];
      acc += x * w;
    }
    const float f = requant(acc, a.bias[o], a.scale[o], a.relu != 0);
    const size_t at = (size_t)m * (size_t)a.dst_ld + (size_t)o;
    switch (a.req_dt) {
      case DFX_F32: reinterpret_cast<float *>(a.dst)[at] = f; break;
      case DFX_S32: reinterpret_cast<int *>(a.dst)[at] = cvt_x86_rt(f, a.rm); break;
      default: {
        const unsigned t = a.req_dt == DFX_S8 ? ((unsigned)sat_s8(cvt_x86_rt(f, a.rm)) & 0xffu) : sat_u8_bits(cvt_x86_rt(f, a.rm));
        a.dst[at] = a.lut ? a.lut[a.lut_u8 ? t : (t ^ 0x80u)] : (unsigned char)t;
      }
    }
  }
}

// (lds is below the 64 KB every kernel may have without asking)
template <int BM, int DST>
static int lin_one(const LinArgs &a, int grid, int lds, hipStream_t s, bool fast) {
  if (fast) linear_tile_kernel<BM, DST, true><<<grid, LIN_THREADS, lds, s>>>(a);
  else linear_tile_kernel<BM, DST, false><<<grid, LIN_THREADS, lds, s>>>(a);
  return 0;
}

template <int BM>
static int lin_bm_one(const LinArgs &a, int grid, int lds, hipStream_t s, bool fast) {
  switch (a.req_dt) {
    case DFX_F32: return lin_one<BM, DFX_F32>(a, grid, lds, s, fast);
    case DFX_S32: return lin_one<BM, DFX_S32>(a, grid, lds, s, fast);
    case DFX_S8: return lin_one<BM, DFX_S8>(a, grid, lds, s, fast);
    case DFX_U8: return lin_one<BM, DFX_U8>(a, grid, lds, s, fast);
  }
  return -1;
}

// -1: no such instance
int launch_linear_tile(const LinArgs &a, int bm, int grid, int lds, hipStream_t s, bool fast) {
  if (bm == 128) return lin_bm_one<128>(a, grid, lds, s, fast);
  if (bm == 64) return lin_bm_one<64>(a, grid, lds, s, fast);
  return -1;
}

int launch_linear_generic(const LinArgs &a, int grid, hipStream_t s) {
  linear_generic_kernel<<<grid, LIN_THREADS, 0, s>>>(a);
  return 0;
}

}  // namespace dfx
