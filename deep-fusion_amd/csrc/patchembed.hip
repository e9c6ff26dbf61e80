// patchembed.hip -- the patch-embedding op's kernels: the instances of the gathering LDS-tiled MFMA kernel (patchembed.cuh) and
// the generic backstop (one thread per output value, any shape and alignment, the exact requant route).
#include "patchembed.cuh"

namespace dfx {

__global__ __launch_bounds__(LIN_THREADS) void patchembed_generic_kernel(PeArgs a) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < a.items; id += stride) {
    const int o = (int)(id % a.n);
    const long long m = id / a.n;
    const long long b = m / a.tokens, tk = m - b * a.tokens;
    const long long ty = tk / a.tw, tx = tk - ty * a.tw;
    const unsigned char *sp = a.src + (size_t)b * (size_t)a.img_bytes + (size_t)(ty * a.ph) * (size_t)a.row_bytes + (size_t)tx * (size_t)a.run;
    const signed char *wp = reinterpret_cast<const signed char *>(a.wpk);
    int acc = 0;
    for (int ky = 0; ky < a.ph; ++ky, sp += a.row_bytes)
      for (int c = 0; c < a.run; ++c) {
        const int w = wp[lin_wei_offset(o, ky * a.run + c, a.k)];  // linear_pack.h: the image is dfx_linear's of {oc, K}
        const int x = a.a_u8 ? (int)sp[c] : (int)(signed char)sp[c];
        acc += x * w;
      }
    const float add = a.table ? a.table[(size_t)tk * (size_t)a.tld + (size_t)o] : a.bias[o];
    const float f = requant(acc, add, a.scale[o], a.relu != 0);
    const size_t at = (size_t)(b * a.img_rows + a.t0 + tk) * (size_t)a.dst_ld + (size_t)o;
    switch (a.dst_dt) {
      case DFX_F32: reinterpret_cast<float *>(a.dst)[at] = f; break;
      case DFX_S32: reinterpret_cast<int *>(a.dst)[at] = cvt_x86_rt(f, a.rm); break;
      case DFX_S8: a.dst[at] = (unsigned char)sat_s8(cvt_x86_rt(f, a.rm)); break;
      default: a.dst[at] = (unsigned char)sat_u8_bits(cvt_x86_rt(f, a.rm));
    }
  }
  if (a.dst_dt == DFX_F32 || a.dst_dt == DFX_S32) pe_store_prefix<4>(a);
  else pe_store_prefix<1>(a);
}

// (lds is below the 64 KB every kernel may have without asking)
template <int BM, int DST, int G>
static int pe_one(const PeArgs &a, int grid, int lds, hipStream_t s, bool fast) {
  if (fast) patchembed_tile_kernel<BM, DST, true, G><<<grid, LIN_THREADS, lds, s>>>(a);
  else patchembed_tile_kernel<BM, DST, false, G><<<grid, LIN_THREADS, lds, s>>>(a);
  return 0;
}

template <int BM, int G>
static int pe_dst_one(const PeArgs &a, int grid, int lds, hipStream_t s, bool fast) {
  switch (a.dst_dt) {
    case DFX_F32: return pe_one<BM, DFX_F32, G>(a, grid, lds, s, fast);
    case DFX_S32: return pe_one<BM, DFX_S32, G>(a, grid, lds, s, fast);
    case DFX_S8: return pe_one<BM, DFX_S8, G>(a, grid, lds, s, fast);
    case DFX_U8: return pe_one<BM, DFX_U8, G>(a, grid, lds, s, fast);
  }
  return -1;
}

// -1: no such instance
int launch_patchembed_tile(const PeArgs &a, int bm, int g, int grid, int lds, hipStream_t s, bool fast) {
  if (bm == 128 && g == 16) return pe_dst_one<128, 16>(a, grid, lds, s, fast);
  if (bm == 128 && g == 4) return pe_dst_one<128, 4>(a, grid, lds, s, fast);
  if (bm == 64 && g == 16) return pe_dst_one<64, 16>(a, grid, lds, s, fast);
  if (bm == 64 && g == 4) return pe_dst_one<64, 4>(a, grid, lds, s, fast);
  return -1;
}

int launch_patchembed_generic(const PeArgs &a, int grid, hipStream_t s) {
  patchembed_generic_kernel<<<grid, LIN_THREADS, 0, s>>>(a);
  return 0;
}

}  // namespace dfx
