// bmm.hip -- the batched matrix product's kernels: the generic backstop (one thread per C element, any strides, the exact
// requant route; it defines the bits) and the instances of the MFMA kernel (bmm.cuh).
#include "bmm.cuh"

namespace dfx {

__global__ __launch_bounds__(BMM_THREADS) void bmm_generic_kernel(BmmArgs a) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long per = (long long)a.m * a.n;
  for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < a.items; id += stride) {
    const long long g = id / per, r = id % per;
    const long long m = r / a.n, n = r % a.n;
    const long long b0 = g / a.batch1, b1 = g % a.batch1;
    const unsigned char *ap = a.a + (size_t)(b0 * a.a_s0 + b1 * a.a_s1 + m * a.lda);
    const signed char *bp = a.b + (size_t)(b0 * a.b_s0 + b1 * a.b_s1 + (a.trans_b ? n * a.ldb : n));
    const long long bstep = a.trans_b ? 1 : a.ldb;
    int acc = 0;
    if (a.a_u8)
      for (int k = 0; k < a.k; ++k) acc += (int)ap[k] * (int)bp[(size_t)(k * bstep)];
    else
      for (int k = 0; k < a.k; ++k) acc += (int)(signed char)ap[k] * (int)bp[(size_t)(k * bstep)];
    const float f = requant(acc, 0.0f, a.scale[n], a.relu != 0);
    const size_t ci = (size_t)(b0 * a.c_s0 + b1 * a.c_s1 + m * a.ldc + n);
    switch (a.dst_dt) {
      case DFX_F32: reinterpret_cast<float *>(a.c)[ci] = f; break;
      case DFX_S32: reinterpret_cast<int *>(a.c)[ci] = cvt_x86_rt(f, a.rm); break;
      case DFX_S8: reinterpret_cast<signed char *>(a.c)[ci] = (signed char)sat_s8(cvt_x86_rt(f, a.rm)); break;
      default: a.c[ci] = (unsigned char)sat_u8_bits(cvt_x86_rt(f, a.rm)); break;
    }
  }
}

template <bool NT, int DST>
static int bmm_one(const BmmArgs &a, int grid, hipStream_t s, bool fast) {
  if (fast) bmm_mfma_kernel<NT, DST, true><<<grid, BMM_THREADS, 0, s>>>(a);
  else bmm_mfma_kernel<NT, DST, false><<<grid, BMM_THREADS, 0, s>>>(a);
  return 0;
}

template <bool NT>
static int bmm_form(const BmmArgs &a, int grid, hipStream_t s, bool fast) {
  switch (a.dst_dt) {
    case DFX_F32: return bmm_one<NT, DFX_F32>(a, grid, s, fast);
    case DFX_S32: return bmm_one<NT, DFX_S32>(a, grid, s, fast);
    case DFX_S8: return bmm_one<NT, DFX_S8>(a, grid, s, fast);
    case DFX_U8: return bmm_one<NT, DFX_U8>(a, grid, s, fast);
  }
  return -1;
}

// -1: no such instance
int launch_bmm_mfma(const BmmArgs &a, int grid, hipStream_t s, bool fast) {
  return a.trans_b ? bmm_form<true>(a, grid, s, fast) : bmm_form<false>(a, grid, s, fast);
}

int launch_bmm_generic(const BmmArgs &a, int grid, hipStream_t s) {
  bmm_generic_kernel<<<grid, BMM_THREADS, 0, s>>>(a);
  return 0;
}

}  // namespace dfx
