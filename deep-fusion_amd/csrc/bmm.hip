// bmm.hip -- the batched matrix product's kernels: the generic backstop (one thread per C element, any strides, the exact
// requant route; it defines the bits) and the instances of the MFMA kernel (bmm.cuh).
#include "bmm.cuh"

namespace dfx {

// ARGS: BmmArgs, or BmmBiasedArgs: requant's bias slot then holds the logit bias's entry
template <class ARGS>
__global__ __launch_bounds__(BMM_THREADS) void bmm_generic_kernel(ARGS a) {
  constexpr bool BIAS = bmm_biased<ARGS>::value;
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
    float bias = 0.0f;
    if constexpr (BIAS) bias = bmm_bias_row(a.bias.img, a.bias.p0, a.bias.p1, a.bias.rows, a.bias.cols, b0, b1, (int)m)[n];
    const float f = requant(acc, bias, a.scale[n], a.relu != 0);
    const size_t ci = (size_t)(b0 * a.c_s0 + b1 * a.c_s1 + m * a.ldc + n);
    switch (a.dst_dt) {
      case DFX_F32: reinterpret_cast<float *>(a.c)[ci] = f; break;
      case DFX_S32: reinterpret_cast<int *>(a.c)[ci] = cvt_x86_rt(f, a.rm); break;
      case DFX_S8: reinterpret_cast<signed char *>(a.c)[ci] = (signed char)sat_s8(cvt_x86_rt(f, a.rm)); break;
      default: a.c[ci] = (unsigned char)sat_u8_bits(cvt_x86_rt(f, a.rm)); break;
    }
  }
}

static BmmBiasedArgs bmm_with(const BmmArgs &a, const BmmBiasArgs &bias) {
  BmmBiasedArgs b;
  static_cast<BmmArgs &>(b) = a;
  b.bias = bias;
  return b;
}

template <bool NT, int DST>
static int bmm_one(const BmmArgs &a, const BmmBiasArgs *bias, int grid, hipStream_t s, bool fast) {
  if (bias) {
    const BmmBiasedArgs b = bmm_with(a, *bias);
    if (fast) bmm_mfma_kernel<NT, DST, true, BmmBiasedArgs><<<grid, BMM_THREADS, 0, s>>>(b);
    else bmm_mfma_kernel<NT, DST, false, BmmBiasedArgs><<<grid, BMM_THREADS, 0, s>>>(b);
  } else {
    if (fast) bmm_mfma_kernel<NT, DST, true, BmmArgs><<<grid, BMM_THREADS, 0, s>>>(a);
    else bmm_mfma_kernel<NT, DST, false, BmmArgs><<<grid, BMM_THREADS, 0, s>>>(a);
  }
  return 0;
}

template <bool NT>
static int bmm_form(const BmmArgs &a, const BmmBiasArgs *bias, int grid, hipStream_t s, bool fast) {
  switch (a.dst_dt) {
    case DFX_F32: return bmm_one<NT, DFX_F32>(a, bias, grid, s, fast);
    case DFX_S32: return bmm_one<NT, DFX_S32>(a, bias, grid, s, fast);
    case DFX_S8: return bmm_one<NT, DFX_S8>(a, bias, grid, s, fast);
    case DFX_U8: return bmm_one<NT, DFX_U8>(a, bias, grid, s, fast);
  }
  return -1;
}

// -1: no such instance.  bias: nullptr, or the logit bias of the biased kernels
int launch_bmm_mfma(const BmmArgs &a, const BmmBiasArgs *bias, int grid, hipStream_t s, bool fast) {
  return a.trans_b ? bmm_form<true>(a, bias, grid, s, fast) : bmm_form<false>(a, bias, grid, s, fast);
}

int launch_bmm_generic(const BmmArgs &a, const BmmBiasArgs *bias, int grid, hipStream_t s) {
  if (bias) bmm_generic_kernel<BmmBiasedArgs><<<grid, BMM_THREADS, 0, s>>>(bmm_with(a, *bias));
  else bmm_generic_kernel<BmmArgs><<<grid, BMM_THREADS, 0, s>>>(a);
  return 0;
}

}  // namespace dfx
