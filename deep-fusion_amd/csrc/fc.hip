// fc.hip -- the fully-connected op's kernels: the split-K MFMA kernel and the instances of its epilogue (fc.cuh), and
// the generic backstop (one thread per output value, any K, the exact requant route).
#include "fc.cuh"

namespace dfx {

__global__ __launch_bounds__(256) void fc_generic_kernel(FcArgs a) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < a.items; id += stride) {
    const int o = (int)(id % a.oc);
    const long long n = id / a.oc;
    const unsigned char *sp = a.src + (size_t)n * a.k;
    const signed char *wp = a.wraw + (size_t)o * a.k;
    int acc = 0;
    for (int y = 0; y < a.ih; ++y)
      for (int x = 0; x < a.iw; ++x) {
        const unsigned char *spx = sp + (size_t)(y * a.iw + x) * a.ic;
        const signed char *wpx = wp + y * a.iw + x;
        for (int c = 0; c < a.ic; ++c) acc += (int)spx[c] * (int)wpx[(size_t)c * a.ih * a.iw];
      }
    const float f = requant(acc, a.bias[o], a.scale[o], a.relu != 0);
    switch (a.dst_dt) {
      case DFX_F32: reinterpret_cast<float *>(a.dst)[id] = f; break;
      case DFX_S32: reinterpret_cast<int *>(a.dst)[id] = cvt_x86_rt(f, a.rm); break;
      case DFX_S8: reinterpret_cast<signed char *>(a.dst)[id] = (signed char)sat_s8(cvt_x86_rt(f, a.rm)); break;
      default: a.dst[id] = (unsigned char)sat_u8_bits(cvt_x86_rt(f, a.rm)); break;
    }
  }
}

// mode 0: launch; mode 1: admit `lds` bytes of dynamic LDS (once per handle, at create)
template <int NCB>
static int fc_one(const FcArgs &a, int grid, int lds, hipStream_t s, int mode) {
  if (mode == 1)
    return (int)hipFuncSetAttribute(reinterpret_cast<const void *>(fc_mfma_kernel<NCB>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  fc_mfma_kernel<NCB><<<grid, FC_THREADS, lds, s>>>(a);
  return 0;
}

// the instance for the chunk's column blocks, lds / (32 * FC_PITCH); -1: no such instance
int launch_fc_mfma(const FcArgs &a, int grid, int lds, hipStream_t s, int mode) {
  switch (lds / (32 * FC_PITCH)) {
    case 1: return fc_one<1>(a, grid, lds, s, mode);
    case 2: return fc_one<2>(a, grid, lds, s, mode);
    case 3: return fc_one<3>(a, grid, lds, s, mode);
    case 4: return fc_one<4>(a, grid, lds, s, mode);
  }
  return -1;
}

template <int DST>
static int fc_ep(const FcArgs &a, int grid, hipStream_t s, bool fast) {
  if (fast) fc_epilogue_kernel<DST, true><<<grid, 256, 0, s>>>(a);
  else fc_epilogue_kernel<DST, false><<<grid, 256, 0, s>>>(a);
  return 0;
}

// -1: no such instance
int launch_fc_epilogue(const FcArgs &a, int grid, hipStream_t s, bool fast) {
  switch (a.dst_dt) {
    case DFX_F32: return fc_ep<DFX_F32>(a, grid, s, fast);
    case DFX_S32: return fc_ep<DFX_S32>(a, grid, s, fast);
    case DFX_S8: return fc_ep<DFX_S8>(a, grid, s, fast);
    case DFX_U8: return fc_ep<DFX_U8>(a, grid, s, fast);
  }
  return -1;
}

int launch_fc_generic(const FcArgs &a, int grid, hipStream_t s) {
  fc_generic_kernel<<<grid, 256, 0, s>>>(a);
  return 0;
}

}  // namespace dfx
