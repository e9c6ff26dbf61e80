// attn.hip -- the instances and the launcher of the fused attention's kernel (attn.cuh).
#include "attn.cuh"

namespace dfx {

// mode 0: launch; mode 1: admit `lds` bytes of dynamic LDS for the instance (at create and whenever the routes change)
template <int DST, bool FL, bool FO, bool BIAS>
static int attn_one(const AttnArgs &a, int grid, int lds, hipStream_t s, int mode) {
  auto k = attn_fused_kernel<DST, FL, FO, BIAS>;
  if (mode == 1) return (int)hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  k<<<grid, ATTN_THREADS, lds, s>>>(a);
  return 0;
}

template <int DST, bool BIAS>
static int attn_routes(const AttnArgs &a, int grid, int lds, hipStream_t s, int mode, bool fl, bool fo) {
  if (fl) return fo ? attn_one<DST, true, true, BIAS>(a, grid, lds, s, mode) : attn_one<DST, true, false, BIAS>(a, grid, lds, s, mode);
  return fo ? attn_one<DST, false, true, BIAS>(a, grid, lds, s, mode) : attn_one<DST, false, false, BIAS>(a, grid, lds, s, mode);
}

template <int DST>
static int attn_dst(const AttnArgs &a, int grid, int lds, hipStream_t s, int mode, bool fl, bool fo, bool bias) {
  return bias ? attn_routes<DST, true>(a, grid, lds, s, mode, fl, fo) : attn_routes<DST, false>(a, grid, lds, s, mode, fl, fo);
}

// -1: no such instance; mode 1 returns the hipError_t of the attribute call.  `bias` chooses the biased instance (mode 0: a.bias
// must then be set)
int launch_attn_fused(const AttnArgs &a, int grid, int lds, hipStream_t s, int mode, bool fast_logits, bool fast_context, bool bias) {
  switch (a.dst_dt) {
    case DFX_F32: return attn_dst<DFX_F32>(a, grid, lds, s, mode, fast_logits, fast_context, bias);
    case DFX_S32: return attn_dst<DFX_S32>(a, grid, lds, s, mode, fast_logits, fast_context, bias);
    case DFX_S8: return attn_dst<DFX_S8>(a, grid, lds, s, mode, fast_logits, fast_context, bias);
    case DFX_U8: return attn_dst<DFX_U8>(a, grid, lds, s, mode, fast_logits, fast_context, bias);
  }
  return -1;
}

}  // namespace dfx
