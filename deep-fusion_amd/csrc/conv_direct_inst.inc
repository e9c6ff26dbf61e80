// conv_direct_inst.inc -- instantiates conv_direct_kernel for one dst dtype (DFX_INST_DST /
// DFX_INST_NAME come from the including .hip file) over (WO, G, WO1) and defines the launcher.
#include "conv_direct.cuh"

namespace dfx {

// (NW, WO, G, WO1, NPB): WO1 = 1 gives every wave one pixel block and ALL 1x1 groups (few groups); WO1 = NW gives
// every wave its own groups and all pixel blocks (each weight byte crosses the L2 port once or twice per unit)
#define DFX_FOR_EACH_DIRECT(X) X(4, 2, 2, 1, 4) X(4, 2, 4, 1, 4) X(4, 4, 2, 1, 4) X(4, 4, 4, 1, 4) X(4, 4, 4, 4, 4) \
                               X(4, 4, 4, 4, 2) X(4, 4, 4, 4, 1) X(4, 4, 2, 4, 2) X(4, 4, 2, 4, 1)                 \
                               X(8, 8, 4, 8, 4) X(8, 8, 4, 8, 2) X(8, 8, 4, 8, 1)

// mode 0: launch; mode 1: raise the dynamic-LDS limit (every requant specialisation); mode 2: resident workgroups per CU
template <int NWV, int W, int GG, int W1, int NP, int QM>
static int direct_one(const ConvArgs &a, const DirectGeom &g, int grid, int lds, hipStream_t s, int mode) {
  auto k = conv_direct_kernel<NWV, W, GG, W1, DFX_INST_DST, NP, QM>;
  if (mode == 1)
    return (int)hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (mode == 2) {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k, 64 * NWV, lds) != hipSuccess) return -1;
    return n;
  }
  k<<<grid, 64 * NWV, lds, s>>>(a, g);
  return 0;
}

int DFX_INST_NAME(const ConvArgs &a, const DirectGeom &g, int nw, int wo, int G, int wo1, int grid, int lds,
                  hipStream_t s, int mode) {
  // the requant specialisation follows the host's proofs (conv_weights.h, pack_streamed): g.m1 is only set together with g.m0
  const int qm = g.m1 == 3 ? 2 : (g.m1 == 2 ? 1 : 0);
#define X(NWV, W, GG, W1, NP)                                                                    \
  if (nw == NWV && wo == W && G == GG && wo1 == W1 && g.npb == NP) {                          \
    if constexpr (DFX_INST_DST == DFX_U8 && GG == 4) {                                         \
      if (mode == 1) {                                                                         \
        const int r1 = direct_one<NWV, W, GG, W1, NP, 1>(a, g, grid, lds, s, 1);               \
        const int r2 = direct_one<NWV, W, GG, W1, NP, 2>(a, g, grid, lds, s, 1);               \
        if (r1 != 0 || r2 != 0) return r1 != 0 ? r1 : r2;                                      \
      } else if (mode == 0 && qm == 1) {                                                       \
        return direct_one<NWV, W, GG, W1, NP, 1>(a, g, grid, lds, s, 0);                       \
      } else if (mode == 0 && qm == 2) {                                                       \
        return direct_one<NWV, W, GG, W1, NP, 2>(a, g, grid, lds, s, 0);                       \
      }                                                                                        \
    }                                                                                          \
    return direct_one<NWV, W, GG, W1, NP, 0>(a, g, grid, lds, s, mode);                        \
  }
  DFX_FOR_EACH_DIRECT(X)
#undef X
  return -1;
}

}  // namespace dfx
