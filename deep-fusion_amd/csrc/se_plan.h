// se_plan.h -- host-only, plain C++: how the squeeze kernel of the squeeze-and-excitation op (se.cuh) cuts an image into
// work.  A workgroup of 256 lanes takes one (image, slice of pixels, chunk of channel groups); a lane owns one 16-channel
// group and walks the slice's pixels `pln` apart, adding bytes as packed 16-bit halves that it flushes to s32 after
// SE_FLUSH pixels at the latest (255 * 257 = 65535).  No HIP in here, so that it can be built and run on its own
// (tools/se_plan_check.cc, under the host sanitizers).
#pragma once

#include <algorithm>

namespace dfx {

constexpr int SE_THREADS = 256;
constexpr int SE_FLUSH = 257;         // pixels a packed 16-bit accumulator takes: 255 * 257 = 65535
constexpr int SE_MIN_SLICE_PX = 64;   // a slice the planner makes has at least this many pixels
constexpr int SE_MAX_PX = 1 << 23;    // ih * iw: 255 * 2^23 < 2^31
constexpr int SE_MAX_C = 16384;       // c and cr: 255 * 127 * 16384 < 2^31

struct SePlan {
  int groups;   // 16-channel groups per pixel
  int gl;       // groups a workgroup takes at once: min(groups, 256)
  int gchunks;  // ceil(groups / gl)
  int pln;      // pixel lanes per group: 256 / gl; a lane walks the slice's pixels pln apart
  int parts;    // second reduction stage: lanes per channel, 1 = none
  int slices;   // pixel slices per image
  long long items;  // workgroup items: bs * slices * gchunks
};

// first pixel of slice s (s == slices: one past the last pixel); floor(s * px / slices) rises strictly while slices <= px
inline int se_slice_begin(int px, int slices, int s) { return (int)((long long)s * px / slices); }

// pixels the lane `pl` of a slice [p0, p1) visits: p0 + pl, p0 + pl + pln, ...
inline int se_lane_pixels(int p0, int p1, int pl, int pln) { return p0 + pl >= p1 ? 0 : (p1 - p0 - pl + pln - 1) / pln; }

// the longest run a lane adds into its packed accumulators before a flush, for `n` pixels of its own
inline int se_flush_run(int n) { return std::min(n, SE_FLUSH); }

// c % 16 == 0, 1 <= px <= SE_MAX_PX, bs >= 1, cus >= 1.  forced_slices <= 0: the planner's own count, at least two
// workgroups per CU where the tensor allows it and at least SE_MIN_SLICE_PX pixels per slice; else that count, clamped
// to 1 .. px.
inline SePlan se_plan(long long bs, int px, int c, int cus, long long forced_slices) {
  SePlan p;
  p.groups = c / 16;
  p.gl = std::min(p.groups, SE_THREADS);
  p.gchunks = (p.groups + p.gl - 1) / p.gl;
  p.pln = SE_THREADS / p.gl;
  const int nch = 16 * p.gl;
  p.parts = std::max(1, std::min(p.pln, SE_THREADS / nch));
  long long s;
  if (forced_slices > 0) {
    s = forced_slices;
  } else {
    const long long per_slice = bs * p.gchunks;
    s = (2ll * cus + per_slice - 1) / per_slice;
    s = std::min<long long>(s, px / SE_MIN_SLICE_PX);
  }
  p.slices = (int)std::max<long long>(1, std::min<long long>(s, px));
  p.items = bs * p.slices * p.gchunks;
  return p;
}

}  // namespace dfx
