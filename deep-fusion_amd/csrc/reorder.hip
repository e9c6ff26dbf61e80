// reorder.hip -- activation reorder: layout (NHWC <-> NCHW), dtype and scale conversion, channel pad / crop
// (gfx950).  The reference ships no such op (its tests and benches lean on MKL-DNN's reorder primitive);
// parity is unpinned, the semantics are MKL-DNN's saturating reorder:
//
//   dst[n,k,y,x] = k < src_c ? cvt(float(src[n,k,y,x]) * scale[k]) : 0          for every k < dst_c
//
// float(): u8 / s8 exact, s32 round-to-nearest-even, f32 as is.  The multiply is ONE separately rounded f32
// operation (__fmul_rn; the library is built with -ffp-contract=off and without flush-to-zero, so denormal
// values pass through).  cvt() for an f32 dst is the identity; for u8 / s8 it is rint() (ties to even) or
// floor(), NaN -> 0, then a clamp to [0,255] / [-128,127].  This is NOT the conv epilogue's conversion
// (dfx_device.cuh: cvt_x86 + vpmovusdb on the bit pattern, where an out-of-range value becomes 0x80000000 and
// saturates from there): a reorder saturates the VALUE, +inf -> 255, -inf -> 0 / -128.
//
// Four kernels, all HBM-bound, both global sides coalesced:
//   flat       same layout, src_c == dst_c: every lane moves 16 bytes of the wider-typed side (4 elements when
//              either side is 4-byte, 16 when both are 1-byte) in a grid-stride loop over tiles of 256 lanes.
//   generic    same layout with channel pad / crop: one dst element per lane (an NHWC pixel is its own short run).
//   smallc     NCHW with src_c <= 4 -> NHWC with dst_c <= 16 (the image case, 3 -> 16): no LDS; a lane reads its
//              pixels from the few planes (consecutive lanes, consecutive pixels; 4 pixels per lane, all loads
//              issued before the first store) and writes whole padded pixels.
//   transpose  NCHW <-> NHWC: a workgroup takes TP (64; 32 for tiny images) consecutive pixels of one image times a
//              block of channels and stages it through LDS.  The plane side (contiguous pixels of one channel) and
//              the pixel side (contiguous channels of consecutive pixels) are both 16-byte-per-lane accesses when
//              the tensor's geometry keeps every tile 16-byte aligned (plane side: h*w*elsize % 16 == 0; pixel
//              side: c*elsize % 16 == 0), else one element per lane in the same order (7x7 f32 planes, 13x17 u8
//              planes ...).  The channel block is 128 bytes (4-byte types) or 64 bytes (1-byte types) of the pixel
//              side: 8 - 16 KiB of LDS, 8 workgroups per CU -- measured faster than deeper tiles, and a tensor no
//              deeper than one block has the pixel side of a tile as ONE contiguous span.  When c*elsize % 16 != 0
//              the block is the whole depth instead (if min(src_c, dst_c) rows fit in 48 KiB) and the span is
//              walked in 16-byte chunks where h*w*c*elsize % 16 == 0.  For pixel-side loads a lane issues the
//              loads of 4 chunks before it converts the first.
//   LDS layout of the transpose: 32-bit words (the converted dst value), tile[k][p] with a row stride of
//   S = TP + 1 words, all accesses ds_*_b32.  S is odd and TP a multiple of 32, so within a 32-lane group
//     plane side: lane (k, j) touches word k*S + V*j + e  (V = 4 or 16 pixels per lane) -> bank (k + V*j + e) % 32:
//                 rows differ by 1 bank, V*j wraps once per row pair -> 2-way at worst;
//     pixel side: lane (p, g) touches word (V*g + i)*S + p -> bank (V*g + i + p) % 32 -> 2-way at worst
//   in both directions (write and transposed read).
//
// Addressing: a tile's base is a 64-bit offset, everything inside a tile is a 32-bit element offset (the host
// refuses images of 2^31 elements or more), so tensors beyond 2^31 bytes work.
#include "dfx_device.cuh"

namespace dfx {

namespace {

template <int DT> struct dt_bytes { static constexpr int v = (DT == DFX_F32 || DT == DFX_S32) ? 4 : 1; };

// element e of a 16-byte (or, in its low word, 4-byte) chunk of SDT elements, as the float the semantics start from
template <int SDT>
__device__ __forceinline__ float chunk_elem(const v4i &raw, int e) {
  if (SDT == DFX_F32) return __int_as_float(raw[e]);
  if (SDT == DFX_S32) return __int2float_rn(raw[e]);
  const int w = raw[e >> 2] >> (8 * (e & 3));
  if (SDT == DFX_U8) return (float)(w & 0xff);
  return (float)(int)(int8_t)(w & 0xff);
}
template <int SDT>
__device__ __forceinline__ float load1(const unsigned char *base, unsigned idx) {
  if (SDT == DFX_F32) return reinterpret_cast<const float *>(base)[idx];
  if (SDT == DFX_S32) return __int2float_rn(reinterpret_cast<const int *>(base)[idx]);
  if (SDT == DFX_U8) return (float)base[idx];
  return (float)(int)reinterpret_cast<const int8_t *>(base)[idx];
}
// the converted value as a 32-bit word: f32 bits, or the saturated integer
template <int DDT>
__device__ __forceinline__ int convert(float v, float scale, int rm) {
  v = __fmul_rn(v, scale);
  if (DDT == DFX_F32) return __float_as_int(v);
  float r = rm ? __builtin_floorf(v) : __builtin_rintf(v);
  const float lo = DDT == DFX_U8 ? 0.0f : -128.0f, hi = DDT == DFX_U8 ? 255.0f : 127.0f;
  r = (v != v) ? 0.0f : r;
  r = r < lo ? lo : (r > hi ? hi : r);
  return (int)r;
}
template <int DDT>
__device__ __forceinline__ void chunk_put(v4i &out, int e, int word) {
  if (dt_bytes<DDT>::v == 4) out[e] = word;
  else out[e >> 2] |= (word & 0xff) << (8 * (e & 3));
}
template <int DDT>
__device__ __forceinline__ void store1(unsigned char *base, unsigned idx, int word) {
  if (dt_bytes<DDT>::v == 4) reinterpret_cast<int *>(base)[idx] = word;
  else base[idx] = (unsigned char)word;
}

// ---- flat: same layout, same channel count ----
template <int SDT, int DDT>
__global__ __launch_bounds__(256) void reorder_flat_kernel(ReorderArgs a) {
  constexpr int ES = dt_bytes<SDT>::v, ED = dt_bytes<DDT>::v;
  constexpr int V = 16 / (ES > ED ? ES : ED);
  const long long tile_elems = 256 * V;
  const long long ntiles = (a.total + tile_elems - 1) / tile_elems;
  const float s0 = a.scales[0];
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long base = t * tile_elems;
    const unsigned off = threadIdx.x * V;
    if (base + off >= a.total) continue;
    const long long left = a.total - base - off;
    // channel of this lane's first element: (index / inner) % c, inner = 1 (NHWC) or h*w (NCHW)
    int k = 0;
    unsigned r = 0;
    if (!a.uniform_scale) {
      const long long q = base / a.inner;
      const unsigned rr = (unsigned)(base - q * a.inner) + off;  // < inner + 4096
      const unsigned dq = rr / (unsigned)a.inner;
      r = rr - dq * (unsigned)a.inner;
      k = (int)(((unsigned)(q % a.src_c) + dq) % (unsigned)a.src_c);
    }
    const unsigned char *sp = a.src + (size_t)base * ES;
    unsigned char *dp = a.dst + (size_t)base * ED;
    if (left >= V) {
      v4i raw = {0, 0, 0, 0};
      if (V * ES == 16) raw = *reinterpret_cast<const v4i *>(sp + (size_t)off * ES);
      else raw[0] = *reinterpret_cast<const int *>(sp + (size_t)off * ES);
      v4i out = {0, 0, 0, 0};
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float sc = a.uniform_scale ? s0 : a.scales[k];
        chunk_put<DDT>(out, e, convert<DDT>(chunk_elem<SDT>(raw, e), sc, a.rm));
        if (!a.uniform_scale && ++r == (unsigned)a.inner) {
          r = 0;
          if (++k == a.src_c) k = 0;
        }
      }
      if (V * ED == 16) dfx_store16(reinterpret_cast<v4i *>(dp + (size_t)off * ED), out);
      else *reinterpret_cast<int *>(dp + (size_t)off * ED) = out[0];
    } else {  // the tensor's last, partial chunk: element by element
      for (int e = 0; e < (int)left; ++e) {
        const float sc = a.uniform_scale ? s0 : a.scales[k];
        store1<DDT>(dp, off + e, convert<DDT>(load1<SDT>(sp, off + e), sc, a.rm));
        if (!a.uniform_scale && ++r == (unsigned)a.inner) {
          r = 0;
          if (++k == a.src_c) k = 0;
        }
      }
    }
  }
}

// ---- generic: same layout, channel pad / crop; one dst element per lane ----
template <int SDT, int DDT>
__global__ __launch_bounds__(256) void reorder_generic_kernel(ReorderArgs a) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long per_image = (long long)a.dst_c * a.hw;
  for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < a.total; id += stride) {
    const long long n = id / per_image;
    const unsigned w = (unsigned)(id - n * per_image);
    unsigned k, p;
    if (a.dst_fmt == DFX_FMT_NHWC) {
      p = w / (unsigned)a.dst_c;
      k = w - p * (unsigned)a.dst_c;
    } else {
      k = w / (unsigned)a.hw;
      p = w - k * (unsigned)a.hw;
    }
    int word = 0;
    if ((int)k < a.src_c) {
      const unsigned char *sp = a.src + (size_t)n * a.src_c * a.hw * dt_bytes<SDT>::v;
      const unsigned so = a.src_fmt == DFX_FMT_NHWC ? p * (unsigned)a.src_c + k : k * (unsigned)a.hw + p;
      word = convert<DDT>(load1<SDT>(sp, so), a.scales[k], a.rm);
    }
    store1<DDT>(a.dst + (size_t)n * per_image * dt_bytes<DDT>::v, w, word);
  }
}

// ---- smallc: NCHW src_c <= 4 -> NHWC dst_c <= 16; whole pixels per lane, no LDS ----
// the padded pixel of one lane: channels 0..3 from `word`, the rest zero
template <int DDT>
__device__ __forceinline__ void smallc_store(unsigned char *dp, const int (&word)[4], int dst_c) {
  constexpr int ED = dt_bytes<DDT>::v;
  const int bytes = dst_c * ED;
  if (bytes % 16 == 0) {
    v4i out = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k) chunk_put<DDT>(out, k, word[k]);  // channels 0..3 sit in the first chunk
    dfx_store16(reinterpret_cast<v4i *>(dp), out);
    const v4i zero = {0, 0, 0, 0};
    for (int c = 1; c < bytes / 16; ++c) dfx_store16(reinterpret_cast<v4i *>(dp) + c, zero);
  } else if (bytes % 4 == 0) {
    for (int c = 0; c < bytes / 4; ++c) {
      int w = 0;
      if (ED == 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) w = (c == k) ? word[k] : w;
      } else if (c == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) w |= (word[k] & 0xff) << (8 * k);
      }
      reinterpret_cast<int *>(dp)[c] = w;
    }
  } else {
    for (int c = 0; c < dst_c; ++c) {
      int w = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) w = (c == k) ? word[k] : w;
      store1<DDT>(dp, c, w);
    }
  }
}

// A workgroup takes SMALLC_PX consecutive pixels of one image; a lane takes pixels tid, tid + 256, ... of them (every
// load and store instruction of a wave covers consecutive pixels) and issues all its loads before the first store.
template <int SDT, int DDT>
__global__ __launch_bounds__(256) void reorder_smallc_kernel(ReorderArgs a) {
  constexpr int U = SMALLC_PX / 256;
  const int n = blockIdx.x / a.ptiles;
  const int p0 = (blockIdx.x - n * a.ptiles) * SMALLC_PX + threadIdx.x;
  const unsigned char *sp = a.src + (size_t)n * a.src_c * a.hw * dt_bytes<SDT>::v;
  float v[U][4];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int p = p0 + u * 256;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[u][k] = 0.0f;
      if (p < a.hw && k < a.src_c && k < a.dst_c) v[u][k] = load1<SDT>(sp, (unsigned)k * a.hw + p);
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int p = p0 + u * 256;
    if (p >= a.hw) continue;
    int word[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) word[k] = (k < a.src_c && k < a.dst_c) ? convert<DDT>(v[u][k], a.scales[k], a.rm) : 0;
    smallc_store<DDT>(a.dst + ((size_t)n * a.hw + p) * a.dst_c * dt_bytes<DDT>::v, word, a.dst_c);
  }
}

// ---- transpose ----
enum { MAP_PLANE = 0, MAP_PIXROWS = 1, MAP_PIXFLAT = 2 };

// (k, p) of the element after (k, p) along a row of the side
template <int MAP>
__device__ __forceinline__ void advance(int &k, int &p, int C) {
  if (MAP == MAP_PLANE) ++p;
  else if (MAP == MAP_PIXROWS) ++k;
  else if (++k == C) { k = 0; ++p; }
}

// One side of a tile is R rows of RL elements, `pitch` elements apart, starting at g.  Element `w` of row `row` is
// (channel, pixel) of the tile:  MAP_PLANE (row, w)   MAP_PIXROWS (w, row)   MAP_PIXFLAT (w % C, w / C).
// V elements per lane and access: 16 / element size when the host found every tile aligned, else 1; a chunk
// that would cross the end of its row goes element by element.  Channels >= kvalid of the tile hold no data.
template <int SDT, int DDT, int V, int MAP, int U>
__device__ __forceinline__ void side_load(const ReorderArgs &a, const unsigned char *g, int R, int RL, int pitch,
                                          int k0, int kvalid, int C, int S, int *lds) {
  // U chunks a lane has in flight: all U loads are issued before the first conversion
  const int cpr = (RL + V - 1) / V, nchunks = R * cpr;
  for (int q0 = threadIdx.x; q0 < nchunks; q0 += U * blockDim.x) {
    v4i raw[U];
    int rows[U], w0s[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int q = q0 + u * blockDim.x;
      raw[u] = v4i{0, 0, 0, 0};
      rows[u] = q / cpr;
      w0s[u] = (q - rows[u] * cpr) * V;
      if (q >= nchunks) continue;
      const unsigned off = (unsigned)rows[u] * (unsigned)pitch + w0s[u];
      if (V > 1) {
        if (w0s[u] + V <= RL) raw[u] = *reinterpret_cast<const v4i *>(g + (size_t)off * dt_bytes<SDT>::v);
      } else {
        raw[u][0] = __float_as_int(load1<SDT>(g, off));
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (q0 + u * blockDim.x >= nchunks) continue;
      const int row = rows[u], w0 = w0s[u];
      int k, p;
      if (MAP == MAP_PLANE) { k = row; p = w0; }
      else if (MAP == MAP_PIXROWS) { p = row; k = w0; }
      else { p = w0 / C; k = w0 - p * C; }
      if (V == 1) {
        if (k < kvalid) lds[k * S + p] = convert<DDT>(__int_as_float(raw[u][0]), a.scales[k0 + k], a.rm);
      } else if (w0 + V <= RL) {
#pragma unroll
        for (int e = 0; e < V; ++e) {
          if (k < kvalid) lds[k * S + p] = convert<DDT>(chunk_elem<SDT>(raw[u], e), a.scales[k0 + k], a.rm);
          advance<MAP>(k, p, C);
        }
      } else {  // a chunk that would cross the end of its row
        const unsigned off = (unsigned)row * (unsigned)pitch + w0;
        for (int e = 0; e < V && w0 + e < RL; ++e) {
          if (k < kvalid) lds[k * S + p] = convert<DDT>(load1<SDT>(g, off + e), a.scales[k0 + k], a.rm);
          advance<MAP>(k, p, C);
        }
      }
    }
  }
}

template <int DDT, int V, int MAP>
__device__ __forceinline__ void side_store(unsigned char *g, int R, int RL, int pitch, int kvalid, int C, int S,
                                           const int *lds) {
  const int cpr = (RL + V - 1) / V;
  for (int q = threadIdx.x; q < R * cpr; q += blockDim.x) {
    const int row = q / cpr, w0 = (q - row * cpr) * V;
    const unsigned off = (unsigned)row * (unsigned)pitch + w0;
    int k, p;
    if (MAP == MAP_PLANE) { k = row; p = w0; }
    else if (MAP == MAP_PIXROWS) { p = row; k = w0; }
    else { p = w0 / C; k = w0 - p * C; }
    if (V > 1 && w0 + V <= RL) {
      v4i out = {0, 0, 0, 0};
#pragma unroll
      for (int e = 0; e < V; ++e) {
        chunk_put<DDT>(out, e, k < kvalid ? lds[k * S + p] : 0);
        advance<MAP>(k, p, C);
      }
      dfx_store16(reinterpret_cast<v4i *>(g + (size_t)off * dt_bytes<DDT>::v), out);
    } else {
      for (int e = 0; e < V && w0 + e < RL; ++e) {
        store1<DDT>(g, off + e, k < kvalid ? lds[k * S + p] : 0);
        advance<MAP>(k, p, C);
      }
    }
  }
}

template <int SDT, int DDT, bool TO_NHWC>
__global__ __launch_bounds__(256) void reorder_transpose_kernel(ReorderArgs a) {
  extern __shared__ int lds[];
  // chunks a lane loads before it converts the first.  Measured: pixel-side loads gain 17 % from 4
  // in flight, plane-side loads lose 12 %.
  constexpr int U = TO_NHWC ? 1 : 4;
  constexpr int ES = dt_bytes<SDT>::v, ED = dt_bytes<DDT>::v;
  constexpr int VS = 16 / ES, VD = 16 / ED;
  const int cbk = blockIdx.x % a.cblocks;
  const int t = blockIdx.x / a.cblocks;
  const int pt = t % a.ptiles, n = t / a.ptiles;
  const int p0 = pt * a.tp, np = min(a.tp, a.hw - p0);
  const int k0 = cbk * a.cb;                   // first channel of the block (0 when the block is the whole depth)
  const int cl = min(a.src_c, a.dst_c);        // channels that carry data
  const int kvalid = max(0, min(a.cb, cl - k0));
  const int S = a.tp + 1;
  if (TO_NHWC) {  // plane-side load, pixel-side store
    const unsigned char *g = a.src + (((size_t)n * a.src_c + k0) * a.hw + p0) * ES;
    if (a.vec_plane) side_load<SDT, DDT, VS, MAP_PLANE, U>(a, g, kvalid, np, a.hw, k0, kvalid, 0, S, lds);
    else side_load<SDT, DDT, 1, MAP_PLANE, U>(a, g, kvalid, np, a.hw, k0, kvalid, 0, S, lds);
    __syncthreads();
    if (a.flat_pixel) {
      unsigned char *d = a.dst + ((size_t)n * a.hw + p0) * a.dst_c * ED;
      if (a.vec_pixel) side_store<DDT, VD, MAP_PIXFLAT>(d, 1, np * a.dst_c, 0, kvalid, a.dst_c, S, lds);
      else side_store<DDT, 1, MAP_PIXFLAT>(d, 1, np * a.dst_c, 0, kvalid, a.dst_c, S, lds);
    } else {
      unsigned char *d = a.dst + (((size_t)n * a.hw + p0) * a.dst_c + k0) * ED;
      const int rl = min(a.cb, a.dst_c - k0);
      if (a.vec_pixel) side_store<DDT, VD, MAP_PIXROWS>(d, np, rl, a.dst_c, kvalid, 0, S, lds);
      else side_store<DDT, 1, MAP_PIXROWS>(d, np, rl, a.dst_c, kvalid, 0, S, lds);
    }
  } else {  // pixel-side load, plane-side store
    if (a.flat_pixel) {
      const unsigned char *g = a.src + ((size_t)n * a.hw + p0) * a.src_c * ES;
      if (a.vec_pixel) side_load<SDT, DDT, VS, MAP_PIXFLAT, U>(a, g, 1, np * a.src_c, 0, 0, kvalid, a.src_c, S, lds);
      else side_load<SDT, DDT, 1, MAP_PIXFLAT, U>(a, g, 1, np * a.src_c, 0, 0, kvalid, a.src_c, S, lds);
    } else {
      const unsigned char *g = a.src + (((size_t)n * a.hw + p0) * a.src_c + k0) * ES;
      const int rl = max(0, min(a.cb, a.src_c - k0));
      if (a.vec_pixel) side_load<SDT, DDT, VS, MAP_PIXROWS, U>(a, g, np, rl, a.src_c, k0, kvalid, 0, S, lds);
      else side_load<SDT, DDT, 1, MAP_PIXROWS, U>(a, g, np, rl, a.src_c, k0, kvalid, 0, S, lds);
    }
    __syncthreads();
    unsigned char *d = a.dst + (((size_t)n * a.dst_c + k0) * a.hw + p0) * ED;
    const int rows = min(a.cb, a.dst_c - k0);
    if (a.vec_plane) side_store<DDT, VD, MAP_PLANE>(d, rows, np, a.hw, kvalid, 0, S, lds);
    else side_store<DDT, 1, MAP_PLANE>(d, rows, np, a.hw, kvalid, 0, S, lds);
  }
}

template <int SDT, int DDT>
int launch_typed(const ReorderArgs &a, hipStream_t s) {
  switch (a.path) {
    case REORDER_FLAT: reorder_flat_kernel<SDT, DDT><<<a.grid, 256, 0, s>>>(a); return 0;
    case REORDER_GENERIC: reorder_generic_kernel<SDT, DDT><<<a.grid, 256, 0, s>>>(a); return 0;
    case REORDER_SMALLC: reorder_smallc_kernel<SDT, DDT><<<a.grid, 256, 0, s>>>(a); return 0;
    case REORDER_TRANSPOSE:
      if (a.dst_fmt == DFX_FMT_NHWC) reorder_transpose_kernel<SDT, DDT, true><<<a.grid, 256, a.lds_bytes, s>>>(a);
      else reorder_transpose_kernel<SDT, DDT, false><<<a.grid, 256, a.lds_bytes, s>>>(a);
      return 0;
  }
  return 1;
}

template <int SDT>
int launch_src(const ReorderArgs &a, hipStream_t s) {
  switch (a.dst_dt) {
    case DFX_F32: return launch_typed<SDT, DFX_F32>(a, s);
    case DFX_S8: return launch_typed<SDT, DFX_S8>(a, s);
    case DFX_U8: return launch_typed<SDT, DFX_U8>(a, s);
  }
  return 1;
}

}  // namespace

// 0 = launched; 1 = a dtype / path the host should have refused
int launch_reorder(const ReorderArgs &a, hipStream_t s) {
  switch (a.src_dt) {
    case DFX_F32: return launch_src<DFX_F32>(a, s);
    case DFX_S32: return launch_src<DFX_S32>(a, s);
    case DFX_S8: return launch_src<DFX_S8>(a, s);
    case DFX_U8: return launch_src<DFX_U8>(a, s);
  }
  return 1;
}

}  // namespace dfx
