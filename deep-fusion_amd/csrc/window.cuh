// window.cuh -- kernels of the window partition / reverse op (dfx_window_* of include/dfx.h; gfx950).  Data movement only,
// HBM-bound, no LDS.  Shift, padding, order and direction exist only in the row map the host built (window_plan.h): both
// kernels are row gathers with contiguous stores,
//     dst row (b, r)  <-  src row b * src_img + map[r]        (map[r] < 0, PARTITION only: a pad token, filled with `pad`)
// with every byte offset computed in 64 bits.
//
//   window_generic_kernel   one thread per element, any alignment and pitch, grid-stride: defines the bits
//   window_row_kernel       a lane moves one 16-byte group; `lanes` = c * esize / 16 consecutive lanes per token (any count), and
//                           consecutive lanes run on into the next destination row: stores are contiguous, loads contiguous
//                           in runs of at least one token.  A workgroup trip covers 256 * WINDOW_UNROLL consecutive groups;
//                           where that run starts (row, image, lane within the token) is divided out once per trip on
//                           uniform values, a lane adds its small 32-bit share.  The lanes of a token read the same map
//                           entry, one request.  All of a trip's loads are issued before its first store.
#pragma once

#include "dfx_device.cuh"
#include "window_plan.h"

namespace dfx {

struct WindowArgs {
  const unsigned char *src;
  unsigned char *dst;
  const int *map;                // the handle's device image: dst_img entries
  long long rows;                // bs * dst_img destination rows
  long long src_img;             // source rows per image
  long long src_pitch, dst_pitch;  // bytes between rows
  int dst_img;                   // destination rows per image, <= 2^22
  int c, esize;
  int lanes;                     // row kernel: 16-byte groups per token
  unsigned pad;                  // the pad pattern as a dword (a 1-byte value replicated)
};

#ifdef DFX_WINDOW_KERNELS

__global__ __launch_bounds__(256) void window_generic_kernel(WindowArgs a) {
  const long long total = a.rows * a.c, stride = (long long)gridDim.x * 256;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
    const long long row = e / a.c;
    const long long col = e - row * a.c;
    const long long b = row / a.dst_img;
    const int m = a.map[row - b * a.dst_img];
    const size_t o = (size_t)row * a.dst_pitch + (size_t)col * a.esize;
    const size_t i = (size_t)(b * a.src_img + m) * a.src_pitch + (size_t)col * a.esize;  // (used where m >= 0)
    if (a.esize == 1) a.dst[o] = m < 0 ? (unsigned char)a.pad : a.src[i];
    else *reinterpret_cast<unsigned *>(a.dst + o) = m < 0 ? a.pad : *reinterpret_cast<const unsigned *>(a.src + i);
  }
}

__global__ __launch_bounds__(256) void window_row_kernel(WindowArgs a) {
  constexpr int U = WINDOW_UNROLL;
  const unsigned lanes = (unsigned)a.lanes, dst_img = (unsigned)a.dst_img;
  const long long total = a.rows * a.lanes, per = 256 * U;
  const v4i padv = {(int)a.pad, (int)a.pad, (int)a.pad, (int)a.pad};
  for (long long base = (long long)blockIdx.x * per; base < total; base += (long long)gridDim.x * per) {
    // where the trip's first group lies: uniform over the workgroup
    const long long row0 = base / lanes;
    const unsigned rem0 = (unsigned)(base - row0 * lanes);
    const long long b0 = row0 / dst_img;
    const unsigned r0 = (unsigned)(row0 - b0 * dst_img);
    // three passes, so that the trip's map entries, then its data loads, are in flight together
    bool ok[U];
    int m[U];
    long long src_row0[U];   // the image's first source row
    size_t dst_off[U];
    unsigned lane16[U];
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const unsigned k = (unsigned)j * 256 + threadIdx.x;   // the lane's group within the trip
      ok[j] = base + k < total;
      const unsigned t = rem0 + k;                          // < lanes + 256 * U
      const unsigned dr = t / lanes;
      lane16[j] = (t - dr * lanes) * 16;
      const unsigned rr = r0 + dr;                          // < 2^22 + 256 * U
      const unsigned db = rr / dst_img;
      m[j] = ok[j] ? a.map[rr - db * dst_img] : -1;
      src_row0[j] = (b0 + db) * a.src_img;
      dst_off[j] = (size_t)(row0 + dr) * a.dst_pitch + lane16[j];
    }
    v4i v[U];
#pragma unroll
    for (int j = 0; j < U; ++j) {
      v[j] = padv;
      if (m[j] >= 0) v[j] = *reinterpret_cast<const v4i *>(a.src + (size_t)(src_row0[j] + m[j]) * a.src_pitch + lane16[j]);
    }
#pragma unroll
    for (int j = 0; j < U; ++j)
      if (ok[j]) dfx_store16(reinterpret_cast<v4i *>(a.dst + dst_off[j]), v[j]);
  }
}

#endif  // DFX_WINDOW_KERNELS

}  // namespace dfx
