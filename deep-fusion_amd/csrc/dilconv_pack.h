// dilconv_pack.h -- host-only: the weight image of the dilated conv's MFMA kernel (dilconv.cuh).  No HIP in here, so
// that the packer can be built and run on its own (tools/dilconv_pack_check.cc, under the host sanitizers).
//
// Class: 3x3 window; ic and oc multiples of 32.  Output blocks (32 channels) are grouped into chunks of DL_PACK_CHUNK
// (the last chunk has the rest); a K-step is 32 input channels; a slab is `slab` consecutive K-steps (the last slab has
// the rest).  The kernel copies one (chunk, slab) to LDS at a time and reads it K-step by K-step, tap by tap, block by
// block, so that is the order of the image:
//   [chunk][slab][K-step of the slab][tap = 3 ky + kx][block of the chunk][lane][16]
// Byte e of lane = w[o = 32 (4 chunk + block) + (lane & 31)][i = 32 s + 16 (lane >> 5) + e][ky][kx]: the order of
// gconv_pack.h's fragments (the A operand of v_mfma_i32_32x32x32_i8).  A slab is a run of whole K-steps of ONE chunk and
// a chunk's K-steps follow each other, so every (chunk, slab) is one contiguous piece whatever `slab` is: the image does
// not depend on the slab size, only the pieces the kernel cuts it into do.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace dfx {

constexpr int DL_PACK_CHUNK = 4;  // output blocks per chunk (dilconv.cuh's DL_CHUNK)

inline size_t dilconv_pack_bytes(int oc, int ic) { return (size_t)(oc / 32) * (ic / 32) * 9 * 1024; }
// output blocks of chunk `chunk`
inline int dilconv_pack_nb(int oc, int chunk) {
  const int left = oc / 32 - chunk * DL_PACK_CHUNK;
  return left < DL_PACK_CHUNK ? left : DL_PACK_CHUNK;
}
// offset of the chunk's first byte: every chunk before it is full
inline size_t dilconv_pack_chunk(int ic, int chunk) { return (size_t)chunk * DL_PACK_CHUNK * (ic / 32) * 9 * 1024; }
// offset and size of the piece (chunk, slab) at `slab` K-steps per slab
inline size_t dilconv_pack_slab(int oc, int ic, int chunk, int slab_idx, int slab) {
  return dilconv_pack_chunk(ic, chunk) + (size_t)slab_idx * slab * 9 * dilconv_pack_nb(oc, chunk) * 1024;
}
inline size_t dilconv_pack_slab_bytes(int oc, int ic, int chunk, int slab_idx, int slab) {
  const int left = ic / 32 - slab_idx * slab;
  return (size_t)(left < slab ? left : slab) * 9 * dilconv_pack_nb(oc, chunk) * 1024;
}
// offset of the fragment (output block ob, K-step s, tap)
inline size_t dilconv_pack_frag(int oc, int ic, int ob, int s, int tap) {
  const int chunk = ob / DL_PACK_CHUNK, obl = ob % DL_PACK_CHUNK;
  return dilconv_pack_chunk(ic, chunk) + (((size_t)s * 9 + tap) * dilconv_pack_nb(oc, chunk) + obl) * 1024;
}

// wei: s8 {oc, ic, 3, 3} row-major; out: dilconv_pack_bytes(oc, ic) bytes, every one of them written
inline void dilconv_pack(const int8_t *wei, int oc, int ic, unsigned char *out) {
  for (int ob = 0; ob < oc / 32; ++ob)
    for (int s = 0; s < ic / 32; ++s)
      for (int tap = 0; tap < 9; ++tap) {
        unsigned char *frag = out + dilconv_pack_frag(oc, ic, ob, s, tap);
        for (int lane = 0; lane < 64; ++lane) {
          const int o = 32 * ob + (lane & 31);
          for (int e = 0; e < 16; ++e) {
            const int i = 32 * s + 16 * (lane >> 5) + e;
            frag[lane * 16 + e] = (unsigned char)wei[((size_t)o * ic + i) * 9 + tap];
          }
        }
      }
}

}  // namespace dfx
