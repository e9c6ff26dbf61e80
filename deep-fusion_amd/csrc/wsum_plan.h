// wsum_plan.h -- host-only, plain C++: what the scaled element-wise sum (dfx_wsum_* of include/dfx.h) decides before a
// kernel runs: the descriptor's validation, which kernel class a descriptor is in, where the per-channel constants and
// the table lie in the handle's device image (the vec kernel copies that image into LDS as it is), how dst may alias the
// inputs, and the grid.  No HIP in here, so that it can be built and run on its own (tools/wsum_plan_check.cc, under the
// host sanitizers).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/dfx.h"
#include "plan_common.h"

namespace dfx {

constexpr int WSUM_THREADS = 256;
constexpr int WSUM_MAX_BLOCKS = 256 * 8;            // grid-stride kernels: 8 workgroups per CU
constexpr long long WSUM_MAX_IMAGE = 1ll << 31;     // elements of one image, exclusive
constexpr long long WSUM_MAX_ELEMS = 1ll << 40;     // elements of a tensor, inclusive
constexpr long long WSUM_MAX_LDS = 64 * 1024;       // the staged constants of the vec kernel
constexpr long long WSUM_AUTO_MIN_ELEMS = 1ll << 19; // auto takes the vec kernel from this many elements on (128 workgroups)

inline bool wsum_src_dt_ok(int dt) { return dt == DFX_F32 || dt == DFX_S32 || dt == DFX_S8 || dt == DFX_U8; }

// DFX_OK, or the code dfx_wsum_create returns with *why set to the reason
inline int wsum_validate(const dfx_wsum_desc &d, const char **why) {
  const char *dummy;
  if (!why) why = &dummy;
  *why = "";
  if (d.bs < 1 || d.h < 1 || d.w < 1 || d.c < 1) return *why = "bs, h, w and c must be at least 1", DFX_ERR_INVALID;
  // h * w < 2^62 and c < 2^31: the quotients are exact and no product is formed before it is known to fit
  if ((long long)d.h * d.w > (WSUM_MAX_IMAGE - 1) / d.c) return *why = "one image of 2^31 elements or more", DFX_ERR_INVALID;
  if (d.bs > WSUM_MAX_ELEMS / ((long long)d.h * d.w * d.c)) return *why = "a tensor of more than 2^40 elements", DFX_ERR_INVALID;
  if (d.n_inputs < 1 || d.n_inputs > DFX_WSUM_MAX_INPUTS) return *why = "n_inputs must lie in 1 .. 8", DFX_ERR_INVALID;
  for (int i = 0; i < d.n_inputs; ++i) {
    if (!wsum_src_dt_ok(d.src_dt[i])) return *why = "bad src dtype", DFX_ERR_INVALID;
    if (d.nscales[i] != 1 && d.nscales[i] != d.c) return *why = "nscales must be 1 or c", DFX_ERR_INVALID;
  }
  if (d.n_bias != 0 && d.n_bias != 1 && d.n_bias != d.c) return *why = "n_bias must be 0, 1 or c", DFX_ERR_INVALID;
  if (d.round_mode != DFX_ROUND_NEAREST && d.round_mode != DFX_ROUND_DOWN) return *why = "bad round mode", DFX_ERR_INVALID;
  if (d.post_relu != 0 && d.post_relu != 1) return *why = "post_relu must be 0 or 1", DFX_ERR_INVALID;
  if (d.lut_in_dt != DFX_UNDEF && d.lut_in_dt != DFX_U8 && d.lut_in_dt != DFX_S8) return *why = "bad table index dtype", DFX_ERR_INVALID;
  if (d.force_path != -1 && d.force_path != DFX_WSUM_VEC && d.force_path != DFX_WSUM_GENERIC) return *why = "bad force_path", DFX_ERR_INVALID;
  if (d.dst_dt == DFX_S32) return *why = "s32 dst", DFX_ERR_UNSUPPORTED;
  if (d.dst_dt != DFX_F32 && d.dst_dt != DFX_S8 && d.dst_dt != DFX_U8) return *why = "bad dst dtype", DFX_ERR_INVALID;
  if (d.lut_in_dt != DFX_UNDEF && d.dst_dt == DFX_F32) return *why = "a table needs a u8 or s8 dst", DFX_ERR_INVALID;
  return DFX_OK;
}

// The handle's device image of the constants: one slot of c floats per per-channel input, in input order, then one for a
// per-channel bias, then the 256 table bytes.  slot[i] / bias_slot: the slot's number, -1 for a per-tensor value (which
// travels as a kernel argument) or none.  Every slot starts on a 16-byte boundary when c % 4 == 0.
struct WsumImage {
  int slot[DFX_WSUM_MAX_INPUTS];
  int bias_slot;
  int slots;
  long long lut_off;  // bytes; -1: no table
  long long bytes;    // of the whole image, rounded up to 16; 0: nothing to stage
};
inline WsumImage wsum_image(const dfx_wsum_desc &d) {
  WsumImage m;
  m.slots = 0;
  for (int i = 0; i < DFX_WSUM_MAX_INPUTS; ++i) m.slot[i] = (i < d.n_inputs && d.c > 1 && d.nscales[i] == d.c) ? m.slots++ : -1;
  m.bias_slot = (d.n_bias != 0 && d.c > 1 && d.n_bias == d.c) ? m.slots++ : -1;
  long long b = ((long long)m.slots * d.c * 4 + 15) / 16 * 16;
  m.lut_off = -1;
  if (d.lut_in_dt != DFX_UNDEF) {
    m.lut_off = b;
    b += 256;
  }
  m.bytes = b;
  return m;
}

// the vec kernel's class, as far as the descriptor decides it (pointer alignment is checked per submit)
inline bool wsum_vec_class(const dfx_wsum_desc &d) { return d.c % 16 == 0 && wsum_image(d).bytes <= WSUM_MAX_LDS; }

inline long long wsum_elems(const dfx_wsum_desc &d) { return (long long)d.bs * d.h * d.w * d.c; }
// the handle's path.  AUTO RULE (include/dfx.h DFX_WSUM_AUTO_NOTE, measured in profiles/wsum/): the vec kernel in its class
// where the tensor has at least 2^19 elements, i.e. where its launch has 128 workgroups or more; smaller tensors sit on
// the launch floor, where the generic kernel's one element per lane spreads over more CUs and is as fast or faster.
inline int wsum_path(const dfx_wsum_desc &d) {
  if (d.force_path != -1) return d.force_path;
  return wsum_vec_class(d) && wsum_elems(d) >= WSUM_AUTO_MIN_ELEMS ? DFX_WSUM_VEC : DFX_WSUM_GENERIC;
}
// work items of one launch: 16-channel groups (vec) or elements (generic)
inline long long wsum_items(const dfx_wsum_desc &d, int path) { return path == DFX_WSUM_VEC ? wsum_elems(d) / 16 : wsum_elems(d); }

// workgroups of 256 lanes for `items` work items; cap <= 0: none (DFX_WSUM_GRID)
inline int wsum_grid(long long items, long long cap) {
  long long blocks = (items + WSUM_THREADS - 1) / WSUM_THREADS;
  if (blocks > WSUM_MAX_BLOCKS) blocks = WSUM_MAX_BLOCKS;
  if (cap > 0 && blocks > cap) blocks = cap;
  return (int)(blocks < 1 ? 1 : blocks);
}

// How dst lies to the inputs of one submit.
enum {
  WSUM_ALIAS_NONE = 0,      // dst overlaps no input
  WSUM_ALIAS_IN_PLACE = 1,  // dst IS at least one input of its own element size, and overlaps no other kind of input
  WSUM_ALIAS_REFUSED = 2    // dst overlaps an input without being it, or is an input of another element size
};
inline int wsum_alias(int n, const uintptr_t *src, const int *src_dt, uintptr_t dst, int dst_dt, unsigned long long elems) {
  int kind = WSUM_ALIAS_NONE;
  const unsigned long long dbytes = elems * (unsigned)plan_dt_size(dst_dt);
  for (int i = 0; i < n; ++i) {
    const unsigned long long sbytes = elems * (unsigned)plan_dt_size(src_dt[i]);
    if (src[i] == dst && sbytes == dbytes) {
      kind = WSUM_ALIAS_IN_PLACE;
      continue;
    }
    if (src[i] < dst + dbytes && dst < src[i] + sbytes) return WSUM_ALIAS_REFUSED;
  }
  return kind;
}

}  // namespace dfx
