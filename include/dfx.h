/*
 * dfx.h -- C ABI of the MI355X (gfx950) implementation of deep-fusion's hot path:
 * the fused int8 conv3x3+relu+conv1x1(+relu) primitive and the concat(+relu)
 * primitive.  Plain pointers and sizes only; no C++/torch types cross this
 * boundary.  The library behind it is libdfx_hip.so (deep-fusion_amd/csrc/).
 *
 * This boundary sits where the reference has
 *     jit_conv_conf_t / jit_conv_call_t / void (*jit_ker_)(jit_conv_call_t*)
 *     (/root/reference/src/jit_call_conf.h:48-99, src/jit_conv_kernel.h:50-51)
 * and the same trio for concat (jit_call_conf.h:29-45, jit_concat_kernel.h:38-39):
 * a create-time POD descriptor, per-call buffer pointers, and one entry point
 * that runs the kernel.  Differences, by design:
 *   - one call per submit (the reference calls the JIT kernel once per output
 *     row, op_conv.cc:217-238); the call enqueues on a HIP stream;
 *   - weights / bias / scales are copied at dfx_conv_set_weights() and owned by
 *     the handle (fixes the dangling scales pointer, op_conv.h:94-95);
 *   - every entry point returns an int status (0 = ok) instead of exit()ing
 *     (log.h:38-42); dfx_last_error() returns the message.
 *
 * There is no CPU fallback: every compute entry point fails with
 * DFX_ERR_NO_DEVICE / DFX_ERR_HIP when no gfx950 device is usable.
 */
#ifndef DFX_H
#define DFX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DFX_VERSION 100

/* status codes */
enum {
  DFX_OK = 0,
  DFX_ERR_INVALID = 1,     /* descriptor violates the reference's shape/dtype rules */
  DFX_ERR_UNSUPPORTED = 2, /* valid for the reference, not implemented here */
  DFX_ERR_HIP = 3,         /* a HIP runtime call failed */
  DFX_ERR_NO_DEVICE = 4,   /* no usable gfx950 device */
  DFX_ERR_STATE = 5        /* e.g. submit before set_weights */
};

/* values of deepfusion::memory::dtype (reference include/deepfusion.h:66-72) */
enum { DFX_UNDEF = 0, DFX_F32 = 1, DFX_S32 = 2, DFX_S8 = 3, DFX_U8 = 4 };
/* deepfusion::round_mode (include/deepfusion.h:46-49) */
enum { DFX_ROUND_NEAREST = 0, DFX_ROUND_DOWN = 1 };

/* kernel variants (dfx_conv_info.variant) */
enum {
  DFX_VARIANT_GENERIC = 0,    /* any shape the reference's init_conf accepts */
  DFX_VARIANT_MFMA_FUSED = 1, /* int8-MFMA implicit GEMM, 3x3 s1 + fused 1x1 */
  DFX_VARIANT_MFMA_CONV = 2,  /* int8-MFMA implicit GEMM, unfused 3x3 s1 conv */
  DFX_VARIANT_MFMA_STREAM = 3 /* int8-MFMA, streamed weights: any kernel/stride/channel count */
};

/* Create-time descriptor.  Mirrors the shape/dtype/flag fields of
 * jit_conv_conf_t (jit_call_conf.h:66-99); the x86 blocking fields
 * (nb_*_blocking, ur_w, typesize_*, use_vnni) are dropped.
 * Tensors: src NHWC u8 {bs,ih,iw,ic}; wei OIhw4i16o4i s8 {oc,ic,kh,kw};
 * wei1x1 OIhw4i16o4i s8 {oc1x1,oc,1,1}; bias format x; dst NHWC. */
typedef struct dfx_conv_desc {
  int32_t bs;
  int32_t ic, ih, iw;
  int32_t oc, oh, ow;      /* conv0 output; oh/ow must equal (in+2p-k)/s+1 */
  int32_t kh, kw, sh, sw;
  int32_t pad_t, pad_l;
  int32_t oc1x1;           /* 0 = unfused conv (deepfusion.h:121-129) */
  int32_t dst_dt;          /* DFX_F32 | DFX_S32 | DFX_S8 | DFX_U8 */
  int32_t bia0_dt;         /* DFX_UNDEF = no bias */
  int32_t bia1_dt;
  int32_t conv0_relu, conv1_relu;
  int32_t conv0_round_mode, conv1_round_mode;
  int32_t conv0_nscales;   /* 1 or oc     (op_conv.cc:311-313) */
  int32_t conv1_nscales;   /* 1 or oc1x1  (op_conv.cc:342-345) */
  int32_t force_variant;   /* -1 = auto, else DFX_VARIANT_* (testing) */
  int32_t fuse_pool;       /* 0 = none; 2 = 2x2 stride-2 max pooling of the conv's output (after ReLU and
                              requantisation) fused into the conv kernel: dst then holds {bs, oh/2, ow/2, oc}.
                              Only for unfused 3x3 stride-1 convs on the resident-weight kernel with even oh, ow;
                              dfx_conv_create returns DFX_ERR_UNSUPPORTED otherwise (the caller then runs
                              dfx_pool_* behind an unpooled conv, as deepfusion::conv_relu_pool does). */
} dfx_conv_desc;

typedef struct dfx_conv_info {
  int32_t variant;
  int32_t grid, block, lds_bytes;
  int32_t rows_per_unit;       /* output rows one workgroup produces */
  int32_t device;              /* ordinal of the device the handle lives on */
  uint64_t algorithmic_ops;    /* 2*MAC of one submit */
  uint64_t algorithmic_bytes;  /* src + weights + dst bytes of one submit */
  char kernel_name[96];
} dfx_conv_info;

typedef struct dfx_concat_desc {
  int32_t n_inputs;
  int32_t bs, h, w;
  int32_t dt;               /* all inputs and dst share it (jit_concat_kernel.cc:184-187) */
  int32_t post_relu;
  const int32_t *channels;  /* n_inputs entries; %16 (1-byte) or %4 (4-byte) */
} dfx_concat_desc;

typedef struct dfx_conv dfx_conv_t;
typedef struct dfx_concat dfx_concat_t;

/* ---- the reference's roadmap ops (README.md:64-65: "conv+relu+pooling fused op",
 *      "eltwise-sum + relu fused op"; planned signature in test/test_conv_relu_pooling.cc:264-281).
 *      The reference ships no implementation: semantics follow the MKL-DNN pipeline its test
 *      builds (test_conv_relu_pooling.cc:30-235).  Parity unpinned. ---- */
typedef enum dfx_pool_algo {
  DFX_POOL_MAX = 0,
  DFX_POOL_AVG_INCLUDE_PADDING = 1,  /* sum over the window's positions inside the input / (kh * kw) */
  DFX_POOL_AVG_EXCLUDE_PADDING = 2   /* ... / number of those positions */
} dfx_pool_algo;
typedef struct dfx_pool_desc {
  int32_t bs, c, ih, iw;    /* NHWC input (the conv's output) */
  int32_t oh, ow;           /* given by the caller like the reference's dst_dims; windows may hang over the
                               bottom / right edge (the test's padR search, test_conv_relu_pooling.cc:178-182) */
  int32_t kh, kw, sh, sw, pad_t, pad_l;
  int32_t dt;               /* dfx_dtype of src and dst */
  int32_t algo;             /* DFX_POOL_MAX: maximum over the window's positions INSIDE the input
                               (padding does not take part, as in MKL-DNN's pooling_max).
                               DFX_POOL_AVG_*: integer types sum exactly, divide in f32 (float(sum) /
                               float(count)), round to nearest even and saturate to the dtype; f32 sums in
                               window order and divides (the reference test's pooling_avg_* flags,
                               test_conv_relu_pooling.cc:189-193; MKL-DNN's reference pooling arithmetic) */
} dfx_pool_desc;
typedef struct dfx_pool dfx_pool_t;

typedef struct dfx_eltwise_desc {
  int32_t n_inputs;         /* 2..8 tensors of identical shape and dtype */
  int64_t elems;            /* elements per tensor */
  int32_t dt;
  int32_t post_relu;        /* dst = relu?(saturate(sum_i src_i)): integer sums are exact and saturate to the
                               dtype's range, f32 sums left to right */
} dfx_eltwise_desc;
typedef struct dfx_eltwise dfx_eltwise_t;

/* ---- activation reorder: layout (NHWC <-> NCHW), dtype and scale conversion, channel pad / crop, on the
 *      device.  The reference ships no reorder (its tests and benches use MKL-DNN's reorder primitive):
 *      parity unpinned; the semantics are MKL-DNN's saturating reorder.  Over a logical {bs, c, h, w}
 *      tensor, for every destination channel k < dst_c:
 *        k >= src_c:  dst = 0 (+0.0f)                                      (channel padding)
 *        else         v = (float)src[n,k,y,x]     u8 / s8 exact, s32 round-to-nearest-even, f32 as is
 *                     v = v * scale[k]            ONE separately rounded f32 multiply; n_scales 0: 1.0f,
 *                                                 1: scale[0] for every channel, src_c: per channel
 *                     f32 dst: store v
 *                     u8 / s8 dst: rint(v) (ties to even; DFX_ROUND_NEAREST) or floor(v) (DFX_ROUND_DOWN),
 *                                  NaN -> 0, else clamped to [0,255] / [-128,127]
 *      Source channels >= dst_c are dropped.  This is NOT the conv epilogue's conversion (vcvtps2dq +
 *      vpmovusdb on the bit pattern): a reorder saturates the value, +inf becomes 255.  Denormal values
 *      are kept (the library is not built with flush-to-zero). ---- */
enum { DFX_FMT_NHWC = 0, DFX_FMT_NCHW = 1 };
typedef struct dfx_reorder_desc {
  int32_t bs, h, w, src_c, dst_c;
  int32_t src_fmt, dst_fmt;  /* DFX_FMT_*; all four combinations */
  int32_t src_dt, dst_dt;    /* src: DFX_F32 | DFX_S32 | DFX_S8 | DFX_U8; dst: DFX_F32 | DFX_U8 | DFX_S8
                                (DFX_S32: DFX_ERR_UNSUPPORTED) */
  int32_t round_mode;        /* DFX_ROUND_* */
  int32_t n_scales;          /* 0 | 1 | src_c */
} dfx_reorder_desc;
enum {  /* dfx_reorder_info.path */
  DFX_REORDER_FLAT = 0,      /* same layout, same channel count: 16 bytes of the wider side per lane */
  DFX_REORDER_GENERIC = 1,   /* same layout with channel pad / crop: one element per lane */
  DFX_REORDER_SMALLC = 2,    /* NCHW, src_c <= 4 -> NHWC, dst_c <= 16 (images): no LDS */
  DFX_REORDER_TRANSPOSE = 3  /* NCHW <-> NHWC through an LDS tile */
};
typedef struct dfx_reorder_info {
  int32_t path;
  int32_t grid, block, lds_bytes;
  int32_t device;
  int32_t tile_pixels, channel_block;  /* transpose path: pixels x channels of one workgroup's tile */
  int32_t vec_plane, vec_pixel;        /* transpose path: 1 = 16-byte accesses on the NCHW / NHWC side */
  uint64_t algorithmic_bytes;          /* bytes read of the channels kept + bytes written, one submit */
  char kernel_name[96];
} dfx_reorder_info;
typedef struct dfx_reorder dfx_reorder_t;

/* ---- channel concat + pointwise conv in one launch: the join of an Inception module, a DenseNet bottleneck, a
 *      SqueezeNet squeeze layer.  n_inputs NHWC u8 branches {bs,h,w,channels[i]} are read IN PLACE by a 1x1
 *      stride-1 unpadded conv over their concatenated channels; the concatenated tensor is never written.  The
 *      result is, bit for bit, dfx_concat_submit of the branches followed by dfx_conv_submit of the unfused
 *      pointwise conv with the same weights, bias, scales and flags (ReLU on a u8 source is the identity, so
 *      the reference's concat(..., post_relu) + conv() pair is covered as well).  Parity unpinned: the
 *      reference ships the two ops only. ---- */
typedef struct dfx_catconv_desc {
  int32_t n_inputs;            /* 2 .. 16 */
  int32_t bs, h, w;            /* shared by all branches and dst; 1x1 window, stride 1, no padding */
  int32_t oc;
  int32_t dst_dt;              /* DFX_F32 | DFX_S32 | DFX_S8 | DFX_U8 */
  int32_t bia_dt;              /* DFX_UNDEF = none */
  int32_t relu, round_mode;
  int32_t nscales;             /* 1 or oc */
  int32_t force_path;          /* -1 auto, else DFX_CATCONV_* (testing) */
  const int32_t *channels;     /* n_inputs entries, each % 16 == 0; ic = their sum */
} dfx_catconv_desc;
enum {  /* dfx_catconv_info.path */
  DFX_CATCONV_FUSED = 0,       /* one launch (catconv_pw.cuh).  Covers: every branch a multiple of 32 channels, ic a
                                  multiple of 256, oc in {64, 128, 256}, oc * ic <= 96 KB, bs*h*w * (widest branch)
                                  < 2^31 */
  DFX_CATCONV_TWO_LAUNCH = 1   /* everything else: concat into a buffer the handle owns, then the unfused conv, both
                                  on the caller's stream */
};
typedef struct dfx_catconv_info {
  int32_t path;
  int32_t grid, block, lds_bytes;  /* of the fused kernel / of the conv kernel of the two-launch path */
  int32_t device;
  uint64_t algorithmic_ops;    /* 2*MAC of one submit */
  uint64_t algorithmic_bytes;  /* branches + weights + dst; two-launch path: + 2 x the concatenated tensor */
  char kernel_name[96];        /* two-launch path: the conv kernel's */
} dfx_catconv_info;
typedef struct dfx_catconv dfx_catconv_t;

/* ---- depthwise int8 conv: every channel is convolved with its own kh x kw window (groups = channels, no channel
 *      multiplier, no dilation): the other half of a MobileNet / EfficientNet / Xception block.  src NHWC u8
 *      {bs,ih,iw,c}; weights s8 {c,kh,kw} plain row-major (goihw with o = i = 1); dst NHWC {bs,oh,ow,c}.
 *        acc[n,oy,ox,k] = sum over ky,kx of src[n, oy*sh - pad_t + ky, ox*sw - pad_l + kx, k] * w[k,ky,kx]
 *                         (taps outside the input are skipped)
 *        f = float(acc);  f = f + bias[k] (if any);  f = f * scale[k or 0];  ReLU (asked for, or dst is u8):
 *        f = (0 > f) ? 0 : f;  dst = store(f, dst_dt, round_mode)
 *      with the conv's arithmetic: separately rounded add and multiply, the bias converted like the conv's, the x86
 *      conversion (NaN / out of range -> 0x80000000 -> u8 255, s8 -128).  For c a multiple of 16 the result is, bit
 *      for bit, the unfused dfx_conv with ic = oc = c and W[o][i][ky][kx] = (o == i) ? w[o][ky][kx] : 0.  oh and ow
 *      are given by the caller as in dfx_pool_desc: windows may hang over the bottom / right edge (TF "SAME" padding
 *      of a stride-2 layer with pad_t = pad_l = 0).  Parity unpinned: the reference asserts ngroups == 1. ---- */
typedef struct dfx_dwconv_desc {
  int32_t bs, c, ih, iw;
  int32_t oh, ow;              /* (oh - 1) * sh - pad_t <= ih - 1, likewise in x */
  int32_t kh, kw;              /* 1 .. 255 */
  int32_t sh, sw;
  int32_t pad_t, pad_l;
  int32_t dst_dt;              /* DFX_F32 | DFX_S32 | DFX_S8 | DFX_U8 */
  int32_t bia_dt;              /* DFX_UNDEF = none */
  int32_t relu, round_mode;
  int32_t nscales;             /* 1 or c */
  int32_t force_path;          /* -1 auto, else DFX_DWCONV_* (testing) */
} dfx_dwconv_desc;
enum {  /* dfx_dwconv_info.path */
  DFX_DWCONV_WINDOW = 0,       /* the sliding-window kernel (dwconv.cuh).  Covers: 3x3 or 5x5, stride (1,1) or (2,2),
                                  c a multiple of 16, one image below 2^31 bytes on either side */
  DFX_DWCONV_GENERIC = 1       /* everything else: one thread per output element, any window / stride / channel count */
};
typedef struct dfx_dwconv_info {
  int32_t path;
  int32_t grid, block, lds_bytes;
  int32_t device;
  uint64_t algorithmic_ops;    /* 2*MAC of one submit */
  uint64_t algorithmic_bytes;  /* src + weights + dst */
  char kernel_name[96];        /* path, window, stride and requant route (valid after set_weights) */
} dfx_dwconv_info;
typedef struct dfx_dwconv dfx_dwconv_t;

/* ---- grouped int8 conv, 1 <= groups <= ic: output channel o reads only the ic / groups input channels of its group
 *      g(o) = o / (oc / groups) -- the 3x3 of a ResNeXt / RegNet block.  src NHWC u8 {bs,ih,iw,ic}; weights s8
 *      {oc, ic/groups, kh, kw} plain row-major (the layout frameworks keep them in); dst NHWC {bs,oh,ow,oc}.
 *        acc[n,oy,ox,o] = sum over i < ic/groups, ky, kx of
 *                         src[n, oy*sh - pad_t + ky, ox*sw - pad_l + kx, g(o) * (ic/groups) + i] * w[o,i,ky,kx]
 *                         (taps outside the input are skipped)
 *        f = float(acc);  f = f + bias[o] (if any);  f = f * scale[o or 0];  ReLU (asked for, or dst is u8):
 *        f = (0 > f) ? 0 : f;  dst = store(f, dst_dt, round_mode)
 *      with the depthwise op's arithmetic: separately rounded add and multiply, the bias converted like the conv's,
 *      the x86 conversion (NaN / out of range -> 0x80000000 -> u8 255, s8 -128).  Where ic and oc are multiples of 16
 *      and oh / ow follow the conv formula the result is, bit for bit, the unfused dfx_conv with
 *      W[o][j] = w[o][j - g(o) * ic/groups] inside o's group and 0 outside.  oh and ow are given by the caller as in
 *      dfx_dwconv_desc: windows may hang over the bottom / right edge.  Parity unpinned: the reference asserts
 *      ngroups == 1. ---- */
typedef struct dfx_gconv_desc {
  int32_t bs, ic, ih, iw;
  int32_t oc, oh, ow;          /* (oh - 1) * sh - pad_t <= ih - 1, likewise in x */
  int32_t groups;              /* divides ic and oc; kh * kw * ic / groups <= 65025 */
  int32_t kh, kw;
  int32_t sh, sw;
  int32_t pad_t, pad_l;
  int32_t dst_dt;              /* DFX_F32 | DFX_S32 | DFX_S8 | DFX_U8 */
  int32_t bia_dt;              /* DFX_UNDEF = none */
  int32_t relu, round_mode;
  int32_t nscales;             /* 1 or oc */
  int32_t force_path;          /* -1 auto, else DFX_GCONV_* (testing) */
} dfx_gconv_desc;
enum {  /* dfx_gconv_info.path */
  DFX_GCONV_MFMA = 0,          /* the int8-MFMA kernel (gconv.cuh).  Covers: 3x3 window; stride (1,1) or (2,2);
                                  ic == oc, a multiple of 32; ic / groups in {4, 8, 16, 32, 64}; one image below 2^31
                                  bytes on either side.  Auto takes it everywhere in this class. */
  DFX_GCONV_GENERIC = 1        /* everything else: one thread per output element, any window / stride / channel
                                  counts / groups (groups = 1 and groups = ic included), exact requant only */
};
typedef struct dfx_gconv_info {
  int32_t path;
  int32_t grid, block, lds_bytes;
  int32_t device;
  uint64_t algorithmic_ops;    /* 2*MAC of one submit: 2 * kh * kw * ic/groups per output value */
  uint64_t algorithmic_bytes;  /* src + weights + dst */
  char kernel_name[96];        /* path, window, stride, cpg, dst type and requant route (valid after set_weights) */
} dfx_gconv_info;
typedef struct dfx_gconv dfx_gconv_t;

/* ---- first-layer conv over a 1- to 4-channel image: the conv1 of ResNet / VGG / MobileNet / Inception, which dfx_conv's
 *      ic % 16 == 0 rule cannot take without padding the image to 16 channels first.  src NHWC u8 {bs,ih,iw,ic} with
 *      1 <= ic <= 4, at ANY byte address (the rows of a 3-channel image start at any byte offset anyway); wei s8
 *      {oc,ic,kh,kw} plain row-major (OIhw4i16o4i cannot express ic < 16); dst NHWC {bs,oh,ow,oc}, any oc >= 1.
 *        acc[n,oy,ox,o] = sum over i < ic, ky, kx of src[n, oy*sh - pad_t + ky, ox*sw - pad_l + kx, i] * w[o,i,ky,kx]
 *                         (taps outside the input are skipped, which equals zero padding)
 *        f = float(acc);  f = f + bias[o] (if any);  f = f * scale[o or 0];  ReLU (asked for, or dst is u8):
 *        f = (0 > f) ? 0 : f;  dst = store(f, dst_dt, round_mode)
 *      with the grouped op's arithmetic, word for word: exact s32 accumulator, separately rounded add and multiply,
 *      the bias converted like the conv's, the x86 conversion (NaN / out of range -> 0x80000000 -> u8 255, s8 -128).
 *      Defining properties (tests/test_gpu_imgconv.py):
 *        1. the result equals, bit for bit, dfx_gconv with groups = 1 on the same tensors;
 *        2. where oc % 16 == 0 and oh / ow follow the conv formula it equals, bit for bit, the unfused dfx_conv on the
 *           image zero-padded to 16 channels, with zero weights on the channels >= ic.
 *      oh and ow are given by the caller as in dfx_gconv_desc: windows may hang over the bottom / right edge.  Windows
 *      are 1 .. 255 on either axis.  Parity unpinned: the reference has no such op. ---- */
typedef struct dfx_imgconv_desc {
  int32_t bs, ic, ih, iw;      /* 1 <= ic <= 4 */
  int32_t oc, oh, ow;          /* (oh - 1) * sh - pad_t <= ih - 1, likewise in x */
  int32_t kh, kw;              /* 1 .. 255; kh * kw * ic <= 65025 */
  int32_t sh, sw;
  int32_t pad_t, pad_l;
  int32_t dst_dt;              /* DFX_F32 | DFX_S32 | DFX_S8 | DFX_U8 */
  int32_t bia_dt;              /* DFX_UNDEF = none */
  int32_t relu, round_mode;
  int32_t nscales;             /* 1 or oc */
  int32_t force_path;          /* -1 auto, else DFX_IMGCONV_* (testing) */
} dfx_imgconv_desc;
enum {  /* dfx_imgconv_info.path */
  DFX_IMGCONV_MFMA = 0,        /* the int8-MFMA kernel (imgconv.cuh), one launch.  Covers: ic 3 or 4; (window, stride)
                                  7x7 / (2,2), 3x3 / (1,1) or 3x3 / (2,2); pad_t, pad_l <= k - 1; oc a multiple of 32,
                                  at most 128; one image below 2^31 bytes on either side.
                                  AUTO RULE: auto takes it everywhere in this class (measured against the generic
                                  kernel on every point of profiles/imgconv/). */
  DFX_IMGCONV_GENERIC = 1      /* everything else (ic 1 or 2, 5x5, 11x11 / 4, any oc): one thread per output element,
                                  exact requant only */
};
typedef struct dfx_imgconv_info {
  int32_t path;
  int32_t grid, block, lds_bytes;
  int32_t device;
  uint64_t algorithmic_ops;    /* 2*MAC of one submit: 2 * kh * kw * ic per output value */
  uint64_t algorithmic_bytes;  /* src + weights + dst, src at its true ic bytes per pixel */
  char kernel_name[96];        /* path, window, stride, ic, oc, dst type and requant route (valid after set_weights) */
} dfx_imgconv_info;
typedef struct dfx_imgconv dfx_imgconv_t;

/* ---- transposed conv ("deconvolution") on int8: the layer that makes feature maps larger (U-Net / FPN up-convs, pose
 *      and CenterNet heads, DCGAN generators, the Mask R-CNN mask head).  src NHWC u8 {bs,ih,iw,ic}; wei s8
 *      {oc,ic,kh,kw} plain row-major, the order of every other op here (PyTorch's ConvTranspose2d.weight is
 *      {ic,oc,kh,kw}: swap the first two axes); dst NHWC {bs,oh,ow,oc}.
 *        acc[n,oy,ox,o] = sum over i < ic, ky < kh, kx < kw
 *                         with (oy + pad_t - ky) % sh == 0, iy = (oy + pad_t - ky) / sh in [0, ih)
 *                         and  (ox + pad_l - kx) % sw == 0, ix = (ox + pad_l - kx) / sw in [0, iw)
 *                         of   src[n,iy,ix,i] * w[o,i,ky,kx]
 *        f = float(acc);  f = f + bias[o] (if any);  f = f * scale[o or 0];  ReLU (asked for, or dst is u8):
 *        f = (0 > f) ? 0 : f;  dst = store(f, dst_dt, round_mode)
 *      with the grouped op's arithmetic, word for word: exact s32 accumulator, separately rounded add and multiply,
 *      the bias converted like the conv's, the x86 conversion (NaN / out of range -> 0x80000000 -> u8 255, s8 -128).
 *      An output element that no tap reaches is requant(0).
 *      Defining properties (tests/test_gpu_deconv.py):
 *        1. the result equals, bit for bit, dfx_gconv with groups = 1, stride 1, padding (kh-1-pad_t, kw-1-pad_l), the
 *           same oh / ow, on the zero-stuffed tensor {bs, (ih-1)*sh+1, (iw-1)*sw+1, ic} (src at the multiples of the
 *           stride, 0 elsewhere) with the spatially flipped weights w[o,i,kh-1-ky,kw-1-kx];
 *        2. where ic and oc are multiples of 16, kh-1-pad_t == kw-1-pad_l and oh / ow are the conv formula's, it equals
 *           the unfused dfx_conv on the same stuffed tensor and flipped weights.
 *      oh and ow are given by the caller as in dfx_gconv_desc (this covers output_padding and cropping):
 *      1 <= oh <= (ih-1)*sh + kh - pad_t, likewise in x.  Parity unpinned: the reference has no such op. ---- */
typedef struct dfx_deconv_desc {
  int32_t bs, ic, ih, iw;
  int32_t oc, oh, ow;          /* 1 <= oh <= (ih - 1) * sh + kh - pad_t, likewise in x */
  int32_t kh, kw;              /* 1 .. 255; kh * kw * ic <= 65025 */
  int32_t sh, sw;              /* 1 .. 255 */
  int32_t pad_t, pad_l;        /* 0 .. kh - 1, 0 .. kw - 1 */
  int32_t dst_dt;              /* DFX_F32 | DFX_S32 | DFX_S8 | DFX_U8 */
  int32_t bia_dt;              /* DFX_UNDEF = none */
  int32_t relu, round_mode;
  int32_t nscales;             /* 1 or oc */
  int32_t force_path;          /* -1 auto, else DFX_DECONV_* */
} dfx_deconv_desc;
enum {  /* dfx_deconv_info.path */
  DFX_DECONV_MFMA = 0,         /* the sub-pixel int8-MFMA kernel (deconv.cuh), one launch: every output parity
                                  ((oy + pad_t) % 2, (ox + pad_l) % 2) is a dense conv of the un-stuffed input with its
                                  own sub-kernel.  Covers: stride (2,2); window 2x2 with pad 0, 4x4 with pad <= 3, or 3x3
                                  with pad <= 2 (packed as a 4x4 window whose last row and column are zero: 16/9 of the
                                  MACs); ic and oc multiples of 32; one output block's fragments in LDS:
                                  128 * (kh > 2 ? 4 : 1) * ic + 21504 <= 163840 bytes (ic <= 1088 for 2x2, ic <= 256
                                  for 3x3 / 4x4); one image below 2^31 bytes on either side.
                                  AUTO RULE: auto takes it everywhere in this class: on the eight layers of
                                  profiles/deconv/ inside the class it is 260 to 1350 times faster than the generic kernel
                                  and 1.2 to 1.9 times faster than dfx_conv on a tensor stuffed in advance (DESIGN.md
                                  section 4.12).  A 4x4 / 3x3 window with ic > 256 (DCGAN's 512 -> 256) is outside the
                                  class and runs on the generic kernel, far slower than dfx_conv on a stuffed tensor. */
  DFX_DECONV_GENERIC = 1       /* everything else: one thread per output element, the gather formula above, any window
                                  / stride / padding / ic / oc, exact requant only */
};
typedef struct dfx_deconv_info {
  int32_t path;
  int32_t grid, block, lds_bytes;
  int32_t device;
  uint64_t algorithmic_ops;    /* 2*MAC of one submit over the taps that exist (not those of the stuffed conv) */
  uint64_t algorithmic_bytes;  /* src + weights + dst, src un-stuffed */
  char kernel_name[96];        /* path, window, stride, ic, oc, dst type and requant route (valid after set_weights) */
} dfx_deconv_info;
typedef struct dfx_deconv dfx_deconv_t;

/* ---- dilated ("atrous") conv on int8: the 3x3 of a DeepLab ASPP branch, of a dilated ResNet's res4 / res5, of the
 *      context modules of PSPNet / RFBNet / SSD's fc6.  src NHWC u8 {bs,ih,iw,ic}; wei s8 {oc,ic,kh,kw} plain
 *      row-major; dst NHWC {bs,oh,ow,oc}; any ic, oc >= 1.
 *        acc[n,oy,ox,o] = sum over i < ic, ky < kh, kx < kw of
 *                         src[n, oy*sh - pad_t + ky*dh, ox*sw - pad_l + kx*dw, i] * w[o,i,ky,kx]
 *                         (taps outside the input are skipped)
 *        f = float(acc);  f = f + bias[o] (if any);  f = f * scale[o or 0];  ReLU (asked for, or dst is u8):
 *        f = (0 > f) ? 0 : f;  dst = store(f, dst_dt, round_mode)
 *      with the grouped op's arithmetic, word for word: exact s32 accumulator, separately rounded add and multiply,
 *      the bias converted like the conv's, the x86 conversion (NaN / out of range -> 0x80000000 -> u8 255, s8 -128).
 *      Defining properties (tests/test_gpu_dilconv.py), with the zero-stuffed weights wz[o,i,ky*dh,kx*dw] = w[o,i,ky,kx],
 *      0 elsewhere, a ((kh-1)*dh+1) x ((kw-1)*dw+1) window:
 *        1. the result equals, bit for bit, dfx_gconv with groups = 1 on wz, same stride, padding and oh / ow, wherever
 *           that descriptor is valid (its window * ic <= 65025);
 *        2. where additionally ic and oc are multiples of 16 and oh / ow follow the conv formula it equals the unfused
 *           dfx_conv on wz;
 *        3. with dh = dw = 1 it equals dfx_gconv (groups = 1) on the same tensors.
 *      oh and ow are given by the caller as in dfx_gconv_desc, with the dilated extent.  Parity unpinned: the
 *      reference has no such op. ---- */
typedef struct dfx_dilconv_desc {
  int32_t bs, ic, ih, iw;
  int32_t oc, oh, ow;          /* (oh - 1) * sh - pad_t <= ih - 1, likewise in x */
  int32_t kh, kw;              /* 1 .. 255; kh * kw * ic <= 65025 (the taps that exist, not the stuffed window) */
  int32_t sh, sw;              /* 1 .. 255 */
  int32_t dh, dw;              /* 1 .. 255; 1 = no dilation */
  int32_t pad_t, pad_l;        /* 0 .. (kh - 1) * dh, 0 .. (kw - 1) * dw */
  int32_t dst_dt;              /* DFX_F32 | DFX_S32 | DFX_S8 | DFX_U8 */
  int32_t bia_dt;              /* DFX_UNDEF = none */
  int32_t relu, round_mode;
  int32_t nscales;             /* 1 or oc */
  int32_t force_path;          /* -1 auto, else DFX_DILCONV_* */
} dfx_dilconv_desc;
enum {  /* dfx_dilconv_info.path */
  DFX_DILCONV_MFMA = 0,        /* the int8-MFMA kernel (dilconv.cuh), one launch: dilation is an address offset of the
                                  activation loads, the weights stream through LDS in K-slabs.  Covers: 3x3 window;
                                  stride (1,1); any dh, dw; any padding the descriptor admits; ic and oc multiples of 32
                                  with NO further cap on ic (9 * ic <= 65025 is the descriptor's own); one image below
                                  2^31 bytes on either side.
                                  AUTO RULE: auto takes it everywhere in this class: on the 16 points of
                                  profiles/dilconv/ (ASPP on ResNet-50 and MobileNetV2 at d 6 / 12 / 18, dilated ResNet res4
                                  / res5, N = 1 and 16) it is 23 to 1094 times faster than the generic kernel.  Against
                                  dfx_conv on zero-stuffed weights, where that can be expressed at all (6 of the 16), it
                                  is 1.3 to 12 times faster on five and 16 % slower on one (res4, d 2, N = 1).  640 to
                                  1036 TOP/s at N = 16, 4.9 to 7.9 times the matrix floor. */
  DFX_DILCONV_GENERIC = 1      /* everything else: one thread per output element, the formula above, any window / stride
                                  / dilation / padding / ic / oc, exact requant only */
};
typedef struct dfx_dilconv_info {
  int32_t path;
  int32_t grid, block, lds_bytes;
  int32_t device;
  uint64_t algorithmic_ops;    /* 2*MAC of one submit: 2 * kh * kw * ic per output value (not the stuffed window's) */
  uint64_t algorithmic_bytes;  /* src + weights + dst, weights un-stuffed */
  char kernel_name[96];        /* path, window, dilation, ic, oc, dst type and requant route (valid after set_weights) */
} dfx_dilconv_info;
typedef struct dfx_dilconv dfx_dilconv_t;

/* ---- activation resize: nearest / bilinear interpolation of an NHWC feature map, optionally with a lateral tensor added
 *      in the same launch: FPN's "nearest x2, add the lateral", DeepLab's / PSPNet's bilinear upsampling, bilinear U-Net
 *      decoders.  src NHWC {bs,ih,iw,c}; dst NHWC {bs,oh,ow,c} of the same dtype; oh and ow are given by the caller.  All
 *      four sizes lie in 1 .. 65535, so that every remainder and denominator below is < 2^24 and float(.) of it exact.
 *      c >= 1.  dtype: u8 / s8 / f32; nearest also takes s32 (it is a copy).
 *      PER-AXIS PLAN, the same for y and x (in, out: the axis's sizes; o: output index).  Exact integer arithmetic, done
 *      once on the host at create time (csrc/resize_plan.h) and uploaded as tables; the kernels only read tables.
 *                                                                              num(o)            den
 *        DFX_COORD_HALF_PIXEL     (PyTorch align_corners=False, nearest-exact) (2o+1)*in - out   2*out
 *        DFX_COORD_ALIGN_CORNERS                                               o*(in-1)          out-1  (out == 1: 0, 1)
 *        DFX_COORD_ASYMMETRIC     (PyTorch legacy 'nearest', Caffe / TF1)      o*in              out
 *        bilinear: num = max(num, 0); i0 = min(num / den, in-1); i1 = min(i0+1, in-1);
 *                  w1 = float(num % den) / float(den) (ONE IEEE f32 division); w0 = 1.0f - w1
 *        nearest:  i0 = i1 = min(idx, in-1), w0 = 1, w1 = 0, with idx = ((2o+1)*in) / (2*out) (HALF_PIXEL),
 *                  (o*in) / out (ASYMMETRIC), (2*num + den) / (2*den) (ALIGN_CORNERS: round half up)
 *      VALUE.  Bilinear, with v = float(src) (exact for u8 / s8), every multiply and add rounded separately (never an FMA):
 *        top = v[y0,x0]*wx0 + v[y0,x1]*wx1;  bot = v[y1,x0]*wx0 + v[y1,x1]*wx1;  out = top*wy0 + bot*wy1
 *      f32 dst stores out; u8 / s8 dst stores rint(out) (ties to even) clamped to the dtype's range (the reorder's
 *      conversion).  f32 specials follow the formula: Inf * 0 is NaN, denormals are kept, and -0*1 + x*0 is +0, so an
 *      identity-size bilinear resize of f32 is NOT a bit copy.  Nearest copies src[y0,x0] bit for bit, NaN payloads
 *      included.
 *      FUSED ADD (add != 0): dst = eltwise_sum(resized, add_tensor) with dfx_eltwise's arithmetic, word for word: the
 *      resized value is first converted to the dtype as above, then an exact integer sum saturated to the dtype, or the
 *      f32 sum resized + add in that operand order, then ReLU if post_relu.  add_tensor has dst's shape and dtype and may
 *      BE dst (in place); an add range that overlaps dst's in any other way is refused.  dst must not overlap src.
 *      Defining properties (tests/test_gpu_resize.py): nearest at an integer factor s equals dfx_deconv with identity
 *      weights (stride s, window s x s); bilinear HALF_PIXEL at oh = ih/2, ow = iw/2 equals dfx_pool's 2x2 / 2 average;
 *      resize + add equals dfx_resize followed by dfx_eltwise.  Parity unpinned: the reference has no such op. ---- */
enum { DFX_RESIZE_NEAREST = 0, DFX_RESIZE_BILINEAR = 1 };                             /* dfx_resize_desc.algo */
enum { DFX_COORD_HALF_PIXEL = 0, DFX_COORD_ALIGN_CORNERS = 1, DFX_COORD_ASYMMETRIC = 2 }; /* dfx_resize_desc.coord */
typedef struct dfx_resize_desc {
  int32_t bs, c, ih, iw;
  int32_t oh, ow;              /* 1 .. 65535, like ih and iw */
  int32_t dt;                  /* DFX_F32 | DFX_S8 | DFX_U8; DFX_S32 with DFX_RESIZE_NEAREST only */
  int32_t algo;                /* DFX_RESIZE_* */
  int32_t coord;               /* DFX_COORD_* */
  int32_t add;                 /* 1: submit takes the tensor to add */
  int32_t post_relu;           /* with add only (DFX_ERR_INVALID otherwise) */
  int32_t force_path;          /* -1 auto, else DFX_RESIZE_BAND | DFX_RESIZE_GENERIC */
} dfx_resize_desc;
enum {  /* dfx_resize_info.path */
  DFX_RESIZE_BAND = 0,         /* resize_band_kernel (resize.cuh): a lane owns 16 bytes of channels of one output column
                                  and a band of consecutive output rows; it keeps the two horizontal interpolations of the
                                  rows y0 and y1 in f32 registers and rebuilds only what the next output row changes.
                                  Class: c * sizeof(element) a multiple of 16; src, dst and add 16-byte aligned (checked
                                  per submit: other pointers take the generic kernel for that submit); one image below
                                  2^31 bytes on either side.  Bit-identical to the generic kernel.
                                  AUTO RULE: see DFX_RESIZE_AUTO_NOTE below. */
  DFX_RESIZE_GENERIC = 1       /* everything else: one thread per output element, grid-stride */
};
/* DFX_RESIZE_AUTO_NOTE: auto takes DFX_RESIZE_BAND everywhere in its class.  On the 16 in-class points of
 * profiles/resize/bench_resize.txt (FPN nearest x2 + add at 16 / 32 / 64 -> x2 on 256 channels, DeepLab 33 -> 129 and its
 * logits at c = 32, PSPNet 6 -> 60, U-Net x2 on u8 and f32; N = 1 and 16; buffers in rotation beyond the Infinity Cache) it
 * is 1.2 to 9.5 times faster than the generic kernel on every one; with warm caches the smallest point (FPN 16 -> 32,
 * N = 1) sits on the launch floor (3 us) and the band kernel is 1 to 4 % slower there.  1.5 to 5.0 TB/s of algorithmic bytes at N = 16. */
typedef struct dfx_resize_info {
  int32_t path;                /* the handle's plan (a misaligned submit falls back without changing it) */
  int32_t grid, block, lds_bytes;
  int32_t device;
  int32_t rows_per_lane;       /* band length of the band kernel (1 on the generic path) */
  uint64_t algorithmic_bytes;  /* src + dst + add tensor, one submit */
  char kernel_name[96];
} dfx_resize_info;
typedef struct dfx_resize dfx_resize_t;

/* ---- fully-connected (inner product) layer on int8: the classifier head the conv ops cannot express.  src NHWC u8
 *      {bs,ih,iw,ic} exactly as the previous conv or pool op wrote it (ih = iw = 1: a plain vector); wei s8
 *      {oc,ic,ih,iw} plain row-major, the flattened-CHW classifier frameworks keep (the library permutes it to src's
 *      order when it packs); dst {bs,oc}, rows oc elements apart.  Any bs >= 1 and oc >= 1.
 *        acc[n,o] = sum over c, y, x of src[n,y,x,c] * w[o,c,y,x]
 *        f = float(acc);  f = f + bias[o] (if any);  f = f * scale[o or 0];  ReLU (asked for, or dst is u8):
 *        f = (0 > f) ? 0 : f;  dst = store(f, dst_dt, round_mode)
 *      with the grouped op's arithmetic: separately rounded add and multiply, the bias converted like the conv's,
 *      the x86 conversion (NaN / out of range -> 0x80000000 -> u8 255, s8 -128).  Where ic and oc are multiples of 16
 *      the result is, bit for bit, the unfused dfx_conv with kh = ih, kw = iw, stride 1, no padding (oh = ow = 1).
 *      Parity unpinned: the reference has no inner product. ---- */
typedef struct dfx_fc_desc {
  int32_t bs, ic, ih, iw;      /* K = ih * iw * ic <= 65025: below it the accumulator cannot leave s32 */
  int32_t oc;
  int32_t dst_dt;              /* DFX_F32 | DFX_S32 | DFX_S8 | DFX_U8 */
  int32_t bia_dt;              /* DFX_UNDEF = none */
  int32_t relu, round_mode;
  int32_t nscales;             /* 1 or oc */
  int32_t force_path;          /* -1 auto, else DFX_FC_* (testing) */
} dfx_fc_desc;
enum {  /* dfx_fc_info.path */
  DFX_FC_MFMA = 0,             /* the split-K int8-MFMA kernel and its epilogue (fc.cuh): two launches.  Covers
                                  K % 64 == 0 with any bs and oc.  Auto takes it everywhere in this class. */
  DFX_FC_GENERIC = 1           /* everything else (a 3-channel input, K = 100): one thread per output value, one
                                  launch, exact requant only */
};
typedef struct dfx_fc_info {
  int32_t path;
  int32_t splitk;              /* K slices of the MFMA path (1 on the generic path) */
  int32_t grid, block, lds_bytes;  /* of the MFMA kernel (the generic kernel on that path) */
  int32_t device;
  uint64_t algorithmic_ops;    /* 2*MAC of one submit: 2 * bs * K * oc */
  uint64_t algorithmic_bytes;  /* src + weights + dst (the slab of partial sums is not algorithmic) */
  char kernel_name[96];        /* path, K, dst type, splitk and requant route (valid after set_weights) */
} dfx_fc_info;
typedef struct dfx_fc dfx_fc_t;

/* ---- squeeze-and-excitation gate: the piece between the depthwise (or grouped) conv and the projecting 1x1 conv of every
 *      EfficientNet block, most MobileNetV3 blocks and every SENet / SE-ResNeXt / RegNetY block: global average, two tiny
 *      fully-connected layers, a gate function, a per-(image, channel) rescale of the activation.
 *        src   NHWC u8 {bs,ih,iw,c};  dst NHWC u8 of the same shape, it may BE src (in place), any other overlap is refused
 *        w1    s8 {cr,c} row-major;   w2 s8 {c,cr} row-major;  biases bia1_dt / bia2_dt as in dfx_fc_desc (DFX_UNDEF = none)
 *        scales1: 1 or cr floats;  scales2: 1 or c floats;  out_scales: 1 or c floats
 *        lut   256 u8 entries given by the caller: lut[i] is the gate for t = i - 128
 *      ARITHMETIC (one round_mode rm for all stages; requant, cvt_x86_rt, sat_u8_bits and sat_s8 are csrc/dfx_device.cuh's:
 *      separately rounded f32 add and multiply, never an FMA; the biases are converted on the host as dfx_fc's are):
 *        sum[n,c] = sum over y, x of src[n,y,x,c]                        exact s32 (ih*iw <= 2^23, so 255*ih*iw < 2^31)
 *        z[n,c]   = rint(float(sum) / float(ih*iw)) clamped to 0 .. 255   dfx_pool's average (avg_finish<u8>)
 *        a1[n,j]  = sum over c of z[n,c] * w1[j,c]                        exact s32
 *        h[n,j]   = sat_u8_bits(cvt_x86_rt(requant(a1, b1[j], s1[j], relu = true), rm))       dfx_fc with dst u8
 *        a2[n,c]  = sum over j of h[n,j] * w2[c,j]
 *        t[n,c]   = sat_s8(cvt_x86_rt(requant(a2, b2[c], s2[c], relu = false), rm))            dfx_fc with dst s8
 *        g[n,c]   = lut[t[n,c] + 128]
 *        dst[n,y,x,c] = sat_u8_bits(cvt_x86_rt(requant(src[n,y,x,c] * g[n,c], +0.0f, out_scale[c], true), rm))
 *      The table turns the requantised logit into the gate: the caller builds it for sigmoid, hard-sigmoid (MobileNetV3) or
 *      anything else; with out_scale = 1/255 and lut = rint(255 * sigmoid(t * s)) the op is the float SE gate to within
 *      quantisation.  No transcendental is evaluated on the device: every stage is exact integer or single-rounded f32.
 *      Defining properties (tests/test_gpu_se.py): DFX_SE_SQUEEZE equals dfx_pool (DFX_POOL_AVG_EXCLUDE_PADDING, window =
 *      image, no padding) bit for bit; DFX_SE_GATE equals that pool -> dfx_fc (relu, u8) -> dfx_fc (s8) -> table lookup;
 *      DFX_SE_SCALE equals the formula above.  Parity unpinned: the reference has no such op. ---- */
enum {  /* dfx_se_desc.mode */
  DFX_SE_SCALE = 0,            /* the whole op: dst as above */
  DFX_SE_GATE = 1,             /* dst is g, u8 {bs,c}, rows c bytes apart: the caller applies the gate elsewhere */
  DFX_SE_SQUEEZE = 2           /* dst is z, u8 {bs,c}: global average pooling at any image size; needs no weights */
};
typedef struct dfx_se_desc {
  int32_t bs, c, ih, iw;       /* ih * iw <= 2^23, c <= 16384 */
  int32_t cr;                  /* the squeezed width, 1 .. 16384 (ignored by the kernels in DFX_SE_SQUEEZE) */
  int32_t mode;                /* DFX_SE_* */
  int32_t bia1_dt, bia2_dt;    /* DFX_UNDEF = none */
  int32_t round_mode;          /* of every stage */
  int32_t nscales1;            /* 1 or cr */
  int32_t nscales2;            /* 1 or c */
  int32_t nscales_out;         /* 1 or c */
  int32_t force_path;          /* -1 auto, else DFX_SE_BAND | DFX_SE_GENERIC */
} dfx_se_desc;
enum {  /* dfx_se_info.path */
  DFX_SE_BAND = 0,             /* se_squeeze_kernel + se_excite_kernel + se_scale_kernel (se.cuh): a lane owns 16 bytes of
                                  channels.  The squeeze sums bytes as packed 16-bit halves, flushed to s32 every 257 pixels
                                  at the latest, one workgroup per (image, slice of pixels), partial sums into the handle's
                                  slab [bs][slices][c]; the scale kernel keeps a lane's 16 gate bytes and scales in
                                  registers and walks down pixels.  Class: c % 16 == 0, src and dst 16-byte aligned (checked
                                  per submit: other pointers take the generic kernels for that submit), one image below
                                  2^31 bytes.  Bit-identical to the generic kernels.  AUTO RULE: DFX_SE_AUTO_NOTE below. */
  DFX_SE_GENERIC = 1           /* everything else (c = 72, 120): se_squeeze_generic, one thread per (image, channel), and
                                  se_scale_generic, one thread per byte, grid-stride; se_excite_kernel serves both paths */
};
/* DFX_SE_AUTO_NOTE: auto takes DFX_SE_BAND everywhere in its class.  On the 18 points of profiles/se/bench_se.txt (the SE
 * blocks of EfficientNet-B0 and SE-ResNeXt-50 at N = 1 and 32, buffers in rotation beyond the Infinity Cache) the generic
 * kernels are 1.4 to 1.8 times slower on the 7x7 maps, 5 times on 14x14 and 16 to 125 times from 28x28 up; no point has
 * them faster.  14 to 35 us per op, about 13 us of it the three dependent launch boundaries. */
typedef struct dfx_se_info {
  int32_t path;                /* the handle's plan (a misaligned submit falls back without changing it) */
  int32_t slices;              /* pixel slices per image of the squeeze kernel (1 on the generic path) */
  int32_t grid, block, lds_bytes;  /* of the squeeze kernel */
  int32_t device;
  uint64_t algorithmic_bytes;  /* DFX_SE_SCALE: src twice + dst; the other modes: src + the {bs,c} result */
  char kernel_name[96];
} dfx_se_info;
typedef struct dfx_se dfx_se_t;

/* ---- scaled element-wise sum: the join of two or more branches that do NOT share one quantisation step -- the ResNet
 *      shortcut (u8 block output + u8 identity), the MobileNetV2 / EfficientNet linear bottleneck (s8 + s8), a quantised FPN
 *      level add with per-channel scales, a conv's s32 / f32 result added to a u8 tensor -- and, with a byte table, any
 *      activation of a 1-byte tensor (swish / h-swish: n_inputs = 1).  dfx_eltwise has no scale anywhere; reorder per branch +
 *      dfx_eltwise costs two or three extra round trips of the largest tensors and rounds twice.
 *        src_i  NHWC {bs,h,w,c} of src_dt[i], i < n_inputs <= 8, dtypes independent of each other;  dst NHWC {bs,h,w,c}
 *        s_i    nscales[i] = 1 (per tensor) or c (per channel) floats;  bias: n_bias = 0, 1 or c floats (zero points and
 *               folded constants);  lut: 256 bytes
 *      ARITHMETIC, for element (n,y,x,k).  Every f32 operation is rounded separately and there is never an FMA:
 *        v      = float(src_0) * s_0[k]            u8 / s8 exact, s32 round-to-nearest-even, f32 as is
 *        v      = v + float(src_i) * s_i[k]        i = 1 .. n-1, left to right: one multiply, then one add
 *        v      = v + bias[k]                      only if n_bias != 0
 *        v      = vmaxps(+0, v)                    only if post_relu: ReLU(-0) = -0, ReLU(NaN) = NaN (dfx_eltwise's rule)
 *        f32 dst: store v
 *        no table: dst = cvt<dst_dt>(v)            the reorder's conversion: rint (ties to even; DFX_ROUND_NEAREST) or floor
 *                                                  (DFX_ROUND_DOWN), NaN -> 0, then clamped to [0,255] / [-128,127]
 *        table:    t = cvt<lut_in_dt>(v);  dst byte = lut[lut_in_dt == DFX_U8 ? t : t + 128]   (dfx_se's index convention),
 *                                                  stored verbatim whatever dst_dt (u8 or s8) is
 *      Denormal values are kept.  Defining properties (tests/test_gpu_wsum.py): n_inputs = 1 without bias, ReLU and table
 *      equals dfx_reorder NHWC -> NHWC with the same dtypes, scales and round mode; all scales 1.0f over one dtype equals
 *      dfx_eltwise wherever the f32 sums are exact; n_inputs = 1, scale 1 with a table is the table.  Not built:
 *      broadcasting, products, NCHW.  Parity unpinned: the reference has no such op. ---- */
enum { DFX_WSUM_MAX_INPUTS = 8 };
typedef struct dfx_wsum_desc {
  int32_t bs, h, w, c;         /* h * w * c < 2^31 (one image); the whole tensor at most 2^40 elements, 64-bit offsets */
  int32_t n_inputs;            /* 1 .. 8 */
  int32_t src_dt[8];           /* DFX_U8 | DFX_S8 | DFX_S32 | DFX_F32 each; entries from n_inputs on are ignored */
  int32_t nscales[8];          /* 1 or c each */
  int32_t n_bias;              /* 0, 1 or c (f32) */
  int32_t dst_dt;              /* DFX_U8 | DFX_S8 | DFX_F32 (DFX_S32: DFX_ERR_UNSUPPORTED, as in the reorder) */
  int32_t round_mode;          /* DFX_ROUND_* */
  int32_t post_relu;           /* 0 | 1 */
  int32_t lut_in_dt;           /* DFX_UNDEF: no table; DFX_U8 | DFX_S8: the table's index type (dst_dt must be u8 or s8) */
  int32_t force_path;          /* -1 auto, else DFX_WSUM_VEC | DFX_WSUM_GENERIC */
} dfx_wsum_desc;
enum {  /* dfx_wsum_info.path */
  DFX_WSUM_VEC = 0,            /* wsum_vec_kernel (wsum.cuh): a lane owns 16 consecutive channels of a pixel: one 16-byte
                                  load from a 1-byte input, four from a 4-byte input; one 16-byte store, four for f32.  The
                                  dtype of each input is a wave-uniform runtime switch; dst type, ReLU, table and round mode
                                  are template parameters.  Per-tensor scales and a single bias travel as kernel arguments;
                                  per-channel scales, a per-channel bias and the table are staged in LDS once per workgroup.
                                  Class: c % 16 == 0; the staged constants ((per-channel inputs + per-channel bias) * c
                                  floats + the table) fit 64 KiB; every pointer 16-byte aligned (checked per submit: other
                                  pointers take the generic kernel for that submit).  Bit-identical to the generic kernel.
                                  AUTO RULE: see DFX_WSUM_AUTO_NOTE below. */
  DFX_WSUM_GENERIC = 1         /* everything else: one thread per output element, grid-stride */
};
/* DFX_WSUM_AUTO_NOTE: auto takes DFX_WSUM_VEC in its class only where the tensor has at least 2^19 elements (a vec launch
 * of 128 workgroups or more), DFX_WSUM_GENERIC below.  On the 10 points of profiles/wsum/bench_wsum.txt (res2 shortcut
 * 56x56x256 u8 + u8 and u8 + s32, MobileNetV2 14x14x96 s8 + s8, FPN 64x64x256 with per-channel scales, an h-swish table
 * pass on 112x112x32; N = 1 and 128 / 16; buffers in rotation beyond the Infinity Cache, three legs interleaved) the vec
 * kernel is 1.3 to 5.4 times faster than the generic one on the 8 points from 802 816 elements up (1.4 to 5.2 TB/s of
 * algorithmic bytes at N = 16 / 128), but both sit on the launch floor below: 14x14x96 at N = 1 (18 816 elements, 5
 * workgroups) is 6 % slower on the vec kernel (6.1 against 5.7 us) and the table pass at N = 1 (401 408 elements, 98
 * workgroups) 1.7 times slower (6.2 against 3.6 us).  The threshold lies between those 98 and the 196 workgroups of the
 * smallest point the vec kernel wins. */
typedef struct dfx_wsum_info {
  int32_t path;                /* the handle's plan (a misaligned submit falls back without changing it) */
  int32_t grid, block, lds_bytes;
  int32_t device;
  uint64_t algorithmic_bytes;  /* all inputs + dst, one submit */
  char kernel_name[96];
} dfx_wsum_info;
typedef struct dfx_wsum dfx_wsum_t;

/* ---- net head: channel top-k / argmax and softmax over a ROW MATRIX, the last layer of every network README lists -- a
 *      classifier's {bs, 1000} logits behind dfx_fc (softmax / top-5) and a segmentation net's logits behind dfx_resize
 *      (argmax: 1 byte per pixel instead of 21, or 32 with the band kernel's padding).
 *        src    `rows` rows of `c` valid channels, consecutive rows src_ld ELEMENTS apart.  No layout change: an NHWC
 *               {bs,h,w,C} tensor is rows = bs*h*w, src_ld = C, c <= C (DeepLab's 21 logits padded to 32 are read in
 *               place); dfx_fc's {bs, oc} dst is rows = bs.  Channels c .. src_ld-1 of a row NEVER take part, whatever
 *               they hold.
 *      DFX_HEAD_TOPK (argmax is k = 1): src u8 / s8 / s32 / f32, k in 1 .. 8, k <= c.
 *        ORDER  total.  Integers order as themselves; f32 orders by IEEE totalOrder on the bit pattern:
 *               -NaN < -Inf < ... < -0 < +0 < ... < +Inf < +NaN.  Row r's results are its k largest elements sorted by
 *               (value descending, channel index ascending): equal values keep the lower index first.  Because the order
 *               is total and ties are decided by the index, all (value, index) pairs of a row are distinct, so a
 *               sequential scan and ANY tree reduction give the same bits: the three kernels agree bit for bit.
 *        idx    {rows, k}, rows idx_ld elements apart, dst_dt = DFX_S32, or DFX_U8 when c <= 256
 *        val    optional (may be NULL at submit): {rows, k} of src's dtype, rows idx_ld elements apart: the elements
 *               themselves, bits verbatim (NaN payloads, -0, denormals)
 *      DFX_HEAD_SOFTMAX: 1-byte src only (u8 / s8; a 4-byte src is DFX_ERR_UNSUPPORTED: dfx_reorder it to 1 byte first).
 *        No exp runs on the device or anywhere in the library: the caller gives a 256-entry uint32 table E
 *        (dfx_head_set_table), indexed by the distance from the row maximum.  For row r:
 *          m   = max_k src[r,k]                    as an integer
 *          d_k = m - src[r,k]                      0 .. 255 for both dtypes
 *          S   = sum_k E[d_k]                      exact in u32 (set_table refuses a table that could overflow it)
 *          p_k = float(E[d_k]) / float(S)          each conversion rounds once to nearest even; ONE correctly rounded f32
 *                                                  division
 *          f32 dst: store p_k
 *          u8 dst:  v = p_k * out_scale            one separately rounded multiply, no FMA;  then the reorder's conversion
 *                                                  (rint to even, clamped to [0,255])
 *        dst rows are dst_ld >= c elements apart; elements c .. dst_ld-1 are NOT written.
 *        THE TABLE.  E[d] = floor(exp(-d * s) * floor((2^32 - 1) / c)) for a logit step s (Python: dfa.softmax_table(s, c))
 *        keeps S within u32 for every row and is within 1e-6 absolute of a float64 softmax for c up to 65535.
 *      Not built: the argmax fused into dfx_resize's store, softmax of s32 / f32 logits, NCHW, softmax + top-k in one
 *      launch.  k > 8 over the channels of one row is dfx_select's (h = w = 1, k up to 4096, 1-byte scores), as is a
 *      selection that crosses pixels.  Parity unpinned: the reference has no such op. ---- */
enum { DFX_HEAD_TOPK = 0, DFX_HEAD_SOFTMAX = 1 };  /* dfx_head_desc.mode */
enum { DFX_HEAD_MAX_K = 8, DFX_HEAD_MAX_C = 65535 };
typedef struct dfx_head_desc {
  int64_t rows;                /* >= 1; rows * max(src_ld, dst_ld or idx_ld) <= 2^40, 64-bit offsets */
  int32_t mode;                /* DFX_HEAD_TOPK | DFX_HEAD_SOFTMAX */
  int32_t src_dt;              /* DFX_U8 | DFX_S8 | DFX_S32 | DFX_F32 (softmax: u8 / s8 only) */
  int32_t dst_dt;              /* TOPK: idx type DFX_S32 | DFX_U8 (u8 needs c <= 256);  SOFTMAX: DFX_F32 | DFX_U8 */
  int32_t c;                   /* valid channels, 1 .. 65535 */
  int32_t src_ld;              /* elements between rows of src, >= c */
  int32_t dst_ld;              /* SOFTMAX: elements between rows of dst, >= c;  TOPK: ignored */
  int32_t idx_ld;              /* TOPK: elements between rows of idx (and of val), >= k;  SOFTMAX: ignored */
  int32_t k;                   /* TOPK: 1 .. 8, <= c;  SOFTMAX: ignored */
  float out_scale;             /* SOFTMAX with u8 dst: finite (255.0f for full range);  ignored otherwise */
  int32_t force_path;          /* -1 auto, else DFX_HEAD_PIXEL | DFX_HEAD_ROW | DFX_HEAD_GENERIC */
} dfx_head_desc;
enum {  /* dfx_head_info.path */
  DFX_HEAD_PIXEL = 0,          /* head_pixel_kernel (head.cuh): a lane owns a row (segmentation: millions of short rows).
                                  Class: 1-byte src; TOPK with k = 1, or SOFTMAX; src_ld % 16 == 0 and src_ld <= 160;
                                  every pointer 16-byte aligned (checked per submit: others take the generic kernel for
                                  that submit).  16-byte loads, the last group masked by c. */
  DFX_HEAD_ROW = 1,            /* head_row_kernel: a wave owns a row, four rows per workgroup (classifier: few long rows).
                                  Class: any dtype, any k, either mode; src_ld * element size % 16 == 0; pointers 16-byte
                                  aligned per submit.  Lanes scan 16-byte groups at a stride of 64 groups and meet through
                                  wave shuffles on (key, index) pairs. */
  DFX_HEAD_GENERIC = 2         /* one thread per row, a sequential scan, any alignment and src_ld, grid-stride.  It
                                  defines the arithmetic of the other two. */
};
/* DFX_HEAD_AUTO_NOTE: auto takes DFX_HEAD_PIXEL everywhere in its class, except a softmax of 160-byte rows, which takes
 * DFX_HEAD_ROW; outside the pixel class it takes DFX_HEAD_ROW in its class where a row has at least 160 bytes (src_ld *
 * element size), and DFX_HEAD_GENERIC everywhere else.  On the 20 points of profiles/head/bench_head.txt (MI355X, buffers in
 * rotation beyond the Infinity Cache, forced legs alternating): the pixel kernel beats the generic one on all 10 points of
 * its class -- argmax and softmax u8 -> u8 at 1x65x65, 16x129x129 and 4x513x513 x 21/32, 8x512x1024x19/32 and
 * 8x128x128x150/160 -- by 1.1x (4.4 against 5.0 us on the launch floor) to 6.5x, 35 us (2.4 TB/s of valid channels +
 * idx) for the Cityscapes-size argmax.  The row kernel beats the generic one on all 11 points with rows of 160 bytes or
 * more (150/160 u8: 1.5x and 2.6x; top-5 / softmax of {bs, 1000} s8 and f32 at bs 1, 8, 128: 18x to 90x, 4.7 to 11.4 us)
 * and loses on the 7 points with 32-byte rows above the launch floor (7x to 39x: 62 of a wave's 64 lanes idle; at 4225
 * rows, on the launch floor, it is 7 % and 13 % faster than the generic one and slower than the pixel one), so it is not on auto below 160 bytes; rows between 32 and 160
 * bytes are unmeasured and stay generic.  At 8x128x128x150/160 the softmax takes
 * 153 us on the row kernel against 181 (pixel) and 393 (generic), the argmax 12.5 us on the pixel kernel against 53.8 (row):
 * hence the one exception. */
typedef struct dfx_head_info {
  int32_t path;                /* the handle's plan (a misaligned submit falls back without changing it) */
  int32_t grid, block, lds_bytes;
  int32_t device;
  uint64_t algorithmic_bytes;  /* what one submit must read and write: rows * c src elements + idx (TOPK; val, when
                                  given, adds rows * k src elements) or + rows * c dst elements (SOFTMAX) */
  char kernel_name[96];        /* mode, dtypes, k and path: "head_row<topk5,s8->s32>", "head_pixel<softmax,u8->u8>" */
} dfx_head_info;
typedef struct dfx_head dfx_head_t;

/* ---- image-wide top-K with peak filter: what every detector does behind its last conv -- CenterNet's 100 best of a
 *      128 x 128 x 80 heat map that are 3x3 local maxima, the 1000 best anchors of a RetinaNet / SSD level above a score
 *      threshold, an RPN's 2000 pre-NMS proposals -- on the device, with the rows of the regression maps (wh / offset, box
 *      deltas) gathered behind it.  dfx_head selects over the channels of ONE pixel; this op selects over a whole image.
 *        src    NHWC {bs, h, w, src_ld}, u8 or s8; c valid channels, 1 <= c <= src_ld <= 65535.  Channels c .. src_ld-1
 *               NEVER take part, whatever they hold.  A {bs, N} row matrix is h = w = 1, c = N.
 *        e      the element index inside an image, over the VALID channels: e = (y * w + x) * c + k, so pixel = e / c and
 *               class = e % c.  h * w * c <= 2^31 - 1; bs * h * w * src_ld <= 2^40.
 *        CANDIDATES.  Element (y, x, k) is a candidate iff (1) src >= min_val (the dtype's minimum: all) and (2) with
 *               peak = DFX_SELECT_PEAK3 it is >= every element of the same channel and image at (y + dy, x + dx), dy, dx in
 *               {-1, 0, 1}, that lies inside the image -- exactly "dfx_pool MAX 3x3 / 1, pad 1 equals src"; equal neighbours
 *               are both candidates.  DFX_SELECT_ALL skips (2).
 *        ORDER  dfx_head's: value descending, e ascending.  All (value, e) pairs are distinct, so the result does not
 *               depend on how the work is cut or scheduled: every kernel gives the same bits.
 *        RESULT for image r: count[r] = min(k, candidates); idx[r][0 .. count-1] the e's of the best candidates in that
 *               order (s32 {bs, k}, rows idx_ld >= k apart); the same entries of the optional val the elements themselves
 *               (src's dtype, the same leading dimension).  Entries count .. k-1 are written too: idx -1, val 0; elements
 *               k .. idx_ld-1 are not written.  count is s32 {bs}, always written.  k may exceed h * w * c.
 *        GATHER n_gather in 0 .. 4 byte maps that share bs, h, w with src: source i has pixel_stride_bytes[i] bytes per
 *               pixel, of which the first row_bytes[i] (1 .. 1024) are copied verbatim, for entry j < count[r] with pixel
 *               p = idx / c, from offset (r * h * w + p) * pixel_stride_bytes[i] into out_i[r][j]; out_i is {bs, k,
 *               row_bytes[i]}, dense; rows j >= count[r] are zero-filled.  Bytes only: dtypes do not matter.
 *      The algorithm is exact for 1-byte scores: a histogram of the 256 keys, the threshold key, compaction, a sort of at
 *      most 4096 pairs.  Not built: s32 / f32 scores (DFX_ERR_UNSUPPORTED: they need a multi-pass radix), k > 4096 (NMS and
 *      box decoding: dfx_nms below), windows other than 3x3, NCHW, the peak test fused into the producing conv's epilogue, a sigmoid
 *      table in front (dfx_wsum with a table today).  Parity unpinned: the reference has no such op. ---- */
enum { DFX_SELECT_ALL = 0, DFX_SELECT_PEAK3 = 1 };  /* dfx_select_desc.peak */
enum { DFX_SELECT_MAX_K = 4096, DFX_SELECT_MAX_GATHER = 4, DFX_SELECT_MAX_ROW_BYTES = 1024 };
typedef struct dfx_select_desc {
  int32_t bs, h, w;
  int32_t c;                   /* valid channels, 1 .. 65535 */
  int32_t src_ld;              /* elements between pixels of src, c .. 65535 */
  int32_t src_dt;              /* DFX_U8 | DFX_S8 (DFX_S32 / DFX_F32: DFX_ERR_UNSUPPORTED) */
  int32_t k;                   /* 1 .. DFX_SELECT_MAX_K */
  int32_t idx_ld;              /* elements between rows of idx (and of val), >= k */
  int32_t peak;                /* DFX_SELECT_ALL | DFX_SELECT_PEAK3 */
  int32_t min_val;             /* in src's dtype range; the dtype's minimum admits every element */
  int32_t n_gather;            /* 0 .. DFX_SELECT_MAX_GATHER */
  int32_t row_bytes[4];        /* 1 .. DFX_SELECT_MAX_ROW_BYTES */
  int32_t pixel_stride_bytes[4]; /* row_bytes[i] .. 65536 */
  int32_t force_path;          /* -1 auto, else DFX_SELECT_HIST | DFX_SELECT_GENERIC */
} dfx_select_desc;
enum {  /* dfx_select_info.path */
  DFX_SELECT_HIST = 0,         /* four launches (select.cuh).  Class: src_ld % 16 == 0; src and every output 16-byte
                                  aligned (checked per submit: others take the generic kernel for that submit).  An image
                                  is cut into chunks of consecutive pixels.  A: a workgroup per (image, chunk), 16-byte
                                  loads, the candidate test on 16 channels at once, per-wave LDS histograms, plain stores
                                  into a slab [bs][chunks][256].  B: a workgroup per image finds the threshold key and every
                                  chunk's offsets and tie-bin quota from the slab alone.  C: the grid of A writes (key, e)
                                  pairs into cand[bs][k]; the tie bin goes to the lowest e's through an ordered rank.  D: a
                                  workgroup per image sorts at most 4096 pairs in LDS, stores idx / val / fill / count and
                                  gathers.  No flags, spins, arrival counters or global atomics. */
  DFX_SELECT_GENERIC = 1       /* one workgroup per image does all of it, byte loads, any alignment and src_ld.  It
                                  defines the bits. */
};
/* DFX_SELECT_AUTO_NOTE: auto takes DFX_SELECT_HIST in its class from images of 4096 bytes (h * w * src_ld) on, and
 * DFX_SELECT_GENERIC below that and outside the class.  On the 15 points of profiles/select/bench_select.txt (MI355X,
 * buffers in rotation beyond the Infinity Cache, forced legs alternating) the histogram path beats the generic kernel on all
 * 13 points whose image has more than one pixel: CenterNet 128x128x80 peak3 k 100 at bs 1 / 8 / 32 in 60 / 73 / 150 us
 * against 7.9 to 8.4 ms; a RetinaNet level 100x136x720 min 128 k 1000 at bs 1 / 8 in 99 / 117 us against 19 ms; RPN
 * 200x304x3/16 k 2000 in 62 against 384 us; 64-channel peak3 maps from 64x64 down to 8x8 (4096 bytes: 25.9 against 32.3 us
 * at bs 1, 28.6 against 34.8 at bs 8).  It loses on both classifier rows {bs, 1000/1008} k 100 (25.7 against 17.0 us at bs 1,
 * 30.3 against 18.1 at bs 128): four launches against one on a kilobyte of work.  Images between 1008 and 4096 bytes are
 * unmeasured and stay generic.  Nothing is near the floor of reading src once: the best point, RetinaNet bs 8, takes 8.8
 * times as long (DESIGN.md section 4.18 says what bounds it). */
typedef struct dfx_select_info {
  int32_t path;                /* the handle's plan (a misaligned submit falls back without changing it) */
  int32_t chunks;              /* chunks per image (1 on the generic path) */
  int32_t chunk_pixels;        /* pixels per chunk (h * w on the generic path) */
  int32_t grid;                /* workgroups of launches A and C (generic: of the one launch) */
  int32_t grid_image;          /* workgroups of launches B and D: one per image */
  int32_t block;               /* lanes of launches A and C (generic: of the one launch) */
  int32_t block_image;         /* lanes of launches B and D */
  int32_t lds_bytes;           /* the largest of the path's kernels */
  int32_t launches;            /* per submit */
  int32_t device;
  uint64_t scratch_bytes;      /* slab + plan + cand, owned by the handle (0 on the generic path) */
  uint64_t algorithmic_bytes;  /* bs * h * w * c src + idx + count + the gather rows read and written (val, when given,
                                  adds bs * k) */
  char kernel_name[96];        /* "select_hist<peak3,u8,k100>", "select_generic<all,s8,k1000>" */
} dfx_select_info;
typedef struct dfx_select dfx_select_t;

/* ---- box decode + greedy non-maximum suppression: what a RetinaNet / SSD level or an RPN does behind its top-K, on the
 *      device.  Per image r the op takes n <= 4096 candidates in PRIORITY ORDER, position 0 best -- what dfx_select emits --
 *      and never looks at a score.  Every floating-point operation below is ONE separately rounded f32 operation in the
 *      order written, so the result is a function of the inputs alone and every kernel gives the same bits.
 *        count_in s32 {bs} or NULL: n_valid[r] = min(max(count_in[r], 0), n), n without it.  Positions >= n_valid do not exist.
 *        mode = DFX_NMS_BOXES   boxes f32 {bs, n, 4} as (x1, y1, x2, y2), dense.
 *        mode = DFX_NMS_DECODE  idx s32 {bs, n}, rows idx_ld apart (select's idx); deltas {bs, n, row_bytes} bytes (a select
 *               gather destination: the pixel row of a delta map, 4 * A bytes used); anchors f32 {n_anchors, 4}, shared by
 *               all images; tab_c, tab_s f32 [256], indexed by the RAW byte (the caller builds them: no exp in the library).
 *               With e = idx[j]: anchor g = e / classes, a = g % A; bytes q0..q3 = row[4a .. 4a+3] (dx, dy, dw, dh);
 *                 aw = ax2 - ax1, ah = ay2 - ay1, acx = ax1 + 0.5 * aw, acy = ay1 + 0.5 * ah,
 *                 cx = acx + tab_c[q0] * aw, cy = acy + tab_c[q1] * ah, w = aw * tab_s[q2], hh = ah * tab_s[q3],
 *                 x1 = cx - 0.5 * w, y1 = cy - 0.5 * hh, x2 = cx + 0.5 * w, y2 = cy + 0.5 * hh;
 *               then, if clip_w > 0: x = x < 0 ? 0 : x; x = x > clip_w ? clip_w : x on x1 and x2, likewise y with clip_h
 *               (the comparisons exactly so: a NaN stays a NaN).  torchvision's BoxCoder.decode_single and
 *               clip_boxes_to_image with dx / wx and exp(min(dw / ww, clip)) folded into the tables.
 *        INVALID  an entry with e < 0 or e >= n_anchors * classes (wherever idx is read): never kept, never suppresses.
 *        LABELS   per_class = 1: label = idx[j] % classes (BOXES mode then needs idx, which it does not read otherwise);
 *               per_class = 0: all labels are equal.
 *        TEST   for positions i < j, a = box i, b = box j (the lower position is always a): area(x) = (x2 - x1) * (y2 - y1);
 *               xx1 = a.x1 > b.x1 ? a.x1 : b.x1, yy1 likewise; xx2 = a.x2 < b.x2 ? a.x2 : b.x2, yy2 likewise;
 *               w = xx2 - xx1; w = w > 0 ? w : 0, h likewise; inter = w * h; u = (area_a + area_b) - inter; i suppresses j
 *               iff the labels are equal and inter / u > iou_thr (0 / 0 is NaN and does not suppress): torchvision's nms.
 *        GREEDY walk j upward; a valid j is kept iff no KEPT i < j suppresses it; stop once max_out are kept.
 *        RESULT keep s32 {bs, max_out}, rows keep_ld >= max_out apart: the kept positions ascending, -1 behind the count
 *               (elements max_out .. keep_ld-1 are not written); count s32 {bs}; the optional boxes_out f32 {bs, max_out, 4}:
 *               the kept boxes (decoded in DECODE mode), zeros behind the count.
 *      Not built: min-size filtering, soft-NMS, rotated boxes, scores re-sorted after the decode, CenterNet's decode (it
 *      needs no NMS), n > 4096.  Parity unpinned: the reference has no such op. ---- */
enum { DFX_NMS_BOXES = 0, DFX_NMS_DECODE = 1 };  /* dfx_nms_desc.mode */
enum { DFX_NMS_MAX_N = 4096 };
typedef struct dfx_nms_desc {
  int32_t bs;
  int32_t n;                   /* candidates per image, 1 .. DFX_NMS_MAX_N */
  int32_t max_out;             /* 1 .. n */
  int32_t keep_ld;             /* elements between rows of keep, >= max_out */
  int32_t mode;                /* DFX_NMS_BOXES | DFX_NMS_DECODE */
  int32_t per_class;           /* 0 | 1 */
  int32_t classes;             /* >= 1 */
  int32_t anchors_per_pixel;   /* A >= 1 */
  int32_t n_anchors;           /* >= 1; n_anchors * classes <= 2^31 - 1 */
  int32_t row_bytes;           /* DECODE: bytes between delta rows, >= 4 * A */
  int32_t idx_ld;              /* elements between rows of idx, >= n */
  float iou_thr;               /* finite */
  float clip_w, clip_h;        /* DECODE: clip_w > 0 clips to [0, clip_w] x [0, clip_h] */
  int32_t force_path;          /* -1 auto, else DFX_NMS_MASK | DFX_NMS_GENERIC */
} dfx_nms_desc;
/* the device pointers of one submit */
typedef struct dfx_nms_io {
  const void *boxes;           /* BOXES */
  const void *idx;             /* DECODE, and BOXES with per_class; else may be NULL */
  const void *deltas, *anchors, *tab_c, *tab_s;  /* DECODE */
  const void *count_in;        /* may be NULL */
  void *keep, *count;
  void *boxes_out;             /* may be NULL */
} dfx_nms_io;
enum {  /* dfx_nms_info.path */
  DFX_NMS_MASK = 0,            /* three launches (nms.cuh) through scratch owned by the handle.  Class, checked per submit:
                                  boxes / idx / anchors and every output 16-byte aligned (others take the generic kernel for
                                  that submit).  A: decode (or copy) into box[bs][n] float4 and lab[bs][n].  B: one wave per
                                  64 x 64 tile of the upper triangle, lane t owns row box t, the 64 column boxes are LDS
                                  broadcast reads; one u64 "row suppresses column" per lane, stored plainly.  C: one wave per
                                  image, lane l holds word l of the removed bitmap; per 64-row block the diagonal tile is
                                  resolved serially, then every lane ORs its word of the kept rows (512 coalesced bytes per
                                  row).  No flags, spins, arrival counters or global atomics. */
  DFX_NMS_GENERIC = 1          /* one workgroup of 1024 lanes per image: boxes, labels and an alive map in LDS, a serial walk
                                  with a barrier per kept box.  One launch, no scratch, any alignment.  It defines the bits. */
};
/* DFX_NMS_AUTO_NOTE: auto takes DFX_NMS_MASK for n >= 200 and max_out >= 100, the smallest of each at which it was measured
 * and won, and DFX_NMS_GENERIC below either.  On the 24 points of profiles/nms/bench_nms.txt (MI355X, buffers in rotation,
 * forced legs alternating; us, mask against generic) the mask path beats the generic kernel on all 20 detector points: a
 * RetinaNet level n 1000, 80 classes, max_out 100 in 30.2 against 52.2 at bs 1 and 31.0 against 52.6 at bs 8, max_out 300 in
 * 51.6 / 53.5 against 143.9 / 145.3; RPN n 2000, thr 0.7, max_out 1000 in 148 / 158 against 675 / 679; SSD n 200 in 38.9 / 41.5
 * against 77.5 / 83.4; n 4096 at 3.4 % kept in 78.7 / 134.7 against 476 / 481 and at 67 % kept in 364 / 420 against 2435 / 2458;
 * BOXES mode within 2 us of DECODE everywhere.  It loses where little is kept: n 1000 with max_out 20 takes 20.4 / 21.5 against
 * 12.5 / 13.0 (three launches against one barrier per kept box), and n 100 is a tie (21.4 / 24.9 against 22.4 / 23.1); those
 * stay generic, as do the unmeasured sizes between.  Against the host round trip it replaces (D2H, scalar loop, H2D: its
 * two copies alone are 17 to 42 us) the mask path is 2x to 140x faster at bs 8 and from n 2000 on, and NOT faster at bs 1
 * with n <= 1000: 29.3 against 28.3 us, 51.6 against 49.1, 38.9 against 34.1 (DESIGN.md section 4.19 says what bounds it). */
typedef struct dfx_nms_info {
  int32_t path;                /* the handle's plan (a misaligned submit falls back without changing it) */
  int32_t tiles;               /* 64 x 64 tiles of the upper triangle per image (0 on the generic path) */
  int32_t grid_prep, grid_mask, grid_scan;  /* workgroups of launches A, B, C (generic: grid_scan is its one launch) */
  int32_t block_prep, block_mask, block_scan;
  int32_t lds_bytes;           /* the largest of the path's kernels */
  int32_t launches;            /* per submit */
  int32_t device;
  uint64_t scratch_bytes;      /* box + lab + mask + tile table, owned by the handle (0 on the generic path) */
  uint64_t algorithmic_bytes;  /* boxes (or idx + 4 * A delta bytes + an anchor) read, keep + count written; boxes_out, when
                                  given, adds bs * max_out * 16 */
  char kernel_name[96];        /* "nms_mask<decode,perclass,n1000>", "nms_generic<boxes,agnostic,n200>" */
} dfx_nms_info;
typedef struct dfx_nms dfx_nms_t;

/* ---- RoIAlign: the step between an RPN's kept boxes and a two-stage detector's heads (Faster R-CNN's 7 x 7 box head,
 *      Mask R-CNN's 14 x 14 mask head), on the device.  Every floating-point operation below is ONE separately rounded f32
 *      operation in the order written, so the result is a function of the inputs alone and every kernel gives the same bits.
 *        LEVELS  1 .. 4 feature maps of one dtype (u8, s8 or f32), level l NHWC {bs, h[l], w[l], c} with pixel stride
 *               src_ld[l] >= c elements (pad channels are never read), h[l], w[l] in 1 .. 65535, and its own
 *               spatial_scale[l], finite and > 0.
 *        ROIS   mode = DFX_ROI_BATCHED  boxes f32 {bs, n, 4} as (x1, y1, x2, y2), dense: dfx_nms's boxes_out with n = its
 *               max_out.  count s32 {bs} or NULL (dfx_nms's count): n_valid[r] = min(max(count[r], 0), n), n without it.
 *               RoI j of image r reads image r; R = bs * n output rows, rows at positions >= n_valid[r] are zeros.
 *               mode = DFX_ROI_LIST     boxes f32 {R, 4} with R = n, batch_idx s32 {R}: row i reads image batch_idx[i]; a row
 *               whose index lies outside [0, bs) is zeros.
 *        OUTPUT dst {R, ph, pw, c} NHWC of src's dtype with pixel stride dst_ld >= c; elements c .. dst_ld-1 of a pixel
 *               are not written.  ph, pw in 1 .. 64; sampling_ratio S in 1 .. 4 (torchvision's adaptive sampling_ratio = 0
 *               is DFX_ERR_UNSUPPORTED); aligned 0 or 1.
 *        LEVEL  area = (x2 - x1) * (y2 - y1); the level is the number of i < levels - 1 with area >= level_area_thr[i]
 *               (finite, non-decreasing; a NaN area gives level 0).  No log2 on the device: the caller builds the thresholds.
 *        ARITHMETIC, with s the level's scale, o = aligned ? 0.5f : 0.0f, H and W the level's size:
 *               rsw = x1 * s - o, rsh = y1 * s - o, rew = x2 * s - o, reh = y2 * s - o              (a mul, then a sub)
 *               rw = rew - rsw, rh = reh - rsh; if (!aligned) { rw = rw > 1 ? rw : 1; rh = rh > 1 ? rh : 1; }
 *               bw = rw / (float)pw, bh = rh / (float)ph
 *               for bin row p and iy in 0 .. S-1:  y = (rsh + (float)p * bh) + (((float)iy + 0.5f) * bh) / (float)S
 *                 yvalid = (y >= -1.0f && y <= (float)H)          (this form exactly: a NaN is invalid)
 *                 if (y <= 0) y = 0; yl = (int)y; if (yl >= H - 1) { yh = yl = H - 1; y = (float)yl; } else yh = yl + 1
 *                 ly = y - (float)yl, hy = 1.0f - ly              (likewise x, xl, xh, lx, hx, xvalid from rsw, bw, W)
 *               sample(iy, ix) = yvalid && xvalid ? ((w1 * v1 + w2 * v2) + w3 * v3) + w4 * v4 : +0.0f
 *                 with w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx and v1 = src[yl][xl], v2 = src[yl][xh],
 *                 v3 = src[yh][xl], v4 = src[yh][xh] converted to f32
 *               acc = +0.0f; acc += sample(iy, ix), iy ascending, ix ascending within iy; out = acc / (float)(S * S)
 *               u8 / s8: out is rounded to nearest even and saturated, as dfx_reorder and dfx_resize convert; f32 is stored
 *               as it is.  A sample is left out only by its valid bits, never because a weight is zero: an f32 Inf under
 *               a zero weight gives NaN on every kernel.
 *      Nothing can fault: invalid coordinates never become addresses and every index that is used is clamped into the map.
 *      This is torchvision's roi_align forward.  Parity unpinned: torchvision's build may contract the multiplies and adds.
 *      Not built: adaptive sampling, RoIPool / max mode, rotated RoIs, NCHW, position-sensitive pooling, u8 -> f32
 *      output. ---- */
enum { DFX_ROI_BATCHED = 0, DFX_ROI_LIST = 1 };  /* dfx_roialign_desc.mode */
enum { DFX_ROIALIGN_MAX_LEVELS = 4, DFX_ROIALIGN_MAX_BINS = 64, DFX_ROIALIGN_MAX_SAMPLING = 4 };
typedef struct dfx_roialign_desc {
  int32_t bs;
  int32_t n;                   /* BATCHED: RoIs per image (R = bs * n); LIST: R */
  int32_t mode;                /* DFX_ROI_BATCHED | DFX_ROI_LIST */
  int32_t levels;              /* 1 .. 4 */
  int32_t c;
  int32_t dt;                  /* DFX_U8 | DFX_S8 | DFX_F32 */
  int32_t h[4], w[4];          /* 1 .. 65535 each; entries from `levels` on are ignored */
  int32_t src_ld[4];           /* elements between pixels of a level, >= c */
  float spatial_scale[4];      /* finite, > 0 */
  float level_area_thr[3];     /* levels - 1 used: finite, non-decreasing */
  int32_t ph, pw;              /* 1 .. 64 */
  int32_t sampling_ratio;      /* 1 .. 4; 0 is DFX_ERR_UNSUPPORTED */
  int32_t aligned;             /* 0 | 1 */
  int32_t dst_ld;              /* elements between pixels of dst, >= c */
  int32_t force_path;          /* -1 auto, else DFX_ROIALIGN_TILE | DFX_ROIALIGN_GENERIC */
} dfx_roialign_desc;
/* the device pointers of one submit */
typedef struct dfx_roialign_io {
  const void *src[4];          /* the levels */
  const void *boxes;
  const void *count;           /* BATCHED; may be NULL */
  const void *batch_idx;       /* LIST */
  void *dst;
} dfx_roialign_io;
enum {  /* dfx_roialign_info.path */
  DFX_ROIALIGN_TILE = 0,       /* one launch (roialign.cuh).  Class: u8 / s8 with c % 16 == 0 or f32 with c % 4 == 0, and every
                                  ld a whole number of 16 bytes; checked per submit: every level, boxes and dst 16-byte aligned
                                  (others take the generic kernel for that submit).  A workgroup owns one RoI, or a run of
                                  bin rows of one where the plan splits RoIs because R is small against the CU count; its
                                  lanes write the two per-axis sample tables (low / high offset, two weights, valid) into
                                  LDS, one barrier, then a lane owns one 16-byte channel group of one bin: four 16-byte
                                  corner loads per sample, bytes converted in registers, one 16-byte store.  No atomics,
                                  flags or cross-workgroup communication. */
  DFX_ROIALIGN_GENERIC = 1     /* one thread per output element; any c, ld and alignment.  It defines the bits. */
};
/* DFX_ROIALIGN_AUTO_NOTE: auto takes DFX_ROIALIGN_TILE inside its class for c * sizeof(element) >= 256 bytes, R >= 100
 * RoIs and ph * pw >= 49 bins, the smallest of each at which it was measured and won, and DFX_ROIALIGN_GENERIC below any
 * of them and outside the class.  On the 8 points of profiles/roialign/bench_roialign.txt (MI355X, buffers in rotation,
 * forced legs alternating; us, tile against generic; S 2, levels by area) the tile kernel wins on every one: the Faster
 * R-CNN-FPN box head (4 levels x 256 u8, n 1000, 7 x 7) in 27.3 against 162.7 at bs 1 and 181 against 1183 at bs 8; the
 * mask head (n 100, 14 x 14) in 15.7 against 67.4 and 79.8 against 483; a C4 head (50 x 76 x 1024 u8, n 300, 14 x 14) in
 * 116 against 687 and 650 against 5116; the box head in f32 in 65.5 against 184 and 486 against 1220.  Nothing smaller
 * was timed (fewer channels, fewer RoIs, fewer bins, S other than 2 -- S is not part of the rule), so those stay on the
 * generic kernel; DFX_ROIALIGN_TILE is reachable there with force_path and gives the same bits.  What bounds it:
 * DESIGN.md section 4.20. */
typedef struct dfx_roialign_info {
  int32_t path;                /* the handle's plan (a misaligned submit falls back without changing it) */
  int32_t grid, block;
  int32_t lds_bytes;
  int32_t launches;            /* per submit: 1 */
  int32_t device;
  int32_t rows_per_group;      /* tile path: bin rows a workgroup owns (ph unless the plan splits RoIs); 0 on generic */
  uint64_t algorithmic_bytes;  /* boxes + count / batch_idx read, four corner pixels per sample read, dst written */
  char kernel_name[96];        /* "roialign_tile<u8,7x7,s2,l4>", "roialign_generic<f32,14x14,s2,l1>" */
} dfx_roialign_info;
typedef struct dfx_roialign dfx_roialign_t;

/* ---- batched int8 matrix product over two DEVICE tensors: the one multiply whose second operand is not a weight the host
 *      packs -- Q.K^T and P.V of a non-local / self-attention block (ResNet / Mask R-CNN non-local, DANet / OCRNet / CCNet
 *      context modules, DETR and ViT-hybrid / MobileViT / Swin encoders) and correlation (cost-volume) layers.  With
 *      dfx_head's table softmax between two of them an int8 attention block runs on the device:
 *      s8 x s8 -> s8 logits, softmax -> u8, u8 x s8 -> s8.
 *        g = b0 * batch1 + b1,   0 <= b0 < batch0, 0 <= b1 < batch1
 *        acc[g,m,n] = sum over k of A[g,m,k] * B[g,n,k]      (trans_b = 1, B is {N,K}, k contiguous:  Q.K^T)
 *                   = sum over k of A[g,m,k] * B[g,k,n]      (trans_b = 0, B is {K,N}, n contiguous:  P.V)
 *        f = float(acc);  f = f * scale[n or 0];  ReLU (asked for, or dst is u8): f = (0 > f) ? 0 : f
 *        C[g,m,n] = store(f, dst_dt, round_mode)
 *      With a LOGIT BIAS set on the handle (dfx_bmm_set_bias, dfx_logit_bias_desc below):
 *        f = float(acc);  f = f + bias(g,m,n);  f = f * scale[n or 0];  ReLU;  C[g,m,n] = store(f, dst_dt, round_mode)
 *      which is requant() verbatim: one separately rounded f32 add BEFORE the multiply, never an FMA.  The bias is therefore
 *      in ACCUMULATOR units: bias_real / (logit_step * logit_scale) for logits whose s8 step is logit_step.
 *      OPERANDS.  A u8 or s8; B s8 (u8 B: DFX_ERR_UNSUPPORTED, not built); C u8 / s8 / s32 / f32.
 *      ADDRESSING, in elements, per operand: element (g, row, col) of A is at a + b0*a_s0 + b1*a_s1 + row*lda + col; B uses
 *      b_s0, b_s1, ldb and C uses c_s0, c_s1, ldc in the same way.  The heads of a {bs, T, heads*d} NHWC tensor are read
 *      without a copy with s0 = T*heads*d, s1 = d, ld = heads*d, and the context is written back interleaved in that shape.
 *      A batch stride of 0 on A or B broadcasts that operand; on C it is never allowed (see the overlap rule below).
 *      PAD COLUMNS.  Columns beyond the valid extent of a row NEVER take part, whatever they hold: K .. lda-1 of A,
 *      K .. ldb-1 of B (trans_b = 1), N .. ldb-1 of B (trans_b = 0); elements N .. ldc-1 of a C row are NOT written
 *      (dfx_head's rule: a softmax output with dst_ld = 208 for 197 tokens is A as it stands).  Every row of A and B is
 *      readable up to its valid columns rounded up to 16, which the leading dimension admits on the MFMA path (that kernel
 *      reads whole 16-byte pieces and masks them).
 *      ARITHMETIC.  dfx_fc's, word for word: exact s32 accumulation (1 <= K <= 65025), requant() / gc_quarter whose bias
 *      slot holds +0.0f (the identity: float(int) is never -0) or the logit bias's {m, n} entry, a separately rounded
 *      multiply, the x86 conversion and saturations of dfx_device.cuh.
 *      REQUANT ROUTE.  The op never sees its operands on the host, so dfx_bmm_set_scales proves the route from the shape
 *      alone: "fast" when the round mode is nearest, DFX_NO_FAST is not set, every scale is finite and
 *      bound * |scale| <= 2^30 with bound = 255*128*K (u8 A) or 128*128*K (s8 A); otherwise "exact".  The generic kernel is
 *      always exact.  Both routes give the same bits wherever "fast" is allowed.
 *      With a logit bias the proof is (bound + max |finite bias entry|) * |scale| <= 2^30 and NO non-finite entry: a -inf
 *      anywhere takes the exact route (the fast route's conversion is not defined there).
 *      LOGIT BIAS VALUES.  Finite f32 values and -inf; +inf or NaN anywhere in the addressed table: DFX_ERR_INVALID.  A -inf
 *      entry follows the exact route's x86 semantics: the sum is -inf, the product -inf, +inf or NaN by the scale's sign,
 *      vcvtps2dq gives 0x80000000 for all three, so an s8 C stores -128 whatever the sign of the scale (no ReLU).
 *      WHAT A MASK GIVES.  The masked logit is -128, no less.  In a softmax behind it (dfx_head, dfx_attn) its probability is
 *      E[max + 128] of the caller's table over the row sum: 0 once that table entry is 0 or the u8 rounding takes it, and not
 *      before.  A FULLY masked row is uniform over all its keys (every logit is -128); torch gives NaN there.
 *      Not built: u8 B, split-K for tiny G*M*N, a per-channel bias vector as dfx_fc has it, K > 65025, s32 / f32 operands;
 *      of the logit bias: a device-resident table (per-batch masks that change every submit without a host call), f16 / s8
 *      storage of the table, skipping fully masked key tiles (a causal speed-up), a mask input to dfx_head, two separate
 *      bias operands (the host sums rel_bias[h] + mask[w] once).  (The softmax fused between the two products, one launch,
 *      is dfx_attn below.)
 *      Parity unpinned: the reference has no such op. ---- */
typedef struct dfx_bmm_desc {
  int32_t batch0, batch1;      /* >= 1; G = batch0 * batch1 matrices */
  int32_t m, n, k;             /* >= 1; m, n <= 2^31 - 32; k <= 65025 */
  int32_t trans_b;             /* 1: B is {N,K} (Q.K^T);  0: B is {K,N} (P.V) */
  int32_t a_dt;                /* DFX_U8 | DFX_S8 */
  int32_t b_dt;                /* DFX_S8 (DFX_U8: DFX_ERR_UNSUPPORTED) */
  int32_t dst_dt;              /* DFX_F32 | DFX_S32 | DFX_S8 | DFX_U8 */
  int32_t relu, round_mode;
  int32_t nscales;             /* 1 or n */
  int32_t force_path;          /* -1 auto, else DFX_BMM_* (testing) */
  int64_t a_s0, a_s1, lda;     /* elements; batch strides >= 0 (0 broadcasts), lda >= k */
  int64_t b_s0, b_s1, ldb;     /* ldb >= k (trans_b = 1) or >= n (trans_b = 0) */
  int64_t c_s0, c_s1, ldc;     /* ldc >= n; no two elements of C may share an address */
} dfx_bmm_desc;
/* The HOST layout of a logit bias (dfx_bmm_set_bias / dfx_attn_set_bias): period0 x period1 tables of {m, n} f32 values in
 * accumulator units, or of one row {n} broadcast over m.  Matrix (b0, b1) uses table (b0 % period0, b1 % period1).
 *   Swin: batch0 = images x windows, batch1 = heads, period0 = nW (the shifted-window mask repeats per image; 1 on
 *   un-shifted blocks), period1 = heads; the host sums rel_bias[h] + mask[w] once.  DETR key padding: period0 = bs,
 *   period1 = 1, ld = 0 (a {bs, tk} table).  Causal: periods 1 and one {T, T} table.
 * The library copies the addressed entries into a device image {period0 * period1, m or 1, n rounded up to 32} it owns (at
 * most 2^30 bytes: larger is DFX_ERR_UNSUPPORTED). */
typedef struct dfx_logit_bias_desc {
  int32_t period0, period1;    /* 1 <= period0 <= batch0, 1 <= period1 <= batch1 */
  int64_t s0, s1, ld;          /* in floats, >= 0: table (p0,p1) row m col n at p0*s0 + p1*s1 + m*ld + n;
                                  ld == 0: one row, broadcast over m; else ld >= n */
} dfx_logit_bias_desc;
enum {  /* dfx_bmm_info.path */
  DFX_BMM_MFMA = 0,            /* bmm_mfma_kernel (bmm.cuh): v_mfma_i32_32x32x32_i8, one launch, requant in the epilogue.
                                  Class: lda, ldb and the batch strides of A and B multiples of 16 elements; a and b 16-byte
                                  aligned (checked per submit: others take the generic kernel for that submit).  Any M, N, K.
                                  AUTO RULE: see DFX_BMM_AUTO_NOTE below. */
  DFX_BMM_GENERIC = 1          /* one thread per C element, grid-stride, any strides and alignment, exact requant.  It
                                  defines the bits. */
};
/* DFX_BMM_AUTO_NOTE: auto takes DFX_BMM_MFMA in its class for M >= 49, N >= 32, K >= 32, G * M * N * K >= 192 * 49 * 49 * 32 and
 * at least 384 tiles of 32 x 32 (G * ceil(M / 32) * ceil(N / 32)), the smallest of each at which it was measured and won, and
 * DFX_BMM_GENERIC everywhere else.  On the 12 points of profiles/bmm/bench_bmm.txt (MI355X, buffers in rotation beyond the
 * Infinity Cache, forced legs alternating, windows of at least 3 ms, median of 5 rounds whose extremes lie within 5 % of it but
 * for one outlying round at each Swin point; both products of an attention block over head-sliced tensors, s8 out): the MFMA
 * kernel beats the generic one on all 12 -- ViT-B (heads 12, T 197, d 64) at bs 8 in 10.3 / 11.0 us (Q.K^T / P.V) against 435 / 200
 * and at bs 64 in 54 / 33 us against 3536 / 1232; a Swin stage (192 windows, T 49, d 32) in 4.9 / 5.6 us against 17.8 / 17.3; a
 * DETR encoder (bs 2, heads 8, T 850, d 32) in 16.0 / 27.7 us against 643 / 275; a non-local block (T 4096, d 256) at bs 1 in
 * 42 / 116 us against 5388 / 2083 and at bs 4 in 160 / 123 us against 23898 / 8848: 3.1x to 150x.  Nothing smaller was timed
 * (M = 1, K < 32, a handful of matrices, a few tiles under a deep K), so those stay on the generic kernel; DFX_BMM_MFMA is
 * reachable there with force_path and gives the same bits.  Against what a caller had before (profiles/bmm/): 1.27x faster
 * than dfx_fc on the one batch-1 NT point, 1.8x to 4.3x faster than torch.matmul on f16 copies at the ViT-B, Swin and DETR
 * Q.K^T points, and SLOWER than torch at DETR P.V (0.97x) and at every non-local point (0.23x to 0.49x of f16 matmul, 0.16x to
 * 0.70x of torch._int_mm).  What bounds it: DESIGN.md section 4.21 (at best 6 % of the int8 matrix peak and 19 % of the HBM
 * peak: one 32 x 32 tile per wave re-reads its operands). */
typedef struct dfx_bmm_info {
  int32_t path;                /* the handle's plan (a misaligned submit falls back without changing it) */
  int32_t grid, block, lds_bytes;
  int32_t device;
  uint64_t algorithmic_ops;    /* 2 * G * M * N * K */
  uint64_t algorithmic_bytes;  /* the distinct bytes of A, B and C: a broadcast operand counts once; plus, while a logit bias is
                                  set, the distinct bytes of its tables */
  char kernel_name[96];        /* "bmm_mfma<nt,u8,s8> fast": form (nt | nn), A type, dst type, route (after set_scales); the
                                  suffix " +bias" while a logit bias is set */
} dfx_bmm_info;
typedef struct dfx_bmm dfx_bmm_t;

/* ---- fused int8 attention: Q.K^T, the table softmax and P.V behind ONE handle and, on the fused path, in ONE launch with
 *      the logits and the probabilities kept on chip.  It is DEFINED as the chain of the three existing ops, by reference
 *      (their arithmetic is not restated here), for every matrix g = b0 * batch1 + b1:
 *        L[m,n] = dfx_bmm (trans_b = 1, a_dt = q_dt, dst s8, nscales 1, no ReLU, scale = logit_scale) of Q[g] {tq,d} and
 *                 K[g] {tk,d}:  m < tq, n < tk, contraction over d
 *        P[m,:] = dfx_head DFX_HEAD_SOFTMAX (src s8, dst u8, c = tk, table E, out_scale = prob_scale) of L[m,:]
 *        O[m,j] = dfx_bmm (trans_b = 0, a_dt u8, scales = out_scales[1 or dv], relu, dst_dt) of P[g] {tq,tk} and V[g] {tk,dv}:
 *                 j < dv, contraction over tk
 *      round_mode applies to both requants; the softmax's u8 conversion is dfx_head's (rint to even).  Because the softmax
 *      is a table lookup on max - x, S an exact u32 sum and the division one correctly rounded f32 division, nothing has to
 *      be rescaled online: the fused kernel is bit-identical to the chain.
 *      OPERANDS.  Q u8 or s8; K and V s8 (u8: DFX_ERR_UNSUPPORTED, not built); O u8 / s8 / s32 / f32.
 *      ADDRESSING.  Each of Q, K, V, O has two batch strides and a leading dimension in elements with dfx_bmm's meaning:
 *      a batch stride of 0 broadcasts Q, K or V and is never allowed on O (dfx_bmm's C-overlap rule holds for O).  Heads of
 *      a {bs, T, heads*d} tensor are read in place and the context is written back interleaved.  Pad columns never take
 *      part (d .. ldq-1 of Q, d .. ldk-1 of K, dv .. ldv-1 of V); elements dv .. ldo-1 of an O row are NOT written.  Every row
 *      of Q, K and V is readable up to its valid columns rounded up to 16 (dfx_bmm's rule: the MFMA kernels read whole pieces).
 *      LIMITS.  1 <= d <= 65025 (dfx_bmm's K), 1 <= tk <= 65025 (the context's K; dfx_head's c would admit 65535), tq and dv <= 2^31 - 32, every
 *      operand's index range and the logits' G * tq * up16(tk) below 2^40.
 *      REQUANT ROUTES.  Proved from the shape as dfx_bmm_set_scales does: bound 128*128*d (s8 Q) or 255*128*d (u8 Q) against
 *      logit_scale for the logits, 255*128*tk against out_scales for the context.
 *      LOGIT BIAS.  dfx_attn_set_bias sets dfx_bmm's logit bias (dfx_logit_bias_desc, its values and its mask semantics, all
 *      above) on the logits' product and on nothing else: L = dfx_bmm(Q, K) WITH that bias, then dfx_head's softmax and
 *      dfx_bmm(P, V), both unchanged.  With m = tq, n = tk, batch = (batch0, batch1): a per-head relative-position table, a
 *      shifted-window mask, a key-padding row and a causal mask are all layouts of it.  A masked logit is -128; its
 *      probability is E[max + 128] over the row sum (0 once the table or the u8 rounding says so); a fully masked row is
 *      uniform over all tk keys (torch: NaN).  The logits' route is then proved with the bias (dfx_bmm's rule).  A bias does
 *      not change the handle's plan: the biased fused kernel was timed against the biased chain at the points of
 *      DFX_ATTN_AUTO_NOTE and won and lost where the unbiased one does (below).
 *      Not built: u8 K / V, P or L as an output, f32 probabilities between the products, multi-device sharding; of the logit
 *      bias: a device-resident table, f16 / s8 storage, skipping fully masked key tiles (a causal speed-up), a mask input
 *      to dfx_head, two separate bias operands, anything for the non-local point's speed.  Parity unpinned: the reference has
 *      no such op. ---- */
typedef struct dfx_attn_desc {
  int32_t batch0, batch1;      /* >= 1; G = batch0 * batch1 matrices */
  int32_t tq, tk, d, dv;       /* >= 1; tq, dv <= 2^31 - 32; tk <= 65025; d <= 65025 */
  int32_t q_dt;                /* DFX_U8 | DFX_S8 */
  int32_t k_dt, v_dt;          /* DFX_S8 (DFX_U8: DFX_ERR_UNSUPPORTED) */
  int32_t dst_dt;              /* DFX_F32 | DFX_S32 | DFX_S8 | DFX_U8 */
  int32_t relu, round_mode;
  int32_t nscales;             /* out scales: 1 or dv */
  int32_t force_path;          /* -1 auto, else DFX_ATTN_* */
  float prob_scale;            /* finite; dfx_head's out_scale (255.0f for full range) */
  int32_t reserved;            /* ignored */
  int64_t q_s0, q_s1, ldq;     /* elements; batch strides >= 0 (0 broadcasts), ldq >= d */
  int64_t k_s0, k_s1, ldk;     /* ldk >= d */
  int64_t v_s0, v_s1, ldv;     /* ldv >= dv */
  int64_t o_s0, o_s1, ldo;     /* ldo >= dv; no two elements of O may share an address */
} dfx_attn_desc;
enum {  /* dfx_attn_info.path */
  DFX_ATTN_FUSED = 0,          /* attn_fused_kernel (attn.cuh): one launch, no scratch in HBM.  A workgroup of four waves owns
                                  a strip of 32 query rows of one g: logits by v_mfma_i32_32x32x32_i8 into an LDS strip, the
                                  softmax in place in LDS, the context by the same MFMA with P read from LDS.
                                  Class: ldq, ldk, ldv and the batch strides of Q, K, V multiples of 16 elements; d <= 256
                                  (the strip's Q fragments stay in 32 VGPRs); tk <= 4096 (the strip, the table and the V images:
                                  1024 + 32 * (up16(tk) + 16) + 12288 bytes of LDS, 141.5 KiB at tk 4096); q, k, v 16-byte
                                  aligned (checked per submit: others take the chain for that submit).
                                  AUTO RULE: see DFX_ATTN_AUTO_NOTE below. */
  DFX_ATTN_CHAIN = 1           /* the three existing ops on the caller's stream, each on its own auto path, with L and P
                                  ({G, tq, up16(tk)} bytes each) in scratch the handle owns.  It accepts everything the
                                  descriptor accepts and, with those ops' generic kernels, defines the bits. */
};
/* DFX_ATTN_AUTO_NOTE: auto takes DFX_ATTN_FUSED in its class for tq >= 49, 49 <= tk <= 850, 32 <= d <= 64, 32 <= dv <= 64 and at
 * least 384 strips of 32 query rows (G * ceil(tq / 32), the fused kernel's workgroups), and DFX_ATTN_CHAIN everywhere else.  The
 * lower bounds are the smallest of each at which it was timed against the chain and won, the upper bounds the largest: beyond them
 * lies a point where it LOSES.  On the 6 points of profiles/attn/bench_attn.txt (MI355X, s8 Q / K / V / O head-sliced in place, forced
 * legs alternating in one process, buffers in rotation beyond the Infinity Cache, windows of at least 3 ms, median of 5 rounds whose
 * extremes lie within 3.6 % of it): ViT-B (heads 12, T 197, d 64) at bs 8 in 22.6 us against the chain's 46.7 (0.48x) and at bs 64 in
 * 134 us against 259 (0.52x); a Swin stage (192 windows of 49, d 32: two strips per window, the second with 17 of its 32 rows) in
 * 12.5 us against 21.8 (0.57x); a DETR encoder (bs 2, heads 8, T 850, d 32) in 41.6 us against 63.8 (0.65x); and a non-local block
 * (T 4096, d = dv = 256) at bs 1 in 389 us against 186 (2.09x SLOWER: 128 workgroups on 256 CUs) and at bs 4 in 780 us against 358
 * (2.18x SLOWER): there a strip holds 141.5 KiB of LDS, so a CU runs ONE workgroup of four waves, and every strip re-reads all of K
 * and V (2 MiB) through L2 with nothing to hide the latency.  The floor (Q, K, V and O once at 8 TB/s) is 0.6 / 4.8 / 0.15 / 0.22 /
 * 0.5 / 2.1 us: the fused kernel is 37x to 750x above it.  Nothing between the box and the non-local point (tk 851 .. 4095, d or dv
 * 65 .. 255), nothing smaller and nothing with fewer strips was timed: all of it stays on the chain; DFX_ATTN_FUSED is reachable
 * there with force_path and gives the same bits.
 * WITH A LOGIT BIAS the rule is the same box (profiles/attn/bench_attn_bias.txt, the same method, the four legs alternating; a
 * key-padding row per image, at the Swin stage one {49, 49} table per (window, head)): the biased fused kernel beats the biased
 * chain at ViT-B bs 8 in 22.8 us against 49.0 (0.47x) and at bs 64 in 134 us against 260 (0.51x), at the Swin stage in 13.4 us
 * against 22.4 (0.60x), at the DETR encoder in 41.9 us against 66.5 (0.63x), every time by far more than the rounds' spread (at
 * most 3.5 %), and loses at the non-local point as it does without a bias (2.06x / 2.15x).  What the bias costs: DESIGN.md
 * section 4.22. */
typedef struct dfx_attn_info {
  int32_t path;                /* the handle's plan (a misaligned submit falls back to the chain without changing it) */
  int32_t grid, block, lds_bytes; /* of the fused kernel; 0 on the chain (see the three ops' own queries) */
  int32_t device;
  int32_t route_logits, route_context; /* 0 exact, 1 fast, as the last set_scales proved them; -1 before it */
  uint64_t scratch_bytes;      /* L and P together, as the handle holds them now: 0 on a fused handle until a submit has fallen
                                  back to the chain */
  uint64_t algorithmic_ops;    /* 2 * G * tq * tk * (d + dv) */
  uint64_t algorithmic_bytes;  /* the distinct bytes of Q, K, V and O: a broadcast operand counts once (the floor); plus, while a
                                  logit bias is set, the distinct bytes of its tables */
  char kernel_name[96];        /* "attn_fused<s8,s8> fast/exact": Q type, dst type, logits / context route; "attn_chain<...>";
                                  the suffix " +bias" while a logit bias is set */
} dfx_attn_info;
typedef struct dfx_attn dfx_attn_t;

/* ---- int8 layer norm / RMS norm over a ROW MATRIX: the normalisation in front of every attention and every MLP of a
 *      transformer block (ViT, Swin, DETR encoders, MobileViT), so that inner_product -> attention -> scaled_sum chains
 *      stay on the device.  No MFMA, HBM-bound.
 *
 *      Inputs.  src is a row matrix as in dfx_head: `rows` rows of `c` valid channels, src_ld >= c elements apart, dtype u8
 *      or s8.  Channels c .. src_ld-1 never take part, whatever they hold.  dst is rows dst_ld >= c elements apart, dtype
 *      u8, s8 or f32.  Elements c .. dst_ld-1 are NOT written.  1 <= c <= DFX_LNORM_MAX_C = 16384.  The other parameters:
 *        gamma[c], beta[c]  f32 per channel, any bit patterns.  beta == NULL means zeros, and the add is still performed.
 *        shift[c]           optional, a u8 per channel with values 0 .. 7.  NULL means all 0.  This is FQ-ViT's power-of-two
 *                           factor and makes an 8-bit layer-norm input realistic.
 *        eps                f32, finite and > 0, in units of the integer domain.  The caller passes eps_real / in_scale^2.
 *
 *      Per row, with x_k the element as an integer:
 *
 *        t_k = x_k * 2^shift[k]                      |t_k| <= 32640
 *        S   = sum t_k                                exact, |S| <= 32640*c < 2^30
 *        Q   = sum t_k^2                              exact, < 2^44 (u64)
 *
 *        DFX_LNORM_LAYER:
 *          D   = c*Q - S^2                            exact u64, 0 <= D < 2^58   (c^2 x the biased variance)
 *          v   = fdiv(u64->f32(D), f32(c*c))          each conversion rounds once to nearest even; ONE correctly rounded division
 *          u_k = c*t_k - S                            exact s32, |u_k| < 2^31
 *          a   = fdiv(fdiv(1.0f, sqrt(fadd(v, eps))), f32(c))     f32(c) is exact
 *        DFX_LNORM_RMS:
 *          v   = fdiv(u64->f32(Q), f32(c))
 *          u_k = t_k
 *          a   = fdiv(1.0f, sqrt(fadd(v, eps)))
 *
 *        y_k = fadd(fmul(fmul(s32->f32(u_k), a), gamma[k]), beta[k])      every operation rounded separately, no FMA
 *        f32 dst: store y_k.   u8 / s8 dst: the reorder's conversion (rint to even, NaN -> 0, clamp to the dtype's range).
 *
 *      The bounds above are what makes 16384 the limit; static assertions in csrc/lnorm_plan.h restate them.  The output
 *      scale is folded into gamma and beta by the caller (Python: dfa.lnorm_params).  S, Q and D are exact integers, so the
 *      order in which lanes add them does not matter; everything behind them is a fixed sequence of single-rounded f32
 *      operations (sqrt is the correctly rounded one), so a sequential scan and any tree give the same bits: both kernels
 *      agree bit for bit.  A constant row has D = 0 and u_k = 0, so y_k = beta[k] exactly.
 *      Not built: s32 / f32 sources (their sums are not order-free), in-place operation, a fused residual add, group /
 *      instance norm, mean / rstd as outputs, c > 16384.  Parity unpinned: the reference has no such op. ---- */
enum { DFX_LNORM_LAYER = 0, DFX_LNORM_RMS = 1 };
enum { DFX_LNORM_MAX_C = 16384, DFX_LNORM_MAX_SHIFT = 7 };
typedef struct dfx_lnorm_desc {
  int64_t rows;                /* >= 1; rows * max(src_ld, dst_ld) <= 2^40 */
  int32_t mode, src_dt /* U8|S8 */, dst_dt /* U8|S8|F32 */, c, src_ld, dst_ld;
  float   eps;                 /* finite, > 0 */
  int32_t force_path;          /* -1 auto | DFX_LNORM_ROW | DFX_LNORM_GENERIC */
} dfx_lnorm_desc;
enum {  /* dfx_lnorm_info.path */
  DFX_LNORM_ROW = 0,           /* lnorm_row_kernel<W> (lnorm.cuh): W in {4, 8, 16, 32, 64} consecutive lanes own a row, W the
                                  smallest of these >= ceil(c / 16), capped at 64; a 256-lane workgroup handles 256 / W rows
                                  per trip, grid-stride.  Class: src_ld % 16 == 0, dst_ld * element size % 16 == 0; pointers
                                  16-byte aligned (checked per submit: others take the generic kernel for that submit).
                                  16-byte loads and stores, the last group masked by c; a lane keeps its first four groups
                                  in registers over both passes; gamma / beta staged in LDS where 8 * c bytes <= 64 KiB. */
  DFX_LNORM_GENERIC = 1        /* one thread per row, sequential, any alignment and leading dimension, grid-stride.  It
                                  defines the bits. */
};
/* DFX_LNORM_AUTO_NOTE: UNMEASURED.  The row kernel has not been timed on an MI355X yet (tools/bench_lnorm is the
 * instrument; profiles/lnorm/README.md), so auto takes DFX_LNORM_GENERIC everywhere and DFX_LNORM_ROW runs only where
 * force_path asks for it -- dfx_dwpw's precedent: no path is on auto before a measurement puts it there. */
typedef struct dfx_lnorm_info {
  int32_t path;                /* the handle's plan (a misaligned submit falls back without changing it) */
  int32_t grid, block, lds_bytes;
  int32_t device;
  uint64_t algorithmic_bytes;  /* what one submit must read and write: rows * c src bytes + rows * c dst elements + gamma,
                                  beta (8 * c) and, when given, shift (c) */
  char kernel_name[96];        /* mode, dtypes, lanes per row, shifts: "lnorm_row<layer,s8->s8,w16,shift>",
                                  "lnorm_generic<rms,u8->f32>" */
} dfx_lnorm_info;
typedef struct dfx_lnorm dfx_lnorm_t;

/* ---- window partition / reverse of an NHWC token grid: what turns a {bs, h, w, C} map into the windows a Swin block attends
 *      over and back (with the cyclic shift of SW-MSA and the padding of maps that are no multiple of the window), Swin's patch
 *      merging gather (a 2 x 2 partition, column-major), depth-to-space (Swin-UNet's patch expanding) and space-to-depth (YOLO's
 *      reorg / Focus).  Data movement only: bytes are moved, never converted; no arithmetic, no requant route.
 *
 *      Two row matrices of ONE dtype (u8 / s8 / s32 / f32):
 *        grid side    bs * h * w tokens of c valid elements; token (b, y, x) is row (b * h + y) * w + x; rows grid_ld >= c
 *                     elements apart.
 *        window side  bs * nW * wh * ww tokens, rows win_ld >= c elements apart, with hp = ceil(h / wh) * wh,
 *                     wp = ceil(w / ww) * ww, nW = (hp / wh) * (wp / ww).  Window (b, wy, wx) is matrix b * nW + wy * (wp / ww)
 *                     + wx: what attention_strides(bs * nW, heads, wh * ww, d, ld) and a logit bias of period0 = nW expect.
 *                     In-window token (iy, ix) is row iy * ww + ix for DFX_WINDOW_ROW_MAJOR and ix * wh + iy for
 *                     DFX_WINDOW_COL_MAJOR (patch merging's x0, x1, x2, x3 order: with wh = ww = 2 and win_ld = c the four rows
 *                     of a window read as one row of 4 c).
 *      The mapping is official Swin's: pad to hp x wp, then torch.roll(-shift).  The window-side token at padded coordinates
 *      (Y, X) = (wy * wh + iy, wx * ww + ix) corresponds to grid (y, x) = ((Y + shift_y) mod hp, (X + shift_x) mod wp); it is a
 *      PAD TOKEN when y >= h or x >= w.
 *        DFX_WINDOW_PARTITION (grid -> window): the c elements of every window-side token are written exactly once; pad tokens
 *                     get pad_value, a 32-bit pattern whose low byte is used for 1-byte dtypes (a u8 zero point).
 *        DFX_WINDOW_REVERSE (window -> grid): the exact inverse; every grid token is written exactly once, pad tokens are not
 *                     read and pad_value is ignored.
 *      On either side columns c .. ld-1 are never read or written.  Limits: bs >= 1; h, w in 1 .. 65535; wh, ww in 1 .. 255 (a
 *      window larger than the image is all padding beyond the image); 0 <= shift_y < hp, 0 <= shift_x < wp; hp * wp <= 2^22;
 *      bs * hp * wp * max(grid_ld, win_ld) <= 2^40.  All byte offsets are 64-bit.
 *      Shift, padding, order and direction exist only in ONE int32 table of the destination's rows within one image, built on the
 *      host with exact integer arithmetic (csrc/window_plan.h) and uploaded at create: both kernels are row gathers with contiguous
 *      stores, dst row (b, r) <- src row b * src_rows_per_image + map[r].
 *      Not built: a fused scaled residual add on reverse, a row map inside dfx_attn / dfx_linear that would make the two passes
 *      disappear, NCHW, dtype conversion, overlapping windows (neighbourhood attention), hp * wp > 2^22.  Parity unpinned: the
 *      reference has no such op. ---- */
enum { DFX_WINDOW_PARTITION = 0, DFX_WINDOW_REVERSE = 1 };
enum { DFX_WINDOW_ROW_MAJOR = 0, DFX_WINDOW_COL_MAJOR = 1 };
enum { DFX_WINDOW_MAX_HW = 65535, DFX_WINDOW_MAX_WIN = 255, DFX_WINDOW_MAX_PADDED = 1 << 22 };
typedef struct dfx_window_desc {
  int32_t dir;                 /* DFX_WINDOW_PARTITION | DFX_WINDOW_REVERSE */
  int32_t dt;                  /* U8 | S8 | S32 | F32, of both sides */
  int32_t bs, h, w, c;
  int32_t wh, ww, shift_y, shift_x;
  int32_t order;               /* DFX_WINDOW_ROW_MAJOR | DFX_WINDOW_COL_MAJOR */
  int64_t grid_ld, win_ld;     /* >= c, in elements */
  uint32_t pad_value;          /* PARTITION: what pad tokens are filled with */
  int32_t force_path;          /* -1 auto | DFX_WINDOW_ROW | DFX_WINDOW_GENERIC */
} dfx_window_desc;
enum {  /* dfx_window_info.path */
  DFX_WINDOW_ROW = 0,          /* window_row_kernel (window.cuh): a lane moves one 16-byte group, c * esize / 16 consecutive lanes
                                  per token (any count: 96 channels -> 6), consecutive lanes run on into the next destination row,
                                  so stores are contiguous and loads contiguous in runs of at least one token; four groups per
                                  lane and trip, all loaded before the first store; no LDS.  Class: c * esize, grid_ld * esize and
                                  win_ld * esize multiples of 16; pointers 16-byte aligned (checked per submit: others take the
                                  generic kernel for that submit). */
  DFX_WINDOW_GENERIC = 1       /* one thread per element, any alignment and pitch, grid-stride.  It defines the bits. */
};
/* DFX_WINDOW_AUTO_NOTE: UNMEASURED.  The row kernel has not been timed on an MI355X yet (tools/bench_window is the
 * instrument; profiles/window/README.md), so auto takes DFX_WINDOW_GENERIC everywhere and DFX_WINDOW_ROW runs only where
 * force_path asks for it -- dfx_lnorm's precedent: no path is on auto before a measurement puts it there. */
typedef struct dfx_window_info {
  int32_t path;                /* the handle's plan (a misaligned submit falls back without changing it) */
  int32_t grid, block;
  int32_t device;
  uint64_t algorithmic_bytes;  /* valid bytes read + valid bytes written + the map: PARTITION bs * (h * w + hp * wp) * c * esize +
                                  4 * hp * wp, REVERSE 2 * bs * h * w * c * esize + 4 * h * w */
  char kernel_name[96];        /* direction, dtype, lanes per token: "window_row<partition,s8,l6>", "window_generic<reverse,f32>" */
} dfx_window_info;
typedef struct dfx_window dfx_window_t;

/* ---- int8 token linear layer over a ROW MATRIX: the four weight multiplies of a transformer block (QKV projection, output
 *      projection, fc1 + GELU, fc2) between dfx_lnorm, dfx_attn and dfx_wsum, weight-stationary.
 *
 *      Operands.  src is a row matrix as in dfx_lnorm and dfx_head: `rows` rows of `k` valid elements, src_ld >= k elements
 *      apart, dtype u8 or s8.  Columns k .. src_ld-1 never take part, whatever they hold.  wei is s8 {n, k}, plain row-major
 *      (an nn.Linear weight), a HOST pointer at set_weights.  bia is an optional per-n vector of any of the four dtypes,
 *      converted as dfx_fc converts it.  scales: 1 or n.  dst is rows dst_ld >= n elements apart, u8 / s8 / s32 / f32;
 *      elements n .. dst_ld-1 are NOT written.  Any rows >= 1 with rows * max(src_ld, dst_ld) <= 2^40, any n >= 1
 *      (n <= 2^31 - 128), 1 <= k <= 65025.
 *
 *      Arithmetic: dfx_fc's, word for word.  acc = sum_c src[m][c] * wei[o][c] is an exact s32; then
 *        f = float(acc); f = f + bias[o]; f = f * scale[o or 0]; ReLU (asked for, or the stored type is u8); store
 *      with a separately rounded add and multiply, never an FMA, and the x86 conversion and saturations of
 *      csrc/dfx_device.cuh (f32: the value; s32: vcvtps2dq under the round mode; s8 / u8: that, then signed / unsigned
 *      saturation).
 *
 *      Optional table (lut_in_dt = DFX_U8 | DFX_S8; DFX_UNDEF: none; dfx_linear_set_table).  The requant above produces the
 *      byte t the op would have stored with dst_dt = lut_in_dt; the op stores lut[lut_in_dt == DFX_U8 ? t : t + 128]
 *      instead -- dfx_wsum's and dfx_se's index convention.  dst_dt must be u8 or s8 and the table's bytes are stored
 *      verbatim.  With a table, ReLU is decided by relu / lut_in_dt, not by dst_dt.  This is how GELU rides behind fc1
 *      without another pass over the widest tensor of the block (Python: dfa.gelu_table).
 *
 *      Requant route: "fast" / "exact", proved at set_weights from the actual weights as dfx_fc proves it: fast when the
 *      round mode is nearest, DFX_NO_FAST is not set and, for every n, bias and scale are finite and
 *      (B + |bias|) * |scale| <= 2^30, B = 255 * max(P, N) for a u8 src and 128 * (P + N) for an s8 src (P, N: the sums of
 *      the row's positive / negative weights' magnitudes).  The generic kernel is always exact and defines the bits.
 *
 *      Not built: a fused residual add (dfx_wsum joins the residual); split-K for few tiles under a deep K; k > 65025;
 *      s32 / f32 sources; u8 weights; a fused layer norm in front; multi-device sharding.
 *      Parity unpinned: the reference has no such op. ---- */
typedef struct dfx_linear_desc {
  int64_t rows;                /* >= 1; rows * max(src_ld, dst_ld) <= 2^40 */
  int32_t k, n;
  int32_t src_dt;              /* DFX_U8 | DFX_S8 */
  int32_t dst_dt;              /* DFX_F32 | DFX_S32 | DFX_S8 | DFX_U8; with a table DFX_S8 | DFX_U8 */
  int32_t bia_dt;              /* DFX_UNDEF = none */
  int32_t relu, round_mode, nscales /* 1 | n */;
  int32_t lut_in_dt;           /* DFX_UNDEF = no table | DFX_U8 | DFX_S8 */
  int32_t force_path;          /* -1 auto | DFX_LINEAR_TILE | DFX_LINEAR_GENERIC */
  int64_t src_ld, dst_ld;      /* elements between rows: >= k, >= n */
} dfx_linear_desc;
enum {  /* dfx_linear_info.path */
  DFX_LINEAR_TILE = 0,         /* linear_tile_kernel<BM> (linear.cuh): 256 lanes own a BM x 128 tile of dst, BM = 128, or 64 where
                                  128 would leave fewer tiles than CUs; K in slabs of 64; each slab of the token tile and of the
                                  weight block goes global -> LDS once per workgroup (two buffers, one barrier per slab) and
                                  feeds v_mfma_i32_32x32x32_i8 through conflict-free 16-byte LDS reads; the weights are packed
                                  by the host in the tile's own order (linear_pack.h).  Class: src_ld % 16 == 0; src 16-byte
                                  aligned (checked per submit: others take the generic kernel for that submit).  In this
                                  class a row is read up to k rounded up to 16, which lies within its pitch and within the
                                  16-byte granule of its last valid byte.  4 adjacent n leave as one store where dst is
                                  aligned for it and dst_ld % 4 == 0. */
  DFX_LINEAR_GENERIC = 1       /* one thread per dst element, grid-stride, any pitch and alignment, exact requant.  It defines
                                  the bits. */
};
/* DFX_LINEAR_AUTO_NOTE: measured with tools/bench_linear on one MI355X (profiles/linear/bench_linear.txt: s8 in and out, forced
 * legs alternating in one process, buffer sets in rotation beyond the Infinity Cache, windows of at least 3 ms, median of 5
 * rounds; the rounds' extremes are in the file: most legs stay within 1 % of their median, the widest reaches + 11 %).  The yardstick is dfx_bmm's MFMA kernel
 * on the same operands (the weights as a device B, no bias).  At the tile height the plan takes, the tile kernel beat it and the
 * generic kernel at all 14 points, by far more than the rounds' spread at 12 of them and by 6 % and 7 % at the two smallest:
 *   ViT-B rows 1576:  768->2304 11.8 us against 29.0;  768->768 10.5 / 16.4;  768->3072 + table 16.7 / 35.9;  3072->768 29.8 / 52.5
 *   ViT-B rows 12608: 768->2304 58.4 / 175.6;  768->768 29.2 / 68.9;  768->3072 + table 80.4 / 231.8;  3072->768 74.7 / 252.7
 *   Swin stage 1 rows 9408: 96->288 6.93 / 7.34;  96->384 + table 6.82 / 7.38;  384->96 7.44 / 8.69
 *   DETR rows 1700:   256->256 6.10 / 6.56;  256->2048 7.31 / 13.1;  2048->256 20.7 / 25.3
 * (the generic kernel: 108 us to 25.9 ms).  AUTO RULE: DFX_LINEAR_TILE in its class from the smallest of each size that was
 * measured -- rows >= 1576, n >= 96, k >= 96, at least 54 tiles of 64 x 128 and 1700 * 256 * 256 multiply-adds -- and
 * DFX_LINEAR_GENERIC everywhere else: nothing smaller was timed.  Where it LOSES: few tiles under a deep K, to dfx_fc's split-K
 * on a u8 copy of src -- 3072->768 at rows 1576 takes 29.8 us against 20.4, 2048->256 at rows 1700 20.7 against 14.3 -- and it
 * reaches 17 % of the 4600 TOP/s int8 matrix peak at best; eager torch._int_mm / f16 torch.matmul (no requant) are 1.18x to 1.35x
 * faster on the four ViT-B rows-12608 matrices and 1.54x at 3072->768 rows 1576 (profiles/linear/speed_vs_torch.txt; DESIGN.md
 * section 4.24). */
typedef struct dfx_linear_info {
  int32_t path;                /* the handle's plan (a misaligned submit falls back without changing it) */
  int32_t grid, block, lds_bytes;
  int32_t device;
  uint64_t algorithmic_ops;    /* 2 * rows * n * k */
  uint64_t algorithmic_bytes;  /* rows * k src bytes + n * k weights + rows * n dst elements + bias (4 n) + scales (4 each) +
                                  the table (256) */
  char kernel_name[96];        /* "linear_tile<s8,s8,bm128> fast +lut", "linear_generic<u8,f32>": src type, dst type */
} dfx_linear_info;
typedef struct dfx_linear dfx_linear_t;

/* ---- int8 patch embedding: the non-overlapping convolution (window == stride) every ViT / DeiT / Swin / ConvNeXt / PVT starts
 *      or downsamples with, as ONE GEMM that writes a TOKEN MATRIX: rows = bs * th * tw, K = ph * pw * ic, n = oc.  It adds a
 *      per-(token, channel) table (conv bias + position embedding) and leaves / fills rows in front of every image's tokens
 *      (class token, DeiT's distillation token, register tokens).
 *
 *      Operands.  src is NHWC {bs, ih, iw, ic}, u8 or s8, ic >= 1, at any byte address.  Patches are ph x pw (1 .. 255 each),
 *      th x tw of them per image, 1 <= th <= ih / ph, 1 <= tw <= iw / pw: pixels beyond th * ph rows / tw * pw columns are
 *      never read; there is no padding.  K = ph * pw * ic <= 65025.  wei is s8 {oc, ic, ph, pw}, plain oihw, a HOST pointer at
 *      set_weights (dfx_imgconv's layout).  dst is a row matrix of bs * img_rows rows, dst_ld >= oc elements apart, u8 / s8 /
 *      s32 / f32: token t = ty * tw + tx of image b is row b * img_rows + tok_offset + t, elements 0 .. oc-1.  Elements
 *      oc .. dst_ld-1 are NOT written; rows tok_offset + th * tw .. img_rows-1 are NOT written.
 *
 *      Arithmetic: dfx_imgconv's, and therefore dfx_fc's, word for word.  acc = the exact s32 sum over (i, ky, kx); then
 *        f = float(acc); f = f + bias[o]  or  f = f + table[t][o]  (one separately rounded add; skipped where neither exists);
 *        f = f * scale[o or 0]; ReLU (asked for, or dst is u8); store
 *      with the x86 conversion and saturations of csrc/dfx_device.cuh, never an FMA.
 *
 *      Table (table = 1; dfx_patchembed_set_table): f32 {th * tw, oc} in ACCUMULATOR units, a host pointer with a leading
 *      dimension; entries must be finite.  table = 1 with bia_dt != DFX_UNDEF is DFX_ERR_INVALID: the caller folds the conv
 *      bias into the table (Python: dfa.patch_embed_table), so there is one add on every route.  The padded device copy
 *      {th * tw, oc rounded up to 4} f32 must not exceed 2^30 bytes.
 *
 *      Prefix (dfx_patchembed_set_prefix): tok_offset * oc elements of dst's dtype from the host, already quantised (Python:
 *      dfa.patch_embed_prefix).  The launch that computes the tokens stores them verbatim into rows 0 .. tok_offset-1 of every
 *      image; every element is written exactly once.  Without a prefix those rows are not written.
 *
 *      Requant route: "fast" / "exact", proved per channel from the actual weights as dfx_linear proves it, with
 *      max_t |table[t][o]| in the place of |bias[o]|; proved again whenever weights or table change.  The generic kernel is
 *      always exact and defines the bits.
 *
 *      Not built: overlapping windows or padding (dfx_imgconv); runs pw * ic that are not multiples of 4 bytes on the tile
 *      kernel (ViT /14 on RGB); f32 / NCHW images (dfx_reorder first); Swin's patch merging; a fused layer norm behind the
 *      embedding; split-K; a device-resident table; interpolated position embeddings.
 *      Parity unpinned: the reference has no such op. ---- */
typedef struct dfx_patchembed_desc {
  int32_t bs, ih, iw, ic;      /* src NHWC; bs * ih * iw * ic <= 2^40; ph * iw * ic < 2^31 */
  int32_t ph, pw;              /* 1 .. 255; K = ph * pw * ic <= 65025 */
  int32_t th, tw;              /* tokens per axis: 1 <= th <= ih / ph, 1 <= tw <= iw / pw */
  int32_t oc;                  /* 1 .. 2^31 - 128 */
  int32_t src_dt;              /* DFX_U8 | DFX_S8 */
  int32_t dst_dt;              /* DFX_F32 | DFX_S32 | DFX_S8 | DFX_U8 */
  int32_t bia_dt;              /* DFX_UNDEF = none; must be DFX_UNDEF with a table */
  int32_t relu, round_mode, nscales /* 1 | oc */;
  int32_t table;               /* 0 | 1: a per-(token, channel) f32 table, dfx_patchembed_set_table */
  int32_t tok_offset;          /* t0 >= 0: dst rows in front of every image's tokens */
  int32_t force_path;          /* -1 auto | DFX_PATCHEMBED_TILE | DFX_PATCHEMBED_GENERIC */
  int64_t img_rows;            /* dst rows per image, >= tok_offset + th * tw; bs * img_rows * dst_ld <= 2^40 */
  int64_t dst_ld;              /* elements between dst rows, >= oc */
} dfx_patchembed_desc;
enum {  /* dfx_patchembed_info.path */
  DFX_PATCHEMBED_TILE = 0,     /* patchembed_tile_kernel<BM, DST, FAST, G> (patchembed.cuh): dfx_linear's tile kernel (256 lanes, a
                                  BM x 128 tile, K in slabs of 64 through two LDS buffers, v_mfma_i32_32x32x32_i8 on conflict-free
                                  16-byte LDS reads, linear_pack.h's weight image in K order (ky, kx, i)) whose token loader
                                  GATHERS: a 16-byte piece of a token's K comes from the image through a per-granule offset table
                                  the host computed, so the kernel divides nothing per slab.  Class: G = 16 where pw * ic and
                                  iw * ic are multiples of 16, G = 4 where both are multiples of 4; src aligned to G (checked per
                                  submit: others take the generic kernel for that submit). */
  DFX_PATCHEMBED_GENERIC = 1   /* one thread per dst element, grid-stride, any shape and alignment, exact requant.  It defines
                                  the bits. */
};
/* DFX_PATCHEMBED_AUTO_NOTE: measured with tools/bench_patchembed on one MI355X (profiles/patchembed/bench_patchembed.txt: s8 out, a
 * token table, forced legs alternating in one process, buffer sets in rotation beyond the Infinity Cache, windows of at least
 * 3 ms, median of 5 rounds; the rounds' extremes are in the file: most legs stay within 1 % of their median, the widest reaches
 * + 9 %).  The yardsticks are the generic kernel and (a) dfx_imgconv on auto with k = s on the same image, which is
 * what a caller had before (imgconv_generic_kernel at every point).  At the tile height the plan takes, us per submit, tile /
 * generic / (a):
 *   ViT-B/16 224  bs 1: 14.2 / 140 / 486      bs 8: 14.9 / 872 / 3545     bs 64: 37.6 / 6485 / 27208
 *   ViT-L/16 224  bs 1: 14.1 / 184 / 587      bs 8: 15.0 / 1122 / 4369    bs 64: 40.2 / 8614 / 33519
 *   ViT-B/16 384  bs 1: 14.3 / 366 / 1295     bs 8: 15.9 / 2385 / 10024   bs 64: 75.9 / 19013 / 79944
 *   ViT-L/16 384  bs 1: 14.4 / 454 / 1551     bs 8: 21.6 / 3300 / 12354   bs 64: 99.7 / 25379 / 99739
 *   ViT-B/32 224  bs 1: 35.0 / 247 / 612      bs 8: 36.2 / 896 / 3668     bs 64: 38.1 / 6699 / 28005
 *   Swin-T stem   bs 1: 7.51 / 17.6 / 19.3    bs 8: 8.71 / 115 / 145      bs 64: 48.7 / 826 / 1101
 *   ConvNeXt 2x2 96->192 s8 (no (a): ic > 4)  bs 1: 9.49 / 71.9   bs 8: 10.1 / 447   bs 64: 29.7 / 3379
 * AUTO RULE: DFX_PATCHEMBED_TILE in its class from the smallest of each size that was measured -- rows >= 49, oc >= 96, K >= 48
 * and 3136 * 96 * 48 multiply-adds -- and DFX_PATCHEMBED_GENERIC everywhere else: nothing smaller was timed.  The tile kernel won
 * at all 21 points, by 2.3x at the least (the Swin-T stem at bs 1), far beyond the rounds' spread.  Where it LOSES: to (b)
 * dfx_linear's tile kernel on a patch matrix gathered beforehand (the gather not timed, no table), at every point, by 1.23x to
 * 1.41x on the ViT points (ViT-B/16 224 bs 64: 37.6 us against 28.9), 1.35x to 1.37x on the ConvNeXt downsample and 1.46x to 1.88x
 * on the Swin-T stem (bs 64: 48.7 against 25.8): that is what the in-kernel gather and the table cost today.  Best: 582 TOP/s (12.6 % of the 4600 TOP/s int8 matrix
 * peak, ViT-L/16 384 bs 64) and 1.0 TB/s (12 % of the HBM peak, the ConvNeXt downsample at bs 64).  DESIGN.md section 4.25. */
typedef struct dfx_patchembed_info {
  int32_t path;                /* the handle's plan (a misaligned submit falls back without changing it) */
  int32_t grid, block, lds_bytes;
  int32_t device;
  int32_t granule;             /* the tile class of the descriptor: 16, 4, or 0 (outside it) */
  uint64_t algorithmic_ops;    /* 2 * bs * th * tw * oc * K */
  uint64_t algorithmic_bytes;  /* the patches' bytes + oc * K weights + the tokens' dst elements + table / bias (as f32) + scales +
                                  the prefix rows written */
  char kernel_name[96];        /* "patchembed_tile<u8,s8,bm128,g16> fast +table", "patchembed_generic<u8,f32>" */
} dfx_patchembed_info;
typedef struct dfx_patchembed dfx_patchembed_t;

/* ---- depthwise conv + pointwise conv: the depthwise-separable block of MobileNet / EfficientNet / Xception with the
 *      u8 tensor between its two convs kept on chip.  src NHWC u8 {bs,ih,iw,c}.
 *        stage 0: the depthwise conv of dfx_dwconv_desc (kh x kw, stride, padding, oh / ow given by the caller) with
 *                 dst type u8 -- ReLU and unsigned saturation are implied; it has bia0_dt, nscales0 (1 or c) and
 *                 round_mode0.
 *        stage 1: a 1x1 stride-1 unpadded conv c -> oc on that u8 tensor with bia1_dt, nscales1 (1 or oc), relu,
 *                 round_mode1 and dst_dt.
 *      dst NHWC {bs,oh,ow,oc}.  The result is, bit for bit, dfx_dwconv_submit (dst u8) followed by dfx_conv_submit of
 *      the unfused pointwise conv with the same numbers; where a dense conv can express the shape (c % 16 == 0, oh /
 *      ow equal to the conv formula) it also equals the FUSED dfx_conv with ic = oc = c, block-diagonal conv0 weights
 *      and oc1x1 = oc.  Parity unpinned: the reference asserts ngroups == 1. ---- */
typedef struct dfx_dwpw_desc {
  int32_t bs, c, ih, iw;
  int32_t oh, ow;              /* (oh - 1) * sh - pad_t <= ih - 1, likewise in x */
  int32_t kh, kw;              /* 1 .. 255 */
  int32_t sh, sw;
  int32_t pad_t, pad_l;
  int32_t oc;
  int32_t dst_dt;              /* DFX_F32 | DFX_S32 | DFX_S8 | DFX_U8 */
  int32_t bia0_dt, bia1_dt;    /* DFX_UNDEF = none */
  int32_t relu;                /* stage 1 (stage 0 always has one: its dst is u8) */
  int32_t round_mode0, round_mode1;
  int32_t nscales0;            /* 1 or c */
  int32_t nscales1;            /* 1 or oc */
  int32_t force_path;          /* -1 auto, else DFX_DWPW_* (testing) */
} dfx_dwpw_desc;
enum {  /* dfx_dwpw_info.path */
  DFX_DWPW_FUSED = 0,          /* one launch (dwpw.cuh).  Class: 3x3, stride (1,1) or (2,2), c a multiple of 32 and
                                  <= 256, oc in {64, 128, 256}, c * oc <= 64 KB, one image below 2^31 bytes on either
                                  side.  AUTO RULE: auto takes this path only where it was measured faster than the two
                                  ops by more than the +-4 % box spread; no shape has such a measurement yet (DESIGN.md
                                  4.8), so today it is reached through force_path only */
  DFX_DWPW_TWO_LAUNCH = 1      /* everything else the two ops accept: dfx_dwconv + dfx_conv through ONE u8 buffer the
                                  handle owns, both on the caller's stream */
};
typedef struct dfx_dwpw_info {
  int32_t path;
  int32_t grid, block, lds_bytes;  /* of the fused kernel / of the conv kernel of the two-launch path */
  int32_t device;
  uint64_t algorithmic_ops;    /* 2*MAC of one submit, both stages */
  uint64_t algorithmic_bytes;  /* src + weights + dst; two-launch path: + 2 x the u8 tensor between the stages */
  char kernel_name[96];        /* path, window, stride, channel counts, both requant routes (valid after set_weights) */
} dfx_dwpw_info;
typedef struct dfx_dwpw dfx_dwpw_t;
typedef void *dfx_stream_t; /* a hipStream_t; NULL = the default stream */
typedef void *dfx_event_t;  /* a hipEvent_t */

/* ---- library / device ---- */
int dfx_version(void);
const char *dfx_last_error(void);        /* thread-local message of the last failure */
int dfx_device_count(int *count);
int dfx_set_device(int ordinal);
int dfx_device_name(char *buf, size_t len);

/* ---- buffers and streams: replace util/memory.cc:21-40 (aligned_malloc/free)
 *      and util/omp_thread.h:18-25 (the OpenMP shim) ---- */
int dfx_mem_alloc_host(void **p, size_t bytes);    /* pinned host memory */
int dfx_mem_free_host(void *p);
int dfx_mem_alloc_device(void **p, size_t bytes);
int dfx_mem_free_device(void *p);
int dfx_memcpy_h2d(void *dst_dev, const void *src_host, size_t bytes, dfx_stream_t s);
int dfx_memcpy_d2h(void *dst_host, const void *src_dev, size_t bytes, dfx_stream_t s);
int dfx_memset_device(void *dst_dev, int value, size_t bytes, dfx_stream_t s);
int dfx_stream_create(dfx_stream_t *s);
int dfx_stream_destroy(dfx_stream_t s);   /* the way to destroy a stream of dfx_stream_create's: a conv handle that was
                                             submitted on it learns of it here.  A stream made elsewhere (a hipStream_t of
                                             the caller's) must outlive the handles submitted on it. */
int dfx_stream_sync(dfx_stream_t s);
/* work enqueued on `waiter` after this call starts only when everything enqueued on `producer`
 * before it has finished (chains of asynchronous submits on different streams) */
int dfx_stream_wait_stream(dfx_stream_t waiter, dfx_stream_t producer);
/* device-side timing (the DEEPFUSION_PROFILE hook of op::submit, deepfusion.cc:91-102) */
int dfx_event_create(dfx_event_t *e);
int dfx_event_record(dfx_event_t e, dfx_stream_t s);
int dfx_event_elapsed_ms(dfx_event_t start, dfx_event_t stop, float *ms); /* waits for `stop` */
int dfx_event_destroy(dfx_event_t e);

/* ---- weight reorder (the reference exposes OIhw4i16o4i, deepfusion.h:59-60,
 *      but ships no reorder, deepfusion.cc:44-50).  Host-side, pure layout. ---- */
int dfx_reorder_oihw_to_blocked(const int8_t *oihw, int8_t *blocked, int O, int I,
                                int KH, int KW);
size_t dfx_blocked_offset(int o, int i, int kh, int kw, int I, int KH, int KW);

/* ---- conv: replaces op_conv<T> (src/op_conv.h:34-96, src/op_conv.cc:31-260)
 *      and jit_conv_kernel (src/jit_conv_kernel.cc:27-510) ---- */
/* validates like op_conv<T>::init_conf + jit_conv_kernel::init_conf
 * (op_conv.cc:262-365, jit_conv_kernel.cc:512-673) minus the defects of
 * SURVEY.md 8(a); picks a kernel variant. */
int dfx_conv_create(const dfx_conv_desc *desc, dfx_conv_t **out);
/* A handle lives on the device that was current (dfx_set_device) when it was created; every
 * later entry point switches to that device for the duration of the call, so one host thread can
 * drive handles on several devices. */
/* host pointers; data is copied (and repacked for the MFMA variant) into
 * device memory owned by the handle.  wei1x1/bia1x1/scales1 are ignored for an
 * unfused op; bias pointers may be NULL when the dtype is DFX_UNDEF. */
int dfx_conv_set_weights(dfx_conv_t *h, const int8_t *wei_blocked, const void *bia0,
                         const float *scales0, const int8_t *wei1x1_blocked,
                         const void *bia1, const float *scales1);
/* asynchronous: enqueues on `s`; src_dev/dst_dev are device pointers that must
 * stay valid until the stream reaches the kernel's end.  A handle may be submitted from several
 * host threads and on several streams at once: every launch works on its own copy of the
 * arguments and its own unit-queue slot.  There are 16 slots per handle: launches on one stream are
 * ordered anyway; with several streams a launch that finds its slot last used on ANOTHER stream first
 * waits, on the device, for that launch (a 17th concurrent launch queues behind the 1st); the launches made
 * while the handle had seen one stream only are covered by one event recorded when the second stream appears.  Every op is ONE
 * kernel launch (the two-launch "split:" ops of earlier versions are gone); dfx_conv_info.kernel_name names
 * the kernel, for the role-specialised one also its stage-1 requant route ("/fma", "/magic"), and says so
 * when an op runs on the scalar kernel because its dst reaches 4 GiB. */
int dfx_conv_submit(dfx_conv_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s);
/* drop-in semantics of op::submit() (deepfusion.cc:90-103): host buffers in,
 * host buffers out, synchronous (H2D, kernel, D2H, stream sync). */
int dfx_conv_submit_host(dfx_conv_t *h, const void *src_host, void *dst_host);
int dfx_conv_query(const dfx_conv_t *h, dfx_conv_info *info);
int dfx_conv_destroy(dfx_conv_t *h);

/* ---- concat: replaces op_concat<T> (src/op_concat.h:28-61, op_concat.cc:22-72)
 *      and jit_concat_kernel (src/jit_concat_kernel.cc:30-197).  create: DFX_ERR_INVALID for a non-positive
 *      size, a bad dtype, a branch whose channels are not a multiple of 16 (1-byte types) or 4 (4-byte types);
 *      DFX_ERR_UNSUPPORTED for more than 64 branches.  submit: asynchronous on `s`; every branch pointer and dst
 *      must be non-null and 16-byte aligned (DFX_ERR_INVALID otherwise, nothing is launched): the kernel moves
 *      16-byte chunks relative to them.  submit_gathered asks the same of the base pointer and of every offset.
 *      Branches may alias each other (one buffer may be given as several branches); dst must not overlap a branch.
 *      Every launch has its own copy of the arguments and submit does not write to the handle: one handle may be
 *      submitted from several host threads and on several streams at once, the launches are independent.
 *      submit_host is synchronous and stages through device buffers and a stream that the handle owns: one thread
 *      at a time per handle.  post_relu is max(0, x) in the element's own type; for f32 it is vmaxps(zero, x),
 *      the second operand wins ties and NaNs: ReLU(-0) = -0 and a NaN passes through with its bits; without
 *      post_relu every value is copied bit for bit. ---- */
int dfx_concat_create(const dfx_concat_desc *desc, dfx_concat_t **out);
int dfx_concat_submit(dfx_concat_t *h, const void *const *srcs_dev, void *dst_dev,
                      dfx_stream_t s);
int dfx_concat_submit_host(dfx_concat_t *h, const void *const *srcs_host, void *dst_host);
/* Concat of channel slices that live in one rank-major staging buffer, as left
 * by an all-gather of per-rank NHWC shards {bs,h,w,channels[r]}:
 * input r starts at byte offset offsets[r] of `gathered_dev`. */
int dfx_concat_submit_gathered(dfx_concat_t *h, const void *gathered_dev,
                               const uint64_t *offsets, void *dst_dev, dfx_stream_t s);
int dfx_concat_destroy(dfx_concat_t *h);

/* ---- pooling stage of conv+relu+pool, eltwise-sum(+relu) (see the descriptors above).
 *      pool create: DFX_ERR_INVALID for a non-positive size / window / stride, a negative padding, a bad dtype or
 *      algorithm, and for an output window that lies entirely in the padding (so pad < window on each axis).
 *      pool submit: asynchronous on `s`; src and dst must be non-null and aligned to the element size (4 bytes for
 *      f32 / s32; DFX_ERR_INVALID otherwise, nothing is launched).  When c * sizeof(element) is a multiple of 16
 *      and both pointers are 16-byte aligned the kernel moves 16 bytes per lane; otherwise it takes one element
 *      per lane, with the same results.  dst must not overlap src.
 *      f32 max pooling is vmaxps(acc, x) over the window positions inside the input, rows outer, columns inner,
 *      starting from -Inf: the second operand wins ties and NaNs.  So a NaN is the result only if it is the LAST
 *      value of its window (then with its bits), an earlier NaN is dropped, and of +0 / -0 the later one wins.
 *      f32 averages and sums are plain IEEE binary32 operations in the documented order, denormals included; a NaN
 *      that an operation PRODUCES (Inf - Inf) is the device's default NaN, not x86's.
 *      eltwise create: DFX_ERR_UNSUPPORTED for n_inputs outside 2..8, DFX_ERR_INVALID for a non-positive size or
 *      a bad dtype.  eltwise submit: asynchronous on `s`; every input and dst must be non-null and 16-byte aligned
 *      (DFX_ERR_INVALID otherwise, nothing is launched).  dst may BE one of the inputs (in place: every element is
 *      read from all inputs before it is written, by the same lane) and one buffer may be given as several
 *      inputs; a dst that overlaps an input at any other offset is undefined.  post_relu for f32 is
 *      vmaxps(zero, x) as for concat: ReLU(-0) = -0, ReLU(NaN) = NaN.
 *      Both: every launch has its own copy of the arguments and submit does not write to the handle, so one
 *      handle may be submitted from several host threads and on several streams at once. ---- */
int dfx_pool_create(const dfx_pool_desc *desc, dfx_pool_t **out);
int dfx_pool_submit(dfx_pool_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s);
int dfx_pool_destroy(dfx_pool_t *h);
int dfx_eltwise_create(const dfx_eltwise_desc *desc, dfx_eltwise_t **out);
int dfx_eltwise_submit(dfx_eltwise_t *h, const void *const *srcs_dev, void *dst_dev, dfx_stream_t s);
int dfx_eltwise_destroy(dfx_eltwise_t *h);

/* ---- activation reorder (dfx_reorder_desc above).  The descriptor is validated before anything touches the
 *      device: DFX_ERR_INVALID for a non-positive dimension, a bad format / dtype / round mode, an n_scales
 *      other than 0, 1 or src_c, a missing or non-finite scale; DFX_ERR_UNSUPPORTED for an s32 dst and for
 *      one image of 2^31 elements or more (whole tensors beyond 2^31 bytes are fine).  The scales are copied;
 *      the handle owns them and lives on the device current at create time.  submit is asynchronous on any
 *      stream, several submits of one handle may be in flight at once.  src_dev and dst_dev must be
 *      16-byte aligned (DFX_ERR_INVALID otherwise, nothing is launched): the kernels use 16-byte accesses
 *      relative to them.  No CPU fallback. ---- */
int dfx_reorder_create(const dfx_reorder_desc *desc, const float *scales_host, dfx_reorder_t **out);
int dfx_reorder_submit(dfx_reorder_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s);
int dfx_reorder_submit_host(dfx_reorder_t *h, const void *src_host, void *dst_host); /* synchronous */
int dfx_reorder_query(const dfx_reorder_t *h, dfx_reorder_info *info);
int dfx_reorder_destroy(dfx_reorder_t *h);

/* ---- concat + pointwise conv (dfx_catconv_desc above).  The descriptor is validated before anything touches a
 *      device: DFX_ERR_INVALID for a non-positive size, n_inputs outside 2..16, a branch that is not a multiple
 *      of 16 channels, a bad dtype / round mode / nscales, and whatever dfx_conv_create rejects for the
 *      equivalent pointwise conv; DFX_ERR_UNSUPPORTED only for force_path = DFX_CATCONV_FUSED on a shape outside
 *      the fused class.  On auto everything outside that class takes the two-launch path, so the op is total.
 *      set_weights: host pointers, copied; wei_blocked is {oc, ic, 1, 1} OIhw4i16o4i over the CONCATENATED ic;
 *      it may be called again (not while a submit of the handle is in flight).  submit: asynchronous on `s`;
 *      every branch pointer and dst must be non-null and 16-byte aligned (DFX_ERR_INVALID otherwise, nothing is
 *      launched); branches may alias each other; DFX_ERR_STATE before set_weights.  A handle may be submitted
 *      from several host threads and on several streams at once.  Fused path: every launch has its own copy of
 *      the arguments, launches are independent.  Two-launch path: the handle owns ONE buffer for the
 *      concatenated tensor, so its submits are SERIALISED, as the conv handle's slot ring serialises the 17th
 *      launch: submits on one stream are ordered by the stream; once the handle has seen a second stream, every
 *      submit records an event behind its conv and a submit on a stream other than the previous one's first
 *      waits, on the device, for that event (the submits made while there was one stream only are covered by
 *      one event recorded on it when the second stream appears).  The host never blocks.  A stream made
 *      elsewhere than dfx_stream_create must outlive the handles submitted on it, as for dfx_conv_submit. ---- */
int dfx_catconv_create(const dfx_catconv_desc *desc, dfx_catconv_t **out);
int dfx_catconv_set_weights(dfx_catconv_t *h, const int8_t *wei_blocked, const void *bia, const float *scales);
int dfx_catconv_submit(dfx_catconv_t *h, const void *const *srcs_dev, void *dst_dev, dfx_stream_t s);
int dfx_catconv_submit_host(dfx_catconv_t *h, const void *const *srcs_host, void *dst_host); /* synchronous */
int dfx_catconv_query(const dfx_catconv_t *h, dfx_catconv_info *info);
int dfx_catconv_destroy(dfx_catconv_t *h);

/* ---- depthwise conv (dfx_dwconv_desc above).  The descriptor is validated before anything touches a device:
 *      DFX_ERR_INVALID for a non-positive size or stride, a negative padding, a window beyond 255 x 255 (the
 *      accumulator then cannot leave s32), an output row / column whose window starts below / right of the input,
 *      a bad dtype / round mode / nscales / force_path, a tensor of 2^31 pixels or more; DFX_ERR_UNSUPPORTED only for
 *      force_path = DFX_DWCONV_WINDOW on a shape outside that class.  On auto everything outside it takes the generic
 *      path, so the op is total.  set_weights: host pointers, copied; wei is s8 {c,kh,kw}; bia has c entries of
 *      bia_dt (NULL when DFX_UNDEF); it may be called again (not while a submit of the handle is in flight) and
 *      chooses the requant route from the actual numbers: "fast" (hardware conversions) when, for every channel,
 *      bias and scale are finite and (255 * max(P, N) + |bias|) * |scale| <= 2^30 (P, N: sums of the channel's
 *      positive / negative weights' magnitudes), the round mode is nearest and DFX_NO_FAST is not set; else "exact".
 *      submit: asynchronous on `s`; src and dst must be non-null and 16-byte aligned (DFX_ERR_INVALID otherwise,
 *      nothing is launched); DFX_ERR_STATE before set_weights.  Every launch has its own copy of the arguments: one
 *      handle serves several streams and host threads at once.  No CPU fallback. ---- */
int dfx_dwconv_create(const dfx_dwconv_desc *desc, dfx_dwconv_t **out);
int dfx_dwconv_set_weights(dfx_dwconv_t *h, const int8_t *wei, const void *bia, const float *scales);
int dfx_dwconv_submit(dfx_dwconv_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s);
int dfx_dwconv_submit_host(dfx_dwconv_t *h, const void *src_host, void *dst_host); /* synchronous */
int dfx_dwconv_query(const dfx_dwconv_t *h, dfx_dwconv_info *info);
int dfx_dwconv_destroy(dfx_dwconv_t *h);

/* ---- grouped conv (dfx_gconv_desc above).  The descriptor is validated before anything touches a device:
 *      DFX_ERR_INVALID for a non-positive size or stride, a negative padding, groups < 1, ic or oc not divisible by
 *      groups, kh * kw * ic/groups > 65025 (= 255^2, the depthwise op's bound: below it the accumulator cannot leave
 *      s32), an output row / column whose window starts below / right of the input, a bad dtype / round mode /
 *      nscales / force_path, a tensor of 2^31 pixels or more; DFX_ERR_UNSUPPORTED only for force_path =
 *      DFX_GCONV_MFMA on a shape outside that class.  On auto everything outside it takes the generic path, groups = 1
 *      and groups = ic included: the op is total and delegates to no other op.  set_weights: host pointers, copied;
 *      wei is s8 {oc, ic/groups, kh, kw}; bia has oc entries of bia_dt (NULL when DFX_UNDEF); it may be called again
 *      (not while a submit of the handle is in flight) and chooses the requant route from the actual numbers: "fast"
 *      (hardware conversions) when, for every output channel, bias and scale are finite and
 *      (255 * max(P, N) + |bias|) * |scale| <= 2^30 (P, N: sums of the channel's positive / negative weights'
 *      magnitudes over its ic/groups * kh * kw taps), the round mode is nearest and DFX_NO_FAST is not set; else
 *      "exact".  The generic kernel is always exact.  submit: asynchronous on `s`; src and dst must be non-null and
 *      16-byte aligned (DFX_ERR_INVALID otherwise, nothing is launched); DFX_ERR_STATE before set_weights.  Every
 *      launch has its own copy of the arguments: one handle serves several streams and host threads at once.  No CPU
 *      fallback. ---- */
int dfx_gconv_create(const dfx_gconv_desc *desc, dfx_gconv_t **out);
int dfx_gconv_set_weights(dfx_gconv_t *h, const int8_t *wei, const void *bia, const float *scales);
int dfx_gconv_submit(dfx_gconv_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s);
int dfx_gconv_submit_host(dfx_gconv_t *h, const void *src_host, void *dst_host); /* synchronous */
int dfx_gconv_query(const dfx_gconv_t *h, dfx_gconv_info *info);
int dfx_gconv_destroy(dfx_gconv_t *h);

/* ---- first-layer conv (dfx_imgconv_desc above).  The descriptor is validated before anything touches a device:
 *      DFX_ERR_INVALID for a non-positive size or stride, ic > 4, a window beyond 255, a negative padding,
 *      kh * kw * ic > 65025, an output row / column whose window starts below / right of the input, a bad dtype / round
 *      mode / nscales / force_path, a tensor of 2^31 pixels or more; DFX_ERR_UNSUPPORTED only for force_path =
 *      DFX_IMGCONV_MFMA on a shape outside that class.  On auto everything outside it takes the generic path: the op is
 *      total and delegates to no other op.  set_weights: host pointers, copied; wei is s8 {oc, ic, kh, kw}; bia has oc
 *      entries of bia_dt (NULL when DFX_UNDEF); it may be called again (not while a submit of the handle is in flight)
 *      and chooses the requant route from the actual numbers exactly as dfx_gconv_set_weights does (one proof,
 *      requant_host.h): "fast" when, for every output channel, bias and scale are finite and
 *      (255 * max(P, N) + |bias|) * |scale| <= 2^30 over its ic * kh * kw taps, the round mode is nearest and
 *      DFX_NO_FAST is not set; else "exact".  The generic kernel is always exact.  submit: asynchronous on `s`; src and
 *      dst must be non-null, dst 16-byte aligned (DFX_ERR_INVALID otherwise, nothing is launched), src at any byte
 *      address: no thread reads outside [src, src + bs*ih*iw*ic); DFX_ERR_STATE before set_weights.  Every launch has
 *      its own copy of the arguments and submit never writes to the handle: one handle serves several streams and host
 *      threads at once.  No CPU fallback. ---- */
int dfx_imgconv_create(const dfx_imgconv_desc *desc, dfx_imgconv_t **out);
int dfx_imgconv_set_weights(dfx_imgconv_t *h, const int8_t *wei, const void *bia, const float *scales);
int dfx_imgconv_submit(dfx_imgconv_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s);
int dfx_imgconv_submit_host(dfx_imgconv_t *h, const void *src_host, void *dst_host); /* synchronous */
int dfx_imgconv_query(const dfx_imgconv_t *h, dfx_imgconv_info *info);
int dfx_imgconv_destroy(dfx_imgconv_t *h);

/* ---- transposed conv (dfx_deconv_desc above).  The descriptor is validated before anything touches a device:
 *      DFX_ERR_INVALID for a non-positive size, a window or stride outside 1 .. 255, a padding outside 0 .. k - 1,
 *      kh * kw * ic > 65025, an output size outside 1 .. (in - 1) * stride + k - pad, a bad dtype / round mode /
 *      nscales / force_path, a tensor of 2^31 pixels or more; DFX_ERR_UNSUPPORTED only for force_path =
 *      DFX_DECONV_MFMA on a shape outside that class.  The op is total and delegates to no other op.  set_weights:
 *      host pointers, copied; wei is s8 {oc, ic, kh, kw}; bia has oc entries of bia_dt (NULL when DFX_UNDEF); it may be
 *      called again (not while a submit of the handle is in flight) and chooses the requant route exactly as
 *      dfx_gconv_set_weights does (one proof, requant_host.h), from the channel's positive and negative weight sums over
 *      ALL its ic * kh * kw taps -- every output sums a subset of them, so the bound holds for each: "fast" when, for
 *      every output channel, bias and scale are finite and (255 * max(P, N) + |bias|) * |scale| <= 2^30, the round mode
 *      is nearest and DFX_NO_FAST is not set; else "exact".  The generic kernel is always exact.  submit: asynchronous
 *      on `s`; src and dst must be non-null and 16-byte aligned on the MFMA path, aligned to the element on the generic
 *      path (DFX_ERR_INVALID otherwise, nothing is launched); DFX_ERR_STATE before set_weights.  Every launch has its
 *      own copy of the arguments and submit never writes to the handle: one handle serves several streams and host
 *      threads at once.  DFX_DECONV_GRID=n (tuning switch) caps the MFMA kernel's grid.  No CPU fallback. ---- */
int dfx_deconv_create(const dfx_deconv_desc *desc, dfx_deconv_t **out);
int dfx_deconv_set_weights(dfx_deconv_t *h, const int8_t *wei, const void *bia, const float *scales);
int dfx_deconv_submit(dfx_deconv_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s);
int dfx_deconv_submit_host(dfx_deconv_t *h, const void *src_host, void *dst_host); /* synchronous */
int dfx_deconv_query(const dfx_deconv_t *h, dfx_deconv_info *info);
int dfx_deconv_destroy(dfx_deconv_t *h);

/* ---- dilated conv (dfx_dilconv_desc above).  The descriptor is validated before anything touches a device:
 *      DFX_ERR_INVALID for a non-positive size, a window, stride or dilation outside 1 .. 255, a padding outside
 *      0 .. (k - 1) * d, kh * kw * ic > 65025, an output row / column whose window starts below / right of the input, a
 *      bad dtype / round mode / nscales / force_path, a tensor of 2^31 pixels or more; DFX_ERR_UNSUPPORTED only for
 *      force_path = DFX_DILCONV_MFMA on a shape outside that class.  The op is total and delegates to no other op.
 *      set_weights: host pointers, copied; wei is s8 {oc, ic, kh, kw}; bia has oc entries of bia_dt (NULL when
 *      DFX_UNDEF); it may be called again (not while a submit of the handle is in flight) and chooses the requant route
 *      exactly as dfx_gconv_set_weights does (one proof, requant_host.h) over the channel's ic * kh * kw taps: "fast"
 *      when, for every output channel, bias and scale are finite and (255 * max(P, N) + |bias|) * |scale| <= 2^30, the
 *      round mode is nearest and DFX_NO_FAST is not set; else "exact".  The generic kernel is always exact.  submit:
 *      asynchronous on `s`; src and dst must be non-null and 16-byte aligned on the MFMA path, dst aligned to its
 *      element on the generic path (DFX_ERR_INVALID otherwise, nothing is launched); DFX_ERR_STATE before set_weights.
 *      Every launch has its own copy of the arguments and submit never writes to the handle: one handle serves several
 *      streams and host threads at once.  Tuning switches: DFX_DILCONV_GRID=n caps the MFMA kernel's grid,
 *      DFX_DILCONV_SLAB=n sets the K-steps per weight slab (clamped to what LDS holds).  No CPU fallback. ---- */
int dfx_dilconv_create(const dfx_dilconv_desc *desc, dfx_dilconv_t **out);
int dfx_dilconv_set_weights(dfx_dilconv_t *h, const int8_t *wei, const void *bia, const float *scales);
int dfx_dilconv_submit(dfx_dilconv_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s);
int dfx_dilconv_submit_host(dfx_dilconv_t *h, const void *src_host, void *dst_host); /* synchronous */
int dfx_dilconv_query(const dfx_dilconv_t *h, dfx_dilconv_info *info);
int dfx_dilconv_destroy(dfx_dilconv_t *h);

/* ---- activation resize (dfx_resize_desc above).  The descriptor is validated before anything touches a device:
 *      DFX_ERR_INVALID for a size outside 1 .. 65535, bs or c below 1, a bad dtype / algo / coord / force_path, add or
 *      post_relu other than 0 / 1, post_relu without add, src or dst of more than 2^40 elements (so that no size product
 *      leaves 64 bits); DFX_ERR_UNSUPPORTED for bilinear on s32 and for force_path =
 *      DFX_RESIZE_BAND on a shape outside that class.  "No HIP device" is reported only for a valid descriptor.
 *      submit: asynchronous on `s`; it never writes to the handle and every launch has its own copy of the arguments:
 *      one handle serves several streams and host threads at once.  src and dst must be non-null; add_dev must be
 *      non-null exactly when the descriptor has add = 1 (DFX_ERR_INVALID otherwise, nothing is launched).  Pointers
 *      aligned to the element but not to 16 bytes take the generic kernel for that submit, as pooling does; a pointer
 *      not aligned to the element, a dst range that overlaps src's, or an add range that overlaps dst's without being
 *      dst, is DFX_ERR_INVALID.  add_dev may be dst_dev.
 *      Tuning switches: DFX_RESIZE_ROWS=n sets the band length (default: 8 rows for bilinear, 2 for nearest, halved
 *      while the launch would have fewer than 512 workgroups), DFX_RESIZE_MAX_GRID=n caps the grid of either kernel.
 *      No CPU fallback. ---- */
int dfx_resize_create(const dfx_resize_desc *desc, dfx_resize_t **out);
int dfx_resize_submit(dfx_resize_t *h, const void *src_dev, const void *add_dev, void *dst_dev, dfx_stream_t s);
int dfx_resize_submit_host(dfx_resize_t *h, const void *src_host, const void *add_host, void *dst_host); /* synchronous */
int dfx_resize_query(const dfx_resize_t *h, dfx_resize_info *info);
int dfx_resize_destroy(dfx_resize_t *h);

/* ---- fully-connected layer (dfx_fc_desc above).  The descriptor is validated before anything touches a device:
 *      DFX_ERR_INVALID for a non-positive size, ih * iw * ic > 65025, bs * oc of 2^31 or more, a bad dtype / round
 *      mode / nscales / force_path; DFX_ERR_UNSUPPORTED only for force_path = DFX_FC_MFMA where K is no multiple of
 *      64.  On auto everything outside that class takes the generic path.  set_weights: host pointers, copied; wei is
 *      s8 {oc, ic, ih, iw}; bia has oc entries of bia_dt (NULL when DFX_UNDEF); it may be called again (not while a
 *      submit of the handle is in flight) and chooses the requant route from the actual numbers as
 *      dfx_gconv_set_weights does, over the K taps of a channel: "fast" when, for every output channel, bias and scale
 *      are finite and (255 * max(P, N) + |bias|) * |scale| <= 2^30, the round mode is nearest and DFX_NO_FAST is not
 *      set; else "exact".  The generic kernel is always exact.  submit: asynchronous on `s`; src and dst must be
 *      non-null and 16-byte aligned (DFX_ERR_INVALID otherwise, nothing is launched); DFX_ERR_STATE before
 *      set_weights.  MFMA path: the handle owns ONE slab of s32 partial sums [splitk][bs rounded up to 32][oc rounded
 *      up to 32] between its two launches, so its submits are SERIALISED on the device exactly as dfx_catconv's and
 *      dfx_dwpw's two-launch path (see there); the host never blocks.  The partial sums are added as integers: every
 *      splitk gives the same bits.  No CPU fallback. ---- */
int dfx_fc_create(const dfx_fc_desc *desc, dfx_fc_t **out);
int dfx_fc_set_weights(dfx_fc_t *h, const int8_t *wei, const void *bia, const float *scales);
int dfx_fc_submit(dfx_fc_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s);
int dfx_fc_submit_host(dfx_fc_t *h, const void *src_host, void *dst_host); /* synchronous */
int dfx_fc_query(const dfx_fc_t *h, dfx_fc_info *info);
int dfx_fc_destroy(dfx_fc_t *h);

/* ---- squeeze-and-excitation (dfx_se_desc above).  The descriptor is validated before anything touches a device:
 *      DFX_ERR_INVALID for a size below 1, ih * iw > 2^23, c or cr > 16384 (the accumulators stay in s32), bs * ih * iw * c
 *      of 2^40 or more, a bad mode / bias dtype / round mode / nscales1 / nscales2 / nscales_out / force_path;
 *      DFX_ERR_UNSUPPORTED only for force_path = DFX_SE_BAND outside that class.  "No HIP device" is reported only for a
 *      valid descriptor.  set_weights: host pointers, copied; w1 s8 {cr,c}, w2 s8 {c,cr}, bia1 cr entries of bia1_dt, bia2
 *      c entries of bia2_dt (NULL when DFX_UNDEF), lut 256 bytes; it may be called again (not while a submit of the handle
 *      is in flight).  submit: asynchronous on `s`; src and dst must be non-null (DFX_ERR_INVALID, nothing is launched);
 *      DFX_ERR_STATE before set_weights in DFX_SE_SCALE and DFX_SE_GATE, never in DFX_SE_SQUEEZE, which takes no weights.
 *      DFX_SE_SCALE: dst may BE src, a dst range that overlaps src's in any other way is DFX_ERR_INVALID; in the other two
 *      modes the {bs,c} result must not overlap src at all.  Pointers that are not 16-byte aligned take the generic kernels
 *      for that submit, as pooling and resize do.  The handle owns the scratch between its launches (two in DFX_SE_GATE
 *      and DFX_SE_SQUEEZE, three in DFX_SE_SCALE): the s32 slab of partial sums [bs][slices][c] and the {bs,c} gate, so its
 *      submits are SERIALISED on the device exactly as dfx_fc's MFMA path and dfx_catconv's two-launch path (see there);
 *      the host never blocks.  The partial sums are integers: every slice count gives the same bits.
 *      Tuning switches: DFX_SE_SLICES=n forces the slice count (clamped to 1 .. ih*iw; default: at least two workgroups per
 *      CU where the tensor allows it and at least 64 pixels per slice), DFX_SE_GRID=n caps the grid of every SE kernel.
 *      No CPU fallback. ---- */
int dfx_se_create(const dfx_se_desc *desc, dfx_se_t **out);
int dfx_se_set_weights(dfx_se_t *h, const int8_t *w1, const void *bia1, const float *scales1, const int8_t *w2, const void *bia2,
                       const float *scales2, const uint8_t *lut, const float *out_scales);
int dfx_se_submit(dfx_se_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s);
int dfx_se_submit_host(dfx_se_t *h, const void *src_host, void *dst_host); /* synchronous */
int dfx_se_query(const dfx_se_t *h, dfx_se_info *info);
int dfx_se_destroy(dfx_se_t *h);

/* ---- scaled element-wise sum (dfx_wsum_desc above).  The descriptor is validated before anything touches a device:
 *      DFX_ERR_INVALID for a size below 1, h * w * c of 2^31 or more, bs * h * w * c beyond 2^40, n_inputs outside 1 .. 8,
 *      a bad src / dst / table dtype, nscales[i] other than 1 or c, n_bias other than 0, 1 or c, a bad round mode /
 *      post_relu / force_path, a table with an f32 dst; DFX_ERR_UNSUPPORTED for dst_dt = DFX_S32 and for force_path =
 *      DFX_WSUM_VEC outside that class.  "No HIP device" is reported only for a valid descriptor.
 *      set_params: host pointers, copied: scales[i] points to nscales[i] floats for every i < n_inputs; bias to n_bias
 *      floats (ignored when n_bias = 0); lut to 256 bytes (ignored without a table).  A scale or bias that is not finite
 *      is DFX_ERR_INVALID.  It may be called again (not while a submit of the handle is in flight).
 *      submit: asynchronous on `s`; ONE launch; it never writes to the handle and every launch has its own copy of the
 *      arguments: one handle serves several streams and host threads at once.  DFX_ERR_STATE before set_params.
 *      srcs_dev[i] and dst must be non-null and aligned to their element.  ALIASING: dst may BE any input whose element
 *      size equals dst's (every element is read from all inputs before its lane writes it); one buffer may be given as
 *      several inputs; any other overlap of dst's range with an input's -- a 4-byte input at dst's address when dst is
 *      1-byte included -- is DFX_ERR_INVALID and nothing is launched.  Pointers that are not 16-byte aligned take the
 *      generic kernel for that submit, as resize and se do.
 *      Tuning switch: DFX_WSUM_GRID=n caps the grid of either kernel.  No CPU fallback. ---- */
int dfx_wsum_create(const dfx_wsum_desc *desc, dfx_wsum_t **out);
int dfx_wsum_set_params(dfx_wsum_t *h, const float *const *scales, const float *bias, const uint8_t *lut);
int dfx_wsum_submit(dfx_wsum_t *h, const void *const *srcs_dev, void *dst_dev, dfx_stream_t s);
int dfx_wsum_submit_host(dfx_wsum_t *h, const void *const *srcs_host, void *dst_host); /* synchronous */
int dfx_wsum_query(const dfx_wsum_t *h, dfx_wsum_info *info);
int dfx_wsum_destroy(dfx_wsum_t *h);

/* ---- net head: top-k / argmax and softmax (dfx_head_desc above).  The descriptor is validated before anything touches
 *      a device: DFX_ERR_INVALID for a bad mode / dtype / force_path, rows < 1, c outside 1 .. 65535, src_ld < c, k
 *      outside 1 .. 8 or above c, idx_ld < k, a u8 idx with c > 256, dst_ld < c, an out_scale that is not finite, more
 *      than 2^40 elements; DFX_ERR_UNSUPPORTED for softmax of a 4-byte src and for a force_path outside that path's
 *      class.  "No HIP device" is reported only for a valid descriptor.
 *      set_table (SOFTMAX only; DFX_ERR_INVALID on a TOPK handle): 256 host uint32, copied.  DFX_ERR_INVALID for
 *      E[0] == 0 (S could be 0) and for (uint64)c * max(E) > 2^32 - 1 (S could leave u32).  It may be called again (not
 *      while a submit of the handle is in flight).
 *      submit: asynchronous on `s`; ONE launch; it never writes to the handle: one handle serves several streams and host
 *      threads at once.  TOPK: idx_or_dst is idx, val_or_null is val or NULL.  SOFTMAX: idx_or_dst is dst, val_or_null
 *      must be NULL; DFX_ERR_STATE before set_table.  Pointers must be non-null (but val) and aligned to their element;
 *      an output that overlaps src or the other output is DFX_ERR_INVALID and nothing is launched.  Pointers that are
 *      not 16-byte aligned take the generic kernel for that submit.
 *      Tuning switch: DFX_HEAD_GRID=n caps the grid of any path.  No CPU fallback. ---- */
int dfx_head_create(const dfx_head_desc *desc, dfx_head_t **out);
int dfx_head_set_table(dfx_head_t *h, const uint32_t *table256);
int dfx_head_submit(dfx_head_t *h, const void *src_dev, void *idx_or_dst_dev, void *val_or_null_dev, dfx_stream_t s);
int dfx_head_query(const dfx_head_t *h, dfx_head_info *info);
int dfx_head_destroy(dfx_head_t *h);

/* ---- image-wide top-K with peak filter (dfx_select_desc above).  The descriptor is validated before anything touches
 *      a device: DFX_ERR_INVALID for sizes outside the limits stated at the descriptor, a bad dtype / peak mode /
 *      force_path, idx_ld < k, a min_val outside src's dtype, a bad gather entry; DFX_ERR_UNSUPPORTED for an s32 / f32 src
 *      and for force_path = DFX_SELECT_HIST with src_ld % 16 != 0.  "No HIP device" is reported only for a valid
 *      descriptor.
 *      submit: asynchronous on `s`.  val may be NULL; gather_src / gather_dst are arrays of n_gather device pointers (may
 *      be NULL when n_gather is 0).  DFX_ERR_INVALID, with nothing launched and every output untouched, for a null
 *      pointer, an idx or count that is not 4-byte aligned, and any output (idx, val, count, a gather destination) that
 *      overlaps src, a gather source or another output.  Pointers (src, idx, val, count, gather destinations) that are
 *      not 16-byte aligned take the generic kernel for that submit.
 *      Histogram path: the handle owns the scratch its four launches meet in (slab, plan, cand), so its submits are
 *      SERIALISED on the device, as dfx_se's: submits on one stream are ordered by the stream; once the handle has seen a
 *      second stream every submit records an event behind its last launch and a submit on another stream than the
 *      previous one's first waits for it, on the device.  The host never blocks, and submit does not write to the handle
 *      otherwise.  Generic path: one launch with its own arguments; submits are independent.
 *      Tuning switch: DFX_SELECT_CHUNK=n sets the pixels per chunk (raised until an image has at most 1024 chunks).
 *      No CPU fallback.  Auto: DFX_SELECT_AUTO_NOTE above. ---- */
int dfx_select_create(const dfx_select_desc *desc, dfx_select_t **out);
int dfx_select_submit(dfx_select_t *h, const void *src_dev, void *idx_dev, void *val_or_null_dev, void *count_dev,
                      const void *const *gather_src_dev, void *const *gather_dst_dev, dfx_stream_t s);
int dfx_select_query(const dfx_select_t *h, dfx_select_info *info);
int dfx_select_destroy(dfx_select_t *h);

/* ---- box decode + greedy NMS (dfx_nms_desc above).  The descriptor is validated before anything touches a device:
 *      DFX_ERR_INVALID for bs < 1, n outside 1 .. 4096, max_out outside 1 .. n, keep_ld < max_out, a bad mode / per_class /
 *      force_path, classes, anchors_per_pixel or n_anchors below 1, n_anchors * classes beyond 2^31 - 1, an iou_thr that is
 *      not finite, and in DECODE mode row_bytes < 4 * A, idx_ld < n (also BOXES with per_class), a clip_w or clip_h that is
 *      NaN, or clip_w > 0 without clip_h >= 0.  "No HIP device" is reported only for a valid descriptor.
 *      submit: asynchronous on `s`; every pointer of dfx_nms_io is a device pointer.  DFX_ERR_INVALID, with nothing launched
 *      and every output untouched, for a null io, a null pointer the mode needs (BOXES: boxes, and idx with per_class;
 *      DECODE: idx, deltas, anchors, tab_c, tab_s; always keep and count), an f32 / s32 pointer that is not 4-byte aligned,
 *      and any output (keep, count, boxes_out) that overlaps an input or another output.  Pointers (boxes, idx, anchors,
 *      keep, count, boxes_out) that are not 16-byte aligned take the generic kernel for that submit.
 *      Mask path: the handle owns the scratch its three launches meet in (box, lab, mask), so its submits are SERIALISED
 *      on the device exactly as dfx_select's histogram path: the host never blocks.  Generic path: one launch with its own
 *      arguments; submits are independent.  No CPU fallback.  Auto: DFX_NMS_AUTO_NOTE above. ---- */
int dfx_nms_create(const dfx_nms_desc *desc, dfx_nms_t **out);
int dfx_nms_submit(dfx_nms_t *h, const dfx_nms_io *io, dfx_stream_t s);
int dfx_nms_query(const dfx_nms_t *h, dfx_nms_info *info);
int dfx_nms_destroy(dfx_nms_t *h);

/* ---- RoIAlign (dfx_roialign_desc above).  The descriptor is validated before anything touches a device: DFX_ERR_INVALID
 *      for bs or n below 1, a bad mode / aligned / force_path, levels outside 1 .. 4, c < 1, a dtype other than u8 / s8 /
 *      f32, an h or w outside 1 .. 65535, an ld below c, a scale that is not finite and > 0, thresholds that are not finite
 *      and non-decreasing, ph or pw outside 1 .. 64, a sampling_ratio outside 0 .. 4, and a force_path of
 *      DFX_ROIALIGN_TILE outside its class; DFX_ERR_UNSUPPORTED for sampling_ratio 0 and for what the kernels' 32-bit byte
 *      offsets cannot address: dst, or any level, of 2^32 bytes or more.  "No HIP device" is reported only for a valid
 *      descriptor.
 *      submit: asynchronous on `s`; every pointer of dfx_roialign_io is a device pointer.  DFX_ERR_INVALID, with nothing
 *      launched and dst untouched, for a null io, a null level, boxes, dst, or batch_idx in LIST mode, an f32 / s32 pointer
 *      that is not 4-byte aligned, and a dst that overlaps an input.  A level, boxes or dst that is not 16-byte aligned
 *      takes the generic kernel for that submit.  One launch with its own arguments: submits are independent, from any
 *      thread on any stream.  No CPU fallback.  Auto: DFX_ROIALIGN_AUTO_NOTE above. ---- */
int dfx_roialign_create(const dfx_roialign_desc *desc, dfx_roialign_t **out);
int dfx_roialign_submit(dfx_roialign_t *h, const dfx_roialign_io *io, dfx_stream_t s);
int dfx_roialign_query(const dfx_roialign_t *h, dfx_roialign_info *info);
int dfx_roialign_destroy(dfx_roialign_t *h);

/* ---- batched int8 matrix product (dfx_bmm_desc above).  The descriptor is validated before anything touches a device, in
 *      this order: DFX_ERR_INVALID for a non-positive size, m or n above 2^31 - 32, K > 65025, a bad trans_b / dtype / round mode / nscales (1 or n) /
 *      force_path, lda < K, ldb < (trans_b ? K : N), ldc < N, a negative stride, a C whose elements could overlap -- take the
 *      (extent, stride) pairs (N,1), (M,ldc), (batch1,c_s1), (batch0,c_s0), drop extents of 1, sort by stride: the first
 *      stride must be >= 1, each further one >= the previous stride x the previous extent (this accepts the interleaved-heads layout) -- and any
 *      operand whose index range reaches 2^40 elements; then DFX_ERR_UNSUPPORTED only for a u8 B and for force_path =
 *      DFX_BMM_MFMA outside that class.  "No HIP device" is reported only for a valid descriptor.
 *      set_scales: 1 or n host floats, copied; may be called again (not while a submit of the handle is in flight); it
 *      chooses the requant route (above).  submit: asynchronous on `s`; DFX_ERR_INVALID, with nothing launched, for a null
 *      pointer, a 4-byte C that is not 4-byte aligned, and a C byte range that overlaps A's or B's; DFX_ERR_STATE before
 *      set_scales.  ONE launch with its own arguments and no scratch: submits are independent, a handle may be submitted
 *      from several host threads and on several streams at once (dfx_pool's contract, not dfx_fc's).
 *      Tuning switch: DFX_BMM_GRID=n caps the grid of either kernel.  No CPU fallback. ---- */
int dfx_bmm_create(const dfx_bmm_desc *desc, dfx_bmm_t **out);
int dfx_bmm_set_scales(dfx_bmm_t *h, const float *scales);
/* The logit bias (dfx_logit_bias_desc above).  DFX_ERR_INVALID for a period outside 1 .. its batch extent, a negative
 * stride, 0 < ld < n, a host extent of 2^40 floats or more, a null table and a +inf or NaN among the addressed entries;
 * DFX_ERR_UNSUPPORTED for a device image above 2^30 bytes; the handle is unchanged by a refused call.  The addressed entries
 * are COPIED at the call: set_scales' contract -- synchronous, not while a submit of the handle is in flight.  It may be called
 * again with another table or layout.  desc == NULL clears the bias (host_table is ignored) and the handle gives its former
 * bits.  Either order with set_scales: whichever setter comes last proves the requant route again. */
int dfx_bmm_set_bias(dfx_bmm_t *h, const dfx_logit_bias_desc *desc, const float *host_table);
int dfx_bmm_submit(dfx_bmm_t *h, const void *a_dev, const void *b_dev, void *c_dev, dfx_stream_t s);
int dfx_bmm_query(const dfx_bmm_t *h, dfx_bmm_info *info);
int dfx_bmm_destroy(dfx_bmm_t *h);

/* ---- fused int8 attention (dfx_attn_desc above).  The descriptor is validated before anything touches a device, in this
 *      order: DFX_ERR_INVALID for a non-positive size, tq or dv above 2^31 - 32, d > 65025, tk > 65025, a bad q / k / v / dst
 *      dtype / round mode / nscales (1 or dv) / force_path, a prob_scale that is not finite, ldq < d, ldk < d, ldv < dv,
 *      ldo < dv, a negative stride, an O whose elements could overlap (dfx_bmm's rule with (dv,1), (tq,ldo), (batch1,o_s1),
 *      (batch0,o_s0)), any operand whose index range reaches 2^40 elements, and logits whose G * tq * up16(tk) reach 2^40;
 *      then DFX_ERR_UNSUPPORTED only for a u8 K or V and for force_path = DFX_ATTN_FUSED outside that class.  "No HIP
 *      device" is reported only for a valid descriptor.
 *      set_table: dfx_head_set_table's checks with c = tk.  set_scales: one logit scale and 1 or dv out scales, host values,
 *      copied; it chooses both requant routes (above).  Both may be called again (not while a submit is in flight).
 *      submit: asynchronous on `s`; DFX_ERR_INVALID, with nothing launched, for a null pointer, a 4-byte O that is not 4-byte
 *      aligned and an O byte range that overlaps Q's, K's or V's; DFX_ERR_STATE before set_table and set_scales.
 *      A handle may be submitted from several host threads and on several streams at once.  Fused path: one launch with its
 *      own arguments, submits are independent.  Chain (planned, or taken for one submit because q, k or v is not 16-byte
 *      aligned): the handle owns ONE scratch for L and P -- allocated at create where the chain is the plan, at the first such
 *      submit on a fused handle (DFX_ERR_HIP from that submit if the device has no room) -- so those submits are
 *      SERIALISED as dfx_dwpw's two-launch path is: ordered by the stream on one stream; once a second stream has been seen,
 *      every chain submit records an event and a submit on a stream other than the previous one's first waits for it on
 *      the device.  The host never blocks.
 *      Tuning switch: DFX_ATTN_GRID=n caps the fused kernel's grid.  No CPU fallback. ---- */
int dfx_attn_create(const dfx_attn_desc *desc, dfx_attn_t **out);
int dfx_attn_set_table(dfx_attn_t *h, const uint32_t *table256);
int dfx_attn_set_scales(dfx_attn_t *h, float logit_scale, const float *out_scales);
/* dfx_bmm_set_bias on the logits' product (m = tq, n = tk), with its checks, its copy and its contract; it reaches the fused
 * kernel, the chain, and the chain a fused handle makes at its first submit that falls back.  desc == NULL clears it. */
int dfx_attn_set_bias(dfx_attn_t *h, const dfx_logit_bias_desc *desc, const float *host_table);
int dfx_attn_submit(dfx_attn_t *h, const void *q_dev, const void *k_dev, const void *v_dev, void *o_dev, dfx_stream_t s);
int dfx_attn_query(const dfx_attn_t *h, dfx_attn_info *info);
int dfx_attn_destroy(dfx_attn_t *h);

/* ---- int8 layer norm / RMS norm (dfx_lnorm_desc above).  The descriptor is validated before anything touches a device,
 *      in this order: DFX_ERR_INVALID for a bad mode, rows < 1, c outside 1 .. 16384, a src dtype other than u8 / s8, a dst
 *      dtype other than u8 / s8 / f32, src_ld < c, dst_ld < c, an eps that is not finite and > 0, a bad force_path, more
 *      than 2^40 elements; then DFX_ERR_UNSUPPORTED only for force_path = DFX_LNORM_ROW outside that class.  "No HIP
 *      device" is reported only for a valid descriptor.
 *      set_params: host pointers, copied to the device; gamma is c floats, beta c floats or NULL (zeros), shift c bytes or
 *      NULL (all 0); a shift above 7 is DFX_ERR_INVALID and leaves the handle as it was.  It may be called again (not
 *      while a submit of the handle is in flight).
 *      submit: asynchronous on `s`; ONE launch with its own arguments; it never writes to the handle: one handle serves
 *      several streams and host threads at once.  DFX_ERR_STATE before set_params.  DFX_ERR_INVALID, with nothing launched,
 *      for a null pointer, an f32 dst that is not 4-byte aligned and a dst that overlaps src (in place is not built: rows
 *      longer than the register budget are re-read).  Pointers that are not 16-byte aligned take the generic kernel for
 *      that submit.
 *      Tuning switch: DFX_LNORM_GRID=n caps the grid of either kernel.  No CPU fallback.  Auto: DFX_LNORM_AUTO_NOTE. ---- */
int dfx_lnorm_create(const dfx_lnorm_desc *desc, dfx_lnorm_t **out);
int dfx_lnorm_set_params(dfx_lnorm_t *h, const float *gamma, const float *beta_or_null, const uint8_t *shift_or_null);
int dfx_lnorm_submit(dfx_lnorm_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s);
int dfx_lnorm_query(const dfx_lnorm_t *h, dfx_lnorm_info *info);
int dfx_lnorm_destroy(dfx_lnorm_t *h);

/* ---- int8 token linear layer (dfx_linear_desc above).  The descriptor is validated before anything touches a device, in
 *      this order: DFX_ERR_INVALID for rows < 1, k outside 1 .. 65025, n outside 1 .. 2^31 - 128, a src dtype other than u8 /
 *      s8, a bad dst dtype, bias dtype, round mode, a scales count other than 1 or n, a lut_in_dt other than none / u8 / s8,
 *      a table with a 4-byte dst, a bad force_path, src_ld < k, dst_ld < n, rows * max(src_ld, dst_ld) > 2^40; then
 *      DFX_ERR_UNSUPPORTED only for force_path = DFX_LINEAR_TILE outside that class.  "No HIP device" is reported only for
 *      a valid descriptor.
 *      set_weights: host pointers, copied: wei s8 {n, k} row-major, bia n entries of bia_dt (NULL when DFX_UNDEF), scales
 *      nscales floats.  It packs the device image (weights in the tile's order | compensation | bias | scale | table),
 *      proves the requant route and may be called again (not while a submit of the handle is in flight).
 *      set_table: 256 host bytes, copied; DFX_ERR_INVALID on a handle created without a table.  May be called again.
 *      submit: asynchronous on `s`; ONE launch with its own arguments; it never writes to the handle: one handle serves
 *      several streams and host threads at once.  DFX_ERR_STATE, with nothing launched, before set_weights and, on a
 *      handle created with a table, before set_table.  DFX_ERR_INVALID, with nothing launched, for a null pointer, a dst
 *      that is not aligned to its element and a dst that overlaps src.  A src that is not 16-byte aligned takes the generic
 *      kernel for that submit.  submit_host: synchronous, densely packed host tensors (src {rows, k}, dst {rows, n}) only
 *      where src_ld == k and dst_ld == n (DFX_ERR_UNSUPPORTED otherwise).
 *      Tuning switches: DFX_LINEAR_GRID=n caps the grid of either kernel; DFX_LINEAR_BM=64|128 fixes the tile height.
 *      No CPU fallback.  Auto: DFX_LINEAR_AUTO_NOTE. ---- */
int dfx_linear_create(const dfx_linear_desc *desc, dfx_linear_t **out);
int dfx_linear_set_weights(dfx_linear_t *h, const int8_t *wei, const void *bia, const float *scales);
int dfx_linear_set_table(dfx_linear_t *h, const uint8_t lut[256]);
int dfx_linear_submit(dfx_linear_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s);
int dfx_linear_submit_host(dfx_linear_t *h, const void *src_host, void *dst_host); /* synchronous */
int dfx_linear_query(const dfx_linear_t *h, dfx_linear_info *info);
int dfx_linear_destroy(dfx_linear_t *h);

/* ---- int8 patch embedding (dfx_patchembed_desc above).  The descriptor is validated before anything touches a device, in
 *      this order: DFX_ERR_INVALID for bs / ih / iw / ic < 1, ph or pw outside 1 .. 255, th outside 1 .. ih / ph, tw outside
 *      1 .. iw / pw, K > 65025, oc outside 1 .. 2^31 - 128, a src dtype other than u8 / s8, a bad dst dtype, bias dtype, round
 *      mode, a scales count other than 1 or oc, table other than 0 / 1, a table together with a bias, tok_offset < 0, a bad
 *      force_path, img_rows < tok_offset + th * tw, dst_ld < oc, bs * ih * iw * ic > 2^40, ph * iw * ic >= 2^31,
 *      bs * img_rows * dst_ld > 2^40, a table image beyond 2^30 bytes; then DFX_ERR_UNSUPPORTED only for force_path =
 *      DFX_PATCHEMBED_TILE outside that class.  "No HIP device" is reported only for a valid descriptor.
 *      set_weights: host pointers, copied: wei s8 {oc, ic, ph, pw}, bia oc entries of bia_dt (NULL when DFX_UNDEF), scales
 *      nscales floats.  set_table: th * tw rows of oc floats, `ld` >= oc floats apart, copied; DFX_ERR_INVALID on a handle
 *      created without a table and for a non-finite entry.  set_prefix: tok_offset * oc elements of dst's dtype, copied;
 *      DFX_ERR_INVALID where tok_offset is 0.  Each may be called again and in any order (not while a submit of the handle is
 *      in flight); the requant route is proved again from the weights and the table the handle then holds.
 *      submit: asynchronous on `s`; ONE launch with its own arguments; it never writes to the handle: one handle serves
 *      several streams and host threads at once.  DFX_ERR_STATE, with nothing launched, before set_weights and, on a handle
 *      created with a table, before set_table.  DFX_ERR_INVALID, with nothing launched, for a null pointer, a dst that is not
 *      aligned to its element and a dst that overlaps src.  A src that is not aligned to the class's granule takes the
 *      generic kernel for that submit.  submit_host: synchronous, densely packed host tensors (src {bs, ih, iw, ic}, dst
 *      {bs * img_rows, dst_ld}); dst's bytes that the op does not write come back as the staging buffer holds them.
 *      Tuning switches: DFX_PATCHEMBED_GRID=n caps the grid of either kernel; DFX_PATCHEMBED_BM=64|128 fixes the tile height.
 *      No CPU fallback.  Auto: DFX_PATCHEMBED_AUTO_NOTE. ---- */
int dfx_patchembed_create(const dfx_patchembed_desc *desc, dfx_patchembed_t **out);
int dfx_patchembed_set_weights(dfx_patchembed_t *h, const int8_t *wei, const void *bia, const float *scales);
int dfx_patchembed_set_table(dfx_patchembed_t *h, const float *table, int64_t ld);
int dfx_patchembed_set_prefix(dfx_patchembed_t *h, const void *rows);
int dfx_patchembed_submit(dfx_patchembed_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s);
int dfx_patchembed_submit_host(dfx_patchembed_t *h, const void *src_host, void *dst_host); /* synchronous */
int dfx_patchembed_query(const dfx_patchembed_t *h, dfx_patchembed_info *info);
int dfx_patchembed_destroy(dfx_patchembed_t *h);

/* ---- window partition / reverse (dfx_window_desc above).  The descriptor is validated before anything touches a device, in
 *      this order: DFX_ERR_INVALID for a bad dir, a bad dtype, bs < 1, h or w outside 1 .. 65535, c < 1, wh or ww outside
 *      1 .. 255, a bad order, shift_y outside 0 .. hp-1, shift_x outside 0 .. wp-1, grid_ld < c, win_ld < c, a bad force_path,
 *      hp * wp > 2^22, bs * hp * wp * max(grid_ld, win_ld) > 2^40; then DFX_ERR_UNSUPPORTED only for force_path =
 *      DFX_WINDOW_ROW outside that class.  "No HIP device" is reported only for a valid descriptor.  create builds the row map
 *      on the host and uploads it.
 *      submit: src is the grid side and dst the window side for PARTITION, the other way round for REVERSE.  Asynchronous on
 *      `s`; ONE launch with its own arguments; it never writes to the handle: one handle serves several streams and host
 *      threads at once.  DFX_ERR_INVALID, with nothing launched, for a null pointer, a pointer of a 4-byte dtype that is not
 *      4-byte aligned and a dst whose extent overlaps src's (a permutation cannot run in place).  Pointers that are not 16-byte
 *      aligned take the generic kernel for that submit.
 *      Tuning switch: DFX_WINDOW_GRID=n caps the grid of either kernel.  No CPU fallback.  Auto: DFX_WINDOW_AUTO_NOTE. ---- */
int dfx_window_create(const dfx_window_desc *desc, dfx_window_t **out);
int dfx_window_submit(dfx_window_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s);
int dfx_window_query(const dfx_window_t *h, dfx_window_info *info);
int dfx_window_destroy(dfx_window_t *h);

/* ---- depthwise + pointwise conv (dfx_dwpw_desc above).  The descriptor is validated before anything touches a
 *      device: DFX_ERR_INVALID for what dfx_dwconv_create rejects for stage 0 (sizes, strides, padding, window,
 *      output size, pixel count), a non-positive oc, a bad dtype / round mode / nscales0 / nscales1 / force_path, and
 *      whatever dfx_conv_create rejects for the pointwise conv; DFX_ERR_UNSUPPORTED only for force_path =
 *      DFX_DWPW_FUSED on a shape outside the fused class.  On auto everything outside it takes the two-launch path,
 *      so the op is total over what the two ops accept.  set_weights: host pointers, copied; wei_dw is s8 {c,kh,kw}
 *      as for dfx_dwconv_set_weights, wei_pw is {oc,c,1,1} in OIhw4i16o4i as for dfx_conv_set_weights; bias pointers
 *      may be NULL when the dtype is DFX_UNDEF; it may be called again (not while a submit of the handle is in
 *      flight).  It chooses each stage's requant route from the actual numbers, independently: "fast" when, for every
 *      output channel of the stage, bias and scale are finite and (255 * max(P, N) + |bias|) * |scale| <= 2^30 (P, N:
 *      sums of the channel's positive / negative weights' magnitudes), the stage's round mode is nearest and
 *      DFX_NO_FAST is not set; else "exact" (the two-launch path: the routes of its two ops).  submit: asynchronous
 *      on `s`; src and dst must be non-null and 16-byte aligned (DFX_ERR_INVALID otherwise, nothing is launched);
 *      DFX_ERR_STATE before set_weights.  A handle may be submitted from several host threads and on several streams
 *      at once.  Fused path: every launch has its own copy of the arguments, launches are independent.  Two-launch
 *      path: the handle owns ONE buffer for the u8 tensor between the stages, so its submits are SERIALISED, as
 *      dfx_catconv's: submits on one stream are ordered by the stream; once the handle has seen a second stream, every
 *      submit records an event behind its conv and a submit on a stream other than the previous one's first waits, on
 *      the device, for that event (the submits made while there was one stream only are covered by one event recorded
 *      on it when the second stream appears).  The host never blocks.  A stream made elsewhere than dfx_stream_create
 *      must outlive the handles submitted on it.  No CPU fallback.
 *      Auto: see the AUTO RULE at DFX_DWPW_FUSED above. ---- */
int dfx_dwpw_create(const dfx_dwpw_desc *desc, dfx_dwpw_t **out);
int dfx_dwpw_set_weights(dfx_dwpw_t *h, const int8_t *wei_dw, const void *bia0, const float *scales0,
                         const int8_t *wei_pw_blocked, const void *bia1, const float *scales1);
int dfx_dwpw_submit(dfx_dwpw_t *h, const void *src_dev, void *dst_dev, dfx_stream_t s);
int dfx_dwpw_submit_host(dfx_dwpw_t *h, const void *src_host, void *dst_host); /* synchronous */
int dfx_dwpw_query(const dfx_dwpw_t *h, dfx_dwpw_info *info);
int dfx_dwpw_destroy(dfx_dwpw_t *h);

/* ---- test hooks (not part of the reference's surface; used by tests/ only) ---- */
/* Overwrites the LDS of every CU with a pattern (asynchronous, on `s`): makes a kernel that
 * reads LDS before publishing it fail deterministically (tests/test_gpu_first_launch.py). */
int dfx_debug_scribble_lds(unsigned pattern, dfx_stream_t s);
/* Sets (value != NULL) or clears a testing / tuning switch (DFX_NO_FAST,
 * DFX_FORCE_GEOM, DFX_STREAM_GRID ...).  The library reads those from the environment once, when
 * it is first used; this is how a test reaches another code path afterwards.  Affects handles
 * created after the call. */
int dfx_debug_set_tuning(const char *key, const char *value);
/* Read-only: how the host hands out the units of a resident-weight op (conv_mfma.cuh, conv_mfma_roles.cuh); launches
 * nothing.  Fills out[0 .. min(n, 13) - 1], in this order:
 *    0 th, 1 tw        unit size in output rows / columns
 *    2 linear          1: a unit spans whole rows (tw == ow); 0: column-split units
 *    3 uy, 4 ux        units per image along y / x
 *    5 total_units     ids the loaders run through (whole units + half units)
 *    6 half_from       ids >= half_from are half units; INT32_MAX: none
 *    7 static_rounds   units a loader owns before it turns to the queue
 *    8 lazy_queue      1: lazy draws (store-bound ops)
 *    9 pool            1: fused 2x2 max pooling
 *   10 teams           loader streams of one launch (grid x 2)
 *   11 roles           1: the role-specialised kernel runs the op (valid after dfx_conv_set_weights)
 *   12 ring_waits      stream waits the queue-ring guard of dfx_conv_submit has issued on this handle so far
 * DFX_ERR_UNSUPPORTED for an op without a unit queue (any other kernel). */
int dfx_debug_conv_sched(const dfx_conv_t *h, int32_t *out, int n);
/* Read-only: pixels per unit when the op runs PIXEL-RUN units (a unit = a run of that many consecutive pixels of one
 * image in row-major order, a multiple of 32; dfx_debug_conv_sched then reports th = the most rows such a run
 * touches, tw = ow, uy = units per image, ux = 1); 0 for row / column units and for every other kernel.  Launches
 * nothing. */
int dfx_debug_conv_unit_px(const dfx_conv_t *h);
/* Read-only: the requant route dfx_conv_set_weights proved for stage 0 (out[0]) and stage 1 (out[1]) from the
 * actual weights, bias and scales; launches nothing.  One numbering for every kernel family:
 *    0 exact   the reference's arithmetic step by step (x86 conversion semantics emulated)
 *    1 fast    hardware conversions, nearest-even, nothing near +-2^31
 *    2 magic   accumulator started from a float bit pattern, v_add_f32 + v_mul_f32
 *    3 fma     accumulator started from a float bit pattern, one v_fma_f32
 *   -1         the op has no such stage (out[1] of an unfused op)
 * Resident-weight kernels report their mode0 / mode1, the streamed kernel its one `fast` switch for both stages,
 * the direct-weight and pointwise kernels fast / m0 / m1, the scalar kernel 0.  dfx_debug_catconv_requant forwards
 * to the op's inner conv handle, whose proofs the fused kernel reads too.  DFX_ERR_STATE before set_weights. */
int dfx_debug_conv_requant(const dfx_conv_t *h, int32_t out[2]);
int dfx_debug_catconv_requant(const dfx_catconv_t *h, int32_t out[2]);
/* the depthwise conv's one stage, same numbering (0 exact, 1 fast) */
int dfx_debug_dwconv_requant(const dfx_dwconv_t *h, int32_t out[1]);
/* the grouped conv's one stage, same numbering (0 exact, 1 fast) */
int dfx_debug_gconv_requant(const dfx_gconv_t *h, int32_t out[1]);
/* the first-layer conv's one stage, same numbering (0 exact, 1 fast) */
int dfx_debug_imgconv_requant(const dfx_imgconv_t *h, int32_t out[1]);
/* the transposed conv's one stage, same numbering (0 exact, 1 fast) */
int dfx_debug_deconv_requant(const dfx_deconv_t *h, int32_t out[1]);
/* the dilated conv's one stage, same numbering (0 exact, 1 fast) */
int dfx_debug_dilconv_requant(const dfx_dilconv_t *h, int32_t out[1]);
/* the fully-connected op's one stage, same numbering (0 exact, 1 fast) */
int dfx_debug_fc_requant(const dfx_fc_t *h, int32_t out[1]);
/* the depthwise + pointwise op's two stages {route0, route1}, same numbering; on the two-launch path the routes of
 * the owned depthwise and conv handles */
int dfx_debug_dwpw_requant(const dfx_dwpw_t *h, int32_t out[2]);
/* Read-only: how many dfx_resize_submit calls of this process have launched the band kernel (out[DFX_RESIZE_BAND]) and
 * the generic kernel (out[DFX_RESIZE_GENERIC]) so far.  Process-wide, since submit does not write to the handle; it is
 * how a test sees the per-submit fallback of 16-byte-misaligned pointers, which dfx_resize_query does not report. */
int dfx_debug_resize_launches(int64_t out[2]);
/* the same for dfx_wsum_submit: out[DFX_WSUM_VEC], out[DFX_WSUM_GENERIC] */
int dfx_debug_wsum_launches(int64_t out[2]);
/* the same for dfx_head_submit: out[DFX_HEAD_PIXEL], out[DFX_HEAD_ROW], out[DFX_HEAD_GENERIC] */
int dfx_debug_head_launches(int64_t out[3]);
/* the same for dfx_select_submit: out[DFX_SELECT_HIST], out[DFX_SELECT_GENERIC] (a submit counts once, whatever the
 * number of its launches) */
int dfx_debug_select_launches(int64_t out[2]);
/* the same for dfx_nms_submit: out[DFX_NMS_MASK], out[DFX_NMS_GENERIC] */
int dfx_debug_nms_launches(int64_t out[2]);
/* the same for dfx_roialign_submit: out[DFX_ROIALIGN_TILE], out[DFX_ROIALIGN_GENERIC] */
int dfx_debug_roialign_launches(int64_t out[2]);
/* the same for dfx_bmm_submit: out[DFX_BMM_MFMA], out[DFX_BMM_GENERIC] */
int dfx_debug_bmm_launches(int64_t out[2]);
/* the matrix product's one stage as the last dfx_bmm_set_scales proved it, same numbering (0 exact, 1 fast; the generic
 * path is always exact).  DFX_ERR_STATE before set_scales. */
int dfx_debug_bmm_requant(const dfx_bmm_t *h, int32_t out[1]);
/* the same for dfx_attn_submit: out[DFX_ATTN_FUSED], out[DFX_ATTN_CHAIN] (a chain submit counts once) */
int dfx_debug_attn_launches(int64_t out[2]);
/* the same for dfx_lnorm_submit: out[DFX_LNORM_ROW], out[DFX_LNORM_GENERIC] */
int dfx_debug_lnorm_launches(int64_t out[2]);
/* the same for dfx_linear_submit: out[DFX_LINEAR_TILE], out[DFX_LINEAR_GENERIC] */
int dfx_debug_linear_launches(int64_t out[2]);
/* the token linear op's one stage as the last dfx_linear_set_weights proved it, same numbering (0 exact, 1 fast; the generic
 * path is always exact).  DFX_ERR_STATE before set_weights. */
int dfx_debug_linear_requant(const dfx_linear_t *h, int32_t out[1]);
/* the same for dfx_patchembed_submit: out[DFX_PATCHEMBED_TILE], out[DFX_PATCHEMBED_GENERIC] */
int dfx_debug_patchembed_launches(int64_t out[2]);
/* the patch embedding's one stage as the handle's weights and table prove it now, same numbering (0 exact, 1 fast; the generic
 * path is always exact).  DFX_ERR_STATE before set_weights. */
int dfx_debug_patchembed_requant(const dfx_patchembed_t *h, int32_t out[1]);
/* the same for dfx_window_submit: out[DFX_WINDOW_ROW], out[DFX_WINDOW_GENERIC] */
int dfx_debug_window_launches(int64_t out[2]);

#ifdef __cplusplus
}
#endif
#endif
