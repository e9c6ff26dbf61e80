// deepfusion.h -- drop-in C++ API of the MI355X (gfx950) build of deep-fusion.
//
// Source-compatible with the public header of the reference
// (/root/reference/include/deepfusion.h): the same namespace, element typedefs,
// `round_mode`, `memory` (formats, dtypes, both constructors, accessors) and the
// same `op::submit()`, `concat()` and two `conv()` entry points with identical
// parameter lists and defaults, so callers such as the reference's
// test/test_concat.cc:89-108 or benchmark/bench_concat.cc:124-161 compile
// unchanged.  Behind it the Xbyak JIT kernels are replaced by HIP kernels reached
// through the C ABI of include/dfx.h.
//
// Host/device coherence (the reference has one address space; this build has two):
//   * memory::data() still returns a HOST pointer that callers read and write
//     directly.  The buffer is pinned host memory.
//   * submit() has the reference's semantics: the caller's host buffers are re-read on EVERY
//     call.  Inputs are uploaded every time (also when the caller refilled them through a
//     pointer fetched once, without calling data() again), borrowed weight / bias tensors are
//     hashed and re-packed when their bytes changed; then ONE kernel is launched, the
//     destination downloaded and the stream synchronised: after submit() returns,
//     dst->data() holds the result, exactly like the reference's synchronous OpenMP
//     execution (deepfusion.cc:90-103).  The one exception: an input whose device copy was
//     written by another op's submit_async() and that nobody has touched through data()
//     since is NOT uploaded -- its host bytes are the stale side.
//   * Extensions for device-resident pipelines (not in the reference):
//     op::submit_async() skips the download and the synchronisation and trusts the
//     per-tensor data() counters instead of re-reading host memory (every call of data()
//     marks the tensor "host-dirty": it is uploaded / its weights are re-packed by the next
//     submit_async()); memory::device_data() exposes the device buffer; memory::download() /
//     op::wait() complete a transfer explicitly.  With DEEPFUSION_PROFILE=1 every submit,
//     submit_async() included, waits for its launch (it prints the launch's duration).
//     Every op runs on a stream of its own, and the library orders the streams on the device:
//     an op waits for the op that wrote its input, and for every op that still reads, or last
//     wrote, the tensor it is about to overwrite.  So ops may be chained, tensors may have
//     several consumers, an op may update a tensor in place, and several frames may be in flight
//     (for frame: a->submit_async(); b->submit_async();) without a wait() in between; ops may be
//     destroyed while their launch is in flight.  Two rules are the caller's:
//       - wait() (on the op that consumed the tensor) before rewriting host bytes which an
//         earlier submit_async() uploaded: the upload reads the host buffer asynchronously;
//       - under DEEPFUSION_DEVICES > 1 (batch shards: host in, host out on per-shard streams,
//         no ordering between ops) a consumer needs the producer's wait() first.
//
// Lifetime rule kept from the reference (op_conv.h:81-95, op_concat.h:53-56):
// an op borrows the tensors it was built from; they must outlive it.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <array>
#include <memory>
#include <vector>

namespace deepfusion {

typedef float f32;
typedef int32_t s32;
typedef int8_t s8;
typedef uint8_t u8;

// kept for source compatibility with code that uses the reference's macro
#ifndef DISABLE_COPY_AND_ASSIGN
#define DISABLE_COPY_AND_ASSIGN(classname)          \
private:                                            \
  classname(const classname &) = delete;            \
  classname(const classname &&) = delete;           \
  classname &operator=(const classname &) = delete; \
  classname &operator=(const classname &&) = delete
#endif

struct opdesc {  // placeholder type of the reference API (deepfusion.h:42-44), unused
  int tmp;
};

// rounding of the f32 -> integer conversion of a requantisation stage
enum round_mode {
  nearest = 0,  // ties to even (vcvtps2dq rn-sae)
  down,         // toward -inf  (vcvtps2dq rd-sae)
};

namespace detail {
struct memory_state;  // pinned host buffer, lazily created device buffer, dirty flags
struct op_state;
}  // namespace detail

struct memory {
public:
  // physical layouts.  nhwc: activations.  OIhw4i16o4i: s8 weights blocked as
  // [O/16][I/16][kh][kw][(i%16)/4][o%16][i%4] (see dfx_reorder_oihw_to_blocked in
  // dfx.h and reorder_weights() below).  x: 1-D (bias).
  enum format {
    format_undef = 0,
    x,
    nchw,
    oihw = nchw,
    nhwc,
    OIhw4i16o4i,
    gOIhw4i16o4i,
  };
  typedef std::vector<int> dims;
  typedef std::array<int, 2> pair_dims;
  typedef std::array<int, 4> nchw_dims;

  enum dtype {
    undef = 0,
    f32,
    s32,
    s8,
    u8,
  };

  // logical nchw / oihw dims; the physical order follows `fmt`
  explicit memory(const nchw_dims &dm, const format fmt, const dtype dt, int alignment = 4096);
  // physical dims as given (used for format x)
  explicit memory(const dims &dm, const format fmt, const dtype dt, int alignment = 4096);
  ~memory();

  size_t size();         // number of elements
  size_t buffer_size();  // bytes
  dims actual_dims() { return dims_; }
  nchw_dims std_dims() { return std_dims_; }  // nchw or oihw
  dtype data_type() { return dt_; }
  format dim_format() { return fmt_; }
  void *data();  // host pointer; marks the tensor host-dirty

  // ---- extensions of this build ----
  const void *host_data() const;  // host pointer without marking it dirty
  void *device_data();            // device buffer (allocated on first use)
  void upload();                  // host -> device now (clears host-dirty)
  void download();                // device -> host now, synchronous
  unsigned long long host_version() const;  // incremented by every data() call

private:
  friend struct detail::op_state;
  void allocate_buffer(int alignment);
  detail::memory_state *st_;
  dims dims_;
  nchw_dims std_dims_;
  format fmt_;
  dtype dt_;

  DISABLE_COPY_AND_ASSIGN(memory);
};

class op {
public:
  explicit op() {}
  virtual ~op() {}
  // synchronous, like the reference: upload dirty inputs, run, download dst, wait
  virtual void submit();
  // extension: enqueue only (inputs uploaded if dirty); result stays on the device
  virtual void submit_async();
  // extension: block until everything this op enqueued has finished
  virtual void wait();

protected:
  virtual void infer() = 0;
  virtual const char *name() = 0;
  DISABLE_COPY_AND_ASSIGN(op);
};

// channel concat of nhwc tensors with optional ReLU (reference deepfusion.h:116-118)
std::unique_ptr<op> concat(const std::vector<std::unique_ptr<memory>> &srcs,
                           std::unique_ptr<memory> &dst,
                           bool post_relu = false);

// convolution only (reference deepfusion.h:121-129)
std::unique_ptr<op> conv(const std::unique_ptr<memory> &src,
                         const std::unique_ptr<memory> &wei,
                         const std::unique_ptr<memory> &bia,
                         std::array<int, 2> sz_stride,
                         std::array<int, 2> sz_padding,
                         std::unique_ptr<memory> &dst,
                         bool conv0_relu = false,
                         std::vector<float> conv0_scales = {1.f},
                         round_mode conv0_round_mode = round_mode::nearest);

// convolution fused with relu + 1x1 convolution (+relu) (reference deepfusion.h:132-145)
std::unique_ptr<op> conv(const std::unique_ptr<memory> &src,
                         const std::unique_ptr<memory> &wei,
                         const std::unique_ptr<memory> &bia,
                         std::array<int, 2> sz_stride,
                         std::array<int, 2> sz_padding,
                         const std::unique_ptr<memory> &wei1x1,
                         const std::unique_ptr<memory> &bia1x1,
                         std::unique_ptr<memory> &dst,
                         bool conv0_relu = false,
                         std::vector<float> conv0_scales = {1.f},
                         round_mode conv0_round_mode = round_mode::nearest,
                         bool conv1_relu = false,
                         std::vector<float> conv1_scales = {1.f},
                         round_mode conv1_round_mode = round_mode::nearest);

// ---- the reference's roadmap ops (README.md:64-65), which it never shipped.  Signature after the
// planned one in test/test_conv_relu_pooling.cc:264-281; semantics of the MKL-DNN pipeline that test
// builds (:30-235): conv (+bias, scale, round) -> relu -> max pooling whose padding takes no part.
// `dst` carries the pooled dims; the conv output dims follow from src / wei / stride / padding. ----
enum class pool_algo {  // the reference test's max_pooling / pooling_avg_* flags (test_conv_relu_pooling.cc:189-193)
  max = 0,
  avg_include_padding,
  avg_exclude_padding,
};
std::unique_ptr<op> conv_relu_pool(const std::unique_ptr<memory> &src,
                                   const std::unique_ptr<memory> &wei,
                                   const std::unique_ptr<memory> &bia,
                                   std::array<int, 2> conv_stride,
                                   std::array<int, 2> conv_padding,
                                   std::array<int, 2> pool_kernel,
                                   std::array<int, 2> pool_stride,
                                   std::array<int, 2> pool_padding,
                                   std::unique_ptr<memory> &dst,
                                   bool conv_relu = true,
                                   std::vector<float> conv_scales = {1.f},
                                   round_mode conv_round_mode = round_mode::nearest,
                                   pool_algo algo = pool_algo::max);

// dst = relu?(saturate(sum of srcs)): same shape, format and dtype everywhere; integer sums are
// exact and saturate to the dtype's range, f32 sums run left to right (README.md:65, the "shortcut
// sum" of test_conv_relu_pooling.cc:118-124)
std::unique_ptr<op> eltwise_sum(const std::vector<std::unique_ptr<memory>> &srcs,
                                std::unique_ptr<memory> &dst,
                                bool post_relu = true);

// ---- extension: activation reorder on the device -- layout (nchw <-> nhwc), dtype and scale conversion with
// channel padding / cropping (dfx_reorder_* in dfx.h; the reference's tests use MKL-DNN's reorder for this,
// parity unpinned).  For every channel k of dst: k < src channels ? cvt(float(src) * scale[k]) : 0, where cvt
// for u8 / s8 rounds (ties to even, or down), maps NaN to 0 and saturates the value; f32 stores the product.
// src: f32 | s32 | s8 | u8, dst: f32 | u8 | s8, each nchw or nhwc; channel counts come from std_dims()[1] and
// may differ (dst wider: zero channels are appended; narrower: the rest is dropped); batch, height and width
// must match.  scales: none (1.0f), one, or one per source channel. ----
std::unique_ptr<op> reorder(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> &dst,
                            const std::vector<float> &scales = {}, round_mode rm = round_mode::nearest);

// ---- extension: channel concat + pointwise (1x1, stride 1, unpadded) conv in ONE launch (dfx_catconv_* in dfx.h): the
// join of an Inception module, a DenseNet bottleneck or a SqueezeNet squeeze layer.  The conv reads the nhwc u8
// branches in place; the concatenated tensor is never written.  dst holds, bit for bit, what concat(srcs, tmp) followed
// by conv(tmp, wei, bia, {1,1}, {0,0}, dst, relu, scales, rm) produces (ReLU on u8 branches is the identity, so a
// post_relu concat is covered too).  wei: OIhw4i16o4i {oc, sum of the branches' channels, 1, 1}; every branch a multiple
// of 16 channels.  Shapes outside the one-launch kernel's class (dfx.h, DFX_CATCONV_FUSED) run as two launches behind
// the same call.  submit / submit_async / wait behave like conv's; borrowed weights are hashed and re-packed like
// conv's.  Under DEEPFUSION_DEVICES the batch is sharded as conv() and concat() shard it (all tensors are batch-major:
// a shard is an offset into every branch); the bytes are the same either way. ----
std::unique_ptr<op> concat_conv(const std::vector<std::unique_ptr<memory>> &srcs,   // nhwc u8
                                const std::unique_ptr<memory> &wei,
                                const std::unique_ptr<memory> &bia,
                                std::unique_ptr<memory> &dst,
                                bool relu = false, std::vector<float> scales = {1.f},
                                round_mode rm = round_mode::nearest);

// ---- extension: depthwise conv (dfx_dwconv_* in dfx.h): every channel is convolved with its own window -- the other
// half of a MobileNet / EfficientNet / Xception block (the reference asserts ngroups == 1).  src: nhwc u8; wei: plain
// oihw s8 of dims {c, 1, kh, kw}; bia: format x, c entries, or null; dst: nhwc u8 / s8 / s32 / f32 with src's batch and
// channels -- ITS height and width are the output size, so windows may hang over the bottom / right edge (TF "SAME"
// padding of a stride-2 layer with padding {0, 0}); padding is {top, left}.  Arithmetic, scales, ReLU and rounding are
// conv()'s: for c a multiple of 16 dst holds, bit for bit, what conv() gives with block-diagonal weights.  3x3 / 5x5
// windows with stride 1 / 2 and c % 16 == 0 run on the sliding-window kernel, everything else on a generic one.
// submit / submit_async / wait behave like conv's; borrowed weights are hashed and re-packed like conv's; under
// DEEPFUSION_DEVICES the batch is sharded as concat_conv() shards it. ----
std::unique_ptr<op> depthwise_conv(const std::unique_ptr<memory> &src,
                                   const std::unique_ptr<memory> &wei,
                                   const std::unique_ptr<memory> &bia,
                                   std::array<int, 2> sz_stride,
                                   std::array<int, 2> sz_padding,
                                   std::unique_ptr<memory> &dst,
                                   bool relu = false, std::vector<float> scales = {1.f},
                                   round_mode rm = round_mode::nearest);

// ---- extension: grouped conv (dfx_gconv_* in dfx.h), 1 <= groups <= ic: output channel o reads only the ic / groups
// input channels of its group o / (oc / groups) -- the 3x3 of a ResNeXt / RegNet block (the reference asserts
// ngroups == 1).  src: nhwc u8; wei: plain oihw s8 of dims {oc, ic / groups, kh, kw}; bia: format x, oc entries, or
// null; dst: nhwc u8 / s8 / s32 / f32 with src's batch and oc channels -- ITS height and width are the output size, as
// for depthwise_conv(); padding is {top, left}.  Arithmetic, scales, ReLU and rounding are conv()'s: where ic and oc are
// multiples of 16 and the output size is conv()'s, dst holds, bit for bit, what conv() gives with block-diagonal
// weights.  3x3 windows with stride 1 / 2, ic == oc a multiple of 32 and ic / groups in {4, 8, 16, 32, 64} run on an
// int8-MFMA kernel that does the groups' work only, everything else on a generic one.  submit / submit_async / wait,
// weight hashing and DEEPFUSION_DEVICES sharding are depthwise_conv()'s. ----
std::unique_ptr<op> grouped_conv(const std::unique_ptr<memory> &src,
                                 const std::unique_ptr<memory> &wei,
                                 const std::unique_ptr<memory> &bia,
                                 int groups,
                                 std::array<int, 2> sz_stride,
                                 std::array<int, 2> sz_padding,
                                 std::unique_ptr<memory> &dst,
                                 bool relu = false, std::vector<float> scales = {1.f},
                                 round_mode rm = round_mode::nearest);

// ---- extension: first-layer conv over a 1- to 4-channel image (dfx_imgconv_* in dfx.h): conv1 of ResNet / VGG /
// MobileNet / Inception, which conv() cannot take without a reorder() that pads the image to 16 channels first.  src:
// nhwc u8 with 1 to 4 channels, as it is; wei: plain oihw s8 of dims {oc, ic, kh, kw}; bia: format x, oc entries, or
// null; dst: nhwc u8 / s8 / s32 / f32 with src's batch and any oc -- ITS height and width are the output size, as for
// grouped_conv(); padding is {top, left}.  Arithmetic, scales, ReLU and rounding are conv()'s: dst holds, bit for bit,
// what grouped_conv() with groups = 1 gives and, where oc is a multiple of 16 and the output size is conv()'s, what
// conv() gives on the image zero-padded to 16 channels.  3 or 4 channels with 7x7 / 2, 3x3 / 1 or 3x3 / 2 windows and
// oc in {32, 64, 96, 128} run on an int8-MFMA kernel in one launch, everything else on a generic one.  submit /
// submit_async / wait, weight hashing and DEEPFUSION_DEVICES sharding are depthwise_conv()'s. ----
std::unique_ptr<op> image_conv(const std::unique_ptr<memory> &src,
                               const std::unique_ptr<memory> &wei,
                               const std::unique_ptr<memory> &bia,
                               std::array<int, 2> sz_stride,
                               std::array<int, 2> sz_padding,
                               std::unique_ptr<memory> &dst,
                               bool relu = false, std::vector<float> scales = {1.f},
                               round_mode rm = round_mode::nearest);

// ---- extension: int8 transposed conv ("deconvolution", dfx_deconv_* in dfx.h): the up-conv of U-Net / FPN decoders, pose
// and CenterNet heads, DCGAN generators and the Mask R-CNN mask head.  src: nhwc u8; wei: plain oihw s8 of dims
// {oc, ic, kh, kw} (oneDNN's logical order; PyTorch's ConvTranspose2d.weight is {ic, oc, kh, kw}); bia: format x, oc
// entries, or null; dst: nhwc u8 / s8 / s32 / f32 with src's batch -- ITS height and width are the output size, at most
// (in - 1) * stride + k - pad (this covers output_padding and cropping), as for image_conv(); padding is {top, left}, at
// most k - 1.  Arithmetic, scales, ReLU and rounding are conv()'s: dst holds, bit for bit, what grouped_conv() with
// groups = 1, stride 1 and padding k - 1 - pad gives on the zero-stuffed tensor with the spatially flipped weights.
// Which shapes run on the sub-pixel int8-MFMA kernel and which on the generic one: DFX_DECONV_MFMA in dfx.h.  submit /
// submit_async / wait, weight hashing and DEEPFUSION_DEVICES sharding are depthwise_conv()'s. ----
std::unique_ptr<op> deconvolution(const std::unique_ptr<memory> &src,
                                  const std::unique_ptr<memory> &wei,
                                  const std::unique_ptr<memory> &bia,
                                  std::array<int, 2> sz_stride,
                                  std::array<int, 2> sz_padding,
                                  std::unique_ptr<memory> &dst,
                                  bool relu = false, std::vector<float> scales = {1.f},
                                  round_mode rm = round_mode::nearest);

// ---- extension: int8 dilated ("atrous") conv (dfx_dilconv_* in dfx.h): the 3x3 of a DeepLab ASPP branch, of a dilated
// ResNet's res4 / res5, of PSPNet / RFBNet context modules.  src: nhwc u8; wei: plain oihw s8 of dims {oc, ic, kh, kw};
// bia: format x, oc entries, or null; dst: nhwc u8 / s8 / s32 / f32 with src's batch -- ITS height and width are the
// output size, as for grouped_conv(); dilation is {dh, dw}, 1 = none; padding is {top, left}, at most (k - 1) * dilation.
// Arithmetic, scales, ReLU and rounding are conv()'s: dst holds, bit for bit, what grouped_conv() with groups = 1 gives
// on the zero-stuffed ((k - 1) * d + 1)^2 window -- where that window can be expressed at all (window * ic <= 65025) --
// at 1 / ((k - 1) d + 1)^2 * k^2 of its MACs and weight bytes.  Which shapes run on the K-slabbed int8-MFMA kernel and
// which on the generic one: DFX_DILCONV_MFMA in dfx.h.  submit / submit_async / wait, weight hashing and
// DEEPFUSION_DEVICES sharding are depthwise_conv()'s. ----
std::unique_ptr<op> dilated_conv(const std::unique_ptr<memory> &src,
                                 const std::unique_ptr<memory> &wei,
                                 const std::unique_ptr<memory> &bia,
                                 std::array<int, 2> sz_stride,
                                 std::array<int, 2> sz_dilation,
                                 std::array<int, 2> sz_padding,
                                 std::unique_ptr<memory> &dst,
                                 bool relu = false, std::vector<float> scales = {1.f},
                                 round_mode rm = round_mode::nearest);

// ---- extension: activation resize (dfx_resize_* in dfx.h): nearest or bilinear interpolation of an nhwc feature map to
// dst's height and width -- FPN's nearest x2, DeepLab's and PSPNet's bilinear upsampling, bilinear U-Net decoders.  src
// and dst: nhwc of one dtype (u8 / s8 / f32; s32 with nearest only) with the same batch and channels.  The index and
// weight arithmetic is dfx.h's, exact integers per axis and separately rounded f32 operations; u8 / s8 results are
// rounded to nearest even.  resize_add() adds `lateral` (dst's dims and dtype; it may BE dst) in the same launch with
// eltwise_sum()'s arithmetic: dst holds, bit for bit, what resize() followed by eltwise_sum({resized, lateral}) gives.
// submit / submit_async / wait and DEEPFUSION_DEVICES sharding over the batch are depthwise_conv()'s. ----
enum class resize_algo { nearest = 0, bilinear };
enum class resize_coord {
  half_pixel = 0,  // PyTorch align_corners=False / 'nearest-exact'
  align_corners,
  asymmetric,      // PyTorch's legacy 'nearest', Caffe / TF1
};
std::unique_ptr<op> resize(const std::unique_ptr<memory> &src, std::unique_ptr<memory> &dst,
                           resize_algo algo = resize_algo::bilinear, resize_coord coord = resize_coord::half_pixel);
std::unique_ptr<op> resize_add(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> &lateral,
                               std::unique_ptr<memory> &dst, resize_algo algo = resize_algo::nearest,
                               resize_coord coord = resize_coord::asymmetric, bool post_relu = false);

// ---- extension: fully-connected (inner product) layer (dfx_fc_* in dfx.h): the classifier head of ResNet / VGG /
// MobileNet, which conv() cannot express where oc is no multiple of 16 (the 1000-class heads).  src: nhwc u8
// {bs, c, h, w}, exactly as the previous conv or pool op left it (h = w = 1: a plain vector); wei: plain oihw s8 of dims
// {oc, c, h, w}, the flattened-CHW order frameworks keep (the library permutes it to src's order when it packs); bia:
// format x, oc entries, or null; dst: nhwc u8 / s8 / s32 / f32 of dims {bs, oc, 1, 1}, any oc >= 1.  c * h * w <= 65025.
// Arithmetic, scales, ReLU and rounding are conv()'s: where c and oc are multiples of 16, dst holds, bit for bit, what
// conv() gives with a window of the whole image.  c * h * w a multiple of 64 runs on a split-K int8-MFMA kernel,
// everything else on a generic one.  submit / submit_async / wait, weight hashing and DEEPFUSION_DEVICES sharding are
// depthwise_conv()'s. ----
std::unique_ptr<op> inner_product(const std::unique_ptr<memory> &src,
                                  const std::unique_ptr<memory> &wei,
                                  const std::unique_ptr<memory> &bia,
                                  std::unique_ptr<memory> &dst,
                                  bool relu = false, std::vector<float> scales = {1.f},
                                  round_mode rm = round_mode::nearest);

// ---- extension: squeeze-and-excitation (dfx_se_* in dfx.h), the gate between the depthwise (or grouped) conv and the
// projecting 1x1 conv of an EfficientNet / MobileNetV3 / SENet / RegNetY block: global average over the image, FC1
// (ReLU, u8), FC2 (s8), a 256-entry table that turns the requantised logit t into the gate (gate_table[t + 128]: the
// caller's sigmoid, hard-sigmoid, ...), and dst = src * gate * out_scale per (image, channel).  src and dst: nhwc u8 of
// the same dims; dst may BE src.  wei1: plain oihw s8 {cr, c, 1, 1}; wei2: plain oihw s8 {c, cr, 1, 1}; biases: format x
// with cr / c entries, or null.  scales1: 1 or cr, scales2 and out_scales: 1 or c entries.  The arithmetic is dfx.h's:
// the average is avg pooling's, the two layers are inner_product()'s, every f32 step is rounded separately.  c a multiple
// of 16 runs on 16-byte kernels, everything else on generic ones.  global_avg_pool() is the op's first stage alone: dst
// {bs, c, 1, 1} u8 holds what avg pooling with the window of the image gives, at any image size -- the layer in front of
// a classifier's inner_product().  submit / submit_async / wait, weight hashing and DEEPFUSION_DEVICES sharding are
// depthwise_conv()'s. ----
std::unique_ptr<op> squeeze_excite(const std::unique_ptr<memory> &src,
                                   const std::unique_ptr<memory> &wei1,
                                   const std::unique_ptr<memory> &bia1,
                                   const std::unique_ptr<memory> &wei2,
                                   const std::unique_ptr<memory> &bia2,
                                   const std::array<u8, 256> &gate_table,
                                   std::unique_ptr<memory> &dst,
                                   std::vector<float> scales1 = {1.f}, std::vector<float> scales2 = {1.f},
                                   std::vector<float> out_scales = {1.f / 255.f},
                                   round_mode rm = round_mode::nearest);
std::unique_ptr<op> global_avg_pool(const std::unique_ptr<memory> &src, std::unique_ptr<memory> &dst);

// ---- extension: scaled element-wise sum (dfx_wsum_* in dfx.h): the join of branches that do not share one quantisation
// step -- the ResNet shortcut, a MobileNetV2 / EfficientNet linear bottleneck, a quantised FPN level add, a conv's s32 / f32
// result added to a u8 tensor -- in ONE launch, where eltwise_sum() (one dtype, no scale) needs a reorder() per branch
// first and rounds twice.  srcs: 1 to 8 nhwc tensors of dst's dims, each u8 / s8 / s32 / f32 on its own; scales: one
// vector per src with 1 or c entries; bias: none, 1 or c floats (zero points, folded constants); dst: nhwc u8 / s8 / f32.
// dst = cvt(relu?(sum_i float(src_i) * scale_i[k] + bias[k])), every multiply and add a separately rounded f32 operation,
// left to right; cvt is reorder()'s conversion.  With a 256-entry `table` (table_in = u8 or s8: the type the value is
// converted to first; index t or t + 128, squeeze_excite()'s convention) the table's byte is stored instead: swish,
// h-swish or any other activation of a 1-byte tensor is scaled_sum({x}, {{s}}, y, {}, false, table, dtype::s8).  dst may BE
// any src of its own element size (in place: the op orders itself behind earlier readers of that tensor), and one tensor
// may be given as several srcs.  c a multiple of 16 runs on a 16-byte kernel, everything else on a generic one.  submit /
// submit_async / wait and DEEPFUSION_DEVICES sharding over the batch are depthwise_conv()'s. ----
std::unique_ptr<op> scaled_sum(const std::vector<std::unique_ptr<memory>> &srcs,
                               const std::vector<std::vector<float>> &scales,
                               std::unique_ptr<memory> &dst,
                               const std::vector<float> &bias = {}, bool post_relu = false,
                               const std::vector<u8> &table = {},
                               memory::dtype table_in = memory::dtype::undef,
                               round_mode rm = round_mode::nearest);

// ---- extension: the net head (dfx_head_* in dfx.h): what turns the last layer's logits into the answer without leaving
// the device.  src: an nhwc tensor {bs, C, h, w} of u8 / s8 / s32 / f32 -- a classifier's inner_product() dst {bs, oc, 1, 1}
// or a segmentation net's resize()d logits; every pixel is a row of C channels of which the first c_valid take part
// (c_valid = 0: all; DeepLab's 21 logits padded to 32 are read in place with c_valid = 21, whatever the pad channels hold).
//   argmax(src, dst_idx)              dst_idx {bs, 1, h, w} s32, or u8 for c_valid <= 256: 1 byte per pixel instead of C
//   top_k(src, dst_idx, dst_val, k)   k in 1 .. 8: dst_idx {bs, k, h, w}; dst_val (may be null) of idx's dims and src's dtype:
//                                     the k largest elements, value descending, the lower channel first among equal values;
//                                     f32 orders by IEEE totalOrder (-NaN < -Inf < -0 < +0 < +Inf < +NaN); bits verbatim
//   softmax(src, table, dst)          u8 / s8 src only (reorder() s32 / f32 logits to 1 byte first); dst {bs, C', h, w} f32 or
//                                     u8, C' >= c_valid.  The kernel does not write the channels from c_valid on; submit()
//                                     and download() copy the whole tensor back, so on the HOST those pad channels are
//                                     UNDEFINED afterwards (they hold what dst's device copy held).  No exp runs anywhere:
//                                     `table` is E[d] = floor(exp(-d * s) * floor((2^32 - 1) / c_valid)) for the logits'
//                                     quantisation step s, indexed by the distance d from the row maximum; p = float(E[d]) /
//                                     float(sum of the row's E), one correctly rounded division; u8 dst: rint(p * out_scale)
//                                     clamped to [0, 255].  A table with E[0] = 0 or c_valid * max(E) > 2^32 - 1 is refused.
// Bit-exact and the same on every kernel path.  submit / submit_async / wait and DEEPFUSION_DEVICES sharding over the batch
// are scaled_sum()'s. ----
std::unique_ptr<op> argmax(const std::unique_ptr<memory> &src, std::unique_ptr<memory> &dst_idx, int c_valid = 0);
std::unique_ptr<op> top_k(const std::unique_ptr<memory> &src, std::unique_ptr<memory> &dst_idx, memory *dst_val /* may be null */,
                          int k, int c_valid = 0);
std::unique_ptr<op> softmax(const std::unique_ptr<memory> &src, const std::array<uint32_t, 256> &table,
                            std::unique_ptr<memory> &dst, float out_scale = 255.f, int c_valid = 0);

// ---- extension: int8 layer norm / RMS norm (dfx_lnorm_* in dfx.h): the normalisation in front of every attention and every
// MLP of a transformer block, so that inner_product() -> attention() -> scaled_sum() chains never leave the device.  src: an
// nhwc tensor {bs, C, h, w} of u8 / s8; every pixel (token) is a row of C channels of which the first c_valid take part
// (c_valid = 0: all), c_valid <= 16384.  dst {bs, C', h, w} of u8 / s8 / f32, C' >= c_valid.  Per row, with t_k = x_k <<
// shifts[k] (shifts: empty, or c_valid values of 0 .. 7, FQ-ViT's power-of-two factors), the sums S = sum t_k and Q = sum t_k^2
// are exact integers and everything behind them is one separately rounded f32 operation per step (dfx.h states the
// sequence):  layer: y_k = (c t_k - S) * a * gamma[k] + beta[k] with a = 1 / sqrt((c Q - S^2) / c^2 + eps) / c;
// rms: y_k = t_k * a * gamma[k] + beta[k] with a = 1 / sqrt(Q / c + eps).  u8 / s8 dst: reorder()'s conversion of y_k.
// eps is in units of the integer domain (eps_real / in_scale^2) and the output scale is folded into gamma and beta by the
// caller.  beta may be empty (zeros).  dst must not be src.  Bit-exact and the same on every kernel path.  c_valid, the
// pad channels of dst (UNDEFINED on the host afterwards), submit / submit_async / wait and DEEPFUSION_DEVICES sharding over
// the batch are softmax()'s.  Not built: s32 / f32 sources, in place, a fused residual add, group / instance norm, mean /
// rstd as outputs. ----
enum class norm_mode { layer = 0, rms = 1 };
std::unique_ptr<op> layer_norm(const std::unique_ptr<memory> &src, const std::vector<float> &gamma,
                               const std::vector<float> &beta, std::unique_ptr<memory> &dst, float eps,
                               norm_mode mode = norm_mode::layer, const std::vector<u8> &shifts = {}, int c_valid = 0);

// ---- extension: int8 token linear layer (dfx_linear_* in dfx.h): the weight multiplies of a transformer block -- QKV and output
// projection, fc1 (+ GELU through a byte table) and fc2 -- between layer_norm(), attention() and scaled_sum().  src: an nhwc
// tensor {bs, C, h, w} of u8 / s8; every pixel (token) is a row of C channels of which the first k_valid take part (0: all),
// as layer_norm() reads them: attention()'s head-interleaved context is read in place.  wei: plain oihw s8 {n, k, 1, 1} (an
// nn.Linear weight), k <= 65025; bia: format x, n entries, or null; scales: 1 or n.  dst: nhwc {bs, C', h, w} of u8 / s8 / s32
// / f32 with C' >= n; the kernel does not write the channels from n on (UNDEFINED on the host afterwards, as softmax()'s).
// Arithmetic, scales, ReLU and rounding are inner_product()'s.  table (256 bytes, or empty) with table_in = u8 / s8: the
// requant produces the byte t it would store into a table_in dst and the op stores table[t] (u8) or table[t + 128] (s8)
// instead, as scaled_sum() does; dst must then be u8 or s8 and ReLU follows relu / table_in.  dst must not be src.  Bit-exact
// and the same on every kernel path.  Weight hashing and submit / submit_async / wait are inner_product()'s; the op runs on
// ONE device (DEEPFUSION_DEVICES does not shard it).  Not built: a fused residual add (scaled_sum() joins the residual),
// split-K, s32 / f32 sources, u8 weights, a fused layer norm in front. ----
std::unique_ptr<op> linear(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> &wei,
                           const std::unique_ptr<memory> &bia, std::unique_ptr<memory> &dst,
                           bool relu = false, std::vector<float> scales = {1.f}, round_mode rm = round_mode::nearest,
                           int k_valid = 0, const std::vector<u8> &table = {},
                           memory::dtype table_in = memory::dtype::undef);

// ---- extension: int8 patch embedding (dfx_patchembed_* in dfx.h): the non-overlapping convolution (window == stride) that a ViT /
// DeiT / Swin / ConvNeXt / PVT starts or downsamples with, as one matrix product that writes the tokens layer_norm(), linear()
// and attention() consume.  src: nhwc u8 / s8 {bs, ic, ih, iw}, any ic; wei: plain oihw s8 {oc, ic, ph, pw}: the window, which
// is the stride, 1 .. 255 each way with ph * pw * ic <= 65025; th = ih / ph by tw = iw / pw patches per image, pixels beyond them
// are not read.  dst: nhwc {bs, C', H, W} of u8 / s8 / s32 / f32 read as bs * H * W rows of C' >= oc channels: token ty * tw + tx of
// an image is its row tok_offset + ty * tw + tx, and H * W >= tok_offset + th * tw.  bia: format x, oc entries, or null.  table:
// empty, or th * tw * oc floats in accumulator units added per (token, channel) in the bias's place (conv bias + position
// embedding; bia must then be null).  prefix: empty, or tok_offset * oc elements of dst's type (class / distillation / register
// tokens, already quantised), stored into rows 0 .. tok_offset-1 of every image by the same launch.  What the kernel does not
// write -- channels from oc on, rows behind the tokens, rows in front of them without a prefix -- is UNDEFINED on the host
// afterwards, as linear()'s pad channels.  Arithmetic, scales, ReLU and rounding are image_conv()'s: without table and prefix,
// with tok_offset 0 and C' = oc, dst holds bit for bit what image_conv() with stride = window and no padding gives.  Weight
// hashing, submit / submit_async / wait and DEEPFUSION_DEVICES sharding over the batch are depthwise_conv()'s; table and prefix
// are copied at construction. ----
std::unique_ptr<op> patch_embed(const std::unique_ptr<memory> &src, const std::unique_ptr<memory> &wei,
                                const std::unique_ptr<memory> &bia, std::unique_ptr<memory> &dst,
                                bool relu = false, std::vector<float> scales = {1.f}, round_mode rm = round_mode::nearest,
                                const std::vector<float> &table = {}, int tok_offset = 0,
                                const std::vector<u8> &prefix = {});

// ---- extension: window partition / reverse of a token grid (dfx_window_* in dfx.h): what a Swin block needs around its
// attention(), and the gather of Swin's patch merging.  grid: an nhwc tensor {bs, C, h, w} of any of the four data types, every
// pixel a token of C channels of which the first c_valid take part (0: all of the narrower tensor).  windows: an nhwc tensor
// {bs, C', H, W} of the same data type with H * W = hp * wp, hp = ceil(h / wh) * wh, wp = ceil(w / ww) * ww, read as bs * nW * wh *
// ww rows of C' channels: window (wy, wx) of an image is its matrix wy * (wp / ww) + wx, in-window token (iy, ix) its row iy * ww
// + ix, or ix * wh + iy with col_major (patch merging's x0, x1, x2, x3 order: a 2 x 2 col_major partition into C' = C reads as one
// row of 4 C per window).  Official Swin's mapping: pad to hp x wp, roll by (-shift_y, -shift_x), cut; window_partition() fills
// the pad tokens with pad_value (a 32-bit pattern, its low byte for u8 / s8), window_reverse() is the exact inverse and reads
// no pad token.  Bytes are moved, never converted; channels from c_valid on are neither read nor written (UNDEFINED on the
// host afterwards, as layer_norm()'s pad channels).  src must not be dst.  submit / submit_async / wait and
// DEEPFUSION_DEVICES sharding over the batch are patch_embed()'s.  Not built: a fused residual add on reverse, nchw, data
// type conversion, overlapping windows. ----
struct window_shape {
  int wh, ww;
  int shift_y, shift_x;
  bool col_major;
};
std::unique_ptr<op> window_partition(const std::unique_ptr<memory> &grid, std::unique_ptr<memory> &windows,
                                     window_shape shape, uint32_t pad_value = 0, int c_valid = 0);
std::unique_ptr<op> window_reverse(const std::unique_ptr<memory> &windows, std::unique_ptr<memory> &grid,
                                   window_shape shape, int c_valid = 0);

// ---- extension: batched int8 matrix product of two DEVICE tensors (dfx_bmm_* in dfx.h): the multiply whose second operand is
// not a weight -- Q.K^T and P.V of an attention / non-local block, a correlation layer.  a (u8 / s8), b (s8) and c (u8 / s8 /
// s32 / f32) are tensors of any dims; `shape` says where the matrices lie in them, in ELEMENTS from each tensor's first:
// element (g = b0 * batch1 + b1, row, col) of A is at b0 * a_s0 + b1 * a_s1 + row * lda + col, likewise for B and C.
//   trans_b: B is {n, k} (Q.K^T);  else B is {k, n} (P.V)
//   c = store(relu?(float(sum_k a * b) * scale[n or 0]))   inner_product()'s arithmetic without a bias; scales: 1 or n floats
// attention_strides(bs, heads, t, d) gives {s0, s1, ld} of the per-head {t, d} matrices of an nhwc {bs, heads * d, t, 1}
// tensor, so that the heads are read, and the context is written back interleaved, without a copy.  Pad columns (k .. lda-1
// of A, behind B's valid columns) never take part and elements n .. ldc-1 of a row of c are not written: softmax()'s dst with
// C' = 48 for 37 tokens is `a` as it stands.  Every operand's last matrix must lie within its tensor, the last row of a and of b up to
// its valid columns rounded up to 16; c's elements must not overlap one another, a or b.  Bit-exact and the same on every kernel
// path.  submit / submit_async / wait are softmax()'s; the op runs on ONE device (DEEPFUSION_DEVICES does not shard it: its
// operands need not be batch-major), and like roi_align() it sends nothing to the host but on submit().
// ON THE HOST the elements of c that the op does not write -- n .. ldc-1 of a row, whatever lies between the matrices -- are
// UNDEFINED after submit() / download(): the kernel leaves them alone in c's DEVICE copy, which is not refreshed from the host
// before the op runs, and the whole tensor is copied back (softmax()'s pad channels behave the same).  Bytes that an earlier
// op wrote into the same device copy -- other heads of an interleaved context -- are kept. ----
struct matmul_shape {
  int batch0, batch1, m, n, k;
  bool trans_b;
  long long a_s0, a_s1, lda, b_s0, b_s1, ldb, c_s0, c_s1, ldc;
};
std::array<long long, 3> attention_strides(int bs, int heads, int t, int d, long long ld = 0 /* heads * d */);
std::unique_ptr<op> matmul(const std::unique_ptr<memory> &a, const std::unique_ptr<memory> &b, std::unique_ptr<memory> &c,
                           const matmul_shape &shape, const std::vector<float> &scales, bool relu = false,
                           round_mode rm = round_mode::nearest);
// A LOGIT BIAS (dfx_logit_bias_desc in dfx.h): c = store(relu?((float(sum_k a * b) + bias(g, row, col)) * scale[n or 0])), one
// separately rounded f32 add before the multiply, so the values are in ACCUMULATOR units; finite or -inf (a mask: an s8 c stores
// -128).  Matrix (b0, b1) uses table (b0 % period0, b1 % period1); table (p0, p1) row m col n is table[p0 * s0 + p1 * s1 + m * ld
// + n], in floats; ld == 0: one row, broadcast over m.  `table` must hold every float the layout addresses; it is copied when
// the op is made.  What dfx.h says about a mask behind a softmax holds: the masked logit is -128, no less.
struct logit_bias {
  std::vector<float> table;
  int period0, period1;
  long long s0, s1, ld;
};
std::unique_ptr<op> matmul(const std::unique_ptr<memory> &a, const std::unique_ptr<memory> &b, std::unique_ptr<memory> &c,
                           const matmul_shape &shape, const std::vector<float> &scales, const logit_bias &bias, bool relu = false,
                           round_mode rm = round_mode::nearest);

// ---- extension: fused int8 attention (dfx_attn_* in dfx.h): o[g] = requant(softmax(requant(q[g] . k[g]^T)) . v[g]) over
// batch0 * batch1 matrices that lie anywhere in four tensors, DEFINED as matmul() (s8 logits, scale logit_scale) -> softmax()
// (u8, table, prob_scale) -> matmul() (out_scales: 1 or dv floats, relu) and bit-identical to that chain; the library keeps the
// logits and the probabilities on chip where its fused kernel serves the shape (dfx.h, DFX_ATTN_AUTO_NOTE) and runs the three
// ops behind the one handle elsewhere.  q u8 or s8, k and v s8, o any of the four dtypes.  Strides are in ELEMENTS with
// matmul_shape's meaning; attention_strides() gives them for head-sliced nhwc tensors.  What holds for matmul()'s pad
// columns, for the bytes of o that the op does not write and for the extent of every operand within its tensor holds here.
// Runs on ONE device (DEEPFUSION_DEVICES does not shard it), like matmul(). ----
struct attention_shape {
  int batch0, batch1, tq, tk, d, dv;
  long long q_s0, q_s1, ldq, k_s0, k_s1, ldk, v_s0, v_s1, ldv, o_s0, o_s1, ldo;
};
std::unique_ptr<op> attention(const std::unique_ptr<memory> &q, const std::unique_ptr<memory> &k, const std::unique_ptr<memory> &v,
                              const std::array<uint32_t, 256> &table, std::unique_ptr<memory> &o, const attention_shape &shape,
                              float logit_scale, const std::vector<float> &out_scales, float prob_scale = 255.f, bool relu = false,
                              round_mode rm = round_mode::nearest);
// the same with matmul()'s logit_bias on the logits (m = tq, n = tk): a relative-position table per head, a shifted-window
// mask, a key-padding row, a causal mask.  A fully masked row is uniform over all tk keys (dfx.h).
std::unique_ptr<op> attention(const std::unique_ptr<memory> &q, const std::unique_ptr<memory> &k, const std::unique_ptr<memory> &v,
                              const std::array<uint32_t, 256> &table, std::unique_ptr<memory> &o, const attention_shape &shape,
                              float logit_scale, const std::vector<float> &out_scales, const logit_bias &bias, float prob_scale = 255.f,
                              bool relu = false, round_mode rm = round_mode::nearest);

// ---- extension: image-wide top-K with peak filter (dfx_select_* in dfx.h): what a detector does behind its last conv,
// without leaving the device.  src: an nhwc score tensor {bs, C, h, w} of u8 / s8 (a conv()'s heat map); the first c_valid
// channels of a pixel take part (0: all).  Per image, the k (1 .. 4096) best elements that are >= min_val and, with peak3,
// >= their 3x3 neighbours of the same channel inside the image (CenterNet's max_pool == heat), ordered by value descending,
// element index e = (y * w + x) * c_valid + channel ascending:
//   dst_idx    s32 {bs, k, 1, 1}: the e's, -1 from the image's count on
//   dst_val    may be null; src's dtype, idx's dims: the elements themselves, 0 from the count on
//   dst_count  s32 {bs, 1, 1, 1}: min(k, candidates)
//   gather_src / gather_dst   up to four pairs: source nhwc {bs, Ci, h, w} of any dtype (wh / offset maps, box deltas),
//              destination nhwc {bs, Ci, k, 1} of the same dtype: the whole pixel row of every selected element, zero rows
//              from the count on
// Bit-exact and the same on every kernel path.  submit / submit_async / wait are scaled_sum()'s; DEEPFUSION_DEVICES does
// not shard this op.  s32 / f32 scores and k > 4096 are not built; NMS and box decoding: box_nms() below. ----
enum { select_all_values = -2147483647 - 1 };  // min_val: the dtype's minimum, every element passes
std::unique_ptr<op> select_top_k(const std::unique_ptr<memory> &src, std::unique_ptr<memory> &dst_idx, memory *dst_val /* may be null */,
                                 std::unique_ptr<memory> &dst_count, int k, bool peak3 = false, int min_val = select_all_values,
                                 int c_valid = 0, const std::vector<memory *> &gather_src = std::vector<memory *>(),
                                 const std::vector<memory *> &gather_dst = std::vector<memory *>());

// ---- extension: box decode + greedy NMS (dfx_nms_* in dfx.h): the steps between select_top_k() and a detector's answer,
// without leaving the device.  Per image, n <= 4096 candidates in priority order (position 0 best: what select_top_k()
// emits; scores are never looked at), standard greedy suppression by IoU > iou_thr, at most max_out survivors.
//   dst_keep   s32 {bs, max_out, 1, 1}: the kept positions ascending, -1 from the count on
//   dst_count  s32 {bs, 1, 1, 1}
//   dst_boxes  may be null; f32 nhwc {bs, 4, max_out, 1}: the kept boxes (x1, y1, x2, y2), zeros from the count on
//   count_in   may be null; s32 {bs, 1, 1, 1}: select_top_k()'s dst_count -- positions from it on do not exist
// First form: boxes f32 nhwc {bs, 4, n, 1}; classes > 0 makes it per class with label = idx % classes (idx s32 {bs, n, 1, 1}
// is then required), classes = 0 class-agnostic (idx is not read).
// Second form: the boxes are decoded on the device from idx (select_top_k()'s dst_idx over a score map of
// anchors_per_pixel * classes channels), deltas (its gather destination of the 1-byte delta map, nhwc {bs, C >= 4 A, n, 1}),
// anchors f32 nhwc {n_anchors, 4, 1, 1} and two tables indexed by the raw delta byte (dx / wx -> tab_c, exp(min(dw / ww,
// clip)) -> tab_s): torchvision's BoxCoder.decode_single; clip_w > 0 clips to the image like clip_boxes_to_image.
// Bit-exact and the same on every kernel path.  submit / submit_async / wait are select_top_k()'s; DEEPFUSION_DEVICES does
// not shard this op.  Min-size filtering, soft-NMS, rotated boxes and n > 4096 are not built. ----
std::unique_ptr<op> box_nms(const std::unique_ptr<memory> &boxes, memory *idx /* may be null */, memory *count_in /* may be null */,
                            std::unique_ptr<memory> &dst_keep, std::unique_ptr<memory> &dst_count, memory *dst_boxes /* may be null */,
                            float iou_thr, int classes = 0);
std::unique_ptr<op> box_nms(const std::unique_ptr<memory> &idx, const std::unique_ptr<memory> &deltas, const std::unique_ptr<memory> &anchors,
                            const std::array<float, 256> &tab_c, const std::array<float, 256> &tab_s, memory *count_in /* may be null */,
                            std::unique_ptr<memory> &dst_keep, std::unique_ptr<memory> &dst_count, memory *dst_boxes /* may be null */,
                            float iou_thr, int classes, bool per_class, int anchors_per_pixel, float clip_w = 0.f, float clip_h = 0.f);

// ---- extension: RoIAlign (dfx_roialign_* in dfx.h): the step between box_nms() and a two-stage detector's heads
// (inner_product() over 7 x 7 tiles, conv() / deconvolution() over 14 x 14 ones), without leaving the device: torchvision's
// roi_align forward with every f32 step rounded separately in a fixed order.
//   levels          1 .. 4 nhwc tensors {bs, C, h_l, w_l} of one dtype (u8, s8, f32); the first c_valid channels take part (0: all)
//   spatial_scales  one per level; level_area_thr: levels - 1 thresholds on (x2 - x1) * (y2 - y1), non-decreasing -- the
//                   level of a RoI is the number of thresholds its area reaches (torchvision's LevelMapper squared: dfx.h)
//   boxes           batch_idx null: f32 nhwc {bs, 4, n, 1}, box_nms()'s dst_boxes, with count (may be null; s32 {bs, 1, 1, 1},
//                   box_nms()'s dst_count): RoI j of image r reads image r, rows from the count on are zeros.
//                   batch_idx given (s32 {R, 1, 1, 1}): boxes f32 nhwc {R, 4, 1, 1}, row i reads image batch_idx[i]; an index
//                   outside [0, bs) gives a row of zeros; count must be null.
//   dst             nhwc {R, C, ph, pw} of the levels' dtype, R = bs * n or R; its height and width are the bin counts (1 .. 64)
// Bit-exact and the same on every kernel path.  submit / submit_async / wait are box_nms()'s; DEEPFUSION_DEVICES does not
// shard this op, as it does not shard select_top_k().  Adaptive sampling (sampling_ratio 0), RoIPool / max mode, rotated
// RoIs, NCHW, position-sensitive pooling and u8 -> f32 output are not built. ----
std::unique_ptr<op> roi_align(const std::vector<memory *> &levels, const std::vector<float> &spatial_scales,
                              const std::vector<float> &level_area_thr, memory *boxes, memory *count /* may be null */,
                              memory *batch_idx /* null: batched */, std::unique_ptr<memory> &dst, int sampling_ratio = 2,
                              bool aligned = false, int c_valid = 0);

// ---- extension: depthwise conv + pointwise conv, the depthwise-separable block (dfx_dwpw_* in dfx.h).  Stage 0 is
// depthwise_conv() with a u8 result (ReLU implied), stage 1 a 1x1 stride-1 unpadded conv() on that tensor; dst holds,
// bit for bit, what the two ops give one after the other.  wei_dw: plain oihw s8 {c, 1, kh, kw}; wei_pw: OIhw4i16o4i
// {oc, c, 1, 1}; biases: format x or null; dst: nhwc {bs, oc, oh, ow}, its height and width are the output size.
// `relu` is stage 1's.  3x3 windows with stride 1 / 2, c % 32 == 0, c <= 256, oc 64 / 128 / 256 and c * oc <= 64 KB
// are the class of a ONE-launch kernel that keeps the u8 tensor in LDS (dfx.h, DFX_DWPW_FUSED); this call leaves the
// path to the library's auto rule, which today takes two launches for every shape (the kernel is not timed yet).  submit / submit_async / wait, weight hashing and DEEPFUSION_DEVICES sharding are
// depthwise_conv()'s. ----
std::unique_ptr<op> depthwise_separable_conv(const std::unique_ptr<memory> &src,
                                             const std::unique_ptr<memory> &wei_dw,
                                             const std::unique_ptr<memory> &bia_dw,
                                             std::array<int, 2> sz_stride,
                                             std::array<int, 2> sz_padding,
                                             const std::unique_ptr<memory> &wei_pw,
                                             const std::unique_ptr<memory> &bia_pw,
                                             std::unique_ptr<memory> &dst,
                                             bool relu = false, std::vector<float> scales_dw = {1.f},
                                             std::vector<float> scales_pw = {1.f},
                                             round_mode rm_dw = round_mode::nearest,
                                             round_mode rm_pw = round_mode::nearest);

// ---- extension: the weight reorder the reference never shipped (deepfusion.cc:44-50) ----
// Writes plain oihw s8 weights into `blocked` (an OIhw4i16o4i memory of the same
// logical dims) in the [O/16][I/16][kh][kw][4i][16o][4i] byte order.
void reorder_weights(const s8 *oihw, const std::unique_ptr<memory> &blocked);

}  // namespace deepfusion
