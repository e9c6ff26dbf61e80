"""ctypes binding of include/dfx.h (the drop-in C ABI).  Plumbing, not product."""
import collections
import ctypes
import os
import re
import subprocess

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG)
_LIB = os.environ.get("DFX_LIB_PATH") or os.path.join(_PKG, "libdfx_hip.so")  # override: debugging only
_HEADER = os.path.join(_ROOT, "include", "dfx.h")

DFX_UNDEF, DFX_F32, DFX_S32, DFX_S8, DFX_U8 = 0, 1, 2, 3, 4
ROUND_NEAREST, ROUND_DOWN = 0, 1
FMT_NHWC, FMT_NCHW = 0, 1
REORDER_FLAT, REORDER_GENERIC, REORDER_SMALLC, REORDER_TRANSPOSE = 0, 1, 2, 3
CATCONV_AUTO, CATCONV_FUSED, CATCONV_TWO_LAUNCH = -1, 0, 1
DWCONV_AUTO, DWCONV_WINDOW, DWCONV_GENERIC = -1, 0, 1
GCONV_AUTO, GCONV_MFMA, GCONV_GENERIC = -1, 0, 1
IMGCONV_AUTO, IMGCONV_MFMA, IMGCONV_GENERIC = -1, 0, 1
DECONV_AUTO, DECONV_MFMA, DECONV_GENERIC = -1, 0, 1
DILCONV_AUTO, DILCONV_MFMA, DILCONV_GENERIC = -1, 0, 1
DWPW_AUTO, DWPW_FUSED, DWPW_TWO_LAUNCH = -1, 0, 1
RESIZE_AUTO, RESIZE_BAND, RESIZE_GENERIC = -1, 0, 1
RESIZE_NEAREST, RESIZE_BILINEAR = 0, 1
COORD_HALF_PIXEL, COORD_ALIGN_CORNERS, COORD_ASYMMETRIC = 0, 1, 2
FC_AUTO, FC_MFMA, FC_GENERIC = -1, 0, 1
SE_AUTO, SE_BAND, SE_GENERIC = -1, 0, 1
SE_SCALE, SE_GATE, SE_SQUEEZE = 0, 1, 2
WSUM_AUTO, WSUM_VEC, WSUM_GENERIC = -1, 0, 1
WSUM_MAX_INPUTS = 8
HEAD_TOPK, HEAD_SOFTMAX = 0, 1
HEAD_AUTO, HEAD_PIXEL, HEAD_ROW, HEAD_GENERIC = -1, 0, 1, 2
SELECT_ALL, SELECT_PEAK3 = 0, 1
SELECT_AUTO, SELECT_HIST, SELECT_GENERIC = -1, 0, 1
SELECT_MAX_K, SELECT_MAX_GATHER = 4096, 4
NMS_BOXES, NMS_DECODE = 0, 1
NMS_AUTO, NMS_MASK, NMS_GENERIC = -1, 0, 1
NMS_MAX_N = 4096
ROI_BATCHED, ROI_LIST = 0, 1
ROIALIGN_AUTO, ROIALIGN_TILE, ROIALIGN_GENERIC = -1, 0, 1
BMM_AUTO, BMM_MFMA, BMM_GENERIC = -1, 0, 1
ATTN_AUTO, ATTN_FUSED, ATTN_CHAIN = -1, 0, 1
LNORM_LAYER, LNORM_RMS = 0, 1
LNORM_AUTO, LNORM_ROW, LNORM_GENERIC = -1, 0, 1
LNORM_MAX_C, LNORM_MAX_SHIFT = 16384, 7
LINEAR_AUTO, LINEAR_TILE, LINEAR_GENERIC = -1, 0, 1
PATCHEMBED_AUTO, PATCHEMBED_TILE, PATCHEMBED_GENERIC = -1, 0, 1
WINDOW_PARTITION, WINDOW_REVERSE = 0, 1
WINDOW_ROW_MAJOR, WINDOW_COL_MAJOR = 0, 1
WINDOW_AUTO, WINDOW_ROW, WINDOW_GENERIC = -1, 0, 1
WINDOW_MAX_HW, WINDOW_MAX_WIN, WINDOW_MAX_PADDED = 65535, 255, 1 << 22
VARIANT_GENERIC, VARIANT_MFMA_FUSED, VARIANT_MFMA_CONV, VARIANT_MFMA_STREAM = 0, 1, 2, 3
_NP = {DFX_F32: np.float32, DFX_S32: np.int32, DFX_S8: np.int8, DFX_U8: np.uint8}
_DT = {np.dtype(np.float32): DFX_F32, np.dtype(np.int32): DFX_S32,
       np.dtype(np.int8): DFX_S8, np.dtype(np.uint8): DFX_U8}


class DfxError(RuntimeError):
    pass


class ConvDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "bs", "ic", "ih", "iw", "oc", "oh", "ow", "kh", "kw", "sh", "sw", "pad_t", "pad_l",
        "oc1x1", "dst_dt", "bia0_dt", "bia1_dt", "conv0_relu", "conv1_relu",
        "conv0_round_mode", "conv1_round_mode", "conv0_nscales", "conv1_nscales",
        "force_variant", "fuse_pool")]


class ConvInfo(ctypes.Structure):
    _fields_ = [("variant", ctypes.c_int32), ("grid", ctypes.c_int32), ("block", ctypes.c_int32),
                ("lds_bytes", ctypes.c_int32), ("rows_per_unit", ctypes.c_int32),
                ("device", ctypes.c_int32), ("algorithmic_ops", ctypes.c_uint64),
                ("algorithmic_bytes", ctypes.c_uint64), ("kernel_name", ctypes.c_char * 96)]


class ConcatDesc(ctypes.Structure):
    _fields_ = [("n_inputs", ctypes.c_int32), ("bs", ctypes.c_int32), ("h", ctypes.c_int32),
                ("w", ctypes.c_int32), ("dt", ctypes.c_int32), ("post_relu", ctypes.c_int32),
                ("channels", ctypes.POINTER(ctypes.c_int32))]


class PoolDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("bs", "c", "ih", "iw", "oh", "ow", "kh", "kw", "sh", "sw",
                                             "pad_t", "pad_l", "dt", "algo")]


class EltwiseDesc(ctypes.Structure):
    _fields_ = [("n_inputs", ctypes.c_int32), ("elems", ctypes.c_int64), ("dt", ctypes.c_int32),
                ("post_relu", ctypes.c_int32)]


class ReorderDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("bs", "h", "w", "src_c", "dst_c", "src_fmt", "dst_fmt", "src_dt",
                                             "dst_dt", "round_mode", "n_scales")]


class ReorderInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("path", "grid", "block", "lds_bytes", "device", "tile_pixels",
                                             "channel_block", "vec_plane", "vec_pixel")] + \
               [("algorithmic_bytes", ctypes.c_uint64), ("kernel_name", ctypes.c_char * 96)]


class CatConvDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("n_inputs", "bs", "h", "w", "oc", "dst_dt", "bia_dt", "relu", "round_mode",
                                             "nscales", "force_path")] + \
               [("channels", ctypes.POINTER(ctypes.c_int32))]


class CatConvInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("path", "grid", "block", "lds_bytes", "device")] + \
               [("algorithmic_ops", ctypes.c_uint64), ("algorithmic_bytes", ctypes.c_uint64),
                ("kernel_name", ctypes.c_char * 96)]


class DwConvDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("bs", "c", "ih", "iw", "oh", "ow", "kh", "kw", "sh", "sw", "pad_t", "pad_l",
                                             "dst_dt", "bia_dt", "relu", "round_mode", "nscales", "force_path")]


class DwConvInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("path", "grid", "block", "lds_bytes", "device")] + \
               [("algorithmic_ops", ctypes.c_uint64), ("algorithmic_bytes", ctypes.c_uint64),
                ("kernel_name", ctypes.c_char * 96)]


class GConvDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("bs", "ic", "ih", "iw", "oc", "oh", "ow", "groups", "kh", "kw", "sh", "sw",
                                             "pad_t", "pad_l", "dst_dt", "bia_dt", "relu", "round_mode", "nscales",
                                             "force_path")]


class GConvInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("path", "grid", "block", "lds_bytes", "device")] + \
               [("algorithmic_ops", ctypes.c_uint64), ("algorithmic_bytes", ctypes.c_uint64),
                ("kernel_name", ctypes.c_char * 96)]


class ImgConvDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("bs", "ic", "ih", "iw", "oc", "oh", "ow", "kh", "kw", "sh", "sw", "pad_t",
                                             "pad_l", "dst_dt", "bia_dt", "relu", "round_mode", "nscales", "force_path")]


class ImgConvInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("path", "grid", "block", "lds_bytes", "device")] + \
               [("algorithmic_ops", ctypes.c_uint64), ("algorithmic_bytes", ctypes.c_uint64),
                ("kernel_name", ctypes.c_char * 96)]


class DeconvDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("bs", "ic", "ih", "iw", "oc", "oh", "ow", "kh", "kw", "sh", "sw", "pad_t",
                                             "pad_l", "dst_dt", "bia_dt", "relu", "round_mode", "nscales", "force_path")]


class DeconvInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("path", "grid", "block", "lds_bytes", "device")] + \
               [("algorithmic_ops", ctypes.c_uint64), ("algorithmic_bytes", ctypes.c_uint64),
                ("kernel_name", ctypes.c_char * 96)]


class DilConvDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("bs", "ic", "ih", "iw", "oc", "oh", "ow", "kh", "kw", "sh", "sw", "dh", "dw",
                                             "pad_t", "pad_l", "dst_dt", "bia_dt", "relu", "round_mode", "nscales",
                                             "force_path")]


class DilConvInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("path", "grid", "block", "lds_bytes", "device")] + \
               [("algorithmic_ops", ctypes.c_uint64), ("algorithmic_bytes", ctypes.c_uint64),
                ("kernel_name", ctypes.c_char * 96)]


class ResizeDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("bs", "c", "ih", "iw", "oh", "ow", "dt", "algo", "coord", "add", "post_relu",
                                             "force_path")]


class ResizeInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("path", "grid", "block", "lds_bytes", "device", "rows_per_lane")] + \
               [("algorithmic_bytes", ctypes.c_uint64), ("kernel_name", ctypes.c_char * 96)]


class FcDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("bs", "ic", "ih", "iw", "oc", "dst_dt", "bia_dt", "relu", "round_mode",
                                             "nscales", "force_path")]


class FcInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("path", "splitk", "grid", "block", "lds_bytes", "device")] + \
               [("algorithmic_ops", ctypes.c_uint64), ("algorithmic_bytes", ctypes.c_uint64),
                ("kernel_name", ctypes.c_char * 96)]


class SeDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("bs", "c", "ih", "iw", "cr", "mode", "bia1_dt", "bia2_dt", "round_mode",
                                             "nscales1", "nscales2", "nscales_out", "force_path")]


class SeInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("path", "slices", "grid", "block", "lds_bytes", "device")] + \
               [("algorithmic_bytes", ctypes.c_uint64), ("kernel_name", ctypes.c_char * 96)]


class WsumDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("bs", "h", "w", "c", "n_inputs")] + \
               [("src_dt", ctypes.c_int32 * 8), ("nscales", ctypes.c_int32 * 8)] + \
               [(n, ctypes.c_int32) for n in ("n_bias", "dst_dt", "round_mode", "post_relu", "lut_in_dt", "force_path")]


class WsumInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("path", "grid", "block", "lds_bytes", "device")] + \
               [("algorithmic_bytes", ctypes.c_uint64), ("kernel_name", ctypes.c_char * 96)]


class HeadDesc(ctypes.Structure):
    _fields_ = [("rows", ctypes.c_int64)] + \
               [(n, ctypes.c_int32) for n in ("mode", "src_dt", "dst_dt", "c", "src_ld", "dst_ld", "idx_ld", "k")] + \
               [("out_scale", ctypes.c_float), ("force_path", ctypes.c_int32)]


class HeadInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("path", "grid", "block", "lds_bytes", "device")] + \
               [("algorithmic_bytes", ctypes.c_uint64), ("kernel_name", ctypes.c_char * 96)]


class SelectDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("bs", "h", "w", "c", "src_ld", "src_dt", "k", "idx_ld", "peak", "min_val",
                                             "n_gather")] + \
               [("row_bytes", ctypes.c_int32 * 4), ("pixel_stride_bytes", ctypes.c_int32 * 4), ("force_path", ctypes.c_int32)]


class SelectInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("path", "chunks", "chunk_pixels", "grid", "grid_image", "block", "block_image",
                                             "lds_bytes", "launches", "device")] + \
               [("scratch_bytes", ctypes.c_uint64), ("algorithmic_bytes", ctypes.c_uint64),
                ("kernel_name", ctypes.c_char * 96)]


class NmsDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("bs", "n", "max_out", "keep_ld", "mode", "per_class", "classes", "anchors_per_pixel",
                                             "n_anchors", "row_bytes", "idx_ld")] + \
               [("iou_thr", ctypes.c_float), ("clip_w", ctypes.c_float), ("clip_h", ctypes.c_float), ("force_path", ctypes.c_int32)]


class NmsIo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("boxes", "idx", "deltas", "anchors", "tab_c", "tab_s", "count_in", "keep", "count",
                                              "boxes_out")]


class NmsInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("path", "tiles", "grid_prep", "grid_mask", "grid_scan", "block_prep", "block_mask",
                                             "block_scan", "lds_bytes", "launches", "device")] + \
               [("scratch_bytes", ctypes.c_uint64), ("algorithmic_bytes", ctypes.c_uint64),
                ("kernel_name", ctypes.c_char * 96)]


class RoiAlignDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("bs", "n", "mode", "levels", "c", "dt")] + \
               [("h", ctypes.c_int32 * 4), ("w", ctypes.c_int32 * 4), ("src_ld", ctypes.c_int32 * 4),
                ("spatial_scale", ctypes.c_float * 4), ("level_area_thr", ctypes.c_float * 3)] + \
               [(n, ctypes.c_int32) for n in ("ph", "pw", "sampling_ratio", "aligned", "dst_ld", "force_path")]


class RoiAlignIo(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p * 4)] + [(n, ctypes.c_void_p) for n in ("boxes", "count", "batch_idx", "dst")]


class RoiAlignInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("path", "grid", "block", "lds_bytes", "launches", "device", "rows_per_group")] + \
               [("algorithmic_bytes", ctypes.c_uint64), ("kernel_name", ctypes.c_char * 96)]


class BmmDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("batch0", "batch1", "m", "n", "k", "trans_b", "a_dt", "b_dt", "dst_dt", "relu",
                                              "round_mode", "nscales", "force_path")] + \
               [(n, ctypes.c_int64) for n in ("a_s0", "a_s1", "lda", "b_s0", "b_s1", "ldb", "c_s0", "c_s1", "ldc")]


class BmmInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("path", "grid", "block", "lds_bytes", "device")] + \
               [("algorithmic_ops", ctypes.c_uint64), ("algorithmic_bytes", ctypes.c_uint64),
                ("kernel_name", ctypes.c_char * 96)]


class LogitBiasDesc(ctypes.Structure):
    _fields_ = [("period0", ctypes.c_int32), ("period1", ctypes.c_int32), ("s0", ctypes.c_int64), ("s1", ctypes.c_int64),
                ("ld", ctypes.c_int64)]


class AttnDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("batch0", "batch1", "tq", "tk", "d", "dv", "q_dt", "k_dt", "v_dt", "dst_dt", "relu",
                                              "round_mode", "nscales", "force_path")] + \
               [("prob_scale", ctypes.c_float), ("reserved", ctypes.c_int32)] + \
               [(n, ctypes.c_int64) for n in ("q_s0", "q_s1", "ldq", "k_s0", "k_s1", "ldk", "v_s0", "v_s1", "ldv", "o_s0", "o_s1", "ldo")]


class AttnInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("path", "grid", "block", "lds_bytes", "device", "route_logits", "route_context")] + \
               [("scratch_bytes", ctypes.c_uint64), ("algorithmic_ops", ctypes.c_uint64), ("algorithmic_bytes", ctypes.c_uint64),
                ("kernel_name", ctypes.c_char * 96)]


class LnormDesc(ctypes.Structure):
    _fields_ = [("rows", ctypes.c_int64)] + \
               [(n, ctypes.c_int32) for n in ("mode", "src_dt", "dst_dt", "c", "src_ld", "dst_ld")] + \
               [("eps", ctypes.c_float), ("force_path", ctypes.c_int32)]


class LnormInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("path", "grid", "block", "lds_bytes", "device")] + \
               [("algorithmic_bytes", ctypes.c_uint64), ("kernel_name", ctypes.c_char * 96)]


class LinearDesc(ctypes.Structure):
    _fields_ = [("rows", ctypes.c_int64)] + \
               [(n, ctypes.c_int32) for n in ("k", "n", "src_dt", "dst_dt", "bia_dt", "relu", "round_mode", "nscales", "lut_in_dt",
                                              "force_path")] + \
               [("src_ld", ctypes.c_int64), ("dst_ld", ctypes.c_int64)]


class LinearInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("path", "grid", "block", "lds_bytes", "device")] + \
               [("algorithmic_ops", ctypes.c_uint64), ("algorithmic_bytes", ctypes.c_uint64),
                ("kernel_name", ctypes.c_char * 96)]


class PatchEmbedDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("bs", "ih", "iw", "ic", "ph", "pw", "th", "tw", "oc", "src_dt", "dst_dt", "bia_dt",
                                             "relu", "round_mode", "nscales", "table", "tok_offset", "force_path")] + \
               [("img_rows", ctypes.c_int64), ("dst_ld", ctypes.c_int64)]


class PatchEmbedInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("path", "grid", "block", "lds_bytes", "device", "granule")] + \
               [("algorithmic_ops", ctypes.c_uint64), ("algorithmic_bytes", ctypes.c_uint64),
                ("kernel_name", ctypes.c_char * 96)]


class WindowDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("dir", "dt", "bs", "h", "w", "c", "wh", "ww", "shift_y", "shift_x", "order")] + \
               [("grid_ld", ctypes.c_int64), ("win_ld", ctypes.c_int64), ("pad_value", ctypes.c_uint32), ("force_path", ctypes.c_int32)]


class WindowInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("path", "grid", "block", "device")] + \
               [("algorithmic_bytes", ctypes.c_uint64), ("kernel_name", ctypes.c_char * 96)]


class DwPwDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("bs", "c", "ih", "iw", "oh", "ow", "kh", "kw", "sh", "sw", "pad_t", "pad_l",
                                             "oc", "dst_dt", "bia0_dt", "bia1_dt", "relu", "round_mode0", "round_mode1",
                                             "nscales0", "nscales1", "force_path")]


class DwPwInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("path", "grid", "block", "lds_bytes", "device")] + \
               [("algorithmic_ops", ctypes.c_uint64), ("algorithmic_bytes", ctypes.c_uint64),
                ("kernel_name", ctypes.c_char * 96)]


# route numbering of dfx_debug_conv_requant (include/dfx.h)
ROUTE_EXACT, ROUTE_FAST, ROUTE_MAGIC, ROUTE_FMA = 0, 1, 2, 3

# order of dfx_debug_conv_sched (include/dfx.h)
ConvSched = collections.namedtuple("ConvSched", "th tw linear uy ux total_units half_from static_rounds lazy_queue "
                                                "pool teams roles ring_waits")


def lib_path():
    return _LIB


def build(force=False, jobs=8):
    """Compile csrc/ for gfx950 into libdfx_hip.so (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-C", os.path.join(_PKG, "csrc"), "clean"],
                              stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", os.path.join(_PKG, "csrc"), "-j%d" % jobs, "-s"])
    return _LIB


def declared_symbols():
    """Every function name include/dfx.h declares."""
    text = open(_HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dfx_[a-z0-9_]+)\s*\(", text)))


_lib = None


def lib():
    """Load libdfx_hip.so; raises DfxError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB):
        raise DfxError("libdfx_hip.so is missing: run __graft_entry__.build() "
                       "(there is no CPU fallback for the deep-fusion hot path)")
    # PyTorch bundles its own HIP runtime under the same soname: when both live in one process
    # torch's must be loaded first (the other order leaves torch with "No HIP GPUs are
    # available").  This binding exists for tests / bench.py, which use torch for device memory.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(_LIB)
    vp, i32, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    sig = {
        "dfx_version": (i32, []),
        "dfx_last_error": (ctypes.c_char_p, []),
        "dfx_device_count": (i32, [ctypes.POINTER(i32)]),
        "dfx_set_device": (i32, [i32]),
        "dfx_device_name": (i32, [ctypes.c_char_p, sz]),
        "dfx_mem_alloc_host": (i32, [ctypes.POINTER(vp), sz]),
        "dfx_mem_free_host": (i32, [vp]),
        "dfx_mem_alloc_device": (i32, [ctypes.POINTER(vp), sz]),
        "dfx_mem_free_device": (i32, [vp]),
        "dfx_memcpy_h2d": (i32, [vp, vp, sz, vp]),
        "dfx_memcpy_d2h": (i32, [vp, vp, sz, vp]),
        "dfx_memset_device": (i32, [vp, i32, sz, vp]),
        "dfx_stream_create": (i32, [ctypes.POINTER(vp)]),
        "dfx_stream_destroy": (i32, [vp]),
        "dfx_stream_sync": (i32, [vp]),
        "dfx_stream_wait_stream": (i32, [vp, vp]),
        "dfx_event_create": (i32, [ctypes.POINTER(vp)]),
        "dfx_event_record": (i32, [vp, vp]),
        "dfx_event_elapsed_ms": (i32, [vp, vp, ctypes.POINTER(ctypes.c_float)]),
        "dfx_event_destroy": (i32, [vp]),
        "dfx_reorder_oihw_to_blocked": (i32, [vp, vp, i32, i32, i32, i32]),
        "dfx_blocked_offset": (sz, [i32] * 7),
        "dfx_conv_create": (i32, [ctypes.POINTER(ConvDesc), ctypes.POINTER(vp)]),
        "dfx_conv_set_weights": (i32, [vp] * 7),
        "dfx_conv_submit": (i32, [vp, vp, vp, vp]),
        "dfx_conv_submit_host": (i32, [vp, vp, vp]),
        "dfx_conv_query": (i32, [vp, ctypes.POINTER(ConvInfo)]),
        "dfx_conv_destroy": (i32, [vp]),
        "dfx_concat_create": (i32, [ctypes.POINTER(ConcatDesc), ctypes.POINTER(vp)]),
        "dfx_concat_submit": (i32, [vp, ctypes.POINTER(vp), vp, vp]),
        "dfx_concat_submit_host": (i32, [vp, ctypes.POINTER(vp), vp]),
        "dfx_concat_submit_gathered": (i32, [vp, vp, ctypes.POINTER(ctypes.c_uint64), vp, vp]),
        "dfx_concat_destroy": (i32, [vp]),
        "dfx_pool_create": (i32, [ctypes.POINTER(PoolDesc), ctypes.POINTER(vp)]),
        "dfx_pool_submit": (i32, [vp, vp, vp, vp]),
        "dfx_pool_destroy": (i32, [vp]),
        "dfx_eltwise_create": (i32, [ctypes.POINTER(EltwiseDesc), ctypes.POINTER(vp)]),
        "dfx_eltwise_submit": (i32, [vp, ctypes.POINTER(vp), vp, vp]),
        "dfx_eltwise_destroy": (i32, [vp]),
        "dfx_reorder_create": (i32, [ctypes.POINTER(ReorderDesc), vp, ctypes.POINTER(vp)]),
        "dfx_reorder_submit": (i32, [vp, vp, vp, vp]),
        "dfx_reorder_submit_host": (i32, [vp, vp, vp]),
        "dfx_reorder_query": (i32, [vp, ctypes.POINTER(ReorderInfo)]),
        "dfx_reorder_destroy": (i32, [vp]),
        "dfx_catconv_create": (i32, [ctypes.POINTER(CatConvDesc), ctypes.POINTER(vp)]),
        "dfx_catconv_set_weights": (i32, [vp, vp, vp, vp]),
        "dfx_catconv_submit": (i32, [vp, ctypes.POINTER(vp), vp, vp]),
        "dfx_catconv_submit_host": (i32, [vp, ctypes.POINTER(vp), vp]),
        "dfx_catconv_query": (i32, [vp, ctypes.POINTER(CatConvInfo)]),
        "dfx_catconv_destroy": (i32, [vp]),
        "dfx_dwconv_create": (i32, [ctypes.POINTER(DwConvDesc), ctypes.POINTER(vp)]),
        "dfx_dwconv_set_weights": (i32, [vp, vp, vp, vp]),
        "dfx_dwconv_submit": (i32, [vp, vp, vp, vp]),
        "dfx_dwconv_submit_host": (i32, [vp, vp, vp]),
        "dfx_dwconv_query": (i32, [vp, ctypes.POINTER(DwConvInfo)]),
        "dfx_dwconv_destroy": (i32, [vp]),
        "dfx_gconv_create": (i32, [ctypes.POINTER(GConvDesc), ctypes.POINTER(vp)]),
        "dfx_gconv_set_weights": (i32, [vp, vp, vp, vp]),
        "dfx_gconv_submit": (i32, [vp, vp, vp, vp]),
        "dfx_gconv_submit_host": (i32, [vp, vp, vp]),
        "dfx_gconv_query": (i32, [vp, ctypes.POINTER(GConvInfo)]),
        "dfx_gconv_destroy": (i32, [vp]),
        "dfx_imgconv_create": (i32, [ctypes.POINTER(ImgConvDesc), ctypes.POINTER(vp)]),
        "dfx_imgconv_set_weights": (i32, [vp, vp, vp, vp]),
        "dfx_imgconv_submit": (i32, [vp, vp, vp, vp]),
        "dfx_imgconv_submit_host": (i32, [vp, vp, vp]),
        "dfx_imgconv_query": (i32, [vp, ctypes.POINTER(ImgConvInfo)]),
        "dfx_imgconv_destroy": (i32, [vp]),
        "dfx_deconv_create": (i32, [ctypes.POINTER(DeconvDesc), ctypes.POINTER(vp)]),
        "dfx_deconv_set_weights": (i32, [vp, vp, vp, vp]),
        "dfx_deconv_submit": (i32, [vp, vp, vp, vp]),
        "dfx_deconv_submit_host": (i32, [vp, vp, vp]),
        "dfx_deconv_query": (i32, [vp, ctypes.POINTER(DeconvInfo)]),
        "dfx_deconv_destroy": (i32, [vp]),
        "dfx_dilconv_create": (i32, [ctypes.POINTER(DilConvDesc), ctypes.POINTER(vp)]),
        "dfx_dilconv_set_weights": (i32, [vp, vp, vp, vp]),
        "dfx_dilconv_submit": (i32, [vp, vp, vp, vp]),
        "dfx_dilconv_submit_host": (i32, [vp, vp, vp]),
        "dfx_dilconv_query": (i32, [vp, ctypes.POINTER(DilConvInfo)]),
        "dfx_dilconv_destroy": (i32, [vp]),
        "dfx_resize_create": (i32, [ctypes.POINTER(ResizeDesc), ctypes.POINTER(vp)]),
        "dfx_resize_submit": (i32, [vp, vp, vp, vp, vp]),
        "dfx_resize_submit_host": (i32, [vp, vp, vp, vp]),
        "dfx_resize_query": (i32, [vp, ctypes.POINTER(ResizeInfo)]),
        "dfx_resize_destroy": (i32, [vp]),
        "dfx_fc_create": (i32, [ctypes.POINTER(FcDesc), ctypes.POINTER(vp)]),
        "dfx_fc_set_weights": (i32, [vp, vp, vp, vp]),
        "dfx_fc_submit": (i32, [vp, vp, vp, vp]),
        "dfx_fc_submit_host": (i32, [vp, vp, vp]),
        "dfx_fc_query": (i32, [vp, ctypes.POINTER(FcInfo)]),
        "dfx_fc_destroy": (i32, [vp]),
        "dfx_se_create": (i32, [ctypes.POINTER(SeDesc), ctypes.POINTER(vp)]),
        "dfx_se_set_weights": (i32, [vp] * 9),
        "dfx_se_submit": (i32, [vp, vp, vp, vp]),
        "dfx_se_submit_host": (i32, [vp, vp, vp]),
        "dfx_se_query": (i32, [vp, ctypes.POINTER(SeInfo)]),
        "dfx_se_destroy": (i32, [vp]),
        "dfx_wsum_create": (i32, [ctypes.POINTER(WsumDesc), ctypes.POINTER(vp)]),
        "dfx_wsum_set_params": (i32, [vp, ctypes.POINTER(vp), vp, vp]),
        "dfx_wsum_submit": (i32, [vp, ctypes.POINTER(vp), vp, vp]),
        "dfx_wsum_submit_host": (i32, [vp, ctypes.POINTER(vp), vp]),
        "dfx_wsum_query": (i32, [vp, ctypes.POINTER(WsumInfo)]),
        "dfx_wsum_destroy": (i32, [vp]),
        "dfx_head_create": (i32, [ctypes.POINTER(HeadDesc), ctypes.POINTER(vp)]),
        "dfx_head_set_table": (i32, [vp, vp]),
        "dfx_head_submit": (i32, [vp, vp, vp, vp, vp]),
        "dfx_head_query": (i32, [vp, ctypes.POINTER(HeadInfo)]),
        "dfx_head_destroy": (i32, [vp]),
        "dfx_dwpw_create": (i32, [ctypes.POINTER(DwPwDesc), ctypes.POINTER(vp)]),
        "dfx_dwpw_set_weights": (i32, [vp] * 7),
        "dfx_dwpw_submit": (i32, [vp, vp, vp, vp]),
        "dfx_dwpw_submit_host": (i32, [vp, vp, vp]),
        "dfx_dwpw_query": (i32, [vp, ctypes.POINTER(DwPwInfo)]),
        "dfx_dwpw_destroy": (i32, [vp]),
        "dfx_debug_scribble_lds": (i32, [ctypes.c_uint, vp]),
        "dfx_debug_set_tuning": (i32, [ctypes.c_char_p, ctypes.c_char_p]),
        "dfx_debug_conv_sched": (i32, [vp, ctypes.POINTER(ctypes.c_int32), i32]),
        "dfx_debug_conv_unit_px": (i32, [vp]),
        "dfx_debug_conv_requant": (i32, [vp, ctypes.POINTER(ctypes.c_int32)]),
        "dfx_debug_catconv_requant": (i32, [vp, ctypes.POINTER(ctypes.c_int32)]),
        "dfx_debug_dwconv_requant": (i32, [vp, ctypes.POINTER(ctypes.c_int32)]),
        "dfx_debug_gconv_requant": (i32, [vp, ctypes.POINTER(ctypes.c_int32)]),
        "dfx_debug_imgconv_requant": (i32, [vp, ctypes.POINTER(ctypes.c_int32)]),
        "dfx_debug_deconv_requant": (i32, [vp, ctypes.POINTER(ctypes.c_int32)]),
        "dfx_debug_dilconv_requant": (i32, [vp, ctypes.POINTER(ctypes.c_int32)]),
        "dfx_debug_dwpw_requant": (i32, [vp, ctypes.POINTER(ctypes.c_int32)]),
        "dfx_debug_fc_requant": (i32, [vp, ctypes.POINTER(ctypes.c_int32)]),
        "dfx_debug_resize_launches": (i32, [ctypes.POINTER(ctypes.c_int64)]),
        "dfx_debug_wsum_launches": (i32, [ctypes.POINTER(ctypes.c_int64)]),
        "dfx_debug_head_launches": (i32, [ctypes.POINTER(ctypes.c_int64)]),
        "dfx_select_create": (i32, [ctypes.POINTER(SelectDesc), ctypes.POINTER(vp)]),
        "dfx_select_submit": (i32, [vp, vp, vp, vp, vp, ctypes.POINTER(vp), ctypes.POINTER(vp), vp]),
        "dfx_select_query": (i32, [vp, ctypes.POINTER(SelectInfo)]),
        "dfx_select_destroy": (i32, [vp]),
        "dfx_debug_select_launches": (i32, [ctypes.POINTER(ctypes.c_int64)]),
        "dfx_nms_create": (i32, [ctypes.POINTER(NmsDesc), ctypes.POINTER(vp)]),
        "dfx_nms_submit": (i32, [vp, ctypes.POINTER(NmsIo), vp]),
        "dfx_nms_query": (i32, [vp, ctypes.POINTER(NmsInfo)]),
        "dfx_nms_destroy": (i32, [vp]),
        "dfx_debug_nms_launches": (i32, [ctypes.POINTER(ctypes.c_int64)]),
        "dfx_roialign_create": (i32, [ctypes.POINTER(RoiAlignDesc), ctypes.POINTER(vp)]),
        "dfx_roialign_submit": (i32, [vp, ctypes.POINTER(RoiAlignIo), vp]),
        "dfx_roialign_query": (i32, [vp, ctypes.POINTER(RoiAlignInfo)]),
        "dfx_roialign_destroy": (i32, [vp]),
        "dfx_debug_roialign_launches": (i32, [ctypes.POINTER(ctypes.c_int64)]),
        "dfx_bmm_create": (i32, [ctypes.POINTER(BmmDesc), ctypes.POINTER(vp)]),
        "dfx_bmm_set_scales": (i32, [vp, vp]),
        "dfx_bmm_set_bias": (i32, [vp, ctypes.POINTER(LogitBiasDesc), vp]),
        "dfx_bmm_submit": (i32, [vp, vp, vp, vp, vp]),
        "dfx_bmm_query": (i32, [vp, ctypes.POINTER(BmmInfo)]),
        "dfx_bmm_destroy": (i32, [vp]),
        "dfx_debug_bmm_launches": (i32, [ctypes.POINTER(ctypes.c_int64)]),
        "dfx_debug_bmm_requant": (i32, [vp, ctypes.POINTER(ctypes.c_int32)]),
        "dfx_attn_create": (i32, [ctypes.POINTER(AttnDesc), ctypes.POINTER(vp)]),
        "dfx_attn_set_table": (i32, [vp, vp]),
        "dfx_attn_set_scales": (i32, [vp, ctypes.c_float, vp]),
        "dfx_attn_set_bias": (i32, [vp, ctypes.POINTER(LogitBiasDesc), vp]),
        "dfx_attn_submit": (i32, [vp, vp, vp, vp, vp, vp]),
        "dfx_attn_query": (i32, [vp, ctypes.POINTER(AttnInfo)]),
        "dfx_attn_destroy": (i32, [vp]),
        "dfx_debug_attn_launches": (i32, [ctypes.POINTER(ctypes.c_int64)]),
        "dfx_lnorm_create": (i32, [ctypes.POINTER(LnormDesc), ctypes.POINTER(vp)]),
        "dfx_lnorm_set_params": (i32, [vp, vp, vp, vp]),
        "dfx_lnorm_submit": (i32, [vp, vp, vp, vp]),
        "dfx_lnorm_query": (i32, [vp, ctypes.POINTER(LnormInfo)]),
        "dfx_lnorm_destroy": (i32, [vp]),
        "dfx_debug_lnorm_launches": (i32, [ctypes.POINTER(ctypes.c_int64)]),
        "dfx_linear_create": (i32, [ctypes.POINTER(LinearDesc), ctypes.POINTER(vp)]),
        "dfx_linear_set_weights": (i32, [vp, vp, vp, vp]),
        "dfx_linear_set_table": (i32, [vp, vp]),
        "dfx_linear_submit": (i32, [vp, vp, vp, vp]),
        "dfx_linear_submit_host": (i32, [vp, vp, vp]),
        "dfx_linear_query": (i32, [vp, ctypes.POINTER(LinearInfo)]),
        "dfx_linear_destroy": (i32, [vp]),
        "dfx_debug_linear_launches": (i32, [ctypes.POINTER(ctypes.c_int64)]),
        "dfx_debug_linear_requant": (i32, [vp, ctypes.POINTER(ctypes.c_int32)]),
        "dfx_patchembed_create": (i32, [ctypes.POINTER(PatchEmbedDesc), ctypes.POINTER(vp)]),
        "dfx_patchembed_set_weights": (i32, [vp, vp, vp, vp]),
        "dfx_patchembed_set_table": (i32, [vp, vp, ctypes.c_int64]),
        "dfx_patchembed_set_prefix": (i32, [vp, vp]),
        "dfx_patchembed_submit": (i32, [vp, vp, vp, vp]),
        "dfx_patchembed_submit_host": (i32, [vp, vp, vp]),
        "dfx_patchembed_query": (i32, [vp, ctypes.POINTER(PatchEmbedInfo)]),
        "dfx_patchembed_destroy": (i32, [vp]),
        "dfx_debug_patchembed_launches": (i32, [ctypes.POINTER(ctypes.c_int64)]),
        "dfx_debug_patchembed_requant": (i32, [vp, ctypes.POINTER(ctypes.c_int32)]),
        "dfx_window_create": (i32, [ctypes.POINTER(WindowDesc), ctypes.POINTER(vp)]),
        "dfx_window_submit": (i32, [vp, vp, vp, vp]),
        "dfx_window_query": (i32, [vp, ctypes.POINTER(WindowInfo)]),
        "dfx_window_destroy": (i32, [vp]),
        "dfx_debug_window_launches": (i32, [ctypes.POINTER(ctypes.c_int64)]),
    }
    for name, (res, args) in sig.items():
        try:
            f = getattr(L, name)
        except AttributeError:
            if os.environ.get("DFX_LIB_PATH"):  # an older diagnostic build (A/B against a past round): bind what it has
                continue
            raise
        f.restype, f.argtypes = res, args
    _lib = L
    return L


def set_tuning(key, value):
    """testing / tuning switch of the library; value None clears it."""
    _check(lib().dfx_debug_set_tuning(key.encode(), None if value is None else str(value).encode()))


def _launches(op, *paths):
    """dfx_debug_<op>_launches' counters in the order of `paths` (the op's path constants index them)"""
    v = (ctypes.c_int64 * len(paths))()
    _check(getattr(lib(), "dfx_debug_%s_launches" % op)(v))
    return tuple(v[p] for p in paths)


def resize_launches():
    """(band, generic): dfx_resize_submit calls of this process that launched each kernel (dfx_debug_resize_launches)"""
    return _launches("resize", RESIZE_BAND, RESIZE_GENERIC)


def wsum_launches():
    """(vec, generic): dfx_wsum_submit calls of this process that launched each kernel (dfx_debug_wsum_launches)"""
    return _launches("wsum", WSUM_VEC, WSUM_GENERIC)


def head_launches():
    """(pixel, row, generic): dfx_head_submit calls of this process that launched each kernel (dfx_debug_head_launches)"""
    return _launches("head", HEAD_PIXEL, HEAD_ROW, HEAD_GENERIC)


def select_launches():
    """(hist, generic): dfx_select_submit calls of this process that ran on each path (dfx_debug_select_launches)"""
    return _launches("select", SELECT_HIST, SELECT_GENERIC)


def nms_launches():
    """(mask, generic): dfx_nms_submit calls of this process that ran on each path (dfx_debug_nms_launches)"""
    return _launches("nms", NMS_MASK, NMS_GENERIC)


def roialign_launches():
    """(tile, generic): dfx_roialign_submit calls of this process that launched each kernel (dfx_debug_roialign_launches)"""
    return _launches("roialign", ROIALIGN_TILE, ROIALIGN_GENERIC)


def bmm_launches():
    """(mfma, generic): dfx_bmm_submit calls of this process that launched each kernel (dfx_debug_bmm_launches)"""
    return _launches("bmm", BMM_MFMA, BMM_GENERIC)


def attn_launches():
    """(fused, chain): dfx_attn_submit calls of this process that ran on each path (dfx_debug_attn_launches)"""
    return _launches("attn", ATTN_FUSED, ATTN_CHAIN)


def lnorm_launches():
    """(row, generic): dfx_lnorm_submit calls of this process that launched each kernel (dfx_debug_lnorm_launches)"""
    return _launches("lnorm", LNORM_ROW, LNORM_GENERIC)


def linear_launches():
    """(tile, generic): dfx_linear_submit calls of this process that launched each kernel (dfx_debug_linear_launches)"""
    return _launches("linear", LINEAR_TILE, LINEAR_GENERIC)


def patchembed_launches():
    """(tile, generic): dfx_patchembed_submit calls of this process that launched each kernel (dfx_debug_patchembed_launches)"""
    return _launches("patchembed", PATCHEMBED_TILE, PATCHEMBED_GENERIC)


def window_launches():
    """(row, generic): dfx_window_submit calls of this process that launched each kernel (dfx_debug_window_launches)"""
    return _launches("window", WINDOW_ROW, WINDOW_GENERIC)


def _pair(v):
    return (int(v), int(v)) if np.ndim(v) == 0 else (int(v[0]), int(v[1]))


def swin_shift_mask(h, w, window, shift):
    """The boolean {nW, wh * ww, wh * ww} attention mask of a shifted-window block, True = masked, for attention_bias(mask=...):
    official Swin's img_mask construction over the PADDED hp x wp map -- each axis is cut into the slices [0, -window),
    [-window, -shift), [-shift, end), the nine regions are labelled, the label map is partitioned into windows and two tokens
    of a window may attend to each other only where their labels agree.  An axis with shift 0 is one region; shift (0, 0) gives
    all False.  window and shift: an int or (y, x); the windows and their tokens are in dfa.WindowOp's row-major order."""
    wh, ww = _pair(window)
    sy, sx = _pair(shift)
    if min(int(h), int(w), wh, ww) < 1:
        raise ValueError("h, w and the window must be positive")
    hp, wp = -(-int(h) // wh) * wh, -(-int(w) // ww) * ww
    if not (0 <= sy < hp and 0 <= sx < wp):
        raise ValueError("the shift must lie within the padded map")

    def labels(n, win, s):
        lab = np.zeros(n, dtype=np.int64)
        if s:
            lab[max(n - win, 0):n - s] = 1     # (slice(-win, -s) of the official code; an empty slice when s >= win)
            lab[n - s:] = 2
        return lab

    img = labels(hp, wh, sy)[:, None] * 3 + labels(wp, ww, sx)[None, :]
    win = img.reshape(hp // wh, wh, wp // ww, ww).transpose(0, 2, 1, 3).reshape(-1, wh * ww)
    return np.ascontiguousarray(win[:, None, :] != win[:, :, None])


def swin_relative_bias(table, window):
    """Expands Swin's relative-position table {(2 wh - 1) * (2 ww - 1), heads} to {heads, wh * ww, wh * ww} for
    attention_bias(rel_bias=...): entry [head, i, j] = table[(yi - yj + wh - 1) * (2 ww - 1) + (xi - xj + ww - 1), head] with
    token i = yi * ww + xi (official Swin's relative_position_index).  The table's dtype is kept."""
    wh, ww = _pair(window)
    t = np.asarray(table)
    if t.ndim != 2 or t.shape[0] != (2 * wh - 1) * (2 * ww - 1):
        raise ValueError("the table is {(2 wh - 1) * (2 ww - 1), heads}")
    ys, xs = np.divmod(np.arange(wh * ww), ww)
    idx = (ys[:, None] - ys[None, :] + wh - 1) * (2 * ww - 1) + (xs[:, None] - xs[None, :] + ww - 1)
    return np.ascontiguousarray(t[idx].transpose(2, 0, 1))


def patch_embed_table(conv_bias, pos_embed, acc_step):
    """The f32 {tokens, oc} table of dfa.PatchEmbed(table=True) from what a float model holds: (bias[o] + pos[t][o]) /
    acc_step[o], the real-valued conv bias (None: 0) and position embedding in accumulator units, acc_step = the input's
    step times the weights' (a scalar or per oc).  Computed in float64 and rounded once to f32."""
    pos = np.asarray(pos_embed, dtype=np.float64)
    if pos.ndim != 2:
        raise ValueError("pos_embed is {tokens, oc}")
    step = np.asarray(acc_step, dtype=np.float64).reshape(-1)
    if step.size not in (1, pos.shape[1]) or not np.all(np.isfinite(step)) or np.any(step == 0):
        raise ValueError("acc_step holds 1 or oc finite non-zero values")
    b = np.zeros(pos.shape[1]) if conv_bias is None else np.asarray(conv_bias, dtype=np.float64).reshape(-1)
    if b.size != pos.shape[1]:
        raise ValueError("conv_bias holds oc values")
    with np.errstate(over="ignore"):      # (a value beyond f32 becomes inf, which set_table refuses)
        return ((b[None, :] + pos) / step[None, :]).astype(np.float32)


def patch_embed_prefix(cls_token, pos_rows, out_step, out_dt=np.int8):
    """The prefix rows of dfa.PatchEmbed.set_prefix: clamp(rint((cls_token + pos_rows) / out_step)) as out_dt (uint8 /
    int8), ties to even, computed in float64.  cls_token and pos_rows are {t0, oc} (or {oc} for one row); pos_rows None: 0."""
    out_dt = np.dtype(out_dt)
    if out_dt not in (np.dtype(np.uint8), np.dtype(np.int8)):
        raise ValueError("out_dt is uint8 or int8")
    if not (np.isfinite(float(out_step)) and float(out_step) > 0):
        raise ValueError("out_step must be finite and positive")
    v = np.atleast_2d(np.asarray(cls_token, dtype=np.float64))
    if pos_rows is not None:
        v = v + np.atleast_2d(np.asarray(pos_rows, dtype=np.float64))
    lo, hi = (0, 255) if out_dt == np.dtype(np.uint8) else (-128, 127)
    return np.clip(np.rint(v / float(out_step)), lo, hi).astype(out_dt)


def gelu_table(in_step, out_step, in_dt=np.int8, out_dt=np.int8):
    """The 256-byte table of dfa.Linear(table=...) for GELU behind a linear layer: entry i stands for the index-type value
    q (i for a uint8 index type, i - 128 for int8: dfx_wsum's convention), x = q * in_step, and holds
    clamp(rint(0.5 * x * (1 + erf(x / sqrt(2))) / out_step)) as out_dt, rint to even, computed in float64 with math.erf.
    Returned as uint8 bytes (an int8 value as its two's complement)."""
    import math
    in_dt, out_dt = np.dtype(in_dt), np.dtype(out_dt)
    if in_dt not in (np.dtype(np.uint8), np.dtype(np.int8)) or out_dt not in (np.dtype(np.uint8), np.dtype(np.int8)):
        raise ValueError("index and output types are uint8 or int8")
    if not (float(in_step) > 0 and float(out_step) > 0 and math.isfinite(in_step) and math.isfinite(out_step)):
        raise ValueError("steps must be finite and positive")
    lo, hi = (0, 255) if out_dt == np.dtype(np.uint8) else (-128, 127)
    out = np.empty(256, dtype=np.uint8)
    for i in range(256):
        x = float(i if in_dt == np.dtype(np.uint8) else i - 128) * float(in_step)
        g = 0.5 * x * (1.0 + math.erf(x / math.sqrt(2.0)))
        v = int(min(max(round(g / float(out_step)), lo), hi))   # round(): ties to even
        out[i] = v & 0xff
    return out


def lnorm_params(gamma, beta, in_scale, out_scale, eps):
    """(gamma', beta', eps_q) for dfa.LayerNorm from a float layer norm's parameters: the input is x = in_scale * code, the
    output code is y / out_scale (out_scale None: an f32 dst, which takes gamma and beta as they are).  eps_q = eps /
    in_scale^2 is eps in units of the integer domain.  Computed in float64 and rounded once.  beta None stays None."""
    g = np.asarray(gamma, dtype=np.float64).reshape(-1)
    b = None if beta is None else np.asarray(beta, dtype=np.float64).reshape(-1)
    if out_scale is not None:
        g = g / float(out_scale)
        b = None if b is None else b / float(out_scale)
    eps_q = np.float32(float(eps) / (float(in_scale) * float(in_scale)))
    return g.astype(np.float32), None if b is None else b.astype(np.float32), eps_q


def attention_strides(bs, heads, t, d, ld=None):
    """(s0, s1, ld) in elements of the per-head {T, d} matrices of a head-sliced {bs, T, heads * d} NHWC tensor whose
    rows are `ld` elements apart (heads * d when None): matrix (b0, b1) = (image, head) starts at b0 * s0 + b1 * s1.
    What dfa.MatMul takes as a_strides / b_strides / c_strides with batch = (bs, heads)."""
    ld = heads * d if ld is None else int(ld)
    if min(bs, heads, t, d) < 1 or ld < heads * d:
        raise ValueError("bs, heads, t, d must be positive and ld at least heads * d")
    return t * ld, d, ld


def _logit_bias_args(table, periods, strides, m, n):
    """(LogitBiasDesc, contiguous f32 array) of a logit bias for an {m, n} product.  strides None: `table` is densely packed,
    {period0, period1, m, n}, or {period0, period1, n} for one row broadcast over m (told apart by its size)."""
    t = np.ascontiguousarray(table, dtype=np.float32).reshape(-1)
    p0, p1 = (int(v) for v in periods)
    b = LogitBiasDesc()
    b.period0, b.period1 = p0, p1
    if strides is None:
        if t.size == p0 * p1 * m * n and (m > 1 or np.ndim(table) != 3):
            b.s0, b.s1, b.ld = p1 * m * n, m * n, n
        elif t.size == p0 * p1 * n:
            b.s0, b.s1, b.ld = p1 * n, n, 0
        else:
            raise ValueError("a dense table holds period0 * period1 * m * n or period0 * period1 * n values, not %d" % t.size)
    else:
        b.s0, b.s1, b.ld = (int(v) for v in strides)
        if min(p0, p1) >= 1 and min(b.s0, b.s1, b.ld) >= 0:          # (the library refuses the rest)
            need = (p0 - 1) * b.s0 + (p1 - 1) * b.s1 + ((m - 1) * b.ld if b.ld else 0) + n
            if t.size < need:
                raise ValueError("the table holds %d values, its layout addresses %d" % (t.size, need))
    return b, t


def attention_bias(rel_bias=None, mask=None, key_padding=None, *, logit_step, logit_scale, acc_bound, mask_value=None):
    """-> (table, periods): the accumulator-unit logit bias of dfa.Attention.set_bias / dfa.MatMul.set_bias (include/dfx.h)
    for an attention over batch = (batch0, batch1) from what a float model holds:
      rel_bias     {heads, tq, tk} real-valued (Swin's relative-position bias per head)        -> period1 = heads
      mask         {nW, tq, tk}: real-valued additive, -inf = masked; or boolean, True = masked  -> period0 = nW
      key_padding  {bs, tk} boolean, True = a padded key                                      -> period0 = bs
    (mask and key_padding both set period0 and must agree on it.)  A real value r becomes r / (logit_step * logit_scale):
    logit_step is the s8 logits' quantisation step, logit_scale the op's scale on the accumulator.  A masked entry becomes
    the FINITE value -(acc_bound + ceil(129 / |logit_scale|)), with logit_scale's sign, rounded away from zero to f32: with
    any accumulator within acc_bound (128 * 128 * d for s8 Q, 255 * 128 * d for u8 Q) the logit saturates to -128, and the
    fast requant route stays provable.  mask_value=-inf keeps -inf (always the exact route).  The table is
    {period0, period1, tq, tk}, or {period0, 1, tk} when only key_padding is given (one row broadcast over the queries)."""
    unit = float(logit_step) * float(logit_scale)
    if not np.isfinite(unit) or unit == 0.0:
        raise ValueError("logit_step * logit_scale must be finite and non-zero")
    if mask_value is None:
        mag = float(acc_bound) + float(np.ceil(129.0 / abs(float(logit_scale))))
        mv = np.float32(mag)
        if float(mv) < mag:
            mv = np.nextafter(mv, np.float32(np.inf))
        mask_value = -mv if logit_scale > 0 else mv
    mask_value = np.float32(mask_value)
    parts, masked = [], []
    if rel_bias is not None:
        r = np.asarray(rel_bias, dtype=np.float64)
        assert r.ndim == 3, "rel_bias is {heads, tq, tk}"
        parts.append(r[None])
    if mask is not None:
        mk = np.asarray(mask)
        assert mk.ndim == 3, "mask is {nW, tq, tk}"
        if mk.dtype == np.bool_:
            masked.append(mk[:, None])
        else:
            mk = mk.astype(np.float64)
            if np.isnan(mk).any() or np.isposinf(mk).any():
                raise ValueError("mask holds NaN or +inf")
            masked.append(np.isneginf(mk)[:, None])
            parts.append(np.where(np.isneginf(mk), 0.0, mk)[:, None])
    if key_padding is not None:
        kp = np.asarray(key_padding, dtype=np.bool_)
        assert kp.ndim == 2, "key_padding is {bs, tk}"
        masked.append(kp[:, None, None, :])
    if not parts and not masked:
        raise ValueError("nothing to build a bias from")
    total = np.zeros((1, 1, 1, 1), dtype=np.float64)
    for x in parts:
        total = total + x
    table = (total / unit).astype(np.float32)
    for x in masked:
        table = np.where(x, mask_value, np.broadcast_to(table, np.broadcast_shapes(table.shape, x.shape))).astype(np.float32)
    p0, p1, rows, cols = table.shape
    if rows == 1:                                      # key padding alone: one row per table
        return np.ascontiguousarray(table.reshape(p0, p1, cols)), (p0, p1)
    return np.ascontiguousarray(table), (p0, p1)


def roi_level_thresholds(k_min, k_max, canonical_scale=224, canonical_level=4, eps=1e-6):
    """The k_max - k_min f32 area thresholds of dfx_roialign's level rule that reproduce torchvision's LevelMapper,
    level = clamp(floor(canonical_level + log2(sqrt(area) / canonical_scale) + eps), k_min, k_max) - k_min: the mapper steps
    from level k - 1 to k at sqrt(area) = canonical_scale * 2^(k - canonical_level - eps), so threshold i is the square of
    that for k = k_min + 1 + i.  Computed in float64, rounded once to f32."""
    k = np.arange(int(k_min) + 1, int(k_max) + 1, dtype=np.float64)
    return ((float(canonical_scale) * np.exp2(k - float(canonical_level) - float(eps))) ** 2).astype(np.float32)


def box_tables(scale, zero_point, weight_xy, weight_wh, clip=float(np.log(1000.0 / 16)), dtype=np.uint8):
    """The two 256-entry f32 tables of dfx_nms's DECODE mode for 1-byte deltas of `dtype` (uint8 or int8) with quantisation
    (q - zero_point) * scale, indexed by the RAW byte: tab_c = d / weight_xy (dx, dy) and tab_s = exp(min(d / weight_wh,
    clip)) (dw, dh) -- torchvision's BoxCoder with its bbox_xform_clip.  Computed in float64, rounded once to f32."""
    raw = np.arange(256, dtype=np.uint8)
    q = raw.view(np.int8).astype(np.float64) if np.dtype(dtype) == np.int8 else raw.astype(np.float64)
    d = (q - float(zero_point)) * float(scale)
    return (d / float(weight_xy)).astype(np.float32), np.exp(np.minimum(d / float(weight_wh), float(clip))).astype(np.float32)


def softmax_table(scale, c):
    """The 256-entry uint32 table of a softmax over `c` channels of 1-byte logits with quantisation step `scale`:
    E[d] = floor(exp(-d * scale) * floor((2^32 - 1) / c)), d the distance from the row maximum (include/dfx.h).  The sum of
    any c entries stays within u32, and the probabilities are within 1e-6 absolute of a float64 softmax."""
    if not 1 <= int(c) <= 65535:
        raise ValueError("c must lie in 1 .. 65535")
    top = (2 ** 32 - 1) // int(c)
    d = np.arange(256, dtype=np.float64)
    return np.floor(np.exp(-d * float(scale)) * top).astype(np.uint32)


def _check(rc):
    if rc != 0:
        raise DfxError("dfx error %d: %s" % (rc, lib().dfx_last_error().decode()))


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def reorder_oihw_to_blocked(w_oihw):
    w = np.ascontiguousarray(w_oihw, dtype=np.int8)
    O, I, KH, KW = w.shape
    out = np.empty(w.size, dtype=np.int8)
    _check(lib().dfx_reorder_oihw_to_blocked(_p(w), _p(out), O, I, KH, KW))
    return out


def _dev_ptr(t):
    """torch CUDA tensor or raw int -> device pointer."""
    return ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr())


def _stream_ptr(stream):
    if stream is None:
        import torch
        stream = torch.cuda.current_stream()
    return ctypes.c_void_p(stream if isinstance(stream, int) else stream.cuda_stream)


class _Handle:
    """What the handle classes share: a dfx_<op>_* handle in _h, made by _create() and released by close(); query,
    requant route and the single-source submits, each one call of the C entry point named after _OP.  An op that lacks
    an entry point (dfx.h) raises AttributeError for it."""

    _OP = None             # C symbol prefix, "dfx_conv"
    _INFO = None           # struct of dfx_<op>_query
    _ROUTES = 0            # requant routes dfx_debug_<op>_requant reports
    src_np_dtype = np.uint8

    def _fn(self, what):
        return getattr(lib(), "%s_%s" % (self._OP, what))

    def _create(self, desc, *more):
        self._h = ctypes.c_void_p()
        _check(self._fn("create")(ctypes.byref(desc), *more, ctypes.byref(self._h)))

    def submit(self, src_dev, dst_dev, stream=None):
        """asynchronous; src_dev / dst_dev are torch CUDA tensors (or raw pointers), 16-byte aligned"""
        _check(self._fn("submit")(self._h, _dev_ptr(src_dev), _dev_ptr(dst_dev), _stream_ptr(stream)))

    def submit_host(self, src_np):
        src = np.ascontiguousarray(src_np, dtype=self.src_np_dtype)
        want = getattr(self, "src_shape", src.shape)
        assert src.shape == want, (src.shape, want)
        dst = np.empty(self.dst_shape, dtype=self.dst_np_dtype)
        _check(self._fn("submit_host")(self._h, _p(src), _p(dst)))
        return dst

    def info(self):
        i = self._INFO()
        _check(self._fn("query")(self._h, ctypes.byref(i)))
        return i

    def requant(self):
        """requant route(s) as set_weights proved them (dfx_debug_<op>_requant; launches nothing): ROUTE_EXACT /
        ROUTE_FAST / ROUTE_MAGIC / ROUTE_FMA, -1 for a stage the op does not have.  One value for an op of one stage,
        the tuple (stage 0, stage 1) otherwise."""
        v = (ctypes.c_int32 * self._ROUTES)()
        _check(getattr(lib(), self._OP.replace("dfx_", "dfx_debug_") + "_requant")(self._h, v))
        return v[0] if self._ROUTES == 1 else tuple(v)

    def close(self):
        if self._h:
            self._fn("destroy")(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _ptr_array(arrays_or_tensors, ptr_of):
    return (ctypes.c_void_p * len(arrays_or_tensors))(*[ptr_of(a) for a in arrays_or_tensors])


class Conv(_Handle):
    """dfx_conv_* handle: the op_conv<T> of the reference (src/op_conv.h:34-96)."""

    _OP, _INFO, _ROUTES = "dfx_conv", ConvInfo, 2

    def __init__(self, src_shape_nhwc, wei_shape_oihw, stride=(1, 1), pad=(1, 1), dst_dt=DFX_U8,
                 oc1x1=0, bia0_dt=DFX_UNDEF, bia1_dt=DFX_UNDEF, conv0_relu=False,
                 conv1_relu=False, rm0=ROUND_NEAREST, rm1=ROUND_NEAREST, nscales0=1, nscales1=1,
                 force_variant=-1, fuse_pool=0):
        bs, ih, iw, ic = src_shape_nhwc
        oc, ic2, kh, kw = wei_shape_oihw
        if ic2 != ic:
            raise DfxError("Input channel do not match")
        d = ConvDesc()
        d.bs, d.ic, d.ih, d.iw, d.oc, d.kh, d.kw = bs, ic, ih, iw, oc, kh, kw
        d.sh, d.sw = stride
        d.pad_t, d.pad_l = pad
        d.oh = (ih + 2 * d.pad_t - kh) // d.sh + 1
        d.ow = (iw + 2 * d.pad_l - kw) // d.sw + 1
        d.oc1x1, d.dst_dt, d.bia0_dt, d.bia1_dt = oc1x1, dst_dt, bia0_dt, bia1_dt
        d.conv0_relu, d.conv1_relu = int(conv0_relu), int(conv1_relu)
        d.conv0_round_mode, d.conv1_round_mode = rm0, rm1
        d.conv0_nscales, d.conv1_nscales = nscales0, nscales1
        d.force_variant = force_variant
        d.fuse_pool = fuse_pool
        self.desc = d
        self._create(d)
        self.dst_shape = ((bs, d.oh // 2, d.ow // 2, oc) if fuse_pool else (bs, d.oh, d.ow, oc1x1 if oc1x1 else oc))
        self.dst_np_dtype = _NP[dst_dt]

    def set_weights(self, wei_blk, scales0, bia0=None, wei1_blk=None, scales1=None, bia1=None):
        ws = [np.ascontiguousarray(wei_blk, dtype=np.int8),
              None if bia0 is None else np.ascontiguousarray(bia0),
              np.ascontiguousarray(scales0, dtype=np.float32),
              None if wei1_blk is None else np.ascontiguousarray(wei1_blk, dtype=np.int8),
              None if bia1 is None else np.ascontiguousarray(bia1),
              None if scales1 is None else np.ascontiguousarray(scales1, dtype=np.float32)]
        _check(lib().dfx_conv_set_weights(self._h, *[_p(w) for w in ws]))

    def sched(self):
        """unit hand-out of a resident-weight op (dfx_debug_conv_sched): a ConvSched; launches nothing."""
        v = (ctypes.c_int32 * len(ConvSched._fields))()
        _check(lib().dfx_debug_conv_sched(self._h, v, len(v)))
        return ConvSched(*v)

    def unit_px(self):
        """pixels per pixel-run unit (dfx_debug_conv_unit_px), 0 for row / column units; launches nothing."""
        v = lib().dfx_debug_conv_unit_px(self._h)
        if v < 0:
            _check(v)
        return v


class Pool(_Handle):
    """dfx_pool_* handle: the pooling stage of the reference's planned conv+relu+pool op (max pooling, NHWC)."""

    _OP = "dfx_pool"
    MAX, AVG_INCLUDE_PADDING, AVG_EXCLUDE_PADDING = 0, 1, 2

    def __init__(self, bs, c, ih, iw, oh, ow, kernel, stride, pad, np_dtype, algo=0):
        d = PoolDesc(bs, c, ih, iw, oh, ow, kernel[0], kernel[1], stride[0], stride[1], pad[0], pad[1],
                     _DT[np.dtype(np_dtype)], algo)
        self.dst_shape = (bs, oh, ow, c)
        self._create(d)


class EltwiseSum(_Handle):
    """dfx_eltwise_* handle: the reference's planned eltwise-sum + relu op."""

    _OP = "dfx_eltwise"

    def __init__(self, n_inputs, elems, np_dtype, post_relu=False):
        self._create(EltwiseDesc(n_inputs, elems, _DT[np.dtype(np_dtype)], int(post_relu)))

    def submit(self, srcs_dev, dst_dev, stream=None):
        ptrs = _ptr_array(srcs_dev, lambda t: _dev_ptr(t).value)
        _check(lib().dfx_eltwise_submit(self._h, ptrs, _dev_ptr(dst_dev), _stream_ptr(stream)))


class Reorder(_Handle):
    """dfx_reorder_* handle: layout (NHWC <-> NCHW), dtype and scale conversion of an activation tensor with
    channel pad / crop (include/dfx.h).  `shape` is the logical (bs, c, h, w) of the source; the physical order
    of src and dst follows src_fmt / dst_fmt."""

    _OP, _INFO = "dfx_reorder", ReorderInfo

    def __init__(self, shape_nchw, src_dtype, dst_dtype, src_fmt=FMT_NCHW, dst_fmt=FMT_NHWC, dst_c=None,
                 scales=None, round_mode=ROUND_NEAREST):
        bs, c, h, w = shape_nchw
        dst_c = c if dst_c is None else dst_c
        src_dt = src_dtype if isinstance(src_dtype, int) else _DT[np.dtype(src_dtype)]
        dst_dt = dst_dtype if isinstance(dst_dtype, int) else _DT[np.dtype(dst_dtype)]
        sc = None if scales is None else np.ascontiguousarray(scales, dtype=np.float32).reshape(-1)
        d = ReorderDesc(bs, h, w, c, dst_c, src_fmt, dst_fmt, src_dt, dst_dt, round_mode, 0 if sc is None else sc.size)
        self.desc = d
        self.src_shape = (bs, h, w, c) if src_fmt == FMT_NHWC else (bs, c, h, w)
        self.dst_shape = (bs, h, w, dst_c) if dst_fmt == FMT_NHWC else (bs, dst_c, h, w)
        self.src_np_dtype, self.dst_np_dtype = _NP.get(src_dt), _NP.get(dst_dt)
        self._create(d, _p(sc))


class ConcatConv(_Handle):
    """dfx_catconv_* handle: channel concat of NHWC u8 branches + pointwise conv in one launch (include/dfx.h).
    The result equals Concat followed by the unfused 1x1 Conv bit for bit; the concatenated tensor is never
    written on the fused path."""

    _OP, _INFO, _ROUTES = "dfx_catconv", CatConvInfo, 2  # (the routes of the inner pointwise conv, as Conv.requant())

    def __init__(self, bs, h, w, channels, oc, dst_dt=DFX_U8, bia_dt=DFX_UNDEF, relu=False, rm=ROUND_NEAREST,
                 nscales=1, force_path=CATCONV_AUTO):
        self.channels = list(channels)
        self._ch = (ctypes.c_int32 * len(self.channels))(*self.channels)
        d = CatConvDesc(len(self.channels), bs, h, w, oc, dst_dt, bia_dt, int(relu), rm, nscales, force_path, self._ch)
        self.desc = d
        self.dst_shape = (bs, h, w, oc)
        self.src_shapes = [(bs, h, w, c) for c in self.channels]
        self.dst_np_dtype = _NP.get(dst_dt)
        self._create(d)

    def set_weights(self, wei_blk, scales, bia=None):
        """wei_blk: {oc, sum(channels), 1, 1} in OIhw4i16o4i order (reorder_oihw_to_blocked)"""
        ws = [np.ascontiguousarray(wei_blk, dtype=np.int8), None if bia is None else np.ascontiguousarray(bia),
              np.ascontiguousarray(scales, dtype=np.float32)]
        _check(lib().dfx_catconv_set_weights(self._h, _p(ws[0]), _p(ws[1]), _p(ws[2])))

    def submit(self, srcs_dev, dst_dev, stream=None):
        """asynchronous; srcs_dev: one torch CUDA tensor (or raw pointer) per branch, 16-byte aligned"""
        ptrs = _ptr_array(srcs_dev, lambda t: _dev_ptr(t).value)
        _check(lib().dfx_catconv_submit(self._h, ptrs, _dev_ptr(dst_dev), _stream_ptr(stream)))

    def submit_host(self, srcs_np):
        srcs = [np.ascontiguousarray(s, dtype=np.uint8) for s in srcs_np]
        assert [s.shape for s in srcs] == self.src_shapes, ([s.shape for s in srcs], self.src_shapes)
        dst = np.empty(self.dst_shape, dtype=self.dst_np_dtype)
        _check(lib().dfx_catconv_submit_host(self._h, _ptr_array(srcs, lambda a: a.ctypes.data), _p(dst)))
        return dst


def _conv_out_hw(ih, iw, kernel, stride, pad):
    return ((ih + 2 * pad[0] - kernel[0]) // stride[0] + 1, (iw + 2 * pad[1] - kernel[1]) // stride[1] + 1)


class DwConv(_Handle):
    """dfx_dwconv_* handle: depthwise int8 conv over NHWC u8 (include/dfx.h).  For c a multiple of 16 the result equals
    the unfused Conv with ic = oc = c and block-diagonal weights bit for bit.  out_hw defaults to the conv's
    (in + 2 * pad - k) // stride + 1; give it for windows that hang over the bottom / right edge."""

    _OP, _INFO, _ROUTES = "dfx_dwconv", DwConvInfo, 1

    def __init__(self, src_shape_nhwc, kernel, stride=(1, 1), pad=(1, 1), out_hw=None, dst_dt=DFX_U8, bia_dt=DFX_UNDEF,
                 relu=False, rm=ROUND_NEAREST, nscales=1, force_path=DWCONV_AUTO):
        bs, ih, iw, c = src_shape_nhwc
        kh, kw = kernel
        if out_hw is None:
            out_hw = _conv_out_hw(ih, iw, kernel, stride, pad)
        d = DwConvDesc(bs, c, ih, iw, out_hw[0], out_hw[1], kh, kw, stride[0], stride[1], pad[0], pad[1], dst_dt, bia_dt,
                       int(relu), rm, nscales, force_path)
        self.desc = d
        self.src_shape = (bs, ih, iw, c)
        self.dst_shape = (bs, out_hw[0], out_hw[1], c)
        self.dst_np_dtype = _NP.get(dst_dt)
        self._create(d)

    def set_weights(self, wei, scales, bia=None):
        """wei: int8 {c, kh, kw}; scales: 1 or c floats; bia: c entries of the descriptor's bias dtype"""
        ws = [np.ascontiguousarray(wei, dtype=np.int8), None if bia is None else np.ascontiguousarray(bia),
              np.ascontiguousarray(scales, dtype=np.float32)]
        assert ws[0].size == self.desc.c * self.desc.kh * self.desc.kw, ws[0].shape
        assert ws[2].size == self.desc.nscales and (bia is None or ws[1].size == self.desc.c)
        _check(lib().dfx_dwconv_set_weights(self._h, _p(ws[0]), _p(ws[1]), _p(ws[2])))


class GroupConv(_Handle):
    """dfx_gconv_* handle: grouped int8 conv over NHWC u8 (include/dfx.h), weights plain oihw {oc, ic/groups, kh, kw}.
    Where ic and oc are multiples of 16 and the output size is the conv's, the result equals the unfused Conv on
    block-diagonal weights bit for bit.  out_hw defaults to the conv's (in + 2 * pad - k) // stride + 1; give it for
    windows that hang over the bottom / right edge."""

    _OP, _INFO, _ROUTES = "dfx_gconv", GConvInfo, 1

    def __init__(self, src_shape_nhwc, oc, groups, kernel, stride=(1, 1), pad=(1, 1), out_hw=None, dst_dt=DFX_U8,
                 bia_dt=DFX_UNDEF, relu=False, rm=ROUND_NEAREST, nscales=1, force_path=GCONV_AUTO):
        bs, ih, iw, ic = src_shape_nhwc
        kh, kw = kernel
        if out_hw is None:
            out_hw = _conv_out_hw(ih, iw, kernel, stride, pad)
        d = GConvDesc(bs, ic, ih, iw, oc, out_hw[0], out_hw[1], groups, kh, kw, stride[0], stride[1], pad[0], pad[1],
                      dst_dt, bia_dt, int(relu), rm, nscales, force_path)
        self.desc = d
        self.src_shape = (bs, ih, iw, ic)
        self.dst_shape = (bs, out_hw[0], out_hw[1], oc)
        self.dst_np_dtype = _NP.get(dst_dt)
        self._create(d)

    def set_weights(self, wei, scales, bia=None):
        """wei: int8 {oc, ic/groups, kh, kw}; scales: 1 or oc floats; bia: oc entries of the descriptor's bias dtype"""
        d = self.desc
        ws = [np.ascontiguousarray(wei, dtype=np.int8), None if bia is None else np.ascontiguousarray(bia),
              np.ascontiguousarray(scales, dtype=np.float32)]
        assert ws[0].size == d.oc * (d.ic // d.groups) * d.kh * d.kw, ws[0].shape
        assert ws[2].size == d.nscales and (bia is None or ws[1].size == d.oc)
        _check(lib().dfx_gconv_set_weights(self._h, _p(ws[0]), _p(ws[1]), _p(ws[2])))


class ImageConv(_Handle):
    """dfx_imgconv_* handle: the first-layer int8 conv over a 1- to 4-channel NHWC u8 image (include/dfx.h), weights plain
    oihw {oc, ic, kh, kw}.  The result equals GroupConv with groups = 1 bit for bit and, where oc is a multiple of 16 and
    the output size is the conv's, the unfused Conv on the image zero-padded to 16 channels.  src may sit at any byte
    address.  out_hw defaults to the conv's (in + 2 * pad - k) // stride + 1; give it for windows that hang over the
    bottom / right edge."""

    _OP, _INFO, _ROUTES = "dfx_imgconv", ImgConvInfo, 1

    def __init__(self, src_shape_nhwc, oc, kernel, stride=(1, 1), pad=(1, 1), out_hw=None, dst_dt=DFX_U8, bia_dt=DFX_UNDEF,
                 relu=False, rm=ROUND_NEAREST, nscales=1, force_path=IMGCONV_AUTO):
        bs, ih, iw, ic = src_shape_nhwc
        kh, kw = kernel
        if out_hw is None:
            out_hw = _conv_out_hw(ih, iw, kernel, stride, pad)
        d = ImgConvDesc(bs, ic, ih, iw, oc, out_hw[0], out_hw[1], kh, kw, stride[0], stride[1], pad[0], pad[1], dst_dt,
                        bia_dt, int(relu), rm, nscales, force_path)
        self.desc = d
        self.src_shape = (bs, ih, iw, ic)
        self.dst_shape = (bs, out_hw[0], out_hw[1], oc)
        self.dst_np_dtype = _NP.get(dst_dt)
        self._create(d)

    def set_weights(self, wei, scales, bia=None):
        """wei: int8 {oc, ic, kh, kw}; scales: 1 or oc floats; bia: oc entries of the descriptor's bias dtype"""
        d = self.desc
        ws = [np.ascontiguousarray(wei, dtype=np.int8), None if bia is None else np.ascontiguousarray(bia),
              np.ascontiguousarray(scales, dtype=np.float32)]
        assert ws[0].size == d.oc * d.ic * d.kh * d.kw, ws[0].shape
        assert ws[2].size == d.nscales and (bia is None or ws[1].size == d.oc)
        _check(lib().dfx_imgconv_set_weights(self._h, _p(ws[0]), _p(ws[1]), _p(ws[2])))


def deconv_out_hw(ih, iw, kernel, stride, pad, output_padding=(0, 0)):
    """the output size of a transposed conv with symmetric padding: (in - 1) * stride - 2 * pad + k + output_padding"""
    return ((ih - 1) * stride[0] - 2 * pad[0] + kernel[0] + output_padding[0],
            (iw - 1) * stride[1] - 2 * pad[1] + kernel[1] + output_padding[1])


class Deconv(_Handle):
    """dfx_deconv_* handle: int8 transposed conv over NHWC u8 (include/dfx.h), weights plain {oc, ic, kh, kw} (PyTorch's
    ConvTranspose2d.weight is {ic, oc, kh, kw}: swap the first two axes).  The result equals GroupConv with groups = 1,
    stride 1 and padding (kh-1-pad_t, kw-1-pad_l) on the zero-stuffed tensor with the spatially flipped weights, bit for
    bit.  pad is {top, left}; out_hw defaults to (in - 1) * stride - 2 * pad + k; give it for output_padding or a crop."""

    _OP, _INFO, _ROUTES = "dfx_deconv", DeconvInfo, 1

    def __init__(self, src_shape_nhwc, oc, kernel, stride=(2, 2), pad=(0, 0), out_hw=None, dst_dt=DFX_U8, bia_dt=DFX_UNDEF,
                 relu=False, rm=ROUND_NEAREST, nscales=1, force_path=DECONV_AUTO):
        bs, ih, iw, ic = src_shape_nhwc
        kh, kw = kernel
        if out_hw is None:
            out_hw = deconv_out_hw(ih, iw, kernel, stride, pad)
        d = DeconvDesc(bs, ic, ih, iw, oc, out_hw[0], out_hw[1], kh, kw, stride[0], stride[1], pad[0], pad[1], dst_dt,
                       bia_dt, int(relu), rm, nscales, force_path)
        self.desc = d
        self.src_shape = (bs, ih, iw, ic)
        self.dst_shape = (bs, out_hw[0], out_hw[1], oc)
        self.dst_np_dtype = _NP.get(dst_dt)
        self._create(d)

    def set_weights(self, wei, scales, bia=None):
        """wei: int8 {oc, ic, kh, kw}; scales: 1 or oc floats; bia: oc entries of the descriptor's bias dtype"""
        d = self.desc
        ws = [np.ascontiguousarray(wei, dtype=np.int8), None if bia is None else np.ascontiguousarray(bia),
              np.ascontiguousarray(scales, dtype=np.float32)]
        assert ws[0].size == d.oc * d.ic * d.kh * d.kw, ws[0].shape
        assert ws[2].size == d.nscales and (bia is None or ws[1].size == d.oc)
        _check(lib().dfx_deconv_set_weights(self._h, _p(ws[0]), _p(ws[1]), _p(ws[2])))


def dilconv_out_hw(ih, iw, kernel, stride, dilation, pad):
    """the output size of a dilated conv with symmetric padding: (in + 2 * pad - ((k - 1) * d + 1)) // stride + 1"""
    return ((ih + 2 * pad[0] - ((kernel[0] - 1) * dilation[0] + 1)) // stride[0] + 1,
            (iw + 2 * pad[1] - ((kernel[1] - 1) * dilation[1] + 1)) // stride[1] + 1)


class DilatedConv(_Handle):
    """dfx_dilconv_* handle: int8 dilated conv over NHWC u8 (include/dfx.h), weights plain oihw {oc, ic, kh, kw}.  The
    result equals GroupConv with groups = 1 on the zero-stuffed ((k-1)*d+1)^2 window bit for bit, wherever that window can
    be expressed.  pad is {top, left}; out_hw defaults to the conv formula's with the dilated extent; give it for windows
    that hang over the bottom / right edge or a cropped output."""

    _OP, _INFO, _ROUTES = "dfx_dilconv", DilConvInfo, 1

    def __init__(self, src_shape_nhwc, oc, kernel, dilation=(1, 1), stride=(1, 1), pad=(0, 0), out_hw=None, dst_dt=DFX_U8,
                 bia_dt=DFX_UNDEF, relu=False, rm=ROUND_NEAREST, nscales=1, force_path=DILCONV_AUTO):
        bs, ih, iw, ic = src_shape_nhwc
        kh, kw = kernel
        if out_hw is None:
            out_hw = dilconv_out_hw(ih, iw, kernel, stride, dilation, pad)
        d = DilConvDesc(bs, ic, ih, iw, oc, out_hw[0], out_hw[1], kh, kw, stride[0], stride[1], dilation[0], dilation[1],
                        pad[0], pad[1], dst_dt, bia_dt, int(relu), rm, nscales, force_path)
        self.desc = d
        self.src_shape = (bs, ih, iw, ic)
        self.dst_shape = (bs, out_hw[0], out_hw[1], oc)
        self.dst_np_dtype = _NP.get(dst_dt)
        self._create(d)

    def set_weights(self, wei, scales, bia=None):
        """wei: int8 {oc, ic, kh, kw}; scales: 1 or oc floats; bia: oc entries of the descriptor's bias dtype"""
        d = self.desc
        ws = [np.ascontiguousarray(wei, dtype=np.int8), None if bia is None else np.ascontiguousarray(bia),
              np.ascontiguousarray(scales, dtype=np.float32)]
        assert ws[0].size == d.oc * d.ic * d.kh * d.kw, ws[0].shape
        assert ws[2].size == d.nscales and (bia is None or ws[1].size == d.oc)
        _check(lib().dfx_dilconv_set_weights(self._h, _p(ws[0]), _p(ws[1]), _p(ws[2])))


class Resize(_Handle):
    """dfx_resize_* handle: nearest / bilinear resize of an NHWC tensor to (oh, ow), optionally with a tensor of dst's
    shape added in the same launch (include/dfx.h).  The index and weight tables are the library's (csrc/resize_plan.h)."""

    _OP, _INFO = "dfx_resize", ResizeInfo

    def __init__(self, src_shape_nhwc, out_hw, np_dtype, algo=RESIZE_BILINEAR, coord=COORD_HALF_PIXEL, add=False,
                 post_relu=False, force_path=RESIZE_AUTO):
        bs, ih, iw, c = src_shape_nhwc
        dt = np_dtype if isinstance(np_dtype, int) else _DT[np.dtype(np_dtype)]
        d = ResizeDesc(bs, c, ih, iw, out_hw[0], out_hw[1], dt, algo, coord, int(add), int(post_relu), force_path)
        self.desc = d
        self.src_shape = (bs, ih, iw, c)
        self.dst_shape = (bs, out_hw[0], out_hw[1], c)
        self.src_np_dtype = self.dst_np_dtype = _NP[dt]
        self._create(d)

    def submit(self, src_dev, dst_dev, add_dev=None, stream=None):
        """asynchronous; add_dev is given exactly when the handle was made with add=True and may be dst_dev"""
        _check(lib().dfx_resize_submit(self._h, _dev_ptr(src_dev), None if add_dev is None else _dev_ptr(add_dev),
                                       _dev_ptr(dst_dev), _stream_ptr(stream)))

    def submit_host(self, src_np, add_np=None):
        src = np.ascontiguousarray(src_np, dtype=self.src_np_dtype)
        assert src.shape == self.src_shape, (src.shape, self.src_shape)
        add = None if add_np is None else np.ascontiguousarray(add_np, dtype=self.dst_np_dtype)
        assert add is None or add.shape == self.dst_shape, (add.shape, self.dst_shape)
        dst = np.empty(self.dst_shape, dtype=self.dst_np_dtype)
        _check(lib().dfx_resize_submit_host(self._h, _p(src), _p(add), _p(dst)))
        return dst


class InnerProduct(_Handle):
    """dfx_fc_* handle: int8 fully-connected layer over NHWC u8 {bs, ih, iw, ic} (include/dfx.h), weights plain oihw
    {oc, ic, ih, iw} as a flattened-CHW classifier keeps them, dst {bs, oc}.  Where ic and oc are multiples of 16 the
    result equals the unfused Conv with the full-image window bit for bit."""

    _OP, _INFO, _ROUTES = "dfx_fc", FcInfo, 1

    def __init__(self, src_shape_nhwc, oc, dst_dt=DFX_U8, bia_dt=DFX_UNDEF, relu=False, rm=ROUND_NEAREST, nscales=1,
                 force_path=FC_AUTO):
        bs, ih, iw, ic = src_shape_nhwc
        d = FcDesc(bs, ic, ih, iw, oc, dst_dt, bia_dt, int(relu), rm, nscales, force_path)
        self.desc = d
        self.src_shape = (bs, ih, iw, ic)
        self.dst_shape = (bs, oc)
        self.dst_np_dtype = _NP.get(dst_dt)
        self._create(d)

    def set_weights(self, wei, scales, bia=None):
        """wei: int8 {oc, ic, ih, iw}; scales: 1 or oc floats; bia: oc entries of the descriptor's bias dtype"""
        d = self.desc
        ws = [np.ascontiguousarray(wei, dtype=np.int8), None if bia is None else np.ascontiguousarray(bia),
              np.ascontiguousarray(scales, dtype=np.float32)]
        assert ws[0].size == d.oc * d.ic * d.ih * d.iw, ws[0].shape
        assert ws[2].size == d.nscales and (bia is None or ws[1].size == d.oc)
        _check(lib().dfx_fc_set_weights(self._h, _p(ws[0]), _p(ws[1]), _p(ws[2])))


class SqueezeExcite(_Handle):
    """dfx_se_* handle: squeeze-and-excitation over NHWC u8 {bs, ih, iw, c} (include/dfx.h): global average, FC1 {cr, c}
    (relu, u8), FC2 {c, cr} (s8), a 256-entry gate table and the per-(image, channel) rescale.  SE_SCALE writes the
    rescaled tensor (dst may be src), SE_GATE the {bs, c} gate, SE_SQUEEZE the {bs, c} average (no weights)."""

    _OP, _INFO = "dfx_se", SeInfo

    def __init__(self, src_shape_nhwc, cr, mode=SE_SCALE, bia1_dt=DFX_UNDEF, bia2_dt=DFX_UNDEF, nscales1=1, nscales2=1,
                 nscales_out=1, rm=ROUND_NEAREST, force_path=SE_AUTO):
        bs, ih, iw, c = src_shape_nhwc
        d = SeDesc(bs, c, ih, iw, cr, mode, bia1_dt, bia2_dt, rm, nscales1, nscales2, nscales_out, force_path)
        self.desc = d
        self.src_shape = (bs, ih, iw, c)
        self.dst_shape = (bs, ih, iw, c) if mode == SE_SCALE else (bs, c)
        self.dst_np_dtype = np.uint8
        self._create(d)

    def set_weights(self, w1, scales1, w2, scales2, lut, out_scales, bia1=None, bia2=None):
        """w1: int8 {cr, c}; w2: int8 {c, cr}; scales1: 1 or cr floats; scales2 and out_scales: 1 or c floats; lut: 256
        uint8; biases: cr / c entries of the descriptor's bias dtypes"""
        d = self.desc
        w1, w2 = np.ascontiguousarray(w1, dtype=np.int8), np.ascontiguousarray(w2, dtype=np.int8)
        s1, s2, so = [np.ascontiguousarray(v, dtype=np.float32) for v in (scales1, scales2, out_scales)]
        lut = np.ascontiguousarray(lut, dtype=np.uint8)
        b1 = None if bia1 is None else np.ascontiguousarray(bia1)
        b2 = None if bia2 is None else np.ascontiguousarray(bia2)
        assert w1.size == d.cr * d.c and w2.size == d.c * d.cr and lut.size == 256, (w1.shape, w2.shape, lut.shape)
        assert s1.size == d.nscales1 and s2.size == d.nscales2 and so.size == d.nscales_out
        assert (b1 is None or b1.size == d.cr) and (b2 is None or b2.size == d.c)
        _check(lib().dfx_se_set_weights(self._h, _p(w1), _p(b1), _p(s1), _p(w2), _p(b2), _p(s2), _p(lut), _p(so)))


class ScaledSum(_Handle):
    """dfx_wsum_* handle: dst = post(sum_i float(src_i) * scale_i[k] + bias[k]) over NHWC tensors of one shape and mixed
    dtypes (include/dfx.h): per-tensor or per-channel scales, optional bias, ReLU and a 256-entry byte table; dst may be
    an input of its own element size.  src_dtypes / dst_dtype / lut_in: DFX_* codes or numpy dtypes."""

    _OP, _INFO = "dfx_wsum", WsumInfo

    def __init__(self, shape_nhwc, src_dtypes, dst_dtype, nscales, n_bias=0, post_relu=False, lut_in=None,
                 rm=ROUND_NEAREST, force_path=WSUM_AUTO):
        code = lambda t: t if isinstance(t, int) else _DT[np.dtype(t)]  # noqa: E731
        bs, h, w, c = shape_nhwc
        d = WsumDesc()
        d.bs, d.h, d.w, d.c, d.n_inputs = bs, h, w, c, len(src_dtypes)
        for i, (t, ns) in enumerate(zip(list(src_dtypes)[:8], list(nscales)[:8])):
            d.src_dt[i], d.nscales[i] = code(t), ns
        d.n_bias, d.dst_dt, d.round_mode, d.post_relu = n_bias, code(dst_dtype), rm, int(post_relu)
        d.lut_in_dt, d.force_path = DFX_UNDEF if lut_in is None else code(lut_in), force_path
        self.desc = d
        self.shape = self.dst_shape = (bs, h, w, c)
        self._create(d)
        self.src_np_dtypes = [_NP[d.src_dt[i]] for i in range(d.n_inputs)]
        self.dst_np_dtype = _NP[d.dst_dt]

    def set_params(self, scales, bias=None, lut=None):
        """scales: one array of nscales[i] floats per input; bias: n_bias floats; lut: 256 bytes"""
        d = self.desc
        sc = [np.ascontiguousarray(s, dtype=np.float32).reshape(-1) for s in scales]
        assert len(sc) == d.n_inputs and all(s.size == d.nscales[i] for i, s in enumerate(sc))
        b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32).reshape(-1)
        assert (b is None and d.n_bias == 0) or (b is not None and b.size == d.n_bias)
        t = None if lut is None else np.ascontiguousarray(lut).view(np.uint8).reshape(-1)
        assert t is None or t.size == 256
        ptrs = _ptr_array(sc, lambda a: a.ctypes.data)
        _check(lib().dfx_wsum_set_params(self._h, ptrs, _p(b), _p(t)))

    def submit(self, srcs_dev, dst_dev, stream=None):
        """asynchronous; srcs_dev: torch CUDA tensors (or raw pointers), dst_dev may be one of them"""
        ptrs = _ptr_array(srcs_dev, lambda t: _dev_ptr(t).value)
        _check(lib().dfx_wsum_submit(self._h, ptrs, _dev_ptr(dst_dev), _stream_ptr(stream)))

    def submit_host(self, srcs_np):
        srcs = [np.ascontiguousarray(s, dtype=t) for s, t in zip(srcs_np, self.src_np_dtypes)]
        assert len(srcs) == self.desc.n_inputs and all(s.shape == self.shape for s in srcs)
        dst = np.empty(self.dst_shape, dtype=self.dst_np_dtype)
        _check(lib().dfx_wsum_submit_host(self._h, _ptr_array(srcs, lambda a: a.ctypes.data), _p(dst)))
        return dst


class Head(_Handle):
    """dfx_head_* handle: channel top-k / argmax (mode HEAD_TOPK) or table softmax (HEAD_SOFTMAX) over a row matrix: `rows`
    rows of `c` valid channels, src_ld elements apart (include/dfx.h).  An NHWC tensor is rows = bs*h*w, src_ld = C.
    TOPK: dst_dtype is idx's (int32, or uint8 when c <= 256); submit(src, idx, val=None).  SOFTMAX: 1-byte src, dst_dtype
    float32 or uint8; set_table() first; submit(src, dst)."""

    _OP, _INFO = "dfx_head", HeadInfo

    def __init__(self, rows, c, src_dtype, dst_dtype, mode=HEAD_TOPK, k=1, src_ld=None, dst_ld=None, idx_ld=None,
                 out_scale=255.0, force_path=HEAD_AUTO):
        code = lambda t: t if isinstance(t, int) else _DT[np.dtype(t)]  # noqa: E731
        d = HeadDesc()
        d.rows, d.mode, d.src_dt, d.dst_dt, d.c, d.k = rows, mode, code(src_dtype), code(dst_dtype), c, k
        d.src_ld = c if src_ld is None else src_ld
        d.dst_ld = c if dst_ld is None else dst_ld
        d.idx_ld = k if idx_ld is None else idx_ld
        d.out_scale, d.force_path = out_scale, force_path
        self.desc = d
        self._create(d)

    def set_table(self, table):
        t = np.ascontiguousarray(table, dtype=np.uint32).reshape(-1)
        assert t.size == 256
        _check(lib().dfx_head_set_table(self._h, _p(t)))

    def submit(self, src_dev, out_dev, val_dev=None, stream=None):
        """asynchronous; torch CUDA tensors (or raw pointers); out_dev: idx (TOPK) or dst (SOFTMAX)"""
        _check(lib().dfx_head_submit(self._h, _dev_ptr(src_dev), _dev_ptr(out_dev),
                                     None if val_dev is None else _dev_ptr(val_dev), _stream_ptr(stream)))


class LayerNorm(_Handle):
    """dfx_lnorm_* handle: int8 layer norm (mode LNORM_LAYER) or RMS norm (LNORM_RMS) over a row matrix: `rows` rows of `c`
    valid channels (include/dfx.h).  src uint8 / int8, dst uint8 / int8 / float32; eps in units of the integer domain
    (lnorm_params()).  set_params(gamma, beta=None, shift=None) first; submit(src, dst)."""

    _OP, _INFO = "dfx_lnorm", LnormInfo

    def __init__(self, rows, c, src_dtype, dst_dtype, eps, mode=LNORM_LAYER, src_ld=None, dst_ld=None, force_path=LNORM_AUTO):
        code = lambda t: t if isinstance(t, int) else _DT[np.dtype(t)]  # noqa: E731
        d = LnormDesc()
        d.rows, d.mode, d.src_dt, d.dst_dt, d.c = rows, mode, code(src_dtype), code(dst_dtype), c
        d.src_ld = c if src_ld is None else src_ld
        d.dst_ld = c if dst_ld is None else dst_ld
        d.eps, d.force_path = eps, force_path
        self.desc = d
        self._create(d)

    def set_params(self, gamma, beta=None, shift=None):
        """gamma, beta: c floats (beta None: zeros); shift: c bytes of 0 .. 7 or None"""
        c = self.desc.c
        g = np.ascontiguousarray(gamma, dtype=np.float32).reshape(-1)
        b = None if beta is None else np.ascontiguousarray(beta, dtype=np.float32).reshape(-1)
        s = None if shift is None else np.ascontiguousarray(shift, dtype=np.uint8).reshape(-1)
        assert g.size == c and (b is None or b.size == c) and (s is None or s.size == c)
        _check(lib().dfx_lnorm_set_params(self._h, _p(g), _p(b), _p(s)))


class WindowOp(_Handle):
    """dfx_window_* handle: window partition (dir WINDOW_PARTITION, grid -> windows) or reverse (WINDOW_REVERSE) of an NHWC token
    grid {bs, h, w, c} (include/dfx.h): rows grid_ld elements apart on the grid side, win_ld on the window side, one dtype on
    both, bytes moved as they are.  window and shift: an int or (y, x).  The window side holds bs * n_windows matrices of
    wh * ww rows (win_rows rows in all); pad tokens of a partition are filled with pad_value.  submit(src, dst): src is the grid
    for a partition, the windows for a reverse."""

    _OP, _INFO = "dfx_window", WindowInfo

    def __init__(self, dir, bs, h, w, c, window, shift=(0, 0), order=WINDOW_ROW_MAJOR, dtype=np.int8, grid_ld=None, win_ld=None,
                 pad_value=0, force_path=WINDOW_AUTO):
        code = lambda t: t if isinstance(t, int) else _DT[np.dtype(t)]  # noqa: E731
        d = WindowDesc()
        d.dir, d.dt, d.bs, d.h, d.w, d.c = dir, code(dtype), bs, h, w, c
        d.wh, d.ww = _pair(window)
        d.shift_y, d.shift_x = _pair(shift)
        d.order = order
        d.grid_ld = c if grid_ld is None else grid_ld
        d.win_ld = c if win_ld is None else win_ld
        d.pad_value, d.force_path = int(pad_value) & 0xffffffff, force_path
        self.desc = d
        if d.wh >= 1 and d.ww >= 1:            # (the library refuses the rest)
            self.hp, self.wp = -(-h // d.wh) * d.wh, -(-w // d.ww) * d.ww
            self.n_windows = (self.hp // d.wh) * (self.wp // d.ww)
            self.win_rows = bs * self.hp * self.wp
        self._create(d)


class Linear(_Handle):
    """dfx_linear_* handle: int8 linear layer over a row matrix of tokens (include/dfx.h): `rows` rows of `k` valid uint8 /
    int8 elements, src_ld apart, times an int8 {n, k} weight (an nn.Linear weight), per-n bias and scales, dst rows dst_ld
    apart in any of the four dtypes.  table: the index type (uint8 / int8) of an optional 256-byte table behind the requant
    (gelu_table()); set_weights() and, with a table, set_table() first; submit(src, dst)."""

    _OP, _INFO, _ROUTES = "dfx_linear", LinearInfo, 1

    def __init__(self, rows, k, n, src_dtype=np.int8, dst_dtype=np.int8, bia_dt=DFX_UNDEF, relu=False, rm=ROUND_NEAREST, nscales=1,
                 src_ld=None, dst_ld=None, table=None, force_path=LINEAR_AUTO):
        code = lambda t: t if isinstance(t, int) else _DT[np.dtype(t)]  # noqa: E731
        d = LinearDesc()
        d.rows, d.k, d.n, d.src_dt, d.dst_dt, d.bia_dt = rows, k, n, code(src_dtype), code(dst_dtype), code(bia_dt)
        d.relu, d.round_mode, d.nscales = int(relu), rm, nscales
        d.lut_in_dt = DFX_UNDEF if table is None else code(table)
        d.force_path = force_path
        d.src_ld = k if src_ld is None else src_ld
        d.dst_ld = n if dst_ld is None else dst_ld
        self.desc = d
        self.src_shape, self.dst_shape = (rows, k), (rows, n)
        self.src_np_dtype, self.dst_np_dtype = _NP.get(d.src_dt), _NP.get(d.dst_dt)
        self._create(d)

    def set_weights(self, wei, scales, bia=None):
        """wei: int8 {n, k}; scales: 1 or n floats; bia: n entries of the descriptor's bias dtype"""
        d = self.desc
        ws = [np.ascontiguousarray(wei, dtype=np.int8), None if bia is None else np.ascontiguousarray(bia),
              np.ascontiguousarray(scales, dtype=np.float32)]
        assert ws[0].size == d.n * d.k, ws[0].shape
        assert ws[2].size == d.nscales and (bia is None or ws[1].size == d.n)
        _check(lib().dfx_linear_set_weights(self._h, _p(ws[0]), _p(ws[1]), _p(ws[2])))

    def set_table(self, table):
        """256 bytes (uint8, or int8 viewed as bytes)"""
        t = np.ascontiguousarray(table).view(np.uint8).reshape(-1)
        assert t.size == 256
        _check(lib().dfx_linear_set_table(self._h, _p(t)))


class PatchEmbed(_Handle):
    """dfx_patchembed_* handle: int8 patch embedding (include/dfx.h): a non-overlapping ph x pw conv over an NHWC uint8 / int8
    image as one GEMM that writes the token matrix {bs * img_rows, dst_ld}: token t of image b at row b * img_rows + tok_offset
    + t.  Weights plain oihw {oc, ic, ph, pw}.  table=True: a per-(token, channel) f32 table in accumulator units
    (patch_embed_table()) in the place of the bias; set_prefix(): tok_offset rows of dst's dtype stored in front of every
    image's tokens (patch_embed_prefix()).  tokens_hw defaults to (ih // ph, iw // pw)."""

    _OP, _INFO, _ROUTES = "dfx_patchembed", PatchEmbedInfo, 1

    def __init__(self, src_shape_nhwc, oc, patch, tokens_hw=None, src_dtype=np.uint8, dst_dtype=np.int8, bia_dt=DFX_UNDEF, relu=False,
                 rm=ROUND_NEAREST, nscales=1, table=False, tok_offset=0, img_rows=None, dst_ld=None, force_path=PATCHEMBED_AUTO):
        code = lambda t: t if isinstance(t, int) else _DT[np.dtype(t)]  # noqa: E731
        bs, ih, iw, ic = src_shape_nhwc
        ph, pw = patch
        th, tw = (ih // ph, iw // pw) if tokens_hw is None else tokens_hw
        d = PatchEmbedDesc()
        d.bs, d.ih, d.iw, d.ic, d.ph, d.pw, d.th, d.tw, d.oc = bs, ih, iw, ic, ph, pw, th, tw, oc
        d.src_dt, d.dst_dt, d.bia_dt = code(src_dtype), code(dst_dtype), code(bia_dt)
        d.relu, d.round_mode, d.nscales, d.table, d.tok_offset, d.force_path = int(relu), rm, nscales, int(table), tok_offset, force_path
        d.img_rows = tok_offset + th * tw if img_rows is None else img_rows
        d.dst_ld = oc if dst_ld is None else dst_ld
        self.desc = d
        self.src_shape, self.dst_shape = (bs, ih, iw, ic), (bs * d.img_rows, d.dst_ld)
        self.src_np_dtype, self.dst_np_dtype = _NP.get(d.src_dt), _NP.get(d.dst_dt)
        self._create(d)

    def set_weights(self, wei, scales, bia=None):
        """wei: int8 {oc, ic, ph, pw}; scales: 1 or oc floats; bia: oc entries of the descriptor's bias dtype"""
        d = self.desc
        ws = [np.ascontiguousarray(wei, dtype=np.int8), None if bia is None else np.ascontiguousarray(bia),
              np.ascontiguousarray(scales, dtype=np.float32)]
        assert ws[0].size == d.oc * d.ic * d.ph * d.pw, ws[0].shape
        assert ws[2].size == d.nscales and (bia is None or ws[1].size == d.oc)
        _check(lib().dfx_patchembed_set_weights(self._h, _p(ws[0]), _p(ws[1]), _p(ws[2])))

    def set_table(self, table):
        """float32 {th * tw, oc}, accumulator units"""
        d = self.desc
        t = np.ascontiguousarray(table, dtype=np.float32)
        assert t.shape == (d.th * d.tw, d.oc), t.shape
        _check(lib().dfx_patchembed_set_table(self._h, _p(t), d.oc))

    def set_prefix(self, rows):
        """{tok_offset, oc} of dst's dtype, stored verbatim"""
        d = self.desc
        r = np.ascontiguousarray(rows, dtype=self.dst_np_dtype)
        assert r.size == d.tok_offset * d.oc, r.shape
        _check(lib().dfx_patchembed_set_prefix(self._h, _p(r)))


class TopK(Head):
    def __init__(self, rows, c, src_dtype, idx_dtype=np.int32, k=1, **kw):
        Head.__init__(self, rows, c, src_dtype, idx_dtype, mode=HEAD_TOPK, k=k, **kw)


class Softmax(Head):
    def __init__(self, rows, c, src_dtype, dst_dtype=np.float32, table=None, **kw):
        Head.__init__(self, rows, c, src_dtype, dst_dtype, mode=HEAD_SOFTMAX, **kw)
        if table is not None:
            self.set_table(table)


class SelectTopK(_Handle):
    """dfx_select_* handle: the k best elements of every image of an NHWC u8 / s8 score tensor {bs, h, w, src_ld} (c valid
    channels), optionally only 3x3 local maxima (peak=SELECT_PEAK3) and only elements >= min_val, ordered by (value
    descending, element index ascending); rows of up to four byte maps gathered behind it (include/dfx.h).  gather: a
    (row_bytes, pixel_stride_bytes) pair per map."""

    _OP, _INFO = "dfx_select", SelectInfo

    def __init__(self, bs, h, w, c, src_dtype, k, src_ld=None, idx_ld=None, peak=SELECT_ALL, min_val=None, gather=(),
                 force_path=SELECT_AUTO):
        d = SelectDesc()
        d.bs, d.h, d.w, d.c, d.k, d.peak, d.force_path = bs, h, w, c, k, peak, force_path
        d.src_dt = src_dtype if isinstance(src_dtype, int) else _DT[np.dtype(src_dtype)]
        d.src_ld = c if src_ld is None else src_ld
        d.idx_ld = k if idx_ld is None else idx_ld
        d.min_val = (-128 if d.src_dt == DFX_S8 else 0) if min_val is None else min_val
        d.n_gather = len(gather)
        for i, (rb, st) in enumerate(list(gather)[:4]):
            d.row_bytes[i], d.pixel_stride_bytes[i] = rb, st
        self.desc = d
        self._create(d)

    def submit(self, src_dev, idx_dev, count_dev, val_dev=None, gather_src=(), gather_dst=(), stream=None):
        """asynchronous; torch CUDA tensors (or raw pointers); idx int32 {bs, idx_ld}, count int32 {bs}, val of src's dtype"""
        gs = _ptr_array(gather_src, lambda t: _dev_ptr(t).value) if len(gather_src) else None
        gd = _ptr_array(gather_dst, lambda t: _dev_ptr(t).value) if len(gather_dst) else None
        _check(lib().dfx_select_submit(self._h, _dev_ptr(src_dev), _dev_ptr(idx_dev),
                                       None if val_dev is None else _dev_ptr(val_dev), _dev_ptr(count_dev), gs, gd,
                                       _stream_ptr(stream)))


class BoxNms(_Handle):
    """dfx_nms_* handle: greedy NMS over n <= 4096 candidates per image in priority order (what SelectTopK emits), on boxes
    (mode NMS_BOXES) or with the boxes decoded from anchors and 1-byte deltas through two tables (NMS_DECODE, box_tables());
    per-class or class-agnostic; at most max_out survivors (include/dfx.h)."""

    _OP, _INFO = "dfx_nms", NmsInfo

    def __init__(self, bs, n, max_out, iou_thr, mode=NMS_BOXES, per_class=False, classes=1, anchors_per_pixel=1, n_anchors=None,
                 row_bytes=None, idx_ld=None, keep_ld=None, clip=None, force_path=NMS_AUTO):
        d = NmsDesc()
        d.bs, d.n, d.max_out, d.mode, d.per_class, d.classes, d.force_path = bs, n, max_out, mode, int(per_class), classes, force_path
        d.anchors_per_pixel = anchors_per_pixel
        d.n_anchors = (2 ** 31 - 1) // max(1, classes) if n_anchors is None else n_anchors
        d.row_bytes = 4 * anchors_per_pixel if row_bytes is None else row_bytes
        d.idx_ld = n if idx_ld is None else idx_ld
        d.keep_ld = max_out if keep_ld is None else keep_ld
        d.iou_thr = iou_thr
        d.clip_w, d.clip_h = (0.0, 0.0) if clip is None else clip
        self.desc = d
        self._create(d)

    def submit(self, keep_dev, count_dev, boxes=None, idx=None, deltas=None, anchors=None, tab_c=None, tab_s=None, count_in=None,
               boxes_out=None, stream=None):
        """asynchronous; torch CUDA tensors (or raw pointers); keep int32 {bs, keep_ld}, count int32 {bs}"""
        io = NmsIo()
        for name, t in (("boxes", boxes), ("idx", idx), ("deltas", deltas), ("anchors", anchors), ("tab_c", tab_c), ("tab_s", tab_s),
                        ("count_in", count_in), ("keep", keep_dev), ("count", count_dev), ("boxes_out", boxes_out)):
            setattr(io, name, None if t is None else _dev_ptr(t).value)
        _check(lib().dfx_nms_submit(self._h, ctypes.byref(io), _stream_ptr(stream)))


class RoiAlign(_Handle):
    """dfx_roialign_* handle: torchvision's roi_align over 1 .. 4 NHWC feature maps of one dtype (u8, s8, f32), the level of a
    RoI chosen by its area against `level_area_thr` (roi_level_thresholds()).  level_shapes: (h, w) per level of tensors
    {bs, h, w, src_ld}; mode ROI_BATCHED takes BoxNms's boxes_out {bs, n, 4} and count, ROI_LIST boxes {n, 4} and batch_idx
    {n}; dst {R, ph, pw, dst_ld} (include/dfx.h)."""

    _OP, _INFO = "dfx_roialign", RoiAlignInfo

    def __init__(self, bs, n, level_shapes, c, dtype, out_hw, spatial_scales, sampling_ratio=2, aligned=False, mode=ROI_BATCHED,
                 level_area_thr=(), src_ld=None, dst_ld=None, force_path=ROIALIGN_AUTO):
        d = RoiAlignDesc()
        d.bs, d.n, d.mode, d.levels, d.c = bs, n, mode, len(level_shapes), c
        d.dt = dtype if isinstance(dtype, int) else _DT[np.dtype(dtype)]
        for l, (h, w) in enumerate(list(level_shapes)[:4]):
            d.h[l], d.w[l] = h, w
            d.src_ld[l] = c if src_ld is None else src_ld[l]
            d.spatial_scale[l] = spatial_scales[l]
        for i, t in enumerate(list(level_area_thr)[:3]):
            d.level_area_thr[i] = t
        d.ph, d.pw = out_hw
        d.sampling_ratio, d.aligned, d.force_path = sampling_ratio, int(aligned), force_path
        d.dst_ld = c if dst_ld is None else dst_ld
        self.desc = d
        self._create(d)

    def submit(self, levels_dev, boxes_dev, dst_dev, count=None, batch_idx=None, stream=None):
        """asynchronous; torch CUDA tensors (or raw pointers); levels_dev: one tensor per level"""
        io = RoiAlignIo()
        for l, t in enumerate(levels_dev):
            io.src[l] = None if t is None else _dev_ptr(t).value
        for name, t in (("boxes", boxes_dev), ("count", count), ("batch_idx", batch_idx), ("dst", dst_dev)):
            setattr(io, name, None if t is None else _dev_ptr(t).value)
        _check(lib().dfx_roialign_submit(self._h, ctypes.byref(io), _stream_ptr(stream)))


class MatMul(_Handle):
    """dfx_bmm_* handle: batched int8 matrix product of two device tensors (include/dfx.h): C[g] = requant(A[g] . B[g]^T)
    (trans_b, B {N, K}: Q.K^T) or A[g] . B[g] (B {K, N}: P.V) over batch = (batch0, batch1) matrices.  a_strides / b_strides /
    c_strides are (s0, s1, ld) in elements (None: densely packed); a batch stride of 0 broadcasts A or B.  A u8 or s8, B s8,
    C any of the four dtypes.  set_scales() first; submit(a, b, c)."""

    _OP, _INFO, _ROUTES = "dfx_bmm", BmmInfo, 1

    def __init__(self, batch, m, n, k, a_dtype=np.uint8, dst_dtype=np.int8, trans_b=True, a_strides=None, b_strides=None,
                 c_strides=None, relu=False, rm=ROUND_NEAREST, nscales=1, b_dtype=np.int8, force_path=BMM_AUTO, scales=None, bias=None):
        code = lambda t: t if isinstance(t, int) else _DT[np.dtype(t)]  # noqa: E731
        batch0, batch1 = (1, batch) if isinstance(batch, int) else batch
        brows, bcols = (n, k) if trans_b else (k, n)

        def dense(rows, cols):
            return batch1 * rows * cols, rows * cols, cols

        d = BmmDesc()
        d.batch0, d.batch1, d.m, d.n, d.k, d.trans_b = batch0, batch1, m, n, k, int(bool(trans_b))
        d.a_dt, d.b_dt, d.dst_dt = code(a_dtype), code(b_dtype), code(dst_dtype)
        d.relu, d.round_mode, d.nscales, d.force_path = int(relu), rm, nscales, force_path
        d.a_s0, d.a_s1, d.lda = dense(m, k) if a_strides is None else a_strides
        d.b_s0, d.b_s1, d.ldb = dense(brows, bcols) if b_strides is None else b_strides
        d.c_s0, d.c_s1, d.ldc = dense(m, n) if c_strides is None else c_strides
        self.desc = d
        self._create(d)
        if scales is not None:
            self.set_scales(scales)
        if bias is not None:
            self.set_bias(*bias) if isinstance(bias, tuple) else self.set_bias(bias)

    def set_scales(self, scales):
        """1 or n floats (the descriptor's nscales); may be called again"""
        s = np.ascontiguousarray(scales, dtype=np.float32).reshape(-1)
        assert s.size == self.desc.nscales, (s.size, self.desc.nscales)
        _check(lib().dfx_bmm_set_scales(self._h, _p(s)))

    def set_bias(self, table, periods=(1, 1), strides=None):
        """the logit bias (include/dfx.h, dfx_logit_bias_desc): f32 values in ACCUMULATOR units added before the scale, finite
        or -inf; matrix (b0, b1) uses table (b0 % periods[0], b1 % periods[1]).  strides None: a dense {p0, p1, m, n} table,
        or {p0, p1, n} for one row broadcast over m; else (s0, s1, ld) in floats over the flat table (ld 0: one row).  The
        values are copied; may be called again; table None clears the bias.  Not while a submit is in flight."""
        if table is None:
            _check(lib().dfx_bmm_set_bias(self._h, None, None))
            return
        b, t = _logit_bias_args(table, periods, strides, self.desc.m, self.desc.n)
        _check(lib().dfx_bmm_set_bias(self._h, ctypes.byref(b), _p(t)))

    def submit(self, a_dev, b_dev, c_dev, stream=None):
        """asynchronous; torch CUDA tensors (or raw pointers)"""
        _check(lib().dfx_bmm_submit(self._h, _dev_ptr(a_dev), _dev_ptr(b_dev), _dev_ptr(c_dev), _stream_ptr(stream)))


class Attention(_Handle):
    """dfx_attn_* handle: int8 attention over batch = (batch0, batch1) matrices (include/dfx.h): O[g] = requant(softmax(
    requant(Q[g] . K[g]^T)) . V[g]), defined as MatMul -> Softmax (u8) -> MatMul and bit-identical to that chain; on the fused
    path it is one launch with the logits and the probabilities kept on chip.  q_strides / k_strides / v_strides / o_strides
    are (s0, s1, ld) in elements (None: densely packed; attention_strides() for head-sliced tensors).  Q u8 or s8, K and V s8,
    O any of the four dtypes.  set_table() and set_scales() first; submit(q, k, v, o)."""

    _OP, _INFO = "dfx_attn", AttnInfo

    def __init__(self, batch, tq, tk, d, dv, q_dtype=np.int8, dst_dtype=np.int8, q_strides=None, k_strides=None, v_strides=None,
                 o_strides=None, relu=False, rm=ROUND_NEAREST, nscales=1, prob_scale=255.0, k_dtype=np.int8, v_dtype=np.int8,
                 force_path=ATTN_AUTO, table=None, logit_scale=None, out_scales=None, bias=None):
        code = lambda t: t if isinstance(t, int) else _DT[np.dtype(t)]  # noqa: E731
        batch0, batch1 = (1, batch) if isinstance(batch, int) else batch

        def dense(rows, cols):
            return batch1 * rows * cols, rows * cols, cols

        dsc = AttnDesc()
        dsc.batch0, dsc.batch1, dsc.tq, dsc.tk, dsc.d, dsc.dv = batch0, batch1, tq, tk, d, dv
        dsc.q_dt, dsc.k_dt, dsc.v_dt, dsc.dst_dt = code(q_dtype), code(k_dtype), code(v_dtype), code(dst_dtype)
        dsc.relu, dsc.round_mode, dsc.nscales, dsc.force_path = int(relu), rm, nscales, force_path
        dsc.prob_scale = prob_scale
        dsc.q_s0, dsc.q_s1, dsc.ldq = dense(tq, d) if q_strides is None else q_strides
        dsc.k_s0, dsc.k_s1, dsc.ldk = dense(tk, d) if k_strides is None else k_strides
        dsc.v_s0, dsc.v_s1, dsc.ldv = dense(tk, dv) if v_strides is None else v_strides
        dsc.o_s0, dsc.o_s1, dsc.ldo = dense(tq, dv) if o_strides is None else o_strides
        self.desc = dsc
        self._create(dsc)
        if table is not None:
            self.set_table(table)
        if logit_scale is not None and out_scales is not None:
            self.set_scales(logit_scale, out_scales)
        if bias is not None:
            self.set_bias(*bias) if isinstance(bias, tuple) else self.set_bias(bias)

    def set_table(self, table):
        """256 uint32 entries (softmax_table(step, tk)); may be called again"""
        t = np.ascontiguousarray(table, dtype=np.uint32).reshape(-1)
        assert t.size == 256, t.size
        _check(lib().dfx_attn_set_table(self._h, _p(t)))

    def set_scales(self, logit_scale, out_scales):
        """the logits' scale and 1 or dv out scales (the descriptor's nscales); may be called again"""
        s = np.ascontiguousarray(out_scales, dtype=np.float32).reshape(-1)
        assert s.size == self.desc.nscales, (s.size, self.desc.nscales)
        _check(lib().dfx_attn_set_scales(self._h, ctypes.c_float(float(np.float32(logit_scale))), _p(s)))

    def set_bias(self, table, periods=(1, 1), strides=None):
        """the logit bias of Q . K^T (include/dfx.h): MatMul.set_bias with m = tq, n = tk; attention_bias() builds the table
        from a relative-position bias, a window mask and a key-padding mask.  table None clears it."""
        if table is None:
            _check(lib().dfx_attn_set_bias(self._h, None, None))
            return
        b, t = _logit_bias_args(table, periods, strides, self.desc.tq, self.desc.tk)
        _check(lib().dfx_attn_set_bias(self._h, ctypes.byref(b), _p(t)))

    def requant(self):
        """(logits route, context route) as the last set_scales / set_bias proved them; (-1, -1) before set_scales"""
        i = self.info()
        return i.route_logits, i.route_context

    def submit(self, q_dev, k_dev, v_dev, o_dev, stream=None):
        """asynchronous; torch CUDA tensors (or raw pointers)"""
        _check(lib().dfx_attn_submit(self._h, _dev_ptr(q_dev), _dev_ptr(k_dev), _dev_ptr(v_dev), _dev_ptr(o_dev), _stream_ptr(stream)))


class DwPwConv(_Handle):
    """dfx_dwpw_* handle: depthwise conv (dst u8) + pointwise 1x1 conv over NHWC u8, the tensor between the two kept on
    chip on the fused path (include/dfx.h).  The result equals DwConv (u8) followed by the unfused 1x1 Conv bit for bit.
    out_hw defaults to the conv's (in + 2 * pad - k) // stride + 1."""

    _OP, _INFO, _ROUTES = "dfx_dwpw", DwPwInfo, 2

    def __init__(self, src_shape_nhwc, kernel, oc, stride=(1, 1), pad=(1, 1), out_hw=None, dst_dt=DFX_U8, bia0_dt=DFX_UNDEF,
                 bia1_dt=DFX_UNDEF, relu=False, rm0=ROUND_NEAREST, rm1=ROUND_NEAREST, nscales0=1, nscales1=1,
                 force_path=DWPW_AUTO):
        bs, ih, iw, c = src_shape_nhwc
        kh, kw = kernel
        if out_hw is None:
            out_hw = _conv_out_hw(ih, iw, kernel, stride, pad)
        d = DwPwDesc(bs, c, ih, iw, out_hw[0], out_hw[1], kh, kw, stride[0], stride[1], pad[0], pad[1], oc, dst_dt,
                     bia0_dt, bia1_dt, int(relu), rm0, rm1, nscales0, nscales1, force_path)
        self.desc = d
        self.src_shape = (bs, ih, iw, c)
        self.dst_shape = (bs, out_hw[0], out_hw[1], oc)
        self.dst_np_dtype = _NP.get(dst_dt)
        self._create(d)

    def set_weights(self, wei_dw, scales0, wei_pw_blk, scales1, bia0=None, bia1=None):
        """wei_dw: int8 {c, kh, kw}; wei_pw_blk: {oc, c, 1, 1} in OIhw4i16o4i order (reorder_oihw_to_blocked)"""
        ws = [np.ascontiguousarray(wei_dw, dtype=np.int8), None if bia0 is None else np.ascontiguousarray(bia0),
              np.ascontiguousarray(scales0, dtype=np.float32), np.ascontiguousarray(wei_pw_blk, dtype=np.int8),
              None if bia1 is None else np.ascontiguousarray(bia1), np.ascontiguousarray(scales1, dtype=np.float32)]
        assert ws[0].size == self.desc.c * self.desc.kh * self.desc.kw, ws[0].shape
        assert ws[2].size == self.desc.nscales0 and ws[5].size == self.desc.nscales1
        assert (bia0 is None or ws[1].size == self.desc.c) and (bia1 is None or ws[4].size == self.desc.oc)
        _check(lib().dfx_dwpw_set_weights(self._h, *[_p(w) for w in ws]))


class Concat(_Handle):
    """dfx_concat_* handle: the op_concat<T> of the reference (src/op_concat.h:28-61)."""

    _OP = "dfx_concat"

    def __init__(self, bs, h, w, channels, np_dtype, post_relu=False):
        self.channels = list(channels)
        self._ch = (ctypes.c_int32 * len(channels))(*channels)
        d = ConcatDesc(len(channels), bs, h, w, _DT[np.dtype(np_dtype)], int(post_relu), self._ch)
        self.np_dtype = np.dtype(np_dtype)
        self.dst_shape = (bs, h, w, sum(channels))
        self._create(d)

    def submit(self, srcs_dev, dst_dev, stream=None):
        ptrs = _ptr_array(srcs_dev, lambda t: _dev_ptr(t).value)
        _check(lib().dfx_concat_submit(self._h, ptrs, _dev_ptr(dst_dev), _stream_ptr(stream)))

    def submit_gathered(self, gathered_dev, offsets, dst_dev, stream=None):
        offs = (ctypes.c_uint64 * len(offsets))(*offsets)
        _check(lib().dfx_concat_submit_gathered(self._h, _dev_ptr(gathered_dev), offs,
                                                _dev_ptr(dst_dev), _stream_ptr(stream)))

    def submit_host(self, srcs_np):
        srcs = [np.ascontiguousarray(s, dtype=self.np_dtype) for s in srcs_np]
        dst = np.empty(self.dst_shape, dtype=self.np_dtype)
        _check(lib().dfx_concat_submit_host(self._h, _ptr_array(srcs, lambda a: a.ctypes.data), _p(dst)))
        return dst
