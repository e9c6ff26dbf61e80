"""deep-fusion_amd -- MI355X (gfx950) implementation of deep-fusion's hot path.

The product is the C-ABI shared library libdfx_hip.so (include/dfx.h) built from
csrc/, plus the C++ drop-in layer in host/ that re-implements the reference's
include/deepfusion.h API on top of it.  This Python package is plumbing only: it
builds the library and binds the C ABI with ctypes so tests and bench.py can
drive it with torch-owned device memory and streams.  There is no Python or CPU
compute path: every op call fails loudly when the HIP library is missing.

Import with ``importlib.import_module("deep-fusion_amd")`` (the directory name
carries a hyphen).
"""
from .capi import (  # noqa: F401
    DFX_F32, DFX_S32, DFX_S8, DFX_U8, DFX_UNDEF, ROUND_NEAREST, ROUND_DOWN,
    VARIANT_GENERIC, VARIANT_MFMA_FUSED, VARIANT_MFMA_CONV, VARIANT_MFMA_STREAM, DfxError, ConvDesc, ConvInfo, ConvSched, Conv, Concat, Pool, EltwiseSum,
    FMT_NHWC, FMT_NCHW, REORDER_FLAT, REORDER_GENERIC, REORDER_SMALLC, REORDER_TRANSPOSE, ReorderDesc, ReorderInfo, Reorder,
    ROUTE_EXACT, ROUTE_FAST, ROUTE_MAGIC, ROUTE_FMA,
    CATCONV_AUTO, CATCONV_FUSED, CATCONV_TWO_LAUNCH, CatConvDesc, CatConvInfo, ConcatConv,
    DWCONV_AUTO, DWCONV_WINDOW, DWCONV_GENERIC, DwConvDesc, DwConvInfo, DwConv,
    GCONV_AUTO, GCONV_MFMA, GCONV_GENERIC, GConvDesc, GConvInfo, GroupConv,
    IMGCONV_AUTO, IMGCONV_MFMA, IMGCONV_GENERIC, ImgConvDesc, ImgConvInfo, ImageConv,
    DECONV_AUTO, DECONV_MFMA, DECONV_GENERIC, DeconvDesc, DeconvInfo, Deconv, deconv_out_hw,
    DILCONV_AUTO, DILCONV_MFMA, DILCONV_GENERIC, DilConvDesc, DilConvInfo, DilatedConv, dilconv_out_hw,
    RESIZE_AUTO, RESIZE_BAND, RESIZE_GENERIC, RESIZE_NEAREST, RESIZE_BILINEAR, COORD_HALF_PIXEL, COORD_ALIGN_CORNERS,
    COORD_ASYMMETRIC, ResizeDesc, ResizeInfo, Resize,
    FC_AUTO, FC_MFMA, FC_GENERIC, FcDesc, FcInfo, InnerProduct,
    SE_AUTO, SE_BAND, SE_GENERIC, SE_SCALE, SE_GATE, SE_SQUEEZE, SeDesc, SeInfo, SqueezeExcite,
    WSUM_AUTO, WSUM_VEC, WSUM_GENERIC, WsumDesc, WsumInfo, ScaledSum, wsum_launches,
    HEAD_TOPK, HEAD_SOFTMAX, HEAD_AUTO, HEAD_PIXEL, HEAD_ROW, HEAD_GENERIC, HeadDesc, HeadInfo, Head, TopK, Softmax,
    head_launches, softmax_table,
    SELECT_ALL, SELECT_PEAK3, SELECT_AUTO, SELECT_HIST, SELECT_GENERIC, SELECT_MAX_K, SelectDesc, SelectInfo, SelectTopK,
    select_launches,
    NMS_BOXES, NMS_DECODE, NMS_AUTO, NMS_MASK, NMS_GENERIC, NMS_MAX_N, NmsDesc, NmsIo, NmsInfo, BoxNms, nms_launches, box_tables,
    ROI_BATCHED, ROI_LIST, ROIALIGN_AUTO, ROIALIGN_TILE, ROIALIGN_GENERIC, RoiAlignDesc, RoiAlignIo, RoiAlignInfo, RoiAlign,
    roialign_launches, roi_level_thresholds,
    BMM_AUTO, BMM_MFMA, BMM_GENERIC, BmmDesc, BmmInfo, MatMul, bmm_launches, attention_strides, LogitBiasDesc, attention_bias,
    ATTN_AUTO, ATTN_FUSED, ATTN_CHAIN, AttnDesc, AttnInfo, Attention, attn_launches,
    LNORM_LAYER, LNORM_RMS, LNORM_AUTO, LNORM_ROW, LNORM_GENERIC, LNORM_MAX_C, LNORM_MAX_SHIFT, LnormDesc, LnormInfo, LayerNorm,
    lnorm_launches, lnorm_params,
    LINEAR_AUTO, LINEAR_TILE, LINEAR_GENERIC, LinearDesc, LinearInfo, Linear, linear_launches, gelu_table,
    PATCHEMBED_AUTO, PATCHEMBED_TILE, PATCHEMBED_GENERIC, PatchEmbedDesc, PatchEmbedInfo, PatchEmbed, patchembed_launches,
    patch_embed_table, patch_embed_prefix,
    WINDOW_PARTITION, WINDOW_REVERSE, WINDOW_ROW_MAJOR, WINDOW_COL_MAJOR, WINDOW_AUTO, WINDOW_ROW, WINDOW_GENERIC,
    WINDOW_MAX_HW, WINDOW_MAX_WIN, WINDOW_MAX_PADDED, WindowDesc, WindowInfo, WindowOp, window_launches, swin_shift_mask,
    swin_relative_bias,
    DWPW_AUTO, DWPW_FUSED, DWPW_TWO_LAUNCH, DwPwDesc, DwPwInfo, DwPwConv,
    lib, lib_path, build, reorder_oihw_to_blocked, declared_symbols,
)
