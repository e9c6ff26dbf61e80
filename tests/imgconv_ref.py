"""Reference, data and case tables of the first-layer conv tests (pure numpy, needs no GPU).

The op is defined by the existing ops: it equals the grouped conv with groups = 1 and, where oc is a multiple of 16 and
the output size is the conv's, the unfused dense conv on the image zero-padded to 16 channels with zero weights on the
channels >= ic.  imgconv_ref is an independent numpy formulation -- an int64 window sum (a strided window view of the
zero-padded image contracted with the plain oihw weights in one einsum), then refmath's _requant / _store, unchanged --
which tests/test_imgconv_cpu.py pins against the C oracle's dense conv and against gconv_ref, and
tests/test_gpu_imgconv.py compares the GPU against, bit for bit.
"""
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

import cases as C
from dwconv_ref import EDGES, EDGE_CHANNEL, LIMIT, OPTIONS  # noqa: F401  (the depthwise op's option rows and proof edges)
from refmath import _requant, _store

F32, S32, S8, U8, UNDEF = C.F32, C.S32, C.S8, C.U8, C.UNDEF
MFMA, GENERIC = 0, 1            # DFX_IMGCONV_MFMA / DFX_IMGCONV_GENERIC
MFMA_WINDOWS = (((7, 7), (2, 2)), ((3, 3), (1, 1)), ((3, 3), (2, 2)))
MFMA_OC = (32, 64, 96, 128)


@dataclass(frozen=True)
class ICase:
    name: str
    bs: int
    c: int                                        # input channels, 1 .. 4
    ih: int
    iw: int
    oc: int
    k: Tuple[int, int] = (3, 3)
    stride: Tuple[int, int] = (1, 1)
    pad: Tuple[int, int] = (1, 1)                 # pad_t, pad_l
    out_hw: Optional[Tuple[int, int]] = None      # None: the conv's (in + 2 * pad - k) // stride + 1
    dst_dt: int = U8
    bia_dt: int = S32
    relu: bool = True
    rm: int = 0
    per_channel: bool = False
    wide: bool = False                            # full-range data, scales that reach both saturation ends
    seed: int = 1234

    @property
    def oh(self):
        return self.out_hw[0] if self.out_hw else (self.ih + 2 * self.pad[0] - self.k[0]) // self.stride[0] + 1

    @property
    def ow(self):
        return self.out_hw[1] if self.out_hw else (self.iw + 2 * self.pad[1] - self.k[1]) // self.stride[1] + 1

    @property
    def mfma_class(self):
        return ((self.k, self.stride) in MFMA_WINDOWS and self.c in (3, 4) and self.pad[0] <= self.k[0] - 1
                and self.pad[1] <= self.k[1] - 1 and self.oc % 32 == 0 and self.oc <= 128)

    @property
    def dense_expressible(self):
        """the dense conv (symmetric padding, derived output size, channel blocks of 16) can express the case on the
        image padded to 16 channels"""
        return self.out_hw is None and self.oc % 16 == 0

    def ident(self):
        return "%s-n%d-c%d-%dx%d-oc%d-k%dx%d-s%dx%d-p%d,%d-o%dx%d-%s-b%s-r%d-m%d-pc%d%s" % (
            self.name, self.bs, self.c, self.ih, self.iw, self.oc, self.k[0], self.k[1], self.stride[0],
            self.stride[1], self.pad[0], self.pad[1], self.oh, self.ow, C.NAME_OF[self.dst_dt], C.NAME_OF[self.bia_dt],
            self.relu, self.rm, self.per_channel, "-wide" if self.wide else "")


def generate(case):
    """-> dict(src NHWC u8, w s8 {oc, ic, kh, kw}, bia, scales).  Reference-range data (cases.py), or "wide": full-range
    activations and weights with -128 and 127 present, and scales eight times the size that centres the output, so
    that both saturation ends of a 1-byte dst are reached.  The weights are random per (o, i, tap)."""
    rng = np.random.default_rng(case.seed)
    kh, kw = case.k
    if case.wide:
        src = rng.integers(0, 256, (case.bs, case.ih, case.iw, case.c)).astype(np.uint8)
        w = rng.integers(-128, 128, (case.oc, case.c, kh, kw)).astype(np.int8)
        w[0].flat[0] = -128
        w[case.oc - 1].flat[-1] = 127
    else:
        src = rng.integers(0, 17, (case.bs, case.ih, case.iw, case.c)).astype(np.uint8)
        w = rng.integers(-10, 11, (case.oc, case.c, kh, kw)).astype(np.int8)
    amp = (74.0 * 147.0 / 8.0 if case.wide else 6.0 * 9.0) * np.sqrt(kh * kw * case.c)
    s = np.float32(80.0 / amp)
    if case.per_channel:
        scales = (s * (0.5 + np.arange(case.oc) / case.oc)).astype(np.float32)
    else:
        scales = np.array([s], dtype=np.float32)
    return dict(src=src, w=w, bia=C._bias(rng, case.oc, case.bia_dt, case.wide), scales=scales)


def imgconv_acc(src, w, stride, pad, out_hw, rows=None):
    """exact int64 accumulators {bs, oh (or len(rows)), ow, oc}: every output pixel's window of the zero-padded image,
    as a strided view, contracted with the plain oihw weights; rows: the output rows to compute (all by default)"""
    bs, ih, iw, c = src.shape
    oc, ic, kh, kw = w.shape
    assert c == ic
    oh, ow = out_hw
    need_h = max((oh - 1) * stride[0] + kh, pad[0] + ih)
    need_w = max((ow - 1) * stride[1] + kw, pad[1] + iw)
    buf = np.zeros((bs, need_h, need_w, c), dtype=np.int64)
    buf[:, pad[0]:pad[0] + ih, pad[1]:pad[1] + iw, :] = src
    win = np.lib.stride_tricks.sliding_window_view(buf, (kh, kw), axis=(1, 2))    # {bs, y, x, c, kh, kw}
    win = win[:, ::stride[0], ::stride[1]][:, :oh, :ow]
    if rows is not None:
        win = win[:, list(rows)]
    return np.einsum('nyxckl,ockl->nyxo', win, w.astype(np.int64))


def imgconv_ref(case, data, rows=None):
    acc = imgconv_acc(data["src"], data["w"], case.stride, case.pad, (case.oh, case.ow), rows)
    f = _requant(acc, data["bia"], data["scales"], case.relu or case.dst_dt == U8)
    return _store(f, case.dst_dt, case.rm)


# --- the dense twin: the image zero-padded to 16 channels, zero weights on the channels >= ic ---------------------------
def pad16(src):
    out = np.zeros(src.shape[:3] + (16,), dtype=np.uint8)
    out[..., :src.shape[3]] = src
    return out


def pad16_weights(w):
    out = np.zeros((w.shape[0], 16) + w.shape[2:], dtype=np.int8)
    out[:, :w.shape[1]] = w
    return out


def dense_case(case):
    """the cases.ConvCase of the equivalent unfused dense conv on 16 channels (dense_expressible cases only)"""
    assert case.dense_expressible, case.ident()
    return C.ConvCase(case.name, case.bs, 16, case.ih, case.iw, case.oc, 0, k=case.k, stride=case.stride,
                      pad=case.pad, dst_dt=case.dst_dt, bia0_dt=case.bia_dt, relu0=case.relu, rm0=case.rm,
                      per_channel0=case.per_channel, wide=case.wide, seed=case.seed)


def dense_data(case, data):
    return dict(src=pad16(data["src"]), w0=pad16_weights(data["w"]), w1=None, bia0=data["bia"], bia1=None,
                scales0=data["scales"], scales1=np.ones(1, dtype=np.float32))


# --- the MFMA kernel's class ---------------------------------------------------------------------------------------------
# (name, window, stride, pad)
MFMA_GEOMS = [
    ("k7s2p3", (7, 7), (2, 2), (3, 3)),
    ("k3s1p1", (3, 3), (1, 1), (1, 1)),
    ("k3s2p1", (3, 3), (2, 2), (1, 1)),
    ("k3s2p0", (3, 3), (2, 2), (0, 0)),
]
# (ih, iw, hang): smaller than the 7x7 window; 9x9; odd row bytes, so that every row of a 3-channel image starts at
# another alignment; output rows longer than one 32-pixel strip that end in a partial one; two rows of 131 pixels; and
# one whose windows hang over the bottom / right edge (the largest output size the descriptor admits)
MFMA_IMAGES = [(5, 5, False), (9, 9, False), (17, 23, False), (33, 70, False), (2, 131, False), (10, 12, True)]


def _largest_out(ih, iw, stride, pad):
    """the largest output size whose last window still starts inside the input"""
    return ((ih - 1 + pad[0]) // stride[0] + 1, (iw - 1 + pad[1]) // stride[1] + 1)


def mfma_table(geom=None):
    """ic in {3, 4} x every geometry x oc in {32, 64, 96, 128} x every image, bs 1 and 3 in turn, the option rows
    rotating through them"""
    out, i = [], 0
    for name, k, s, p in MFMA_GEOMS:
        for ih, iw, hang in MFMA_IMAGES:
            for c in (3, 4):
                for oc in MFMA_OC:
                    ohw = _largest_out(ih, iw, s, p) if hang else None
                    if not hang and (ih + 2 * p[0] < k[0] or iw + 2 * p[1] < k[1]):
                        ohw = _largest_out(ih, iw, s, p)      # (2 x 131 without padding: the conv formula gives no row)
                    opt = OPTIONS[i % len(OPTIONS)]
                    if geom in (None, name):
                        out.append(ICase("%s-%dx%d" % (name, ih, iw), 1 + 2 * (i % 2), c, ih, iw, oc, k=k, stride=s, pad=p,
                                         out_hw=ohw, seed=21000 + 13 * i, **opt))
                    i += 1
    return out


# what only the generic path covers: ic in {1, 2, 3} x windows 5x5 / 1 and 11x11 / 4 x oc in {7, 16, 48}
def generic_table():
    out, i = [], 0
    for k, s, p, ih, iw in (((5, 5), (1, 1), (2, 2), 9, 10), ((11, 11), (4, 4), (2, 2), 23, 27)):
        for c in (1, 2, 3):
            for oc in (7, 16, 48):
                out.append(ICase("gen", 2, c, ih, iw, oc, k=k, stride=s, pad=p, seed=22000 + i, **OPTIONS[i % len(OPTIONS)]))
                i += 1
    return out


def all_tables():
    return mfma_table() + generic_table()


# --- permutation: within an output channel every (c, ky, kx) weight is distinct, and at every (c, ky, kx) the 32 output
#     channels' weights are distinct, so that a swapped axis in the packer or in the reference cannot pass.  (s8 has 256
#     values: all oc * ic * kh * kw weights cannot differ.)  s32 dst, scale 1, no bias: the accumulators themselves. ------
def permutation_case(k, stride, c):
    pad = (k[0] // 2, k[1] // 2)
    case = ICase("perm", 2, c, 11, 13, 32, k=k, stride=stride, pad=pad, dst_dt=S32, bia_dt=UNDEF, relu=False,
                 seed=23000 + 10 * k[0] + c)
    taps = c * k[0] * k[1]
    idx = np.arange(taps)[None, :] + 7 * np.arange(32)[:, None]
    w = ((idx % 255) - 127).astype(np.int8).reshape(32, c, k[0], k[1])
    src = np.random.default_rng(case.seed).integers(0, 256, (2, 11, 13, c)).astype(np.uint8)
    return case, dict(src=src, w=w, bia=None, scales=np.ones(1, dtype=np.float32))


# --- fast-route proof edges (dfx.h, dfx_imgconv_set_weights): dwconv_ref's EDGES, the edge channel's nine prescribed
#     weights on its first nine taps (input channel 0's 3x3 window), every other tap of the channel zero.  The
#     activations of image 0 / 1 attain the accumulator's maximum 255 P / minimum -255 N at the centre pixel of a 3x3
#     image (pad 1: the centre window is the whole image). ---------------------------------------------------------------
EDGE_IC, EDGE_OC = 3, 32


def edge_case(edge, dst_dt):
    """-> (case, data): 2 images of 3x3x3, per-channel scales and s32 bias; channel EDGE_CHANNEL as prescribed"""
    case = ICase("edge-" + edge.name, 2, EDGE_IC, 3, 3, EDGE_OC, dst_dt=dst_dt, bia_dt=S32, relu=False, rm=0,
                 per_channel=True, seed=24000)
    data = generate(case)
    w = data["w"].copy()
    w[EDGE_CHANNEL] = 0
    w[EDGE_CHANNEL].flat[:9] = edge.weights
    src = np.random.default_rng(24001).integers(0, 256, data["src"].shape).astype(np.uint8)
    src[0] = np.where(w[EDGE_CHANNEL] > 0, 255, 0).transpose(1, 2, 0)      # attains 255 P at the centre
    src[1] = np.where(w[EDGE_CHANNEL] < 0, 255, 0).transpose(1, 2, 0)      # attains -255 N
    bia = data["bia"].copy()
    bia[EDGE_CHANNEL] = edge.bias
    scales = data["scales"].copy()
    scales[EDGE_CHANNEL] = np.float32(edge.scale)
    return case, dict(src=src, w=w, bia=bia, scales=scales)


def edge_attained(edge, case, data):
    """the centre-pixel accumulator of the edge channel on the attaining image, and the bound the proof uses"""
    acc = imgconv_acc(data["src"], data["w"], case.stride, case.pad, (case.oh, case.ow))
    w = np.asarray(edge.weights, dtype=np.int64)
    P, N = int(w[w > 0].sum()), int(-w[w < 0].sum())
    img = 0 if edge.which == "max" else 1
    return int(acc[img, 1, 1, EDGE_CHANNEL]), (255 * P if edge.which == "max" else -255 * N), P, N
