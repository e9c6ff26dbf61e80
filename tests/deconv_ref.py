"""Reference, data and case tables of the transposed conv tests (pure numpy, needs no GPU).

The op is defined by the existing ops: it equals the grouped conv with groups = 1, stride 1 and padding
(kh-1-pad_t, kw-1-pad_l) on the zero-stuffed tensor with the spatially flipped weights and, where ic and oc are
multiples of 16, that padding is the same on both axes and the output size is the conv formula's, the unfused dense
conv on the same tensors.  deconv_ref is an independent numpy formulation -- a SCATTER: every input pixel adds its
kh x kw x oc contribution into an int64 canvas of (in - 1) * stride + k rows / columns, of which the output is the
window that starts at (pad_t, pad_l); then refmath's _requant / _store, unchanged -- which tests/test_deconv_cpu.py
pins against the C oracle's dense conv and against gconv_ref, and tests/test_gpu_deconv.py compares the GPU against,
bit for bit.  Neither the kernel's gather nor its parity split appears in it.
"""
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

import cases as C
from dwconv_ref import EDGES, EDGE_CHANNEL, LIMIT, OPTIONS  # noqa: F401  (the depthwise op's option rows and proof edges)
from refmath import _requant, _store

F32, S32, S8, U8, UNDEF = C.F32, C.S32, C.S8, C.U8, C.UNDEF
MFMA, GENERIC = 0, 1            # DFX_DECONV_MFMA / DFX_DECONV_GENERIC
LDS_LIMIT, FIXED_LDS, CHUNK = 160 * 1024, 21504, 4      # the MFMA kernel's LDS plan (deconv.cuh, deconv_api.hip)


@dataclass(frozen=True)
class DCase:
    name: str
    bs: int
    c: int                                        # input channels
    ih: int
    iw: int
    oc: int
    k: Tuple[int, int] = (2, 2)
    stride: Tuple[int, int] = (2, 2)
    pad: Tuple[int, int] = (0, 0)                 # pad_t, pad_l
    out_hw: Optional[Tuple[int, int]] = None      # None: (in - 1) * stride - 2 * pad + k
    dst_dt: int = U8
    bia_dt: int = S32
    relu: bool = True
    rm: int = 0
    per_channel: bool = False
    wide: bool = False                            # full-range data, scales that reach both saturation ends
    seed: int = 1234

    @property
    def oh(self):
        return self.out_hw[0] if self.out_hw else (self.ih - 1) * self.stride[0] - 2 * self.pad[0] + self.k[0]

    @property
    def ow(self):
        return self.out_hw[1] if self.out_hw else (self.iw - 1) * self.stride[1] - 2 * self.pad[1] + self.k[1]

    @property
    def mfma_class(self):
        k = self.k[0]
        window = (self.k[0] == self.k[1] and self.stride == (2, 2)
                  and ((k == 2 and self.pad == (0, 0)) or k in (3, 4)))
        return (window and self.c % 32 == 0 and self.oc % 32 == 0
                and 128 * (1 if k == 2 else 4) * self.c + FIXED_LDS <= LDS_LIMIT)

    @property
    def lds_blocks(self):
        """output blocks of 32 channels whose fragments the MFMA kernel keeps in LDS at once"""
        wblk = 128 * (1 if self.k[0] == 2 else 4) * self.c
        return min(CHUNK, self.oc // 32, (LDS_LIMIT - FIXED_LDS) // wblk)

    @property
    def dense_expressible(self):
        """the dense conv (symmetric padding, derived output size, channel blocks of 16) can express the case on the
        stuffed tensor"""
        return (self.out_hw is None and self.c % 16 == 0 and self.oc % 16 == 0
                and self.k[0] - 1 - self.pad[0] == self.k[1] - 1 - self.pad[1])

    def ident(self):
        return "%s-n%d-c%d-%dx%d-oc%d-k%dx%d-s%dx%d-p%d,%d-o%dx%d-%s-b%s-r%d-m%d-pc%d%s" % (
            self.name, self.bs, self.c, self.ih, self.iw, self.oc, self.k[0], self.k[1], self.stride[0],
            self.stride[1], self.pad[0], self.pad[1], self.oh, self.ow, C.NAME_OF[self.dst_dt], C.NAME_OF[self.bia_dt],
            self.relu, self.rm, self.per_channel, "-wide" if self.wide else "")


def taps_per_output(case):
    """the mean number of (ky, kx) taps that reach an output pixel, at least 1"""
    return max(1.0, case.k[0] * case.k[1] / float(case.stride[0] * case.stride[1]))


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
    amp = (74.0 * 147.0 / 8.0 if case.wide else 6.0 * 9.0) * np.sqrt(taps_per_output(case) * case.c)
    s = np.float32(80.0 / amp)
    if case.per_channel:
        scales = (s * (0.5 + np.arange(case.oc) / case.oc)).astype(np.float32)
    else:
        scales = np.array([s], dtype=np.float32)
    return dict(src=src, w=w, bia=C._bias(rng, case.oc, case.bia_dt, case.wide), scales=scales)


def deconv_acc(src, w, stride, pad, out_hw, rows=None):
    """exact int64 accumulators {bs, oh (or len(rows)), ow, oc}, as a scatter: for every tap (ky, kx) all input pixels
    add src[n,iy,ix,:] . w[:,:,ky,kx] into the canvas at (iy * sh + ky, ix * sw + kx); the output is the canvas from
    (pad_t, pad_l) on.  (The products go through a float64 matrix product: every partial sum is an integer far below
    2^53, so it is exact.)  rows: the output rows to return (all by default)"""
    bs, ih, iw, c = src.shape
    oc, ic, kh, kw = w.shape
    assert c == ic and kh * kw * ic * 255 * 128 < 2 ** 53
    sh, sw = stride
    oh, ow = out_hw
    H, W = (ih - 1) * sh + kh, (iw - 1) * sw + kw
    assert 1 <= oh <= H - pad[0] and 1 <= ow <= W - pad[1], (out_hw, H, W, pad)
    canvas = np.zeros((bs, H, W, oc), dtype=np.int64)
    flat = src.reshape(-1, c).astype(np.float64)
    for ky in range(kh):
        for kx in range(kw):
            contrib = (flat @ w[:, :, ky, kx].T.astype(np.float64)).reshape(bs, ih, iw, oc)
            canvas[:, ky:ky + (ih - 1) * sh + 1:sh, kx:kx + (iw - 1) * sw + 1:sw, :] += contrib.astype(np.int64)
    out = canvas[:, pad[0]:pad[0] + oh, pad[1]:pad[1] + ow, :]
    return out[:, list(rows)] if rows is not None else out


def deconv_ref(case, data, rows=None):
    acc = deconv_acc(data["src"], data["w"], case.stride, case.pad, (case.oh, case.ow), rows)
    f = _requant(acc, data["bia"], data["scales"], case.relu or case.dst_dt == U8)
    return _store(f, case.dst_dt, case.rm)


# --- the twins of the defining properties: a stride-1 conv on the zero-stuffed tensor with the flipped weights ------------
def stuff(src, stride):
    """{bs, ih, iw, c} -> {bs, (ih-1)*sh+1, (iw-1)*sw+1, c}: src at the multiples of the stride, 0 elsewhere"""
    bs, ih, iw, c = src.shape
    out = np.zeros((bs, (ih - 1) * stride[0] + 1, (iw - 1) * stride[1] + 1, c), dtype=src.dtype)
    out[:, ::stride[0], ::stride[1], :] = src
    return out


def flip(w):
    """w[o, i, kh-1-ky, kw-1-kx]"""
    return np.ascontiguousarray(w[:, :, ::-1, ::-1])


def twin_pad(case):
    return (case.k[0] - 1 - case.pad[0], case.k[1] - 1 - case.pad[1])


def dense_case(case):
    """the cases.ConvCase of the equivalent unfused dense conv on the stuffed tensor (dense_expressible cases only)"""
    assert case.dense_expressible, case.ident()
    return C.ConvCase(case.name, case.bs, case.c, (case.ih - 1) * case.stride[0] + 1, (case.iw - 1) * case.stride[1] + 1,
                      case.oc, 0, k=case.k, stride=(1, 1), pad=twin_pad(case), dst_dt=case.dst_dt, bia0_dt=case.bia_dt,
                      relu0=case.relu, rm0=case.rm, per_channel0=case.per_channel, wide=case.wide, seed=case.seed)


def dense_data(case, data):
    return dict(src=stuff(data["src"], case.stride), w0=flip(data["w"]), w1=None, bia0=data["bia"], bia1=None,
                scales0=data["scales"], scales1=np.ones(1, dtype=np.float32))


# --- the MFMA kernel's class ---------------------------------------------------------------------------------------------
# (name, window, pad, output_padding)
MFMA_GEOMS = [
    ("k2s2p0", (2, 2), (0, 0), 0),
    ("k4s2p1", (4, 4), (1, 1), 0),
    ("k3s2p1", (3, 3), (1, 1), 1),      # oh = 2 ih: Keras-style "same" decoders
    ("k4s2p0", (4, 4), (0, 0), 0),
]
# (ih, iw, crop): one pixel; a small odd image; one full 32-pixel strip plus one pixel; several strips and rows; and one
# whose output is cropped to the odd size 2 * in - 1, so that the last row and column have one parity only
MFMA_IMAGES = [(1, 1, False), (3, 5, False), (2, 33, False), (5, 70, False), (4, 6, True)]
# (ic, oc): one block; partial chunk; several K-steps; the first oc that needs a second weight chunk (5 blocks > CHUNK)
MFMA_CHANNELS = [(32, 32), (64, 96), (160, 64), (32, 160)]


def mfma_table(geom=None):
    """every geometry x image x channel pair, bs 1 and 3 in turn, the option rows rotating through them"""
    out, i = [], 0
    for name, k, p, op in MFMA_GEOMS:
        for ih, iw, crop in MFMA_IMAGES:
            for c, oc in MFMA_CHANNELS:
                if crop:
                    ohw = (2 * ih - 1, 2 * iw - 1)
                else:
                    ohw = ((ih - 1) * 2 - 2 * p[0] + k[0] + op, (iw - 1) * 2 - 2 * p[1] + k[1] + op) if op else None
                opt = OPTIONS[i % len(OPTIONS)]
                if geom in (None, name):
                    out.append(DCase("%s-%dx%d" % (name, ih, iw), 1 + 2 * (i % 2), c, ih, iw, oc, k=k, stride=(2, 2), pad=p,
                                     out_hw=ohw, seed=31000 + 13 * i, **opt))
                i += 1
    return out


# what only the generic path covers: (window, stride, pad, ih, iw, out_hw) x ic in {1, 3, 20} x oc in {1, 7, 48}
GENERIC_GEOMS = [
    ((3, 3), (1, 1), (1, 1), 5, 6, None),           # stride 1: a plain conv with flipped weights
    ((2, 2), (3, 3), (0, 0), 4, 5, None),           # holes: every third row / column is reached by no tap
    ((3, 3), (2, 1), (0, 1), 4, 7, None),           # mixed strides
    ((5, 5), (2, 2), (2, 2), 5, 4, (10, 8)),        # output_padding 1
]


def generic_table():
    out, i = [], 0
    for k, s, p, ih, iw, ohw in GENERIC_GEOMS:
        for c in (1, 3, 20):
            for oc in (1, 7, 48):
                out.append(DCase("gen", 2, c, ih, iw, oc, k=k, stride=s, pad=p, out_hw=ohw, seed=32000 + i,
                                 **OPTIONS[i % len(OPTIONS)]))
                i += 1
    return out


def all_tables():
    return mfma_table() + generic_table()


# --- permutation: within an output channel every (i, ky, kx) weight is distinct, and at every (i, ky, kx) the 32 output
#     channels' weights are distinct, so that a swapped axis or a wrong flip in the packer, the kernel or the reference
#     cannot pass.  s32 dst, scale 1, no bias: the accumulators themselves.  (32 * 4 * 4 = 512 taps exceed s8's 256
#     values, so the channel's weights repeat with period 255 along i * kh * kw -- never within a (ky, kx) plane of 32
#     input channels whose indices are kh * kw apart, nor between the taps of one input channel.) ------------------------
def permutation_case(name):
    _, k, p, op = [g for g in MFMA_GEOMS if g[0] == name][0]
    ih, iw = 5, 7
    ohw = (2 * ih, 2 * iw) if op else None
    case = DCase("perm-" + name, 2, 32, ih, iw, 32, k=k, stride=(2, 2), pad=p, out_hw=ohw, dst_dt=S32, bia_dt=UNDEF,
                 relu=False, seed=33000 + 10 * k[0] + p[0])
    taps = 32 * k[0] * k[1]
    idx = np.arange(taps)[None, :] + 7 * np.arange(32)[:, None]
    w = ((idx % 255) - 127).astype(np.int8).reshape(32, 32, k[0], k[1])
    src = np.random.default_rng(case.seed).integers(0, 256, (2, ih, iw, 32)).astype(np.uint8)
    return case, dict(src=src, w=w, bia=None, scales=np.ones(1, dtype=np.float32))


# --- fast-route proof edges (dfx.h, dfx_deconv_set_weights): dwconv_ref's EDGES on a 4x4 / 2 pad 1 op over a 3x3 image.
#     Output pixel (1, 1) has parity (0, 0): it sums the taps (ky, kx) in {0, 2}^2 of the input pixels
#     (1 - ky / 2, 1 - kx / 2).  The edge channel's nine prescribed weights sit on nine (tap, input channel) positions of
#     that ONE parity; every other weight of the channel is zero.  Image 0 / 1 holds 255 where the weight is positive /
#     negative, so the accumulator of (1, 1) attains 255 P / -255 N. --------------------------------------------------------
EDGE_IC, EDGE_OC, EDGE_PIXEL = 32, 32, (1, 1)
EDGE_POSITIONS = [(0, 0, 0), (0, 0, 1), (0, 0, 31), (0, 2, 0), (0, 2, 17), (2, 0, 3), (2, 0, 4), (2, 2, 16), (2, 2, 31)]  # (ky, kx, i)


def edge_case(edge, dst_dt):
    """-> (case, data): 2 images of 3x3x32, per-channel scales and s32 bias; channel EDGE_CHANNEL as prescribed"""
    case = DCase("edge-" + edge.name, 2, EDGE_IC, 3, 3, EDGE_OC, k=(4, 4), stride=(2, 2), pad=(1, 1), dst_dt=dst_dt, bia_dt=S32,
                 relu=False, rm=0, per_channel=True, seed=34000)
    data = generate(case)
    w = data["w"].copy()
    w[EDGE_CHANNEL] = 0
    src = np.random.default_rng(34001).integers(0, 256, data["src"].shape).astype(np.uint8)
    for (ky, kx, i), v in zip(EDGE_POSITIONS, edge.weights):
        w[EDGE_CHANNEL, i, ky, kx] = v
        iy, ix = EDGE_PIXEL[0] - ky // 2, EDGE_PIXEL[1] - kx // 2
        src[0, iy, ix, i] = 255 if v > 0 else 0      # attains 255 P at EDGE_PIXEL
        src[1, iy, ix, i] = 255 if v < 0 else 0      # attains -255 N
    bia = data["bia"].copy()
    bia[EDGE_CHANNEL] = edge.bias
    scales = data["scales"].copy()
    scales[EDGE_CHANNEL] = np.float32(edge.scale)
    return case, dict(src=src, w=w, bia=bia, scales=scales)


def edge_attained(edge, case, data):
    """EDGE_PIXEL's accumulator of the edge channel on the attaining image, and the bound the proof uses"""
    acc = deconv_acc(data["src"], data["w"], case.stride, case.pad, (case.oh, case.ow))
    w = np.asarray(edge.weights, dtype=np.int64)
    P, N = int(w[w > 0].sum()), int(-w[w < 0].sum())
    img = 0 if edge.which == "max" else 1
    return int(acc[img, EDGE_PIXEL[0], EDGE_PIXEL[1], EDGE_CHANNEL]), (255 * P if edge.which == "max" else -255 * N), P, N
