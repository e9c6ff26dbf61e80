"""Reference, data and case tables of the depthwise conv tests (pure numpy, needs no GPU).

The op is defined by the existing conv: for c a multiple of 16 it equals the unfused dense conv with ic = oc = c and
W[o][i] = (o == i) ? w[o] : 0.  dw_ref is an independent numpy formulation -- an int64 tap loop for the accumulator,
then refmath's _requant / _store, unchanged -- which tests/test_dwconv_cpu.py pins against the C oracle's dense conv
and tests/test_gpu_dwconv.py compares the GPU against, bit for bit.
"""
from dataclasses import dataclass, replace
from typing import Optional, Tuple

import numpy as np

import cases as C
from refmath import _requant, _store

F32, S32, S8, U8, UNDEF = C.F32, C.S32, C.S8, C.U8, C.UNDEF
WINDOW, GENERIC = 0, 1          # DFX_DWCONV_WINDOW / DFX_DWCONV_GENERIC


@dataclass(frozen=True)
class DwCase:
    name: str
    bs: int
    c: int
    ih: int
    iw: int
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
    def dense_expressible(self):
        """the dense conv (symmetric padding, derived output size) can express the case"""
        return self.out_hw is None and self.c % 16 == 0

    def ident(self):
        return "%s-n%d-c%d-%dx%d-k%dx%d-s%dx%d-p%d,%d-o%dx%d-%s-b%s-r%d-m%d-pc%d%s" % (
            self.name, self.bs, self.c, self.ih, self.iw, self.k[0], self.k[1], self.stride[0], self.stride[1],
            self.pad[0], self.pad[1], self.oh, self.ow, C.NAME_OF[self.dst_dt], C.NAME_OF[self.bia_dt], self.relu,
            self.rm, self.per_channel, "-wide" if self.wide else "")


def generate(case):
    """-> dict(src NHWC u8, w s8 {c, kh, kw}, bia, scales).  Reference-range data (cases.py), or "wide": full-range
    activations and weights with -128 and 127 present, and scales eight times the size that centres the output, so
    that both saturation ends of a 1-byte dst are reached."""
    rng = np.random.default_rng(case.seed)
    kh, kw = case.k
    if case.wide:
        src = rng.integers(0, 256, (case.bs, case.ih, case.iw, case.c)).astype(np.uint8)
        w = rng.integers(-128, 128, (case.c, kh, kw)).astype(np.int8)
        w[0].flat[0] = -128
        w[case.c - 1].flat[-1] = 127
    else:
        src = rng.integers(0, 17, (case.bs, case.ih, case.iw, case.c)).astype(np.uint8)
        w = rng.integers(-10, 11, (case.c, kh, kw)).astype(np.int8)
    amp = (74.0 * 147.0 / 8.0 if case.wide else 6.0 * 9.0) * np.sqrt(kh * kw)
    s = np.float32(80.0 / amp)
    if case.per_channel:
        scales = (s * (0.5 + np.arange(case.c) / case.c)).astype(np.float32)
    else:
        scales = np.array([s], dtype=np.float32)
    return dict(src=src, w=w, bia=C._bias(rng, case.c, case.bia_dt, case.wide), scales=scales)


def dw_acc(src, w, stride, pad, out_hw):
    """exact int64 accumulators: a tap loop over shifted strided views of the zero-padded source"""
    bs, ih, iw, c = src.shape
    kh, kw = w.shape[1:]
    oh, ow = out_hw
    need_h = max((oh - 1) * stride[0] + kh, pad[0] + ih)
    need_w = max((ow - 1) * stride[1] + kw, pad[1] + iw)
    buf = np.zeros((bs, need_h, need_w, c), dtype=np.int64)
    buf[:, pad[0]:pad[0] + ih, pad[1]:pad[1] + iw, :] = src
    acc = np.zeros((bs, oh, ow, c), dtype=np.int64)
    for ky in range(kh):
        for kx in range(kw):
            v = buf[:, ky:ky + (oh - 1) * stride[0] + 1:stride[0], kx:kx + (ow - 1) * stride[1] + 1:stride[1], :]
            acc += v * w[:, ky, kx].astype(np.int64)
    return acc


def dw_ref(case, data):
    acc = dw_acc(data["src"], data["w"], case.stride, case.pad, (case.oh, case.ow))
    f = _requant(acc, data["bia"], data["scales"], case.relu or case.dst_dt == U8)
    return _store(f, case.dst_dt, case.rm)


def diag_weights(w):
    """{c, kh, kw} -> dense oihw {c, c, kh, kw} with the depthwise windows on the diagonal"""
    c, kh, kw = w.shape
    d = np.zeros((c, c, kh, kw), dtype=np.int8)
    d[np.arange(c), np.arange(c)] = w
    return d


def dense_case(case):
    """the cases.ConvCase of the equivalent unfused dense conv (dense_expressible cases only)"""
    assert case.dense_expressible, case.ident()
    return C.ConvCase(case.name, case.bs, case.c, case.ih, case.iw, case.c, 0, k=case.k, stride=case.stride,
                      pad=case.pad, dst_dt=case.dst_dt, bia0_dt=case.bia_dt, relu0=case.relu, rm0=case.rm,
                      per_channel0=case.per_channel, wide=case.wide, seed=case.seed)


def dense_data(data):
    return dict(src=data["src"], w0=diag_weights(data["w"]), w1=None, bia0=data["bia"], bia1=None,
                scales0=data["scales"], scales1=np.ones(1, dtype=np.float32))


# --- options: every dst dtype, every bias dtype, one / per-channel scales, both round modes, relu on / off ------------
OPTIONS = [
    dict(dst_dt=U8, bia_dt=S32, per_channel=False, rm=0, relu=True),
    dict(dst_dt=S8, bia_dt=S8, per_channel=True, rm=1, relu=False),
    dict(dst_dt=S32, bia_dt=UNDEF, per_channel=False, rm=0, relu=False),
    dict(dst_dt=F32, bia_dt=F32, per_channel=True, rm=0, relu=True),
    dict(dst_dt=U8, bia_dt=U8, per_channel=True, rm=1, relu=False),       # u8 dst forces the ReLU
    dict(dst_dt=S8, bia_dt=S32, per_channel=False, rm=0, relu=True, wide=True),
    dict(dst_dt=S32, bia_dt=F32, per_channel=True, rm=1, relu=True),
    dict(dst_dt=U8, bia_dt=UNDEF, per_channel=False, rm=0, relu=False, wide=True),
    dict(dst_dt=S8, bia_dt=S8, per_channel=True, rm=0, relu=False, wide=True),
    dict(dst_dt=F32, bia_dt=S8, per_channel=False, rm=1, relu=False),
    dict(dst_dt=S32, bia_dt=U8, per_channel=True, rm=0, relu=False),
    dict(dst_dt=S8, bia_dt=F32, per_channel=False, rm=0, relu=False),
]

CHANNELS = (16, 48, 144)

# --- the window kernel's class: (name, kernel, stride, pad, [(bs, ih, iw, out_hw)]) --------------------------------------
WINDOW_GEOMS = [
    ("k3s1p1", (3, 3), (1, 1), (1, 1), [(2, 1, 1, None), (2, 3, 3, None), (2, 7, 7, None), (2, 5, 9, None), (2, 13, 37, None)]),
    ("k3s1p0", (3, 3), (1, 1), (0, 0), [(2, 5, 6, None)]),
    ("k3s1p2", (3, 3), (1, 1), (2, 2), [(2, 4, 5, None)]),                             # corner windows all padding
    ("k3s2p1", (3, 3), (2, 2), (1, 1), [(2, 8, 8, None), (2, 7, 7, None), (2, 9, 14, None)]),
    ("k3s2same", (3, 3), (2, 2), (0, 0), [(2, 8, 8, (4, 4)), (2, 7, 10, (4, 5))]),      # windows hang over
    ("k5s1p2", (5, 5), (1, 1), (2, 2), [(2, 5, 5, None), (2, 11, 14, None)]),          # 5x5: every window clipped
    ("k5s2p2", (5, 5), (2, 2), (2, 2), [(2, 9, 9, None), (2, 10, 7, None)]),
]


def window_table():
    """every geometry x channel count, the options rotating through them"""
    out, i = [], 0
    for name, k, s, p, imgs in WINDOW_GEOMS:
        for bs, ih, iw, ohw in imgs:
            for c in CHANNELS:
                opt = OPTIONS[i % len(OPTIONS)]
                out.append(DwCase("%s-%dx%d" % (name, ih, iw), bs, c, ih, iw, k=k, stride=s, pad=p, out_hw=ohw,
                                  seed=2000 + 13 * i, **opt))
                i += 1
    # a row longer than any strip of lanes (one image), and 5x5 beyond 64 channel groups (weights per lane in LDS)
    out.append(DwCase("k3s1p1-long", 1, 16, 3, 200, seed=2999, **OPTIONS[0]))
    out.append(DwCase("k5s1p2-g65", 1, 16 * 65, 5, 5, k=(5, 5), pad=(2, 2), seed=2998, **OPTIONS[1]))
    out.append(DwCase("k5s2p2-g65", 1, 16 * 65, 6, 5, k=(5, 5), stride=(2, 2), pad=(2, 2), seed=2997, **OPTIONS[0]))
    return out


def options_table():
    """every option row on one 3x3 and one 5x5 geometry of the window class"""
    out = []
    for i, opt in enumerate(OPTIONS):
        out.append(DwCase("opt%d-k3" % i, 2, 48, 9, 11, seed=3000 + i, **opt))
        out.append(DwCase("opt%d-k5s2" % i, 2, 32, 9, 11, k=(5, 5), stride=(2, 2), pad=(2, 2), seed=3100 + i, **opt))
    return out


def generic_table():
    """what only the generic path covers: mixed strides, other windows, channel counts that are no multiple of 16"""
    geoms = [((3, 3), (1, 2), (1, 1)), ((3, 3), (2, 1), (1, 1)), ((7, 7), (1, 1), (3, 3)), ((1, 3), (1, 1), (0, 1)),
             ((3, 1), (1, 1), (1, 0)), ((7, 7), (2, 2), (3, 3))]
    out, i = [], 0
    for k, s, p in geoms:
        for c in (1, 3, 20, 24):
            out.append(DwCase("gen", 2, c, 9, 10, k=k, stride=s, pad=p, seed=4000 + i, **OPTIONS[i % len(OPTIONS)]))
            i += 1
    # inside the window class by window and stride, outside it by the channel count; and c % 16 == 0 on a 7x7
    out.append(DwCase("gen-c24", 2, 24, 7, 9, seed=4100, **OPTIONS[0]))
    out.append(DwCase("gen-c32k7", 2, 32, 9, 10, k=(7, 7), pad=(3, 3), seed=4101, **OPTIONS[5]))
    return out


def all_tables():
    return window_table() + options_table() + generic_table()


# --- fast-route proof edges (dfx.h, dfx_dwconv_set_weights): per channel, bias and scale finite and
#     (255 * max(P, N) + |bias|) * |scale| <= 2^30.  One channel (EDGE_CHANNEL) of a 3x3 op carries prescribed weights;
#     the activations of image 0 / 1 attain its accumulator's maximum 255 P / minimum -255 N at the centre pixel of a
#     3x3 image (pad 1: the centre window is the whole image). ------------------------------------------------------------
EDGE_CHANNEL = 5
LIMIT = 1 << 30


@dataclass(frozen=True)
class Edge:
    name: str
    weights: Tuple[int, ...]      # the edge channel's nine taps
    bias: int                     # s32
    scale: float                  # a power of two: the bound is hit exactly
    fast: bool                    # what the proof must say
    which: str                    # "max" | "min": the side that attains the bound


def _edge(name, weights, side, scale_log2, over):
    """(255 * max(P, N) + |bias|) * 2^scale_log2 == 2^30 (+ 2^scale_log2 when `over`), bias carrying the side's sign"""
    w = np.asarray(weights, dtype=np.int64)
    P, N = int(w[w > 0].sum()), int(-w[w < 0].sum())
    assert (P >= N) == (side == "max") and P != N
    mag = (LIMIT >> scale_log2) - 255 * max(P, N) + (1 if over else 0)
    assert mag > 0
    return Edge(name, tuple(int(v) for v in weights), mag if side == "max" else -mag, float(2 ** scale_log2), not over, side)


EDGES = [
    _edge("P-last-admitted", (127, 0, 0, 100, -3, 0, 0, 0, 0), "max", 10, False),
    _edge("P-first-rejected", (127, 0, 0, 100, -3, 0, 0, 0, 0), "max", 10, True),
    _edge("N-last-admitted", (-128, 0, 2, 0, -128, 0, 0, -77, 0), "min", 12, False),
    _edge("N-first-rejected", (-128, 0, 2, 0, -128, 0, 0, -77, 0), "min", 12, True),
    _edge("all-taps-127-admitted", (127,) * 9, "max", 8, False),
    _edge("all-taps-min-rejected", (-128,) * 9, "min", 8, True),
]


def edge_case(edge, dst_dt):
    """-> (case, data): 2 images of 3x3x16, per-channel scales and s32 bias; channel EDGE_CHANNEL as prescribed"""
    case = DwCase("edge-" + edge.name, 2, 16, 3, 3, dst_dt=dst_dt, bia_dt=S32, relu=False, rm=0, per_channel=True,
                  seed=5000)
    data = generate(case)
    w = data["w"].copy()
    w[EDGE_CHANNEL] = np.asarray(edge.weights, dtype=np.int8).reshape(3, 3)
    src = np.random.default_rng(5001).integers(0, 256, data["src"].shape).astype(np.uint8)
    src[0, :, :, EDGE_CHANNEL] = np.where(w[EDGE_CHANNEL] > 0, 255, 0)      # attains 255 P at the centre
    src[1, :, :, EDGE_CHANNEL] = np.where(w[EDGE_CHANNEL] < 0, 255, 0)      # attains -255 N
    bia = data["bia"].copy()
    bia[EDGE_CHANNEL] = edge.bias
    scales = data["scales"].copy()
    scales[EDGE_CHANNEL] = np.float32(edge.scale)
    return case, dict(src=src, w=w, bia=bia, scales=scales)


def edge_attained(edge, case, data):
    """the centre-pixel accumulator of the edge channel on the attaining image, and the bound the proof uses"""
    acc = dw_acc(data["src"], data["w"], case.stride, case.pad, (case.oh, case.ow))
    w = np.asarray(edge.weights, dtype=np.int64)
    P, N = int(w[w > 0].sum()), int(-w[w < 0].sum())
    img = 0 if edge.which == "max" else 1
    return int(acc[img, 1, 1, EDGE_CHANNEL]), (255 * P if edge.which == "max" else -255 * N), P, N
