"""Reference, data and case tables of the grouped conv tests (pure numpy, needs no GPU).

The op is defined by the existing conv: where ic and oc are multiples of 16 and the output size is the conv's, it equals
the unfused dense conv with block-diagonal weights.  gconv_ref is an independent numpy formulation -- an int64 tap loop
with one einsum over (group, input channel of the group) per tap, then refmath's _requant / _store, unchanged -- which
tests/test_gconv_cpu.py pins against the C oracle's dense conv and tests/test_gpu_gconv.py compares the GPU against,
bit for bit.
"""
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

import cases as C
from dwconv_ref import EDGES, EDGE_CHANNEL, LIMIT, OPTIONS  # noqa: F401  (the depthwise op's option rows and proof edges)
from refmath import _requant, _store

F32, S32, S8, U8, UNDEF = C.F32, C.S32, C.S8, C.U8, C.UNDEF
MFMA, GENERIC = 0, 1            # DFX_GCONV_MFMA / DFX_GCONV_GENERIC
MFMA_CPG = (4, 8, 16, 32, 64)


@dataclass(frozen=True)
class GCase:
    name: str
    bs: int
    c: int                                        # input channels
    ih: int
    iw: int
    oc: int
    groups: int
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
    def cpg(self):
        return self.c // self.groups

    @property
    def mfma_class(self):
        return (self.k == (3, 3) and self.stride in ((1, 1), (2, 2)) and self.c == self.oc and self.c % 32 == 0
                and self.cpg in MFMA_CPG)

    @property
    def dense_expressible(self):
        """the dense conv (symmetric padding, derived output size, channel blocks of 16) can express the case"""
        return self.out_hw is None and self.c % 16 == 0 and self.oc % 16 == 0

    def ident(self):
        return "%s-n%d-c%d-%dx%d-oc%d-g%d-k%dx%d-s%dx%d-p%d,%d-o%dx%d-%s-b%s-r%d-m%d-pc%d%s" % (
            self.name, self.bs, self.c, self.ih, self.iw, self.oc, self.groups, self.k[0], self.k[1], self.stride[0],
            self.stride[1], self.pad[0], self.pad[1], self.oh, self.ow, C.NAME_OF[self.dst_dt], C.NAME_OF[self.bia_dt],
            self.relu, self.rm, self.per_channel, "-wide" if self.wide else "")


def generate(case):
    """-> dict(src NHWC u8, w s8 {oc, ic/groups, kh, kw}, bia, scales).  Reference-range data (cases.py), or "wide":
    full-range activations and weights with -128 and 127 present, and scales eight times the size that centres the
    output, so that both saturation ends of a 1-byte dst are reached.  The weights are random per (o, i, tap): a
    transposed or permuted fragment cannot pass."""
    rng = np.random.default_rng(case.seed)
    kh, kw = case.k
    if case.wide:
        src = rng.integers(0, 256, (case.bs, case.ih, case.iw, case.c)).astype(np.uint8)
        w = rng.integers(-128, 128, (case.oc, case.cpg, kh, kw)).astype(np.int8)
        w[0].flat[0] = -128
        w[case.oc - 1].flat[-1] = 127
    else:
        src = rng.integers(0, 17, (case.bs, case.ih, case.iw, case.c)).astype(np.uint8)
        w = rng.integers(-10, 11, (case.oc, case.cpg, kh, kw)).astype(np.int8)
    amp = (74.0 * 147.0 / 8.0 if case.wide else 6.0 * 9.0) * np.sqrt(kh * kw * case.cpg)
    s = np.float32(80.0 / amp)
    if case.per_channel:
        scales = (s * (0.5 + np.arange(case.oc) / case.oc)).astype(np.float32)
    else:
        scales = np.array([s], dtype=np.float32)
    return dict(src=src, w=w, bia=C._bias(rng, case.oc, case.bia_dt, case.wide), scales=scales)


def gconv_acc(src, w, groups, stride, pad, out_hw):
    """exact int64 accumulators: a tap loop over shifted strided views of the zero-padded source, one einsum over
    (group, input channel of the group) per tap"""
    bs, ih, iw, c = src.shape
    oc, icg, kh, kw = w.shape
    assert c == icg * groups and oc % groups == 0
    oh, ow = out_hw
    need_h = max((oh - 1) * stride[0] + kh, pad[0] + ih)
    need_w = max((ow - 1) * stride[1] + kw, pad[1] + iw)
    buf = np.zeros((bs, need_h, need_w, c), dtype=np.int64)
    buf[:, pad[0]:pad[0] + ih, pad[1]:pad[1] + iw, :] = src
    wg = w.astype(np.int64).reshape(groups, oc // groups, icg, kh, kw)
    acc = np.zeros((bs, oh, ow, groups, oc // groups), dtype=np.int64)
    for ky in range(kh):
        for kx in range(kw):
            v = buf[:, ky:ky + (oh - 1) * stride[0] + 1:stride[0], kx:kx + (ow - 1) * stride[1] + 1:stride[1], :]
            acc += np.einsum('nyxgi,goi->nyxgo', v.reshape(bs, oh, ow, groups, icg), wg[:, :, :, ky, kx])
    return acc.reshape(bs, oh, ow, oc)


def gconv_ref(case, data):
    acc = gconv_acc(data["src"], data["w"], case.groups, case.stride, case.pad, (case.oh, case.ow))
    f = _requant(acc, data["bia"], data["scales"], case.relu or case.dst_dt == U8)
    return _store(f, case.dst_dt, case.rm)


def block_diag_weights(w, groups):
    """{oc, ic/groups, kh, kw} -> dense oihw {oc, ic, kh, kw}: W[o][j] = w[o][j - g(o) * ic/groups] inside o's group"""
    oc, icg, kh, kw = w.shape
    ocg = oc // groups
    d = np.zeros((oc, icg * groups, kh, kw), dtype=np.int8)
    for g in range(groups):
        d[g * ocg:(g + 1) * ocg, g * icg:(g + 1) * icg] = w[g * ocg:(g + 1) * ocg]
    return d


def dense_case(case):
    """the cases.ConvCase of the equivalent unfused dense conv (dense_expressible cases only)"""
    assert case.dense_expressible, case.ident()
    return C.ConvCase(case.name, case.bs, case.c, case.ih, case.iw, case.oc, 0, k=case.k, stride=case.stride,
                      pad=case.pad, dst_dt=case.dst_dt, bia0_dt=case.bia_dt, relu0=case.relu, rm0=case.rm,
                      per_channel0=case.per_channel, wide=case.wide, seed=case.seed)


def dense_data(case, data):
    return dict(src=data["src"], w0=block_diag_weights(data["w"], case.groups), w1=None, bia0=data["bia"], bia1=None,
                scales0=data["scales"], scales1=np.ones(1, dtype=np.float32))


# --- the MFMA kernel's class.  (c, cpg): full and partial 128-channel chunks (32, 96, 160: the last chunk partial), a
#     group that straddles nothing (cpg <= 32), one block (cpg 32) or two (cpg 64; c = 192: the third group sits alone in
#     the second chunk). ------------------------------------------------------------------------------------------------
MFMA_CHANNELS = [(c, cpg) for c in (32, 96, 128, 160, 256) for cpg in (4, 8, 16, 32)] + [(c, 64) for c in (64, 128, 192)]

# (name, stride, pad, [(ih, iw, out_hw)]); bs = 2 throughout: image boundaries fall inside a strip of 32 pixels
MFMA_GEOMS = [
    ("s1p1", (1, 1), (1, 1), [(1, 1, None), (3, 3, None), (7, 7, None), (5, 9, None), (13, 37, None)]),
    ("s1p0", (1, 1), (0, 0), [(5, 6, None)]),
    ("s1p2", (1, 1), (2, 2), [(4, 5, None)]),                                # corner windows all padding
    ("s2p1", (2, 2), (1, 1), [(8, 8, None), (7, 7, None), (9, 14, None)]),
    ("s2same", (2, 2), (0, 0), [(8, 8, (4, 4)), (7, 10, (4, 5))]),           # windows hang over
]


def mfma_table():
    """every geometry x (c, cpg), the options rotating through them; one row longer than any strip"""
    out, i = [], 0
    for name, s, p, imgs in MFMA_GEOMS:
        for ih, iw, ohw in imgs:
            for c, cpg in MFMA_CHANNELS:
                opt = OPTIONS[i % len(OPTIONS)]
                out.append(GCase("%s-%dx%d" % (name, ih, iw), 2, c, ih, iw, c, c // cpg, stride=s, pad=p, out_hw=ohw,
                                 seed=12000 + 13 * i, **opt))
                i += 1
    out.append(GCase("s1p1-long", 2, 96, 3, 200, 96, 12, seed=12999, **OPTIONS[0]))
    return out


def options_table():
    """every option row on one stride-1 and one stride-2 geometry at c = 96, cpg 8"""
    out = []
    for i, opt in enumerate(OPTIONS):
        out.append(GCase("opt%d-s1" % i, 2, 96, 9, 11, 96, 12, seed=13000 + i, **opt))
        out.append(GCase("opt%d-s2" % i, 2, 96, 9, 11, 96, 12, stride=(2, 2), seed=13100 + i, **opt))
    return out


# (ic, oc, groups, k, stride, pad): what only the generic path covers
GENERIC_SHAPES = [
    (24, 36, 3, (3, 3), (1, 1), (1, 1)),        # ic != oc, cpg 8
    (240, 60, 3, (3, 3), (2, 2), (1, 1)),       # ic != oc, cpg 80
    (32, 64, 4, (1, 1), (1, 1), (0, 0)),        # ic != oc, 1x1
    (20, 20, 20, (5, 5), (1, 1), (2, 2)),       # groups = ic (cpg 1), c = 20
    (20, 20, 10, (7, 7), (1, 1), (3, 3)),       # cpg 2
    (24, 24, 8, (1, 3), (1, 1), (0, 1)),        # cpg 3
    (24, 24, 2, (3, 3), (1, 2), (1, 1)),        # cpg 12, mixed strides
    (48, 48, 2, (3, 3), (2, 1), (1, 1)),        # cpg 24, mixed strides
    (48, 48, 1, (3, 3), (2, 2), (1, 1)),        # groups = 1
    (64, 64, 4, (5, 5), (2, 2), (2, 2)),        # the MFMA class's channels, not its window
    (64, 64, 16, (3, 3), (3, 3), (1, 1)),       # ... not its stride
    (64, 64, 32, (3, 3), (1, 1), (1, 1)),       # ... not its cpg (2)
]


def generic_table():
    out = []
    for i, (ic, oc, g, k, s, p) in enumerate(GENERIC_SHAPES):
        out.append(GCase("gen", 2, ic, 9, 10, oc, g, k=k, stride=s, pad=p, seed=14000 + i, **OPTIONS[i % len(OPTIONS)]))
    return out


def all_tables():
    return mfma_table() + options_table() + generic_table()


# --- group isolation: with the source non-zero only in the channels of groups != g, the output channels of group g
#     see nothing but the bias ------------------------------------------------------------------------------------------
def isolation_case(c, cpg, g):
    """-> (case, data, expected value of group g's channels {ocg}): s32 dst, scale 1, s32 bias"""
    case = GCase("isolate", 2, c, 6, 7, c, c // cpg, dst_dt=S32, bia_dt=S32, relu=False, seed=15000 + cpg)
    data = generate(case)
    src = np.random.default_rng(15001).integers(1, 256, data["src"].shape).astype(np.uint8)
    src[..., g * cpg:(g + 1) * cpg] = 0
    data = dict(data, src=src, scales=np.ones(1, dtype=np.float32))
    return case, data, data["bia"][g * cpg:(g + 1) * cpg].astype(np.int32)


# --- fast-route proof edges (dfx.h, dfx_gconv_set_weights): dwconv_ref's EDGES, the edge channel's nine prescribed
#     weights spread over the four input channels of its group (tap t on input channel t % 4).  The activations of
#     image 0 / 1 attain the accumulator's maximum 255 P / minimum -255 N at the centre pixel of a 3x3 image. ----------
EDGE_C, EDGE_CPG = 32, 4


def edge_weights(edge):
    w = np.zeros((EDGE_CPG, 3, 3), dtype=np.int8)
    for t, v in enumerate(edge.weights):
        w[t % EDGE_CPG, t // 3, t % 3] = v
    return w


def edge_case(edge, dst_dt):
    """-> (case, data): 2 images of 3x3x32, cpg 4, per-channel scales and s32 bias; channel EDGE_CHANNEL as prescribed"""
    case = GCase("edge-" + edge.name, 2, EDGE_C, 3, 3, EDGE_C, EDGE_C // EDGE_CPG, dst_dt=dst_dt, bia_dt=S32, relu=False,
                 rm=0, per_channel=True, seed=16000)
    data = generate(case)
    w = data["w"].copy()
    w[EDGE_CHANNEL] = edge_weights(edge)
    g0 = (EDGE_CHANNEL // EDGE_CPG) * EDGE_CPG
    src = np.random.default_rng(16001).integers(0, 256, data["src"].shape).astype(np.uint8)
    src[0, :, :, g0:g0 + EDGE_CPG] = np.where(w[EDGE_CHANNEL] > 0, 255, 0).transpose(1, 2, 0)   # attains 255 P at the centre
    src[1, :, :, g0:g0 + EDGE_CPG] = np.where(w[EDGE_CHANNEL] < 0, 255, 0).transpose(1, 2, 0)   # attains -255 N
    bia = data["bia"].copy()
    bia[EDGE_CHANNEL] = edge.bias
    scales = data["scales"].copy()
    scales[EDGE_CHANNEL] = np.float32(edge.scale)
    return case, dict(src=src, w=w, bia=bia, scales=scales)


def edge_attained(edge, case, data):
    """the centre-pixel accumulator of the edge channel on the attaining image, and the bound the proof uses"""
    acc = gconv_acc(data["src"], data["w"], case.groups, case.stride, case.pad, (case.oh, case.ow))
    w = np.asarray(edge.weights, dtype=np.int64)
    P, N = int(w[w > 0].sum()), int(-w[w < 0].sum())
    img = 0 if edge.which == "max" else 1
    return int(acc[img, 1, 1, EDGE_CHANNEL]), (255 * P if edge.which == "max" else -255 * N), P, N
