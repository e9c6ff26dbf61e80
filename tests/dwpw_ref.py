"""Reference, data and case tables of the depthwise + pointwise conv tests (pure numpy, needs no GPU).

The op is defined by the two ops it replaces: dwconv_ref.dw_ref to u8, then an unfused 1x1 conv on that tensor.
`ref` is the numpy formulation of that (refmath's _requant / _store, unchanged); `ref_oracle` computes stage 1 with
the C oracle's unfused conv, and `fused_dense` is the oracle's FUSED conv with block-diagonal conv0 weights.
tests/test_dwpw_cpu.py pins the three against each other; tests/test_gpu_dwpw.py compares the GPU with `ref`.
"""
from dataclasses import dataclass, replace
from typing import Optional, Tuple

import numpy as np

import cases as C
import dwconv_ref as DW
from refmath import _requant, _store

F32, S32, S8, U8, UNDEF = C.F32, C.S32, C.S8, C.U8, C.UNDEF
FUSED, TWO_LAUNCH = 0, 1          # DFX_DWPW_FUSED / DFX_DWPW_TWO_LAUNCH
EXACT, FAST = 0, 1


@dataclass(frozen=True)
class DwPwCase:
    name: str
    bs: int
    c: int
    ih: int
    iw: int
    oc: int
    k: Tuple[int, int] = (3, 3)
    stride: Tuple[int, int] = (1, 1)
    pad: Tuple[int, int] = (1, 1)
    out_hw: Optional[Tuple[int, int]] = None
    dst_dt: int = U8
    bia0_dt: int = S32
    bia1_dt: int = S32
    relu: bool = True                 # stage 1
    rm0: int = 0
    rm1: int = 0
    pc0: bool = False
    pc1: bool = False
    wide: bool = False
    seed: int = 1234

    @property
    def dw(self):
        """stage 0 as a dwconv_ref case (dst u8)"""
        return DW.DwCase(self.name, self.bs, self.c, self.ih, self.iw, k=self.k, stride=self.stride, pad=self.pad,
                         out_hw=self.out_hw, dst_dt=U8, bia_dt=self.bia0_dt, relu=True, rm=self.rm0,
                         per_channel=self.pc0, wide=self.wide, seed=self.seed)

    @property
    def oh(self):
        return self.dw.oh

    @property
    def ow(self):
        return self.dw.ow

    @property
    def dense_expressible(self):
        return self.dw.dense_expressible

    @property
    def in_class(self):
        """the fused kernel's class (dfx.h, DFX_DWPW_FUSED); the 2^31-byte clause never binds in these tables"""
        return (self.k == (3, 3) and self.stride in ((1, 1), (2, 2)) and self.c % 32 == 0 and self.c <= 256 and
                self.oc in (64, 128, 256) and self.c * self.oc <= 65536)

    def ident(self):
        return "%s-n%d-c%d-oc%d-%dx%d-k%dx%d-s%dx%d-p%d,%d-o%dx%d-%s-b%s,%s-r%d-m%d%d-pc%d%d%s" % (
            self.name, self.bs, self.c, self.oc, self.ih, self.iw, self.k[0], self.k[1], self.stride[0], self.stride[1],
            self.pad[0], self.pad[1], self.oh, self.ow, C.NAME_OF[self.dst_dt], C.NAME_OF[self.bia0_dt],
            C.NAME_OF[self.bia1_dt], self.relu, self.rm0, self.rm1, self.pc0, self.pc1, "-wide" if self.wide else "")


def generate(case):
    """-> dict(src, w, bia0, scales0 (dwconv_ref.generate of stage 0), w1 oihw {oc, c, 1, 1}, bia1, scales1).
    "wide": full-range data in both stages; the stage-1 scale is eight times the size that centres the output."""
    d0 = DW.generate(case.dw)
    rng = np.random.default_rng(case.seed + 7919)
    if case.wide:
        w1 = rng.integers(-128, 128, (case.oc, case.c, 1, 1)).astype(np.int8)
        amp = 74.0 * 147.0 / 8.0 * np.sqrt(case.c)
    else:
        w1 = rng.integers(-10, 11, (case.oc, case.c, 1, 1)).astype(np.int8)
        amp = 6.0 * 40.0 * np.sqrt(case.c)
    s = np.float32(60.0 / amp)
    if case.pc1:
        scales1 = (s * (0.5 + np.arange(case.oc) / case.oc)).astype(np.float32)
    else:
        scales1 = np.array([s], dtype=np.float32)
    return dict(src=d0["src"], w=d0["w"], bia0=d0["bia"], scales0=d0["scales"], w1=w1,
                bia1=C._bias(rng, case.oc, case.bia1_dt, case.wide), scales1=scales1)


def dw_data(data):
    return dict(src=data["src"], w=data["w"], bia=data["bia0"], scales=data["scales0"])


def mid_ref(case, data):
    """the u8 tensor between the stages"""
    return DW.dw_ref(case.dw, dw_data(data))


def acc1_of(mid, w1):
    return mid.astype(np.int64) @ w1.reshape(w1.shape[0], w1.shape[1]).astype(np.int64).T


def ref(case, data):
    f = _requant(acc1_of(mid_ref(case, data), data["w1"]), data["bia1"], data["scales1"], case.relu or case.dst_dt == U8)
    return _store(f, case.dst_dt, case.rm1)


def pw_case(case):
    """the cases.ConvCase of the unfused pointwise conv on the tensor between the stages"""
    return C.ConvCase(case.name, case.bs, case.c, case.oh, case.ow, case.oc, 0, k=(1, 1), stride=(1, 1), pad=(0, 0),
                      dst_dt=case.dst_dt, bia0_dt=case.bia1_dt, relu0=case.relu, rm0=case.rm1, per_channel0=case.pc1,
                      wide=case.wide, seed=case.seed)


def pw_data(case, data, mid):
    return dict(src=mid, w0=data["w1"], w1=None, bia0=data["bia1"], bia1=None, scales0=data["scales1"],
                scales1=np.ones(1, dtype=np.float32))


def fused_dense_case(case):
    """the cases.ConvCase of the FUSED dense conv with ic = oc = c and oc1x1 = oc (dense_expressible cases only)"""
    assert case.dense_expressible, case.ident()
    return C.ConvCase(case.name, case.bs, case.c, case.ih, case.iw, case.c, case.oc, k=case.k, stride=case.stride,
                      pad=case.pad, dst_dt=case.dst_dt, bia0_dt=case.bia0_dt, bia1_dt=case.bia1_dt, relu0=True,
                      relu1=case.relu, rm0=case.rm0, rm1=case.rm1, per_channel0=case.pc0, per_channel1=case.pc1,
                      wide=case.wide, seed=case.seed)


def fused_dense_data(data):
    return dict(src=data["src"], w0=DW.diag_weights(data["w"]), w1=data["w1"], bia0=data["bia0"], bia1=data["bia1"],
                scales0=data["scales0"], scales1=data["scales1"])


# --- the fused kernel's tile plan, as dwpw_api.hip computes it ---------------------------------------------------------
def lds_plan(c, oc, dst_dt, th):
    tw = 256 // (c // 16)
    nblk = -(-th * tw // 32)
    stage = 32 * (oc + 16) if dst_dt in (U8, S8) else 32 * 144
    return c * oc + 12 * oc + nblk * 32 * (c + 16) + 4 * stage


def two_workgroups_fit(case):
    """the instances that run two waves per SIMD (profiles/dwpw/isa_counts.txt): stride 2 with oc = 64.  Only there
    can a second workgroup share the CU, so only there does the host prefer an LDS plan within 80 KB"""
    return case.stride == (2, 2) and case.oc == 64


def tile_of(case):
    """-> (th, tw): the largest height of 16 / 8 / 4 / 2 whose plan fits 160 KB; where two workgroups fit a CU in
    registers, the largest whose plan fits 80 KB if there is one"""
    tw = 256 // (case.c // 16)
    for lim in ((80 << 10, 160 << 10) if two_workgroups_fit(case) else (160 << 10,)):
        for th in (16, 8, 4, 2):
            if lds_plan(case.c, case.oc, case.dst_dt, th) <= lim:
                return th, tw
    raise AssertionError(case.ident())


def heights_that_fit(case):
    return [th for th in (16, 8, 4, 2) if lds_plan(case.c, case.oc, case.dst_dt, th) <= (160 << 10)]


# --- options: dst x bias types (both stages) x relu x round modes x scales, plus wide data ----------------------------
OPTIONS = [
    dict(dst_dt=U8, bia0_dt=S32, bia1_dt=S32, pc0=False, pc1=False, rm0=0, rm1=0, relu=True),
    dict(dst_dt=S8, bia0_dt=S8, bia1_dt=F32, pc0=True, pc1=True, rm0=1, rm1=0, relu=False),
    dict(dst_dt=S32, bia0_dt=UNDEF, bia1_dt=U8, pc0=False, pc1=True, rm0=0, rm1=1, relu=False),
    dict(dst_dt=F32, bia0_dt=F32, bia1_dt=S8, pc0=True, pc1=False, rm0=0, rm1=0, relu=True),
    dict(dst_dt=U8, bia0_dt=U8, bia1_dt=UNDEF, pc0=True, pc1=True, rm0=1, rm1=1, relu=False),
    dict(dst_dt=S8, bia0_dt=S32, bia1_dt=S32, pc0=False, pc1=False, rm0=0, rm1=0, relu=True, wide=True),
    dict(dst_dt=S32, bia0_dt=F32, bia1_dt=F32, pc0=True, pc1=True, rm0=0, rm1=0, relu=True),
    dict(dst_dt=U8, bia0_dt=UNDEF, bia1_dt=S8, pc0=False, pc1=False, rm0=0, rm1=0, relu=False, wide=True),
    dict(dst_dt=S8, bia0_dt=S8, bia1_dt=UNDEF, pc0=True, pc1=True, rm0=0, rm1=0, relu=False, wide=True),
    dict(dst_dt=F32, bia0_dt=S8, bia1_dt=S32, pc0=False, pc1=True, rm0=1, rm1=1, relu=False),
    dict(dst_dt=S32, bia0_dt=U8, bia1_dt=S8, pc0=True, pc1=False, rm0=0, rm1=0, relu=False, wide=True),
    dict(dst_dt=F32, bia0_dt=S32, bia1_dt=U8, pc0=False, pc1=False, rm0=0, rm1=0, relu=False),
]

CHANNELS = (32, 96, 128, 256)
OUT_CHANNELS = (64, 128, 256)

# (name, stride, pad, [(bs, ih, iw, out_hw)])
SHAPE_GEOMS = [
    ("s1p1", (1, 1), (1, 1), [(1, 1, 1, None), (2, 2, 3, None), (3, 7, 7, None), (2, 9, 37, None), (1, 3, 130, None)]),
    ("s2same", (2, 2), (0, 0), [(2, 8, 8, (4, 4)), (2, 7, 10, (4, 5))]),          # windows hang over
    ("s2p1", (2, 2), (1, 1), [(2, 8, 8, None), (2, 9, 14, None)]),
]


def shape_table():
    """every geometry x channel count, the output channel counts and the options rotating through them (the option
    index advances by one more per round of 12, so a (c, oc) pair does not keep meeting the same options): all 12
    (c, oc) pairs of the class occur.  Then the cases the rotation does not guarantee: oh = TH + 1 at TH = 16 and at
    TH = 8, a partly empty last 32-pixel block (TW = 42 at TH = 8), and every one of the 24 kernel instances
    (stride x oc x dst type) on a small image."""
    out, i = [], 0
    for name, s, p, imgs in SHAPE_GEOMS:
        for bs, ih, iw, ohw in imgs:
            for c in CHANNELS:
                oc = OUT_CHANNELS[i % 3]
                opt = OPTIONS[(i + i // 12) % len(OPTIONS)]
                out.append(DwPwCase("%s-%dx%d" % (name, ih, iw), bs, c, ih, iw, oc, stride=s, pad=p, out_hw=ohw,
                                    seed=7000 + 13 * i, **opt))
                i += 1
    out.append(DwPwCase("th16+1", 1, 128, 17, 37, 128, seed=7400, **OPTIONS[0]))
    out.append(DwPwCase("th8+1", 1, 256, 9, 37, 256, seed=7401, **OPTIONS[1]))
    out.append(DwPwCase("tw42-th8", 2, 96, 17, 90, 64, stride=(2, 2), seed=7402, **OPTIONS[3]))
    j = 0
    for stride in ((1, 1), (2, 2)):
        for oc in OUT_CHANNELS:
            for dst_dt in (U8, S8, S32, F32):
                opt = dict(OPTIONS[j % len(OPTIONS)], dst_dt=dst_dt)
                out.append(DwPwCase("inst", 1, 32, 5, 6, oc, stride=stride, seed=7450 + j, **opt))
                j += 1
    return out


def options_table():
    out = []
    for i, opt in enumerate(OPTIONS):
        out.append(DwPwCase("opt%d-s1" % i, 2, 32, 9, 11, 64, seed=7500 + i, **opt))
        out.append(DwPwCase("opt%d-s2" % i, 2, 64, 9, 11, 128, stride=(2, 2), seed=7600 + i, **opt))
    return out


def outside_table():
    """outside the fused class, inside what the two ops accept: 5x5, c = 48, c = 512, oc = 96, mixed strides"""
    return [
        DwPwCase("out-k5", 2, 32, 9, 10, 64, k=(5, 5), pad=(2, 2), seed=7700, **OPTIONS[0]),
        DwPwCase("out-c48", 2, 48, 7, 9, 64, seed=7701, **OPTIONS[1]),
        DwPwCase("out-c512", 1, 512, 5, 6, 64, seed=7702, **OPTIONS[2]),
        DwPwCase("out-oc96", 2, 32, 7, 9, 96, seed=7703, **OPTIONS[3]),
        DwPwCase("out-s1x2", 2, 32, 9, 10, 64, stride=(1, 2), seed=7704, **OPTIONS[4]),
        DwPwCase("out-c256oc512", 1, 256, 5, 6, 512, seed=7705, **OPTIONS[0]),       # c * oc beyond 64 KB
    ]


def all_tables():
    return shape_table() + options_table() + outside_table()


# --- fast-route proof edges, per stage: bias and scale finite and (255 * max(P, N) + |bias|) * |scale| <= 2^30.
#     Stage 0: channel EDGE_CHANNEL of the depthwise weights is prescribed (dwconv_ref.EDGES, unchanged); image 0 / 1
#     attains 255 P / -255 N at the centre pixel of a 3x3 image.
#     Stage 1: output channel EDGE_CHANNEL of the pointwise weights is prescribed; the depthwise stage (centre tap 127,
#     scale 1, no bias) drives the tensor between the stages to 255 where the source is 255 and to 0 where it is 0, so
#     image 0 / 1 attains 255 P / -255 N at every pixel. ------------------------------------------------------------------
EDGE_CHANNEL = DW.EDGE_CHANNEL
LIMIT = DW.LIMIT
EDGE_C, EDGE_OC = 32, 64


def _edge1(name, weights, side, scale_log2, over):
    w = np.asarray(weights, dtype=np.int64)
    assert w.size == EDGE_C
    P, N = int(w[w > 0].sum()), int(-w[w < 0].sum())
    assert (P >= N) == (side == "max") and P != N
    mag = (LIMIT >> scale_log2) - 255 * max(P, N) + (1 if over else 0)
    assert mag > 0
    return DW.Edge(name, tuple(int(v) for v in weights), mag if side == "max" else -mag, float(2 ** scale_log2), not over, side)


_WP = (127, 0, -3, 100) * 8
_WN = (-128, 2, -128, -77) * 8
EDGES1 = [
    _edge1("P-last-admitted", _WP, "max", 8, False),
    _edge1("P-first-rejected", _WP, "max", 8, True),
    _edge1("N-last-admitted", _WN, "min", 10, False),
    _edge1("N-first-rejected", _WN, "min", 10, True),
]
EDGES0 = DW.EDGES


def edge0_case(edge, dst_dt):
    """stage-0 edge: dwconv_ref.edge_case widened to 32 channels, under an ordinary pointwise stage"""
    case = DwPwCase("edge0-" + edge.name, 2, EDGE_C, 3, 3, EDGE_OC, dst_dt=dst_dt, bia0_dt=S32, bia1_dt=S32, relu=False,
                    pc0=True, pc1=False, seed=5000)
    data = generate(case)
    w = data["w"].copy()
    w[EDGE_CHANNEL] = np.asarray(edge.weights, dtype=np.int8).reshape(3, 3)
    src = np.random.default_rng(5001).integers(0, 256, data["src"].shape).astype(np.uint8)
    src[0, :, :, EDGE_CHANNEL] = np.where(w[EDGE_CHANNEL] > 0, 255, 0)
    src[1, :, :, EDGE_CHANNEL] = np.where(w[EDGE_CHANNEL] < 0, 255, 0)
    bia0 = data["bia0"].copy()
    bia0[EDGE_CHANNEL] = edge.bias
    scales0 = data["scales0"].copy()
    scales0[EDGE_CHANNEL] = np.float32(edge.scale)
    return case, dict(data, src=src, w=w, bia0=bia0, scales0=scales0)


def edge0_attained(edge, case, data):
    acc = DW.dw_acc(data["src"], data["w"], case.stride, case.pad, (case.oh, case.ow))
    w = np.asarray(edge.weights, dtype=np.int64)
    P, N = int(w[w > 0].sum()), int(-w[w < 0].sum())
    img = 0 if edge.which == "max" else 1
    return int(acc[img, 1, 1, EDGE_CHANNEL]), (255 * P if edge.which == "max" else -255 * N), P, N


def edge1_case(edge, dst_dt):
    case = DwPwCase("edge1-" + edge.name, 2, EDGE_C, 3, 3, EDGE_OC, dst_dt=dst_dt, bia0_dt=UNDEF, bia1_dt=S32, relu=False,
                    pc0=False, pc1=True, seed=5100)
    data = generate(case)
    w = np.zeros((EDGE_C, 3, 3), dtype=np.int8)
    w[:, 1, 1] = 127
    w1 = data["w1"].copy()
    w1[EDGE_CHANNEL, :, 0, 0] = np.asarray(edge.weights, dtype=np.int8)
    src = np.random.default_rng(5101).integers(0, 256, data["src"].shape).astype(np.uint8)
    row = w1[EDGE_CHANNEL, :, 0, 0]
    src[0] = np.where(row > 0, 255, 0)
    src[1] = np.where(row < 0, 255, 0)
    bia1 = data["bia1"].copy()
    bia1[EDGE_CHANNEL] = edge.bias
    scales1 = data["scales1"].copy()
    scales1[EDGE_CHANNEL] = np.float32(edge.scale)
    return case, dict(data, src=src, w=w, bia0=None, scales0=np.ones(1, dtype=np.float32), w1=w1, bia1=bia1, scales1=scales1)


def edge1_attained(edge, case, data):
    """the edge channel's stage-1 accumulator on the attaining image (every pixel has it), and the proof's bound"""
    acc = acc1_of(mid_ref(case, data), data["w1"])
    w = np.asarray(edge.weights, dtype=np.int64)
    P, N = int(w[w > 0].sum()), int(-w[w < 0].sum())
    img = 0 if edge.which == "max" else 1
    vals = set(int(v) for v in acc[img, :, :, EDGE_CHANNEL].flat)
    assert len(vals) == 1, vals
    return vals.pop(), (255 * P if edge.which == "max" else -255 * N), P, N
