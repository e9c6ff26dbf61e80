"""Reference, data and case tables of the fully-connected op's tests (pure numpy, needs no GPU).

The op is defined by the existing conv: where ic and oc are multiples of 16 it equals the unfused dense conv whose window
is the whole image (kh = ih, kw = iw, stride 1, no padding, oh = ow = 1).  fc_ref is an independent numpy formulation --
one int64 matrix product of the flattened NHWC source with the weights permuted from oihw to (y, x, c) order, then
refmath's _requant / _store, unchanged -- which tests/test_fc_cpu.py pins against the C oracle's dense conv and
tests/test_gpu_fc.py compares the GPU against, bit for bit.
"""
from dataclasses import dataclass, replace

import numpy as np

import cases as C
from dwconv_ref import EDGES, LIMIT, OPTIONS  # noqa: F401  (the depthwise op's option rows and proof edges)
from refmath import _requant, _store

F32, S32, S8, U8, UNDEF = C.F32, C.S32, C.S8, C.U8, C.UNDEF
MFMA, GENERIC = 0, 1            # DFX_FC_MFMA / DFX_FC_GENERIC
KMAX = 65025


@dataclass(frozen=True)
class FcCase:
    name: str
    bs: int
    ic: int
    ih: int
    iw: int
    oc: int
    dst_dt: int = U8
    bia_dt: int = S32
    relu: bool = True
    rm: int = 0
    per_channel: bool = False
    wide: bool = False                            # full-range data, scales that reach both saturation ends
    seed: int = 1234

    @property
    def K(self):
        return self.ih * self.iw * self.ic

    @property
    def mfma_class(self):
        return self.K % 64 == 0

    @property
    def dense_expressible(self):
        """the dense conv (channel blocks of 16) can express the case"""
        return self.ic % 16 == 0 and self.oc % 16 == 0

    def ident(self):
        return "%s-n%d-%dx%dx%d-oc%d-%s-b%s-r%d-m%d-pc%d%s" % (
            self.name, self.bs, self.ih, self.iw, self.ic, self.oc, C.NAME_OF[self.dst_dt], C.NAME_OF[self.bia_dt],
            self.relu, self.rm, self.per_channel, "-wide" if self.wide else "")


def generate(case):
    """-> dict(src NHWC u8, w s8 {oc, ic, ih, iw}, bia, scales).  Reference-range data (cases.py), or "wide": full-range
    activations and weights with -128 and 127 present, and scales eight times the size that centres the output, so
    that both saturation ends of a 1-byte dst are reached.  The weights are random per (o, c, y, x): a transposed or
    permuted fragment cannot pass."""
    rng = np.random.default_rng(case.seed)
    if case.wide:
        src = rng.integers(0, 256, (case.bs, case.ih, case.iw, case.ic)).astype(np.uint8)
        w = rng.integers(-128, 128, (case.oc, case.ic, case.ih, case.iw)).astype(np.int8)
        w[0].flat[0] = -128
        w[case.oc - 1].flat[-1] = 127
    else:
        src = rng.integers(0, 17, (case.bs, case.ih, case.iw, case.ic)).astype(np.uint8)
        w = rng.integers(-10, 11, (case.oc, case.ic, case.ih, case.iw)).astype(np.int8)
    amp = (74.0 * 147.0 / 8.0 if case.wide else 6.0 * 9.0) * np.sqrt(case.K)
    s = np.float32(80.0 / amp)
    if case.per_channel:
        scales = (s * (0.5 + np.arange(case.oc) / case.oc)).astype(np.float32)
    else:
        scales = np.array([s], dtype=np.float32)
    return dict(src=src, w=w, bia=C._bias(rng, case.oc, case.bia_dt, case.wide), scales=scales)


def fc_acc(src, w):
    """exact int64 accumulators {bs, oc}: the flattened NHWC source against the weights in (y, x, c) order"""
    bs, oc = src.shape[0], w.shape[0]
    return src.reshape(bs, -1).astype(np.int64) @ w.transpose(0, 2, 3, 1).reshape(oc, -1).astype(np.int64).T


def fc_ref(case, data):
    f = _requant(fc_acc(data["src"], data["w"]), data["bia"], data["scales"], case.relu or case.dst_dt == U8)
    return _store(f, case.dst_dt, case.rm)


def dense_case(case):
    """the cases.ConvCase of the equivalent unfused dense conv (dense_expressible cases only): the window is the image"""
    assert case.dense_expressible, case.ident()
    return C.ConvCase(case.name, case.bs, case.ic, case.ih, case.iw, case.oc, 0, k=(case.ih, case.iw), stride=(1, 1),
                      pad=(0, 0), dst_dt=case.dst_dt, bia0_dt=case.bia_dt, relu0=case.relu, rm0=case.rm,
                      per_channel0=case.per_channel, wide=case.wide, seed=case.seed)


def dense_data(case, data):
    return dict(src=data["src"], w0=data["w"], w1=None, bia0=data["bia"], bia1=None, scales0=data["scales"],
                scales1=np.ones(1, dtype=np.float32))


# --- the planner of fc_api.hip, mirrored: the tests assert info().splitk from it --------------------------------------
SLAB_CAP, TILE = 64 << 20, 8


def planned_splitk(case, cus, forced=None):
    nks = case.K // 64
    ocb = -(-case.oc // 32)
    base = -(-ocb // 4) * -(-case.bs // 128)
    if forced is not None:
        sk = forced
    else:
        sk = max(1, cus // base)
        sk = min(sk, max(1, SLAB_CAP // (-(-case.bs // 32) * 32 * ocb * 32 * 4)))
        sk = min(sk, -(-nks // TILE))
    return max(1, min(sk, nks))


# --- the MFMA kernel's class: K % 64 == 0 ---------------------------------------------------------------------------------
MFMA_BS = (1, 2, 31, 32, 33, 130)          # partial column blocks; a second batch chunk with a partial tail
MFMA_OC = (1, 10, 32, 33, 96, 130)         # partial oc blocks; 1-byte rows that are not 4-byte aligned
MFMA_SHAPES = [(1, 1, 64), (1, 1, 192), (2, 2, 16), (1, 3, 64), (7, 7, 64), (1, 1, 2048)]   # (ih, iw, ic)


def mfma_table():
    """every shape x bs x oc, the options rotating through them"""
    out, i = [], 0
    for ih, iw, ic in MFMA_SHAPES:
        for bs in MFMA_BS:
            for oc in MFMA_OC:
                out.append(FcCase("mfma", bs, ic, ih, iw, oc, seed=20000 + 7 * i, **OPTIONS[i % len(OPTIONS)]))
                i += 1
    return out


SPLITK_SHAPES = [(1, 1, 448), (7, 7, 64)]  # 7 and 49 k-steps
SPLITK_VALUES = (1, 2, 3, 7, 64)


def splitk_table():
    """four option rows (every dst type) per shape; bs and oc with partial blocks"""
    out = []
    for j, (ih, iw, ic) in enumerate(SPLITK_SHAPES):
        for i in range(4):
            out.append(FcCase("splitk", 33, ic, ih, iw, 130 if i % 2 else 33, seed=21000 + 10 * j + i, **OPTIONS[i]))
    return out


GENERIC_SHAPES = [(1, 1, 100), (5, 5, 3), (1, 1, 17)]


def generic_table():
    out, i = [], 0
    for ih, iw, ic in GENERIC_SHAPES:
        for oc in (7, 16):
            for bs in (1, 5):
                out.append(FcCase("gen", bs, ic, ih, iw, oc, seed=22000 + i, **OPTIONS[i % len(OPTIONS)]))
                i += 1
    return out


TWIN_SHAPES = [((1, 1, 256), 64), ((3, 3, 32), 48), ((7, 7, 64), 32)]


def twin_table():
    """conv equivalence: every dst type per shape"""
    out = []
    for j, ((ih, iw, ic), oc) in enumerate(TWIN_SHAPES):
        for i, opt in enumerate(OPTIONS[:4]):
            out.append(FcCase("twin", 5, ic, ih, iw, oc, seed=23000 + 10 * j + i, **opt))
    return out


def all_tables():
    return mfma_table() + splitk_table() + generic_table() + twin_table()


def permutation_case():
    """ih * iw > 1 and a weight tensor whose every (o, c, y, x) holds another value (mod 251, then centred): a packer
    or a reference that swaps two axes cannot pass"""
    case = FcCase("perm", 3, 16, 2, 3, 16, dst_dt=S32, bia_dt=UNDEF, relu=False, seed=24000)
    data = generate(case)
    w = ((np.arange(16 * 16 * 2 * 3) * 37) % 251 - 125).astype(np.int8).reshape(16, 16, 2, 3)
    return case, dict(data, w=w, scales=np.ones(1, dtype=np.float32))


# --- accumulator bounds: K = 65024, the largest K of the MFMA class -------------------------------------------------------
def bounds_case():
    """-> (case, data): channel 0 all 127, channel 1 all -128; image 0 all 255, image 1 all 0; s32 dst, scale 1"""
    case = FcCase("bounds", 2, 65024, 1, 1, 32, dst_dt=S32, bia_dt=UNDEF, relu=False, seed=25000)
    data = generate(case)
    w = data["w"].copy()
    w[0], w[1] = 127, -128
    src = data["src"].copy()
    src[0], src[1] = 255, 0
    return case, dict(src=src, w=w, bia=None, scales=np.ones(1, dtype=np.float32))


# --- fast-route proof edges (dfx.h, dfx_fc_set_weights): dwconv_ref's EDGES, the edge channel's nine prescribed weights
#     on the first nine of its K = 64 taps, zero on the others.  The activations of image 0 / 1 attain the accumulator's
#     maximum 255 P / minimum -255 N. ---------------------------------------------------------------------------------
EDGE_CHANNEL = 5


def _next_scale(e):
    """the edge with the next f32 scale above: (255 * max(P, N) + |bias|) * scale is 2^30 * (1 + 2^-23), rejected"""
    return replace(e, name=e.name.replace("admitted", "next-scale-rejected"), fast=False,
                   scale=float(np.nextafter(np.float32(e.scale), np.float32(np.inf))))


FC_EDGES = [e2 for e in EDGES if e.fast for e2 in (e, _next_scale(e))]


def edge_case(edge, dst_dt):
    """-> (case, data): 2 images of 1x1x64, oc 33, per-channel scales and s32 bias; channel EDGE_CHANNEL as prescribed"""
    case = FcCase("edge-" + edge.name, 2, 64, 1, 1, 33, dst_dt=dst_dt, bia_dt=S32, relu=False, rm=0, per_channel=True, seed=26000)
    data = generate(case)
    w = data["w"].copy()
    w[EDGE_CHANNEL] = 0
    w[EDGE_CHANNEL, :9, 0, 0] = edge.weights
    src = np.random.default_rng(26001).integers(0, 256, data["src"].shape).astype(np.uint8)
    src[0, 0, 0, :] = np.where(w[EDGE_CHANNEL, :, 0, 0] > 0, 255, 0)      # attains 255 P
    src[1, 0, 0, :] = np.where(w[EDGE_CHANNEL, :, 0, 0] < 0, 255, 0)      # attains -255 N
    bia = data["bia"].copy()
    bia[EDGE_CHANNEL] = edge.bias
    scales = data["scales"].copy()
    scales[EDGE_CHANNEL] = np.float32(edge.scale)
    return case, dict(src=src, w=w, bia=bia, scales=scales)


def edge_attained(edge, case, data):
    """the edge channel's accumulator on the attaining image, and the bound the proof uses"""
    acc = fc_acc(data["src"], data["w"])
    w = np.asarray(edge.weights, dtype=np.int64)
    P, N = int(w[w > 0].sum()), int(-w[w < 0].sum())
    img = 0 if edge.which == "max" else 1
    return int(acc[img, EDGE_CHANNEL]), (255 * P if edge.which == "max" else -255 * N), P, N
