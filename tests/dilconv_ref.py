"""Reference, data and case tables of the dilated conv tests (pure numpy, needs no GPU).

The op is defined by the existing ops: with the zero-stuffed weights wz[o,i,ky*dh,kx*dw] = w[o,i,ky,kx] it equals the
grouped conv with groups = 1 on wz (same stride, padding and output size) wherever that window can be expressed, where
ic and oc are multiples of 16 and the output size is the conv formula's the unfused dense conv on wz, and at
dh = dw = 1 the grouped conv on the same tensors.  dilconv_ref is an independent numpy formulation -- a GATHER: for
every tap (ky, kx) the strided view of the zero-padded source that starts at (ky*dh, kx*dw) is multiplied with
w[:, :, ky, kx] (a float64 matrix product: every partial sum is an integer far below 2^53, so it is exact); then
refmath's _requant / _store, unchanged -- which tests/test_dilconv_cpu.py pins against the C oracle's dense conv on wz
and against gconv_ref, and tests/test_gpu_dilconv.py compares the GPU against, bit for bit.  No stuffed weight and no
zero tap appears in it.
"""
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

import cases as C
from dwconv_ref import EDGES, EDGE_CHANNEL, LIMIT, OPTIONS  # noqa: F401  (the depthwise op's option rows and proof edges)
from refmath import _requant, _store

F32, S32, S8, U8, UNDEF = C.F32, C.S32, C.S8, C.U8, C.UNDEF
MFMA, GENERIC = 0, 1            # DFX_DILCONV_MFMA / DFX_DILCONV_GENERIC
# the MFMA kernel's LDS plan (dilconv.cuh, dilconv_api.hip): 9 KB per K-step and output block, chunks of 4 blocks, the
# constants (3 x 128 dwords) and 8 waves' staging rows (32 x 144 bytes each)
LDS_LIMIT, FIXED_LDS, CHUNK, KSTEP, WAVES = 160 * 1024, 3 * 128 * 4 + 8 * 32 * 144, 4, 9 * 1024, 8
WREG = 5                                          # 16-byte pieces of a slab a thread carries in registers (two slab buffers)
DEFAULT_SLAB, DEFAULT_STRIPS = 3, 1


@dataclass(frozen=True)
class DlCase:
    name: str
    bs: int
    c: int                                        # input channels
    ih: int
    iw: int
    oc: int
    k: Tuple[int, int] = (3, 3)
    stride: Tuple[int, int] = (1, 1)
    dil: Tuple[int, int] = (1, 1)                 # dh, dw
    pad: Tuple[int, int] = (0, 0)                 # pad_t, pad_l
    out_hw: Optional[Tuple[int, int]] = None      # None: (in + 2 * pad - ((k - 1) * d + 1)) // stride + 1
    dst_dt: int = U8
    bia_dt: int = S32
    relu: bool = True
    rm: int = 0
    per_channel: bool = False
    wide: bool = False                            # full-range data, scales that reach both saturation ends
    seed: int = 1234

    @property
    def ext(self):
        """the stuffed window ((kh - 1) * dh + 1, (kw - 1) * dw + 1)"""
        return ((self.k[0] - 1) * self.dil[0] + 1, (self.k[1] - 1) * self.dil[1] + 1)

    @property
    def oh(self):
        return self.out_hw[0] if self.out_hw else (self.ih + 2 * self.pad[0] - self.ext[0]) // self.stride[0] + 1

    @property
    def ow(self):
        return self.out_hw[1] if self.out_hw else (self.iw + 2 * self.pad[1] - self.ext[1]) // self.stride[1] + 1

    @property
    def mfma_class(self):
        return self.k == (3, 3) and self.stride == (1, 1) and self.c % 32 == 0 and self.oc % 32 == 0

    @property
    def stuffed_expressible(self):
        """dfx_gconv accepts the stuffed window (its accumulator bound counts the zero taps too)"""
        return self.ext[0] * self.ext[1] * self.c <= 65025 and max(self.ext) <= 255

    @property
    def dense_expressible(self):
        """the dense conv (symmetric padding, derived output size, channel blocks of 16) can express the case on wz"""
        return self.stuffed_expressible and self.out_hw is None and self.c % 16 == 0 and self.oc % 16 == 0

    def ident(self):
        return "%s-n%d-c%d-%dx%d-oc%d-k%dx%d-s%dx%d-d%dx%d-p%d,%d-o%dx%d-%s-b%s-r%d-m%d-pc%d%s" % (
            self.name, self.bs, self.c, self.ih, self.iw, self.oc, self.k[0], self.k[1], self.stride[0], self.stride[1],
            self.dil[0], self.dil[1], self.pad[0], self.pad[1], self.oh, self.ow, C.NAME_OF[self.dst_dt],
            C.NAME_OF[self.bia_dt], self.relu, self.rm, self.per_channel, "-wide" if self.wide else "")


def lds_plan(c, oc, slab=None):
    """-> (K-steps per slab, slab buffers, LDS bytes) as dfx_dilconv_create plans them for a request of `slab` K-steps
    per slab (None: the default).  Nothing but the clamp to the K-steps that exist depends on ic."""
    wblocks, ksteps = min(CHUNK, oc // 32), c // 32
    kstep_bytes = wblocks * KSTEP
    s = min(max(1, min(DEFAULT_SLAB if slab is None else slab, (LDS_LIMIT - FIXED_LDS) // kstep_bytes)), ksteps)
    nbuf = 2 if (s < ksteps and 2 * s * kstep_bytes + FIXED_LDS <= LDS_LIMIT and s * kstep_bytes <= WREG * WAVES * 64 * 16) else 1
    return s, nbuf, nbuf * s * kstep_bytes + FIXED_LDS


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


def dilconv_acc(src, w, stride, dil, pad, out_hw, rows=None):
    """exact int64 accumulators {bs, oh (or len(rows)), ow, oc}, as a gather: for every tap (ky, kx) the view of the
    zero-padded source at rows oy * sh + ky * dh and columns ox * sw + kx * dw times w[:, :, ky, kx].  rows: the output
    rows to return (all by default)"""
    bs, ih, iw, c = src.shape
    oc, ic, kh, kw = w.shape
    assert c == ic and kh * kw * ic * 255 * 128 < 2 ** 53
    (sh, sw), (dh, dw), (oh, ow) = stride, dil, out_hw
    assert (oh - 1) * sh - pad[0] <= ih - 1 and (ow - 1) * sw - pad[1] <= iw - 1, (out_hw, src.shape, pad)
    need_h = max((oh - 1) * sh + (kh - 1) * dh + 1, pad[0] + ih)
    need_w = max((ow - 1) * sw + (kw - 1) * dw + 1, pad[1] + iw)
    buf = np.zeros((bs, need_h, need_w, c), dtype=np.float64)
    buf[:, pad[0]:pad[0] + ih, pad[1]:pad[1] + iw, :] = src
    ys = np.arange(oh) if rows is None else np.asarray(list(rows))
    acc = np.zeros((bs, len(ys), ow, oc), dtype=np.int64)
    for ky in range(kh):
        for kx in range(kw):
            v = buf[:, ys * sh + ky * dh][:, :, kx * dw:kx * dw + (ow - 1) * sw + 1:sw, :]
            acc += (v.reshape(-1, c) @ w[:, :, ky, kx].T.astype(np.float64)).reshape(bs, len(ys), ow, oc).astype(np.int64)
    return acc


def dilconv_ref(case, data, rows=None):
    acc = dilconv_acc(data["src"], data["w"], case.stride, case.dil, case.pad, (case.oh, case.ow), rows)
    f = _requant(acc, data["bia"], data["scales"], case.relu or case.dst_dt == U8)
    return _store(f, case.dst_dt, case.rm)


# --- the twins of the defining properties: the same conv on the zero-stuffed weights ---------------------------------------
def stuff_weights(w, dil):
    """{oc, ic, kh, kw} -> {oc, ic, (kh-1)*dh+1, (kw-1)*dw+1}: w at the multiples of the dilation, 0 elsewhere"""
    oc, ic, kh, kw = w.shape
    wz = np.zeros((oc, ic, (kh - 1) * dil[0] + 1, (kw - 1) * dil[1] + 1), dtype=w.dtype)
    wz[:, :, ::dil[0], ::dil[1]] = w
    return wz


def dense_case(case):
    """the cases.ConvCase of the equivalent unfused dense conv on wz (dense_expressible cases only)"""
    assert case.dense_expressible, case.ident()
    return C.ConvCase(case.name, case.bs, case.c, case.ih, case.iw, case.oc, 0, k=case.ext, stride=case.stride, pad=case.pad,
                      dst_dt=case.dst_dt, bia0_dt=case.bia_dt, relu0=case.relu, rm0=case.rm, per_channel0=case.per_channel,
                      wide=case.wide, seed=case.seed)


def dense_data(case, data):
    return dict(src=data["src"], w0=stuff_weights(data["w"], case.dil), w1=None, bia0=data["bia"], bia1=None,
                scales0=data["scales"], scales1=np.ones(1, dtype=np.float32))


# --- the MFMA kernel's class: the smallest shapes at which each mechanism can go wrong -----------------------------------
# (name, bs, ih, iw, ic, oc, (dh, dw), (pad_t, pad_l), out_hw)
MFMA_GEOMS = [
    ("base", 1, 8, 8, 32, 32, (2, 2), (2, 2), None),                # two full strips
    ("rows-d1", 2, 7, 5, 32, 32, (1, 1), (1, 1), None),             # 70 pixels: strips cross rows and images, ragged last strip
    ("rows-d2", 2, 7, 5, 32, 32, (2, 2), (2, 2), None),
    ("far-d18", 2, 7, 5, 32, 32, (18, 18), (18, 18), None),         # every tap but the centre is outside the image
    ("aniso31-p10", 2, 11, 9, 32, 32, (3, 1), (1, 0), None),        # dh != dw, pad < d: 7 x 7
    ("aniso31-p00", 2, 11, 9, 32, 32, (3, 1), (0, 0), None),        # pad 0: the output shrinks to 5 x 7
    ("aniso25-p10", 2, 11, 9, 32, 32, (2, 5), (1, 0), (8, 4)),      # cropped (9 rows exist); the 11-wide window hangs over
    ("aniso25-p00", 2, 11, 9, 32, 32, (2, 5), (0, 0), (6, 3)),
    ("slabs", 1, 6, 7, 96, 32, (2, 2), (2, 2), None),               # three K-steps
    ("slabs-oc160", 1, 6, 7, 96, 160, (2, 1), (2, 1), None),        # ... under chunks of 4 + 1 blocks
    ("chunks", 1, 6, 7, 32, 160, (2, 2), (2, 2), None),             # chunks of 4 + 1 blocks
    ("strips", 2, 13, 12, 32, 160, (3, 3), (3, 3), None),           # 312 pixels: ten strips (the last one ragged) for eight waves
]


def mfma_case(name, opt=0, **kw):
    _, bs, ih, iw, c, oc, d, p, ohw = [g for g in MFMA_GEOMS if g[0] == name][0]
    args = dict(OPTIONS[opt % len(OPTIONS)])
    args.update(kw)
    return DlCase(name, bs, c, ih, iw, oc, dil=d, pad=p, out_hw=ohw, seed=41000 + 17 * opt + len(name), **args)


def mfma_table(geom=None):
    """every geometry under every option row: all four dst types, every bias type and none, ReLU on / off, both round
    modes, one / per-channel scales, reference-range and wide data"""
    return [mfma_case(g[0], i) for g in MFMA_GEOMS if geom in (None, g[0]) for i in range(len(OPTIONS))]


# what only the generic path covers: (window, stride, dilation, pad, ih, iw, out_hw) x ic in {3, 20} x oc in {5, 48}
GENERIC_GEOMS = [
    ((5, 5), (2, 2), (3, 3), (6, 6), 15, 14, None),        # 5x5 window, stride 2, d 3
    ((3, 3), (2, 2), (2, 2), (2, 2), 9, 8, None),          # the class's window at stride 2
    ((3, 3), (1, 1), (2, 3), (2, 0), 8, 9, None),          # the class's window and stride on channels that are not blocks
    ((1, 3), (1, 2), (1, 4), (0, 4), 5, 11, None),         # a row window
    ((2, 2), (1, 1), (7, 7), (3, 3), 6, 6, (6, 6)),        # even window, output size given
]


def generic_table():
    out, i = [], 0
    for k, s, d, p, ih, iw, ohw in GENERIC_GEOMS:
        for c in (3, 20):
            for oc in (5, 48):
                out.append(DlCase("gen", 2, c, ih, iw, oc, k=k, stride=s, dil=d, pad=p, out_hw=ohw, seed=42000 + i,
                                  **OPTIONS[i % len(OPTIONS)]))
                i += 1
    # inside the window / stride clauses of the class but outside its channel clause, and the reverse
    out.append(DlCase("gen-c48", 1, 48, 6, 6, 32, dil=(2, 2), pad=(2, 2), seed=42100, **OPTIONS[0]))
    out.append(DlCase("gen-s2", 1, 32, 9, 9, 32, stride=(2, 2), dil=(2, 2), pad=(2, 2), seed=42101, **OPTIONS[1]))
    return out


def all_tables():
    return mfma_table() + generic_table()


# --- permutation: within an output channel every run of 255 taps that are consecutive in (i, ky, kx) order is distinct,
#     and at every (i, ky, kx) the output channels of a 32-block are distinct, and the activations are random over the
#     whole range, so that a swapped tap, channel, K-step, slab or block in the packer or the kernel changes the bytes.
#     s32 dst, scale 1, no bias: the accumulators themselves. -----------------------------------------------------------------
def permutation_case(name):
    base = mfma_case(name)
    case = DlCase("perm-" + name, base.bs, base.c, base.ih, base.iw, base.oc, dil=base.dil, pad=base.pad, out_hw=base.out_hw,
                  dst_dt=S32, bia_dt=UNDEF, relu=False, seed=43000 + len(name))
    taps = case.c * 9
    idx = np.arange(taps)[None, :] + 7 * np.arange(case.oc)[:, None]
    w = ((idx % 255) - 127).astype(np.int8).reshape(case.oc, case.c, 3, 3)
    src = np.random.default_rng(case.seed).integers(0, 256, (case.bs, case.ih, case.iw, case.c)).astype(np.uint8)
    return case, dict(src=src, w=w, bia=None, scales=np.ones(1, dtype=np.float32))


# --- fast-route proof edges (dfx.h, dfx_dilconv_set_weights): dwconv_ref's EDGES on a 3x3 d 2 pad 2 op over a 5x5 image.
#     Output pixel (2, 2) reaches all nine taps, at the input pixels (2 ky, 2 kx).  The edge channel's nine prescribed
#     weights sit on nine (tap, input channel) positions, one per tap; every other weight of the channel is zero.  Image
#     0 / 1 holds 255 where the weight is positive / negative, so the accumulator of (2, 2) attains 255 P / -255 N. -----
EDGE_IC, EDGE_OC, EDGE_PIXEL, EDGE_DIL = 64, 32, (2, 2), (2, 2)
EDGE_POSITIONS = [(0, 0, 0), (0, 1, 1), (0, 2, 31), (1, 0, 32), (1, 1, 17), (1, 2, 63), (2, 0, 4), (2, 1, 48), (2, 2, 33)]  # (ky, kx, i)


def edge_case(edge, dst_dt):
    """-> (case, data): 2 images of 5x5x64 (two K-steps), per-channel scales and s32 bias; channel EDGE_CHANNEL as prescribed"""
    case = DlCase("edge-" + edge.name, 2, EDGE_IC, 5, 5, EDGE_OC, dil=EDGE_DIL, pad=(2, 2), dst_dt=dst_dt, bia_dt=S32,
                  relu=False, rm=0, per_channel=True, seed=44000)
    data = generate(case)
    w = data["w"].copy()
    w[EDGE_CHANNEL] = 0
    src = np.random.default_rng(44001).integers(0, 256, data["src"].shape).astype(np.uint8)
    for (ky, kx, i), v in zip(EDGE_POSITIONS, edge.weights):
        w[EDGE_CHANNEL, i, ky, kx] = v
        iy, ix = EDGE_PIXEL[0] - 2 + ky * EDGE_DIL[0], EDGE_PIXEL[1] - 2 + kx * EDGE_DIL[1]
        src[0, iy, ix, i] = 255 if v > 0 else 0      # attains 255 P at EDGE_PIXEL
        src[1, iy, ix, i] = 255 if v < 0 else 0      # attains -255 N
    bia = data["bia"].copy()
    bia[EDGE_CHANNEL] = edge.bias
    scales = data["scales"].copy()
    scales[EDGE_CHANNEL] = np.float32(edge.scale)
    return case, dict(src=src, w=w, bia=bia, scales=scales)


def edge_attained(edge, case, data):
    """EDGE_PIXEL's accumulator of the edge channel on the attaining image, and the bound the proof uses"""
    acc = dilconv_acc(data["src"], data["w"], case.stride, case.dil, case.pad, (case.oh, case.ow))
    w = np.asarray(edge.weights, dtype=np.int64)
    P, N = int(w[w > 0].sum()), int(-w[w < 0].sum())
    img = 0 if edge.which == "max" else 1
    return int(acc[img, EDGE_PIXEL[0], EDGE_PIXEL[1], EDGE_CHANNEL]), (255 * P if edge.which == "max" else -255 * N), P, N
