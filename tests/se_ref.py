"""Reference, data and case tables of the squeeze-and-excitation op's tests (pure numpy, needs no GPU).

The op is defined by ops the library has: its first stage is average pooling with the window of the image, its two tiny
layers are the fully-connected op with u8 (ReLU) and s8 results, then a 256-entry table and a per-(image, channel)
rescale with the conv's requant chain (include/dfx.h).  `stages` is an independent numpy formulation -- int64 sums and
matrix products, refmath's _requant / _store unchanged -- which tests/test_se_cpu.py pins against a scalar loop, refmath's
average pooling and fc_ref, and tests/test_gpu_se.py compares the GPU against, bit for bit.
"""
import functools
from dataclasses import dataclass, replace

import numpy as np

import cases as C
import requant_edges as E
from refmath import _requant, _store

F32, S32, S8, U8, UNDEF = C.F32, C.S32, C.S8, C.U8, C.UNDEF
BAND, GENERIC = 0, 1                    # DFX_SE_BAND / DFX_SE_GENERIC
SCALE, GATE, SQUEEZE = 0, 1, 2          # DFX_SE_SCALE / DFX_SE_GATE / DFX_SE_SQUEEZE
MODES = (SCALE, GATE, SQUEEZE)
FLUSH = 257                             # pixels a packed 16-bit accumulator of the squeeze kernel takes
MAX_PX, MAX_C = 1 << 23, 16384


@dataclass(frozen=True)
class SeCase:
    name: str
    bs: int
    ih: int
    iw: int
    c: int
    cr: int
    bia1_dt: int = S32
    bia2_dt: int = S32
    rm: int = 0
    per_channel: bool = False
    wide: bool = False                  # out_scale = 1 / 100: u8 saturation of dst on purpose
    seed: int = 4000

    @property
    def px(self):
        return self.ih * self.iw

    @property
    def band_class(self):
        return self.c % 16 == 0 and self.px * self.c < 2 ** 31

    def ident(self):
        return "%s-n%d-%dx%dx%d-cr%d-b%s%s-m%d-pc%d%s" % (
            self.name, self.bs, self.ih, self.iw, self.c, self.cr, C.NAME_OF[self.bia1_dt], C.NAME_OF[self.bia2_dt], self.rm,
            self.per_channel, "-wide" if self.wide else "")


def sigmoid_table(div=24.0):
    """lut[i] = rint(255 * sigmoid((i - 128) / div))"""
    t = np.arange(256, dtype=np.float64) - 128
    return np.rint(255.0 / (1.0 + np.exp(-t / div))).astype(np.uint8)


def hard_sigmoid_table(div=16.0):
    """MobileNetV3's gate: rint(255 * relu6(t / div + 3) / 6)"""
    t = np.arange(256, dtype=np.float64) - 128
    return np.rint(255.0 * np.clip(t / div + 3.0, 0.0, 6.0) / 6.0).astype(np.uint8)


def _bias(rng, n, dt):
    if dt == UNDEF:
        return None
    v = rng.integers(-2000, 2001, n)
    return (v + 0.5).astype(np.float32) if dt == F32 else v.astype(np.int32)


def _draw(case, seed):
    rng = np.random.default_rng(seed)
    amp = rng.integers(1, 256, (case.bs, 1, 1, case.c))         # an amplitude per (image, channel): the means differ
    src = (rng.integers(0, 256, (case.bs, case.ih, case.iw, case.c)) * amp // 255).astype(np.uint8)
    w1 = rng.integers(-127, 128, (case.cr, case.c)).astype(np.int8)
    w2 = rng.integers(-127, 128, (case.c, case.cr)).astype(np.int8)
    s1 = np.float32(96.0 / (np.sqrt(case.c) * 64.0 * 73.0))
    s2 = np.float32(48.0 / (np.sqrt(case.cr) * 60.0 * 73.0))
    so = np.float32(1.0 / 100.0 if case.wide else 1.0 / 255.0)
    if case.per_channel:
        scales1 = (s1 * (0.9 + 0.2 * np.arange(case.cr) / case.cr)).astype(np.float32)
        scales2 = (s2 * (0.9 + 0.2 * np.arange(case.c) / case.c)).astype(np.float32)
        out_scales = (so * (0.9 + 0.2 * ((np.arange(case.c) * 7) % 11) / 11.0)).astype(np.float32)
    else:
        scales1, scales2, out_scales = (np.array([v], dtype=np.float32) for v in (s1, s2, so))
    return dict(src=src, w1=w1, w2=w2, bia1=_bias(rng, case.cr, case.bia1_dt), bia2=_bias(rng, case.c, case.bia2_dt),
                scales1=scales1, scales2=scales2, out_scales=out_scales, lut=sigmoid_table())


def gate_stages(case, data):
    """-> dict(sum, z, h, t, g): the formula of dfx.h up to the gate, in int64 / float32"""
    tot = data["src"].sum(axis=(1, 2), dtype=np.int64)                                    # {bs, c}, exact
    q = np.rint(tot.astype(np.float32) / np.float32(case.px))
    z = np.clip(q, 0, 255).astype(np.uint8)
    a1 = z.astype(np.int64) @ data["w1"].astype(np.int64).T
    h = _store(_requant(a1, data["bia1"], data["scales1"], True), U8, case.rm)
    a2 = h.astype(np.int64) @ data["w2"].astype(np.int64).T
    t = _store(_requant(a2, data["bia2"], data["scales2"], False), S8, case.rm)
    g = data["lut"][t.astype(np.int64) + 128]
    return dict(sum=tot, z=z, h=h, t=t, g=g)


def stages(case, data):
    """-> dict(sum, z, h, t, g, dst): every stage"""
    st = gate_stages(case, data)
    m = data["src"].astype(np.int64) * st["g"].astype(np.int64)[:, None, None, :]
    st["dst"] = _store(_requant(m, None, data["out_scales"], True), U8, case.rm)
    return st


def conditions(case, data, st):
    """-> list of violated conditions: the data of a case must not let a kernel error hide behind a degenerate stage"""
    bad = []
    h, t, g, dst, src = st["h"], st["t"], st["g"], st["dst"], data["src"]
    if np.mean(h == 0) > 0.85:
        bad.append("h == 0 on %.2f" % np.mean(h == 0))
    if np.mean(h == 255) > 0.10:
        bad.append("h == 255 on %.2f" % np.mean(h == 255))
    if np.mean((t == -128) | (t == 127)) > 0.10:
        bad.append("t saturated on %.2f" % np.mean((t == -128) | (t == 127)))
    if len(np.unique(g)) < min(12, case.bs * case.c / 2):
        bad.append("%d distinct gates" % len(np.unique(g)))
    if not case.wide and np.mean((dst == 0) | (dst == 255)) > 0.20:
        bad.append("dst in {0, 255} on %.2f" % np.mean((dst == 0) | (dst == 255)))
    if np.mean(dst != src) < 0.5:
        bad.append("dst != src on %.2f only" % np.mean(dst != src))
    return bad


@functools.lru_cache(maxsize=None)
def generate(case):
    """-> (data, stages): the recipe of _draw on the first of the seeds case.seed, case.seed + 1, ... whose data keeps
    every condition (tiny cases -- one image of one pixel and one channel -- need a few draws).  Computed once per case and
    shared: treat both as read-only."""
    for k in range(200):
        data = _draw(case, case.seed + k)
        st = stages(case, data)
        if not conditions(case, data, st):
            for v in list(data.values()) + list(st.values()):
                if v is not None:
                    v.setflags(write=False)
            return data, st
    raise AssertionError("no seed keeps the conditions for " + case.ident())


def scalar_stages(case, data):
    """the formula as plain loops over Python ints and np.float32 scalars (small cases only)"""
    f32 = np.float32
    src, w1, w2, lut = data["src"], data["w1"], data["w2"], data["lut"]

    def cvt(f):
        if not (f >= f32(-2147483648.0) and f < f32(2147483648.0)):
            return -2 ** 31
        return int(np.floor(f)) if case.rm else int(np.rint(f))

    def rq(acc, bias, scale, relu):
        f = f32(acc)
        f = f32(f + (f32(0.0) if bias is None else f32(bias)))
        f = f32(f * f32(scale))
        return f32(0.0) if relu and f32(0.0) > f else f

    def sat_u8(v):
        return 255 if v < 0 or v > 255 else v

    def pick(a, i):
        return a[0] if len(a) == 1 else a[i]

    z = np.zeros((case.bs, case.c), np.uint8)
    h = np.zeros((case.bs, case.cr), np.uint8)
    t = np.zeros((case.bs, case.c), np.int8)
    g = np.zeros((case.bs, case.c), np.uint8)
    dst = np.zeros_like(src)
    for n in range(case.bs):
        for ch in range(case.c):
            s = sum(int(src[n, y, x, ch]) for y in range(case.ih) for x in range(case.iw))
            z[n, ch] = min(255, max(0, int(np.rint(f32(f32(s) / f32(case.px))))))
        for j in range(case.cr):
            acc = sum(int(z[n, ch]) * int(w1[j, ch]) for ch in range(case.c))
            h[n, j] = sat_u8(cvt(rq(acc, None if data["bia1"] is None else data["bia1"][j], pick(data["scales1"], j), True)))
        for ch in range(case.c):
            acc = sum(int(h[n, j]) * int(w2[ch, j]) for j in range(case.cr))
            t[n, ch] = min(127, max(-128, cvt(rq(acc, None if data["bia2"] is None else data["bia2"][ch], pick(data["scales2"], ch), False))))
            g[n, ch] = lut[int(t[n, ch]) + 128]
            for y in range(case.ih):
                for x in range(case.iw):
                    dst[n, y, x, ch] = sat_u8(cvt(rq(int(src[n, y, x, ch]) * int(g[n, ch]), None, pick(data["out_scales"], ch), True)))
    return dict(z=z, h=h, t=t, g=g, dst=dst)


# --- the planner of csrc/se_plan.h, mirrored: the tests assert info().slices from it -----------------------------------
def planned_slices(case, cus, forced=None):
    groups = case.c // 16
    gchunks = -(-groups // min(groups, 256))
    if forced is not None:
        s = forced
    else:
        per = case.bs * gchunks
        s = min(-(-2 * cus // per), case.px // 64)
    return max(1, min(s, case.px))


# --- the table: every channel count with every image size, the squeezed widths, batch sizes and options rotating ------------
BAND_C = (16, 32, 48, 64, 96, 1152)
GENERIC_C = (1, 3, 17, 40, 72)
CRS = (1, 4, 5, 12, 48)
IMAGES = ((1, 1), (3, 3), (5, 9), (7, 7), (14, 14), (33, 17))
BATCHES = (1, 2, 3)
OPTIONS = [dict(), dict(bia1_dt=UNDEF, bia2_dt=F32), dict(per_channel=True), dict(bia1_dt=F32, bia2_dt=UNDEF, per_channel=True),
           dict(rm=1), dict(rm=1, per_channel=True, bia2_dt=UNDEF), dict(wide=True)]


def table():
    out, i = [], 0
    for c in BAND_C + GENERIC_C:
        for k, (ih, iw) in enumerate(IMAGES):
            out.append(SeCase("band" if c % 16 == 0 else "gen", BATCHES[i % 3], ih, iw, c, CRS[(i + k // 2) % 5], seed=4000 + 100 * i,
                              **OPTIONS[i % len(OPTIONS)]))
            i += 1
    return out


def small_table():
    """what a scalar loop walks in a moment"""
    return [c for c in table() if c.bs * c.px * c.c * max(1, c.cr // 4) <= 40000]


SLICE_CASE = SeCase("slices", 2, 33, 17, 32, 8, seed=5000)          # 561 pixels: 7 slices of 80 / 81, 561 of one
SLICE_VALUES = (1, 2, 3, 7, 561, 10 ** 6)
GRID_CASES = [SeCase("grid", 3, 14, 14, 48, 12, seed=5100), SeCase("grid", 2, 33, 17, 1152, 48, per_channel=True, seed=5200)]
GRID_VALUES = (1, 3)
FLUSH_PIXELS = (256, 257, 258, 561)


# --- rescale ties: sat_u8(cvt(src * gate * out_scale)) with out_scale = 2^-8 (the natural deployment value) and 2^-7 puts
#     every product src * gate that is an odd multiple of 2^(k-1) on a tie.  The table's out_scales (1 / 255, 1 / 100
#     and per-channel multiples) never do. ------------------------------------------------------------------------------
TIE_CASE = SeCase("ties", 3, 14, 14, 64, 12)
TIE_LOG2 = (8, 7)


def tie_data(k, rm):
    """-> (case, data, stages, counts): generate(TIE_CASE with round mode rm) with out_scales = 2^-k.  Refuses data
    whose products src * gate do not hold requant_edges' numbers of ties inside the u8 range (assert_enough_ties; the
    products are never negative)."""
    case = replace(TIE_CASE, rm=rm)
    data = dict(generate(case)[0], out_scales=np.array([2.0 ** -k], dtype=np.float32))
    st = stages(case, data)
    m = data["src"].astype(np.int64) * st["g"].astype(np.int64)[:, None, None, :]
    n = E.count_ties_of(m, k, U8, True)
    E.assert_enough_ties(n, (case.ident(), k))
    return case, data, st, n
