"""CPU reference of the scaled element-wise sum (dfx_wsum_* of include/dfx.h), an independent witness of it, and the case
table + seeded input generator the wsum tests share.

For element (n,y,x,k) of n NHWC tensors of one shape, every f32 operation rounded separately (never an FMA):
    v = float32(src_0) * s_0[k]               u8 / s8 exact, s32 round-to-nearest-even, f32 as is
    v = v + float32(src_i) * s_i[k]           i = 1 .. n-1, left to right
    v = v + bias[k]                           only with a bias
    v = (0 > v) ? 0 : v                       only with ReLU: vmaxps(+0, v), so -0 stays -0 and NaN stays NaN
    f32 dst: v;  u8 / s8 dst: rint(v) (ties to even) or floor(v), NaN -> 0, clamp to the range (the reorder's conversion)
    table:  t = that conversion to lut_in;  dst byte = lut[t] (u8 index) or lut[t + 128] (s8 index)"""
from dataclasses import dataclass
from typing import Tuple

import numpy as np

UNDEF, F32, S32, S8, U8 = 0, 1, 2, 3, 4
NEAREST, DOWN = 0, 1
VEC, GENERIC = 0, 1
NP_OF = {F32: np.float32, S32: np.int32, S8: np.int8, U8: np.uint8}
NAME_OF = {F32: "f32", S32: "s32", S8: "s8", U8: "u8"}
RANGE = {U8: (0, 255), S8: (-128, 127)}
SIZE_OF = {F32: 4, S32: 4, S8: 1, U8: 1}
MAX_LDS = 64 * 1024
AUTO_MIN_ELEMS = 1 << 19     # csrc/wsum_plan.h: auto takes the vec kernel in its class from this many elements on


@dataclass(frozen=True)
class WsumCase:
    name: str
    shape: Tuple[int, int, int, int]     # (bs, h, w, c)
    src_dts: Tuple[int, ...]
    dst_dt: int
    per_channel: Tuple[bool, ...]        # per input: c scales instead of one
    bias: str = "0"                      # "0" | "1" | "c"
    relu: bool = False
    rm: int = NEAREST
    lut_in: int = UNDEF
    exact: bool = False                  # dyadic scales and bias: every product and sum of 1-byte inputs is exact, ties stay ties
    seed: int = 11

    def ident(self):
        return "%s-%s" % (self.name, "x".join(str(v) for v in self.shape))

    @property
    def n(self):
        return len(self.src_dts)

    @property
    def c(self):
        return self.shape[3]

    def nscales(self):
        return [self.c if (pc and self.c > 1) else 1 for pc in self.per_channel]

    def n_bias(self):
        return {"0": 0, "1": 1, "c": self.c}[self.bias]

    def image_bytes(self):
        """csrc/wsum_plan.h wsum_image(): the constants the vec kernel stages in LDS"""
        slots = sum(1 for ns in self.nscales() if ns == self.c and self.c > 1) + (1 if self.bias == "c" and self.c > 1 else 0)
        b = (slots * self.c * 4 + 15) // 16 * 16
        return b + (256 if self.lut_in != UNDEF else 0)

    @property
    def vec_class(self):
        return self.c % 16 == 0 and self.image_bytes() <= MAX_LDS


def auto_path(case):
    """csrc/wsum_plan.h wsum_path() with force_path = -1"""
    elems = case.shape[0] * case.shape[1] * case.shape[2] * case.shape[3]
    return VEC if case.vec_class and elems >= AUTO_MIN_ELEMS else GENERIC


def planned_grid(items, cap=0):
    """csrc/wsum_plan.h wsum_grid()"""
    blocks = min((items + 255) // 256, 2048)
    if cap > 0:
        blocks = min(blocks, cap)
    return max(1, blocks)


_DYADIC = [1.5, 0.5, -1.0, 0.25, -0.75, 0.5, 2.0, -1.25]
_F32_SPECIAL = [0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 254.5, 255.5, 126.5, 127.5, -127.5, -128.5, 0.0, -0.0,
                254.49, 255.51, 256.0, -0.49, -0.51, 127.49, 127.51, 128.0, -128.49, -128.51, -129.0,
                1e-40, -1e-40, 1.4e-45, 1.1754942e-38, 1e10, -1e10, 3.0e37, -3.0e37, 2147483648.0, 16777217.0]
_S32_SPECIAL = [2**31 - 1, -2**31, 2**31 - 65, 2**24 + 1, 2**24 + 3, -(2**24 + 1), 2**30 + 65, 123456789, -987654321,
                0, 1, -1, 255, 256, 509, 511, 513, -255, -257]


def make_params(case):
    """scales (one f32 array per input), bias (or None), lut (256 u8, or None)"""
    c = case.c
    scales = []
    for i, ns in enumerate(case.nscales()):
        if case.exact:
            base = np.float32(_DYADIC[i % len(_DYADIC)])
            s = base * np.where(np.arange(ns) % 3 == 2, np.float32(0.5), np.float32(1.0)).astype(np.float32)
        else:
            sign = np.float32(-1.0 if i % 3 == 1 else 1.0)
            s = sign * (np.float32(0.37) / np.float32(1 + i) + np.arange(ns, dtype=np.float32) * np.float32(0.9 / max(c, 1)))
            if case.src_dts[i] == S32:
                s = s * np.float32(0.25)
        scales.append(np.ascontiguousarray(s, dtype=np.float32).reshape(-1))
    nb = case.n_bias()
    bias = None
    if nb:
        k = np.arange(nb, dtype=np.float32)
        bias = ((k % 7) - np.float32(3.0)) * np.float32(0.5) if case.exact else (k % 5) * np.float32(1.7) - np.float32(2.9)
        bias = np.ascontiguousarray(bias, dtype=np.float32)
    lut = None
    if case.lut_in != UNDEF:
        lut = np.random.default_rng(case.seed + 77).permutation(256).astype(np.uint8)   # any index error shows
    return scales, bias, lut


def hswish_table(s_in, s_out):
    """lut[t + 128] = h-swish(t * s_in) / s_out as s8 bytes: the table a MobileNetV3 / EfficientNet-lite caller builds"""
    x = (np.arange(256) - 128) * float(s_in)
    y = x * np.clip(x + 3.0, 0.0, 6.0) / 6.0
    return np.clip(np.rint(y / float(s_out)), -128, 127).astype(np.int8).view(np.uint8)


def generate(case):
    """seeded inputs, special values planted at seeded positions.  Exact cases get many .5 ties by construction (1-byte
    values times dyadic scales); s32 inputs carry values beyond 2^24; f32 inputs carry ties, +-0, denormals, +-Inf (only
    the first f32 input when dst is f32, so that no Inf - Inf makes a NaN whose payload would be compared) and, for
    integer destinations only, NaN."""
    rng = np.random.default_rng(case.seed + 131 * sum(case.shape) + 7 * case.n + case.dst_dt)
    n = int(np.prod(case.shape))
    srcs, first_f32 = [], True
    for dt in case.src_dts:
        if dt == U8:
            flat = rng.integers(0, 256, n).astype(np.uint8)
        elif dt == S8:
            flat = rng.integers(-128, 128, n).astype(np.int8)
        elif dt == S32:
            flat = rng.integers(-700, 701, n).astype(np.int32)
            sp = np.array(_S32_SPECIAL, dtype=np.int64).astype(np.int32)
            pos = rng.permutation(n)[:len(sp)]
            flat[pos] = sp[:len(pos)]
        else:
            flat = rng.uniform(-300.0, 600.0, n).astype(np.float32)
            half = rng.integers(-600, 1200, n // 4 + 1).astype(np.float32) / np.float32(2.0)
            pos = rng.permutation(n)[:len(half)]
            flat[pos] = half[:len(pos)]
            sp = list(_F32_SPECIAL)
            if case.dst_dt != F32 or first_f32:
                sp += [np.inf, -np.inf]
            if case.dst_dt != F32:
                sp.append(np.nan)
            first_f32 = False
            sp = np.array(sp, dtype=np.float32)
            pos = rng.permutation(n)[:len(sp)]
            flat[pos] = sp[:len(pos)]
        srcs.append(flat.reshape(case.shape))
    return srcs


def _chan(v, c):
    v = np.asarray(v, dtype=np.float32).reshape(-1)
    assert v.size in (1, c), (v.size, c)
    return v.reshape(1, 1, 1, -1)


def convert(v, dt, rm):
    """the reorder's conversion of f32 values to u8 / s8"""
    r = np.floor(v) if rm == DOWN else np.rint(v)
    r = np.where(np.isnan(v), np.float32(0), r)
    lo, hi = RANGE[dt]
    return np.clip(r, lo, hi).astype(NP_OF[dt])


def reference_value(case, srcs, scales, bias):
    """the f32 value before the conversion: numpy f32 arrays, one multiply and one add per step"""
    c = case.c
    with np.errstate(all="ignore"):
        v = None
        for x, s in zip(srcs, scales):
            term = x.astype(np.float32) * _chan(s, c)
            assert term.dtype == np.float32
            v = term if v is None else v + term
        if bias is not None:
            v = v + _chan(bias, c)
        if case.relu:
            v = np.where(np.float32(0) > v, np.float32(0), v)
        assert v.dtype == np.float32
    return v


def finish(case, v, lut):
    with np.errstate(all="ignore"):
        if case.lut_in != UNDEF:
            t = convert(v, case.lut_in, case.rm).astype(np.int64)
            return np.ascontiguousarray(np.take(lut, t + (128 if case.lut_in == S8 else 0)).view(NP_OF[case.dst_dt]))
        if case.dst_dt == F32:
            return np.ascontiguousarray(v)
        return np.ascontiguousarray(convert(v, case.dst_dt, case.rm))


def reference(case, srcs, scales, bias, lut):
    return finish(case, reference_value(case, srcs, scales, bias), lut)


def _round_witness(v32, dt, rm):
    lo, hi = RANGE[dt]
    d = v32.astype(np.float64)
    finite = np.isfinite(d)
    dz = np.where(finite, d, 0.0)
    fl = np.floor(dz)
    if rm == DOWN:
        r = fl
    else:
        rem = dz - fl                                     # exact: an f32 value has at most 24 significant bits
        odd = np.mod(fl, 2.0) == 1.0
        r = fl + ((rem > 0.5) | ((rem == 0.5) & odd))
    r = np.minimum(np.maximum(r, lo), hi)
    r = np.where(finite, r, np.where(np.isnan(d), 0.0, np.where(d > 0, hi, lo)))
    return r.astype(np.int64)


def witness(case, srcs, scales, bias, lut):
    """independent formulation: every multiply and every add in float64, rounded ONCE to f32 (the f64 product of two f32
    values is exact; the f64 sum of two f32 values rounded to f32 is the correctly rounded f32 sum, 53 >= 2 * 24 + 2);
    rounding to integer by floor + remainder arithmetic; channel by channel with explicit scalar constants"""
    bs, h, w, c = case.shape
    out = np.zeros(case.shape, dtype=NP_OF[case.dst_dt])
    with np.errstate(all="ignore"):
        for k in range(c):
            v = None
            for x, s, dt in zip(srcs, scales, case.src_dts):
                plane = x[..., k]
                f = plane.astype(np.int64).astype(np.float64).astype(np.float32) if dt in (S32, S8, U8) else plane
                sk = np.float64(s[k if s.size > 1 else 0])
                term = (f.astype(np.float64) * sk).astype(np.float32)
                v = term if v is None else (v.astype(np.float64) + term.astype(np.float64)).astype(np.float32)
            if bias is not None:
                v = (v.astype(np.float64) + np.float64(bias[k if bias.size > 1 else 0])).astype(np.float32)
            if case.relu:
                neg = v < 0                               # (NaN and -0 compare false: they stay)
                v = np.where(neg, np.float32(0), v)
            if case.lut_in != UNDEF:
                t = _round_witness(v, case.lut_in, case.rm)
                o = np.array([lut[int(i) + (128 if case.lut_in == S8 else 0)] for i in t.reshape(-1)], dtype=np.uint8)
                out[..., k] = o.reshape(t.shape).view(NP_OF[case.dst_dt])
            elif case.dst_dt == F32:
                out[..., k] = v
            else:
                out[..., k] = _round_witness(v, case.dst_dt, case.rm).astype(NP_OF[case.dst_dt])
    return out


# ---- the case table ----------------------------------------------------------------------------------------------------------
# the smallest shapes at which the kernels can still go wrong: one element; one channel group and an odd pixel count; three
# groups; two generic-class channel counts; several grid-stride passes under DFX_WSUM_GRID=2 with a ragged last one; a
# tensor of more than one workgroup per pass with 16 groups per pixel
SHAPES = [(1, 1, 1, 1), (2, 5, 7, 16), (1, 3, 3, 48), (2, 4, 4, 72), (1, 5, 3, 17), (1, 33, 17, 256)]
GRID_SHAPE = (3, 9, 11, 32)      # run under DFX_WSUM_GRID=2
T, F = True, False
# name, src dtypes, dst, per-channel flags, bias, relu, round mode, table index, exact
CONFIGS = [
    ("u8x2", (U8, U8), U8, (F, F), "0", T, NEAREST, UNDEF, T),
    ("u8x2down", (U8, U8), S8, (F, F), "0", F, DOWN, UNDEF, T),
    ("s8x2", (S8, S8), S8, (F, F), "1", F, NEAREST, UNDEF, T),
    ("u8s8", (U8, S8), S8, (T, F), "c", F, DOWN, UNDEF, T),
    ("u8s32", (U8, S32), U8, (F, T), "0", T, NEAREST, UNDEF, F),
    ("mix4f", (F32, U8, S8, S32), F32, (T, F, T, F), "c", F, NEAREST, UNDEF, F),
    ("mix4u", (F32, U8, S8, S32), U8, (F, T, F, T), "1", T, DOWN, UNDEF, F),
    ("n1lut_s8", (S8,), U8, (F,), "0", F, NEAREST, S8, T),
    ("n1lut_u8", (U8,), S8, (T,), "c", T, DOWN, U8, F),
    ("n1f32", (F32,), F32, (T,), "1", T, NEAREST, UNDEF, F),
    ("n3u8", (U8, U8, U8), U8, (F, T, F), "0", F, NEAREST, UNDEF, T),
    ("n3f", (S8, S32, U8), F32, (F, F, F), "0", T, NEAREST, UNDEF, F),
    ("n8u8", (U8,) * 8, U8, (T,) * 8, "c", T, NEAREST, UNDEF, F),
    ("n8s8", (S8,) * 8, S8, (F,) * 8, "0", F, NEAREST, UNDEF, T),
    ("n8mix", (U8, S8, S32, F32) * 2, S8, (T, F) * 4, "1", F, NEAREST, S8, F),
    ("n2lut", (U8, S8), U8, (F, F), "0", T, NEAREST, U8, T),
    ("s32x2", (S32, S32), S8, (T, T), "c", F, DOWN, UNDEF, F),
]


def _case(cfg, shape):
    name, sdt, ddt, pc, bias, relu, rm, lut_in, exact = cfg
    return WsumCase(name, shape, sdt, ddt, pc, bias, relu, rm, lut_in, exact)


def table():
    return [_case(cfg, shape) for shape in SHAPES for cfg in CONFIGS]


def grid_cases():
    return [_case(cfg, GRID_SHAPE) for cfg in CONFIGS if cfg[0] in ("u8x2", "mix4f", "n8mix", "n1lut_u8", "u8s32")]


# the designated tie case: u8 * 1.0 + u8 * (-1.5) -> s8 lies in -382.5 .. 255: half of the sums are exact .5 ties, and the
# range saturates on both sides
TIE_CASE = WsumCase("ties", (2, 5, 7, 16), (U8, U8), S8, (F, F), "0", F, NEAREST, UNDEF, True)


def tie_params():
    return [np.array([1.0], np.float32), np.array([-1.5], np.float32)], None, None
