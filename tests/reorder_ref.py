"""CPU reference of the activation reorder (dfx_reorder_* of include/dfx.h), an independent witness of it, and
the case table + seeded input generator the reorder tests share.

Semantics (MKL-DNN's saturating reorder; the reference project ships no reorder, parity is unpinned): over a
logical {bs, c, h, w} tensor, for every destination channel k < dst_c
    k >= src_c:  0
    else         v = float32(src[n,k,y,x])      u8 / s8 exact, s32 round-to-nearest-even, f32 as is
                 v = v * scale[k]               one f32 multiply (no scales: 1.0f; one: scale[0])
                 f32 dst: v;  u8 / s8 dst: rint(v) (ties to even) or floor(v), NaN -> 0, clamp to the range
Source channels >= dst_c are dropped."""
from dataclasses import dataclass
from typing import Tuple

import numpy as np

UNDEF, F32, S32, S8, U8 = 0, 1, 2, 3, 4
NHWC, NCHW = 0, 1
NEAREST, DOWN = 0, 1
NP_OF = {F32: np.float32, S32: np.int32, S8: np.int8, U8: np.uint8}
NAME_OF = {F32: "f32", S32: "s32", S8: "s8", U8: "u8"}
FMT_NAME = {NHWC: "nhwc", NCHW: "nchw"}
RANGE = {U8: (0, 255), S8: (-128, 127)}


@dataclass(frozen=True)
class ReorderCase:
    shape: Tuple[int, int, int, int]   # logical (bs, src_c, h, w)
    dst_c: int
    src_fmt: int
    dst_fmt: int
    src_dt: int
    dst_dt: int
    scale_mode: str = "none"           # none | one | per
    rm: int = NEAREST
    seed: int = 7

    def ident(self):
        bs, c, h, w = self.shape
        return "%dx%dx%dx%d->%d-%s-%s-%s-%s-%s-rm%d" % (bs, c, h, w, self.dst_c, FMT_NAME[self.src_fmt], FMT_NAME[self.dst_fmt],
                                                      NAME_OF[self.src_dt], NAME_OF[self.dst_dt], self.scale_mode, self.rm)

    @property
    def src_shape(self):
        bs, c, h, w = self.shape
        return (bs, h, w, c) if self.src_fmt == NHWC else (bs, c, h, w)

    @property
    def dst_shape(self):
        bs, _, h, w = self.shape
        return (bs, h, w, self.dst_c) if self.dst_fmt == NHWC else (bs, self.dst_c, h, w)


def make_scales(case):
    """None, one scale (a power of two, so that planted ties stay ties) or one per source channel."""
    c = case.shape[1]
    if case.scale_mode == "none":
        return None
    if case.scale_mode == "one":
        return np.array([0.5], dtype=np.float32)
    return (np.float32(0.37) + np.arange(c, dtype=np.float32) * np.float32(1.3 / max(c, 1))).astype(np.float32)


# planted into f32 inputs (and their doubles, which the scale 0.5 turns back into these)
_F32_SPECIAL = [0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 254.5, 255.5, 126.5, 127.5, -127.5, -128.5,      # exact ties
                0.0, -0.0, np.inf, -np.inf,
                254.49, 255.49, 255.51, 256.0, -0.49, -0.51, -1.0, 127.49, 127.51, 128.0, -128.49, -128.51, -129.0,
                1e-40, -1e-40, 1.4e-45, 1.1754942e-38,                                              # denormals
                1e10, -1e10, 3.0e38, -3.0e38, 2147483648.0, -2147483904.0, 16777217.0]
_S32_SPECIAL = [2**31 - 1, -2**31, 2**31 - 65, 2**24 + 1, 2**24 + 3, -(2**24 + 1), 2**30 + 65, 123456789, -987654321,
                0, 1, -1, 255, 256, 509, 511, 513, -255, -257]


def generate(case):
    """seeded source tensor in its physical layout, special values planted at seeded positions"""
    rng = np.random.default_rng(case.seed + 1000003 * case.src_dt + 17 * case.dst_dt + sum(case.shape))
    n = int(np.prod(case.src_shape))
    if case.src_dt == U8:
        flat = rng.integers(0, 256, n).astype(np.uint8)
    elif case.src_dt == S8:
        flat = rng.integers(-128, 128, n).astype(np.int8)
    elif case.src_dt == S32:
        flat = rng.integers(-700, 701, n).astype(np.int32)
        special = np.array(_S32_SPECIAL, dtype=np.int64).astype(np.int32)
        pos = rng.permutation(n)[:len(special)]
        flat[pos] = special[:len(pos)]
    else:
        flat = rng.uniform(-300.0, 600.0, n).astype(np.float32)
        half = rng.integers(-600, 1200, n // 4 + 1).astype(np.float32) / np.float32(2.0)    # many exact .5 / .0 values
        flat[rng.permutation(n)[:len(half)]] = half[:min(len(half), n)]
        sp = list(_F32_SPECIAL) + [2.0 * v for v in _F32_SPECIAL if np.isfinite(v) and abs(v) < 1e38]
        if case.dst_dt != F32:
            sp.append(np.nan)           # NaN goes to integer destinations only: f32 results stay bit-comparable
        special = np.array(sp, dtype=np.float32)
        pos = rng.permutation(n)[:len(special)]
        flat[pos] = special[:len(pos)]
    return flat.reshape(case.src_shape)


def _scale_vector(case, scales):
    c = case.shape[1]
    if scales is None:
        return np.ones(c, dtype=np.float32)
    s = np.asarray(scales, dtype=np.float32).reshape(-1)
    assert s.size in (1, c), s.size
    return np.broadcast_to(s, (c,)).astype(np.float32) if s.size == 1 else s


def reference(src, case, scales):
    """numpy f32 formulation"""
    c = case.shape[1]
    x = src if case.src_fmt == NCHW else np.transpose(src, (0, 3, 1, 2))          # logical nchw
    with np.errstate(all="ignore"):
        v = x.astype(np.float32) * _scale_vector(case, scales).reshape(1, c, 1, 1)
        assert v.dtype == np.float32
        if case.dst_dt != F32:
            r = np.floor(v) if case.rm == DOWN else np.rint(v)
            r = np.where(np.isnan(v), np.float32(0), r)
            lo, hi = RANGE[case.dst_dt]
            v = np.clip(r, lo, hi).astype(NP_OF[case.dst_dt])
    if case.dst_c > c:
        v = np.pad(v, ((0, 0), (0, case.dst_c - c), (0, 0), (0, 0)))
    else:
        v = v[:, :case.dst_c]
    if case.dst_fmt == NHWC:
        v = np.transpose(v, (0, 2, 3, 1))
    return np.ascontiguousarray(v)


def witness(src, case, scales):
    """independent formulation: the product in float64 rounded ONCE to f32 (the f64 product of two f32 values is
    exact), rounding to integer by floor + integer arithmetic on the remainder, layout by explicit index loops
    over channels into a zero-filled destination"""
    bs, c, h, w = case.shape
    sv = _scale_vector(case, scales).astype(np.float64)
    out = np.zeros(case.dst_shape, dtype=NP_OF[case.dst_dt])
    with np.errstate(all="ignore"):
        for k in range(min(c, case.dst_c)):
            plane = src[:, k, :, :] if case.src_fmt == NCHW else src[:, :, :, k]          # (bs, h, w)
            if case.src_dt == S32:
                f = plane.astype(np.int64).astype(np.float64).astype(np.float32)            # one RNE rounding
            else:
                f = plane.astype(np.float32)
            v = (f.astype(np.float64) * sv[k]).astype(np.float32)
            if case.dst_dt != F32:
                lo, hi = RANGE[case.dst_dt]
                d = v.astype(np.float64)
                finite = np.isfinite(d)
                dz = np.where(finite, d, 0.0)
                fl = np.floor(dz)
                if case.rm == DOWN:
                    r = fl
                else:
                    rem = dz - fl                                  # exact: |dz| < 2^128 has at most 24 significant bits
                    odd = np.mod(fl, 2.0) == 1.0
                    r = fl + ((rem > 0.5) | ((rem == 0.5) & odd))
                r = np.minimum(np.maximum(r, lo), hi)
                r = np.where(finite, r, np.where(np.isnan(d), 0.0, np.where(d > 0, hi, lo)))
                v = r.astype(np.int64).astype(NP_OF[case.dst_dt])
            if case.dst_fmt == NCHW:
                out[:, k, :, :] = v
            else:
                out[:, :, :, k] = v
    return out


LAYOUTS = [(NCHW, NHWC), (NHWC, NCHW), (NHWC, NHWC), (NCHW, NCHW)]
DTYPE_PAIRS = [(F32, U8), (F32, S8), (U8, F32), (S8, F32), (S32, F32), (F32, F32), (U8, U8), (S32, U8)]
SHAPES = [(1, 1, 1, 1), (2, 3, 7, 7), (3, 17, 13, 17), (2, 24, 5, 100), (4, 64, 56, 56), (2, 100, 9, 31),
          (1, 1024, 7, 7), (2, 256, 14, 14), (1, 3, 224, 224)]
# (shape, dst_c): channel padding 3->16, 3->4, 17->32; crop 64->48, 16->3
PAD_CROP = [((2, 3, 7, 7), 16), ((1, 3, 224, 224), 16), ((2, 3, 7, 7), 4), ((1, 3, 224, 224), 4), ((3, 17, 13, 17), 32),
            ((4, 64, 56, 56), 48), ((2, 16, 9, 31), 3)]
SCALE_MODES = ["none", "one", "per"]
ROUND_MODES = [NEAREST, DOWN]
_SMALL = 60000   # elements: below, every scale mode x round mode; above, one combination per case, cycling


def table(layouts=None, dtype_pairs=None):
    """the shared case table, optionally restricted to some layout / dtype pairs"""
    out = []
    combos = [(s, r) for s in SCALE_MODES for r in ROUND_MODES]
    for lay in (layouts or LAYOUTS):
        for dts in (dtype_pairs or DTYPE_PAIRS):
            for j, (shape, dst_c) in enumerate([(s, s[1]) for s in SHAPES] + PAD_CROP):
                if int(np.prod(shape)) <= _SMALL and dst_c == shape[1]:
                    todo = combos
                else:
                    todo = [combos[(LAYOUTS.index(lay) * 7 + DTYPE_PAIRS.index(dts) * 3 + j) % len(combos)]]
                for sm, rm in todo:
                    out.append(ReorderCase(shape, dst_c, lay[0], lay[1], dts[0], dts[1], sm, rm))
    return out
