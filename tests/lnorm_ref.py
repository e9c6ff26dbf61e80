"""The arithmetic of the int8 layer norm / RMS norm (dfx_lnorm_*, include/dfx.h) restated in numpy -- int64 statistics, then
one np.float32 operation per step -- plus an independent pure-Python witness that rounds every step from exact rationals,
the plan the library must report (path, lanes, grid, LDS, bytes, kernel name) and the case generators of the tests."""
import collections
import fractions
import math

import numpy as np

F32, S32, S8, U8 = 1, 2, 3, 4                      # include/dfx.h
NP_OF = {F32: np.float32, S8: np.int8, U8: np.uint8}
SIZE_OF = {F32: 4, S8: 1, U8: 1}
NAME_OF = {F32: "f32", S8: "s8", U8: "u8"}
LAYER, RMS = 0, 1
ROW, GENERIC = 0, 1
MAX_C, MAX_SHIFT = 16384, 7
THREADS, MAX_BLOCKS, LDS_MAX = 256, 2048, 64 * 1024

_Case = collections.namedtuple("LnCase", "name rows c src_ld dst_ld src_dt dst_dt mode shift eps dst_off seed kind")


class LnCase(_Case):
    """kind: how make_src / make_params fill the case ("random" unless a test plants something)"""

    def __new__(cls, name, rows, c, src_dt=S8, dst_dt=S8, mode=LAYER, shift=False, src_ld=None, dst_ld=None, eps=2.0 ** -10,
                dst_off=0, seed=0, kind="random"):
        return _Case.__new__(cls, name, rows, c, c if src_ld is None else src_ld, c if dst_ld is None else dst_ld, src_dt, dst_dt,
                             mode, shift, eps, dst_off, seed, kind)

    def ident(self):
        return "%s-%dx%d-ld%d.%d-%s%s-%s%s%s" % (self.name, self.rows, self.c, self.src_ld, self.dst_ld, NAME_OF[self.src_dt],
                                                 NAME_OF[self.dst_dt], "rms" if self.mode == RMS else "ln", "-sh" if self.shift else "",
                                                 "-o%d" % self.dst_off if self.dst_off else "")


def up16(n):
    return (n + 15) // 16 * 16


# ---- the reference ---------------------------------------------------------------------------------------------------------
def statistics(src, c, shift):
    """-> (t, S, Q) as int64, with the bounds of include/dfx.h asserted"""
    t = src[:, :c].astype(np.int64)
    if shift is not None:
        sh = np.asarray(shift, dtype=np.int64).reshape(-1)
        assert sh.shape == (c,) and sh.min() >= 0 and sh.max() <= MAX_SHIFT
        t = t << sh
    S, Q = t.sum(axis=1), (t * t).sum(axis=1)
    assert np.abs(t).max() <= 32640 and np.abs(S).max() < 2 ** 30 and Q.max() < 2 ** 44
    return t, S, Q


def row_factor(S, Q, c, eps, mode):
    """-> (a, D): the row's f32 factor and (LAYER) the exact c^2 x variance"""
    eps = np.float32(eps)
    fc = np.float32(c)
    one = np.float32(1.0)
    if mode == LAYER:
        D = c * Q - S * S
        assert D.min() >= 0 and D.max() < 2 ** 58
        v = D.astype(np.float32) / np.int64(c * c).astype(np.float32)
        return (one / np.sqrt(v + eps)) / fc, D
    v = Q.astype(np.float32) / fc
    return one / np.sqrt(v + eps), None


def convert(y, dst_dt):
    """the reorder's conversion: rint to even, NaN -> 0, clamp"""
    if dst_dt == F32:
        return y
    lo, hi = (0, 255) if dst_dt == U8 else (-128, 127)
    with np.errstate(invalid="ignore"):
        r = np.rint(y)
    r = np.where(np.isnan(y), np.float32(0), r)
    return np.clip(r, lo, hi).astype(NP_OF[dst_dt])


def reference_values(src, c, gamma, beta, shift, eps, mode):
    """-> y {rows, c} float32, bit for bit what both kernels must compute"""
    t, S, Q = statistics(src, c, shift)
    a, _ = row_factor(S, Q, c, eps, mode)
    u = c * t - S[:, None] if mode == LAYER else t
    assert np.abs(u).max() < 2 ** 31
    g = np.asarray(gamma, dtype=np.float32).reshape(1, c)
    b = np.zeros((1, c), dtype=np.float32) if beta is None else np.asarray(beta, dtype=np.float32).reshape(1, c)
    with np.errstate(all="ignore"):
        y = u.astype(np.float32) * a[:, None].astype(np.float32)
        y = y * g
        y = y + b
    assert y.dtype == np.float32
    return y


def reference(case, src, params):
    gamma, beta, shift = params
    return convert(reference_values(src, case.c, gamma, beta, shift, case.eps, case.mode), case.dst_dt)


# ---- the witness: every step rounded from exact rationals ---------------------------------------------------------------------
def _round_f32(x):
    """Fraction -> Fraction: the nearest binary32 (ties to even, denormals, overflow to +-inf as float('inf'))"""
    if x == 0:
        return fractions.Fraction(0)
    sign = -1 if x < 0 else 1
    x = abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()       # 2^(e-1) <= x < 2^(e+1)
    if x < fractions.Fraction(2) ** e:
        e -= 1                                                      # 2^e <= x < 2^(e+1)
    e = max(e, -126)
    ulp = fractions.Fraction(2) ** (e - 23)
    q = x / ulp
    n = q.numerator // q.denominator
    rem = q - n
    if rem > fractions.Fraction(1, 2) or (rem == fractions.Fraction(1, 2) and n % 2 == 1):
        n += 1
    r = n * ulp
    if r >= fractions.Fraction(2) ** 128:
        return sign * math.inf
    return sign * r


def _sqrt_f32(x):
    """correctly rounded square root of a non-negative Fraction that is a binary32"""
    if x == 0:
        return fractions.Fraction(0)
    p, q = x.numerator, x.denominator
    s = 200                                                          # sqrt(p / q) = sqrt(p * q * 4^s) / (q * 2^s)
    n = math.isqrt(p * q << (2 * s))
    exact = n * n == p * q << (2 * s)
    # an inexact root lies strictly between n and n + 1 at this scale; no binary32 and no midpoint of two lies in between
    return _round_f32(fractions.Fraction(n, q << s) if exact else fractions.Fraction(2 * n + 1, q << (s + 1)))


def _frac(v):
    return fractions.Fraction(float(np.float32(v)))


def witness_row(x, gamma, beta, shift, eps, mode, only=None):
    """one row of integers -> list of binary32 values as Python floats (of the channels `only`, when given); finite gamma /
    beta only"""
    c = len(x)
    t = [int(v) << (int(shift[k]) if shift is not None else 0) for k, v in enumerate(x)]
    S, Q = sum(t), sum(v * v for v in t)
    eps = _frac(eps)
    one = fractions.Fraction(1)
    if mode == LAYER:
        D = c * Q - S * S
        v = _round_f32(_round_f32(fractions.Fraction(D)) / _round_f32(fractions.Fraction(c * c)))
        a = _round_f32(_round_f32(one / _sqrt_f32(_round_f32(v + eps))) / c)
        u = [c * v_ - S for v_ in t]
    else:
        v = _round_f32(_round_f32(fractions.Fraction(Q)) / c)
        a = _round_f32(one / _sqrt_f32(_round_f32(v + eps)))
        u = t
    out = []
    for k in (range(c) if only is None else only):
        y = _round_f32(_round_f32(fractions.Fraction(u[k])) * a)
        y = _round_f32(y * _frac(gamma[k]))
        y = _round_f32(y + (_frac(beta[k]) if beta is not None else 0))
        out.append(float(y))
    return out


# ---- float64 layer norm (for the derived tolerance) ---------------------------------------------------------------------------
def float64_norm(src, c, gamma, beta, shift, eps, mode):
    """-> (y64, bound_term): the layer norm in float64 and |xhat * gamma| + |beta| per element"""
    t = src[:, :c].astype(np.float64)
    if shift is not None:
        t = t * (2.0 ** np.asarray(shift, dtype=np.float64)).reshape(1, c)
    eps = float(np.float32(eps))
    if mode == LAYER:
        mu = t.mean(axis=1, keepdims=True)
        xhat = (t - mu) / np.sqrt(((t - mu) ** 2).mean(axis=1, keepdims=True) + eps)
    else:
        xhat = t / np.sqrt((t * t).mean(axis=1, keepdims=True) + eps)
    g = np.asarray(gamma, dtype=np.float64).reshape(1, c)
    b = np.zeros((1, c)) if beta is None else np.asarray(beta, dtype=np.float64).reshape(1, c)
    return xhat * g + b, np.abs(xhat * g) + np.abs(b)


# ---- the plan the library must report ------------------------------------------------------------------------------------------
def lanes(c):
    groups, w = (c + 15) // 16, 4
    while w < groups and w < 64:
        w *= 2
    return w


def in_class(case, path):
    if path == GENERIC:
        return True
    return case.src_ld % 16 == 0 and (case.dst_ld * SIZE_OF[case.dst_dt]) % 16 == 0


def auto_path(case):
    """the AUTO RULE of include/dfx.h (DFX_LNORM_AUTO_NOTE): the row kernel is unmeasured, nothing takes it on auto"""
    return GENERIC


def planned_grid(case, path, cap=0):
    per = THREADS // lanes(case.c) if path == ROW else THREADS
    blocks = min((case.rows + per - 1) // per, MAX_BLOCKS)
    if cap > 0:
        blocks = min(blocks, cap)
    return max(blocks, 1)


def lds_bytes(case, path):
    b = 8 * up16(case.c)
    return b if path == ROW and b <= LDS_MAX else 0


def algorithmic_bytes(case):
    return case.rows * case.c * (1 + SIZE_OF[case.dst_dt]) + case.c * (9 if case.shift else 8)


def kernel_name(case, path):
    s = "lnorm_row<" if path == ROW else "lnorm_generic<"
    s += ("rms," if case.mode == RMS else "layer,") + NAME_OF[case.src_dt] + "->" + NAME_OF[case.dst_dt]
    if path == ROW:
        s += ",w%d" % lanes(case.c)
    return s + (",shift>" if case.shift else ">")


# ---- generators ----------------------------------------------------------------------------------------------------------------
def _rng(case):
    return np.random.RandomState((case.seed * 1000003 + case.rows * 7919 + case.c * 31 + case.src_dt * 5 + case.mode) % (2 ** 31))


def make_src(case):
    """{rows, src_ld} of the src dtype; pad channels hold 0xFF"""
    rng = _rng(case)
    dt = NP_OF[case.src_dt]
    lo, hi = (0, 256) if case.src_dt == U8 else (-128, 128)
    src = np.full((case.rows, case.src_ld), 0xFF, dtype=np.uint8).view(dt)
    body = rng.randint(lo, hi, size=(case.rows, case.c))
    if case.rows > 1:
        body[1] = body[1, 0]                                          # a constant row: y = beta
    if case.rows > 2:
        body[2] = rng.randint(-3, 4, size=case.c) + (100 if case.src_dt == U8 else 0)   # a narrow row
    src[:, :case.c] = body.astype(dt)
    return src


def make_params(case):
    """-> (gamma, beta, shift or None); scaled so that a 1-byte dst uses its whole range and saturates now and then"""
    rng = _rng(case)
    rng.randint(0, 2, size=7)
    span = 1.0 if case.dst_dt == F32 else 40.0
    gamma = (rng.standard_normal(case.c) * span).astype(np.float32)
    beta = (rng.standard_normal(case.c) * span * 0.5 + (100.0 if case.dst_dt == U8 else 0.0)).astype(np.float32)
    shift = rng.randint(0, MAX_SHIFT + 1, size=case.c).astype(np.uint8) if case.shift else None
    return gamma, beta, shift


C_AXIS = (1, 15, 16, 17, 63, 64, 65, 96, 100, 768, 1000, 1024, 1025, 4096, 4097)
ROWS_AXIS = (1, 3, 4, 5, 63, 257)
W_EDGES = (128, 129, 256, 257, 512, 513)


def grid_cases():
    """every c meets at least two row counts and every row count at least two c; dtypes, mode, shifts, ld > c and the dst
    offset rotate across the grid"""
    out = []
    dts = [(S8, S8), (U8, U8), (S8, F32), (U8, S8), (S8, U8), (U8, F32)]
    n = 0
    for i, c in enumerate(C_AXIS):
        for j in range(3):
            rows = ROWS_AXIS[(i + 2 * j) % len(ROWS_AXIS)]
            if c >= 4096 and rows > 63:
                rows = 5
            sdt, ddt = dts[n % len(dts)]
            pad = (n // 2) % 3                                        # 0: ld = c; 1: the next multiple of 16; 2: 16 more, dst ld odd
            src_ld = c if pad == 0 else up16(c) + (16 if pad == 2 else 0)
            dst_ld = c if pad == 0 else up16(c) if pad == 1 else c + 3
            out.append(LnCase("grid", rows, c, sdt, ddt, mode=(n // 3) % 2, shift=n % 2 == 1, src_ld=src_ld, dst_ld=dst_ld,
                              dst_off=(0, 0, 0, 4 if ddt == F32 else 1)[n % 4], seed=n))
            n += 1
    # every c also in the row class (ld multiples of 16), so that the row kernel meets every W and the masked last group
    # ... and both sides of the switches of W the axis does not reach (128 / 256 / 512 bytes)
    for i, c in enumerate(C_AXIS + W_EDGES):
        sdt, ddt = dts[(i + 1) % len(dts)]
        rows = ROWS_AXIS[(i + 1) % len(ROWS_AXIS)]
        if c >= 4096 and rows > 63:
            rows = 4
        out.append(LnCase("rowc", rows, c, sdt, ddt, mode=i % 2, shift=i % 3 == 0, src_ld=up16(c), dst_ld=up16(c) + (16 if i % 2 else 0),
                          seed=100 + i))
    return out


def auto_cases():
    """cases on both sides of every bound of the auto rule: inside and outside the row class, short and long rows, few and many
    rows"""
    return [LnCase("auto", 9, 768), LnCase("auto", 9, 768, src_ld=769), LnCase("auto", 300, 96, U8, F32, mode=RMS),
            LnCase("auto", 5, 4096, shift=True), LnCase("auto", 3, 100, src_ld=112, dst_ld=100), LnCase("auto", 3, 100, src_ld=112, dst_ld=112),
            LnCase("auto", 70, 16, S8, U8), LnCase("auto", 2, 16384, S8, F32)]
