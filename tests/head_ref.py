"""CPU reference of the net head (dfx_head_* of include/dfx.h: channel top-k / argmax and softmax over a row matrix), an
independent witness of it, and the case table + seeded input generators the head tests share.

TOPK: the order is total (integers as themselves, f32 by IEEE totalOrder on the bit pattern); row r's results are its k
largest elements by (value descending, channel ascending).  The reference maps every element to a u32 key and sorts one
u64 per element with numpy; the witness is a pure-Python sort on (-key, channel) with a sign-magnitude key taken from the
raw bytes by struct, a different formula.
SOFTMAX: m = max, d = m - src, S = sum E[d] exact, p = float32(E[d]) / float32(S), u8: rint(p * out_scale) clamped.  The
reference is numpy float32 arithmetic; the witness uses Python ints for S and float32(float64 / float64) for the division
(the double rounding is harmless at 53 >= 2 * 24 + 2 bits)."""
import struct
from dataclasses import dataclass

import numpy as np

UNDEF, F32, S32, S8, U8 = 0, 1, 2, 3, 4
TOPK, SOFTMAX = 0, 1
PIXEL, ROW, GENERIC = 0, 1, 2
PATH_NAME = {PIXEL: "head_pixel", ROW: "head_row", GENERIC: "head_generic"}
NP_OF = {F32: np.float32, S32: np.int32, S8: np.int8, U8: np.uint8}
NAME_OF = {F32: "f32", S32: "s32", S8: "s8", U8: "u8"}
SIZE_OF = {F32: 4, S32: 4, S8: 1, U8: 1}
PIXEL_MAX_LD = 160           # csrc/head_plan.h
ROW_AUTO_MIN_BYTES = 160     # csrc/head_plan.h: auto takes the row kernel in its class from rows of this many bytes on
MAX_BLOCKS = 2048


@dataclass(frozen=True)
class HeadCase:
    name: str
    mode: int
    rows: int
    c: int
    ld: int                  # src_ld
    src_dt: int
    dst_dt: int              # TOPK: idx dtype (S32 | U8); SOFTMAX: F32 | U8
    k: int = 1
    dst_ld: int = 0          # SOFTMAX: 0 -> c
    out_scale: float = 255.0
    table: str = "exp"       # SOFTMAX: "exp" (softmax_table(0.0625, c)) | "bound" (c * max(E) = 2^32 - 1 exactly) | "onehot"
    plant: str = "mixed"     # generator: "mixed" | "special"
    seed: int = 5

    def ident(self):
        m = "softmax" if self.mode == SOFTMAX else "top%d" % self.k
        return "%s-%s-r%d-c%d-ld%d-%s-%s%s" % (self.name, m, self.rows, self.c, self.ld, NAME_OF[self.src_dt], NAME_OF[self.dst_dt],
                                              "-dld%d" % self.dst_ld if self.dst_ld else "")

    @property
    def out_ld(self):
        return self.k if self.mode == TOPK else (self.dst_ld or self.c)

    @property
    def out_cols(self):
        return self.k if self.mode == TOPK else self.c


# ---- the plan, mirrored from csrc/head_plan.h ---------------------------------------------------------------------------------
def in_class(case, path):
    if path == PIXEL:
        return SIZE_OF[case.src_dt] == 1 and (case.mode == SOFTMAX or case.k == 1) and case.ld % 16 == 0 and case.ld <= PIXEL_MAX_LD
    if path == ROW:
        return case.ld * SIZE_OF[case.src_dt] % 16 == 0
    return True


def paths(case):
    return [p for p in (PIXEL, ROW, GENERIC) if in_class(case, p)]


def auto_path(case):
    """the AUTO RULE of include/dfx.h (DFX_HEAD_AUTO_NOTE)"""
    long_row = in_class(case, ROW) and case.ld * SIZE_OF[case.src_dt] >= ROW_AUTO_MIN_BYTES
    if case.mode == SOFTMAX and long_row:
        return ROW
    if in_class(case, PIXEL):
        return PIXEL
    return ROW if long_row else GENERIC


def planned_grid(rows, path, cap=0):
    per = 4 if path == ROW else 256
    blocks = min((rows + per - 1) // per, MAX_BLOCKS)
    if cap > 0:
        blocks = min(blocks, cap)
    return max(blocks, 1)


def lds_bytes(case, path):
    return 1024 if case.mode == SOFTMAX and path != GENERIC else 0


def algorithmic_bytes(case):
    return case.rows * case.c * SIZE_OF[case.src_dt] + case.rows * case.out_cols * SIZE_OF[case.dst_dt]


def kernel_name(case, path):
    m = "softmax" if case.mode == SOFTMAX else "topk%d" % case.k
    return "%s<%s,%s->%s>" % (PATH_NAME[path], m, NAME_OF[case.src_dt], NAME_OF[case.dst_dt])


# ---- tables ---------------------------------------------------------------------------------------------------------------
def softmax_table(scale, c):
    """E[d] = floor(exp(-d * scale) * floor((2^32 - 1) / c)): the recipe of include/dfx.h (dfa.softmax_table)"""
    top = (2 ** 32 - 1) // int(c)
    return np.floor(np.exp(-np.arange(256, dtype=np.float64) * float(scale)) * top).astype(np.uint32)


def make_table(case):
    if case.table == "onehot":
        e = np.zeros(256, dtype=np.uint32)
        e[0] = (2 ** 32 - 1) // case.c
        return e
    if case.table == "bound":           # every entry at the largest admitted value: an all-equal row sums to c * max(E)
        assert (2 ** 32 - 1) % case.c == 0, "choose c so that the bound is met exactly"
        return np.full(256, (2 ** 32 - 1) // case.c, dtype=np.uint32)
    return softmax_table(0.0625, case.c)


# ---- TOPK -------------------------------------------------------------------------------------------------------------------
def key_u32(a):
    """monotone map of the elements of `a` onto uint32"""
    if a.dtype == np.uint8:
        return a.astype(np.uint32)
    if a.dtype == np.int8:
        return (a.astype(np.int32) + 128).astype(np.uint32)
    bits = np.ascontiguousarray(a).view(np.uint32)
    if a.dtype == np.int32:
        return bits ^ np.uint32(0x80000000)
    assert a.dtype == np.float32
    return np.where(bits >> 31 != 0, ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def reference_topk(src, c, k):
    """src: (rows, ld) array -> idx (rows, k) int64, val (rows, k) of src's dtype"""
    valid = np.ascontiguousarray(src[:, :c])
    pair = (key_u32(valid).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(c, dtype=np.uint64))[None, :]
    order = np.argsort(pair, axis=1, kind="stable")[:, ::-1][:, :k]
    return order.astype(np.int64), np.take_along_axis(valid, order, axis=1)


def _witness_key(raw, dt):
    if dt == U8:
        return struct.unpack("<B", raw)[0]
    if dt == S8:
        return struct.unpack("<b", raw)[0]
    if dt == S32:
        return struct.unpack("<i", raw)[0]
    bits = struct.unpack("<I", raw)[0]
    mag = bits & 0x7FFFFFFF
    return -mag - 1 if bits >> 31 else mag          # sign-magnitude: -0 -> -1 < +0 -> 0; -NaN lowest, +NaN highest


def witness_topk(src, c, k, dt):
    rows = src.shape[0]
    es = SIZE_OF[dt]
    idx = np.zeros((rows, k), dtype=np.int64)
    val = np.zeros((rows, k), dtype=NP_OF[dt])
    vbytes = val.view(np.uint8).reshape(rows, k, es)
    for r in range(rows):
        raw = np.ascontiguousarray(src[r, :c]).tobytes()
        order = sorted((-_witness_key(raw[j * es:(j + 1) * es], dt), j) for j in range(c))[:k]
        for t, (_, j) in enumerate(order):
            idx[r, t] = j
            vbytes[r, t, :] = np.frombuffer(raw[j * es:(j + 1) * es], dtype=np.uint8)
    return idx, val


# ---- SOFTMAX ------------------------------------------------------------------------------------------------------------------
def reference_softmax(src, c, table, dst_dt, out_scale):
    """src: (rows, ld) u8 / s8 -> (rows, c) float32 or uint8"""
    x = src[:, :c].astype(np.int64)
    d = x.max(axis=1, keepdims=True) - x
    e = table[d]
    s = e.sum(axis=1, dtype=np.uint64)
    assert int(s.max()) < 2 ** 32 and int(s.min()) > 0
    p = e.astype(np.float32) / s.astype(np.uint32).astype(np.float32)[:, None]
    assert p.dtype == np.float32
    if dst_dt == F32:
        return p
    v = p * np.float32(out_scale)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def witness_softmax(src, c, table, dst_dt, out_scale):
    rows = src.shape[0]
    out = np.zeros((rows, c), dtype=NP_OF[dst_dt])
    tab = [int(t) for t in table]
    for r in range(rows):
        x = [int(v) for v in src[r, :c]]
        m = max(x)
        e = [tab[m - v] for v in x]
        fs = float(np.float32(sum(e)))                         # one rounding of the exact integer sum
        for j in range(c):
            p = np.float32(float(np.float32(e[j])) / fs)       # f32(f64 / f64) of the two rounded operands
            if dst_dt == F32:
                out[r, j] = p
            else:
                v = float(np.float32(float(p) * float(np.float32(out_scale))))   # (a 24 x 24-bit product is exact in f64)
                out[r, j] = min(max(round(v), 0), 255)         # Python rounds ties to even
    return out


def reference(case, src):
    """-> (idx, val) for TOPK, dst for SOFTMAX, in the dtypes the op writes"""
    if case.mode == TOPK:
        idx, val = reference_topk(src, case.c, case.k)
        return idx.astype(NP_OF[case.dst_dt]), val
    return reference_softmax(src, case.c, make_table(case), case.dst_dt, case.out_scale)


def witness(case, src):
    if case.mode == TOPK:
        idx, val = witness_topk(src, case.c, case.k, case.src_dt)
        return idx.astype(NP_OF[case.dst_dt]), val
    return witness_softmax(src, case.c, make_table(case), case.dst_dt, case.out_scale)


# ---- generators ---------------------------------------------------------------------------------------------------------------
# valid channels stay below VALID_HI[dt]; the pad channels c .. ld-1 hold PAD[dt], LARGER than every valid value
VALID_LO = {U8: 0, S8: -128, S32: -(2 ** 30), F32: -1000.0}
VALID_HI = {U8: 200, S8: 90, S32: 2 ** 30, F32: 1000.0}
POS_NAN_MAX = 0x7FFFFFFF


def pad_value(dt):
    if dt == F32:
        return np.array([POS_NAN_MAX], dtype=np.uint32).view(np.float32)[0]
    return {U8: 255, S8: 127, S32: 2 ** 31 - 1}[dt]


def seam(dt):
    """the last channel of the first 16-byte group"""
    return 16 // SIZE_OF[dt] - 1


def generate(case):
    """(rows, ld) array of src_dt.  Row 0: the maximum at channel 0; row 1: at c-1; row 2: twice, on both sides of the first
    16-byte seam (if c reaches it); row 3: all equal; row 4: the maximum in the last 16-byte group and at channel 63 * 16 /
    elemsize if there is one (lane 63's first group); every other row: random with the row maximum planted twice."""
    rng = np.random.RandomState(case.seed + case.c * 7 + case.rows)
    dt, c, rows, ld = case.src_dt, case.c, case.rows, case.ld
    if dt == F32:
        a = (rng.randint(-4000, 4000, size=(rows, ld)) * 0.25).astype(np.float32)
        a[rng.rand(rows, ld) < 0.02] = np.float32(-0.0)
        a[rng.rand(rows, ld) < 0.02] = np.float32(0.0)
        a[rng.rand(rows, ld) < 0.02] = np.float32(1e-41)               # a denormal
    elif dt == S32:
        a = rng.randint(-(2 ** 30), 2 ** 30, size=(rows, ld)).astype(np.int32)
        small = rng.rand(rows, ld) < 0.5
        a[small] = rng.randint(-3, 4, size=int(small.sum()))           # many duplicates
    else:
        a = rng.randint(VALID_LO[dt], VALID_HI[dt], size=(rows, ld)).astype(NP_OF[dt])
    top = NP_OF[dt](VALID_HI[dt])
    for r in range(rows):
        kind = r % 8
        if kind == 0:
            a[r, 0] = top
        elif kind == 1:
            a[r, c - 1] = top
        elif kind == 2 and c > seam(dt) + 1:
            a[r, seam(dt)] = a[r, seam(dt) + 1] = top
        elif kind == 3:
            a[r, :c] = a[r, 0]
        elif kind == 4:
            a[r, c - 1 - (c - 1) % (seam(dt) + 1)] = top               # first channel of the last group
            if c > 63 * (seam(dt) + 1):
                a[r, 63 * (seam(dt) + 1)] = top
        else:
            m = a[r, :c].max()
            if c >= 2:
                a[r, rng.choice(c, size=2, replace=False)] = m
    a[:, c:] = pad_value(dt)
    return a


def special_rows(dt, c, ld):
    """hand-planted rows (3 or more channels): extremes of the dtype, f32 +-NaN with payloads, +-0, +-Inf, denormals"""
    assert c >= 3
    if dt == F32:
        bits = [0x7FC00001, 0x7F800000, 0xFFC00123, 0xFF800000, 0x80000000, 0x00000000, 0x00000001, 0x80000001, 0x7F800001, 0x3F800000]
        rows = []
        for s in range(4):
            row = [bits[(j * 3 + s) % len(bits)] for j in range(c)]
            rows.append(row + [POS_NAN_MAX] * (ld - c))
        rows.append([0x80000000] * (c - 1) + [0x00000000] + [POS_NAN_MAX] * (ld - c))     # -0 ... -0 +0: +0 wins
        rows.append([0xFF800000, 0xFFC00000] + [0xFF800000] * (c - 2) + [POS_NAN_MAX] * (ld - c))   # -NaN loses to -Inf
        return np.array(rows, dtype=np.uint32).view(np.float32)
    lo, hi = {U8: (0, 255), S8: (-128, 127), S32: (-(2 ** 31), 2 ** 31 - 1)}[dt]
    rows = [[lo] * c, [hi] * c, [lo] * (c - 1) + [hi], [hi] + [lo] * (c - 1), [lo, hi] * (c // 2) + [lo] * (c % 2),
            [hi - 1] * (c - 2) + [hi, hi]]
    return np.array([r + [hi] * (ld - c) for r in rows], dtype=np.int64).astype(NP_OF[dt])


def make_src(case):
    if case.plant == "tie":
        return tie_src(case)
    if case.plant == "special":
        a = special_rows(case.src_dt, case.c, case.ld)
        assert a.shape == (case.rows, case.ld), (a.shape, case.ident())
        return a
    return generate(case)


# ---- the case table -------------------------------------------------------------------------------------------------------------
def _ld(c, dt):
    per = 16 // SIZE_OF[dt]
    return (c + per - 1) // per * per


def pixel_cases():
    out = []
    geo = [(21, 32), (19, 32), (16, 16), (1, 16), (33, 48), (64, 64), (150, 160), (161, 176)]   # 160: the largest src_ld in
    for c, ld in geo:                                                                          # the class; 176: outside
        for rows in (2 * 5 * 7, 64 * 3 + 1):                   # the whole product: every geometry with every variant
            for src_dt in (U8, S8):
                for idx_dt in (U8, S32):
                    out.append(HeadCase("px", TOPK, rows, c, ld, src_dt, idx_dt))
                for dst_dt in (F32, U8):
                    for dst_ld in (0, ld):
                        out.append(HeadCase("px", SOFTMAX, rows, c, ld, src_dt, dst_dt, dst_ld=dst_ld))
    return out


def row_cases():
    out = []
    dts, n = (S8, F32, U8, S32), 0
    for c in (1, 7, 15, 16, 17, 1000, 1023, 1024, 1025, 4097):
        for bs in (1, 3, 130):
            ks = sorted({1, min(5, c), min(8, c)}) + ([c] if c <= 8 else [])
            for k in sorted(set(ks)):
                n += 1
                dt = dts[n % 4]
                out.append(HeadCase("row", TOPK, bs, c, _ld(c, dt), dt, U8 if (c <= 256 and n % 2) else S32, k=k))
    for dt in dts:                                   # the classifier: every dtype with every k
        for k in (1, 5, 8):
            out.append(HeadCase("cls", TOPK, 3, 1000, 1008 if SIZE_OF[dt] == 1 else 1000, dt, S32, k=k))
    for c in (1, 15, 16, 17, 1000, 1023, 1024, 1025, 4097):
        for bs, dst_dt in ((1, F32), (3, U8), (130, F32)):
            out.append(HeadCase("row", SOFTMAX, bs, c, _ld(c, S8), S8 if bs != 3 else U8, dst_dt, dst_ld=0 if bs != 130 else _ld(c, S8)))
    out.append(HeadCase("cls", SOFTMAX, 3, 1000, 1008, S8, U8))
    out.append(HeadCase("bound", SOFTMAX, 3, 65535, 65536, U8, F32, table="bound"))      # 65535 * 65537 = 2^32 - 1
    out.append(HeadCase("bound", SOFTMAX, 1, 65535, 65536, S8, U8, table="exp"))
    return out


def generic_cases():
    return [HeadCase("odd", TOPK, 70, 21, 21, U8, U8), HeadCase("odd", TOPK, 70, 21, 21, S8, S32, k=5),
            HeadCase("odd", SOFTMAX, 70, 21, 21, U8, U8), HeadCase("odd", SOFTMAX, 70, 21, 21, S8, F32, dst_ld=23),
            HeadCase("odd", TOPK, 3, 1000, 1001, S8, S32, k=8), HeadCase("odd", SOFTMAX, 3, 1000, 1001, S8, F32),
            HeadCase("odd", TOPK, 5, 7, 7, F32, U8, k=7), HeadCase("odd", TOPK, 5, 9, 11, S32, S32, k=8)]


def special_cases():
    out = []
    for dt in (F32, S32, U8, S8):
        for c, ld in ((3, 16 // SIZE_OF[dt]), (20, 32), (67, 80)):
            for k in (1, 3):
                out.append(HeadCase("special", TOPK, 6, c, ld, dt, S32 if k == 3 else U8, k=k, plant="special"))
    return out


# two maxima under the one-hot table: p = 0.5 at both; u8 128 at out_scale 255 (127.5 ties to even), 0 at out_scale 1
def tie_case(out_scale, dst_dt=U8, rows=5):
    return HeadCase("tie", SOFTMAX, rows, 21, 32, U8, dst_dt, out_scale=out_scale, table="onehot", plant="tie")


def tie_src(case):
    a = np.full((case.rows, case.ld), 255, dtype=np.uint8)
    a[:, :case.c] = 7
    for r in range(case.rows):
        a[r, r % case.c] = 100
        a[r, (r + 16) % case.c] = 100      # (16 apart: on both sides of a 16-byte seam for most rows)
    return a


def table():
    return pixel_cases() + row_cases() + generic_cases() + special_cases()
