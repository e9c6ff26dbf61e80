"""Reference, data, plan mirror and case tables of the int8 token linear op's tests (dfx_linear_*, include/dfx.h; pure numpy,
needs no GPU).

The arithmetic is the fully-connected op's: one int64 matrix product of the valid columns of src with the {n, k} weights,
then refmath's _requant / _store, unchanged (fc_ref is built on the same two), then the optional byte table.
tests/test_linear_cpu.py pins this against an element-by-element witness and against fc_ref where the two ops coincide;
tests/test_gpu_linear.py compares the GPU against it, bit for bit, over dst's whole storage.
"""
import functools
from dataclasses import dataclass, replace

import numpy as np

from refmath import _requant, _store

UNDEF, F32, S32, S8, U8 = 0, 1, 2, 3, 4
NP_OF = {F32: np.float32, S32: np.int32, S8: np.int8, U8: np.uint8}
NAME_OF = {UNDEF: "none", F32: "f32", S32: "s32", S8: "s8", U8: "u8"}
SIZE_OF = {F32: 4, S32: 4, S8: 1, U8: 1}
TILE, GENERIC = 0, 1            # DFX_LINEAR_TILE / DFX_LINEAR_GENERIC
INVALID, UNSUPPORTED = 1, 2
KMAX = 65025
NMAX = 2 ** 31 - 128
MAX_ELEMS = 1 << 40
POISON = 0xCD                   # hipref.POISON_BYTE
# csrc/linear_plan.h
BN, KS, BMS, THREADS = 128, 64, (64, 128), 256
WBLOCK = BN * KS
TILE_GRID_PER_CU, GEN_GRID_PER_CU = 2, 16


def up(v, m):
    return -(-v // m) * m


@dataclass(frozen=True)
class LinCase:
    name: str
    rows: int
    k: int
    n: int
    src_dt: int = S8
    dst_dt: int = S8
    bia_dt: int = UNDEF
    relu: bool = False
    rm: int = 0
    per_channel: bool = False
    src_ld: int = None            # None: k rounded up to 16 (the tile kernel's class)
    dst_ld: int = None            # None: n
    lut_in: int = UNDEF
    scale: float = None           # None: centred (see make_scales)
    small: bool = False           # small-integer data (ties)
    saturating: bool = False      # built to saturate: exempt from the 10 % cap
    seed: int = 1

    @property
    def sld(self):
        return up(self.k, 16) if self.src_ld is None else self.src_ld

    @property
    def dld(self):
        return self.n if self.dst_ld is None else self.dst_ld

    @property
    def req_dt(self):
        """the type the requant produces: dst's, or the table's index type"""
        return self.lut_in if self.lut_in != UNDEF else self.dst_dt

    @property
    def does_relu(self):
        return self.relu or self.req_dt == U8

    @property
    def nscales(self):
        return self.n if self.per_channel else 1

    def ident(self):
        return "%s-r%d-k%d-n%d-%s-%s-b%s-r%d-m%d-pc%d-ld%d,%d-lut%s" % (
            self.name, self.rows, self.k, self.n, NAME_OF[self.src_dt], NAME_OF[self.dst_dt], NAME_OF[self.bia_dt], self.relu, self.rm,
            self.per_channel, self.sld, self.dld, NAME_OF[self.lut_in])


def src_storage(case):
    """bytes of src's storage: whole rows (the tile kernel reads a row up to k rounded up to 16, within its pitch)"""
    return case.rows * case.sld


def dst_storage(case):
    """elements of dst's storage: up to the last valid element"""
    return (case.rows - 1) * case.dld + case.n


def acc_sd(case):
    """the accumulator's standard deviation under generate()'s uniform data"""
    return (147.0 if case.src_dt == U8 else 74.0) * 74.0 * np.sqrt(case.k)


def make_scales(case):
    """scales that centre the output, chosen from k: a 1-byte requant type gets a standard deviation of about 40 (a value of
    127 is beyond three of them, so far less than 10 % saturate); a 4-byte dst gets a scale near 0.37, which no accumulator of
    k <= 65025 can take to 2^31"""
    if case.scale is not None:
        s = np.float32(case.scale)
    elif case.req_dt in (S32, F32):
        s = np.float32(0.37)
    else:
        s = np.float32(40.0 / acc_sd(case))
    if case.per_channel:
        return (s * (0.5 + np.arange(case.n) / case.n)).astype(np.float32)
    return np.array([s], dtype=np.float32)


def make_bias(case, rng):
    """n entries of the bias dtype, about a third of the accumulator's standard deviation wide where the dtype can hold it"""
    if case.bia_dt == UNDEF:
        return None
    amp = max(1.0, acc_sd(case) / 3.0)
    if case.bia_dt == F32:
        return (rng.standard_normal(case.n) * amp).astype(np.float32)
    if case.bia_dt == S32:
        return np.rint(rng.standard_normal(case.n) * amp).astype(np.int32)
    if case.bia_dt == S8:
        return rng.integers(-128, 128, case.n).astype(np.int8)
    return rng.integers(0, 256, case.n).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def generate(case):
    """_generate(case); where a ReLU leaves a case of a few outputs all zero, the next seed is drawn (no case is all zero)"""
    for attempt in range(16):
        out = _generate(case, case.seed + 7919 * attempt)
        if not case.does_relu or case.saturating or requant_values(case, out).any():
            break
    return out


def _generate(case, seed):
    """-> dict(src: flat storage bytes viewed as the src dtype, w {n, k} int8, bia, scales, lut).  Valid elements are uniform
    over the whole dtype (small: 0 .. 3 against -3 .. 3); every pad column of src holds 0xFF: pad columns that took part would
    show.  The table, where the case has one, is a random permutation of the 256 bytes: a wrong index cannot hide."""
    rng = np.random.default_rng(seed)
    raw = np.full((case.rows, case.sld), 0xFF, dtype=np.uint8)
    if case.small:
        raw[:, :case.k] = rng.integers(0, 4, (case.rows, case.k)).astype(np.uint8)
        w = rng.integers(-3, 4, (case.n, case.k)).astype(np.int8)
    else:
        raw[:, :case.k] = rng.integers(0, 256, (case.rows, case.k)).astype(np.uint8)
        w = rng.integers(-128, 128, (case.n, case.k)).astype(np.int8)
    if case.does_relu and case.src_dt == U8 and not case.small:
        # a u8 src against a weight row of negative sum leaves little but the ReLU's zeros in that column: the rows with an
        # even n are negated where their sum is not positive, so that no case is all zero
        wv = w.astype(np.int16)
        flip = wv.sum(axis=1, keepdims=True) <= 0
        flip[1::2] = False
        wv = np.where(flip, np.clip(-wv, -127, 127), wv)
        wv[:, 0] = np.where(flip[:, 0] & (wv.sum(axis=1) <= 0), 1, wv[:, 0])
        w = wv.astype(np.int8)
    out = dict(src=raw.reshape(-1).view(NP_OF[case.src_dt]), w=w, bia=make_bias(case, rng), scales=make_scales(case), lut=None)
    if case.lut_in != UNDEF:
        out["lut"] = rng.permutation(256).astype(np.uint8)
    return out


def valid_src(case, data):
    """{rows, k} of the src dtype"""
    return data["src"].reshape(case.rows, case.sld)[:, :case.k]


def accumulate(case, data):
    """exact int64 accumulators {rows, n}"""
    return valid_src(case, data).astype(np.int64) @ data["w"].astype(np.int64).T


def requant_values(case, data):
    """{rows, n} of the requant type: what the op stores without a table"""
    with np.errstate(invalid="ignore", over="ignore"):
        f = _requant(accumulate(case, data), data["bia"], data["scales"], case.does_relu)
        return _store(f, case.req_dt, case.rm)


def apply_table(case, t, lut):
    """lut[t] for a u8 index type, lut[t + 128] for s8 (dfx_wsum's convention), as dst's dtype, bytes verbatim"""
    idx = t.astype(np.int64) + (128 if case.lut_in == S8 else 0)
    return np.asarray(lut, dtype=np.uint8)[idx].view(NP_OF[case.dst_dt])


def values(case, data):
    """the valid elements of dst, {rows, n}"""
    t = requant_values(case, data)
    return t if case.lut_in == UNDEF else apply_table(case, t, data["lut"])


def reference(case, data):
    """dst's whole storage as bytes: POISON everywhere but the valid elements"""
    vals = values(case, data)
    out = np.full(dst_storage(case), POISON, dtype=np.uint8).repeat(SIZE_OF[case.dst_dt]).view(NP_OF[case.dst_dt])
    idx = np.arange(case.rows, dtype=np.int64).reshape(-1, 1) * case.dld + np.arange(case.n, dtype=np.int64).reshape(1, -1)
    out[idx.reshape(-1)] = vals.reshape(-1)
    return out.view(np.uint8)


def bias_f32(case, bia, o):
    """the bias as the library converts it (vcvtdq2ps behind a sign / zero extension)"""
    return np.float32(0) if bia is None else np.float32(bia[o]) if case.bia_dt == F32 else np.float32(int(bia[o]))


def witness(case, data):
    """the same storage, element by element on Python ints and np.float32 scalars"""
    src, w, scales, bia = data["src"], data["w"], data["scales"], data["bia"]
    out = np.full(dst_storage(case), POISON, dtype=np.uint8).repeat(SIZE_OF[case.dst_dt]).view(NP_OF[case.dst_dt])
    for m in range(case.rows):
        for o in range(case.n):
            acc = 0
            for c in range(case.k):
                acc += int(src[m * case.sld + c]) * int(w[o, c])
            with np.errstate(invalid="ignore", over="ignore"):
                f = np.float32(acc)
                if bia is not None:
                    f = np.float32(f + bias_f32(case, bia, o))
                f = np.float32(f * np.float32(scales[o if len(scales) > 1 else 0]))
            if case.does_relu and np.float32(0) > f:
                f = np.float32(0)
            if case.req_dt == F32:
                v = f
            else:
                if not (f >= np.float32(-2147483648.0) and f < np.float32(2147483648.0)):
                    v = -2147483648
                else:
                    v = int(np.floor(f)) if case.rm == 1 else int(np.rint(f))
                if case.req_dt == S8:
                    v = max(-128, min(127, v))
                elif case.req_dt == U8:
                    v = 255 if (v < 0 or v > 255) else v
            if case.lut_in != UNDEF:
                v = int(data["lut"][v + (128 if case.lut_in == S8 else 0)])
                v = v - 256 if (case.dst_dt == S8 and v > 127) else v
            out[m * case.dld + o] = v
    return out.view(np.uint8)


def saturated_fraction(case, vals):
    """share of the requant's outputs on a saturation bound of its conversion (u8: 255; s8: -128 / 127; s32: +-2^31; f32:
    none).  A ReLU's 0 is the op's own result, not a saturation: the CPU test asks separately that a case is not all zero."""
    if case.req_dt == F32:
        return 0.0
    lo, hi = {U8: (None, 255), S8: (-128, 127), S32: (-2 ** 31, 2 ** 31 - 1)}[case.req_dt]
    hit = vals == hi
    if lo is not None:
        hit = hit | (vals == lo)
    return float(hit.mean())


# --- the plan of linear_plan.h and the image of linear_pack.h, mirrored ---------------------------------------------------------
def desc_of(case, force_path=-1):
    """the dict of dfx_linear_desc's fields of a case"""
    return dict(rows=case.rows, k=case.k, n=case.n, src_dt=case.src_dt, dst_dt=case.dst_dt, bia_dt=case.bia_dt, relu=int(case.relu),
                round_mode=case.rm, nscales=case.nscales, lut_in_dt=case.lut_in, force_path=force_path, src_ld=case.sld, dst_ld=case.dld)


def tile_class(d):
    return d["src_ld"] % 16 == 0


def validate(d):
    """0, INVALID or UNSUPPORTED for a descriptor given as a dict of dfx_linear_desc's fields, in the header's order"""
    if d["rows"] < 1 or not 1 <= d["k"] <= KMAX or not 1 <= d["n"] <= NMAX:
        return INVALID
    if d["src_dt"] not in (U8, S8) or d["dst_dt"] not in NP_OF or (d["bia_dt"] != UNDEF and d["bia_dt"] not in NP_OF):
        return INVALID
    if d["round_mode"] not in (0, 1) or d["nscales"] not in (1, d["n"]) or d["lut_in_dt"] not in (UNDEF, U8, S8):
        return INVALID
    if d["lut_in_dt"] != UNDEF and d["dst_dt"] not in (U8, S8):
        return INVALID
    if d["force_path"] not in (-1, TILE, GENERIC) or d["src_ld"] < d["k"] or d["dst_ld"] < d["n"]:
        return INVALID
    if d["rows"] * max(d["src_ld"], d["dst_ld"]) > MAX_ELEMS:
        return INVALID
    if d["force_path"] == TILE and not tile_class(d):
        return UNSUPPORTED
    return 0


AUTO_MIN_ROWS, AUTO_MIN_N, AUTO_MIN_K, AUTO_MIN_TILES64, AUTO_MIN_MACS = 1576, 96, 96, 54, 1700 * 256 * 256


def auto_path(d):
    """the AUTO RULE of include/dfx.h (DFX_LINEAR_AUTO_NOTE): the tile kernel in its class from the smallest rows, n, k, tile
    count (of 64 x 128 tiles) and multiply-adds at which it was measured and beat the generic kernel and dfx_bmm; generic
    everywhere else"""
    if d["force_path"] != -1:
        return d["force_path"]
    big = d["rows"] >= AUTO_MIN_ROWS and d["n"] >= AUTO_MIN_N and d["k"] >= AUTO_MIN_K and -(-d["rows"] // 64) * -(-d["n"] // BN) >= AUTO_MIN_TILES64 and \
        d["rows"] * d["n"] * d["k"] >= AUTO_MIN_MACS
    return TILE if big and tile_class(d) else GENERIC


def nblocks(n):
    return -(-n // BN)


def nslabs(k):
    return -(-k // KS)


def tiles(d, bm):
    return -(-d["rows"] // bm) * nblocks(d["n"])


def planned_bm(d, cus, forced=0):
    if forced in BMS:
        return forced
    return 128 if tiles(d, 128) >= max(1, cus) else 64


def planned_grid(d, path, bm, cus, cap=0):
    blocks = tiles(d, bm) if path == TILE else -(-(d["rows"] * d["n"]) // THREADS)
    blocks = min(blocks, max(1, cus) * (TILE_GRID_PER_CU if path == TILE else GEN_GRID_PER_CU))
    if cap > 0:
        blocks = min(blocks, cap)
    return max(1, blocks)


def lds_bytes(path, bm):
    return 2 * (bm * KS + WBLOCK) + 3 * BN * 4 + 256 if path == TILE else 0


def image_offsets(n, k):
    """(off_comp, off_bias, off_scale, off_table, bytes) of the device image"""
    consts = nblocks(n) * BN * 4
    packed = nblocks(n) * nslabs(k) * WBLOCK
    return packed, packed + consts, packed + 2 * consts, packed + 3 * consts, packed + 3 * consts + 256


def pack_weights(w):
    """the weight section and the compensation of linear_pack.h from int8 {n, k}: (bytes, int32[nblocks * 128])"""
    n, k = w.shape
    nb, ns = nblocks(n), nslabs(k)
    full = np.zeros((nb * BN, ns * KS), dtype=np.int8)
    full[:n, :k] = w
    # [nb][f][r] x [ks][j][h][b] -> [nb][ks][f][j][h][r][b]
    img = full.reshape(nb, 4, 32, ns, 2, 2, 16).transpose(0, 3, 1, 4, 5, 2, 6)
    comp = np.zeros(nb * BN, dtype=np.int32)
    comp[:n] = 128 * w.astype(np.int64).sum(axis=1)
    return np.ascontiguousarray(img).reshape(-1).view(np.uint8), comp


def fast_ok(case, data):
    """the fast route's proof of linear_pack.h from the actual weights, bias and scales"""
    if case.rm != 0:
        return False
    w = data["w"].astype(np.int64)
    pos, neg = np.where(w > 0, w, 0).sum(axis=1), -np.where(w < 0, w, 0).sum(axis=1)
    bound = 255.0 * np.maximum(pos, neg) if case.src_dt == U8 else 128.0 * (pos + neg)
    for o in range(case.n):
        b = float(bias_f32(case, data["bia"], o))
        s = float(data["scales"][o if case.per_channel else 0])
        if not (np.isfinite(b) and np.isfinite(s)) or (float(bound[o]) + abs(b)) * abs(s) > 2.0 ** 30:
            return False
    return True


def kernel_name(case, path, bm, route):
    lut = " +lut" if case.lut_in != UNDEF else ""
    if path == TILE:
        return "linear_tile<%s,%s,bm%d> %s%s" % (NAME_OF[case.src_dt], NAME_OF[case.dst_dt], bm, "fast" if route else "exact", lut)
    return "linear_generic<%s,%s>%s" % (NAME_OF[case.src_dt], NAME_OF[case.dst_dt], lut)


def algorithmic_ops(d):
    return 2 * d["rows"] * d["n"] * d["k"]


def algorithmic_bytes(d):
    return d["rows"] * d["k"] + d["n"] * d["k"] + d["rows"] * d["n"] * SIZE_OF[d["dst_dt"]] + (4 * d["n"] if d["bia_dt"] != UNDEF else 0) + \
        4 * d["nscales"] + (256 if d["lut_in_dt"] != UNDEF else 0)


# --- case tables -------------------------------------------------------------------------------------------------------------------
def grid_axes(bm):
    """the tails of the issue's grid for tile height bm"""
    return ((1, bm - 1, bm, bm + 1, 2 * bm + 2), (1, 3, 4, BN - 1, BN, BN + 1, 2 * BN + 8), (1, 15, 16, 17, KS - 1, KS, KS + 1, 2 * KS + 8, 200))


def _dst_ld(n, which):
    """0: dense; 1: a multiple of 4 above n (vector stores wherever n allows); 2: odd and above n (element stores)"""
    return (n, up(n, 4) + 4, (n + 3) | 1)[which]


@functools.lru_cache(maxsize=None)
def shape_grid(bm, src_dt):
    """A pairwise cover of rows x n x k: every (rows, n), every (rows, k) and every (n, k) pair occurs, the third size
    rotating.  dst dtype, dst's pitch (vector / element stores), ReLU, round mode and per-channel scales follow the sum of
    the three indices, the bias dtype the case's number: every tail meets all four dst dtypes and both kinds of store
    (tests/test_linear_cpu.py asserts it)."""
    rs, ns, ks = grid_axes(bm)
    triples = [(i, j, (i + 2 * j) % 9) for i in range(5) for j in range(7)]
    triples += [(i, (i + kk) % 7, kk) for i in range(5) for kk in range(9)]
    triples += [((j + kk) % 5, j, kk) for j in range(7) for kk in range(9)]
    seen, out = set(), []
    for t in triples:
        if t in seen:
            continue
        seen.add(t)
        x = len(out)
        i, j, kk = t
        n = ns[j]
        out.append(LinCase("grid", rs[i], ks[kk], n, src_dt=src_dt, dst_dt=(S8, U8, S32, F32)[(i + j + kk) % 4], bia_dt=(UNDEF, S32, F32, S8, U8)[x % 5],
                           relu=bool((i + kk) % 2), rm=(j + kk) % 2, per_channel=bool((i + j) % 2), dst_ld=_dst_ld(n, (i + 2 * j + kk) % 3),
                           seed=1000 * bm + 100 * src_dt + x))
    return tuple(out)


def compensation_cases():
    """k = 200 and 65025: a u8 src row of all 255 and one of all 0 against a weight row of all -128 and one of all 127; s32 out,
    scale 1, so nothing is hidden by saturation: 255 * 127 * 65025 and 255 * -128 * 65025 are reached"""
    out = []
    for k in (200, KMAX):
        case = LinCase("comp", 2, k, 2, src_dt=U8, dst_dt=S32, scale=1.0, seed=20000 + k)
        raw = np.full((2, case.sld), 0xFF, dtype=np.uint8)
        raw[1, :k] = 0
        w = np.empty((2, k), dtype=np.int8)
        w[0], w[1] = -128, 127
        out.append((case, dict(src=raw.reshape(-1), w=w, bia=None, scales=np.ones(1, dtype=np.float32), lut=None)))
    return out


def lane_map_case(bm):
    """identity-like src rows (row m holds the single value 1 + m // k at column m % k) against asymmetric weights
    (every (o, c) its own residue): a transposed, swapped or shifted fragment shows in every element; s32 out, scale 1"""
    rows, k, n = 2 * bm, 96, 2 * BN + 8
    case = LinCase("lanes%d" % bm, rows, k, n, src_dt=S8, dst_dt=S32, scale=1.0, seed=21000 + bm)
    raw = np.full((rows, case.sld), 0xFF, dtype=np.uint8)
    raw[:, :k] = 0
    m = np.arange(rows)
    raw[m, m % k] = 1 + m // k
    o, c = np.arange(n).reshape(-1, 1), np.arange(k).reshape(1, -1)
    w = ((o * 7 + c * 13 + (o * c) % 5) % 251 - 125).astype(np.int8)
    return case, dict(src=raw.reshape(-1).view(np.int8), w=w, bia=None, scales=np.ones(1, dtype=np.float32), lut=None)


def bias_cases():
    """bias of every dtype with per-channel scales, both src dtypes"""
    return [LinCase("bias", 70, 100, 133, src_dt=(S8, U8)[i % 2], dst_dt=(S8, U8, S32, F32)[i], bia_dt=b, per_channel=True, seed=22000 + i)
            for i, b in enumerate((F32, S32, S8, U8))]


def tie_cases():
    """small integers at scale 0.5: every odd accumulator is a tie, in both round modes; s8 and u8 out"""
    return [LinCase("ties", 66, 17, 40, src_dt=(U8, S8)[i % 2], dst_dt=(S8, U8)[i // 2], rm=rm, scale=0.5, small=True, seed=23000 + i + 10 * rm)
            for i in range(4) for rm in (0, 1)]


def nonfinite_cases():
    """scales of inf and NaN (the exact route only: set_weights must refuse to call them fast): the x86 0x80000000 pattern and
    its saturations; built to saturate"""
    return [LinCase("nonfinite", 33, 40, 34, src_dt=(U8, S8)[i % 2], dst_dt=dst, scale=scale, saturating=True, seed=24000 + i)
            for scale in (float("inf"), float("nan")) for i, dst in enumerate((U8, S8, S32, F32))]


def table_cases():
    """u8 and s8 index types against u8 and s8 dst, with a random permutation table, with and without ReLU and bias"""
    out = []
    for i, (lut_in, dst) in enumerate(((U8, U8), (U8, S8), (S8, U8), (S8, S8))):
        out.append(LinCase("table", 130, 72, 200, src_dt=(S8, U8)[i % 2], dst_dt=dst, bia_dt=(UNDEF, S32)[i % 2], relu=bool(i // 2 == 1 and i % 2),
                           lut_in=lut_in, dst_ld=_dst_ld(200, i % 3), seed=25000 + i))
    return out


def pitched_cases():
    """src_ld > k (a slice of a wider tensor), dst_ld > n, and both: a projection written into a third of a QKV-shaped tensor"""
    return [LinCase("slice-src", 100, 64, 96, src_ld=192, seed=26000), LinCase("pad-dst", 100, 80, 60, dst_ld=77, dst_dt=U8, seed=26001),
            LinCase("qkv-third", 100, 64, 64, src_ld=64, dst_ld=192, bia_dt=S32, seed=26002),
            LinCase("pitched-f32", 65, 48, 36, src_dt=U8, src_ld=80, dst_ld=40, dst_dt=F32, seed=26003)]


GRID_CAP_CASE = LinCase("gridcap", 3 * 64 + 5, 100, 2 * BN + 8, src_dt=U8, dst_dt=S8, bia_dt=S32, seed=27000)   # 4 x 3 = 12 tiles of 64


def fc_twin_cases():
    """u8 src, src_ld = k, dst_ld = n: the op coincides with dfx_fc (ih = iw = 1, ic = k, bs = rows); all four dst dtypes, both
    round modes, with and without bias; k = 128 reaches dfx_fc's MFMA kernel, k = 96 its generic one"""
    out = []
    for i, dst in enumerate((U8, S8, S32, F32)):
        for rm in (0, 1):
            out.append(LinCase("fctwin", 37, (128, 96)[i % 2], 70, src_dt=U8, dst_dt=dst, bia_dt=(UNDEF, S32)[(i + rm) % 2], rm=rm,
                               relu=bool(i % 2), src_ld=(128, 96)[i % 2], per_channel=bool(rm), seed=28000 + 2 * i + rm))
    return out


def bmm_twin_cases():
    """no bias: the op coincides with dfx_bmm (trans_b, one matrix, the weights uploaded as B): u8 and s8 src, dense and pitched"""
    return [LinCase("bmmtwin", 70, 100, 90, src_dt=U8, dst_dt=S8, seed=29000), LinCase("bmmtwin", 70, 100, 90, src_dt=S8, dst_dt=U8, seed=29001),
            LinCase("bmmtwin", 50, 64, 64, src_dt=S8, dst_dt=S32, src_ld=192, dst_ld=96, per_channel=True, seed=29002),
            LinCase("bmmtwin", 50, 40, 36, src_dt=U8, dst_dt=F32, src_ld=48, dst_ld=40, rm=1, seed=29003)]


AUTO_POINT_CASE = LinCase("auto-detr", 1700, 256, 256, src_dt=S8, dst_dt=S8, bia_dt=S32, seed=37000)   # the smallest measured point
MISALIGNED_CASES = (LinCase("misaligned", 70, 100, 64, src_dt=U8, dst_dt=S8, bia_dt=S32, seed=33000),
                    LinCase("misaligned", 70, 64, 64, src_dt=S8, dst_dt=F32, seed=33001))
ERROR_CASES = (LinCase("errors", 40, 64, 48, dst_dt=F32, seed=34000), LinCase("errors", 40, 64, 48, dst_dt=S8, lut_in=S8, seed=34001))
THREADS_CASE = LinCase("threads", 150, 136, 140, src_dt=U8, dst_dt=S8, bia_dt=S32, seed=35000)
GELU_CASE = LinCase("gelu", 70, 64, 256, src_dt=S8, dst_dt=S8, bia_dt=S32, lut_in=S8, seed=31000)      # (the test swaps dfa.gelu_table in)
QKV_CASES = tuple(LinCase("qkv", 100, 64, 64, src_ld=64, dst_ld=192, bia_dt=S32, seed=32000 + third) for third in range(3))
HOST_CASE = LinCase("host", 70, 96, 50, src_dt=U8, dst_dt=S32, bia_dt=S8, src_ld=96, per_channel=True, seed=38000)
CXX_FC1_CASE = LinCase("fc1", 2 * 50, 64, 256, src_dt=S8, dst_dt=S8, bia_dt=S32, lut_in=S8, seed=36000)


def generated_cases():
    """every case whose data comes from generate(): what test_linear_cpu holds to the regime condition"""
    out = []
    for bm in BMS:
        for src_dt in (U8, S8):
            out += list(shape_grid(bm, src_dt))
    return out + bias_cases() + tie_cases() + nonfinite_cases() + table_cases() + pitched_cases() + [GRID_CAP_CASE] + fc_twin_cases() + \
        bmm_twin_cases() + [AUTO_POINT_CASE, THREADS_CASE, GELU_CASE, HOST_CASE, CXX_FC1_CASE] + list(MISALIGNED_CASES + ERROR_CASES + QKV_CASES)


def with_dst(case, **kw):
    return replace(case, **kw)
