"""Reference, data, case tables and plan mirror of the batched int8 matrix product's tests (pure numpy, needs no GPU).

The op (include/dfx.h, dfx_bmm_*): for g = b0 * batch1 + b1
    acc[g,m,n] = sum_k A[g,m,k] * B[g,n,k] (trans_b) or A[g,m,k] * B[g,k,n];  f = float(acc) * scale[n or 0];
    ReLU (asked for, or dst u8): f = (0 > f) ? 0 : f;  C[g,m,n] = store(f, dst_dt, round_mode)
with per-operand addressing base + b0*s0 + b1*s1 + row*ld + col.  `reference` works on whole STORAGE arrays: it gathers the
operands through their strides (pad columns never take part), accumulates in int64, runs the np.float32 steps in the
order above, and scatters into a poisoned copy of C's storage, so that a comparison of the whole storage also checks that
elements N .. ldc-1 of every row, and everything between the matrices, are not written.  tests/test_bmm_cpu.py pins it
against a pure-Python witness and against fc_ref (itself pinned to the C oracle).
"""
from dataclasses import dataclass, replace

import numpy as np

F32, S32, S8, U8 = 1, 2, 3, 4
NP_OF = {F32: np.float32, S32: np.int32, S8: np.int8, U8: np.uint8}
NAME_OF = {F32: "f32", S32: "s32", S8: "s8", U8: "u8"}
SIZE_OF = {F32: 4, S32: 4, S8: 1, U8: 1}
MFMA, GENERIC = 0, 1            # DFX_BMM_MFMA / DFX_BMM_GENERIC
KMAX = 65025
MN_MAX = 2 ** 31 - 32
POISON = 0xCD                   # hipref.POISON_BYTE
DST_ROTATION = (U8, S8, S32, F32)


def up16(v):
    return -(-v // 16) * 16


@dataclass(frozen=True)
class BmmCase:
    name: str
    m: int
    n: int
    k: int
    trans_b: bool = True
    a_dt: int = U8
    dst_dt: int = S8
    batch: tuple = (1, 1)
    relu: bool = False
    rm: int = 0
    per_channel: bool = False
    a_strides: tuple = None       # (s0, s1, ld) in elements; None: matrices packed one behind the other, ld = up16(cols)
    b_strides: tuple = None
    c_strides: tuple = None       # None: ld = n + 3 (odd rows, never vector-aligned) unless c_ld is given
    c_ld: int = None
    scale: float = None           # None: centred (see make_scales)
    saturating: bool = False      # built to saturate: exempt from the 10 % cap of test_bmm_cpu
    seed: int = 1

    @property
    def g(self):
        return self.batch[0] * self.batch[1]

    @property
    def b_shape(self):
        return (self.n, self.k) if self.trans_b else (self.k, self.n)

    def strides(self, which):
        """(s0, s1, ld) of operand 'a' | 'b' | 'c'"""
        given = {"a": self.a_strides, "b": self.b_strides, "c": self.c_strides}[which]
        if given is not None:
            return tuple(int(v) for v in given)
        rows, cols = {"a": (self.m, self.k), "b": self.b_shape, "c": (self.m, self.n)}[which]
        ld = (self.c_ld or self.n + 3) if which == "c" else up16(cols)
        return self.batch[1] * rows * ld, rows * ld, ld

    def ident(self):
        return "%s-%s-%dx%d-m%d-n%d-k%d-%s-%s-r%d-m%d-pc%d" % (
            self.name, "nt" if self.trans_b else "nn", self.batch[0], self.batch[1], self.m, self.n, self.k, NAME_OF[self.a_dt],
            NAME_OF[self.dst_dt], self.relu, self.rm, self.per_channel)


def index(case, which):
    """int64 {batch0, batch1, rows, cols}: the element index of every valid element of operand `which`"""
    s0, s1, ld = case.strides(which)
    rows, cols = {"a": (case.m, case.k), "b": case.b_shape, "c": (case.m, case.n)}[which]
    b0 = np.arange(case.batch[0], dtype=np.int64).reshape(-1, 1, 1, 1) * s0
    b1 = np.arange(case.batch[1], dtype=np.int64).reshape(1, -1, 1, 1) * s1
    return b0 + b1 + np.arange(rows, dtype=np.int64).reshape(1, 1, -1, 1) * ld + np.arange(cols, dtype=np.int64).reshape(1, 1, 1, -1)


def storage_elems(case, which):
    """elements of the operand's storage: for A and B up to the valid columns of the last row rounded up to 16, within the
    leading dimension (what the MFMA kernel, which reads whole 16-byte pieces of a row, may touch: a head-sliced operand
    then ends where its {bs, T, heads * d} tensor ends); for C up to the last valid element"""
    s0, s1, ld = case.strides(which)
    rows, cols = {"a": (case.m, case.k), "b": case.b_shape, "c": (case.m, case.n)}[which]
    last = (case.batch[0] - 1) * s0 + (case.batch[1] - 1) * s1 + (rows - 1) * ld
    return last + (cols if which == "c" else min(ld, up16(cols)))


def make_scales(case):
    """scales that centre the output: a 1-byte dst gets a standard deviation of about 40 (a value of 127 is beyond three of
    them, so far less than 10 % saturate); a 4-byte dst gets a scale near 0.37, which no accumulator of K <= 65025 can take
    to 2^31"""
    if case.scale is not None:
        s = np.float32(case.scale)
    elif case.dst_dt in (S32, F32):
        s = np.float32(0.37)
    else:
        sd = (147.0 if case.a_dt == U8 else 74.0) * 74.0 * np.sqrt(case.k)
        s = np.float32(40.0 / sd)
    if case.per_channel:
        return (s * (0.5 + np.arange(case.n) / case.n)).astype(np.float32)
    return np.array([s], dtype=np.float32)


def generate(case):
    """-> dict(a, b: flat storage arrays; scales).  Valid elements are uniform over the whole dtype; every other byte of A's
    storage is 0xFF (255 as u8, -1 as s8) and of B's a random NON-ZERO byte: pad columns that took part would show."""
    rng = np.random.default_rng(case.seed)
    out = {}
    for which, dt in (("a", case.a_dt), ("b", S8)):
        n = storage_elems(case, which)
        raw = rng.integers(0, 256, n).astype(np.uint8)
        valid = np.zeros(n, dtype=bool)
        valid[index(case, which).reshape(-1)] = True
        raw[~valid] = 0xFF if which == "a" else rng.integers(1, 256, int((~valid).sum())).astype(np.uint8)
        out[which] = raw.view(NP_OF[dt])
    if (case.relu or case.dst_dt == U8) and case.a_dt == U8:
        # a u8 A against a B row of negative sum leaves little but the ReLU's zeros in that column (all of C where N = 1):
        # the rows of B with an even n are negated where their sum is not positive, so that no case of the tables is all zero
        ib = index(case, "b")
        ib = ib if case.trans_b else np.swapaxes(ib, 2, 3)              # {b0, b1, n, k}
        bv = out["b"][ib].astype(np.int16)
        flip = bv.sum(axis=3, keepdims=True) <= 0
        flip[:, :, 1::2] = False
        bv = np.where(flip, np.clip(-bv, -127, 127), bv)
        bv[..., 0] = np.where(flip[..., 0] & (bv.sum(axis=3) <= 0), 1, bv[..., 0])   # (a row of zeros)
        out["b"][ib.reshape(-1)] = bv.astype(np.int8).reshape(-1)
    out["scales"] = make_scales(case)
    return out


def accumulate(case, a, b):
    """exact int64 accumulators {batch0, batch1, m, n}"""
    av = a[index(case, "a")].astype(np.int64)
    bv = b[index(case, "b")].astype(np.int64)
    if case.trans_b:
        bv = np.swapaxes(bv, 2, 3)
    return np.matmul(av, bv)


def cvt_x86(f, rm):
    """vcvtps2dq: nearest even or floor; NaN / out of range -> 0x80000000"""
    with np.errstate(invalid="ignore"):
        ok = (f >= np.float32(-2147483648.0)) & (f < np.float32(2147483648.0))
        r = np.floor(f) if rm == 1 else np.rint(f)
        return np.where(ok, np.where(ok, r, 0).astype(np.int64), -2147483648)


def finish(acc, scales, dst_dt, relu, rm):
    """the np.float32 steps behind the accumulator, in the op's order; scales broadcast over the last axis"""
    with np.errstate(invalid="ignore", over="ignore"):
        f = acc.astype(np.float32)                                  # int -> f32, nearest even
        f = (f * np.asarray(scales, dtype=np.float32)).astype(np.float32)   # one separately rounded multiply
        if relu or dst_dt == U8:
            f = np.where(np.float32(0) > f, np.float32(0), f)       # vmaxps(zero, f): NaN and -0 pass
    if dst_dt == F32:
        return f.astype(np.float32)
    v = cvt_x86(f, rm)
    if dst_dt == S32:
        return v.astype(np.int32)
    if dst_dt == S8:
        return np.clip(v, -128, 127).astype(np.int8)
    return np.where((v < 0) | (v > 255), 255, v).astype(np.uint8)    # unsigned saturation of the bit pattern


def values(case, data):
    """the valid elements of C, {batch0, batch1, m, n}"""
    return finish(accumulate(case, data["a"], data["b"]), data["scales"], case.dst_dt, case.relu, case.rm)


def reference(case, data):
    """C's whole storage as bytes: POISON everywhere but the valid elements"""
    vals = values(case, data)
    out = np.full(storage_elems(case, "c"), POISON, dtype=np.uint8).repeat(SIZE_OF[case.dst_dt]).view(NP_OF[case.dst_dt])
    out[index(case, "c").reshape(-1)] = vals.reshape(-1)
    return out.view(np.uint8)


def witness(case, data):
    """the same storage, element by element on Python ints and np.float32 scalars"""
    sa, sb, sc = case.strides("a"), case.strides("b"), case.strides("c")
    a, b, scales = data["a"], data["b"], data["scales"]
    out = np.full(storage_elems(case, "c"), POISON, dtype=np.uint8).repeat(SIZE_OF[case.dst_dt]).view(NP_OF[case.dst_dt])
    for b0 in range(case.batch[0]):
        for b1 in range(case.batch[1]):
            for m in range(case.m):
                for n in range(case.n):
                    acc = 0
                    for k in range(case.k):
                        bi = (n * sb[2] + k) if case.trans_b else (k * sb[2] + n)
                        acc += int(a[b0 * sa[0] + b1 * sa[1] + m * sa[2] + k]) * int(b[b0 * sb[0] + b1 * sb[1] + bi])
                    with np.errstate(invalid="ignore", over="ignore"):
                        f = np.float32(acc) * np.float32(scales[n if len(scales) > 1 else 0])
                    if (case.relu or case.dst_dt == U8) and np.float32(0) > f:
                        f = np.float32(0)
                    if case.dst_dt == F32:
                        v = f
                    else:
                        if not (f >= np.float32(-2147483648.0) and f < np.float32(2147483648.0)):
                            v = -2147483648
                        else:
                            v = int(np.floor(f)) if case.rm == 1 else int(np.rint(f))
                        if case.dst_dt == S8:
                            v = max(-128, min(127, v))
                        elif case.dst_dt == U8:
                            v = 255 if (v < 0 or v > 255) else v
                    out[b0 * sc[0] + b1 * sc[1] + m * sc[2] + n] = v
    return out.view(np.uint8)


def saturated_fraction(case, vals):
    """share of the outputs on a saturation bound of dst's conversion (u8: 255; s8: -128 / 127; s32: +-2^31; f32: none).
    A ReLU's 0 is the op's own result, not a saturation: the CPU test asks separately that a case is not all zero."""
    if case.dst_dt == F32:
        return 0.0
    lo, hi = {U8: (None, 255), S8: (-128, 127), S32: (-2 ** 31, 2 ** 31 - 1)}[case.dst_dt]
    hit = vals == hi
    if lo is not None:
        hit = hit | (vals == lo)
    return float(hit.mean())


# --- the plan of bmm_plan.h, mirrored ---------------------------------------------------------------------------------------
INVALID, UNSUPPORTED = 1, 2
MAX_ELEMS = 1 << 40
GRID_PER_CU, WAVES, THREADS = 16, 4, 256
NN_LDS = WAVES * 2 * 32 * 48


def c_disjoint(n, m, batch1, batch0, ldc, c_s1, c_s0):
    """the C-overlap rule of include/dfx.h"""
    pairs = [(e, s) for e, s in ((n, 1), (m, ldc), (batch1, c_s1), (batch0, c_s0)) if e != 1]
    pairs.sort(key=lambda p: p[1])
    if pairs and pairs[0][1] < 1:                      # a stride of 0 under an extent above 1
        return False
    return all(pairs[i][1] >= pairs[i - 1][1] * pairs[i - 1][0] for i in range(1, len(pairs)))


def span(batch0, batch1, s0, s1, ld, rows, cols):
    return (batch0 - 1) * s0 + (batch1 - 1) * s1 + (rows - 1) * ld + cols


def mfma_class(d):
    return d["b_dt"] == S8 and all(d[k] % 16 == 0 for k in ("lda", "ldb", "a_s0", "a_s1", "b_s0", "b_s1"))


def validate(d):
    """0, INVALID or UNSUPPORTED for a descriptor given as a dict of dfx_bmm_desc's fields, in the header's order"""
    if min(d["batch0"], d["batch1"], d["m"], d["n"], d["k"]) < 1 or max(d["m"], d["n"]) > MN_MAX or d["k"] > KMAX:
        return INVALID
    if d["trans_b"] not in (0, 1) or d["a_dt"] not in (U8, S8) or d["b_dt"] not in (U8, S8) or d["dst_dt"] not in NP_OF:
        return INVALID
    if d["round_mode"] not in (0, 1) or d["nscales"] not in (1, d["n"]) or d["force_path"] not in (-1, MFMA, GENERIC):
        return INVALID
    brows, bcols = (d["n"], d["k"]) if d["trans_b"] else (d["k"], d["n"])
    if d["lda"] < d["k"] or d["ldb"] < bcols or d["ldc"] < d["n"]:
        return INVALID
    if min(d[k] for k in ("a_s0", "a_s1", "b_s0", "b_s1", "c_s0", "c_s1")) < 0:
        return INVALID
    if not c_disjoint(d["n"], d["m"], d["batch1"], d["batch0"], d["ldc"], d["c_s1"], d["c_s0"]):
        return INVALID
    if max(span(d["batch0"], d["batch1"], d["a_s0"], d["a_s1"], d["lda"], d["m"], d["k"]),
           span(d["batch0"], d["batch1"], d["b_s0"], d["b_s1"], d["ldb"], brows, bcols),
           span(d["batch0"], d["batch1"], d["c_s0"], d["c_s1"], d["ldc"], d["m"], d["n"])) >= MAX_ELEMS:
        return INVALID
    if d["b_dt"] == U8:
        return UNSUPPORTED
    if d["force_path"] == MFMA and not mfma_class(d):
        return UNSUPPORTED
    return 0


def desc_of(case, force_path=-1):
    """the dict of dfx_bmm_desc's fields of a case"""
    a, b, c = case.strides("a"), case.strides("b"), case.strides("c")
    return dict(batch0=case.batch[0], batch1=case.batch[1], m=case.m, n=case.n, k=case.k, trans_b=int(case.trans_b), a_dt=case.a_dt,
                b_dt=S8, dst_dt=case.dst_dt, relu=int(case.relu), round_mode=case.rm, nscales=case.n if case.per_channel else 1,
                force_path=force_path, a_s0=a[0], a_s1=a[1], lda=a[2], b_s0=b[0], b_s1=b[1], ldb=b[2], c_s0=c[0], c_s1=c[1], ldc=c[2])


AUTO_MIN_M, AUTO_MIN_N, AUTO_MIN_K, AUTO_MIN_MACS, AUTO_MIN_TILES = 49, 32, 32, 192 * 49 * 49 * 32, 384


def auto_path(d):
    """the AUTO RULE (DFX_BMM_AUTO_NOTE): the MFMA kernel in its class from the smallest of each size at which it was measured
    and won (M, N, K and the multiply-adds of the Swin window point, and 384 tiles of 32 x 32); generic everywhere else"""
    if d["force_path"] != -1:
        return d["force_path"]
    big = d["m"] >= AUTO_MIN_M and d["n"] >= AUTO_MIN_N and d["k"] >= AUTO_MIN_K and tiles(d) >= AUTO_MIN_TILES and \
        d["batch0"] * d["batch1"] * d["m"] * d["n"] * d["k"] >= AUTO_MIN_MACS
    return MFMA if big and mfma_class(d) else GENERIC


def tiles(d):
    return d["batch0"] * d["batch1"] * -(-d["m"] // 32) * -(-d["n"] // 32)


def planned_grid(d, path, cus, cap=0):
    blocks = -(-tiles(d) // WAVES) if path == MFMA else -(-(d["batch0"] * d["batch1"] * d["m"] * d["n"]) // THREADS)
    blocks = min(blocks, max(1, cus) * GRID_PER_CU)
    if cap > 0:
        blocks = min(blocks, cap)
    return max(1, blocks)


def lds_bytes(d, path):
    return NN_LDS if path == MFMA and not d["trans_b"] else 0


def fast_ok(d, scales):
    if d["round_mode"] != 0:
        return False
    bound = (255.0 if d["a_dt"] == U8 else 128.0) * 128.0 * d["k"]
    return all(np.isfinite(s) and bound * abs(float(s)) <= 2.0 ** 30 for s in np.asarray(scales, dtype=np.float32))


def algorithmic_ops(d):
    return 2 * d["batch0"] * d["batch1"] * d["m"] * d["n"] * d["k"]


def algorithmic_bytes(d):
    ga = (1 if d["a_s0"] == 0 else d["batch0"]) * (1 if d["a_s1"] == 0 else d["batch1"])
    gb = (1 if d["b_s0"] == 0 else d["batch0"]) * (1 if d["b_s1"] == 0 else d["batch1"])
    return ga * d["m"] * d["k"] + gb * d["k"] * d["n"] + d["batch0"] * d["batch1"] * d["m"] * d["n"] * SIZE_OF[d["dst_dt"]]


def kernel_name(case, path, route):
    form = "nt" if case.trans_b else "nn"
    if path == MFMA:
        return "bmm_mfma<%s,%s,%s> %s" % (form, NAME_OF[case.a_dt], NAME_OF[case.dst_dt], "fast" if route else "exact")
    return "bmm_generic<%s,%s,%s> exact" % (form, NAME_OF[case.a_dt], NAME_OF[case.dst_dt])


# --- case tables ------------------------------------------------------------------------------------------------------------
GRID_MN = (1, 31, 32, 33, 65, 130)
GRID_K = (1, 15, 16, 17, 63, 64, 65, 96, 200)


def shape_grid():
    """M, N x K for both forms and both A dtypes; the dst dtype, relu, the round mode, per-channel scales and C's leading
    dimension (n + 3: never aligned; up16(n): vector stores) rotate through the grid"""
    out, i = [], 0
    for trans_b in (True, False):
        for a_dt in (U8, S8):
            for m in GRID_MN:
                for n in GRID_MN:
                    for k in GRID_K:
                        out.append(BmmCase("grid", m, n, k, trans_b=trans_b, a_dt=a_dt, dst_dt=DST_ROTATION[i % 4], relu=(i // 4) % 3 == 1,
                                           rm=(i // 12) % 2, per_channel=(i // 3) % 2 == 1, c_ld=up16(n) if (i // 5) % 2 else None,
                                           seed=30000 + i))
                        i += 1
    return out


HEADS, T, D, BS = 3, 37, 32, 2


def attention_strides(bs, heads, t, d, ld=None):
    ld = heads * d if ld is None else ld
    return t * ld, d, ld


def batch_cases():
    """(1,1) and (2,3) batches, dense; head-sliced A and B of a {bs, T, heads * d} tensor with C = the logits {bs, heads, T, T}
    (rows 48 apart); C written interleaved back into {bs, T, heads * d}; B broadcast over batch1"""
    hs = attention_strides(BS, HEADS, T, D)
    out = []
    i = 0
    for a_dt in (U8, S8):
        for batch in ((1, 1), (2, 3)):
            for trans_b in (True, False):
                out.append(BmmCase("dense", 33, 37, 40, trans_b=trans_b, a_dt=a_dt, dst_dt=DST_ROTATION[i % 4], batch=batch, seed=31000 + i))
                i += 1
        # Q . K^T over the heads: A, B head-sliced; logits {bs, heads, T, 48}
        out.append(BmmCase("heads-qk", T, T, D, trans_b=True, a_dt=a_dt, dst_dt=S8, batch=(BS, HEADS), a_strides=hs, b_strides=hs,
                           c_strides=(HEADS * T * 48, T * 48, 48), seed=31100 + i))
        # P . V: A = probabilities {bs, heads, T, 48} (K = 37 over rows 48 apart), B = V head-sliced, C interleaved back
        out.append(BmmCase("heads-pv", T, D, T, trans_b=False, a_dt=a_dt, dst_dt=DST_ROTATION[i % 4], batch=(BS, HEADS),
                           a_strides=(HEADS * T * 48, T * 48, 48), b_strides=hs, c_strides=hs, seed=31200 + i))
        # B broadcast over batch1 (one key matrix for every head)
        out.append(BmmCase("bcast", 33, 37, 40, trans_b=True, a_dt=a_dt, dst_dt=S32, batch=(2, 3), b_strides=(37 * 48, 0, 48), seed=31300 + i))
        out.append(BmmCase("bcast", 33, 37, 40, trans_b=False, a_dt=a_dt, dst_dt=S8, batch=(2, 3), b_strides=(0, 0, 48), per_channel=True,
                           seed=31400 + i))
    return out


def compensation_cases():
    """-> [(case, data)]: u8 A all 255 / all 0 / random against B all -128 / all 127 / random, s32 dst, scale 1: K = 200, and
    K = 65025 with M = N = 33 and one batch"""
    out = []
    for k, m, n in ((200, 40, 70), (KMAX, 33, 33)):
        for trans_b in (True, False):
            case = BmmCase("comp", m, n, k, trans_b=trans_b, a_dt=U8, dst_dt=S32, scale=1.0, seed=32000 + k % 7 + int(trans_b))
            base = generate(case)
            ia, ib = index(case, "a").reshape(-1), index(case, "b").reshape(-1)
            for fa in (255, 0, None):
                for fb in (-128, 127, None):
                    a, b = base["a"].copy(), base["b"].copy()
                    if fa is not None:
                        a[ia] = fa
                    if fb is not None:
                        b[ib] = fb
                    out.append((replace(case, name="comp-a%s-b%s" % (fa, fb)), dict(a=a, b=b, scales=base["scales"])))
    return out


def lane_map_case(trans_b):
    """-> (case, data, want): A = identity-like rows (A[m][k] = 1 where k == m), B asymmetric: (3 n + 5 k) mod 251 - 125 at
    logical (n, k); C must be B (transposed into {m, n}) exactly: C[m][n] = B[n][k = m]"""
    m = n = k = 70
    case = BmmCase("lanes", m, n, k, trans_b=trans_b, a_dt=S8, dst_dt=S32, scale=1.0, seed=33000)
    data = generate(case)
    a, b = data["a"].copy(), data["b"].copy()
    a[index(case, "a").reshape(-1)] = np.eye(m, k, dtype=np.int8).reshape(-1)
    nn, kk = np.meshgrid(np.arange(n), np.arange(k), indexing="ij")
    logical = ((3 * nn + 5 * kk) % 251 - 125).astype(np.int8)           # {n, k}
    b[index(case, "b").reshape(-1)] = (logical if trans_b else logical.T).reshape(-1)
    return case, dict(a=a, b=b, scales=data["scales"]), logical.T.astype(np.int32)   # {m = k, n}


def tie_cases():
    """-> [(case, data)]: scale 0.5 with every accumulator odd (A = 1 in column 0, 0 elsewhere; B odd in k = 0), both round
    modes, u8 / s8 / s32 dst: nearest-even against floor on every value"""
    out = []
    for trans_b in (True, False):
        for rm in (0, 1):
            for dst in (U8, S8, S32):
                case = BmmCase("ties", 33, 40, 17, trans_b=trans_b, a_dt=U8, dst_dt=dst, rm=rm, scale=0.5, seed=34000)
                data = generate(case)
                a, b = data["a"].copy(), data["b"].copy()
                av = np.zeros((33, 17), dtype=np.uint8)
                av[:, 0] = 1
                a[index(case, "a").reshape(-1)] = av.reshape(-1)
                logical = np.random.default_rng(34001).integers(-128, 128, (40, 17)).astype(np.int8)
                logical[:, 0] |= 1                                         # odd
                b[index(case, "b").reshape(-1)] = (logical if trans_b else logical.T).reshape(-1)
                out.append((case, dict(a=a, b=b, scales=data["scales"])))
    return out


def nonfinite_cases():
    """scales of inf and NaN (the exact route only: set_scales must refuse to call them fast): the x86 0x80000000 pattern and
    its saturations (u8 255, s8 -128); built to saturate"""
    out = []
    for scale in (float("inf"), float("nan")):
        for dst in (U8, S8, S32, F32):
            out.append(BmmCase("nonfinite", 33, 34, 40, trans_b=dst in (U8, S32), a_dt=U8 if dst in (U8, S8) else S8, dst_dt=dst, scale=scale,
                               saturating=True, seed=35000))
    return out


GRID_CAP_CASE = BmmCase("cap", 70, 130, 96, trans_b=True, a_dt=U8, dst_dt=S8, batch=(1, 2), seed=36000)   # 2 * 3 * 5 = 30 tiles, 8 units

FC_TWIN = [(k, m, n) for k in (64, 192) for m in (1, 33) for n in (10, 96)]


def table():
    """every case whose data comes from generate(): what test_bmm_cpu holds to the regimes"""
    return shape_grid() + batch_cases() + nonfinite_cases() + [GRID_CAP_CASE]
