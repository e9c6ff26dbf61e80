"""Reference, data, case tables and plan mirror of the logit bias's tests (pure numpy, needs no GPU).

The logit bias (include/dfx.h, dfx_bmm_set_bias / dfx_attn_set_bias, dfx_logit_bias_desc) makes the matrix product
    f = float(acc[g,m,n]);  f = f + bias(g,m,n);  f = f * scale[n or 0];  ReLU;  C = store(f)
with bias(g,m,n) = table (b0 % period0, b1 % period1), row m (row 0 where the table has one row), column n, and the attention
stays the chain: that product with the bias -> head_ref's softmax -> bmm_ref's product.  The reference takes bmm_ref's exact
integer accumulators, adds the bias as one np.float32 addition, multiplies as one np.float32 multiplication and then follows
bmm_ref.finish step for step; `witness` does the same element by element on Python ints and np.float32 scalars.  The host
table is built in the caller's layout with NaN in every float the layout does not address: a library that read one of them
would refuse the table.  tests/test_attn_bias_cpu.py pins reference against witness, the regimes of the cases and the mirror of
csrc/bias_plan.h against tools/bias_plan_check.
"""
from dataclasses import dataclass, replace

import numpy as np

import attn_ref as A
import bmm_ref as B
import head_ref as H

F32, S32, S8, U8 = B.F32, B.S32, B.S8, B.U8
POISON = B.POISON
NINF = np.float32(-np.inf)


@dataclass(frozen=True)
class Bias:
    """a logit bias over an {m, n} product with batch (batch0, batch1)"""
    periods: tuple = (1, 1)
    one_row: bool = False         # ld = 0: a {n} row broadcast over m
    strides: tuple = None         # host (s0, s1, ld) in floats; None: densely packed
    mask: str = None              # None | "random" (10 % of the entries) | "causal" | "keypad" (the last keys of a row, by table) |
    #                               "window" (Swin's: two regions per table) | "row0" (all of row 0 of every table: a fully masked row)
    mask_value: str = "finite"    # "finite": attention_bias()'s value; "ninf": -inf
    finite: bool = True           # draw the finite entries (False: 0 wherever nothing is masked)
    seed: int = 1

    def layout(self, m, n):
        if self.strides is not None:
            return tuple(int(v) for v in self.strides)
        rows = 1 if self.one_row else m
        return self.periods[1] * rows * n, rows * n, 0 if self.one_row else n

    def rows(self, m):
        return 1 if self.one_row else m


def acc_bound(a_dt, k):
    return (255 if a_dt == U8 else 128) * 128 * k


def finite_mask_value(bound, logit_scale):
    """dfa.attention_bias()'s value for a masked entry: -(acc_bound + ceil(129 / |logit_scale|)), with the scale's sign, rounded
    away from zero to f32"""
    mag = float(bound) + float(np.ceil(129.0 / abs(float(logit_scale))))
    mv = np.float32(mag)
    if float(mv) < mag:
        mv = np.nextafter(mv, np.float32(np.inf))
    return np.float32(-mv if logit_scale > 0 else mv)


def mask_of(bias, m, n):
    """bool {p0, p1, rows, n}: the masked entries"""
    p0, p1 = bias.periods
    rows = bias.rows(m)
    shape = (p0, p1, rows, n)
    rng = np.random.default_rng(bias.seed + 101)
    if bias.mask is None:
        return np.zeros(shape, dtype=bool)
    if bias.mask == "random":
        return rng.random(shape) < 0.10
    if bias.mask == "causal":
        assert rows == m
        return np.broadcast_to(np.arange(n)[None, :] > np.arange(m)[:, None], shape).copy()
    if bias.mask == "keypad":                           # table t pads its last n // 5 + 1 + 5 t keys (never all of them)
        out = np.zeros(shape, dtype=bool)
        for t in range(p0 * p1):
            out[t // p1, t % p1, :, n - min(n - 1, n // 5 + 1 + 5 * t):] = True
        return out
    if bias.mask == "window":                           # table (w, .): queries and keys below / above a cut 7 (w + 1) see only their side
        out = np.zeros(shape, dtype=bool)
        for w in range(p0):
            cut = 7 * (w + 1)
            side_q, side_k = np.arange(rows) < min(cut, rows - 1), np.arange(n) < min(cut, n - 1)
            out[w] = (side_q[:, None] != side_k[None, :])[None]
        return out
    if bias.mask == "row0":
        out = rng.random(shape) < 0.10
        out[:, :, 0, :] = True
        return out
    raise ValueError(bias.mask)


def make_bias(bias, m, n, scale, bound):
    """-> dict(values {p0, p1, rows, n} f32, table: the flat host array in the caller's layout (NaN in the gaps), layout (s0, s1, ld),
    masked: bool {p0, p1, rows, n}).  Finite entries: value * scale uniform in [-32, 32] output steps."""
    p0, p1 = bias.periods
    rows = bias.rows(m)
    rng = np.random.default_rng(bias.seed)
    steps = rng.uniform(-32.0, 32.0, (p0, p1, rows, n)) if bias.finite else np.zeros((p0, p1, rows, n))
    values = (steps / float(scale)).astype(np.float32)
    mv = NINF if bias.mask_value == "ninf" else finite_mask_value(bound, scale)
    values[mask_of(bias, m, n)] = mv
    s0, s1, ld = bias.layout(m, n)
    table = np.full(host_elems(dict(m=m, n=n), dict(period0=p0, period1=p1, s0=s0, s1=s1, ld=ld)), np.nan, dtype=np.float32)
    idx = host_index(bias, m, n)
    table[idx.reshape(-1)] = values.reshape(-1)
    values = table[idx]                                  # (tables that share floats -- a stride of 0 -- hold what was written last)
    masked = (values == mv) if bias.mask is not None else np.zeros(values.shape, dtype=bool)
    return dict(values=values, table=table, layout=(s0, s1, ld), masked=masked)


def host_index(bias, m, n):
    """int64 {p0, p1, rows, n}: the float index of every addressed entry of the host table"""
    s0, s1, ld = bias.layout(m, n)
    p0, p1 = bias.periods
    return np.arange(p0, dtype=np.int64).reshape(-1, 1, 1, 1) * s0 + np.arange(p1, dtype=np.int64).reshape(1, -1, 1, 1) * s1 + \
        np.arange(bias.rows(m), dtype=np.int64).reshape(1, 1, -1, 1) * ld + np.arange(n, dtype=np.int64).reshape(1, 1, 1, -1)


def expand(bias, values, batch, m):
    """{batch0, batch1, m, n} f32: the entry every element of every matrix uses"""
    p0, p1 = bias.periods
    t = values[np.arange(batch[0]) % p0][:, np.arange(batch[1]) % p1]
    return np.broadcast_to(t, (batch[0], batch[1], m, values.shape[3])).copy()


def finish(acc, bias_full, scales, dst_dt, relu, rm):
    """bmm_ref.finish with the one np.float32 addition in front of the multiplication"""
    with np.errstate(invalid="ignore", over="ignore"):
        f = acc.astype(np.float32)
        f = (f + bias_full).astype(np.float32)                       # one separately rounded add
        f = (f * np.asarray(scales, dtype=np.float32)).astype(np.float32)
        if relu or dst_dt == U8:
            f = np.where(np.float32(0) > f, np.float32(0), f)
    if dst_dt == F32:
        return f.astype(np.float32)
    v = B.cvt_x86(f, rm)
    if dst_dt == S32:
        return v.astype(np.int32)
    if dst_dt == S8:
        return np.clip(v, -128, 127).astype(np.int8)
    return np.where((v < 0) | (v > 255), 255, v).astype(np.uint8)


def prestore(case, data, bias, bd):
    """the f32 values in front of the ReLU and the store, {batch0, batch1, m, n}: (float(acc) + bias) * scale; bias None: float(acc) * scale"""
    with np.errstate(invalid="ignore", over="ignore"):
        f = B.accumulate(case, data["a"], data["b"]).astype(np.float32)
        if bias is not None:
            f = (f + expand(bias, bd["values"], case.batch, case.m)).astype(np.float32)
        return (f * np.asarray(data["scales"], dtype=np.float32)).astype(np.float32)


def prestore_saturates(case, f):
    """bool: the elements whose store leaves dst's range (a ReLU's 0 is the op's own result, not a saturation; f32 has none)"""
    with np.errstate(invalid="ignore"):
        r = np.floor(f) if case.rm == 1 else np.rint(f)
        if case.dst_dt == F32:
            return np.zeros(f.shape, dtype=bool)
        if case.dst_dt == S32:
            return ~((f >= np.float32(-2147483648.0)) & (f < np.float32(2147483648.0)))
        if case.dst_dt == U8:
            return r > 255
        return (r > 127) | ((r < -128) & (not case.relu))


def bmm_values(case, data, bias, bd):
    """the valid elements of C, {batch0, batch1, m, n}; bias None: bmm_ref's"""
    if bias is None:
        return B.values(case, data)
    return finish(B.accumulate(case, data["a"], data["b"]), expand(bias, bd["values"], case.batch, case.m), data["scales"], case.dst_dt, case.relu, case.rm)


def bmm_reference(case, data, bias, bd):
    """C's whole storage as bytes: POISON everywhere but the valid elements"""
    vals = bmm_values(case, data, bias, bd)
    out = np.full(B.storage_elems(case, "c"), POISON, dtype=np.uint8).repeat(B.SIZE_OF[case.dst_dt]).view(B.NP_OF[case.dst_dt])
    out[B.index(case, "c").reshape(-1)] = vals.reshape(-1)
    return out.view(np.uint8)


def bmm_witness(case, data, bias, bd):
    """the same storage, element by element on Python ints and np.float32 scalars, the bias read from the HOST table through
    the caller's layout"""
    sa, sb, sc = case.strides("a"), case.strides("b"), case.strides("c")
    a, b, scales = data["a"], data["b"], data["scales"]
    s0, s1, ld = bd["layout"]
    p0, p1 = bias.periods
    out = np.full(B.storage_elems(case, "c"), POISON, dtype=np.uint8).repeat(B.SIZE_OF[case.dst_dt]).view(B.NP_OF[case.dst_dt])
    for b0 in range(case.batch[0]):
        for b1 in range(case.batch[1]):
            for m in range(case.m):
                for n in range(case.n):
                    acc = 0
                    for k in range(case.k):
                        bi = (n * sb[2] + k) if case.trans_b else (k * sb[2] + n)
                        acc += int(a[b0 * sa[0] + b1 * sa[1] + m * sa[2] + k]) * int(b[b0 * sb[0] + b1 * sb[1] + bi])
                    entry = np.float32(bd["table"][(b0 % p0) * s0 + (b1 % p1) * s1 + m * ld + n])
                    with np.errstate(invalid="ignore", over="ignore"):
                        f = np.float32(np.float32(acc) + entry)
                        f = np.float32(f * np.float32(scales[n if len(scales) > 1 else 0]))
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


# --- the attention: the chain with the biased logits -------------------------------------------------------------------------
def attn_bias_data(case, data, bias):
    """make_bias for the logits' product of an attention case"""
    return make_bias(bias, case.tq, case.tk, data["logit_scale"][0], acc_bound(case.q_dt, case.d))


def attn_chain(case, data, bias, bd, witness=False):
    """-> (logits {G*tq, ldl} int8 with poison pad, probabilities likewise uint8, O's whole storage as bytes); bias None: attn_ref's"""
    if bias is None:
        return A.chain(case, data)
    rows = case.g * case.tq
    qk = A.qk_case(case)
    qd = dict(a=data["q"], b=data["k"], scales=data["logit_scale"])
    lbytes = (bmm_witness if witness else bmm_reference)(qk, qd, bias, bd)
    logits = A._full(case, lbytes).view(np.int8).reshape(rows, case.ldl)
    probs = np.full((rows, case.ldl), POISON, dtype=np.uint8)
    probs[:, :case.tk] = (H.witness_softmax if witness else H.reference_softmax)(logits, case.tk, data["table"], H.U8, case.prob_scale)
    o = (B.witness if witness else B.reference)(A.pv_case(case), dict(a=probs.reshape(-1), b=data["v"], scales=data["out_scales"]))
    return logits, probs, o


def attn_reference(case, data, bias, bd):
    return attn_chain(case, data, bias, bd)[2]


def attn_witness(case, data, bias, bd):
    return attn_chain(case, data, bias, bd, witness=True)[2]


# --- the plan of bias_plan.h, mirrored ---------------------------------------------------------------------------------------
INVALID, UNSUPPORTED = 1, 2
IMAGE_MAX_BYTES = 1 << 30


def up32(v):
    return -(-v // 32) * 32


def layout_dict(bias, m, n):
    s0, s1, ld = bias.layout(m, n)
    return dict(period0=bias.periods[0], period1=bias.periods[1], s0=s0, s1=s1, ld=ld)


def rows_of(d, b):
    return 1 if b["ld"] == 0 else d["m"]


def host_elems(d, b):
    return (b["period0"] - 1) * b["s0"] + (b["period1"] - 1) * b["s1"] + (rows_of(d, b) - 1) * b["ld"] + d["n"]


def image_elems(d, b):
    return b["period0"] * b["period1"] * rows_of(d, b) * up32(d["n"])


def validate(d, b):
    """0, INVALID or UNSUPPORTED for a layout (dict of dfx_logit_bias_desc's fields) against a valid descriptor, in the header's order"""
    if not 1 <= b["period0"] <= d["batch0"] or not 1 <= b["period1"] <= d["batch1"]:
        return INVALID
    if min(b["s0"], b["s1"], b["ld"]) < 0 or (b["ld"] != 0 and b["ld"] < d["n"]):
        return INVALID
    if host_elems(d, b) >= B.MAX_ELEMS:
        return INVALID
    if image_elems(d, b) * 4 > IMAGE_MAX_BYTES:
        return UNSUPPORTED
    return 0


def image_index(b, rows, cols, b0, b1, m, n):
    t = (b0 % b["period0"]) * b["period1"] + (b1 % b["period1"])
    return (t * rows + (0 if rows == 1 else m)) * cols + n


def image(d, b, table):
    """the device image {tables * rows, up32(n)} f32 of a host table: pads zero"""
    rows, cols = rows_of(d, b), up32(d["n"])
    img = np.zeros((b["period0"] * b["period1"] * rows, cols), dtype=np.float32)
    for p0 in range(b["period0"]):
        for p1 in range(b["period1"]):
            for m in range(rows):
                at = p0 * b["s0"] + p1 * b["s1"] + m * b["ld"]
                img[(p0 * b["period1"] + p1) * rows + m, :d["n"]] = table[at:at + d["n"]]
    return img


def scan(values):
    """(rc, max |finite entry|, has -inf) over the addressed entries"""
    v = np.asarray(values, dtype=np.float32)
    if np.isnan(v).any() or np.isposinf(v).any():
        return INVALID, 0.0, False
    fin = np.isfinite(v)
    return 0, float(np.abs(v[fin].astype(np.float64)).max()) if fin.any() else 0.0, bool(np.isneginf(v).any())


def distinct_bytes(d, b):
    return (1 if b["s0"] == 0 else b["period0"]) * (1 if b["s1"] == 0 else b["period1"]) * rows_of(d, b) * d["n"] * 4


def fast_ok_biased(d, scales, max_abs, has_ninf):
    if d["round_mode"] != 0 or has_ninf:
        return False
    bound = (255.0 if d["a_dt"] == U8 else 128.0) * 128.0 * d["k"]
    return all(np.isfinite(s) and (bound + max_abs) * abs(float(s)) <= 2.0 ** 30 for s in np.asarray(scales, dtype=np.float32))


def bmm_fast(case, data, bias, bd):
    """the route dfx_bmm proves for a case (the MFMA path), with or without a bias"""
    d = B.desc_of(case)
    if bias is None:
        return B.fast_ok(d, data["scales"])
    rc, mx, ninf = scan(bd["values"])
    assert rc == 0
    return fast_ok_biased(d, data["scales"], mx, ninf)


def attn_fast_logits(case, data, bias, bd):
    d = A.bmm_desc_logits(A.desc_of(case))
    if bias is None:
        return B.fast_ok(d, data["logit_scale"])
    rc, mx, ninf = scan(bd["values"])
    assert rc == 0
    return fast_ok_biased(d, data["logit_scale"], mx, ninf)


# --- case tables ------------------------------------------------------------------------------------------------------------
def bmm_tail_cases():
    """m 33, n 37, k 40 (every tail): NT and NN, A u8 / s8, all four dst types, C's leading dimension odd (41) and vector-
    aligned (48: c_vec): -> [(BmmCase, Bias)]; the bias's periods, layout and masks rotate"""
    out, i = [], 0
    for trans_b in (True, False):
        for a_dt in (U8, S8):
            for dst in B.DST_ROTATION:
                for c_ld in (41, 48):
                    per_channel = i % 4 == 3
                    # bmm_ref's per-channel scales run from 0.5 to 1.5 times the base: on a 1-byte dst the base is two thirds of the
                    # centred scale, so that the widest channel is the centred one and the case stays inside the 2 % regime
                    scale = 40.0 / ((147.0 if a_dt == U8 else 74.0) * 74.0 * np.sqrt(40.0)) / 1.5 if per_channel and dst in (S8, U8) else None
                    case = B.BmmCase("bias", 33, 37, 40, trans_b=trans_b, a_dt=a_dt, dst_dt=dst, batch=(2, 3), c_ld=c_ld, relu=i % 5 == 1, rm=(i // 3) % 2,
                                     per_channel=per_channel, scale=scale, seed=70000 + i)
                    periods = ((1, 1), (1, 3), (2, 1), (2, 3))[i % 4]
                    # masks on the 1-byte dsts only (a 4-byte dst shows the finite mask value itself, which is fine, but -inf on
                    # f32 with a NaN product would pin NaN bit patterns): every third case masks at random with the finite value
                    mask = "random" if dst in (S8, U8) and i % 3 == 0 else None
                    out.append((case, Bias(periods=periods, one_row=i % 7 == 6, mask=mask, seed=71000 + i)))
                    i += 1
    return out


def bmm_layout_cases():
    """batch (2,3) with every period pair, dense and with one row; host strides with gaps; n = 1 and m = 1; -inf on s8 / u8 / s32"""
    out = []
    base = dict(trans_b=True, a_dt=S8, dst_dt=S8, batch=(2, 3))
    for i, periods in enumerate(((1, 1), (1, 3), (2, 1), (2, 3))):
        for one_row in (False, True):
            out.append((B.BmmCase("periods", 33, 37, 40, seed=72000 + 2 * i + one_row, **base), Bias(periods=periods, one_row=one_row, seed=72100 + 2 * i + one_row)))
    # host strides with gaps: rows 41 apart, tables 1500 apart, table groups 5000 apart; and overlapping one-row tables 1 apart
    out.append((B.BmmCase("gaps", 33, 37, 40, seed=72200, **base), Bias(periods=(2, 3), strides=(5000, 1500, 41), seed=72201)))
    out.append((B.BmmCase("gaps-row", 33, 37, 40, seed=72202, **dict(base, a_dt=U8)), Bias(periods=(2, 3), one_row=True, strides=(200, 50, 0), seed=72203)))
    out.append((B.BmmCase("shared", 33, 37, 40, seed=72204, **base), Bias(periods=(2, 3), strides=(0, 33 * 37, 37), seed=72205)))   # s0 = 0: period0 shares
    for trans_b in (True, False):
        out.append((B.BmmCase("n1", 33, 1, 40, trans_b=trans_b, a_dt=S8, dst_dt=S8, batch=(2, 3), seed=72300 + trans_b), Bias(periods=(2, 3), seed=72310 + trans_b)))
        out.append((B.BmmCase("m1", 1, 37, 40, trans_b=trans_b, a_dt=U8, dst_dt=S32, batch=(2, 3), seed=72320 + trans_b), Bias(periods=(1, 3), seed=72330 + trans_b)))
    for j, (dst, a_dt) in enumerate(((S8, S8), (U8, U8), (S32, S8))):
        out.append((B.BmmCase("ninf", 33, 37, 40, trans_b=j != 1, a_dt=a_dt, dst_dt=dst, batch=(2, 3), seed=72400 + j),
                    Bias(periods=(2, 1), mask="random", mask_value="ninf", seed=72410 + j)))
    # several units per workgroup column: 70 x 130 gives 3 x 5 tiles per matrix
    out.append((B.BmmCase("tiles", 70, 130, 96, trans_b=True, a_dt=U8, dst_dt=S8, batch=(1, 2), seed=72500), Bias(periods=(1, 2), mask="causal", seed=72501)))
    out.append((B.BmmCase("tiles", 70, 130, 96, trans_b=False, a_dt=S8, dst_dt=U8, batch=(1, 2), seed=72502), Bias(periods=(1, 1), seed=72503)))
    return out


SWIN = A.AttnCase("swin", 49, 49, 32, 32, q_dt=S8, dst_dt=S8, batch=(4, 3), o_ld=32, seed=73000)
TAILS = A.AttnCase("tails", 33, 70, 40, 24, q_dt=U8, dst_dt=S8, batch=(1, 2), seed=73001)
KEYPAD = A.AttnCase("keypad", 40, 197, 64, 64, q_dt=S8, dst_dt=S8, batch=(1, 2), o_ld=64, seed=73002)
CAUSAL = A.AttnCase("causal", 40, 40, 32, 32, q_dt=S8, dst_dt=U8, batch=(1, 2), seed=73003)


def attn_cases():
    """-> [(AttnCase, Bias)]: Swin with its shifted-window mask (periods (2,3): two masks, three heads); tails with split keys and a
    random mask; a key-padding row at tk 197; a causal 40 x 40"""
    return [(SWIN, Bias(periods=(2, 3), mask="window", seed=73100)),
            (TAILS, Bias(periods=(1, 2), mask="random", seed=73101)),
            (KEYPAD, Bias(periods=(1, 1), one_row=True, mask="keypad", seed=73102)),
            (CAUSAL, Bias(periods=(1, 1), mask="causal", seed=73103))]


FULL_ROW = (A.AttnCase("fullrow", 33, 70, 32, 33, q_dt=S8, dst_dt=S8, batch=(1, 2), seed=73200), Bias(periods=(1, 2), mask="row0", seed=73201))
GRID_CAP = (A.AttnCase("cap", 65, 70, 32, 33, q_dt=U8, dst_dt=S8, batch=(2, 2), seed=73300), Bias(periods=(2, 2), mask="random", seed=73301))
OFFSET = (A.AttnCase("off", 33, 40, 50, 36, q_dt=U8, dst_dt=S8, o_ld=48, seed=73400), Bias(periods=(1, 1), mask="causal", seed=73401))
STREAMS = (A.AttnCase("streams", 130, 130, 64, 64, q_dt=S8, dst_dt=S8, batch=(2, 3), o_ld=64, seed=73500), Bias(periods=(1, 3), mask="random", seed=73501))
AUTO = (A.AttnCase("auto", 49, 49, 32, 32, q_dt=S8, dst_dt=S8, batch=(64, 3), o_ld=32, seed=73600), Bias(periods=(64, 3), mask="window", seed=73601))


def cxx_cases():
    """what tools/attn_bias_check runs through the C++ overloads: (AttnCase, Bias) for attention(), (BmmCase, Bias) for matmul()"""
    return [(A.AttnCase("cxx", 33, 70, 40, 35, q_dt=S8, dst_dt=S8, batch=(2, 2), seed=74000), Bias(periods=(2, 2), mask="random", seed=74001))], \
        [(B.BmmCase("cxx", 33, 37, 40, trans_b=True, a_dt=U8, dst_dt=S8, batch=(2, 3), seed=74002), Bias(periods=(1, 3), one_row=True, seed=74003))]


def attn_table():
    """every attention case of the GPU tests"""
    return attn_cases() + [FULL_ROW, GRID_CAP, OFFSET, STREAMS, AUTO] + cxx_cases()[0]


def bmm_table():
    return bmm_tail_cases() + bmm_layout_cases() + cxx_cases()[1]


def with_ninf(bias):
    return replace(bias, mask_value="ninf")
