"""Reference, data, case tables and plan mirror of the fused int8 attention's tests (pure numpy, needs no GPU).

The op (include/dfx.h, dfx_attn_*) is DEFINED as dfx_bmm (NT, -> s8 logits) -> dfx_head's table softmax (-> u8) -> dfx_bmm (NN),
so the reference is nothing but bmm_ref.reference -> head_ref.reference_softmax -> bmm_ref.reference, chained over whole STORAGE
arrays: the logits and the probabilities live in {G, tq, up16(tk)} arrays whose pad holds poison, and O's whole storage is
poisoned before the valid elements are scattered into it, so a comparison of the whole storage also shows that elements
dv .. ldo-1 of every row, and everything between the matrices, are not written.  tests/test_attn_cpu.py pins it against the
chained pure-Python witnesses of the two ops.
"""
from dataclasses import dataclass, replace

import numpy as np

import bmm_ref as B
import head_ref as H

F32, S32, S8, U8 = B.F32, B.S32, B.S8, B.U8
NP_OF, NAME_OF, SIZE_OF = B.NP_OF, B.NAME_OF, B.SIZE_OF
FUSED, CHAIN = 0, 1             # DFX_ATTN_FUSED / DFX_ATTN_CHAIN
POISON = B.POISON
DST_ROTATION = B.DST_ROTATION
up16 = B.up16


@dataclass(frozen=True)
class AttnCase:
    name: str
    tq: int
    tk: int
    d: int
    dv: int
    q_dt: int = S8
    dst_dt: int = S8
    batch: tuple = (1, 1)
    relu: bool = False
    rm: int = 0
    per_channel: bool = False
    q_strides: tuple = None       # (s0, s1, ld) in elements; None: matrices packed one behind the other, ld = up16(cols)
    k_strides: tuple = None
    v_strides: tuple = None
    o_strides: tuple = None       # None: ld = dv + 3 (odd rows, never vector-aligned) unless o_ld is given
    o_ld: int = None
    logit_scale: float = None     # None: centred, standard deviation about 40 (bmm_ref.make_scales)
    out_scale: float = None       # None: 1 / 256 (s8), 1 / 128 (u8), 0.37 (4-byte dst)
    table_step: float = 0.0625
    prob_scale: float = 255.0
    saturating: bool = False      # built to saturate: exempt from the regime checks of test_attn_cpu
    seed: int = 1

    @property
    def g(self):
        return self.batch[0] * self.batch[1]

    @property
    def ldl(self):
        return up16(self.tk)

    def strides(self, which):
        given = {"q": self.q_strides, "k": self.k_strides, "v": self.v_strides, "o": self.o_strides}[which]
        if given is not None:
            return tuple(int(v) for v in given)
        rows, cols = {"q": (self.tq, self.d), "k": (self.tk, self.d), "v": (self.tk, self.dv), "o": (self.tq, self.dv)}[which]
        ld = (self.o_ld or self.dv + 3) if which == "o" else up16(cols)
        return self.batch[1] * rows * ld, rows * ld, ld

    @property
    def l_strides(self):
        return self.batch[1] * self.tq * self.ldl, self.tq * self.ldl, self.ldl

    def ident(self):
        return "%s-%dx%d-tq%d-tk%d-d%d-dv%d-%s-%s-r%d-m%d-pc%d" % (
            self.name, self.batch[0], self.batch[1], self.tq, self.tk, self.d, self.dv, NAME_OF[self.q_dt], NAME_OF[self.dst_dt], self.relu,
            self.rm, self.per_channel)


def qk_case(case):
    """the dfx_bmm that gives the logits"""
    return B.BmmCase(case.name + "-qk", case.tq, case.tk, case.d, trans_b=True, a_dt=case.q_dt, dst_dt=S8, batch=case.batch,
                     rm=case.rm, a_strides=case.strides("q"), b_strides=case.strides("k"), c_strides=case.l_strides, scale=case.logit_scale,
                     seed=case.seed)


def pv_case(case):
    """the dfx_bmm that gives the context"""
    scale = case.out_scale
    if scale is None and case.dst_dt in (S8, U8):
        scale = 1.0 / 256.0 if case.dst_dt == S8 else 1.0 / 128.0      # the row sum of P is about 255: |acc| <= about 255 * 128
    return B.BmmCase(case.name + "-pv", case.tq, case.dv, case.tk, trans_b=False, a_dt=U8, dst_dt=case.dst_dt, batch=case.batch, relu=case.relu,
                     rm=case.rm, per_channel=case.per_channel, a_strides=case.l_strides, b_strides=case.strides("v"),
                     c_strides=case.strides("o"), scale=scale, seed=case.seed + 7919)


def make_table(case):
    return H.softmax_table(case.table_step, case.tk)


def generate(case):
    """-> dict(q, k, v: flat storage arrays; logit_scale (1,), out_scales, table).  bmm_ref.generate's data: valid elements
    uniform over the dtype, Q's pad 0xFF, K's and V's pads random non-zero bytes."""
    qk = B.generate(qk_case(case))
    pvc = pv_case(case)
    pv = B.generate(pvc)
    v = pv["b"]
    if case.relu or case.dst_dt == U8:
        # a softmax row weighs a few keys only, so a column of V of positive sum can still leave nothing but the ReLU's zeros
        # (all of O where dv = 1): the even columns of V are made non-negative
        idx = B.index(pvc, "b")                                            # {b0, b1, tk, dv}
        vv = v[idx].astype(np.int16)
        vv[..., ::2] = np.minimum(np.abs(vv[..., ::2]), 127)
        v[idx.reshape(-1)] = vv.astype(np.int8).reshape(-1)
    out_scales = pv["scales"][:1]
    if case.per_channel:                                                   # (0.5 .. 1) x the centred scale: none above it
        out_scales = (out_scales[0] * (0.5 + 0.5 * np.arange(case.dv) / case.dv)).astype(np.float32)
    return dict(q=qk["a"], k=qk["b"], v=v, logit_scale=qk["scales"], out_scales=out_scales, table=make_table(case))


def _full(case, bytes_):
    """a bmm_ref storage of L / P (which ends behind the last valid element) inside the whole {G, tq, ldl} array"""
    out = np.full(case.g * case.tq * case.ldl, POISON, dtype=np.uint8)
    out[:bytes_.size] = bytes_
    return out


def chain(case, data):
    """-> (logits {G*tq, ldl} int8 with poison pad, probabilities {G*tq, ldl} uint8 with poison pad, O's whole storage as bytes)"""
    rows = case.g * case.tq
    logits = _full(case, B.reference(qk_case(case), dict(a=data["q"], b=data["k"], scales=data["logit_scale"]))).view(np.int8).reshape(rows, case.ldl)
    probs = np.full((rows, case.ldl), POISON, dtype=np.uint8)
    probs[:, :case.tk] = H.reference_softmax(logits, case.tk, data["table"], H.U8, case.prob_scale)
    o = B.reference(pv_case(case), dict(a=probs.reshape(-1), b=data["v"], scales=data["out_scales"]))
    return logits, probs, o


def reference(case, data):
    """O's whole storage as bytes: POISON everywhere but the valid elements"""
    return chain(case, data)[2]


def o_values(case, data, probs=None):
    """the valid elements of O, {batch0, batch1, tq, dv}"""
    probs = chain(case, data)[1] if probs is None else probs
    return B.values(pv_case(case), dict(a=probs.reshape(-1), b=data["v"], scales=data["out_scales"]))


def witness(case, data):
    """the same storage through the element-by-element pure-Python witnesses of the two ops"""
    rows = case.g * case.tq
    logits = _full(case, B.witness(qk_case(case), dict(a=data["q"], b=data["k"], scales=data["logit_scale"]))).view(np.int8).reshape(rows, case.ldl)
    probs = np.full((rows, case.ldl), POISON, dtype=np.uint8)
    probs[:, :case.tk] = H.witness_softmax(logits, case.tk, data["table"], H.U8, case.prob_scale)
    return B.witness(pv_case(case), dict(a=probs.reshape(-1), b=data["v"], scales=data["out_scales"]))


def storage_elems(case, which):
    if which == "o":
        return B.storage_elems(pv_case(case), "c")
    return B.storage_elems(qk_case(case), {"q": "a", "k": "b"}[which]) if which in "qk" else B.storage_elems(pv_case(case), "b")


def o_index(case):
    return B.index(pv_case(case), "c")


# --- the plan of attn_plan.h, mirrored --------------------------------------------------------------------------------------
INVALID, UNSUPPORTED = 1, 2
MAX_ELEMS = 1 << 40
THREADS, WAVES, STRIP, D_MAX, TK_MAX, GRID_PER_CU, LDS_MAX = 256, 4, 32, 256, 4096, 8, 160 * 1024
V_LDS = B.NN_LDS
TABLE_BYTES = 1024
TK_LIMIT = B.KMAX                # tk is the context product's K (dfx_head's c alone would admit 65535)
FIELDS = ("batch0", "batch1", "tq", "tk", "d", "dv", "q_dt", "k_dt", "v_dt", "dst_dt", "relu", "round_mode", "nscales", "force_path",
          "prob_scale", "reserved", "q_s0", "q_s1", "ldq", "k_s0", "k_s1", "ldk", "v_s0", "v_s1", "ldv", "o_s0", "o_s1", "ldo")


def desc_of(case, force_path=-1):
    """the dict of dfx_attn_desc's fields of a case"""
    q, k, v, o = (case.strides(w) for w in "qkvo")
    return dict(batch0=case.batch[0], batch1=case.batch[1], tq=case.tq, tk=case.tk, d=case.d, dv=case.dv, q_dt=case.q_dt, k_dt=S8, v_dt=S8,
                dst_dt=case.dst_dt, relu=int(case.relu), round_mode=case.rm, nscales=case.dv if case.per_channel else 1, force_path=force_path,
                prob_scale=float(case.prob_scale), reserved=0, q_s0=q[0], q_s1=q[1], ldq=q[2], k_s0=k[0], k_s1=k[1], ldk=k[2],
                v_s0=v[0], v_s1=v[1], ldv=v[2], o_s0=o[0], o_s1=o[1], ldo=o[2])


def lds_bytes(d):
    return TABLE_BYTES + STRIP * (up16(d["tk"]) + 16) + V_LDS


def fused_class(d):
    return d["k_dt"] == S8 and d["v_dt"] == S8 and all(d[k] % 16 == 0 for k in ("ldq", "ldk", "ldv", "q_s0", "q_s1", "k_s0", "k_s1", "v_s0", "v_s1")) \
        and d["d"] <= D_MAX and d["tk"] <= TK_MAX and lds_bytes(d) <= LDS_MAX


def validate(d):
    """0, INVALID or UNSUPPORTED for a descriptor given as a dict of dfx_attn_desc's fields, in the header's order"""
    if min(d["batch0"], d["batch1"], d["tq"], d["tk"], d["d"], d["dv"]) < 1 or max(d["tq"], d["dv"]) > B.MN_MAX or d["d"] > B.KMAX:
        return INVALID
    if d["tk"] > TK_LIMIT:
        return INVALID
    if d["q_dt"] not in (U8, S8) or d["k_dt"] not in (U8, S8) or d["v_dt"] not in (U8, S8) or d["dst_dt"] not in NP_OF:
        return INVALID
    if d["round_mode"] not in (0, 1) or d["nscales"] not in (1, d["dv"]) or d["force_path"] not in (-1, FUSED, CHAIN):
        return INVALID
    if not np.isfinite(np.float32(d["prob_scale"])):
        return INVALID
    if d["ldq"] < d["d"] or d["ldk"] < d["d"] or d["ldv"] < d["dv"] or d["ldo"] < d["dv"]:
        return INVALID
    if min(d[k] for k in ("q_s0", "q_s1", "k_s0", "k_s1", "v_s0", "v_s1", "o_s0", "o_s1")) < 0:
        return INVALID
    if not B.c_disjoint(d["dv"], d["tq"], d["batch1"], d["batch0"], d["ldo"], d["o_s1"], d["o_s0"]):
        return INVALID
    b0, b1 = d["batch0"], d["batch1"]
    if max(B.span(b0, b1, d["q_s0"], d["q_s1"], d["ldq"], d["tq"], d["d"]), B.span(b0, b1, d["k_s0"], d["k_s1"], d["ldk"], d["tk"], d["d"]),
           B.span(b0, b1, d["v_s0"], d["v_s1"], d["ldv"], d["tk"], d["dv"]), B.span(b0, b1, d["o_s0"], d["o_s1"], d["ldo"], d["tq"], d["dv"])) >= MAX_ELEMS:
        return INVALID
    if b0 * b1 * d["tq"] * up16(d["tk"]) >= MAX_ELEMS:
        return INVALID
    if d["k_dt"] == U8 or d["v_dt"] == U8:
        return UNSUPPORTED
    if d["force_path"] == FUSED and not fused_class(d):
        return UNSUPPORTED
    return 0


AUTO_MIN_TQ, AUTO_MIN_TK, AUTO_MAX_TK, AUTO_MIN_D, AUTO_MAX_D, AUTO_MIN_STRIPS = 49, 49, 850, 32, 64, 384


def auto_path(d):
    """the AUTO RULE (DFX_ATTN_AUTO_NOTE): the fused kernel in its class inside the box of the points at which it was measured
    and won (tq >= 49, tk 49 .. 850, d and dv 32 .. 64, at least 384 strips); the chain everywhere else"""
    if d["force_path"] != -1:
        return d["force_path"]
    box = d["tq"] >= AUTO_MIN_TQ and AUTO_MIN_TK <= d["tk"] <= AUTO_MAX_TK and AUTO_MIN_D <= d["d"] <= AUTO_MAX_D and \
        AUTO_MIN_D <= d["dv"] <= AUTO_MAX_D and strips(d) >= AUTO_MIN_STRIPS
    return FUSED if box and fused_class(d) else CHAIN


def strips(d):
    return d["batch0"] * d["batch1"] * -(-d["tq"] // STRIP)


def kparts(d):
    t = -(-d["dv"] // 32)
    return 1 if t >= WAVES else WAVES // t


def planned_grid(d, cus, cap=0):
    blocks = min(strips(d), max(1, cus) * GRID_PER_CU)
    if cap > 0:
        blocks = min(blocks, cap)
    return max(1, blocks)


def bmm_desc_logits(d):
    ldl = up16(d["tk"])
    return dict(batch0=d["batch0"], batch1=d["batch1"], m=d["tq"], n=d["tk"], k=d["d"], trans_b=1, a_dt=d["q_dt"], b_dt=d["k_dt"], dst_dt=S8,
                relu=0, round_mode=d["round_mode"], nscales=1, force_path=-1, a_s0=d["q_s0"], a_s1=d["q_s1"], lda=d["ldq"], b_s0=d["k_s0"],
                b_s1=d["k_s1"], ldb=d["ldk"], c_s0=d["batch1"] * d["tq"] * ldl, c_s1=d["tq"] * ldl, ldc=ldl)


def bmm_desc_context(d):
    ldl = up16(d["tk"])
    return dict(batch0=d["batch0"], batch1=d["batch1"], m=d["tq"], n=d["dv"], k=d["tk"], trans_b=0, a_dt=U8, b_dt=d["v_dt"], dst_dt=d["dst_dt"],
                relu=d["relu"], round_mode=d["round_mode"], nscales=d["nscales"], force_path=-1, a_s0=d["batch1"] * d["tq"] * ldl,
                a_s1=d["tq"] * ldl, lda=ldl, b_s0=d["v_s0"], b_s1=d["v_s1"], ldb=d["ldv"], c_s0=d["o_s0"], c_s1=d["o_s1"], ldc=d["ldo"])


def fast_logits(d, logit_scale):
    """128 * 128 * d (s8 Q) or 255 * 128 * d (u8 Q) against the logit scale"""
    return B.fast_ok(bmm_desc_logits(d), np.asarray(logit_scale, dtype=np.float32).reshape(-1))


def fast_context(d, out_scales):
    """255 * 128 * tk against the out scales"""
    return B.fast_ok(bmm_desc_context(d), out_scales)


def scratch_bytes(d):
    return 2 * d["batch0"] * d["batch1"] * d["tq"] * up16(d["tk"])


def algorithmic_ops(d):
    return 2 * d["batch0"] * d["batch1"] * d["tq"] * d["tk"] * (d["d"] + d["dv"])


def algorithmic_bytes(d):
    def g(s0, s1):
        return (1 if d[s0] == 0 else d["batch0"]) * (1 if d[s1] == 0 else d["batch1"])
    return g("q_s0", "q_s1") * d["tq"] * d["d"] + g("k_s0", "k_s1") * d["tk"] * d["d"] + g("v_s0", "v_s1") * d["tk"] * d["dv"] + \
        d["batch0"] * d["batch1"] * d["tq"] * d["dv"] * SIZE_OF[d["dst_dt"]]


def kernel_name(case, path, route_l, route_o):
    return "%s<%s,%s> %s/%s" % ("attn_fused" if path == FUSED else "attn_chain", NAME_OF[case.q_dt], NAME_OF[case.dst_dt],
                                "fast" if route_l else "exact", "fast" if route_o else "exact")


# --- case tables ------------------------------------------------------------------------------------------------------------
AX_TQ = (1, 31, 32, 33, 65)
AX_TK = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130, 200)
AX_D = (1, 16, 17, 32, 33, 64, 96, 256)
AX_DV = (1, 31, 32, 33, 64, 130)
AXES = (AX_TQ, AX_TK, AX_D, AX_DV)


def covering_shapes():
    """(tq, tk, d, dv) tuples in which every value of an axis meets at least two values of each other axis: for every pair of
    axes the longer one is walked three times against the shorter one at three different offsets, the two other axes
    rotating; duplicates dropped.  test_attn_cpu checks the covering property itself."""
    out = []
    step = 0
    for i in range(4):
        for j in range(i + 1, 4):
            a, b = AXES[i], AXES[j]
            n = max(len(a), len(b))
            for off in (0, 1, 3):
                for t in range(n):
                    shape = [None] * 4
                    shape[i] = a[t % len(a)]
                    shape[j] = b[(t + off + (t // len(b) if len(b) < len(a) else t // len(a))) % len(b)]
                    for r in range(4):
                        if shape[r] is None:
                            shape[r] = AXES[r][(step * (r + 2) + off) % len(AXES[r])]
                    step += 1
                    out.append(tuple(shape))
    seen, uniq = set(), []
    for s in out:
        if s not in seen:
            seen.add(s)
            uniq.append(s)
    return uniq


def shape_grid():
    """the covering table; Q's dtype, the dst dtype, relu, the round mode, per-channel scales and O's leading dimension (dv + 3:
    never aligned; up16(dv): vector stores) rotate through it"""
    out = []
    for i, (tq, tk, d, dv) in enumerate(covering_shapes()):
        out.append(AttnCase("grid", tq, tk, d, dv, q_dt=(S8, U8)[i % 2], dst_dt=DST_ROTATION[(i // 2) % 4], relu=(i // 8) % 3 == 1, rm=(i // 3) % 2,
                            per_channel=(i // 5) % 2 == 1, o_ld=up16(dv) if (i // 7) % 2 else None, seed=50000 + i))
    return out


HEADS, T, D, BS = 2, 37, 32, 2


def batch_cases():
    """(2,3) dense; (bs 2, heads 2, T 37, d 32) head-sliced with the context interleaved back into {bs, T, heads * d}; K and V
    broadcast over the heads / over everything"""
    hs = B.attention_strides(BS, HEADS, T, D)
    out = []
    for i, q_dt in enumerate((S8, U8)):
        out.append(AttnCase("dense", 33, 37, 40, 35, q_dt=q_dt, dst_dt=DST_ROTATION[i], batch=(2, 3), seed=51000 + i))
        for j, dst in enumerate(DST_ROTATION[2 * i:2 * i + 2]):
            out.append(AttnCase("heads", T, T, D, D, q_dt=q_dt, dst_dt=dst, batch=(BS, HEADS), q_strides=hs, k_strides=hs, v_strides=hs,
                                o_strides=hs, seed=51100 + 2 * i + j))
        out.append(AttnCase("bcast-heads", 33, 37, 40, 35, q_dt=q_dt, dst_dt=S8, batch=(2, 3), k_strides=(37 * 48, 0, 48), v_strides=(37 * 48, 0, 48),
                            seed=51200 + i))
        out.append(AttnCase("bcast-all", 33, 37, 40, 35, q_dt=q_dt, dst_dt=S32, batch=(2, 3), k_strides=(0, 0, 48), v_strides=(0, 0, 48),
                            per_channel=True, seed=51300 + i))
    return out


def _fill(case, data, which, vals):
    """data with the valid elements of q / k / v replaced ({tq|tk, cols} per matrix, broadcast over the batch)"""
    bc = qk_case(case) if which in "qk" else pv_case(case)
    idx = B.index(bc, {"q": "a", "k": "b", "v": "b"}[which])
    arr = data[which].copy()
    arr[idx.reshape(-1)] = np.broadcast_to(np.asarray(vals, dtype=arr.dtype), idx.shape).reshape(-1)
    return dict(data, **{which: arr})


def softmax_edge_cases():
    """-> [(case, data)]: a row of equal logits (S = tk * E[0]); logits on both saturation bounds (distance 255); a table with
    E[255] = 0; tk = 1 (P = 255) against all -128 / all 127 V with s32 out and scale 1: the compensation's extreme"""
    out = []
    # equal logits: Q = 0 -> every logit 0
    case = AttnCase("equal", 33, 70, 32, 33, q_dt=S8, dst_dt=S8, seed=52000)
    out.append((case, _fill(case, generate(case), "q", 0)))
    # both bounds in every row: Q = 127 everywhere, K rows alternately all 127 and all -128, logit scale 1: +-(127 * 127 * 32)
    case = AttnCase("bounds", 33, 70, 32, 33, q_dt=S8, dst_dt=S8, logit_scale=1.0, saturating=True, seed=52001)
    data = _fill(case, generate(case), "q", 127)
    krows = np.where(np.arange(70)[:, None] % 2 == 0, 127, -128) * np.ones((1, 32), dtype=np.int64)
    out.append((case, _fill(case, data, "k", krows)))
    # the same with a table whose far end is 0
    case = replace(case, name="bounds-e255", table_step=0.25)
    d2 = dict(out[-1][1], table=make_table(case))
    assert d2["table"][255] == 0 and d2["table"][0] > 0
    out.append((case, d2))
    # tk = 1: P = 255 whatever the logit is
    for fill in (-128, 127):
        for q_dt in (S8, U8):
            case = AttnCase("tk1-v%d" % fill, 33, 1, 17, 33, q_dt=q_dt, dst_dt=S32, out_scale=1.0, seed=52100)
            out.append((case, _fill(case, generate(case), "v", fill)))
    return out


def tie_cases():
    """-> [(case, data)]: out scale 0.5 with every context accumulator odd (tk = 1 and prob_scale 1: P = 1, V odd), logit scale 0.5 with odd
    logit accumulators (Q = 1 in column 0, K odd there); both round modes; u8 / s8 / s32 dst"""
    out = []
    for rm in (0, 1):
        for dst in (U8, S8, S32):
            case = AttnCase("ties", 33, 1, 17, 40, q_dt=U8, dst_dt=dst, rm=rm, logit_scale=0.5, out_scale=0.5, prob_scale=1.0, seed=53000)
            data = generate(case)
            qv = np.zeros((33, 17), dtype=np.uint8)
            qv[:, 0] = 1
            data = _fill(case, data, "q", qv)
            v = np.random.default_rng(53001).integers(-128, 128, (1, 40)).astype(np.int8) | 1
            out.append((case, _fill(case, data, "v", v)))
        # ties in the logits: tk 40 keys, odd accumulators times 0.5
        case = AttnCase("ties-logits", 33, 40, 17, 33, q_dt=U8, dst_dt=S8, rm=rm, logit_scale=0.5, seed=53100)
        data = generate(case)
        qv = np.zeros((33, 17), dtype=np.uint8)
        qv[:, 0] = 1
        data = _fill(case, data, "q", qv)
        kv = np.random.default_rng(53101).integers(-100, 100, (40, 17)).astype(np.int8)
        kv[:, 0] |= 1
        out.append((case, _fill(case, data, "k", kv)))
    return out


def nonfinite_cases():
    """logit / out scales of inf and NaN: neither route may be called fast; built to saturate"""
    out = []
    for i, (ls, os_) in enumerate(((float("inf"), None), (float("nan"), None), (None, float("inf")), (None, float("nan")))):
        out.append(AttnCase("nonfinite", 33, 34, 40, 33, q_dt=(S8, U8)[i % 2], dst_dt=DST_ROTATION[i], logit_scale=ls, out_scale=os_,
                            saturating=True, seed=54000 + i))
    return out


CLASS_BOUND_CASE = AttnCase("tkmax", 33, TK_MAX, 16, 32, q_dt=S8, dst_dt=S8, o_ld=32, seed=55000)
GRID_CAP_CASE = AttnCase("cap", 65, 70, 32, 33, q_dt=U8, dst_dt=S8, batch=(2, 2), seed=56000)          # 4 matrices of 3 strips
REGIME_SHAPES = ((31, 15, 17, 31), (33, 17, 33, 33), (65, 65, 64, 64), (33, 200, 96, 130), (5, 130, 256, 64), (33, 4096, 16, 32), (64, 1024, 64, 64))


def auto_cases():
    """-> [(case, planned path)]: the auto rule at both sides of each of its bounds, on the Swin stage's 64 x 3 windows"""
    def c(i, path, **kw):
        a = dict(tq=49, tk=49, d=32, dv=32, batch=(64, 3))
        a.update(kw)
        return AttnCase("auto", a["tq"], a["tk"], a["d"], a["dv"], q_dt=(S8, U8)[i % 2], dst_dt=S8, batch=a["batch"], o_ld=up16(a["dv"]),
                        q_strides=a.get("q_strides"), seed=57000 + i), path
    return [c(0, FUSED), c(1, CHAIN, tq=48), c(2, CHAIN, tk=48), c(3, CHAIN, d=31), c(4, CHAIN, dv=31), c(5, CHAIN, batch=(63, 3)),
            c(6, FUSED, tk=850, d=64, dv=64), c(7, CHAIN, tk=851), c(8, CHAIN, d=65), c(9, CHAIN, dv=65),
            c(10, CHAIN, q_strides=(3 * 49 * 40, 49 * 40, 40))]                  # outside the class: ldq 40


OFFSET_CASE = AttnCase("off", 33, 40, 50, 36, q_dt=U8, dst_dt=S8, o_ld=48, seed=57100)                 # the per-submit fallback
STATE_CASE = AttnCase("state", 33, 40, 50, 36, q_dt=U8, dst_dt=S32, o_ld=36, seed=57200)               # submit checks
STREAMS_CASE = AttnCase("streams", 130, 130, 64, 64, q_dt=S8, dst_dt=S8, batch=(2, 3), o_ld=64, seed=57300)


def three_ops_case(q_dt):
    """the head-sliced block the GPU test also runs as dfa.MatMul -> dfa.Softmax -> dfa.MatMul"""
    hs = B.attention_strides(BS, HEADS, T, D)
    return AttnCase("three", T, T, D, D, q_dt=q_dt, dst_dt=S8, batch=(BS, HEADS), q_strides=hs, k_strides=hs, v_strides=hs, o_strides=hs, seed=57400)


def cxx_cases():
    """what tools/attn_check runs through deepfusion::attention(): the head-sliced block and a ragged dense shape"""
    hs = B.attention_strides(BS, HEADS, T, D)
    return [AttnCase("heads", T, T, D, D, q_dt=S8, dst_dt=S8, batch=(BS, HEADS), q_strides=hs, k_strides=hs, v_strides=hs, o_strides=hs, seed=58000),
            AttnCase("ragged", 33, 70, 40, 35, q_dt=U8, dst_dt=S32, batch=(1, 2), per_channel=True, rm=1, seed=58001)]


def single_cases():
    """the cases the GPU tests use one by one; test_attn_cpu holds them to the regimes like the tables"""
    return [OFFSET_CASE, STATE_CASE, STREAMS_CASE, three_ops_case(S8), three_ops_case(U8)] + cxx_cases()


def table():
    """every case of the tables whose data comes from generate(): what test_attn_cpu holds to the regimes"""
    return shape_grid() + batch_cases() + nonfinite_cases() + [CLASS_BOUND_CASE, GRID_CAP_CASE] + [c for c, _ in auto_cases()]
