"""tests/golden/conv_weights.json: what dfx_conv_set_weights made of generated inputs, recorded on an MI355X from the commit
before the weight packing and the requant proofs moved into csrc/conv_weights.h (the library was built with a recording
patch that appended, at the end of dfx_conv_set_weights, the line tools/conv_weights_check prints: routes, roles, block,
region sizes, a 64-bit hash of each host buffer just before upload, the kernel's name).

"cases": [name, name of the case of conv_plans.json the desc comes from, the 25 descriptor integers, KEY=VALUE switches,
workgroups per CU, the recipe, the recorded line, tag].  The desc is the plan golden's but for the six fields planning
never reads (bias dtypes, round modes, scale counts).  Weights are not stored: the recipe generates them, here
(generate) as in the tool -- its header documents the recipe and the integer generator.  tag: "" or
  "<predicate>:<bound>:<stage>:pass" / ":fail"   the two cases of a pair straddle one bound of one named proof of
                                             conv_weights.h: every other proof of the stage holds alike in both
  "gpu" / "gpu+submit"                       tests/test_gpu_conv_weights.py takes the case
This module also ports the six proofs (proofs()), in their mathematical form over a channel's P and N, so that the CPU
test can say WHICH proof decides a recorded route.

Reachability of the bounds, with lo = -(128 P + 127 N), hi = 127 P + 128 N the raw accumulator's range: magic1's
hi <= MAGIC1_HI can never decide alone: lo >= MAGIC1_LO gives 127 (P + N) <= 0x22F983, so hi <= 128 (P + N) < 2.4e6, far
below MAGIC1_HI = 6.1e6; the golden holds a case beyond MAGIC1_HI (it fails both).  Stage 1 of the resident kernels has
K = oc <= 64 taps (P, N <= 8192): its P / N bounds are met through the bias; MAGIC1_LO is met on an unfused resident op
(K = 288) and on the direct kernel's 1x1 stage (K = 256)."""
import json
import os

import numpy as np

UNDEF, F32, S32, S8, U8 = 0, 1, 2, 3, 4
DESC_FIELDS = ("bs ic ih iw oc oh ow kh kw sh sw pad_t pad_l oc1x1 dst_dt bia0_dt bia1_dt conv0_relu conv1_relu conv0_round_mode "
               "conv1_round_mode conv0_nscales conv1_nscales force_variant fuse_pool").split()
FREE_FIELDS = ("bia0_dt", "bia1_dt", "conv0_round_mode", "conv1_round_mode", "conv0_nscales", "conv1_nscales")  # planning never reads them
MAGIC1_LO, MAGIC1_HI = -0x22F983, 0x7FFFFF - 0x22F983
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_weights.json")


def load():
    with open(PATH) as f:
        g = json.load(f)
    g["cases"] = [dict(name=n, origin=o, desc=[int(v) for v in d.split()], tuning=dict(kv.split("=", 1) for kv in t.split()), per_cu=w,
                       recipe=dict(kv.split("=", 1) for kv in r.split()), line=ln, tag=tag) for n, o, d, t, w, r, ln, tag in g["cases"]]
    return g


def tool_line(c, ncu, extra=""):
    """the case as one input line of tools/conv_weights_check"""
    return " ".join([str(v) for v in c["desc"]] + [str(ncu), str(c["per_cu"])] + ["%s=%s" % kv for kv in c["tuning"].items()] +
                    ["%s=%s" % kv for kv in c["recipe"].items()] + ([extra] if extra else [])) + "\n"


def fields(line):
    """a recorded line as a dict: routes (r0, r1), roles, block, w0, w1, cst (ints), h0, h1, hc (hex strings), name"""
    head, name = line.split(" name=", 1)
    f = dict(kv.split("=", 1) for kv in head.split(" "))
    out = {k: int(f[k]) for k in ("roles", "block", "w0", "w1", "cst")}
    out.update(routes=tuple(int(v) for v in f["routes"].split(",")), h0=f["h0"], h1=f["h1"], hc=f["hc"], name=name)
    return out


# ---- the generator (tools/conv_weights_check.cc documents it) ----
_M = np.uint64


def _mix(z):
    z = z ^ (z >> _M(30))
    z = z * _M(0xBF58476D1CE4E5B9)
    z = z ^ (z >> _M(27))
    z = z * _M(0x94D049BB133111EB)
    return z ^ (z >> _M(31))


def _rnd(seed, s, k):
    with np.errstate(over="ignore"):
        return _mix((k.astype(np.uint64) + _M(1)) * _M(0x9E3779B97F4A7C15) + _M(seed) * _M(0xD1B54A32D192ED03) + _M(s))


def _f32(bits):
    return np.array([int(bits, 16)], dtype=np.uint32).view(np.float32)[0]


def _stage(recipe, s, nch, K, nscales, bia_dt):
    S = str(s)
    seed, R = int(recipe.get("@seed", 1)), int(recipe.get("@r" + S, 3))
    P, N, only = int(recipe.get("@p" + S, -1)), int(recipe.get("@n" + S, -1)), int(recipe.get("@c" + S, -1))
    with np.errstate(over="ignore"):
        w = ((_rnd(seed, s, np.arange(nch * K)) >> _M(32)) % _M(2 * R + 1)).astype(np.int64) - R
    w = w.reshape(nch, K)
    if P >= 0 or N >= 0:
        p, n = max(P, 0), max(N, 0)
        run = [127] * (p // 127) + ([p % 127] if p % 127 else []) + [-128] * (n // 128) + ([-(n % 128)] if n % 128 else [])
        assert len(run) <= K, "the recipe's P / N do not fit %d taps" % K
        for c in range(nch):
            if only < 0 or only == c:
                w[c] = 0
                w[c, (5 * c + np.arange(len(run))) % K] = run
    sc = _f32(recipe.get("@s" + S, "3B800000"))
    scales = np.full(nch if nscales > 1 else 1, sc, dtype=np.float32)
    if "@t" + S in recipe:
        scales[1::2] = _f32(recipe["@t" + S])
    B = int(recipe.get("@b" + S, 0))
    if bia_dt == UNDEF:
        bia = None
    elif bia_dt == F32:
        bia = np.full(nch, np.float32(B) + _f32(recipe.get("@f" + S, "0")), dtype=np.float32)
    else:
        bia = np.full(nch, B & 0xFF if bia_dt in (S8, U8) else B, dtype=np.int64).astype({S32: np.int32, S8: np.uint8, U8: np.uint8}[bia_dt])
        if bia_dt == S8:
            bia = bia.view(np.int8)
    return w.astype(np.int8), scales, bia


def generate(desc, recipe):
    """-> dict(w0 oihw s8, w1 oihw s8 | None, scales0, scales1 | None, bia0, bia1) of a case's desc (25 ints) and recipe"""
    d = dict(zip(DESC_FIELDS, desc))
    w0, s0, b0 = _stage(recipe, 0, d["oc"], d["ic"] * d["kh"] * d["kw"], d["conv0_nscales"], d["bia0_dt"])
    out = dict(w0=w0.reshape(d["oc"], d["ic"], d["kh"], d["kw"]), scales0=s0, bia0=b0, w1=None, scales1=None, bia1=None)
    if d["oc1x1"]:
        w1, s1, b1 = _stage(recipe, 1, d["oc1x1"], d["oc"], d["conv1_nscales"], d["bia1_dt"])
        out.update(w1=w1.reshape(d["oc1x1"], d["oc"], 1, 1), scales1=s1, bia1=b1)
    return out


def blocked(w):
    """oihw -> the reference's blocked layout [o/16][i/16][kh][kw][(i%16)/4][o%16][i%4], flat (dfx_blocked_offset)"""
    O, I, KH, KW = w.shape
    return np.ascontiguousarray(w.reshape(O // 16, 16, I // 16, 4, 4, KH, KW).transpose(0, 2, 5, 6, 3, 1, 4)).reshape(-1)


def inputs_hash(data):
    """what the tool prints for @inputs=1"""
    parts = [blocked(data["w0"])] + ([blocked(data["w1"])] if data["w1"] is not None else []) + [data["scales0"]]
    parts += [data[k] for k in ("scales1", "bia0", "bia1") if data[k] is not None]
    b = np.concatenate([np.ascontiguousarray(p).view(np.uint8).reshape(-1) for p in parts]).astype(np.uint64)
    with np.errstate(over="ignore"):
        i = np.arange(b.size, dtype=np.uint64)
        return "%016x" % int(((b + _M(1)) * ((_M(2) * i + _M(1)) * _M(0x9E3779B97F4A7C15))).sum(dtype=np.uint64))


# ---- the six proofs of conv_weights.h, over every channel of a stage ----
def _pn(w):
    w = w.reshape(w.shape[0], -1).astype(np.int64)
    return np.where(w > 0, w, 0).sum(1), -np.where(w < 0, w, 0).sum(1)


def proofs(data, stage):
    """-> {proof: holds for every channel of the stage}"""
    w = data["w%d" % stage]
    P, N = _pn(w)
    n = w.shape[0]
    sc = np.broadcast_to(data["scales%d" % stage], (n,)) if data["scales%d" % stage].size == 1 else data["scales%d" % stage]
    bia = data["bia%d" % stage]
    out = dict(fast_magnitude=True, fast_fold=True, magic0=True, magic1=True, fma0=True, fma1=True)
    for c in range(n):
        p, q, s = int(P[c]), int(N[c]), float(sc[c])
        b = 0.0 if bia is None else float(np.float32(bia[c]))
        integer = b == np.floor(b)
        lo, hi, comp, amax = -(128 * p + 127 * q), 127 * p + 128 * q, 128 * (p - q), 255 * max(p, q)
        finite = bool(np.isfinite(b) and np.isfinite(s))
        mag = finite and (amax + abs(b)) * abs(s) * 1.0001 + 2.0 < 2147480000.0
        k = comp + b - 2 ** 23 - 0x22F983
        with np.errstate(over="ignore"):
            fin26 = bool(np.isfinite(np.float32(s) * np.float32(2.0 ** 26)))
            fin23 = bool(np.isfinite(np.float32(s) * np.float32(2.0 ** 23)))
            prod = k * s
            exact = bool(np.isfinite(prod)) and float(np.float32(prod)) == prod
        res = dict(
            fast_magnitude=mag,
            fast_fold=mag and integer and abs(comp + b) < 2 ** 24 and amax + abs(b) < 2 ** 24 and abs(comp) + amax < 2 ** 24,
            magic0=integer and lo + comp + b > -2 ** 22 and hi + comp + b < 2 ** 22,
            magic1=integer and lo >= MAGIC1_LO and hi <= MAGIC1_HI and abs(k) < 2 ** 24 and abs(lo + comp + b) < 2 ** 24 and
                   abs(hi + comp + b) < 2 ** 24 and fin26,
            fma0=integer and s >= 0 and fin23 and lo + comp + b > -2 ** 23 and hi + comp + b < 2 ** 23,
            fma1=exact)
        for name, v in res.items():
            out[name] = out[name] and bool(v)
    return out
