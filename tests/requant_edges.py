"""Adversarial inputs for the requant routes (pure numpy, needs no GPU).

dfx_conv_set_weights proves, per output channel, that a cheaper requant arithmetic gives the reference's bytes.
Every proof bounds the accumulator by its worst case over ALL activations.  With P the sum of a channel's positive
weights and N the sum of its negative weights' magnitudes, and activations u8 (stored as u8 - 128 by the kernels):

    raw accumulator   sum w * (a - 128)   lies in [-(128 P + 127 N), 127 P + 128 N]
    true accumulator  sum w * a           lies in [-255 N, 255 P]

Random activations stay within a few sqrt(K) of zero and never come near these bounds.  This module builds
  * weights with PRESCRIBED P and N (solve_pn: a small Diophantine search; weights_with_pn),
  * activations that ATTAIN both bounds for chosen channels ("max": 255 where w > 0, 0 elsewhere; "min": the inverse)
    on the smallest shapes -- 3x3 kernels: ih = iw = 3, pad 0, one output pixel per image, the batch index enumerates
    (channel, max / min) pairs; 1x1 kernels: one image whose pixels enumerate the pairs,
  * for stage 1 of a fused op a conv0 that COPIES its input (w0[oc][ic = oc][centre] = 1, scale 1, no bias), so that
    the intermediate is the source's centre pixel and the same patterns drive the 1x1 stage,
  * tie data: cases.generate's reference-range data with a power-of-two scale, with the exact int64 accumulators
    counted so that enough values land on k + 1/2 (tie_data refuses data that does not).
"""
from dataclasses import replace

import numpy as np

import cases as C

W_MIN, W_MAX = -128, 127


def taps_needed(P, N):
    return -(-P // W_MAX) + -(-N // -W_MIN)


def solve_pn(a, b, target, K, prefer_small_p=True):
    """-> (P, N) with a * P + b * N == target, P and N non-negative and realisable with K int8 taps
    (ceil(P / 127) + ceil(N / 128) <= K), or None.  The smallest (or largest) such P."""
    assert a > 0 and b > 0 and K > 0
    if target < 0:
        return None
    p_hi = min(target // a, W_MAX * K)
    rng = range(0, p_hi + 1) if prefer_small_p else range(p_hi, -1, -1)
    for P in rng:
        rest = target - a * P
        if rest % b:
            continue
        N = rest // b
        if taps_needed(P, N) <= K:
            return P, N
    return None


def weights_with_pn(K, P, N, seed=0):
    """-> int8[K] whose positive entries sum to P and whose negative entries sum to -N, at seeded positions."""
    assert taps_needed(P, N) <= K, (K, P, N)
    vals = [W_MAX] * (P // W_MAX) + ([P % W_MAX] if P % W_MAX else [])
    vals += [W_MIN] * (N // -W_MIN) + ([-(N % -W_MIN)] if N % -W_MIN else [])
    w = np.zeros(K, dtype=np.int64)
    w[np.random.default_rng(seed).permutation(K)[:len(vals)]] = vals
    assert w[w > 0].sum() == P and -w[w < 0].sum() == N
    return w.astype(np.int8)


def pn_of(w):
    w = np.asarray(w, dtype=np.int64).reshape(-1)
    return int(w[w > 0].sum()), int(-w[w < 0].sum())


def pattern(w, which):
    """u8 activations (shape of w) that attain the true accumulator's maximum 255 P ("max") or minimum -255 N"""
    w = np.asarray(w)
    return np.where(w > 0 if which == "max" else w < 0, 255, 0).astype(np.uint8)


def _slots(targets):
    return [(c, which) for c in targets for which in ("max", "min")]


def edge_op(base, stage, channel_weights, seed=77):
    """An op whose inputs attain both accumulator bounds of the given output channels of `stage`.

    base: a cases.ConvCase giving ic / oc / oc1x1 / k and the options (dtypes, relu, round modes); its bs / ih / iw /
    pad are replaced by the smallest shape.  channel_weights: {channel: int8[K]} in (ic, kh, kw) order for stage 0,
    (oc,) order for stage 1; every other channel keeps reference-range random weights.
    -> (case, data, slots): slots[i] = (channel, "max" | "min") is the pair that output position i serves (position
    = image index for 3x3 kernels, pixel index of the one image for 1x1 kernels); two more positions hold random
    data.  data has per-channel scales and s32 biases of cases.generate's kind for the caller to overwrite."""
    slots = _slots(sorted(channel_weights))
    npos = len(slots) + 2
    kh, kw = base.k
    if (kh, kw) == (3, 3):
        case = replace(base, bs=npos, ih=3, iw=3, pad=(0, 0), stride=(1, 1))
    else:
        assert (kh, kw) == (1, 1)
        case = replace(base, bs=1, ih=1, iw=npos, pad=(0, 0), stride=(1, 1))
    case = replace(case, seed=seed, per_channel0=True, per_channel1=bool(base.oc1x1))
    data = C.generate(case)
    rng = np.random.default_rng(seed + 1)
    src = rng.integers(0, 256, data["src"].shape).astype(np.uint8)     # full range everywhere else
    cy, cx = kh // 2, kw // 2
    if stage == 0:
        w0 = data["w0"].copy()
        for c, w in channel_weights.items():
            w0[c] = np.asarray(w, dtype=np.int8).reshape(case.ic, kh, kw)
        data["w0"] = w0
        for i, (c, which) in enumerate(slots):
            pat = pattern(w0[c], which)                                 # (ic, kh, kw)
            if (kh, kw) == (3, 3):
                src[i] = pat.transpose(1, 2, 0)
            else:
                src[0, 0, i] = pat[:, 0, 0]
    else:
        assert case.oc1x1 and case.ic >= case.oc, "stage 1 needs a copying conv0: ic >= oc"
        w0 = np.zeros_like(data["w0"])
        for o in range(case.oc):
            w0[o, o, cy, cx] = 1
        w1 = data["w1"].copy()
        for c, w in channel_weights.items():
            w1[c, :, 0, 0] = np.asarray(w, dtype=np.int8)
        data.update(w0=w0, w1=w1, scales0=np.ones(case.oc, dtype=np.float32), bia0=None)
        case = replace(case, bia0_dt=C.UNDEF, relu0=True, rm0=0)
        for i, (c, which) in enumerate(slots):
            pat = pattern(w1[c, :, 0, 0], which)
            if (kh, kw) == (3, 3):
                src[i, cy, cx, :case.oc] = pat
            else:
                src[0, 0, i, :case.oc] = pat
    data["src"] = src
    return case, data, slots


def attain_op(case, data, stage):
    """the same inputs with the stage's accumulator made visible: s32 dst, scale 1, no bias, no ReLU
    (stage 0: the unfused conv0; stage 1: conv0 as it is, the 1x1 stage neutral)"""
    if stage == 0:
        c = replace(case, oc1x1=0, dst_dt=C.S32, bia0_dt=C.UNDEF, relu0=False, rm0=0, per_channel0=False)
        d = dict(data, w1=None, bia0=None, bia1=None, scales0=np.ones(1, dtype=np.float32))
    else:
        c = replace(case, dst_dt=C.S32, bia1_dt=C.UNDEF, relu1=False, rm1=0, per_channel1=False)
        d = dict(data, bia1=None, scales1=np.ones(1, dtype=np.float32))
    return c, d


def position(out, case, i):
    """output vector (all channels) of position i of an edge_op"""
    return out[i, 0, 0] if tuple(case.k) == (3, 3) else out[0, 0, i]


def assert_attained(acc_s32, case, data, stage, slots):
    """acc_s32: the oracle's output of attain_op.  Every slot must hold exactly 255 P / -255 N of its channel --
    as the reference shows an accumulator: converted to f32 on its way out (vcvtdq2ps), so a bound beyond 2^24 (K =
    576 and 1024 reach 1.9e7 and 3.3e7) appears rounded to the nearest f32, and is compared as such."""
    for i, (c, which) in enumerate(slots):
        w = data["w0"][c] if stage == 0 else data["w1"][c]
        P, N = pn_of(w)
        bound = 255 * P if which == "max" else -255 * N
        want = int(np.float32(bound))                                   # == bound while |bound| <= 2^24
        got = int(position(acc_s32, case, i)[c])
        assert got == want, "stage %d channel %d %s: accumulator %d, the bound is %d (P %d, N %d)" % (
            stage, c, which, got, want, P, N)


# --- ties ---------------------------------------------------------------------------------------------------------
def exact_acc(case, data):
    """-> (acc0, acc1): exact int64 accumulators before bias; acc1 (None for an unfused op) follows the oracle's u8
    intermediate, which the caller passes as data["mid"] or which is recomputed here with float32 arithmetic"""
    from refmath import _acc_conv, _requant, _store
    acc0 = _acc_conv(data["src"], data["w0"], case.stride, case.pad)
    if not case.oc1x1:
        return acc0, None
    mid = _store(_requant(acc0, data["bia0"], data["scales0"], True), C.U8, case.rm0).astype(np.int64)
    return acc0, mid @ data["w1"].reshape(case.oc1x1, case.oc).astype(np.int64).T


def count_ties_of(t, k, dt, relu):
    """ties of t * 2^-k (t: exact int64 accumulator + bias) among the values that stay inside the unsaturated range of
    the output type dt after the ReLU (if any): dict with total / below (the even neighbour is the one below:
    nearest-even rounds down) / above / negative / need_negative.  Shared with op_ties.py."""
    half = 1 << (k - 1)
    tie = (t & ((1 << k) - 1)) == half
    fl = t >> k                                                   # floor(t / 2^k); the tie sits at fl + 1/2
    lo, hi = {C.U8: (0, 255), C.S8: (-128, 127)}.get(dt, (-(1 << 31), (1 << 31) - 1))
    if relu:
        lo = max(lo, 0)
    inside = tie & (fl >= lo) & (fl + 1 <= hi)
    return dict(total=int(inside.sum()), below=int((inside & (fl % 2 == 0)).sum()),
                above=int((inside & (fl % 2 != 0)).sum()), negative=int((inside & (fl < 0)).sum()),
                need_negative=(not relu) and dt in (C.S8, C.S32, C.F32))


def count_ties(case, acc, bias, k, stage):
    """count_ties_of for one stage of a conv case: the intermediate of a fused op is u8 behind a ReLU"""
    fused = bool(case.oc1x1)
    final = stage == 1 or not fused
    relu = (case.relu1 if stage == 1 else case.relu0) or (not final) or case.dst_dt == C.U8
    dt = case.dst_dt if final else C.U8
    return count_ties_of(acc + (0 if bias is None else bias.astype(np.int64)), k, dt, relu)


def assert_enough_ties(n, what):
    """at least 50 ties, 15 with the even neighbour below, 15 above and, where negative results survive, 15 negative"""
    assert n["total"] >= 50 and n["below"] >= 15 and n["above"] >= 15, (what, n)
    assert not n["need_negative"] or n["negative"] >= 15, (what, n)


def tie_data(case, stage, k):
    """cases.generate(case) (reference-range data, integer biases) with the stage's scale replaced by 2^-k.
    Refuses data without at least 50 exact ties inside the unsaturated output range, 15 of them rounding to the even
    value below, 15 to the even value above, and -- where negative results survive (no ReLU, signed or 4-byte
    dst) -- 15 negative ones.  -> (data, counts)"""
    data = C.generate(case)
    s = np.float32(2.0 ** -k)
    if stage == 0:
        data["scales0"] = np.full_like(data["scales0"], s)
    else:
        data["scales1"] = np.full_like(data["scales1"], s)
    acc0, acc1 = exact_acc(case, data)
    bias = data["bia0"] if stage == 0 else data["bia1"]
    assert bias is None or bias.dtype != np.float32, "tie data needs integer biases"
    n = count_ties(case, acc0 if stage == 0 else acc1, bias, k, stage)
    assert_enough_ties(n, (case.ident(), stage, k))
    return data, n


# --- the tie table (shared by the CPU test of the counts and the GPU test) -----------------------------------------
# (family, base case, stage).  SMALL / SMALL64 and the smallest shape of every other kernel family's list:
# d64 and u64 (test_gpu_parity DIRECT_SHAPES / UNFUSED_DIRECT_SHAPES), pw1px grown to 9 x 11 pixels, the 128 + 128
# join at 297 pixels (test_gpu_catconv), k1 (STREAM_SHAPES).  SMALL64 forced onto the direct-weight kernel gives
# that kernel a 1x1 stage in groups of four, the only form with the stage-1 "magic" / "fma" routes.
TIE_SHAPES = {
    "resident_fused": C.SMALL,
    "resident_unfused": C.unfused(C.SMALL),
    "roles": C.SMALL64,
    "stream_fused": C.SMALL,
    "stream": C.ConvCase("k1", 2, 32, 5, 5, 32, 0, k=(1, 1), pad=(0, 0), dst_dt=C.S32),
    "direct_fused": C.ConvCase("d64", 2, 64, 12, 10, 64, 64, dst_dt=C.S8, relu1=False),
    "direct_fused_g4": C.SMALL64,
    "direct_unfused": C.ConvCase("u64", 3, 64, 12, 10, 64, 0, dst_dt=C.U8),
    "pointwise": C.ConvCase("pw9x11", 1, 256, 9, 11, 64, 0, k=(1, 1), pad=(0, 0), dst_dt=C.U8),
    "catconv": C.ConvCase("128+128-px297", 1, 256, 11, 27, 64, 0, k=(1, 1), pad=(0, 0), dst_dt=C.U8),
}
TIE_KS = (4, 3)
TIE_DSTS = (C.U8, C.S8, C.S32)


def tie_case(family, stage, dst_dt, rm):
    """the family's shape with the dst type and round mode under test; signed and 4-byte outputs drop the storing
    stage's ReLU so that negative halves reach the conversion"""
    base = TIE_SHAPES[family]
    relu = dst_dt == C.U8
    c = replace(base, dst_dt=dst_dt, bia0_dt=C.S32, bia1_dt=C.S32, wide=False, per_channel0=False, per_channel1=False)
    if base.oc1x1:
        return replace(c, relu0=True, relu1=relu, rm0=rm if stage == 0 else 0, rm1=rm if stage == 1 else 0)
    return replace(c, relu0=relu, rm0=rm)


def tie_table():
    """-> [(family, stage)]"""
    return [(f, s) for f, base in TIE_SHAPES.items() for s in ((0, 1) if base.oc1x1 else (0,))]
