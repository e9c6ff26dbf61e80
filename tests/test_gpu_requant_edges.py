"""GPU: every requant route at the edge of its host-side proof, bit for bit against the CPU oracle.

dfx_conv_set_weights picks a requant route per stage (0 exact, 1 fast, 2 magic, 3 fma; Conv.requant()) by proving
from the actual weights, bias and scale that the cheaper arithmetic gives the reference's bytes.  The table below
puts, for every kernel family, stage and clause, one op at the LAST value the clause admits and one at the FIRST it
rejects, drives both with activations that attain the accumulator bounds (requant_edges.py), and checks
  1. the bytes against hipref.oracle_conv for every dst type the family has, inside guard bands, with the scalar
     kernel as a second witness,
  2. the route: the last-admitted op reports the route the clause guards, the first-rejected op a lesser one,
  3. from the oracle's s32 output that the bounds were attained.

The clauses, as mathematics.  P / N: sums of a channel's positive / negative weights' magnitudes; b the bias as f32;
s the scale; raw in [L, H] = [-(128 P + 127 N), 127 P + 128 N]; comp = 128 (P - N); t = raw + comp + b, the biased
true accumulator, in [t_lo, t_hi] = [-255 N + b, 255 P + b].

  binade22   "magic" stage 0 of the resident fused kernel: the accumulator starts as the BITS of 1.5 * 2^23 plus
             comp + b; adding raw must stay inside that float's mantissa, whose ulp is 1: -2^22 < t < 2^22.
  binade23   "fma" stage 0 (role-specialised, direct-weight, pointwise, catconv): start bits of 2^23; t >= 0 reads
             as 2^23 + t, which needs t < 2^23; t < 0 borrows from the exponent and reads as 2^23 - |t| / 2, still
             negative after the fma as long as t > -2^23; ReLU + unsigned saturation make it 0.
  room       "magic" with the start value 1 / (2 pi) = 0x3E22F983 (ulp 2^-26): mantissa 0x22F983 + raw must stay in
             [0, 0x7FFFFF]: L >= -0x22F983 and H <= 0x7FFFFF - 0x22F983.
  kexact     the same route adds k = comp + b - 2^23 - 0x22F983 as ONE float: |k| < 2^24.  k < 2^24 follows from
             t_hi < 2^24; the lower side is comp + b >= 2^23 + 0x22F983 - 2^24 + 1 = -6096508.
  sum24      acc + b in one exact f32 add: |t| < 2^24 at both ends ("magic" 1 / (2 pi); "fast" of the streamed,
             direct-weight and pointwise kernels, which add comp + b to float(raw)).
  rawroom    "fast" of the streamed / direct-weight / pointwise kernels converts raw with v_cvt_f32_i32: exact while
             max |raw| <= 2^24.  The proof asks for |comp| + 255 max(P, N) < 2^24, three times as strict with one-sided
             weights; the rows sit at THAT bound, the only one the weights of these shapes reach.
  cvt31      every route but "exact" converts with hardware semantics: |t * s| < 2^31.  The proof keeps a relative
             margin of about 1e-4 below 2^31; last admitted sits at 2^31 (1 - 2^-12), first rejected at 2^31 itself.
  intbias    start values and k absorb the bias as an integer: b == floor(b).
  scale>=0   "fma" stage 0 maps negative t to SOME negative float and relies on ReLU: s >= 0 (-0.0 included).
  finite23 / finite26   the constants s * 2^23 ("fma" stage 0) and s * 2^26 ("magic" 1 / (2 pi)) must be finite.
             Reached with a channel of all-zero weights and zero bias, the only kind cvt31 lets through.
  fma1exact  "fma" stage 1 folds k * s into the addend: exact only if the product fits 24 bits (power-of-two s).

UNREACHABLE (findings; no row):
  room, stage 1 of resident / role-specialised / direct-weight kernels with K = oc <= 128: max |raw| = 128 * 128 * K
             <= 2097152 < 0x22F983.  K = 256 (direct-weight, 256 -> 256 -> 128) reaches the low side.
  room HIGH side, everywhere: H - |L| = N - P <= 128 K, so with the low side admitted H <= 0x22F983 + 128 K, which
             stays below 0x7FFFFF - 0x22F983 = 6096508 for every K < 29722.  The clause is redundant; the weights
             that sit ON it (127 P + 128 N = 6096508, K = 576) exist, requant_edges' CPU test builds them, but
             they fail the low side first.
  sum24 LOW side of the 1 / (2 pi) route: t_lo = L + comp + b >= -0x22F983 + (-6096508) = -8388607 > -2^24 once
             room's low side and kexact hold.  Redundant as well.  (The "fast" proof of the streamed / direct /
             pointwise kernels has neither of those clauses: both sides of ITS sum24 are in the table.)
  kexact upper side (k < 2^24) everywhere: comp + b <= 128 P + b < t_hi < 2^24 < 2^24 + 2^23 + 0x22F983.
  |comp + b| < 2^24 of the "fast" proof (streamed / direct / pointwise): implied by sum24's proof form
             255 max(P, N) + |b| < 2^24 whenever any weight is non-zero; with all-zero weights it IS sum24.
  rawroom, stage 1 (K <= 256) and pointwise ic = 256: 383 * 127 * 256 < 2^24.
  binade22 / binade23 LOW side: reachable and in the table, but beyond it t * s is negative and the stage's ReLU
             turns it into 0 either way: the bytes cannot tell (conservative by construction).

MEASURED with each integer clause loosened by one step in a scratch build (the route assertion of the first-rejected
row goes red in every case; this is about the BYTES of that row):
  room low side       wrong bytes (resident unfused, s32 and f32 dst: 1 of 256 values): the clause is tight.
  room high side      nothing changes: unreachable, see above.
  binade22 / binade23 no byte changes: t = 2^22 (2^23) turns the start bits into exactly the first float of the next
                      binade, which still reads back as t; the first wrong read-back is at limit + 1.  Conservative
                      by one count on the high side, by the ReLU on the low side.
  sum24 / kexact      no byte changes: 2^24 itself is a float, so the add is still exact one step beyond.
"""
import importlib
from collections import namedtuple
from dataclasses import replace

import numpy as np
import pytest

import cases as C
import requant_edges as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import hipref
    return hipref


T22, T23, T24, T31 = 1 << 22, 1 << 23, 1 << 24, 1 << 31
MANT = 0x22F983
ROOM_LO, ROOM_HI = MANT, 0x7FFFFF - MANT
K_LOW = T23 + MANT - T24 + 1                  # comp + b >= K_LOW  <=>  k > -2^24
EXACT, FAST, MAGIC, FMA = 0, 1, 2, 3
ALL = (C.U8, C.S8, C.S32, C.F32)
STREAM, GENERIC = 3, 0                        # VARIANT_MFMA_STREAM / VARIANT_GENERIC of the binding (asserted in test_hook)
K1 = dict(k=(1, 1), pad=(0, 0))

# family -> base shape, forced variant, switches, kernel-name prefixes (the first: what a last-admitted op must run on),
# dst types, branch split (catconv)
Fam = namedtuple("Fam", "base force switches kernels dsts channels")
FAMILIES = {
    "resident_fused": Fam(C.ConvCase("rf", 1, 32, 3, 3, 32, 32), -1, {}, ("conv_mfma_fused_kernel",), ALL, None),
    "resident_unfused": Fam(C.ConvCase("ru", 1, 64, 3, 3, 64, 0), -1, {}, ("conv_mfma_fused_kernel",), ALL, None),
    "roles": Fam(C.ConvCase("ro", 1, 64, 3, 3, 64, 128), -1, {}, ("conv_mfma_roles_kernel", "conv_mfma_fused_kernel"),
                 (C.U8, C.S8), None),
    "roles256": Fam(C.ConvCase("ro256", 1, 64, 3, 3, 64, 256), -1, {}, ("conv_mfma_roles_kernel", "conv_mfma_fused_kernel"),
                    (C.U8, C.S8), None),
    "stream": Fam(C.ConvCase("st", 1, 64, 3, 3, 64, 64), STREAM, {"DFX_STREAM_DIRECT": "0"}, ("conv_stream_kernel",), ALL, None),
    "direct_fused": Fam(C.ConvCase("df", 1, 64, 3, 3, 64, 128), STREAM, {}, ("conv_direct_kernel",), ALL, None),
    "direct_fused256": Fam(C.ConvCase("df256", 1, 256, 3, 3, 256, 128), STREAM, {}, ("conv_direct_kernel",), (C.U8,), None),
    "direct_unfused": Fam(C.ConvCase("du", 1, 64, 3, 3, 64, 0), STREAM, {}, ("conv_direct_kernel",), ALL, None),
    "pointwise": Fam(C.ConvCase("pw256", 1, 256, 1, 1, 64, 0, **K1), -1, {}, ("conv_pw_kernel",), ALL, None),
    "pointwise1024": Fam(C.ConvCase("pw1024", 1, 1024, 1, 1, 64, 0, **K1), -1, {}, ("conv_pw_kernel",), ALL, None),
    "catconv": Fam(C.ConvCase("cat", 1, 256, 1, 1, 64, 0, **K1), -1, {}, ("catconv_pw_kernel",), ALL, [128, 128]),
}
# the route a (family, stage) reaches with every clause comfortably inside, and the dst types that have it
TOP = {
    ("resident_fused", 0): ({MAGIC}, ALL), ("resident_fused", 1): ({MAGIC}, ALL),
    ("resident_unfused", 0): ({MAGIC}, ALL),
    ("roles", 0): ({FMA}, (C.U8, C.S8)), ("roles", 1): ({MAGIC, FMA}, (C.U8, C.S8)),
    ("roles256", 0): ({FMA}, (C.U8, C.S8)), ("roles256", 1): ({MAGIC, FMA}, (C.U8, C.S8)),
    ("stream", 0): ({FAST}, ALL), ("stream", 1): ({FAST}, ALL),
    ("direct_fused", 0): ({FMA}, ALL), ("direct_fused", 1): ({MAGIC, FMA}, (C.U8,)),
    ("direct_fused256", 1): ({MAGIC, FMA}, (C.U8,)),
    ("direct_unfused", 0): ({FMA}, (C.U8,)),
    ("pointwise", 0): ({FMA}, (C.U8,)), ("pointwise1024", 0): ({FMA}, (C.U8,)),
    ("catconv", 0): ({FMA}, (C.U8,)),
}
ANY_FAST = {FAST, MAGIC, FMA}
# clauses of each top route (the docstring's names); "fast" clauses guard every route above "exact"
FMA0 = ("binade23", "intbias", "scale>=0", "finite23")
MAGIC1 = ("room", "kexact", "sum24", "intbias", "finite26")
CLAUSES = {
    ("resident_fused", 0): ("binade22", "intbias", "cvt31"),
    ("resident_fused", 1): MAGIC1 + ("cvt31",),
    ("resident_unfused", 0): MAGIC1 + ("cvt31",),
    ("roles", 0): FMA0 + ("cvt31",), ("roles", 1): MAGIC1 + ("fma1exact", "cvt31"),
    ("roles256", 0): ("binade23",), ("roles256", 1): ("kexact", "fma1exact"),      # two channel groups: the edges again
    ("stream", 0): ("sum24", "rawroom", "intbias", "cvt31"), ("stream", 1): ("sum24", "rawroom", "intbias", "cvt31"),
    ("direct_fused", 0): FMA0 + ("sum24", "rawroom", "cvt31"),
    ("direct_fused", 1): MAGIC1 + ("fma1exact", "rawroom", "cvt31"),
    ("direct_unfused", 0): FMA0 + ("sum24", "rawroom", "cvt31"),
    ("pointwise", 0): FMA0 + ("sum24", "rawroom", "cvt31"),
    ("catconv", 0): FMA0 + ("sum24", "rawroom", "cvt31"),
}
# (family, stage, clause) without a row: see UNREACHABLE in the docstring
UNREACHABLE = {
    ("resident_fused", 1, "room"), ("roles", 1, "room"),
    ("stream", 1, "rawroom"), ("direct_fused", 1, "rawroom"), ("catconv", 0, "rawroom"),
}
# a family whose rows stand in for another's clause (same proof code path is NOT assumed: same family, other shape)
STAND_IN = {("direct_fused", 1, "room"): "direct_fused256", ("pointwise", 0, "rawroom"): "pointwise1024"}

# the route codes a family has: every one must be REPORTED by some row of its table (test_edge_table)
ROUTE_CODES = {"resident_fused": {0, 1, 2}, "resident_unfused": {0, 1, 2}, "roles": {0, 1, 2, 3}, "stream": {0, 1},
               "direct_fused": {0, 1, 2, 3}, "direct_unfused": {0, 1, 3}, "pointwise": {0, 1, 3}, "catconv": {0, 1, 3}}

Row = namedtuple("Row", "family stage clause side P N bias scale dsts want")
FLT_MAX = float(np.finfo(np.float32).max)


def taps_of(family, stage):
    b = FAMILIES[family].base
    return b.ic * b.k[0] * b.k[1] if stage == 0 else b.oc


def _other(K):
    """a modest sum for the side of the weights a clause does not look at (so that a swapped P / N shows)"""
    return min(3000, 16 * K)


def _rows_t(family, stage, clause, limit, want, dsts, cap=1 << 30, sides=("hi", "lo")):
    """t_hi = 255 P + b at limit (last) / limit + 1 (first), and t_lo = -255 N + b at -limit / -(limit + 1);
    the weights carry as much of it as K taps can (up to `cap`, which keeps rawroom comfortable), the bias tops it up"""
    K, out = taps_of(family, stage), []
    o = _other(K)
    big = min(limit // 255, 127 * (K - E.taps_needed(0, o) - 1), cap)
    b = limit - 255 * big
    if "hi" in sides:
        out.append(Row(family, stage, clause + ".hi", "last", big, o, b, None, dsts, want))
        out.append(Row(family, stage, clause + ".hi", "first", big, o, b + 1, None, dsts, want))
    if "lo" in sides:
        out.append(Row(family, stage, clause + ".lo", "last", o, big, -b, None, dsts, want))
        out.append(Row(family, stage, clause + ".lo", "first", o, big, -b - 1, None, dsts, want))
    return out


def _solve_from(a, b, target, K, start):
    """solve_pn with both sides of the weights in play: the first solution with P >= start"""
    for P in range(start, target // a + 1):
        if (target - a * P) % b == 0 and E.taps_needed(P, (target - a * P) // b) <= K:
            return P, (target - a * P) // b
    raise AssertionError("no (P, N) for %d P + %d N = %d within %d taps" % (a, b, target, K))


def rows_of(family, stage, clause):
    """the last-admitted / first-rejected rows of one clause (several pairs where it has two sides)"""
    want, top_dsts = TOP[(family, stage)]
    fam = FAMILIES[family]
    K = taps_of(family, stage)
    mid_p, mid_n = min(20 * K, 40000), min(10 * K, 20000)          # comfortable weights: |t| well below 2^22
    if clause == "binade22":
        return _rows_t(family, stage, clause, T22 - 1, want, top_dsts)
    if clause == "binade23":
        return _rows_t(family, stage, clause, T23 - 1, want, top_dsts)
    if clause == "sum24":
        if family.startswith(("resident", "roles")):               # the 1 / (2 pi) route's clause; "fast" there adds twice
            # (high side only, and P small enough for room's low side: see UNREACHABLE)
            return _rows_t(family, stage, clause, T24 - 1, want, top_dsts, cap=14000, sides=("hi",))
        return _rows_t(family, stage, clause, T24 - 1, ANY_FAST, fam.dsts, cap=30000)   # the "fast" proof's clause
    if clause == "room":
        lo = _solve_from(128, 127, ROOM_LO, K, min(8000, 127 * (K // 4)))
        lo1 = _solve_from(128, 127, ROOM_LO + 1, K, min(8000, 127 * (K // 4)))
        rows = [Row(family, stage, "room.lo", "last", lo[0], lo[1], 4, None, top_dsts, want),
                Row(family, stage, "room.lo", "first", lo1[0], lo1[1], 4, None, top_dsts, want)]
        return rows                                                # (no room.hi rows: see UNREACHABLE)
    if clause == "kexact":
        pn = min(1000, 60 * K)
        return [Row(family, stage, clause, "last", pn, pn, K_LOW, None, top_dsts, want),
                Row(family, stage, clause, "first", pn, pn, K_LOW - 1, None, top_dsts, want)]
    if clause == "rawroom":
        n = 10
        p = (T24 - 1 + 128 * n) // 383                             # largest P with 383 P - 128 N < 2^24
        assert 383 * p - 128 * n < T24 <= 383 * (p + 1) - 128 * n and E.taps_needed(p + 1, n) <= K, (family, K)
        return [Row(family, stage, clause, "last", p, n, 0, None, fam.dsts, ANY_FAST),
                Row(family, stage, clause, "first", p + 1, n, 0, None, fam.dsts, ANY_FAST)]
    if clause == "cvt31":
        big = min((T22 - 1) // 255, 127 * (K - 2))
        b = T22 - 255 * big                                        # t_hi = 2^22: t_hi * s is exact for both scales
        return [Row(family, stage, clause, "last", big, 100, b, 512.0 * (1 - 2.0 ** -12), fam.dsts, ANY_FAST),
                Row(family, stage, clause, "first", big, 100, b, 512.0, fam.dsts, ANY_FAST)]
    if clause == "intbias":
        return [Row(family, stage, clause, "last", mid_p, mid_n, 1000.0, None, top_dsts, want),
                Row(family, stage, clause, "first", mid_p, mid_n, 1000.5, None, top_dsts, want)]
    if clause == "scale>=0":
        return [Row(family, stage, clause, "last", mid_p, mid_n, 7, -0.0, top_dsts, want),
                Row(family, stage, clause, "first", mid_p, mid_n, 7, -float(np.finfo(np.float32).smallest_subnormal), top_dsts, want)]
    if clause in ("finite23", "finite26"):
        e = 23 if clause == "finite23" else 26
        return [Row(family, stage, clause, "last", 0, 0, 0, FLT_MAX / 2.0 ** e, top_dsts, want),
                Row(family, stage, clause, "first", 0, 0, 0, 2.0 ** (128 - e), top_dsts, want)]
    if clause == "fma1exact":
        s = np.float32(2.0 ** -12)                                 # b even: k = comp + b - 2^23 - 0x22F983 is odd
        return [Row(family, stage, clause, "last", mid_p, mid_n, 6, float(s), top_dsts, {FMA}),
                Row(family, stage, clause, "first", mid_p, mid_n, 6, float(np.nextafter(s, np.float32(1))), top_dsts, {FMA})]
    raise KeyError(clause)


def table(family):
    """every row whose ops run on `family` (stand-in shapes serve the family they stand in for)"""
    out = []
    for (f, stage), clauses in CLAUSES.items():
        for cl in clauses:
            if (f, stage, cl) in UNREACHABLE:
                continue
            runs_on = STAND_IN.get((f, stage, cl), f)
            if runs_on == family:
                out += rows_of(runs_on, stage, cl)
    return out


# --- running one op --------------------------------------------------------------------------------------------------
def build_op(row, dst_dt):
    """-> (case, data, slots): the row's op for one dst type"""
    fam = FAMILIES[row.family]
    fused = bool(fam.base.oc1x1)
    relu = dst_dt == C.U8                                          # signed and 4-byte outputs keep their negative halves
    f32_bias = isinstance(row.bias, float)
    base = replace(fam.base, dst_dt=dst_dt, relu0=True if fused else relu, relu1=relu,
                   bia0_dt=C.F32 if (f32_bias and row.stage == 0) else C.S32,
                   bia1_dt=(C.F32 if (f32_bias and row.stage == 1) else C.S32) if fused else C.S32)
    K = taps_of(row.family, row.stage)
    ch = 13 if row.stage == 0 else fam.base.oc1x1 - 3
    case, data, slots = E.edge_op(base, row.stage, {ch: E.weights_with_pn(K, row.P, row.N, seed=row.P + 3 * row.N)})
    t_hi, t_lo = 255 * row.P + row.bias, -255 * row.N + row.bias
    scale = row.scale
    if scale is None:                                              # 1-byte dst: the extremes land near +-100; 4-byte: every count shows
        scale = 3.0 if dst_dt in (C.S32, C.F32) and (row.stage == 1 or not fused) else 100.37 / max(abs(t_hi), abs(t_lo), 1)
    bkey, skey = ("bia0", "scales0") if row.stage == 0 else ("bia1", "scales1")
    bias = np.rint(data[bkey]).astype(np.float32 if f32_bias else np.int32)   # (every other channel integer-valued)
    bias[ch] = row.bias
    data[bkey] = bias
    sc = data[skey].copy()
    if row.clause == "fma1exact":                                  # the one-fma route needs k * s exact on EVERY channel
        sc[:] = np.float32(2.0 ** -12)
    sc[ch] = np.float32(scale)
    data[skey] = sc
    return case, data, slots


def run_op(hip, case, data, force, channels=None):
    """one submit into a guarded dst -> (dst ndarray, kernel name, routes); channels: the branch split of a
    concat + conv op on its fused path"""
    import torch
    import test_gpu_catconv as CC
    if channels:
        op = CC.make_op(case, data, channels, force_path=CC.FUSED)
        try:
            name, routes = op.info().kernel_name.decode(), op.requant()
            dev = [torch.from_numpy(b).cuda() for b in CC.branches_of(data, channels)]
            buf, dst = CC.guarded_dst(op, case)
            op.submit(dev, dst)
            torch.cuda.synchronize()
            hip.assert_guards(buf, CC.BAND, name)
            return dst.cpu().numpy(), name, routes
        finally:
            op.close()
    op = hip.make_conv(case, data, force)
    try:
        name, routes = op.info().kernel_name.decode(), op.requant()
        src = torch.from_numpy(data["src"]).cuda()
        if name.startswith("conv_mfma_"):
            sched = op.sched()
            hip.check_sched(case, sched)
            buf, dst, band = hip.guarded_dst(op, case, sched)
        else:
            buf, dst = CC.guarded_dst(op, case)
            band = CC.BAND
        op.submit(src, dst)
        torch.cuda.synchronize()
        hip.assert_guards(buf, band, name)
        return dst.cpu().numpy(), name, routes
    finally:
        op.close()


def check_row(hip, oracle, row, failures, seen):
    fam = FAMILIES[row.family]
    for n, dst_dt in enumerate(row.dsts):
        what = "%s stage %d %s %s dst %s (P %d N %d bias %r scale %r)" % (
            row.family, row.stage, row.clause, row.side, C.NAME_OF[dst_dt], row.P, row.N, row.bias, row.scale)
        try:
            case, data, slots = build_op(row, dst_dt)
            if n == 0:                                             # 3. the builder's promise, on every row
                ac, ad = E.attain_op(case, data, row.stage)
                E.assert_attained(hip.oracle_conv(oracle, ac, ad), case, data, row.stage, slots)
            ref = hip.oracle_conv(oracle, case, data)
            got, name, routes = run_op(hip, case, data, fam.force, fam.channels)
            hip.assert_bit_equal(got, ref, what + " [" + name + "]")                             # 1.
            wit, wname, wroutes = run_op(hip, case, data, GENERIC)
            assert wname.startswith("conv_generic_kernel") and wroutes[row.stage] == EXACT, (wname, wroutes)
            hip.assert_bit_equal(wit, ref, what + " [scalar witness]")
            r = routes[row.stage]                                                               # 2.
            seen.add(r)
            if row.side == "last":
                assert name.startswith(fam.kernels[0]), "%s: ran on %s" % (what, name)
                assert r in row.want, "%s: route %d, the clause guards %s [%s]" % (what, r, sorted(row.want), name)
            else:
                assert name.startswith(fam.kernels), "%s: ran on %s" % (what, name)
                assert r < min(row.want), "%s: route %d although the clause fails (guards %s) [%s]" % (what, r, sorted(row.want), name)
        except AssertionError as e:
            failures.append(str(e)[:600])


def _switches(tuning, family):
    for k, v in FAMILIES[family].switches.items():
        tuning.setenv(k, v)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_edge_table(hip, oracle, tuning, family):
    """every row of the family: bytes, scalar witness, route, attained bounds"""
    rows = table(family)
    assert rows, family
    _switches(tuning, family)
    failures, seen = [], set()
    for row in rows:
        check_row(hip, oracle, row, failures, seen)
    print("%s: %d rows, %d failures, route codes reported %s" % (family, len(rows), len(failures), sorted(seen)))
    assert not failures, "%d of %d rows:\n%s" % (len(failures), len(rows), "\n".join(failures))
    assert seen >= ROUTE_CODES.get(family, set()), "%s reported %s of its route codes %s" % (family, sorted(seen), sorted(ROUTE_CODES[family]))


def test_hook(hip):
    """Conv.requant(): DFX_ERR_STATE before set_weights, -1 for the missing stage, 0 on the scalar kernel"""
    import test_gpu_catconv as CC
    assert (hip.dfa.VARIANT_MFMA_STREAM, hip.dfa.VARIANT_GENERIC) == (STREAM, GENERIC)
    capi = importlib.import_module("deep-fusion_amd.capi")
    assert (hip.dfa.ROUTE_EXACT, hip.dfa.ROUTE_FAST, hip.dfa.ROUTE_MAGIC, hip.dfa.ROUTE_FMA) == (EXACT, FAST, MAGIC, FMA)
    cat = CC.make_case("hook", [128, 128], 1, 3, 5, **CC.OPTIONS[0])
    for path in (CC.FUSED, CC.TWO):
        op = hip.dfa.ConcatConv(cat.bs, cat.ih, cat.iw, [128, 128], cat.oc, dst_dt=cat.dst_dt, bia_dt=cat.bia0_dt, relu=True, force_path=path)
        try:
            with pytest.raises(capi.DfxError, match="set_weights"):
                op.requant()
            data = C.generate(cat)
            op.set_weights(hip.dfa.reorder_oihw_to_blocked(data["w0"]), data["scales0"], bia=data["bia0"])
            assert op.requant() == (FMA, -1), (path, op.requant())      # both paths read the inner conv handle's proofs
        finally:
            op.close()
    case = C.unfused(C.SMALL)
    data = C.generate(case)
    op = hip.dfa.Conv(data["src"].shape, data["w0"].shape, dst_dt=case.dst_dt, bia0_dt=case.bia0_dt, conv0_relu=True)
    try:
        with pytest.raises(capi.DfxError, match="set_weights"):
            op.requant()
    finally:
        op.close()
    for c, fv, want in ((case, -1, (MAGIC, -1)), (case, GENERIC, (EXACT, -1)), (C.SMALL, GENERIC, (EXACT, EXACT)),
                        (C.SMALL, -1, (MAGIC, MAGIC)), (replace(C.SMALL, rm0=1), -1, (EXACT, MAGIC))):
        op = hip.make_conv(c, C.generate(c), fv)
        try:
            assert op.requant() == want, (c.ident(), fv, op.requant(), want)
        finally:
            op.close()


def test_table_covers_what_it_should():
    """for every (family, stage, clause): a last-admitted and a first-rejected row, or an UNREACHABLE entry; every
    route code a family has is the guarded route of some row; both sides of two-sided clauses are present"""
    rows = [r for f in FAMILIES for r in table(f)]
    for (f, stage), clauses in CLAUSES.items():
        for cl in clauses:
            runs_on = STAND_IN.get((f, stage, cl), f)
            mine = [r for r in rows if r.family == runs_on and r.stage == stage and r.clause.split(".")[0] == cl]
            if (f, stage, cl) in UNREACHABLE:
                assert not mine or runs_on != f, (f, stage, cl)
                continue
            sides = {(r.clause, r.side) for r in mine}
            assert sides and all((c, "last") in sides and (c, "first") in sides for c, _ in sides), (f, stage, cl, sides)
            if cl in ("binade22", "binade23") or (cl == "sum24" and not f.startswith(("resident", "roles"))):
                assert {c for c, _ in sides} == {cl + ".hi", cl + ".lo"}, (f, stage, cl)
    assert {(f, s, c) for f, s, c in UNREACHABLE} <= {(f, s, c) for (f, s), cs in CLAUSES.items() for c in cs}
    # all eight kernel families, every stage they have
    assert {f.rstrip("0123456789") for f, _ in CLAUSES} == {"resident_fused", "resident_unfused", "roles", "stream", "direct_fused",
                                       "direct_unfused", "pointwise", "catconv"}
    for (f, stage) in CLAUSES:
        assert stage == 0 or FAMILIES[f].base.oc1x1, (f, stage)
        if FAMILIES[f].base.oc1x1:
            assert (f, 1) in CLAUSES
    # route codes: guarded by a last-admitted row (want) and reported by a first-rejected one (anything below)
    for f, codes in ROUTE_CODES.items():
        mine = [r for r in rows if r.family.rstrip("0123456789") == f]
        guarded = set().union(*[r.want for r in mine if r.side == "last"])
        below = {c for r in mine if r.side == "first" for c in codes if c < min(r.want)}
        assert codes <= guarded | below, (f, codes, guarded, below)
    # every row's weights are realisable and every one-byte-only route runs on the dst that has it
    for r in rows:
        assert E.taps_needed(r.P, r.N) <= taps_of(r.family, r.stage), r
        assert set(r.dsts) <= set(FAMILIES[r.family].dsts), r


# --- ties ------------------------------------------------------------------------------------------------------------
TIE_RUN = {   # family -> (forced variant, switches, kernel prefix per dst: 1-byte / 4-byte, catconv split)
    "resident_fused": (-1, {}, "conv_mfma_fused_kernel", None),
    "resident_unfused": (-1, {}, "conv_mfma_fused_kernel", None),
    "roles": (-1, {}, "conv_mfma_", None),                      # u8 / s8: role-specialised; s32: resident fused
    "stream_fused": (STREAM, {"DFX_STREAM_DIRECT": "0"}, "conv_stream_kernel", None),
    "stream": (STREAM, {"DFX_STREAM_DIRECT": "0"}, "conv_stream_kernel", None),
    "direct_fused": (STREAM, {}, "conv_direct_kernel", None),
    "direct_fused_g4": (STREAM, {}, "conv_direct_kernel", None),
    "direct_unfused": (STREAM, {}, "conv_direct_kernel", None),
    "pointwise": (-1, {}, "conv_pw_kernel", None),
    "catconv": (-1, {}, "catconv_pw_kernel", [128, 128]),
}


def _run_tie(hip, family, case, data):
    force, _, prefix, channels = TIE_RUN[family]
    got, name, routes = run_op(hip, case, data, force, channels)
    assert name.startswith(prefix), (family, name)
    return got, name, routes


@pytest.mark.parametrize("family,stage", E.tie_table(), ids=lambda v: str(v))
def test_rounding_ties(hip, oracle, tuning, family, stage):
    """power-of-two scales 2^-4 and 2^-3 put hundreds of values on k + 1/2 (tie_data counts them): nearest-even in
    v_cvt_pk_u8_f32 / rintf / cvt_x86_rt, floor on negative halves (rm 1), under every route switch; the routes that
    need an exact k * s (stage-1 "fma") must come with the power of two and go with scale * 1.37"""
    for k, v in TIE_RUN[family][1].items():
        tuning.setenv(k, v)
    failures = []
    for k in E.TIE_KS:
        for dst_dt in E.TIE_DSTS:
            for rm in (0, 1):
                case = E.tie_case(family, stage, dst_dt, rm)
                data, n = E.tie_data(case, stage, k)
                ref = hip.oracle_conv(oracle, case, data)
                skey = "scales0" if stage == 0 else "scales1"
                odd = dict(data, **{skey: data[skey] * np.float32(1.37)})
                ref_odd = hip.oracle_conv(oracle, case, odd)
                for switch in (None, "DFX_NO_MAGIC", "DFX_NO_FAST"):
                    if switch:
                        tuning.setenv(switch, "1")
                    what = "%s stage %d 2^-%d dst %s rm %d %s" % (family, stage, k, C.NAME_OF[dst_dt], rm, switch)
                    try:
                        got, name, routes = _run_tie(hip, family, case, data)
                        hip.assert_bit_equal(got, ref, what + " [" + name + "] " + str(n))
                        got, name_odd, routes_odd = _run_tie(hip, family, case, odd)
                        hip.assert_bit_equal(got, ref_odd, what + " x 1.37 [" + name_odd + "]")
                        if switch == "DFX_NO_FAST" or rm == 1:
                            assert routes[stage] == EXACT, (what, routes)
                        if switch == "DFX_NO_MAGIC":
                            assert max(routes) <= FAST, (what, routes)
                        fma1 = (family == "roles" and dst_dt in (C.U8, C.S8)) or (family == "direct_fused_g4" and dst_dt == C.U8)
                        if switch is None and rm == 0 and stage == 1 and fma1:
                            assert routes[1] == FMA, "%s: power-of-two scale must take the one-fma route: %r [%s]" % (what, routes, name)
                            assert routes_odd[1] == MAGIC, "%s: scale x 1.37 must take the magic route: %r [%s]" % (what, routes_odd, name_odd)
                    except AssertionError as e:
                        failures.append(str(e)[:600])
                    finally:
                        if switch:
                            tuning.setenv(switch, None)
    assert not failures, "%d:\n%s" % (len(failures), "\n".join(failures))


# --- extreme constants ---------------------------------------------------------------------------------------------
S32_BIASES = [T24 - 1, -(T24 - 1), T24, -T24, T24 + 1, -(T24 + 1), T31 - 1, -T31]
F32_BIASES = [0.5, -0.0, 1e30, float("inf"), float("-inf"), float("nan")]
SCALES = [0.0, -0.0, -0.0123, 1e-40, 2.0 ** -126, 3e38, float("inf"), float("nan")]
EXTREME_FAMILIES = ["resident_fused", "resident_unfused", "roles", "stream", "direct_fused", "direct_unfused", "pointwise", "catconv"]


@pytest.mark.parametrize("family", EXTREME_FAMILIES)
def test_extreme_constants(hip, oracle, tuning, family):
    """one constant at a time on ONE channel of a per-channel op (the other channels keep normal values, the route
    decision is per op): s32 biases around 2^24 (their conversion to f32 rounds) and at the ends of the type, f32
    biases and scales that are fractional, signed zeros, denormal, huge, infinite, NaN"""
    _switches(tuning, family)
    fam = FAMILIES[family]
    failures, n = [], 0
    for stage in ((0, 1) if fam.base.oc1x1 else (0,)):
        K = taps_of(family, stage)
        consts = ([("bias", b) for b in S32_BIASES] + [("bias", b) for b in F32_BIASES] + [("scale", s) for s in SCALES])
        for kind, value in consts:
            for dst_dt in fam.dsts:
                row = Row(family, stage, "extreme", "-", min(20 * K, 40000), min(10 * K, 20000),
                          value if kind == "bias" else 7, value if kind == "scale" else None, (dst_dt,), None)
                what = "%s stage %d %s %r dst %s" % (family, stage, kind, value, C.NAME_OF[dst_dt])
                try:
                    if kind == "bias" and isinstance(value, float) and not np.isfinite(value):
                        row = row._replace(scale=0.01)                 # (the automatic scale divides by |t|)
                    case, data, slots = build_op(row, dst_dt)
                    ref = hip.oracle_conv(oracle, case, data)
                    got, name, routes = run_op(hip, case, data, fam.force, fam.channels)
                    assert name.startswith(fam.kernels), (what, name)
                    hip.assert_bit_equal(got, ref, what + " [" + name + "] routes " + str(routes))
                    wit, wname, _ = run_op(hip, case, data, GENERIC)
                    hip.assert_bit_equal(wit, ref, what + " [scalar witness]")
                    n += 1
                except AssertionError as e:
                    failures.append(str(e)[:600])
    assert not failures, "%d of %d:\n%s" % (len(failures), n + len(failures), "\n".join(failures))


# --- the benchmarked ops keep their routes -------------------------------------------------------------------------
# BASELINE.json's shapes at small N with cases.generate's reference-range data: kernel-name prefix and Conv.requant()
# as reported by commit 760fb5e ("Add concat + pointwise conv op that reads the branches in place"), the parent of
# the commit that added this hook (the hook changes no proof).  A fix that over-tightens a proof moves one of these
# to a slower route: that has to be a decision, not an accident.
HEADLINE = {
    "cfg2": (C.CONFIG2, ("conv_mfma_fused_kernel", (2, 2))),
    "cfg3n2-s32": (C.CONFIG3_SMALL, ("conv_mfma_fused_kernel", (2, 2))),
    "cfg3n2-u8": (replace(C.CONFIG3_SMALL, dst_dt=C.U8), ("conv_mfma_roles_kernel", (3, 3))),
    "cfg5n1": (C.CONFIG5_TINY, ("conv_mfma_fused_kernel", (2, 2))),
    "res3n2": (C.ConvCase("res3", 2, 128, 28, 28, 128, 512, dst_dt=C.U8), ("conv_direct_kernel", (3, 2))),
    "res4n2": (C.ConvCase("res4", 2, 256, 14, 14, 256, 1024, dst_dt=C.U8), ("conv_direct_kernel", (3, 3))),
}


@pytest.mark.parametrize("which", list(HEADLINE))
def test_headline_routes_are_pinned(hip, which):
    case, want = HEADLINE[which]
    op = hip.make_conv(case, C.generate(case))
    try:
        got = (op.info().kernel_name.decode().split("<")[0], op.requant())
    finally:
        op.close()
    print("HEADLINE %s %r" % (which, got))
    assert got == want, (which, got, want)
