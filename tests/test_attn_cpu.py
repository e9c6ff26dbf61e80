"""CPU-only checks of the fused int8 attention (dfx_attn_*): the numpy reference the GPU tests compare against
(tests/attn_ref.py: bmm_ref -> head_ref's softmax -> bmm_ref) equals the chained pure-Python witnesses of the two ops on tiny
cases; every case of the GPU tables holds the regime it is meant to hold; the covering table covers; the C ABI validates
descriptors in the documented order before it touches a device, every clause at the last value it admits and the first it
rejects; the ctypes mirrors match the header; the op's host-side plan (csrc/attn_plan.h) agrees with its Python mirror and is
clean under the host sanitizers as a stand-alone program."""
import ctypes
import importlib
import itertools
import os
import subprocess

import numpy as np
import pytest

import attn_ref as A
import bmm_ref as R

dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-fusion_amd")
INVALID, UNSUPPORTED, HIP, NO_DEVICE, STATE = 1, 2, 3, 4, 5
CAP = 0.10            # at most this share of the logits / of O on a saturation bound, except in the cases built to saturate


@pytest.fixture(autouse=True)
def the_package_knows_the_op():
    """every test of this file is about dfx_attn: the reference checks too stand on the package that binds it"""
    assert hasattr(dfa, "Attention") and dfa.ATTN_FUSED == A.FUSED and dfa.ATTN_CHAIN == A.CHAIN
    assert "dfx_attn_create" in dfa.declared_symbols()


# ---- 1. the reference against the witnesses -----------------------------------------------------------------------------------
TINY = [A.AttnCase("tiny", 3, 5, 4, 3, q_dt=A.S8, dst_dt=A.S8, seed=60000), A.AttnCase("tiny", 2, 17, 3, 5, q_dt=A.U8, dst_dt=A.U8, rm=1, seed=60001),
        A.AttnCase("tiny", 4, 1, 2, 2, q_dt=A.U8, dst_dt=A.S32, per_channel=True, seed=60002),
        A.AttnCase("tiny", 3, 6, 5, 4, q_dt=A.S8, dst_dt=A.F32, batch=(2, 2), relu=True, seed=60003),
        A.AttnCase("tiny-heads", 5, 5, 4, 4, q_dt=A.S8, dst_dt=A.S8, batch=(2, 2), seed=60004,
                   **{w + "_strides": R.attention_strides(2, 2, 5, 4) for w in "qkvo"})]


@pytest.mark.parametrize("case", TINY, ids=lambda c: c.ident())
def test_reference_equals_the_witness(case):
    data = A.generate(case)
    got, want = A.reference(case, data), A.witness(case, data)
    assert got.dtype == want.dtype == np.uint8 and got.size == A.storage_elems(case, "o") * A.SIZE_OF[case.dst_dt]
    assert np.array_equal(got, want), case.ident()
    o = got.view(A.NP_OF[case.dst_dt])
    untouched = np.ones(o.size, dtype=bool)
    untouched[A.o_index(case).reshape(-1)] = False
    assert (got.reshape(-1, A.SIZE_OF[case.dst_dt])[untouched] == A.POISON).all()       # the poison fill survives


def test_special_cases_equal_the_witness():
    for case, data in A.tie_cases()[::3] + [cd for cd in A.softmax_edge_cases() if cd[0].name.startswith("tk1")][:2]:
        assert np.array_equal(A.reference(case, data), A.witness(case, data)), case.ident()


def test_the_round_mode_applies_to_both_requants():
    case = A.AttnCase("rm", 5, 9, 7, 6, q_dt=A.U8, dst_dt=A.S8, rm=1, seed=60100)
    assert A.qk_case(case).rm == 1 and A.pv_case(case).rm == 1
    data = A.generate(case)
    down, near = A.chain(case, data)[0], A.chain(A.AttnCase(**dict(case.__dict__, rm=0)), data)[0]
    assert not np.array_equal(down, near) and (down[:, :9].astype(int) <= near[:, :9].astype(int)).all()


# ---- 2. the regime of every case of the GPU tables ----------------------------------------------------------------------------
def _regime(case, data):
    logits, probs, _ = A.chain(case, data)
    lv, pv = logits[:, :case.tk], probs[:, :case.tk]
    ov = A.o_values(case, data, probs)
    return (float(((lv == 127) | (lv == -128)).mean()), float((pv > 0).sum(axis=1).mean()), R.saturated_fraction(A.pv_case(case), ov),
            bool((ov != 0).any()))


def test_tables_hold_their_regimes():
    """every table case that is not flagged `saturating`: at most 10 % of the logits on 127 / -128, on average at least 2 non-zero
    probabilities per row wherever tk >= 15, at most 10 % of O on a saturation bound, no O all zero"""
    t = A.table()
    assert len(t) == len(A.shape_grid()) + len(A.batch_cases()) + 4 + 2 + len(A.auto_cases()) and len(A.shape_grid()) >= 120
    built = 0
    for case in t:
        if case.saturating:
            built += 1
            continue
        lsat, nz, osat, any_o = _regime(case, A.generate(case))
        assert lsat <= CAP, (case.ident(), lsat)
        assert case.tk < 15 or nz >= 2.0, (case.ident(), nz)
        assert osat <= CAP, (case.ident(), osat)
        assert any_o, case.ident()
    assert built == 4
    assert [c.ident() for c in t if not A.fused_class(A.desc_of(c))] == [A.auto_cases()[-1][0].ident()]
    assert len(A.single_cases()) == 7
    for case in A.single_cases():
        lsat, nz, osat, any_o = _regime(case, A.generate(case))                     # the single cases of the GPU tests
        assert lsat <= CAP and nz >= 2.0 and osat <= CAP and any_o, case.ident()


@pytest.mark.parametrize("shape", A.REGIME_SHAPES + ((33, 1, 17, 33), (1, 1, 1, 1)), ids=lambda s: "x".join(map(str, s)))
def test_the_generator_keeps_the_reference_inside_the_regime(shape):
    """uniform operands, the centred logit scale, softmax_table(0.0625, tk), prob_scale 255, out scale 1 / 256 (s8) and 1 / 128
    (u8), held to the figures recorded for them: logit saturation 0.1 to 0.2 %, O saturation below 0.1 %, 10 to 120 non-zero
    probabilities per row for tk from 15 to 4096.  The logit figure is a rate over n = G * tq * tk samples, so a case is held
    to the upper recorded rate p = 0.2 % plus four standard deviations of a sample of its size, 4 * sqrt(p / n)."""
    tq, tk, d, dv = shape
    for dst in (A.S8, A.U8):
        case = A.AttnCase("regime", tq, tk, d, dv, q_dt=A.S8, dst_dt=dst, seed=61000)
        lsat, nz, osat, any_o = _regime(case, A.generate(case))
        assert lsat <= 0.002 + 4.0 * (0.002 / (tq * tk)) ** 0.5, (shape, lsat)
        # (tk = 1: P = 255 and O = rint(255 V / 256), so V = -128 lands on -128 unclipped: 1 / 256 of a uniform V, a few per
        #  cent of a 33-column sample; those shapes are held to the tables' cap)
        assert osat <= (0.001 if tk > 1 else CAP) and any_o, (shape, osat)
        if tk >= 15:
            assert 10.0 <= nz <= 120.0, (shape, nz)
        else:
            assert nz == 1.0


def test_the_covering_table_covers():
    shapes = A.covering_shapes()
    assert 120 <= len(shapes) <= 200 and len(set(shapes)) == len(shapes)
    for i, j in itertools.permutations(range(4), 2):
        for v in A.AXES[i]:
            partners = {s[j] for s in shapes if s[i] == v}
            assert len(partners) >= 2, (i, j, v, partners)
    g = A.shape_grid()
    assert {c.q_dt for c in g} == {A.S8, A.U8} and {c.dst_dt for c in g} == set(A.DST_ROTATION) and {c.rm for c in g} == {0, 1}
    assert {c.relu for c in g} == {True, False} and {c.per_channel for c in g} == {True, False}
    assert {c.strides("o")[2] % 4 == 0 for c in g} == {True, False}
    assert {A.kparts(A.desc_of(c)) for c in g} == {1, 2, 4}                          # every key split of the context
    assert A.strips(A.desc_of(A.GRID_CAP_CASE)) == 12 and A.CLASS_BOUND_CASE.tk == A.TK_MAX


# ---- 3. the plan: the stand-alone program against the Python mirror, and under the host sanitizers ------------------------------
TQ_EDGE = -(-2 ** 40 // R.up16(R.KMAX))       # the first tq whose logits G * tq * up16(tk) reach 2^40 at tk's limit, one matrix


def _variants():
    """descriptors around every clause: table cases, then one field at a time moved off a valid descriptor"""
    out = [A.desc_of(c, fp) for c in A.table()[::9] + A.batch_cases() for fp in (-1, A.FUSED, A.CHAIN)]
    base = A.desc_of(A.AttnCase("v", 33, 37, 40, 35, batch=(2, 3)))
    for key, vals in (("batch0", (0, 1)), ("batch1", (0, 1)), ("tq", (0, 1)), ("dv", (0, 1)), ("d", (0, 1, 256, 257, R.KMAX, R.KMAX + 1)),
                      ("tk", (0, 1, 4096, 4097, R.KMAX, R.KMAX + 1, 65535)), ("q_dt", range(0, 6)), ("k_dt", range(0, 6)), ("v_dt", range(0, 6)),
                      ("dst_dt", range(0, 6)), ("round_mode", (-1, 0, 1, 2)), ("nscales", (0, 1, 34, 35, 36)), ("force_path", (-2, -1, 0, 1, 2)),
                      ("prob_scale", (255.0, -1.0, 3.0e38, float("inf"), float("nan"))), ("ldq", (39, 40, 41, 48)), ("ldk", (39, 40, 48)),
                      ("ldv", (34, 35, 48)), ("ldo", (34, 35)), ("q_s0", (-1, 0, 8, 16)), ("q_s1", (-16, 0, 24)), ("k_s0", (-1, 0)), ("k_s1", (-1, 0, 8)),
                      ("v_s0", (-1, 0, 8)), ("v_s1", (-1, 0)), ("o_s0", (-1, 0, 3 * 33 * 38 - 1, 3 * 33 * 38, 2 ** 40)), ("o_s1", (-1, 0, 33 * 38 - 1, 33 * 38)),
                      ("q_s0", (2 ** 40 - 2 * 33 * 48 - 33 * 48 + 7, 2 ** 40, 2 ** 62))):
        for v in vals:
            for fp in (-1, A.FUSED):
                d = dict(base, force_path=fp)
                d[key] = v
                if key == "d" and v > 40:
                    d["ldq"] = d["ldk"] = R.up16(v)
                    d["q_s1"], d["k_s1"] = 33 * d["ldq"], 37 * d["ldk"]
                    d["q_s0"], d["k_s0"] = 3 * d["q_s1"], 3 * d["k_s1"]
                if key == "tk":
                    d["k_s1"], d["v_s1"] = max(v, 1) * 48, max(v, 1) * 48
                    d["k_s0"], d["v_s0"] = 3 * d["k_s1"], 3 * d["v_s1"]
                out.append(d)
    one = dict(base, batch0=1, batch1=1)
    out += [dict(one, tq=R.MN_MAX, tk=1, d=1, dv=1, ldo=1), dict(one, tq=R.MN_MAX + 1, tk=1, d=1, dv=1, ldo=1),
            dict(one, tq=TQ_EDGE, tk=R.KMAX, k_s1=R.KMAX * 48, v_s1=R.KMAX * 48), dict(one, tq=TQ_EDGE - 1, tk=R.KMAX, k_s1=R.KMAX * 48, v_s1=R.KMAX * 48),
            dict(one, tk=R.KMAX, d=R.KMAX, ldq=R.up16(R.KMAX), ldk=R.up16(R.KMAX), k_s1=R.KMAX * 48, v_s1=R.KMAX * 48)]
    heads = [c for c in A.batch_cases() if c.name == "heads"][0]
    hd = A.desc_of(heads)
    out += [hd, dict(hd, o_s1=A.D - 1), dict(hd, ldo=A.HEADS * A.D - 1), dict(hd, o_s0=hd["o_s0"] - 1), dict(hd, k_dt=A.U8), dict(hd, k_dt=A.U8, ldo=1)]
    return out


def _plan_lines(exe, descs, cus, cap, ls, os_):
    def fmt(d, f):
        return repr(float(d[f])) if f == "prob_scale" else str(int(d[f]))
    text = "".join(" ".join(fmt(d, f) for f in A.FIELDS) + " %d %d %r %r\n" % (cus, cap, ls, os_) for d in descs)
    p = subprocess.run([exe, "-"], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    lines = p.stdout.decode().splitlines()
    assert len(lines) == len(descs), p.stdout.decode()[-2000:]
    return lines


def _check_against_mirror(exe):
    descs = _variants()
    seen, fast = set(), set()
    for cus, cap, ls, os_ in ((256, 0, 0.004, 1.0 / 256), (8, 0, 1.0e6, 1.0e6), (256, 3, float("nan"), float("inf"))):
        for d, line in zip(descs, _plan_lines(exe, descs, cus, cap, ls, os_)):
            got = [int(x) for x in line.split()]
            rc = A.validate(d)
            seen.add(rc)
            assert got[0] == rc, (d, line)
            if rc == INVALID:
                continue
            want = [rc, int(A.fused_class(d)), -1 if rc else A.auto_path(d), A.lds_bytes(d), A.strips(d), A.kparts(d), A.planned_grid(d, cus, cap),
                    int(A.fast_logits(d, ls)), int(A.fast_context(d, [os_] * d["nscales"])), A.scratch_bytes(d), A.algorithmic_ops(d),
                    A.algorithmic_bytes(d), -1 if rc else 1]           # (last: dfx_bmm and dfx_head accept the chain's descriptors)
            fast.add((want[7], want[8]))
            assert got == want, (d, got, want)
    assert seen == {0, INVALID, UNSUPPORTED} and (1, 1) in fast and (0, 0) in fast


def test_attn_plan_check_agrees_with_the_mirror_and_is_clean_under_the_host_sanitizers(tmp_path):
    """tools/attn_plan_check.cc, a stand-alone host program over csrc/attn_plan.h, built with the flags of the host Makefile's
    SAN=1 rule (ASan + UBSan) into a scratch directory and run directly: its self-check, then the descriptors of the Python
    mirror through its stdin mode.  Nothing is loaded into Python."""
    src = os.path.join(PKG, "tools", "attn_plan_check.cc")
    assert os.path.exists(src), "tools/attn_plan_check.cc is missing"
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert "$(TOOLS)/attn_plan_check: $(TOOLS)/attn_plan_check.cc ../csrc/attn_plan.h" in mk
    exe = tmp_path / "attn_plan_check"
    flags = ["-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++"] + flags + [src, "-o", str(exe)])
    p = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()
    assert "attn plans: validation order, the O-overlap rule, the 2^40 limits, the fused class, both routes' edges and grids hold" in p.stdout.decode()
    _check_against_mirror(str(exe))
    built = os.path.join(PKG, "tools", "attn_plan_check")
    assert os.path.exists(built) and os.access(built, os.X_OK), "run __graft_entry__.build() first"
    _check_against_mirror(built)


def test_the_mirror_of_the_class_the_routes_and_the_names():
    d = A.desc_of(A.CLASS_BOUND_CASE)
    assert A.fused_class(d) and A.lds_bytes(d) == 1024 + 32 * (4096 + 16) + 12288 == 144896 <= A.LDS_MAX
    assert not A.fused_class(dict(d, tk=4097)) and not A.fused_class(dict(d, d=257, ldq=272, ldk=272)) and not A.fused_class(dict(d, ldv=40))
    d = A.desc_of(A.AttnCase("r", 33, 64, 64, 32))
    assert A.fast_logits(d, 1024.0) and not A.fast_logits(d, np.nextafter(np.float32(1024.0), np.float32(2000.0)))
    assert not A.fast_logits(dict(d, q_dt=A.U8), 1024.0) and A.fast_logits(dict(d, q_dt=A.U8), 512.0)
    assert A.fast_context(d, [500.0]) and not A.fast_context(d, [520.0]) and not A.fast_context(d, [float("nan")])
    assert not A.fast_logits(dict(d, round_mode=1), 1.0) and not A.fast_context(dict(d, round_mode=1), [1.0])
    assert A.kernel_name(A.CLASS_BOUND_CASE, A.FUSED, 1, 0) == "attn_fused<s8,s8> fast/exact"
    assert A.kernel_name(A.GRID_CAP_CASE, A.CHAIN, 0, 1) == "attn_chain<u8,s8> exact/fast"
    assert A.auto_path(d) == A.CHAIN and A.auto_path(dict(d, force_path=A.FUSED)) == A.FUSED
    paths = [A.auto_path(A.desc_of(c)) for c, _ in A.auto_cases()]
    assert paths == [p for _, p in A.auto_cases()] and paths.count(A.FUSED) == 2 and len(paths) == 11
    swin, vit, detr = (A.desc_of(A.AttnCase("p", t, t, dd, dd, batch=b, **{w + "_strides": R.attention_strides(b[0], b[1], t, dd) for w in "qkvo"}))
                       for t, dd, b in ((49, 32, (64, 3)), (197, 64, (8, 12)), (850, 32, (2, 8))))
    assert A.auto_path(swin) == A.auto_path(vit) == A.auto_path(detr) == A.FUSED          # the measured wins
    nl = A.desc_of(A.AttnCase("p", 4096, 4096, 256, 256, batch=(4, 1)))
    assert A.fused_class(nl) and A.strips(nl) == 512 and A.auto_path(nl) == A.CHAIN       # the measured loss
    assert [A.kparts(dict(d, dv=v)) for v in (1, 32, 33, 64, 65, 96, 97, 128, 130)] == [4, 4, 2, 2, 1, 1, 1, 1, 1]


# ---- 4. descriptor and build checks -------------------------------------------------------------------------------------------
def _create(d):
    desc = capi.AttnDesc()
    for k, v in d.items():
        setattr(desc, k, v)
    h = ctypes.c_void_p()
    rc = capi.lib().dfx_attn_create(ctypes.byref(desc), ctypes.byref(h))
    msg = capi.lib().dfx_last_error().decode()
    if rc == 0:
        assert capi.lib().dfx_attn_destroy(h) == 0
    else:
        assert not h.value
    return rc, msg


def test_validation_order_through_the_library_needs_no_device():
    """every DFX_ERR_INVALID clause at the last value it admits and the first it rejects, through dfx_attn_create; INVALID
    before UNSUPPORTED; "no HIP device" only for a valid descriptor"""
    base = A.desc_of(A.AttnCase("v", 33, 37, 40, 35, batch=(2, 3)))
    heads = A.desc_of([c for c in A.batch_cases() if c.name == "heads"][0])

    def admitted(d):
        rc, msg = _create(d)
        assert rc in (0, NO_DEVICE) and A.validate(d) == 0, (d, rc, msg)

    def refused(d, code, word):
        rc, msg = _create(d)
        assert rc == code == A.validate(d) and word in msg, (d, rc, msg)

    admitted(base)
    for key in ("batch0", "batch1", "tq", "tk", "d"):
        admitted(dict(base, **{key: 1}))
        refused(dict(base, **{key: 0}), INVALID, "non-positive")
    admitted(dict(base, dv=1))
    refused(dict(base, dv=0), INVALID, "non-positive")
    one = dict(base, batch0=1, batch1=1)
    admitted(dict(one, tq=R.MN_MAX, tk=1, d=1, dv=1, ldo=1, force_path=A.FUSED))   # (a fused handle allocates no L / P at create)
    refused(dict(one, tq=R.MN_MAX + 1, tk=1, d=1, dv=1, ldo=1), INVALID, "2^31 - 32")
    big = R.up16(R.KMAX)
    admitted(dict(one, d=R.KMAX, ldq=big, ldk=big))
    refused(dict(one, d=R.KMAX + 1, ldq=big, ldk=big), INVALID, "65025")
    admitted(dict(one, tk=R.KMAX))                                                 # the context product's K, not dfx_head's 65535
    refused(dict(one, tk=R.KMAX + 1), INVALID, "65025")
    refused(dict(one, tk=65535), INVALID, "65025")
    for key, good, bad, word in (("q_dt", (A.U8, A.S8), (0, A.F32, A.S32, 5), "q dtype"), ("dst_dt", A.DST_ROTATION, (0, 5), "dst dtype"),
                                 ("round_mode", (0, 1), (-1, 2), "round mode"), ("nscales", (1, 35), (0, 34, 36), "scales"),
                                 ("force_path", (-1, 0, 1), (-2, 2), "force_path")):
        for v in good:
            admitted(dict(base, **{key: v}))
        for v in bad:
            refused(dict(base, **{key: v}), INVALID, word)
    for key, word in (("k_dt", "k dtype"), ("v_dt", "v dtype")):
        for v in (0, A.F32, A.S32, 5):
            refused(dict(base, **{key: v}), INVALID, word)
        refused(dict(base, **{key: A.U8}), UNSUPPORTED, "u8 K / V")
        refused(dict(base, **{key: A.U8, "ldo": 34}), INVALID, "ldo")              # invalid is reported before unsupported
    admitted(dict(base, prob_scale=3.0e38))
    for v in (float("inf"), float("-inf"), float("nan")):
        refused(dict(base, prob_scale=v), INVALID, "prob_scale")
    for key, at, word in (("ldq", 40, "ldq"), ("ldk", 40, "ldk"), ("ldv", 35, "ldv"), ("ldo", 35, "ldo")):
        d = dict(base, **{key: at})
        if key == "ldo":
            d.update(o_s1=33 * 35, o_s0=3 * 33 * 35)
        admitted(d)
        refused(dict(base, **{key: at - 1}), INVALID, word)
    for key in ("q_s0", "q_s1", "k_s0", "k_s1", "v_s0", "v_s1"):
        admitted(dict(base, **{key: 0}))                                            # a broadcast
        refused(dict(base, **{key: -1}), INVALID, "negative")
    for key in ("o_s0", "o_s1"):
        refused(dict(base, **{key: -1}), INVALID, "negative")
        refused(dict(base, **{key: 0}), INVALID, "overlap")                         # never on O
        refused(dict(base, **{key: base[key] - 1}), INVALID, "overlap")
    admitted(dict(base, o_s0=base["o_s0"] + 1))
    admitted(heads)                                                                 # the interleaved-heads layout
    refused(dict(heads, o_s1=A.D - 1), INVALID, "overlap")
    refused(dict(heads, ldo=A.HEADS * A.D - 1), INVALID, "overlap")
    span_q = R.span(2, 3, 0, base["q_s1"], base["ldq"], 33, 40)
    admitted(dict(base, q_s0=2 ** 40 - 1 - span_q))
    refused(dict(base, q_s0=2 ** 40 - span_q), INVALID, "2^40")
    refused(dict(base, v_s0=2 ** 62), INVALID, "2^40")
    refused(dict(base, o_s0=2 ** 40), INVALID, "2^40")
    refused(dict(one, tq=TQ_EDGE, tk=R.KMAX), INVALID, "logits")
    # a forced fused path outside its class
    for key in ("ldq", "ldk", "ldv", "q_s0", "q_s1", "k_s0", "k_s1", "v_s0", "v_s1"):
        d = dict(base, force_path=A.FUSED)
        admitted(d)
        d[key] += 8
        refused(d, UNSUPPORTED, "class")
        admitted(dict(d, force_path=A.CHAIN))
        admitted(dict(d, force_path=-1))
    admitted(dict(one, force_path=A.FUSED, d=256, ldq=256, ldk=256))
    refused(dict(one, force_path=A.FUSED, d=257, ldq=272, ldk=272), UNSUPPORTED, "class")
    admitted(dict(one, force_path=A.FUSED, tk=4096))
    refused(dict(one, force_path=A.FUSED, tk=4097), UNSUPPORTED, "class")
    lib = capi.lib()
    assert lib.dfx_attn_create(None, None) == INVALID
    assert lib.dfx_attn_set_table(None, None) == INVALID
    assert lib.dfx_attn_set_scales(None, 1.0, None) == INVALID
    assert lib.dfx_attn_submit(None, None, None, None, None, None) == INVALID
    assert lib.dfx_attn_query(None, None) == INVALID
    assert lib.dfx_debug_attn_launches(None) == INVALID
    assert lib.dfx_attn_destroy(None) == 0
    assert "null" in lib.dfx_last_error().decode()


def test_valid_descriptors_and_no_cpu_fallback():
    import torch
    base = A.desc_of(A.AttnCase("v", 33, 37, 40, 35, batch=(2, 3)))
    for d in (base, dict(base, force_path=A.FUSED), dict(base, force_path=A.CHAIN)):
        rc, msg = _create(d)
        if torch.cuda.is_available():
            assert rc == 0, (d, msg)
        else:
            assert rc == NO_DEVICE and "no HIP device" in msg, (d, rc, msg)
    if not torch.cuda.is_available():
        with pytest.raises(dfa.DfxError) as e:
            dfa.Attention((2, 3), 33, 37, 40, 35)
        assert "dfx error 4" in str(e.value) and "no HIP device" in str(e.value)


def test_attn_structs_match_the_header(tmp_path):
    """dfx_attn_desc / dfx_attn_info compiled by gcc have the sizes and field offsets of the ctypes mirrors"""
    pairs = {"dfx_attn_desc": capi.AttnDesc, "dfx_attn_info": capi.AttnInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dfx.h"', 'int main(void) {']
    for cname, ct in pairs.items():
        lines.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in ct._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    for name in ("DFX_ATTN_FUSED", "DFX_ATTN_CHAIN", "DFX_VERSION"):
        lines.append('printf("enum %s %%d\\n", %s);' % (name, name))
    lines.append('printf("dfx_bmm_desc size %zu\\n", sizeof(dfx_bmm_desc));')
    lines.append("return 0; }")
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = {}
    for ln in subprocess.check_output([str(exe)]).decode().splitlines():
        a, b, c = ln.split()
        seen[(a, b)] = int(c)
    for cname, ct in pairs.items():
        assert seen[(cname, "size")] == ctypes.sizeof(ct), cname
        for fname, _ in ct._fields_:
            assert seen[(cname, fname)] == getattr(ct, fname).offset, (cname, fname)
    assert [n for n, _ in capi.AttnDesc._fields_] == list(A.FIELDS)
    assert seen[("enum", "DFX_ATTN_FUSED")] == capi.ATTN_FUSED == A.FUSED == 0 and seen[("enum", "DFX_ATTN_CHAIN")] == capi.ATTN_CHAIN == A.CHAIN == 1
    assert capi.ATTN_AUTO == -1 and seen[("enum", "DFX_VERSION")] == 100
    assert ctypes.sizeof(capi.AttnDesc) == 160
    assert ctypes.sizeof(capi.BmmDesc) == seen[("dfx_bmm_desc", "size")]              # the others are untouched


def test_library_exports_the_attn_entry_points():
    L = capi.lib()
    for s in ("dfx_attn_create", "dfx_attn_set_table", "dfx_attn_set_scales", "dfx_attn_submit", "dfx_attn_query", "dfx_attn_destroy",
              "dfx_debug_attn_launches"):
        assert s in dfa.declared_symbols() and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s                                # bound with a signature
    assert not [s for s in dfa.declared_symbols() if not hasattr(L, s)]
    for name in ("Attention", "AttnDesc", "AttnInfo", "ATTN_AUTO", "ATTN_FUSED", "ATTN_CHAIN", "attn_launches", "attention_strides", "softmax_table"):
        assert hasattr(dfa, name), name
    for what in ("set_table", "set_scales", "submit", "info", "requant", "close"):
        assert callable(getattr(dfa.Attention, what)), what
    capi.set_tuning("DFX_ATTN_GRID", "1")                                           # known to the library
    capi.set_tuning("DFX_ATTN_GRID", None)
    with pytest.raises(dfa.DfxError):
        capi.set_tuning("DFX_ATTN_STRIPS", "1")
    for tool in ("attn_check", "bench_attn", "attn_plan_check"):
        assert os.access(os.path.join(PKG, "tools", tool), os.X_OK), "run __graft_entry__.build() first: " + tool
