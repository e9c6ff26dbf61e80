"""CPU-only checks of the batched int8 matrix product (dfx_bmm_*): the numpy reference the GPU tests compare against
(tests/bmm_ref.py) equals an independent pure-Python witness and, at batch 1 / NT / u8 A, the fully-connected op's reference
(fc_ref, pinned to the C oracle by tests/test_fc_cpu.py); the case tables hold the regimes they are meant to hold; the C ABI
validates descriptors in the documented order before it touches a device, every clause at the last value it admits and the
first it rejects; the ctypes mirrors match the header; the op's host-side plan (csrc/bmm_plan.h) agrees with its Python mirror
and is clean under the host sanitizers as a stand-alone program."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

import bmm_ref as R
import fc_ref as F

dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-fusion_amd")
INVALID, UNSUPPORTED, HIP, NO_DEVICE, STATE = 1, 2, 3, 4, 5
SAT_CAP = 0.10        # at most this share of a case's outputs on a saturation bound, except in the cases built to saturate


@pytest.fixture(autouse=True)
def the_package_knows_the_op():
    """every test of this file is about dfx_bmm: the reference checks too stand on the package that binds it"""
    assert hasattr(dfa, "MatMul") and dfa.BMM_GENERIC == R.GENERIC and dfa.BMM_MFMA == R.MFMA
    assert "dfx_bmm_create" in dfa.declared_symbols()


# ---- 1. independent formulations -------------------------------------------------------------------------------------------
def _small(case):
    return case.g * case.m * case.n * case.k <= 60000


WITNESSED = [c for c in R.table() if _small(c)][::7] + R.batch_cases()[:2] + [c for c in R.batch_cases() if c.name.startswith("heads")][:2]


@pytest.mark.parametrize("group", [tuple(WITNESSED[i::8]) for i in range(8)], ids=lambda g: "w%d" % len(g))
def test_reference_equals_the_witness(group):
    assert dfa.BMM_GENERIC == R.GENERIC and dfa.BMM_MFMA == R.MFMA           # (the package knows the op at all)
    assert len(WITNESSED) > 100
    for case in group:
        data = R.generate(case)
        got, want = R.reference(case, data), R.witness(case, data)
        assert got.dtype == want.dtype == np.uint8 and got.size == R.storage_elems(case, "c") * R.SIZE_OF[case.dst_dt]
        assert np.array_equal(got, want), case.ident()


def test_special_cases_equal_the_witness():
    for case, data in R.tie_cases() + [(c, d) for c, d in R.compensation_cases() if c.k == 200][::5]:
        assert np.array_equal(R.reference(case, data), R.witness(case, data)), case.ident()
    for trans_b in (True, False):
        case, data, want = R.lane_map_case(trans_b)
        assert np.array_equal(R.values(case, data)[0, 0], want) and not np.array_equal(want, want.T)


def test_hand_computed_values():
    f = R.finish
    acc = np.array([3, -3, 5, -5, 255, 511, -257], dtype=np.int64)
    assert f(acc, [0.5], R.S32, False, 0).tolist() == [2, -2, 2, -2, 128, 256, -128]        # ties to even
    assert f(acc, [0.5], R.S32, False, 1).tolist() == [1, -2, 2, -3, 127, 255, -129]        # floor
    assert f(acc, [0.5], R.S8, False, 0).tolist() == [2, -2, 2, -2, 127, 127, -128]
    assert f(acc, [0.5], R.U8, False, 0).tolist() == [2, 0, 2, 0, 128, 255, 0]              # u8 implies the ReLU
    assert f(acc, [0.5], R.S8, True, 0).tolist() == [2, 0, 2, 0, 127, 127, 0]
    inf, nan = float("inf"), float("nan")
    assert f(acc[:2], [inf], R.S32, False, 0).tolist() == [-2 ** 31] * 2
    assert f(acc[:2], [inf], R.S8, False, 0).tolist() == [-128, -128] and f(acc[:2], [inf], R.U8, False, 0).tolist() == [255, 0]
    assert f(acc[:2], [nan], R.U8, False, 0).tolist() == [255, 255] and f(acc[:2], [nan], R.S32, True, 0).tolist() == [-2 ** 31] * 2
    assert np.isnan(f(acc[:1], [nan], R.F32, True, 0)).all()                                # vmaxps lets NaN pass
    assert f(np.array([2 ** 31 - 1]), [1.0], R.S32, False, 0).tolist() == [-2 ** 31]        # float(2^31 - 1) = 2^31: out of range
    assert f(np.array([0]), [-1.0], R.F32, False, 0).view(np.uint32).tolist() == [0x80000000]   # -0 without the ReLU ...
    assert f(np.array([0]), [-1.0], R.F32, True, 0).view(np.uint32).tolist() == [0x80000000]    # ... and through it: 0 > -0 is false
    # pad columns never take part
    case = R.BmmCase("pad", 2, 3, 5, a_dt=R.U8, dst_dt=R.S32, scale=1.0)
    data = R.generate(case)
    a = data["a"].reshape(2, 16)
    assert (a[:, 5:] == 0xFF).all() and (data["b"].view(np.uint8).reshape(3, 16)[:, 5:] != 0).all()
    want = a[:, :5].astype(np.int64) @ data["b"].reshape(3, 16)[:, :5].astype(np.int64).T
    assert np.array_equal(R.values(case, data)[0, 0], want)


@pytest.mark.parametrize("k,m,n", R.FC_TWIN)
def test_reference_equals_the_fully_connected_reference(k, m, n):
    """batch 1, NT, u8 A: fc_ref's own route with w = B, ih = iw = 1, no bias; all four dst dtypes, both round modes"""
    for dst in R.DST_ROTATION:
        for rm in (0, 1):
            for relu in (False, True):
                case = R.BmmCase("fc", m, n, k, trans_b=True, a_dt=R.U8, dst_dt=dst, relu=relu, rm=rm, c_ld=n, per_channel=bool(rm), seed=38000 + k + m + n)
                data = R.generate(case)
                fc = F.FcCase("twin", m, k, 1, 1, n, dst_dt=dst, bia_dt=F.UNDEF, relu=relu, rm=rm, per_channel=bool(rm))
                want = F.fc_ref(fc, dict(src=data["a"].reshape(m, 1, 1, k), w=data["b"].reshape(n, k, 1, 1), bia=None, scales=data["scales"]))
                got = R.values(case, data)[0, 0]
                assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), case.ident()


# ---- 2. the regimes the tables are meant to hold ------------------------------------------------------------------------------
def test_tables_hold_their_regimes():
    """for every table case the reference output is neither all-saturated nor all-zero; at most 10 % of a case's outputs sit on
    a saturation bound (u8 255, s8 -128 / 127, s32 +-2^31), except in the cases built to saturate; a ReLU's zeros are the op's own
    result, but at least a quarter of a ReLU case's outputs must be non-zero wherever it has 64 outputs or more"""
    t = R.table()
    assert len(t) == 2 * 2 * 36 * 9 + len(R.batch_cases()) + 8 + 1
    built = 0
    for case in t:
        vals = R.values(case, R.generate(case))
        sat = R.saturated_fraction(case, vals)
        if case.saturating:
            built += 1
            assert sat > 0.4 or case.dst_dt == R.F32, case.ident()
            continue
        assert sat <= SAT_CAP, (case.ident(), sat)
        if vals.size >= 64:
            assert (vals != 0).mean() >= 0.25, (case.ident(), float((vals != 0).mean()))
            assert len(np.unique(vals)) > 2, case.ident()                          # neither constant nor two-valued
    assert built == 8
    for case, data in R.tie_cases():
        assert R.saturated_fraction(case, R.values(case, data)) <= SAT_CAP, case.ident()
    g = R.shape_grid()
    assert {(c.m, c.n, c.k) for c in g} == {(m, n, k) for m in R.GRID_MN for n in R.GRID_MN for k in R.GRID_K}
    for trans_b in (True, False):
        for a_dt in (R.U8, R.S8):
            here = [c for c in g if c.trans_b == trans_b and c.a_dt == a_dt]
            assert {c.dst_dt for c in here} == set(R.DST_ROTATION) and {c.rm for c in here} == {0, 1}
            assert {c.relu for c in here} == {True, False} and {c.per_channel for c in here} == {True, False}
            assert {c.strides("c")[2] % 4 == 0 for c in here} == {True, False}
    assert all(R.mfma_class(R.desc_of(c)) for c in t)
    assert R.tiles(R.desc_of(R.GRID_CAP_CASE)) >= 7 * 4


# ---- 3. the plan: the stand-alone program against the Python mirror, and under the host sanitizers -------------------------------
FIELDS = ("batch0", "batch1", "m", "n", "k", "trans_b", "a_dt", "b_dt", "dst_dt", "relu", "round_mode", "nscales", "force_path",
          "a_s0", "a_s1", "lda", "b_s0", "b_s1", "ldb", "c_s0", "c_s1", "ldc")


def _variants():
    """descriptors around every clause: table cases, then one field at a time moved off a valid descriptor"""
    out = [R.desc_of(c, fp) for c in R.table()[::41] + R.batch_cases() for fp in (-1, R.MFMA, R.GENERIC)]
    base = R.desc_of(R.BmmCase("v", 33, 37, 40, batch=(2, 3)))
    for key, vals in (("batch0", (0, 1)), ("batch1", (0, 1)), ("m", (0, 1)), ("n", (0, 1)), ("k", (0, 1, R.KMAX, R.KMAX + 1)),
                      ("trans_b", (-1, 0, 1, 2)), ("a_dt", range(0, 6)), ("b_dt", range(0, 6)), ("dst_dt", range(0, 6)),
                      ("round_mode", (-1, 0, 1, 2)), ("nscales", (0, 1, 36, 37, 38)), ("force_path", (-2, -1, 0, 1, 2)),
                      ("lda", (39, 40, 41, 48)), ("ldb", (39, 40, 48)), ("ldc", (36, 37)), ("a_s0", (-1, 0, 8, 16)), ("a_s1", (-16, 0, 24)),
                      ("b_s0", (-1, 0)), ("b_s1", (-1, 0, 8)), ("c_s0", (-1, 0, 3 * 33 * 40 - 1, 3 * 33 * 40, 2 ** 40)), ("c_s1", (-1, 0, 33 * 40 - 1, 33 * 40)),
                      ("a_s0", (2 ** 40 - 2 * 33 * 48 - 33 * 48 + 7, 2 ** 40, 2 ** 62))):
        for v in vals:
            for fp in (-1, R.MFMA):
                d = dict(base, force_path=fp)
                d[key] = v
                if key in ("n",) and d["nscales"] != 1:
                    d["nscales"] = v
                out.append(d)
    out.append(dict(base, ldc=40, n=37, c_s1=33 * 40, c_s0=3 * 33 * 40))
    one = dict(base, batch0=1, batch1=1)
    out += [dict(one, m=R.MN_MAX), dict(one, m=R.MN_MAX + 1), dict(one, m=1, n=R.MN_MAX, ldc=R.MN_MAX, trans_b=1),
            dict(one, m=1, n=R.MN_MAX + 1, ldc=R.MN_MAX + 1, trans_b=1)]
    # the auto rule's edges: the Swin point, one less of each bound, few tiles under a deep K
    for t in (0, 1):
        n, k = (49, 32) if t else (32, 49)
        for kw in (dict(), dict(m=48), dict(batch0=63), dict(batch0=1, batch1=1, k=R.KMAX), dict(batch0=1, batch1=1, m=384, n=1024, k=4096),
                   dict(batch0=1, batch1=1, m=384, n=992, k=4096)):
            c = dict(m=49, n=n, k=k, batch0=64, batch1=3)
            c.update(kw)
            out.append(R.desc_of(R.BmmCase("auto", c["m"], c["n"], c["k"], trans_b=bool(t), batch=(c["batch0"], c["batch1"]))))
    # interleaved heads: accepted; c_s1 = d - 1: rejected
    heads = R.desc_of([c for c in R.batch_cases() if c.name == "heads-pv"][0])
    out += [heads, dict(heads, c_s1=R.D - 1), dict(heads, ldc=R.HEADS * R.D - 1), dict(heads, c_s0=heads["c_s0"] - 1), dict(heads, trans_b=0, k=R.KMAX + 1)]
    return out


def _plan_lines(exe, descs, cus, cap):
    text = "".join(" ".join(str(int(d[f])) for f in FIELDS) + " %d %d\n" % (cus, cap) for d in descs)
    p = subprocess.run([exe, "-"], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()
    lines = p.stdout.decode().splitlines()
    assert len(lines) == len(descs), p.stdout.decode()[-2000:]
    return lines


def _check_against_mirror(exe):
    descs = _variants()
    seen = set()
    for cus, cap in ((256, 0), (8, 0), (256, 3)):
        for d, line in zip(descs, _plan_lines(exe, descs, cus, cap)):
            got = [int(x) for x in line.split()]
            rc = R.validate(d)
            seen.add(rc)
            assert got[0] == rc, (d, line)
            if rc == INVALID:
                continue
            brows, bcols = (d["n"], d["k"]) if d["trans_b"] else (d["k"], d["n"])
            want = [rc, int(R.mfma_class(d)), -1 if rc else R.auto_path(d), R.tiles(d), R.planned_grid(d, R.MFMA, cus, cap),
                    R.planned_grid(d, R.GENERIC, cus, cap), R.lds_bytes(d, R.MFMA), R.algorithmic_ops(d), R.algorithmic_bytes(d),
                    R.span(d["batch0"], d["batch1"], d["a_s0"], d["a_s1"], d["lda"], d["m"], d["k"]),
                    R.span(d["batch0"], d["batch1"], d["b_s0"], d["b_s1"], d["ldb"], brows, bcols),
                    R.span(d["batch0"], d["batch1"], d["c_s0"], d["c_s1"], d["ldc"], d["m"], d["n"])]
            assert got == want, (d, got, want)
    assert seen == {0, INVALID, UNSUPPORTED}


def test_bmm_plan_check_agrees_with_the_mirror_and_is_clean_under_the_host_sanitizers(tmp_path):
    """tools/bmm_plan_check.cc, a stand-alone host program over csrc/bmm_plan.h, built with the flags of the host Makefile's
    SAN=1 rule (ASan + UBSan) into a scratch directory and run directly: its self-check, then the descriptors of the Python
    mirror through its stdin mode.  Nothing is loaded into Python."""
    src = os.path.join(PKG, "tools", "bmm_plan_check.cc")
    assert os.path.exists(src), "tools/bmm_plan_check.cc is missing"
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert "$(TOOLS)/bmm_plan_check: $(TOOLS)/bmm_plan_check.cc ../csrc/bmm_plan.h" in mk
    exe = tmp_path / "bmm_plan_check"
    flags = ["-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++"] + flags + [src, "-o", str(exe)])
    p = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()
    assert "bmm plans: validation order, the C-overlap rule, the 2^40 limit, classes, the route's edge and grids hold" in p.stdout.decode()
    _check_against_mirror(str(exe))
    built = os.path.join(PKG, "tools", "bmm_plan_check")
    assert os.path.exists(built) and os.access(built, os.X_OK), "run __graft_entry__.build() first"
    _check_against_mirror(built)


def test_the_mirror_of_the_overlap_rule_and_of_the_route():
    assert R.c_disjoint(32, 37, 3, 2, 96, 32, 37 * 96) and not R.c_disjoint(32, 37, 3, 2, 96, 31, 37 * 96)
    assert not R.c_disjoint(32, 37, 3, 2, 96, 0, 37 * 96) and R.c_disjoint(32, 37, 1, 1, 32, 0, 0)
    assert R.c_disjoint(1, 1, 1, 1, 1, 0, 0) and not R.c_disjoint(4, 1, 1, 2, 4, 0, 3) and R.c_disjoint(4, 1, 1, 2, 4, 0, 4)
    d = R.desc_of(R.BmmCase("r", 33, 37, 64, a_dt=R.S8))
    assert R.fast_ok(d, [1024.0]) and not R.fast_ok(d, [np.nextafter(np.float32(1024.0), np.float32(2000.0))])
    assert not R.fast_ok(d, [float("inf")]) and not R.fast_ok(d, [float("nan")]) and not R.fast_ok(dict(d, round_mode=1), [1.0])
    assert R.attention_strides(2, 3, 37, 32) == dfa.attention_strides(2, 3, 37, 32) == dfa.attention_strides(2, 3, 37, 32, 96) == (37 * 96, 32, 96)
    assert dfa.attention_strides(8, 12, 197, 64, 768) == (197 * 768, 64, 768)
    with pytest.raises(ValueError):
        dfa.attention_strides(2, 3, 37, 32, 95)


# ---- 4. descriptor and build checks -------------------------------------------------------------------------------------------
def _create(d):
    desc = capi.BmmDesc()
    for k, v in d.items():
        setattr(desc, k, v)
    h = ctypes.c_void_p()
    rc = capi.lib().dfx_bmm_create(ctypes.byref(desc), ctypes.byref(h))
    msg = capi.lib().dfx_last_error().decode()
    if rc == 0:
        assert capi.lib().dfx_bmm_destroy(h) == 0
    else:
        assert not h.value
    return rc, msg


def test_validation_order_through_the_library_needs_no_device():
    """every DFX_ERR_INVALID clause at the last value it admits and the first it rejects, through dfx_bmm_create; INVALID
    before UNSUPPORTED; "no HIP device" only for a valid descriptor"""
    base = R.desc_of(R.BmmCase("v", 33, 37, 40, batch=(2, 3)))
    heads = R.desc_of([c for c in R.batch_cases() if c.name == "heads-pv"][0])

    def admitted(d):
        rc, msg = _create(d)
        assert rc in (0, NO_DEVICE) and R.validate(d) == 0, (d, rc, msg)

    def refused(d, code, word):
        rc, msg = _create(d)
        assert rc == code == R.validate(d) and word in msg, (d, rc, msg)

    admitted(base)
    for key in ("batch0", "batch1", "m", "k"):
        admitted(dict(base, **{key: 1}))
        refused(dict(base, **{key: 0}), INVALID, "non-positive")
    admitted(dict(base, n=1, ldc=1))
    admitted(dict(base, batch0=1, batch1=1, m=R.MN_MAX))                            # m, n rounded up to 32 fit an int
    refused(dict(base, batch0=1, batch1=1, m=R.MN_MAX + 1), INVALID, "2^31 - 32")
    admitted(dict(base, batch0=1, batch1=1, m=1, n=R.MN_MAX, ldc=R.MN_MAX))
    refused(dict(base, batch0=1, batch1=1, m=1, n=R.MN_MAX + 1, ldc=R.MN_MAX + 1), INVALID, "2^31 - 32")
    refused(dict(base, n=0), INVALID, "non-positive")
    big = dict(base, m=33, n=33, batch0=1, batch1=1)
    admitted(dict(big, k=R.KMAX, lda=R.KMAX + 15, ldb=R.KMAX + 15))
    refused(dict(big, k=R.KMAX + 1, lda=R.KMAX + 15, ldb=R.KMAX + 15), INVALID, "65025")
    for key, good, bad, word in (("trans_b", (0, 1), (-1, 2), "trans_b"), ("a_dt", (R.U8, R.S8), (0, R.F32, R.S32, 5), "a dtype"),
                                 ("dst_dt", R.DST_ROTATION, (0, 5), "dst dtype"), ("round_mode", (0, 1), (-1, 2), "round mode"),
                                 ("nscales", (1, 37), (0, 36, 38), "scales"), ("force_path", (-1, 0, 1), (-2, 2), "force_path")):
        for v in good:
            admitted(dict(base, **{key: v}))
        for v in bad:
            refused(dict(base, **{key: v}), INVALID, word)
    for v in (0, R.F32, R.S32, 5):
        refused(dict(base, b_dt=v), INVALID, "b dtype")
    refused(dict(base, b_dt=R.U8), UNSUPPORTED, "u8 B")
    refused(dict(base, b_dt=R.U8, ldc=36), INVALID, "ldc")                          # invalid is reported before unsupported
    admitted(dict(base, lda=40))
    refused(dict(base, lda=39), INVALID, "lda")
    admitted(dict(base, ldb=40))
    refused(dict(base, ldb=39), INVALID, "ldb below k")
    admitted(dict(base, trans_b=0, ldb=37))
    refused(dict(base, trans_b=0, ldb=36), INVALID, "ldb below n")
    admitted(dict(base, ldc=37, c_s1=33 * 37, c_s0=3 * 33 * 37))
    refused(dict(base, ldc=36), INVALID, "ldc")
    for key in ("a_s0", "a_s1", "b_s0", "b_s1"):
        admitted(dict(base, **{key: 0}))                                            # a broadcast
        refused(dict(base, **{key: -1}), INVALID, "negative")
    for key in ("c_s0", "c_s1"):
        refused(dict(base, **{key: -1}), INVALID, "negative")
        refused(dict(base, **{key: 0}), INVALID, "overlap")                         # never on C
        refused(dict(base, **{key: base[key] - 1}), INVALID, "overlap")
    admitted(dict(base, c_s0=base["c_s0"] + 1))
    admitted(heads)                                                                 # the interleaved-heads layout
    assert (heads["n"], heads["c_s1"], heads["ldc"], heads["c_s0"]) == (R.D, R.D, R.HEADS * R.D, R.T * R.HEADS * R.D)
    refused(dict(heads, c_s1=R.D - 1), INVALID, "overlap")
    refused(dict(heads, ldc=R.HEADS * R.D - 1), INVALID, "overlap")
    # an index range that reaches 2^40 elements
    span_a = R.span(2, 3, 0, base["a_s1"], base["lda"], 33, 40)
    admitted(dict(base, a_s0=2 ** 40 - 1 - span_a))
    refused(dict(base, a_s0=2 ** 40 - span_a), INVALID, "2^40")
    refused(dict(base, b_s0=2 ** 62), INVALID, "2^40")
    refused(dict(base, c_s0=2 ** 40), INVALID, "2^40")
    # a forced MFMA path outside its class
    for key in ("lda", "ldb", "a_s0", "a_s1", "b_s0", "b_s1"):
        d = dict(base, force_path=R.MFMA)
        admitted(d)
        d[key] += 8
        refused(d, UNSUPPORTED, "class")
        admitted(dict(d, force_path=R.GENERIC))
        admitted(dict(d, force_path=-1))
    lib = capi.lib()
    assert lib.dfx_bmm_create(None, None) == INVALID
    assert lib.dfx_bmm_set_scales(None, None) == INVALID
    assert lib.dfx_bmm_submit(None, None, None, None, None) == INVALID
    assert lib.dfx_bmm_query(None, None) == INVALID
    assert lib.dfx_debug_bmm_launches(None) == INVALID
    assert lib.dfx_debug_bmm_requant(None, None) == INVALID
    assert lib.dfx_bmm_destroy(None) == 0
    assert "null" in lib.dfx_last_error().decode()


def test_valid_descriptors_and_no_cpu_fallback():
    import torch
    base = R.desc_of(R.BmmCase("v", 33, 37, 40, batch=(2, 3)))
    for d in (base, dict(base, force_path=R.MFMA), dict(base, trans_b=0)):
        rc, msg = _create(d)
        if torch.cuda.is_available():
            assert rc == 0, (d, msg)
        else:
            assert rc == NO_DEVICE and "no HIP device" in msg, (d, rc, msg)
    if not torch.cuda.is_available():
        with pytest.raises(dfa.DfxError) as e:
            dfa.MatMul((2, 3), 33, 37, 40, scales=[1.0])
        assert "dfx error 4" in str(e.value) and "no HIP device" in str(e.value)


def test_bmm_structs_match_the_header(tmp_path):
    """dfx_bmm_desc / dfx_bmm_info compiled by gcc have the sizes and field offsets of the ctypes mirrors"""
    pairs = {"dfx_bmm_desc": capi.BmmDesc, "dfx_bmm_info": capi.BmmInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dfx.h"', 'int main(void) {']
    for cname, ct in pairs.items():
        lines.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in ct._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    for name in ("DFX_BMM_MFMA", "DFX_BMM_GENERIC", "DFX_VERSION"):
        lines.append('printf("enum %s %%d\\n", %s);' % (name, name))
    lines.append('printf("dfx_head_desc size %zu\\n", sizeof(dfx_head_desc));')
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
    assert [n for n, _ in capi.BmmDesc._fields_] == list(FIELDS)
    assert [n for n, _ in capi.BmmInfo._fields_] == ["path", "grid", "block", "lds_bytes", "device", "algorithmic_ops", "algorithmic_bytes",
                                                     "kernel_name"]
    assert seen[("enum", "DFX_BMM_MFMA")] == capi.BMM_MFMA == R.MFMA == 0 and seen[("enum", "DFX_BMM_GENERIC")] == capi.BMM_GENERIC == R.GENERIC == 1
    assert capi.BMM_AUTO == -1 and seen[("enum", "DFX_VERSION")] == 100
    assert ctypes.sizeof(capi.BmmDesc) == 128
    assert ctypes.sizeof(capi.HeadDesc) == seen[("dfx_head_desc", "size")]            # the others are untouched


def test_library_exports_the_bmm_entry_points():
    L = capi.lib()
    for s in ("dfx_bmm_create", "dfx_bmm_set_scales", "dfx_bmm_submit", "dfx_bmm_query", "dfx_bmm_destroy", "dfx_debug_bmm_launches",
              "dfx_debug_bmm_requant"):
        assert s in dfa.declared_symbols() and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s                                # bound with a signature
    assert not [s for s in dfa.declared_symbols() if not hasattr(L, s)]
    for name in ("MatMul", "BmmDesc", "BmmInfo", "BMM_AUTO", "BMM_MFMA", "BMM_GENERIC", "bmm_launches", "attention_strides"):
        assert hasattr(dfa, name), name
    for what in ("set_scales", "submit", "info", "requant", "close"):
        assert callable(getattr(dfa.MatMul, what)), what
    capi.set_tuning("DFX_BMM_GRID", "1")                                            # known to the library
    capi.set_tuning("DFX_BMM_GRID", None)
    with pytest.raises(dfa.DfxError):
        capi.set_tuning("DFX_BMM_TILES", "1")
