"""CPU-only checks of the logit bias of dfx_bmm / dfx_attn (dfx_bmm_set_bias, dfx_attn_set_bias): the numpy reference the GPU
tests compare against (tests/attn_bias_ref.py) equals its element-by-element witness on tiny cases; every case of the GPU
tables holds the regime it is meant to hold; the host-side plan (csrc/bias_plan.h) agrees with its Python mirror and is clean
under the host sanitizers as a stand-alone program (tools/bias_plan_check: layouts, the image, the scan, the routes); the
helper dfa.attention_bias builds what it documents; the ctypes mirror and prototypes match the header; the library exports
both entry points."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import attn_bias_ref as R
import attn_ref as A
import bmm_ref as B

dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-fusion_amd")
INVALID, UNSUPPORTED = 1, 2
SAT_CAP = 0.02        # at most this share of the UNMASKED logits on 127 / -128
CHANGED = 0.90        # at least this share of the logits differs from the unbiased ones


@pytest.fixture(autouse=True)
def the_package_knows_the_bias():
    """every test of this file is about the logit bias: the reference checks too stand on the package that binds it"""
    assert hasattr(dfa, "attention_bias") and hasattr(dfa, "LogitBiasDesc") and callable(getattr(dfa.MatMul, "set_bias", None))
    assert "dfx_bmm_set_bias" in dfa.declared_symbols() and "dfx_attn_set_bias" in dfa.declared_symbols()


# ---- 1. the reference against the witness -------------------------------------------------------------------------------------
TINY_BMM = [(B.BmmCase("tiny", 3, 5, 4, trans_b=True, a_dt=B.S8, dst_dt=B.S8, batch=(2, 3), seed=80000), R.Bias(periods=(2, 3), mask="random", seed=80001)),
            (B.BmmCase("tiny", 4, 3, 5, trans_b=False, a_dt=B.U8, dst_dt=B.U8, batch=(2, 2), rm=1, seed=80002), R.Bias(periods=(1, 2), one_row=True, seed=80003)),
            (B.BmmCase("tiny", 3, 4, 2, trans_b=True, a_dt=B.U8, dst_dt=B.S32, batch=(3, 1), per_channel=True, seed=80004),
             R.Bias(periods=(2, 1), strides=(40, 0, 7), mask="random", mask_value="ninf", seed=80005)),
            (B.BmmCase("tiny", 2, 6, 3, trans_b=False, a_dt=B.S8, dst_dt=B.F32, batch=(1, 2), relu=True, seed=80006), R.Bias(periods=(1, 1), seed=80007)),
            (B.BmmCase("tiny", 3, 4, 2, trans_b=True, a_dt=B.S8, dst_dt=B.S8, batch=(2, 2), scale=-0.01, seed=80008),
             R.Bias(periods=(2, 2), mask="random", mask_value="ninf", seed=80009))]


@pytest.mark.parametrize("case,bias", TINY_BMM, ids=lambda c: c.ident() if hasattr(c, "ident") else "b%d" % c.seed)
def test_bmm_reference_equals_the_witness(case, bias):
    data = B.generate(case)
    bd = R.make_bias(bias, case.m, case.n, data["scales"][0], R.acc_bound(case.a_dt, case.k))
    got, want = R.bmm_reference(case, data, bias, bd), R.bmm_witness(case, data, bias, bd)
    assert got.dtype == want.dtype == np.uint8 and np.array_equal(got, want), case.ident()
    assert not np.array_equal(got, B.reference(case, data)), case.ident()            # the bias shows
    if bias.mask_value == "ninf" and case.dst_dt == B.S8:                            # -128 whatever the sign of the scale
        vals = R.bmm_values(case, data, bias, bd)
        assert (vals[R.expand(bias, bd["masked"], case.batch, case.m)] == -128).all() and bd["masked"].any()


def test_attn_reference_equals_the_witness():
    for i, (case, bias) in enumerate(((A.AttnCase("tiny", 3, 5, 4, 3, q_dt=A.S8, dst_dt=A.S8, batch=(2, 2), seed=80100), R.Bias(periods=(2, 1), mask="random", seed=80101)),
                                      (A.AttnCase("tiny", 4, 6, 3, 2, q_dt=A.U8, dst_dt=A.S32, seed=80102), R.Bias(one_row=True, mask="keypad", mask_value="ninf", seed=80103)))):
        data = A.generate(case)
        bd = R.attn_bias_data(case, data, bias)
        assert np.array_equal(R.attn_reference(case, data, bias, bd), R.attn_witness(case, data, bias, bd)), case.ident()
        assert np.array_equal(R.attn_reference(case, data, None, None), A.reference(case, data))


# ---- 2. the regime of every case of the GPU tables ----------------------------------------------------------------------------
def test_attention_cases_hold_their_regimes():
    """per case, on the reference alone: at most 2 % of the unmasked logits on a saturation bound, at least 90 % of the logits
    changed by the bias, every masked logit -128, every row with an unmasked key (but the case built to have fully masked
    rows, whose rows are then uniform), O different from the unbiased O"""
    table = R.attn_table()
    assert len(table) == 10
    for case, bias in table:
        data = A.generate(case)
        bd = R.attn_bias_data(case, data, bias)
        logits, probs, o = R.attn_chain(case, data, bias, bd)
        plain = A.chain(case, data)
        lv = logits[:, :case.tk]
        masked = R.expand(bias, bd["masked"], case.batch, case.tq).reshape(-1, case.tk)
        assert masked.any() and (lv[masked] == -128).all(), case.ident()
        sat = float(((lv == 127) | (lv == -128))[~masked].mean())
        changed = float((lv != plain[0][:, :case.tk]).mean())
        assert sat <= SAT_CAP, (case.ident(), sat)
        assert changed >= CHANGED, (case.ident(), changed)
        full = masked.all(axis=1)
        if bias.mask == "row0":
            assert full.sum() == case.g and len(np.unique(probs[full, :case.tk])) == 1   # uniform over all tk keys
        else:
            assert not full.any(), case.ident()
        assert not np.array_equal(o, plain[2]), case.ident()
        assert R.attn_fast_logits(case, data, bias, bd)                                # the finite mask keeps the fast route provable
        ninf = R.with_ninf(bias)
        nd = R.attn_bias_data(case, data, ninf)
        assert not R.attn_fast_logits(case, data, ninf, nd)
        assert np.array_equal(R.attn_reference(case, data, ninf, nd), o), case.ident()   # -inf and the finite mask: the same bits


def test_matrix_product_cases_hold_their_regimes():
    """every case of the tables (none is built to saturate), whatever its dst type, ReLU and scales, on the f32 values in front of
    the ReLU and the store: at most 2 % of the unmasked elements leave dst's range, at least 90 % are changed by the bias; C
    differs from the unbiased C; on the s8 cases without ReLU and with one scale the stored values say the same and every masked
    element is -128; the tables cover what the issue lists"""
    tails, layouts = R.bmm_tail_cases(), R.bmm_layout_cases()
    assert len(tails) == 2 * 2 * 4 * 2
    assert {(c.trans_b, c.a_dt, c.dst_dt, c.strides("c")[2] % 4 == 0) for c, _ in tails} == \
        {(t, a, d, v) for t in (True, False) for a in (B.U8, B.S8) for d in B.DST_ROTATION for v in (True, False)}
    assert {b.periods for c, b in layouts if c.name == "periods"} == {(1, 1), (1, 3), (2, 1), (2, 3)}
    assert {c.name for c, _ in layouts} == {"periods", "gaps", "gaps-row", "shared", "n1", "m1", "ninf", "tiles"}
    for case, bias in R.bmm_table():
        data = B.generate(case)
        bd = R.make_bias(bias, case.m, case.n, data["scales"][0], R.acc_bound(case.a_dt, case.k))
        vals, plain = R.bmm_values(case, data, bias, bd), B.values(case, data)
        assert not np.array_equal(vals.view(np.uint8), plain.view(np.uint8)), case.ident()
        assert not np.isnan(bd["values"]).any() and (bias.strides is None or np.isnan(bd["table"]).any() or bias.strides[0] == 0)
        assert not case.saturating
        fb, fp = R.prestore(case, data, bias, bd), R.prestore(case, data, None, None)
        unmasked = ~R.expand(bias, bd["masked"], case.batch, case.m)
        assert unmasked.any() and np.isfinite(fb[unmasked]).all(), case.ident()
        assert float(R.prestore_saturates(case, fb)[unmasked].mean()) <= SAT_CAP, case.ident()
        assert float((fb != fp).mean()) >= CHANGED, case.ident()
        if case.dst_dt == B.S8 and not case.relu and not case.per_channel:
            masked = R.expand(bias, bd["masked"], case.batch, case.m)
            assert (vals[masked] == -128).all(), case.ident()
            assert float(((vals == 127) | (vals == -128))[~masked].mean()) <= SAT_CAP, case.ident()
            assert float((vals != plain).mean()) >= CHANGED, case.ident()


# ---- 3. the plan: the stand-alone program against the Python mirror, and under the host sanitizers ------------------------------
def _layouts():
    """(descriptor dict, layout dict) around every clause"""
    d = dict(batch0=4, batch1=3, m=33, n=37, k=40, a_dt=B.S8, round_mode=0, nscales=1)
    out = []
    for p0 in (0, 1, 2, 4, 5):
        for p1 in (0, 1, 3, 4):
            out.append((d, dict(period0=p0, period1=p1, s0=3 * 33 * 37, s1=33 * 37, ld=37)))
    for ld in (-1, 0, 1, 36, 37, 38, 64):
        out.append((d, dict(period0=2, period1=3, s0=9000, s1=3000, ld=ld)))
    for s0, s1 in ((-1, 0), (0, -1), (0, 0), (1, 1), (2 ** 40 - 1 - 32 * 37 - 37, 0), (2 ** 40 - 32 * 37 - 37, 0), (2 ** 62, 2 ** 62)):
        out.append((d, dict(period0=2, period1=2, s0=s0, s1=s1, ld=37)))
    big = dict(d, batch0=2, batch1=1, m=8192, n=32768, k=16)
    for p0, m, ld in ((1, 8192, 32768), (2, 8192, 32768), (1, 8193, 32768), (2, 8193, 0), (1, 8193, 32767)):
        out.append((dict(big, m=m), dict(period0=p0, period1=1, s0=0, s1=0, ld=ld)))
    out.append((dict(d, a_dt=B.U8, round_mode=1, nscales=37), dict(period0=1, period1=1, s0=0, s1=0, ld=0)))
    return out


def _check_against_mirror(exe):
    pairs = _layouts()
    seen, fast = set(), set()
    for max_abs, ninf, scale in ((100.0, 0, 0.004), (1.0e9, 0, 1.0), (5.0, 1, 0.004), (0.0, 0, float("inf")), (2.0 ** 20, 0, 512.0)):
        text = "".join("%d %d %d %d %d %d %d %d %d %d %d %d %d %r %d %r\n" % (
            d["batch0"], d["batch1"], d["m"], d["n"], d["k"], d["a_dt"], d["round_mode"], d["nscales"], b["period0"], b["period1"], b["s0"], b["s1"], b["ld"],
            max_abs, ninf, scale) for d, b in pairs)
        p = subprocess.run([exe, "-"], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert p.returncode == 0, p.stdout.decode()[-2000:]
        lines = p.stdout.decode().splitlines()
        assert len(lines) == len(pairs), p.stdout.decode()[-2000:]
        for (d, b), line in zip(pairs, lines):
            got = [int(x) for x in line.split()]
            rc = R.validate(d, b)
            seen.add(rc)
            assert got[0] == rc, (d, b, line)
            if rc == INVALID:
                continue
            want = [rc, R.host_elems(d, b), R.rows_of(d, b), R.up32(d["n"]), R.image_elems(d, b), R.distinct_bytes(d, b),
                    int(R.fast_ok_biased(d, [scale] * d["nscales"], max_abs, bool(ninf)))]
            fast.add(want[6])
            assert got == want, (d, b, got, want)
    assert seen == {0, INVALID, UNSUPPORTED} and fast == {0, 1}


def _scan(exe, d, b, table):
    words = " ".join("nan" if np.isnan(v) else "inf" if v == np.inf else "-inf" if v == -np.inf else repr(float(v)) for v in table)
    text = "%d %d %d %d %d %d %d %d\n%s\n" % (b["period0"], b["period1"], b["s0"], b["s1"], b["ld"], d["m"], d["n"], table.size, words)
    p = subprocess.run([exe, "scan"], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    lines = p.stdout.decode().splitlines()
    rc, mx, ninf = lines[0].split()
    img = np.array([[float(x) for x in ln.split()] for ln in lines[1:]], dtype=np.float32)
    return int(rc), float(mx), bool(int(ninf)), img


def _check_scans(exe):
    """host tables in three layouts with NaN in every gap: the image, max |finite| and the -inf flag against the mirror; +inf and
    NaN among the addressed entries are refused; the routes follow"""
    for bias in (R.Bias(periods=(2, 3), strides=(500, 150, 41), mask="random", mask_value="ninf", seed=81000), R.Bias(periods=(2, 2), seed=81001),
                 R.Bias(periods=(3, 1), one_row=True, strides=(50, 0, 0), mask="keypad", seed=81002)):
        m, n = 5, 37
        d = dict(batch0=bias.periods[0], batch1=bias.periods[1], m=m, n=n, k=16, a_dt=B.S8, round_mode=0, nscales=1)
        b = R.layout_dict(bias, m, n)
        bd = R.make_bias(bias, m, n, 0.01, R.acc_bound(B.S8, 16))
        assert bd["table"].size == R.host_elems(d, b)
        rc, mx, ninf, img = _scan(exe, d, b, bd["table"])
        want = R.scan(bd["values"])
        assert (rc, ninf) == (want[0], want[2]) == (0, bias.mask_value == "ninf") and np.float32(mx) == np.float32(want[1]), (bias, rc, mx, ninf, want)   # (printed with 9 digits: an f32 round trip)
        assert np.array_equal(img, R.image(d, b, bd["table"])) and img.shape == (R.image_elems(d, b) // 64, 64)
        assert (img[:, n:] == 0).all()
        # the routes: finite within the bound -> fast; beyond it -> exact; any -inf -> exact
        assert R.fast_ok_biased(d, [0.01], mx, ninf) == (not ninf)
        assert not R.fast_ok_biased(d, [0.01], 2.0 ** 30 / 0.01, False)
        for bad in (np.inf, np.nan):                                                 # +inf / NaN -> invalid
            t = bd["table"].copy()
            t[R.host_index(bias, m, n).reshape(-1)[-1]] = bad
            assert _scan(exe, d, b, t)[0] == INVALID
            assert R.scan(np.array([1.0, bad], dtype=np.float32))[0] == INVALID


def test_bias_plan_check_agrees_with_the_mirror_and_is_clean_under_the_host_sanitizers(tmp_path):
    """tools/bias_plan_check.cc, a stand-alone host program over csrc/bias_plan.h, built with the flags of the host Makefile's
    SAN=1 rule (ASan + UBSan) into a scratch directory and run directly: its self-check, the layouts of the Python mirror
    through its stdin mode and host tables through its scan mode.  Nothing is loaded into Python."""
    src = os.path.join(PKG, "tools", "bias_plan_check.cc")
    assert os.path.exists(src), "tools/bias_plan_check.cc is missing"
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert "$(TOOLS)/bias_plan_check: $(TOOLS)/bias_plan_check.cc ../csrc/bias_plan.h" in mk
    exe = tmp_path / "bias_plan_check"
    flags = ["-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++"] + flags + [src, "-o", str(exe)])
    p = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()
    assert "bias plans: validation order, the host extent, the image and its index, the scan and the biased route's edge hold" in p.stdout.decode()
    _check_against_mirror(str(exe))
    _check_scans(str(exe))
    built = os.path.join(PKG, "tools", "bias_plan_check")
    assert os.path.exists(built) and os.access(built, os.X_OK), "run __graft_entry__.build() first"
    _check_against_mirror(built)


def test_the_mirror_of_the_image_and_the_routes():
    d = dict(batch0=4, batch1=3, m=33, n=37, k=64, a_dt=B.S8, round_mode=0, nscales=1)
    b = dict(period0=2, period1=3, s0=5000, s1=1500, ld=41)
    assert R.validate(d, b) == 0 and R.host_elems(d, b) == 5000 + 2 * 1500 + 32 * 41 + 37 and R.image_elems(d, b) == 6 * 33 * 64
    assert R.image_index(b, 33, 64, 3, 2, 7, 5) == ((1 * 3 + 2) * 33 + 7) * 64 + 5 and R.image_index(dict(b, ld=0), 1, 64, 3, 2, 7, 5) == 5 * 64 + 5
    assert R.fast_ok_biased(d, [512.0], 2.0 ** 20, False) and not R.fast_ok_biased(d, [512.0], 2.0 ** 20 + 1, False)      # bound 2^20
    assert not R.fast_ok_biased(d, [1.0], 0.0, True) and not R.fast_ok_biased(dict(d, round_mode=1), [1.0], 0.0, False)
    assert not R.fast_ok_biased(d, [float("nan")], 0.0, False)
    assert R.fast_ok_biased(d, [1024.0], 0.0, False) == B.fast_ok(dict(d, trans_b=1), [1024.0]) is True


# ---- 4. the helper ---------------------------------------------------------------------------------------------------------------
def test_attention_bias_builds_accumulator_units_and_a_finite_mask_that_saturates():
    heads, nw, t, d = 3, 2, 9, 32
    step, ls = 0.0625, np.float32(0.004)
    bound = 128 * 128 * d
    rng = np.random.default_rng(82000)
    rel = rng.normal(0, 1, (heads, t, t))
    mask = np.where(rng.random((nw, t, t)) < 0.3, -np.inf, 0.0)
    table, periods = dfa.attention_bias(rel_bias=rel, mask=mask, logit_step=step, logit_scale=ls, acc_bound=bound)
    assert table.shape == (nw, heads, t, t) and periods == (nw, heads) and table.dtype == np.float32
    mv = R.finite_mask_value(bound, ls)
    assert np.isfinite(mv) and -mv >= bound + 129 / ls
    hit = np.broadcast_to(np.isneginf(mask)[:, None], table.shape)
    assert (table[hit] == mv).all()
    want = (rel[None] / (step * float(ls))).astype(np.float32)
    assert np.array_equal(table[~hit], np.broadcast_to(want, table.shape)[~hit])
    # every accumulator within the bound saturates to -128 under the finite mask, at both ends and in between
    for acc in (-bound, -1, 0, 1, bound):
        f = np.float32(np.float32(np.float32(acc) + mv) * ls)
        assert np.rint(f) <= -129, (acc, f)
    rc, mx, ninf = R.scan(table)
    assert rc == 0 and not ninf and R.fast_ok_biased(dict(round_mode=0, a_dt=B.S8, k=d), [ls], mx, ninf)    # the fast route stays provable
    # a negative scale: the mask value changes sign with it
    tneg, _ = dfa.attention_bias(mask=mask, logit_step=step, logit_scale=-ls, acc_bound=bound)
    assert (tneg[np.isneginf(mask)[:, None]] == -mv).all() and np.rint(np.float32(np.float32(np.float32(-bound) - mv) * -ls)) <= -129
    # -inf kept on request; a boolean mask; key padding alone is one row per image
    tinf, _ = dfa.attention_bias(rel_bias=rel, mask=np.isneginf(mask), logit_step=step, logit_scale=ls, acc_bound=bound, mask_value=-np.inf)
    assert np.isneginf(tinf[hit]).all() and np.array_equal(tinf[~hit], table[~hit])
    kp = np.zeros((4, 11), dtype=bool)
    kp[1, 7:] = kp[3, 2:] = True
    tk, pk = dfa.attention_bias(key_padding=kp, logit_step=step, logit_scale=ls, acc_bound=bound)
    assert tk.shape == (4, 1, 11) and pk == (4, 1) and (tk[kp[:, None]] == mv).all() and (tk[~kp[:, None]] == 0).all()
    both, pb = dfa.attention_bias(rel_bias=rel[:, :, :9], key_padding=np.zeros((4, 9), dtype=bool), logit_step=step, logit_scale=ls, acc_bound=bound)
    assert both.shape == (4, heads, t, 9) and pb == (4, heads)
    with pytest.raises(ValueError):
        dfa.attention_bias(logit_step=step, logit_scale=ls, acc_bound=bound)
    with pytest.raises(ValueError):
        dfa.attention_bias(mask=np.full((1, 2, 2), np.nan), logit_step=step, logit_scale=ls, acc_bound=bound)


def test_set_bias_arguments_from_tables_and_strides():
    b, t = capi._logit_bias_args(np.zeros((2, 3, 5, 7)), (2, 3), None, 5, 7)
    assert (b.period0, b.period1, b.s0, b.s1, b.ld) == (2, 3, 105, 35, 7) and t.dtype == np.float32 and t.size == 210
    b, t = capi._logit_bias_args(np.zeros((2, 3, 7)), (2, 3), None, 5, 7)
    assert (b.s0, b.s1, b.ld) == (21, 7, 0)
    b, t = capi._logit_bias_args(np.zeros((2, 1, 7)), (2, 1), None, 1, 7)
    assert (b.s0, b.s1, b.ld) == (7, 7, 0)
    b, t = capi._logit_bias_args(np.zeros(1000), (2, 3), (300, 90, 9), 5, 7)
    assert (b.s0, b.s1, b.ld) == (300, 90, 9)
    with pytest.raises(ValueError):
        capi._logit_bias_args(np.zeros(100), (2, 3), None, 5, 7)
    with pytest.raises(ValueError):
        capi._logit_bias_args(np.zeros(300 + 180 + 36 + 6), (2, 3), (300, 90, 9), 5, 7)       # one float short


# ---- 5. header, prototypes, exports ------------------------------------------------------------------------------------------------
def test_logit_bias_desc_and_prototypes_match_the_header(tmp_path):
    """dfx_logit_bias_desc compiled by gcc has the size and field offsets of the ctypes mirror; no existing struct changed size; the
    header's two prototypes are what ctypes binds"""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dfx.h"', 'int main(void) {',
             'printf("dfx_logit_bias_desc size %zu\\n", sizeof(dfx_logit_bias_desc));']
    for fname, _ in capi.LogitBiasDesc._fields_:
        lines.append('printf("dfx_logit_bias_desc %s %%zu\\n", offsetof(dfx_logit_bias_desc, %s));' % (fname, fname))
    for s in ("dfx_bmm_desc", "dfx_bmm_info", "dfx_attn_desc", "dfx_attn_info"):
        lines.append('printf("%s size %%zu\\n", sizeof(%s));' % (s, s))
    lines += ["int (*f)(dfx_bmm_t *, const dfx_logit_bias_desc *, const float *) = dfx_bmm_set_bias;",
              "int (*g)(dfx_attn_t *, const dfx_logit_bias_desc *, const float *) = dfx_attn_set_bias;", "return f == 0 || g == 0; }"]
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-L", PKG, "-ldfx_hip", "-Wl,-rpath," + PKG, "-o", str(exe)])
    seen = {}
    for ln in subprocess.check_output([str(exe)]).decode().splitlines():
        a, b, c = ln.split()
        seen[(a, b)] = int(c)
    assert seen[("dfx_logit_bias_desc", "size")] == ctypes.sizeof(capi.LogitBiasDesc) == 32
    for fname, _ in capi.LogitBiasDesc._fields_:
        assert seen[("dfx_logit_bias_desc", fname)] == getattr(capi.LogitBiasDesc, fname).offset, fname
    assert [n for n, _ in capi.LogitBiasDesc._fields_] == ["period0", "period1", "s0", "s1", "ld"]
    for cname, ct, size in (("dfx_bmm_desc", capi.BmmDesc, 128), ("dfx_bmm_info", capi.BmmInfo, None), ("dfx_attn_desc", capi.AttnDesc, 160),
                            ("dfx_attn_info", capi.AttnInfo, None)):
        assert seen[(cname, "size")] == ctypes.sizeof(ct) and size in (None, ctypes.sizeof(ct)), cname
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dfx.h")).read(), flags=re.S)
    assert "int dfx_bmm_set_bias(dfx_bmm_t *h, const dfx_logit_bias_desc *desc, const float *host_table);" in header
    assert "int dfx_attn_set_bias(dfx_attn_t *h, const dfx_logit_bias_desc *desc, const float *host_table);" in header
    L = capi.lib()
    for name in ("dfx_bmm_set_bias", "dfx_attn_set_bias"):
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int32 and len(fn.argtypes) == 3 and fn.argtypes[1] is ctypes.POINTER(capi.LogitBiasDesc), name


def test_library_exports_the_bias_entry_points():
    L = capi.lib()
    for s in ("dfx_bmm_set_bias", "dfx_attn_set_bias"):
        assert s in dfa.declared_symbols() and hasattr(L, s), s
    assert not [s for s in dfa.declared_symbols() if not hasattr(L, s)]
    assert L.dfx_bmm_set_bias(None, None, None) == INVALID and "null" in L.dfx_last_error().decode()
    assert L.dfx_attn_set_bias(None, None, None) == INVALID and "null" in L.dfx_last_error().decode()
    for name in ("LogitBiasDesc", "attention_bias"):
        assert hasattr(dfa, name), name
    assert callable(dfa.MatMul.set_bias) and callable(dfa.Attention.set_bias)
    for tool in ("bias_plan_check", "attn_bias_check"):
        assert os.access(os.path.join(PKG, "tools", tool), os.X_OK), "run __graft_entry__.build() first: " + tool


def test_the_header_states_the_mask_semantics_and_what_stays_unbuilt():
    text = " ".join(open(os.path.join(ROOT, "include", "dfx.h")).read().split())
    for phrase in ("The masked logit is -128", "E[max + 128]", "uniform over all", "torch gives NaN", "a device-resident table",
                   "skipping fully masked key tiles", "a mask input to dfx_head", "two separate bias operands"):
        assert phrase.replace(" ", "") in text.replace(" * ", " ").replace(" ", ""), phrase
    assert "an additive mask / relative-position bias on the logits" not in text and "a mask or relative-position bias on the logits" not in text
