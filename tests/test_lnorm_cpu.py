"""CPU-only checks of the int8 layer norm / RMS norm: the numpy reference the GPU tests compare against (tests/lnorm_ref.py)
equals an independent pure-Python witness that rounds every step from exact rationals; it stays within a DERIVED bound of a
float64 layer norm and within one code of torch's; the hand-computed tie rows round to even; the C ABI validates descriptors,
in the documented order, before it touches a device; the ctypes mirrors match the header, the symbols are exported and bound,
the drop-in layer and the tools are built; and the op's host-side plan (csrc/lnorm_plan.h) is clean under the host
sanitizers as a stand-alone program."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

import lnorm_ref as L

dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-fusion_amd")
INVALID, UNSUPPORTED, HIP, NO_DEVICE, STATE = 1, 2, 3, 4, 5


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. the reference against the witness ------------------------------------------------------------------------------------
def _witness_rows():
    rng = np.random.RandomState(7)
    rows = []
    for c in (1, 4, 17, 96, 100):
        for dt in (np.int8, np.uint8):
            lo, hi = (0, 256) if dt == np.uint8 else (-128, 128)
            rows.append((rng.randint(lo, hi, size=c).astype(dt), rng.randint(0, 8, size=c).astype(np.uint8), 2.0 ** -10))
            rows.append((rng.randint(lo, hi, size=c).astype(dt), None, 1e-3))
    # the extremes: the largest Q and u_k, the largest |S| with D = 0, an outlier, the two ends of eps
    c = 16384
    alt = np.where(np.arange(c) % 2 == 0, -128, 127).astype(np.int8)
    rows.append((alt, np.full(c, 7, dtype=np.uint8), 1.0))
    rows.append((np.full(c, 255, dtype=np.uint8), np.full(c, 7, dtype=np.uint8), 1.0))
    out = np.zeros(768, dtype=np.int8)
    out[5] = 127
    rows.append((out, None, 2.0 ** -20))
    tiny, huge = np.float32(1e-45), np.float32(3e38)
    assert 0 < float(tiny) < 1.5e-45
    for eps in (tiny, huge):
        rows.append((rng.randint(-128, 128, size=33).astype(np.int8), None, eps))
        rows.append((np.full(33, 9, dtype=np.int8), rng.randint(0, 8, size=33).astype(np.uint8), eps))
    return rows


@pytest.mark.parametrize("mode", [L.LAYER, L.RMS], ids=["layer", "rms"])
def test_reference_equals_the_witness(mode):
    assert dfa.LNORM_LAYER == L.LAYER and dfa.LNORM_RMS == L.RMS           # (the package knows the op at all)
    rng = np.random.RandomState(11)
    for x, shift, eps in _witness_rows():
        c = x.size
        n = min(c, 64)                                                     # the witness is slow: all statistics, 64 outputs
        gamma = (rng.standard_normal(c) * 3).astype(np.float32)
        beta = rng.standard_normal(c).astype(np.float32)
        got = L.reference_values(x.reshape(1, c), c, gamma, beta, shift, eps, mode)[0]
        keep = np.r_[0:n // 2, c - (n - n // 2):c] if c > n else np.arange(c)
        want = np.array(L.witness_row(x.tolist(), gamma, beta, shift, eps, mode, only=keep.tolist()), dtype=np.float32)
        assert np.array_equal(_bits(got[keep]), _bits(want)), (c, x.dtype, mode, float(eps))
        nob = L.reference_values(x.reshape(1, c), c, gamma, None, shift, eps, mode)[0]       # beta NULL: + 0 is still performed
        zero = L.reference_values(x.reshape(1, c), c, gamma, np.zeros(c, np.float32), shift, eps, mode)[0]
        assert np.array_equal(_bits(nob), _bits(zero))


def test_bounds_and_constant_rows():
    for c in (1, 15, 16, 17, 96, 100, 768, 1000, 1025, 4097, 16384):
        for shift in (None, np.full(c, 7, dtype=np.uint8)):
            for dt, ext in ((np.uint8, 255), (np.int8, -128)):
                src = np.full((2, c), ext, dtype=dt)
                src[1, ::2] = 0 if dt == np.uint8 else 127
                beta = np.linspace(-3, 3, c).astype(np.float32)
                gamma = np.full(c, 1e30, dtype=np.float32)
                y = L.reference_values(src, c, gamma, beta, shift, 0.5, L.LAYER)       # (asserts the intermediate bounds)
                assert np.array_equal(_bits(y[0]), _bits(beta)), c                     # D = 0, u = 0: beta exactly
                L.reference_values(src, c, gamma, beta, shift, 0.5, L.RMS)
    # c = 1: a layer norm of one channel is beta
    y = L.reference_values(np.array([[77]], dtype=np.int8), 1, [5.0], [0.25], None, 1e-5, L.LAYER)
    assert y.tolist() == [[0.25]]


# ---- 2. the derived tolerance ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [L.LAYER, L.RMS], ids=["layer", "rms"])
def test_within_the_derived_bound_of_a_float64_norm(mode):
    """|y - y64| <= 16 * 2^-24 * (|xhat * gamma| + |beta|): at most ten roundings of <= 2^-24 relative each between the
    exact statistics and y (two conversions, the division, the add, the square root -- which halves what came before it --
    two more divisions, the conversion of u, two multiplies, the add).  Derived, not measured."""
    rng = np.random.RandomState(3)
    worst = 0.0
    for c in (1, 15, 16, 17, 96, 100, 768, 1000, 1025, 4097, 16384):
        for dt in (np.int8, np.uint8):
            for shifted in (False, True):
                lo, hi = (0, 256) if dt == np.uint8 else (-128, 128)
                src = rng.randint(lo, hi, size=(3, c)).astype(dt)
                shift = rng.randint(0, 8, size=c).astype(np.uint8) if shifted else None
                gamma = (rng.standard_normal(c) * 2).astype(np.float32)
                beta = rng.standard_normal(c).astype(np.float32)
                eps = 1e-5 / 0.05 ** 2
                y = L.reference_values(src, c, gamma, beta, shift, eps, mode).astype(np.float64)
                y64, term = L.float64_norm(src, c, gamma, beta, shift, eps, mode)
                err = np.abs(y - y64)
                assert (err <= 16 * 2.0 ** -24 * term).all(), (c, dt, shifted, float((err / np.maximum(term, 1e-300)).max() * 2 ** 24))
                worst = max(worst, float((err[term > 0] / term[term > 0]).max() * 2 ** 24))
    print("worst deviation: %.2f * 2^-24 * (|xhat gamma| + |beta|)" % worst)


def test_within_one_code_of_torch_layer_norm():
    """torch.nn.functional.layer_norm in float64 on the dequantised input, lnorm_params folding the scales: the u8 / s8
    result is within 1 code everywhere"""
    import torch
    rng = np.random.RandomState(5)
    in_scale, eps = 0.037, 1e-5
    for c, dst_dt, out_scale in ((96, L.S8, 0.031), (768, L.U8, 0.02), (100, L.S8, 0.05), (1000, L.F32, None)):
        src = rng.randint(-128, 128, size=(9, c)).astype(np.int8)
        gamma = (1.0 + 0.2 * rng.standard_normal(c)).astype(np.float32)
        beta = (0.3 * rng.standard_normal(c) + (2.0 if dst_dt == L.U8 else 0.0)).astype(np.float32)
        g, b, eps_q = dfa.lnorm_params(gamma, beta, in_scale, out_scale, eps)
        assert g.dtype == b.dtype == np.float32 and isinstance(eps_q, np.float32)
        assert eps_q == np.float32(eps / in_scale ** 2)
        if out_scale is None:
            assert np.array_equal(g, gamma) and np.array_equal(b, beta)
        else:
            assert np.array_equal(g, (gamma.astype(np.float64) / out_scale).astype(np.float32))
            assert np.array_equal(b, (beta.astype(np.float64) / out_scale).astype(np.float32))
        got = L.convert(L.reference_values(src, c, g, b, None, eps_q, L.LAYER), dst_dt)
        x = torch.from_numpy(src.astype(np.float64) * in_scale)
        want = torch.nn.functional.layer_norm(x, (c,), torch.from_numpy(gamma.astype(np.float64)), torch.from_numpy(beta.astype(np.float64)),
                                              eps).numpy()
        if dst_dt == L.F32:
            assert np.abs(got - want).max() < 1e-5
        else:
            lo, hi = (0, 255) if dst_dt == L.U8 else (-128, 127)
            code = np.clip(np.rint(want / out_scale), lo, hi)
            assert np.abs(got.astype(np.float64) - code).max() <= 1, (c, dst_dt)
            assert (got.astype(np.float64) == code).mean() > 0.95
    assert dfa.lnorm_params([1.0], None, 0.5, 0.25, 1e-5)[1] is None


# ---- 3. the hand-computed tie rows ---------------------------------------------------------------------------------------------------
def test_tie_rows_round_to_even():
    """RMS of (2, -2, 2, -2) and LAYER of (5, 1, 5, 1) with eps = 2^-30 give xhat = +-1 exactly (v = 4, the eps is absorbed,
    sqrt = 2), so gamma = k + 0.5 puts every output on a tie: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4 and the negatives"""
    gamma = np.array([0.5, 1.5, 2.5, 3.5], dtype=np.float32)
    eps = 2.0 ** -30
    for mode, rows in ((L.RMS, [[2, -2, 2, -2], [-2, 2, -2, 2]]), (L.LAYER, [[5, 1, 5, 1], [1, 5, 1, 5]])):
        src = np.array(rows, dtype=np.int8)
        xhat = L.reference_values(src, 4, np.ones(4, np.float32), None, None, eps, mode)
        assert xhat.tolist() == [[1, -1, 1, -1], [-1, 1, -1, 1]]
        y = L.reference_values(src, 4, gamma, None, None, eps, mode)
        assert y.tolist() == [[0.5, -1.5, 2.5, -3.5], [-0.5, 1.5, -2.5, 3.5]]
        assert L.convert(y, L.S8).tolist() == [[0, -2, 2, -4], [0, 2, -2, 4]]
        assert L.convert(y, L.U8).tolist() == [[0, 0, 2, 0], [0, 2, 0, 4]]
        for r in range(2):
            assert L.witness_row(rows[r], gamma, None, None, eps, mode) == y[r].tolist()
    # the conversion: NaN -> 0, then clamp
    v = np.array([np.nan, np.inf, -np.inf, 300.0, -300.0, 254.5, 255.5, -128.5, -0.5], dtype=np.float32)
    assert L.convert(v, L.U8).tolist() == [0, 255, 0, 255, 0, 254, 255, 0, 0]
    assert L.convert(v, L.S8).tolist() == [0, 127, -128, 127, -128, 127, 127, -128, 0]


def test_generators_cover_the_grid():
    cases = L.grid_cases()
    assert len({c.ident() for c in cases}) == len(cases)
    for c in L.C_AXIS:
        assert len({x.rows for x in cases if x.c == c}) >= 2, c
    for r in L.ROWS_AXIS:
        assert len({x.c for x in cases if x.rows == r}) >= 2, r
    assert {L.lanes(x.c) for x in cases if L.in_class(x, L.ROW)} == {4, 8, 16, 32, 64}
    assert {x.c for x in cases if L.in_class(x, L.ROW)} >= set(L.C_AXIS)
    assert any(not L.in_class(x, L.ROW) for x in cases) and any(x.dst_off for x in cases)
    assert {(x.src_dt, x.dst_dt) for x in cases} == {(s, d) for s in (L.S8, L.U8) for d in (L.S8, L.U8, L.F32)}
    assert {(x.mode, x.shift) for x in cases} == {(m, s) for m in (0, 1) for s in (False, True)}
    assert [L.lanes(c) for c in (1, 64, 65, 96, 128, 129, 256, 257, 512, 513, 768, 1024, 1025, 16384)] == \
        [4, 4, 8, 8, 8, 16, 16, 32, 32, 64, 64, 64, 64, 64]
    src = L.make_src(cases[0])
    assert src.shape == (cases[0].rows, cases[0].src_ld)
    padded = [x for x in cases if x.src_ld > x.c][0]
    assert (L.make_src(padded)[:, padded.c:].view(np.uint8) == 0xFF).all()


# ---- 4. the plan under the host sanitizers ---------------------------------------------------------------------------------------
def test_lnorm_plan_check_is_clean_under_the_host_sanitizers(tmp_path):
    """tools/lnorm_plan_check.cc, a stand-alone host program over csrc/lnorm_plan.h, built with the flags of the host
    Makefile's SAN=1 rule (ASan + UBSan) into a scratch directory and run directly.  Nothing is loaded into Python."""
    src = os.path.join(PKG, "tools", "lnorm_plan_check.cc")
    assert os.path.exists(src), "tools/lnorm_plan_check.cc is missing"
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert "$(TOOLS)/lnorm_plan_check: $(TOOLS)/lnorm_plan_check.cc ../csrc/lnorm_plan.h" in mk
    exe = tmp_path / "lnorm_plan_check"
    flags = ["-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++"] + flags + [src, "-o", str(exe)])
    p = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()
    assert "lnorm plans: validation order, bounds, classes, lanes, grids and the 2^40 limit hold" in p.stdout.decode()


# ---- 5. descriptor and build checks ------------------------------------------------------------------------------------------------
def _desc(**kw):
    d = dict(rows=70, mode=capi.LNORM_LAYER, src_dt=capi.DFX_S8, dst_dt=capi.DFX_S8, c=96, src_ld=96, dst_ld=96, eps=1e-3,
             force_path=capi.LNORM_AUTO)
    d.update(kw)
    desc = capi.LnormDesc()
    for k, v in d.items():
        setattr(desc, k, v)
    return desc


def _create(**kw):
    desc = _desc(**kw)
    h = ctypes.c_void_p()
    rc = capi.lib().dfx_lnorm_create(ctypes.byref(desc), ctypes.byref(h))
    msg = capi.lib().dfx_last_error().decode()
    if rc == 0:
        assert capi.lib().dfx_lnorm_destroy(h) == 0
    else:
        assert not h.value
    return rc, msg


def _admitted(**kw):
    rc, msg = _create(**kw)
    assert rc in (0, NO_DEVICE), (kw, rc, msg)


def test_descriptor_validation_needs_no_device():
    # every refusal, in the order of the checks: a descriptor with faults i and j > i reports i
    faults = [(dict(mode=2), "mode"), (dict(rows=0), "rows"), (dict(c=0), "c must"), (dict(src_dt=capi.DFX_F32), "src dtype"),
              (dict(dst_dt=capi.DFX_S32), "dst dtype"), (dict(src_ld=95), "src_ld"), (dict(dst_ld=95), "dst_ld"), (dict(eps=0.0), "eps"),
              (dict(force_path=2), "force_path"), (dict(rows=2 ** 40), "2^40")]
    for i, (kw, word) in enumerate(faults):
        rc, msg = _create(**kw)
        assert rc == INVALID and word in msg, (kw, rc, msg)
        for kw2, _ in faults[i + 1:]:
            both = dict(kw2)
            both.update(kw)
            if set(kw) & set(kw2):
                continue
            rc, msg = _create(**both)
            assert rc == INVALID and word in msg, (both, rc, msg)
    for kw, word in ((dict(c=16385, src_ld=16400, dst_ld=16400), "16384"), (dict(c=-1), "c must"), (dict(rows=-5), "rows"), (dict(mode=-1), "mode"),
                     (dict(src_dt=capi.DFX_S32), "src dtype"), (dict(src_dt=0), "src dtype"), (dict(dst_dt=0), "dst dtype"),
                     (dict(eps=-1e-3), "eps"), (dict(eps=float("inf")), "eps"), (dict(eps=float("nan")), "eps"), (dict(force_path=-2), "force_path")):
        rc, msg = _create(**kw)
        assert rc == INVALID and word in msg, (kw, rc, msg)
    for kw in (dict(), dict(c=16384, src_ld=16384, dst_ld=16384), dict(c=1, src_ld=1, dst_ld=1), dict(src_dt=capi.DFX_U8, dst_dt=capi.DFX_F32),
               dict(dst_dt=capi.DFX_U8, mode=capi.LNORM_RMS), dict(eps=1e-45), dict(eps=3e38), dict(src_ld=100, dst_ld=99),
               dict(rows=2 ** 40 // 96), dict(force_path=capi.LNORM_ROW), dict(force_path=capi.LNORM_GENERIC),
               dict(force_path=capi.LNORM_ROW, dst_dt=capi.DFX_F32, dst_ld=100)):
        _admitted(**kw)
    assert _create(rows=2 ** 40 // 96 + 1)[0] == INVALID
    assert _create(rows=2 ** 40 // 128 + 1, dst_ld=128)[0] == INVALID
    # a forced path outside its class: unsupported, and only after everything invalid
    for kw in (dict(force_path=capi.LNORM_ROW, src_ld=100), dict(force_path=capi.LNORM_ROW, dst_ld=100),
               dict(force_path=capi.LNORM_ROW, c=15, src_ld=15, dst_ld=16), dict(force_path=capi.LNORM_ROW, dst_dt=capi.DFX_F32, dst_ld=98)):
        rc, msg = _create(**kw)
        assert rc == UNSUPPORTED and "class" in msg, (kw, rc, msg)
        assert _create(eps=0.0, **kw)[0] == INVALID
        kw["force_path"] = capi.LNORM_GENERIC
        _admitted(**kw)
        kw["force_path"] = capi.LNORM_AUTO
        _admitted(**kw)
    lib = capi.lib()
    assert lib.dfx_lnorm_create(None, None) == INVALID
    assert lib.dfx_lnorm_set_params(None, None, None, None) == INVALID
    assert lib.dfx_lnorm_submit(None, None, None, None) == INVALID
    assert lib.dfx_lnorm_query(None, None) == INVALID
    assert lib.dfx_debug_lnorm_launches(None) == INVALID
    assert lib.dfx_lnorm_destroy(None) == 0
    assert "null" in lib.dfx_last_error().decode()


def test_valid_descriptors_and_no_cpu_fallback():
    import torch
    for kw in (dict(), dict(mode=capi.LNORM_RMS, dst_dt=capi.DFX_F32), dict(force_path=capi.LNORM_ROW)):
        rc, msg = _create(**kw)
        if torch.cuda.is_available():
            assert rc == 0, (kw, msg)
        else:
            assert rc == NO_DEVICE and "no HIP device" in msg, (kw, rc, msg)
    if not torch.cuda.is_available():
        with pytest.raises(dfa.DfxError) as e:
            dfa.LayerNorm(70, 96, np.int8, np.int8, 1e-3)
        assert "dfx error 4" in str(e.value) and "no HIP device" in str(e.value)


def test_lnorm_structs_match_the_header(tmp_path):
    """dfx_lnorm_desc / dfx_lnorm_info compiled by gcc have the sizes and field offsets of the ctypes mirrors"""
    pairs = {"dfx_lnorm_desc": capi.LnormDesc, "dfx_lnorm_info": capi.LnormInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dfx.h"', 'int main(void) {']
    for cname, ct in pairs.items():
        lines.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in ct._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    enums = ("DFX_LNORM_LAYER", "DFX_LNORM_RMS", "DFX_LNORM_ROW", "DFX_LNORM_GENERIC", "DFX_LNORM_MAX_C", "DFX_LNORM_MAX_SHIFT", "DFX_VERSION")
    for name in enums:
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
    assert [n for n, _ in capi.LnormDesc._fields_] == ["rows", "mode", "src_dt", "dst_dt", "c", "src_ld", "dst_ld", "eps", "force_path"]
    assert [n for n, _ in capi.LnormInfo._fields_] == ["path", "grid", "block", "lds_bytes", "device", "algorithmic_bytes", "kernel_name"]
    assert seen[("enum", "DFX_LNORM_LAYER")] == capi.LNORM_LAYER == L.LAYER == 0 and seen[("enum", "DFX_LNORM_RMS")] == capi.LNORM_RMS == L.RMS == 1
    assert seen[("enum", "DFX_LNORM_ROW")] == capi.LNORM_ROW == L.ROW == 0 and seen[("enum", "DFX_LNORM_GENERIC")] == capi.LNORM_GENERIC == L.GENERIC == 1
    assert seen[("enum", "DFX_LNORM_MAX_C")] == capi.LNORM_MAX_C == L.MAX_C == 16384 and capi.LNORM_AUTO == -1
    assert seen[("enum", "DFX_LNORM_MAX_SHIFT")] == capi.LNORM_MAX_SHIFT == L.MAX_SHIFT == 7 and seen[("enum", "DFX_VERSION")] == 100
    assert ctypes.sizeof(capi.LnormDesc) == 40
    assert ctypes.sizeof(capi.HeadDesc) == seen[("dfx_head_desc", "size")]            # the others are untouched


def test_library_exports_the_lnorm_entry_points():
    lib = capi.lib()
    for s in ("dfx_lnorm_create", "dfx_lnorm_set_params", "dfx_lnorm_submit", "dfx_lnorm_query", "dfx_lnorm_destroy", "dfx_debug_lnorm_launches"):
        assert s in dfa.declared_symbols() and hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s                              # bound with a signature
    assert not [s for s in dfa.declared_symbols() if not hasattr(lib, s)]
    for name in ("LayerNorm", "LnormDesc", "LnormInfo", "LNORM_AUTO", "LNORM_ROW", "LNORM_GENERIC", "LNORM_LAYER", "LNORM_RMS", "lnorm_params",
                 "lnorm_launches"):
        assert hasattr(dfa, name), name
    capi.set_tuning("DFX_LNORM_GRID", "1")                                          # known to the library
    capi.set_tuning("DFX_LNORM_GRID", None)
    with pytest.raises(dfa.DfxError):
        capi.set_tuning("DFX_LNORM_ROWS", "1")
    header = open(os.path.join(ROOT, "include", "dfx.h")).read()
    assert "DFX_LNORM_AUTO_NOTE" in header


def test_dropin_layer_exports_layer_norm_and_tools_are_built():
    so = os.path.join(PKG, "libdeepfusion.so")
    assert os.path.exists(so), "run __graft_entry__.build() first"
    syms = subprocess.check_output(["nm", "-D", "-C", "--defined-only", so]).decode()
    assert "deepfusion::layer_norm(" in syms
    for tool in ("lnorm_check", "lnorm_plan_check", "bench_lnorm"):
        exe = os.path.join(PKG, "tools", tool)
        assert os.path.exists(exe) and os.access(exe, os.X_OK), tool
    p = subprocess.run([os.path.join(PKG, "tools", "lnorm_plan_check")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0 and "the 2^40 limit hold" in p.stdout.decode(), p.stdout.decode()
    ignore = open(os.path.join(ROOT, ".gitignore")).read().split()
    for tool in ("lnorm_check", "lnorm_plan_check", "bench_lnorm"):
        assert "deep-fusion_amd/tools/" + tool in ignore, tool
    # the trace stub knows the new C-ABI calls: coherence_check links against it
    stub = open(os.path.join(PKG, "tools", "dfx_trace_stub.cc")).read()
    for s in ("dfx_lnorm_create", "dfx_lnorm_set_params", "dfx_lnorm_submit", "dfx_lnorm_destroy"):
        assert "int %s(" % s in stub, s
