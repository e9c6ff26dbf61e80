"""CPU-only checks of the int8 token linear op (dfx_linear_*): the numpy reference the GPU tests compare against
(tests/linear_ref.py) equals an element-by-element witness and, for a u8 src with src_ld = k and dst_ld = n, the fully-connected
op's reference (fc_ref, pinned to the C oracle by tests/test_fc_cpu.py); the case tables hold the regime they are meant to hold;
the op's host-side plan and packer (csrc/linear_plan.h, linear_pack.h) agree with their Python mirror, byte for byte, and are
clean under the host sanitizers as a stand-alone program; the C ABI validates descriptors in the documented order before it
touches a device, every clause at the last value it admits and the first it rejects; the ctypes mirrors match the header;
gelu_table follows its formula."""
import ctypes
import importlib
import math
import os
import subprocess

import numpy as np
import pytest

import fc_ref
import linear_ref as R

dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-fusion_amd")
INVALID, UNSUPPORTED, HIP, NO_DEVICE, STATE = 1, 2, 3, 4, 5
SAT_CAP = 0.10        # at most this share of a case's outputs on a saturation bound, except in the cases built to saturate


# ---- 1. the reference ------------------------------------------------------------------------------------------------------------
def _small_cases():
    out = [c for bm in R.BMS for dt in (R.U8, R.S8) for c in R.shape_grid(bm, dt) if c.rows * c.n * c.k <= 40000][::3]
    out += [R.with_dst(c, rows=9, n=11) for c in R.bias_cases() + R.tie_cases()[:4] + R.nonfinite_cases() + R.table_cases()]
    out += [R.with_dst(c, rows=7) for c in R.pitched_cases()]
    return out


def test_reference_equals_the_witness():
    """whole storage, bytes: every dst dtype, bias dtype, round mode, ReLU, per-channel scales, pitches, tables, inf / NaN scales"""
    cases = _small_cases()
    assert len(cases) > 60
    seen = set()
    for case in cases:
        data = R.generate(case)
        assert np.array_equal(R.reference(case, data), R.witness(case, data)), case.ident()
        seen.add((case.src_dt, case.dst_dt, case.bia_dt, case.rm, case.lut_in))
    assert {s[1] for s in seen} == {R.U8, R.S8, R.S32, R.F32} and {s[2] for s in seen} == {R.UNDEF, R.U8, R.S8, R.S32, R.F32}
    assert {s[4] for s in seen} == {R.UNDEF, R.U8, R.S8} and {s[3] for s in seen} == {0, 1}
    for case, data in R.compensation_cases()[:1] + [R.lane_map_case(64)]:
        small = R.with_dst(case, rows=2)
        sdata = dict(data, src=data["src"][:2 * case.sld])
        assert np.array_equal(R.reference(small, sdata), R.witness(small, sdata)), case.ident()


def test_reference_equals_fc_ref_where_the_ops_coincide():
    """u8 src, src_ld = k, dst_ld = n: fc_ref on {rows, 1, 1, k} with the weights as {n, k, 1, 1}"""
    for case in R.fc_twin_cases():
        data = R.generate(case)
        fcase = fc_ref.FcCase("twin", case.rows, case.k, 1, 1, case.n, dst_dt=case.dst_dt, bia_dt=case.bia_dt, relu=case.relu, rm=case.rm,
                              per_channel=case.per_channel)
        fdata = dict(src=R.valid_src(case, data).reshape(case.rows, 1, 1, case.k), w=data["w"].reshape(case.n, case.k, 1, 1), bia=data["bia"],
                     scales=data["scales"])
        want = fc_ref.fc_ref(fcase, fdata)
        got = R.values(case, data)
        assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), case.ident()


def test_tables_hold_their_regime():
    """for every generated case the GPU files use: at most 10 % of the requant's outputs on a saturation bound (u8 255, s8 -128 /
    127, s32 +-2^31), except in the cases built to saturate, and no case all zero; a ReLU's zeros are the op's own result, but at
    least a quarter of a ReLU case's outputs are non-zero wherever it has 64 outputs or more.  The scales come from k alone."""
    cases = R.generated_cases()
    assert len(cases) > 500
    built = 0
    for case in cases:
        data = R.generate(case)
        t = R.requant_values(case, data)
        sat = R.saturated_fraction(case, t)
        if case.saturating:
            built += 1
            assert sat > 0.4 or case.req_dt == R.F32, case.ident()
            continue
        assert sat <= SAT_CAP, (case.ident(), sat)
        assert R.values(case, data).view(np.uint8).any(), case.ident()
        if case.does_relu and t.size >= 64:
            assert (t != 0).mean() >= 0.25, case.ident()
        if t.size >= 64:
            assert len(np.unique(t)) > 2, case.ident()
    assert built == 8
    for bm in R.BMS:                                                       # the grid is a pairwise cover of the issue's tails
        rs, ns, ks = R.grid_axes(bm)
        for dt in (R.U8, R.S8):
            g = R.shape_grid(bm, dt)
            assert {(c.rows, c.n) for c in g} == {(r, n) for r in rs for n in ns}
            assert {(c.rows, c.k) for c in g} == {(r, k) for r in rs for k in ks}
            assert {(c.n, c.k) for c in g} == {(n, k) for n in ns for k in ks}
            for axis, vals in (("rows", rs), ("n", ns), ("k", ks)):
                for v in vals:
                    mine = [c for c in g if getattr(c, axis) == v]
                    assert {c.dst_dt for c in mine} == {R.U8, R.S8, R.S32, R.F32}, (axis, v)
                    assert {c.dld % 4 == 0 for c in mine} == {True, False}, (axis, v)
    # the hand-built cases
    for case, data in R.compensation_cases():
        assert abs(R.accumulate(case, data)).max() == 255 * 128 * case.k and R.values(case, data).any()
    for bm in R.BMS:
        case, data = R.lane_map_case(bm)
        assert R.saturated_fraction(case, R.values(case, data)) == 0.0 and case.rows == 2 * bm
    assert R.tiles(R.desc_of(R.GRID_CAP_CASE), 64) >= 6


# ---- 2. the plan and the packer against their mirror ------------------------------------------------------------------------------
PLAN_SHAPES = [(1, 1, 1, 16, 1, 256, 0, 0), (300, 200, 133, 208, 133, 256, 0, 0), (300, 200, 133, 208, 140, 4, 0, 0), (1576, 768, 2304, 768, 2304, 256, 0, 0),
               (1576, 768, 2304, 768, 2304, 200, 0, 7), (130, 65, 129, 80, 129, 256, 128, 0), (130, 63, 127, 64, 127, 256, 64, 3), (64, 17, 3, 32, 4, 2, 0, 0)]


def _plan_tool(tmp_path, exe, shape, seed):
    rows, k, n, sld, dld, cus, forced, cap = shape
    w = np.random.default_rng(seed).integers(-128, 128, (n, k)).astype(np.int8)
    wf, imf = tmp_path / "w.bin", tmp_path / "img.bin"
    w.tofile(str(wf))
    out = subprocess.check_output([str(exe), "plan"] + [str(v) for v in shape] + [str(wf), str(imf)]).decode()
    plan = {ln.split()[0]: int(ln.split()[1]) for ln in out.splitlines() if len(ln.split()) == 2}
    return w, plan, np.fromfile(str(imf), dtype=np.uint8)


def _check_plans(tmp_path, exe):
    for i, shape in enumerate(PLAN_SHAPES):
        rows, k, n, sld, dld, cus, forced, cap = shape
        w, plan, img = _plan_tool(tmp_path, exe, shape, 100 + i)
        d = R.desc_of(R.LinCase("plan", rows, k, n, src_ld=sld, dst_ld=dld), force_path=R.TILE)
        assert plan["validate"] == R.validate(d) == 0, shape
        bm = R.planned_bm(d, cus, forced)
        offs = R.image_offsets(n, k)
        assert plan["path"] == R.auto_path(d) == R.TILE and plan["bm"] == bm and plan["tiles"] == R.tiles(d, bm), (shape, plan)
        assert plan["grid_tile"] == R.planned_grid(d, R.TILE, bm, cus, cap) and plan["grid_generic"] == R.planned_grid(d, R.GENERIC, bm, cus, cap), (shape, plan)
        assert plan["lds"] == R.lds_bytes(R.TILE, bm) and plan["fast"] == 1, (shape, plan)
        assert (plan["off_comp"], plan["off_bias"], plan["off_scale"], plan["off_table"], plan["bytes"]) == offs, (shape, plan)
        packed, comp = R.pack_weights(w)
        assert img.size == offs[3]
        assert np.array_equal(img[:offs[0]], packed), shape                                    # the weight section, byte for byte
        assert np.array_equal(img[offs[0]:offs[1]].view(np.int32), comp), shape                # the compensation
        assert not img[offs[1]:offs[2]].any(), shape                                           # no bias
        scale = img[offs[2]:offs[3]].view(np.float32)
        assert (scale[:n] == 1.0).all() and not scale[n:].any(), shape
    # one weight's place, spelled out: W[o][c] with o = 128 nb + 32 f + r, c = 64 ks + 32 j + 16 h + b
    w = np.zeros((264, 200), dtype=np.int8)
    w[128 + 32 * 3 + 5, 64 * 2 + 32 + 16 + 7] = 77
    packed, comp = R.pack_weights(w)
    at = (1 * 4 + 2) * 8192 + ((3 * 2 + 1) * 64 + 32 + 5) * 16 + 7
    assert packed[at] == 77 and np.count_nonzero(packed) == 1 and comp[128 + 101] == 128 * 77 and np.count_nonzero(comp) == 1


def test_linear_plan_check_is_clean_under_the_host_sanitizers_and_agrees_with_the_mirror(tmp_path):
    """tools/linear_plan_check.cc, a stand-alone host program over csrc/linear_plan.h and linear_pack.h, built with the flags of
    the host Makefile's SAN=1 rule (ASan + UBSan) into a scratch directory and run directly: its own checks, then plans and
    images of shapes with n and k tails against the Python mirror.  Nothing is loaded into Python."""
    src = os.path.join(PKG, "tools", "linear_plan_check.cc")
    assert os.path.exists(src), "tools/linear_plan_check.cc is missing"
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert "$(TOOLS)/linear_plan_check: $(TOOLS)/linear_plan_check.cc ../csrc/linear_plan.h ../csrc/linear_pack.h" in mk
    exe = tmp_path / "linear_plan_check"
    flags = ["-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++"] + flags + [src, "-o", str(exe)])
    p = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()
    assert "linear plans: validation order, classes, tile heights, grids, LDS, image sections, the packer and the route's proof hold" in p.stdout.decode()
    _check_plans(tmp_path, exe)


def test_mirror_validation_agrees_with_the_header_order():
    base = R.desc_of(R.LinCase("v", 70, 96, 40))
    assert R.validate(base) == 0 and R.tile_class(base)
    for kw in (dict(rows=0), dict(k=0), dict(k=R.KMAX + 1, src_ld=R.KMAX + 1), dict(n=0), dict(src_dt=R.F32), dict(dst_dt=0), dict(bia_dt=5),
               dict(round_mode=2), dict(nscales=2), dict(lut_in_dt=R.F32), dict(lut_in_dt=R.S8, dst_dt=R.F32), dict(force_path=2), dict(src_ld=95),
               dict(dst_ld=39), dict(rows=2 ** 40 // 96 + 1)):
        assert R.validate(dict(base, **kw)) == R.INVALID, kw
    assert R.validate(dict(base, src_ld=100, force_path=R.TILE)) == R.UNSUPPORTED
    assert R.validate(dict(base, src_ld=100, force_path=R.TILE, nscales=3)) == R.INVALID
    assert R.validate(dict(base, rows=2 ** 40 // 96)) == 0 and R.validate(dict(base, k=R.KMAX, src_ld=R.KMAX)) == 0


# ---- 3. descriptor and build checks ------------------------------------------------------------------------------------------------
def _desc(**kw):
    d = dict(rows=70, k=96, n=40, src_dt=capi.DFX_S8, dst_dt=capi.DFX_S8, bia_dt=capi.DFX_UNDEF, relu=0, round_mode=0, nscales=1,
             lut_in_dt=capi.DFX_UNDEF, force_path=capi.LINEAR_AUTO, src_ld=96, dst_ld=40)
    d.update(kw)
    desc = capi.LinearDesc()
    for k, v in d.items():
        setattr(desc, k, v)
    return desc


def _create(**kw):
    desc = _desc(**kw)
    h = ctypes.c_void_p()
    rc = capi.lib().dfx_linear_create(ctypes.byref(desc), ctypes.byref(h))
    msg = capi.lib().dfx_last_error().decode()
    if rc == 0:
        assert capi.lib().dfx_linear_destroy(h) == 0
    else:
        assert not h.value
    return rc, msg


def _admitted(**kw):
    rc, msg = _create(**kw)
    assert rc in (0, NO_DEVICE), (kw, rc, msg)


def test_descriptor_validation_needs_no_device():
    # every refusal, in the order of the checks: a descriptor with faults i and j > i reports i
    faults = [(dict(rows=0), "rows"), (dict(k=0), "k must"), (dict(n=0), "n must"), (dict(src_dt=capi.DFX_F32), "src dtype"), (dict(dst_dt=5), "dst dtype"),
              (dict(bia_dt=5), "bias dtype"), (dict(round_mode=2), "round mode"), (dict(nscales=2), "scales count"), (dict(lut_in_dt=capi.DFX_S32), "lut_in_dt"),
              (dict(force_path=2), "force_path"), (dict(src_ld=95), "src_ld"), (dict(dst_ld=39), "dst_ld")]
    for i, (kw, word) in enumerate(faults):
        rc, msg = _create(**kw)
        assert rc == INVALID and word in msg, (kw, rc, msg)
        for kw2, _ in faults[i + 1:]:
            both = dict(kw2)
            both.update(kw)
            rc, msg = _create(**both)
            assert rc == INVALID and word in msg, (both, rc, msg)
    rc, msg = _create(lut_in_dt=capi.DFX_S8, dst_dt=capi.DFX_F32)
    assert rc == INVALID and "1-byte dst" in msg
    rc, msg = _create(lut_in_dt=capi.DFX_U8, dst_dt=capi.DFX_S32, force_path=2)             # the table's clause comes before force_path's
    assert rc == INVALID and "1-byte dst" in msg
    for kw, word in ((dict(k=65026, src_ld=65040), "65025"), (dict(k=-1), "k must"), (dict(rows=-5), "rows"), (dict(n=2 ** 31 - 127, dst_ld=2 ** 31), "n must"),
                     (dict(src_dt=capi.DFX_S32), "src dtype"), (dict(src_dt=0), "src dtype"), (dict(dst_dt=0), "dst dtype"), (dict(bia_dt=-1), "bias dtype"),
                     (dict(round_mode=-1), "round mode"), (dict(nscales=0), "scales count"), (dict(nscales=41), "scales count"), (dict(lut_in_dt=5), "lut_in_dt"),
                     (dict(force_path=-2), "force_path"), (dict(rows=2 ** 40 // 96 + 1), "2^40"), (dict(rows=2 ** 40 // 128 + 1, dst_ld=128), "2^40")):
        rc, msg = _create(**kw)
        assert rc == INVALID and word in msg, (kw, rc, msg)
    for kw in (dict(), dict(k=65025, src_ld=65025), dict(k=1, src_ld=1, n=1, dst_ld=1), dict(src_dt=capi.DFX_U8, dst_dt=capi.DFX_F32), dict(nscales=40),
               dict(bia_dt=capi.DFX_U8, dst_dt=capi.DFX_S32), dict(lut_in_dt=capi.DFX_U8, dst_dt=capi.DFX_S8), dict(lut_in_dt=capi.DFX_S8, dst_dt=capi.DFX_U8),
               dict(src_ld=100, dst_ld=99), dict(rows=2 ** 40 // 96), dict(rows=2 ** 40 // 128, dst_ld=128), dict(round_mode=1, relu=1),
               dict(force_path=capi.LINEAR_TILE), dict(force_path=capi.LINEAR_GENERIC), dict(force_path=capi.LINEAR_TILE, src_ld=112, dst_ld=41)):
        _admitted(**kw)
    # a forced path outside its class: unsupported, and only after everything invalid
    for kw in (dict(force_path=capi.LINEAR_TILE, src_ld=100), dict(force_path=capi.LINEAR_TILE, k=15, src_ld=15), dict(force_path=capi.LINEAR_TILE, src_ld=97)):
        rc, msg = _create(**kw)
        assert rc == UNSUPPORTED and "class" in msg, (kw, rc, msg)
        assert _create(dst_ld=39, **kw)[0] == INVALID
        assert _create(rows=2 ** 40, **kw)[0] == INVALID
        kw["force_path"] = capi.LINEAR_GENERIC
        _admitted(**kw)
        kw["force_path"] = capi.LINEAR_AUTO
        _admitted(**kw)
    lib = capi.lib()
    assert lib.dfx_linear_create(None, None) == INVALID
    assert lib.dfx_linear_set_weights(None, None, None, None) == INVALID
    assert lib.dfx_linear_set_table(None, None) == INVALID
    assert lib.dfx_linear_submit(None, None, None, None) == INVALID
    assert lib.dfx_linear_submit_host(None, None, None) == INVALID
    assert lib.dfx_linear_query(None, None) == INVALID
    assert lib.dfx_debug_linear_launches(None) == INVALID
    assert lib.dfx_debug_linear_requant(None, None) == INVALID
    assert lib.dfx_linear_destroy(None) == 0
    assert "null" in lib.dfx_last_error().decode()


def test_valid_descriptors_and_no_cpu_fallback():
    import torch
    for kw in (dict(), dict(src_dt=capi.DFX_U8, dst_dt=capi.DFX_F32), dict(force_path=capi.LINEAR_TILE)):
        rc, msg = _create(**kw)
        if torch.cuda.is_available():
            assert rc == 0, (kw, msg)
        else:
            assert rc == NO_DEVICE and "no HIP device" in msg, (kw, rc, msg)
    if not torch.cuda.is_available():
        with pytest.raises(dfa.DfxError) as e:
            dfa.Linear(70, 96, 40)
        assert "dfx error 4" in str(e.value) and "no HIP device" in str(e.value)


def test_linear_structs_match_the_header(tmp_path):
    """dfx_linear_desc / dfx_linear_info compiled by gcc have the sizes and field offsets of the ctypes mirrors"""
    pairs = {"dfx_linear_desc": capi.LinearDesc, "dfx_linear_info": capi.LinearInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dfx.h"', 'int main(void) {']
    for cname, ct in pairs.items():
        lines.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in ct._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    enums = ("DFX_LINEAR_TILE", "DFX_LINEAR_GENERIC", "DFX_VERSION")
    for name in enums:
        lines.append('printf("enum %s %%d\\n", %s);' % (name, name))
    lines.append('printf("dfx_lnorm_desc size %zu\\n", sizeof(dfx_lnorm_desc));')
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
    assert [n for n, _ in capi.LinearDesc._fields_] == ["rows", "k", "n", "src_dt", "dst_dt", "bia_dt", "relu", "round_mode", "nscales", "lut_in_dt",
                                                        "force_path", "src_ld", "dst_ld"]
    assert [n for n, _ in capi.LinearInfo._fields_] == ["path", "grid", "block", "lds_bytes", "device", "algorithmic_ops", "algorithmic_bytes", "kernel_name"]
    assert seen[("enum", "DFX_LINEAR_TILE")] == capi.LINEAR_TILE == R.TILE == 0 and seen[("enum", "DFX_LINEAR_GENERIC")] == capi.LINEAR_GENERIC == R.GENERIC == 1
    assert capi.LINEAR_AUTO == -1 and seen[("enum", "DFX_VERSION")] == 100
    assert ctypes.sizeof(capi.LinearDesc) == 64
    assert ctypes.sizeof(capi.LnormDesc) == seen[("dfx_lnorm_desc", "size")]            # the others are untouched


def test_library_exports_the_linear_entry_points():
    lib = capi.lib()
    for s in ("dfx_linear_create", "dfx_linear_set_weights", "dfx_linear_set_table", "dfx_linear_submit", "dfx_linear_submit_host", "dfx_linear_query",
              "dfx_linear_destroy", "dfx_debug_linear_launches", "dfx_debug_linear_requant"):
        assert s in dfa.declared_symbols() and hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s                              # bound with a signature
    assert not [s for s in dfa.declared_symbols() if not hasattr(lib, s)]
    for name in ("Linear", "LinearDesc", "LinearInfo", "LINEAR_AUTO", "LINEAR_TILE", "LINEAR_GENERIC", "linear_launches", "gelu_table"):
        assert hasattr(dfa, name), name
    for key in ("DFX_LINEAR_GRID", "DFX_LINEAR_BM"):                                 # known to the library
        capi.set_tuning(key, "1")
        capi.set_tuning(key, None)
    with pytest.raises(dfa.DfxError):
        capi.set_tuning("DFX_LINEAR_TILES", "1")
    header = open(os.path.join(ROOT, "include", "dfx.h")).read()
    assert "DFX_LINEAR_AUTO_NOTE" in header
    # the tile constants of the header, the plan and the mirror are the same
    plan = open(os.path.join(PKG, "csrc", "linear_plan.h")).read()
    assert "LIN_BN = %d;" % R.BN in plan and "LIN_KS = %d;" % R.KS in plan and "LIN_BM_MAX = %d, LIN_BM_MIN = %d;" % (max(R.BMS), min(R.BMS)) in plan
    assert "LIN_TILE_GRID_PER_CU = %d;" % R.TILE_GRID_PER_CU in plan and "LIN_GEN_GRID_PER_CU = %d;" % R.GEN_GRID_PER_CU in plan


def test_dropin_layer_exports_linear_and_tools_are_built():
    so = os.path.join(PKG, "libdeepfusion.so")
    assert os.path.exists(so), "run __graft_entry__.build() first"
    syms = subprocess.check_output(["nm", "-D", "-C", "--defined-only", so]).decode()
    assert "deepfusion::linear(" in syms
    for tool in ("linear_check", "linear_plan_check", "bench_linear"):
        exe = os.path.join(PKG, "tools", tool)
        assert os.path.exists(exe) and os.access(exe, os.X_OK), tool
    p = subprocess.run([os.path.join(PKG, "tools", "linear_plan_check")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0 and "the route's proof hold" in p.stdout.decode(), p.stdout.decode()
    ignore = open(os.path.join(ROOT, ".gitignore")).read().split()
    for tool in ("linear_check", "linear_plan_check", "bench_linear"):
        assert "deep-fusion_amd/tools/" + tool in ignore, tool
    # the trace stub knows the new C-ABI calls: coherence_check links against it
    stub = open(os.path.join(PKG, "tools", "dfx_trace_stub.cc")).read()
    for s in ("dfx_linear_create", "dfx_linear_set_weights", "dfx_linear_set_table", "dfx_linear_submit", "dfx_linear_destroy"):
        assert "int %s(" % s in stub, s


# ---- 4. gelu_table ---------------------------------------------------------------------------------------------------------------------
def _gelu(x):
    return 0.5 * x * (1.0 + math.erf(x / math.sqrt(2.0)))


def test_gelu_table_follows_its_formula():
    """at its ends, at zero and at a tie; clamped; both index conventions"""
    t = dfa.gelu_table(0.05, 0.04, np.int8, np.int8)
    assert t.dtype == np.uint8 and t.shape == (256,)
    s = t.view(np.int8)
    assert s[128] == 0                                                          # q = 0
    assert s[0] == int(round(_gelu(-128 * 0.05) / 0.04)) == 0                   # q = -128: gelu(-6.4) is -1e-10
    assert s[255] == 127 and _gelu(127 * 0.05) / 0.04 > 127                     # q = 127: 158.7, clamped
    assert s[128 + 20] == int(round(_gelu(1.0) / 0.04)) == 21                   # gelu(1) = 0.8413
    assert s[128 - 15] == int(round(_gelu(-0.75) / 0.04)) == -4                 # the dip below zero survives
    assert s.min() == -4 and (np.diff(s[128:].astype(int)) >= 0).all()
    for i in range(256):
        want = min(max(round(_gelu((i - 128) * 0.05) / 0.04), -128), 127)
        assert int(s[i]) == want, i
    # a tie: in_step 1, out_step chosen so that gelu(1) / out_step = 2.5 exactly in float64 -> 2 (even), and 3.5 -> 4
    for half, even in ((2.5, 2), (3.5, 4)):
        step = _gelu(1.0) / half
        assert _gelu(1.0) / step == half
        assert int(dfa.gelu_table(1.0, step, np.uint8, np.uint8)[1]) == even
    u = dfa.gelu_table(0.1, 0.05, np.uint8, np.uint8)
    assert u[0] == 0 and u[255] == 255 and u[10] == int(round(_gelu(1.0) / 0.05))  # a u8 index type starts at q = 0
    m = dfa.gelu_table(0.05, 0.04, np.int8, np.uint8)
    assert m[:128].max() == 0 and m[255] == int(round(_gelu(127 * 0.05) / 0.04)) == 159   # negative outputs clamp to 0 in u8
    for bad in ((0.0, 1.0), (1.0, -1.0), (float("inf"), 1.0), (1.0, float("nan"))):
        with pytest.raises(ValueError):
            dfa.gelu_table(*bad)
    with pytest.raises(ValueError):
        dfa.gelu_table(1.0, 1.0, np.int32, np.int8)
