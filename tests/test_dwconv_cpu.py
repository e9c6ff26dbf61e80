"""CPU-only checks of the depthwise conv op: the C ABI validates descriptors before it touches a device, the ctypes
mirrors match the header, the symbols are exported, the drop-in layer and its tools are built, the numpy reference
the GPU tests compare against equals the C oracle's dense conv with block-diagonal weights, and the test data keeps
the promises the GPU tests rely on."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

import cases as C
import dwconv_ref as R
import hipref

dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-fusion_amd")
INVALID, UNSUPPORTED, NO_DEVICE = 1, 2, 4


def _create(**kw):
    d = dict(bs=2, c=32, ih=9, iw=11, oh=9, ow=11, kh=3, kw=3, sh=1, sw=1, pad_t=1, pad_l=1, dst_dt=capi.DFX_U8,
             bia_dt=capi.DFX_UNDEF, relu=0, round_mode=capi.ROUND_NEAREST, nscales=1, force_path=capi.DWCONV_AUTO)
    d.update(kw)
    desc = capi.DwConvDesc(**d)
    h = ctypes.c_void_p()
    rc = capi.lib().dfx_dwconv_create(ctypes.byref(desc), ctypes.byref(h))
    msg = capi.lib().dfx_last_error().decode()
    if rc == 0:
        assert capi.lib().dfx_dwconv_destroy(h) == 0
    else:
        assert not h.value
    return rc, msg


def test_descriptor_validation_needs_no_device():
    for bad in ("bs", "c", "ih", "iw", "oh", "ow", "kh", "kw", "sh", "sw"):
        assert _create(**{bad: 0})[0] == INVALID, bad
        assert _create(**{bad: -3})[0] == INVALID, bad
    assert _create(pad_t=-1)[0] == INVALID
    assert _create(pad_l=-1)[0] == INVALID
    assert _create(kh=256, pad_t=128)[0] == INVALID                   # kh, kw <= 255: the accumulator stays in s32
    assert _create(kw=256, pad_l=128)[0] == INVALID
    # (oh - 1) * sh - pad_t <= ih - 1, likewise in x: the last admitted and the first rejected output size
    assert _create(oh=11)[0] == INVALID                                # 10 * 1 - 1 = 9 > 8
    assert _create(ow=13)[0] == INVALID
    assert _create(sh=2, sw=2, pad_t=0, pad_l=0, oh=6, ow=6)[0] == INVALID      # 5 * 2 = 10 > 8
    assert _create(dst_dt=capi.DFX_UNDEF)[0] == INVALID
    assert _create(dst_dt=9)[0] == INVALID
    assert _create(bia_dt=7)[0] == INVALID
    assert _create(bia_dt=-1)[0] == INVALID
    assert _create(round_mode=2)[0] == INVALID
    assert _create(nscales=0)[0] == INVALID
    assert _create(nscales=7)[0] == INVALID
    assert _create(force_path=2)[0] == INVALID
    assert _create(force_path=-2)[0] == INVALID
    assert _create(bs=1 << 12, ih=1 << 10, iw=1 << 10, oh=1 << 10, ow=1 << 10)[0] == INVALID     # 2^32 pixels
    # force_path = WINDOW outside the window class: every clause of the class
    for kw in (dict(c=24), dict(kh=7, kw=7, pad_t=3, pad_l=3), dict(kh=3, kw=5, pad_l=2), dict(kh=1, kw=1, pad_t=0, pad_l=0),
               dict(sh=1, sw=2, ow=6), dict(sh=3, sw=3, oh=3, ow=4), dict(kh=4, kw=4),
               dict(bs=1, c=1 << 20, ih=64, iw=64, oh=64, ow=64),                      # one source image of 2^32 bytes
               dict(bs=1, c=1 << 18, ih=64, iw=64, oh=64, ow=64, dst_dt=capi.DFX_S32)):  # one dst image of 2^32 bytes
        rc, msg = _create(force_path=capi.DWCONV_WINDOW, **kw)
        assert rc == UNSUPPORTED and "window kernel's class" in msg, (kw, rc, msg)
    # null arguments
    L = capi.lib()
    assert L.dfx_dwconv_create(None, ctypes.byref(ctypes.c_void_p())) == INVALID
    assert L.dfx_dwconv_submit(None, None, None, None) == INVALID
    assert L.dfx_dwconv_submit_host(None, None, None) == INVALID
    assert L.dfx_dwconv_set_weights(None, None, None, None) == INVALID
    assert L.dfx_dwconv_query(None, None) == INVALID
    assert L.dfx_debug_dwconv_requant(None, None) == INVALID
    assert L.dfx_dwconv_destroy(None) == 0
    # a bad descriptor is refused through the Python class as well
    with pytest.raises(dfa.DfxError) as e:
        dfa.DwConv((1, 4, 4, 32), (3, 3), nscales=5)
    assert "dfx error 1" in str(e.value)


VALID = [
    dict(),                                                                         # window class
    dict(kh=5, kw=5, pad_t=2, pad_l=2, sh=2, sw=2, oh=5, ow=6, dst_dt=capi.DFX_S32, bia_dt=capi.DFX_F32, nscales=32),
    dict(sh=2, sw=2, pad_t=0, pad_l=0, oh=5, ow=6, relu=1, round_mode=capi.ROUND_DOWN),     # windows hang over
    dict(force_path=capi.DWCONV_WINDOW),
    dict(force_path=capi.DWCONV_GENERIC),
    dict(c=24, nscales=24),                                                         # outside it: the generic path
    dict(c=1), dict(kh=7, kw=7, pad_t=3, pad_l=3), dict(kh=1, kw=3, pad_t=0), dict(sh=1, sw=2, ow=6),
    dict(kh=255, kw=255, pad_t=127, pad_l=127),
    dict(pad_t=5, pad_l=4, oh=14, ow=15),                                           # windows entirely in the padding
]


def test_valid_descriptors_and_no_cpu_fallback():
    """valid descriptors pass validation, inside and outside the window class: with a device they create and destroy
    cleanly, without one they fail with DFX_ERR_NO_DEVICE (there is no CPU path)"""
    import torch
    for kw in VALID:
        rc, msg = _create(**kw)
        if torch.cuda.is_available():
            assert rc == 0, (kw, msg)
        else:
            assert rc == NO_DEVICE and "no HIP device" in msg, (kw, rc, msg)
    if not torch.cuda.is_available():
        with pytest.raises(dfa.DfxError) as e:
            dfa.DwConv((1, 4, 4, 32), (3, 3))
        assert "dfx error 4" in str(e.value) and "no HIP device" in str(e.value)


def test_dwconv_structs_match_the_header(tmp_path):
    """dfx_dwconv_desc / dfx_dwconv_info compiled by gcc have the sizes and field offsets of the ctypes mirrors"""
    pairs = {"dfx_dwconv_desc": capi.DwConvDesc, "dfx_dwconv_info": capi.DwConvInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dfx.h"', 'int main(void) {']
    for cname, ct in pairs.items():
        lines.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in ct._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines.append('printf("path window %d\\n", DFX_DWCONV_WINDOW); printf("path generic %d\\n", DFX_DWCONV_GENERIC);')
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
    assert seen[("path", "window")] == capi.DWCONV_WINDOW == R.WINDOW and seen[("path", "generic")] == capi.DWCONV_GENERIC == R.GENERIC
    assert [n for n, _ in capi.DwConvDesc._fields_] == ["bs", "c", "ih", "iw", "oh", "ow", "kh", "kw", "sh", "sw", "pad_t",
                                                        "pad_l", "dst_dt", "bia_dt", "relu", "round_mode", "nscales",
                                                        "force_path"]
    assert [n for n, _ in capi.DwConvInfo._fields_] == ["path", "grid", "block", "lds_bytes", "device", "algorithmic_ops",
                                                        "algorithmic_bytes", "kernel_name"]
    assert ctypes.sizeof(capi.ConvDesc) == 100 and len(capi.ConvDesc._fields_) == 25      # the conv's is untouched


def test_library_exports_the_dwconv_entry_points():
    L = capi.lib()
    for s in ("dfx_dwconv_create", "dfx_dwconv_set_weights", "dfx_dwconv_submit", "dfx_dwconv_submit_host",
              "dfx_dwconv_query", "dfx_dwconv_destroy", "dfx_debug_dwconv_requant"):
        assert s in dfa.declared_symbols() and hasattr(L, s), s
    assert not [s for s in dfa.declared_symbols() if not hasattr(L, s)]
    for name in ("DwConv", "DwConvDesc", "DwConvInfo", "DWCONV_AUTO", "DWCONV_WINDOW", "DWCONV_GENERIC"):
        assert hasattr(dfa, name), name


def test_dropin_layer_exports_depthwise_conv_and_tools_are_built():
    so = os.path.join(PKG, "libdeepfusion.so")
    assert os.path.exists(so), "run __graft_entry__.build() first"
    syms = subprocess.check_output(["nm", "-D", "-C", "--defined-only", so]).decode()
    assert "deepfusion::depthwise_conv(" in syms
    for tool in ("dwconv_check", "bench_dwconv"):
        exe = os.path.join(PKG, "tools", tool)
        assert os.path.exists(exe) and os.access(exe, os.X_OK), tool


def test_tables_cover_what_they_should():
    w, o, g = R.window_table(), R.options_table(), R.generic_table()
    assert {(c.k, c.stride) for c in w} == {((3, 3), (1, 1)), ((3, 3), (2, 2)), ((5, 5), (1, 1)), ((5, 5), (2, 2))}
    assert {c.c for c in w} >= {16, 48, 144, 16 * 65}
    assert {(c.ih, c.iw) for c in w if c.k == (3, 3) and c.stride == (1, 1) and c.pad == (1, 1)} >= {(1, 1), (3, 3), (7, 7), (5, 9), (13, 37), (3, 200)}
    assert any(c.out_hw == (4, 4) and (c.ih, c.iw) == (8, 8) for c in w) and any(c.out_hw == (4, 5) and (c.ih, c.iw) == (7, 10) for c in w)
    for t in (o, w + g):
        assert {c.dst_dt for c in t} == {C.U8, C.S8, C.S32, C.F32}
        assert {c.bia_dt for c in t} == {C.UNDEF, C.F32, C.S32, C.S8, C.U8}
        assert {c.per_channel for c in t} == {True, False} and {c.rm for c in t} == {0, 1} and {c.relu for c in t} == {True, False}
        assert any(c.wide for c in t)
    assert {c.stride for c in g} >= {(1, 2), (2, 1)} and {c.k for c in g} >= {(7, 7), (1, 3), (3, 1)}
    assert {c.c for c in g} >= {1, 3, 20, 24}
    assert len({c.ident() for c in R.all_tables()}) == len(R.all_tables())


@pytest.mark.parametrize("impl", ["scalar_mt", "avx512"])
def test_reference_equals_the_oracles_dense_conv_with_diagonal_weights(oracle, impl):
    """every table case with c % 16 == 0 and a symmetric window: this pins the reference of the GPU tests"""
    if impl == "avx512" and not oracle.have_avx512_vnni():
        impl = "scalar"       # the oracle's other implementation on a host without AVX-512 VNNI
    n = 0
    for case in R.all_tables():
        if not case.dense_expressible:
            continue
        data = R.generate(case)
        want = hipref.oracle_conv(oracle, R.dense_case(case), R.dense_data(data), impl=impl)
        hipref.assert_bit_equal(R.dw_ref(case, data), want, "%s vs oracle %s" % (case.ident(), impl))
        n += 1
    assert n >= 50


def test_wide_cases_reach_both_ends_of_the_range():
    """a "wide" 1-byte case's expected output holds both ends of what its dtype and ReLU flag can reach"""
    n = 0
    for case in R.all_tables():
        if not case.wide or case.dst_dt not in (C.U8, C.S8) or case.bs * case.oh * case.ow < 16:
            continue
        ref = R.dw_ref(case, R.generate(case))
        lo = 0 if (case.relu or case.dst_dt == C.U8) else -128
        hi = 255 if case.dst_dt == C.U8 else 127
        assert ref.min() == lo and ref.max() == hi, (case.ident(), ref.min(), ref.max())
        n += 1
    assert n >= 8


def test_nan_and_inf_scales_give_the_x86_results():
    """NaN -> 0x80000000 -> u8 255 / s8 -128; +inf * positive likewise (out of range), on the reference"""
    for dst_dt, bad in ((C.U8, 255), (C.S8, -128)):
        case = R.DwCase("nan", 1, 16, 4, 4, dst_dt=dst_dt, bia_dt=C.UNDEF, relu=False, per_channel=True)
        data = R.generate(case)
        data["scales"][3] = np.nan
        data["scales"][7] = np.inf
        data["src"][...] = np.maximum(data["src"], 1)
        data["w"][7] = np.abs(data["w"][7]) + 1
        ref = R.dw_ref(case, data)
        assert (ref[..., 3] == bad).all() and (ref[..., 7] == bad).all()


@pytest.mark.parametrize("edge", R.EDGES, ids=lambda e: e.name)
def test_edge_data_attains_the_bound_the_proof_uses(edge):
    """(255 * max(P, N) + |bias|) * scale is exactly 2^30 at the last admitted value, one scale step beyond at the first
    rejected one, and the centre pixel's accumulator is exactly 255 P / -255 N"""
    case, data = R.edge_case(edge, C.S32)
    acc, bound, P, N = R.edge_attained(edge, case, data)
    assert acc == bound and abs(bound) == 255 * max(P, N)
    reach = (255 * max(P, N) + abs(edge.bias)) * edge.scale
    assert reach == (R.LIMIT if edge.fast else R.LIMIT + edge.scale)
    assert float(np.float32(edge.bias)) == edge.bias and float(np.float32(edge.scale)) == edge.scale     # exact in f32
    ref = R.dw_ref(case, data)
    img = 0 if edge.which == "max" else 1
    sign = 1 if edge.which == "max" else -1
    assert int(ref[img, 1, 1, R.EDGE_CHANNEL]) == sign * int(reach)            # the s32 result shows it: no saturation yet
