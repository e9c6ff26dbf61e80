"""CPU-only checks of the grouped conv op: the C ABI validates descriptors before it touches a device, the ctypes
mirrors match the header, the symbols are exported, the drop-in layer and its tools are built, the numpy reference the
GPU tests compare against equals the C oracle's dense conv with block-diagonal weights, and the test data keeps the
promises the GPU tests rely on."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

import cases as C
import gconv_ref as R
import hipref

dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-fusion_amd")
INVALID, UNSUPPORTED, NO_DEVICE = 1, 2, 4


def _create(**kw):
    d = dict(bs=2, ic=32, ih=9, iw=11, oc=32, oh=9, ow=11, groups=4, kh=3, kw=3, sh=1, sw=1, pad_t=1, pad_l=1,
             dst_dt=capi.DFX_U8, bia_dt=capi.DFX_UNDEF, relu=0, round_mode=capi.ROUND_NEAREST, nscales=1,
             force_path=capi.GCONV_AUTO)
    d.update(kw)
    desc = capi.GConvDesc(**d)
    h = ctypes.c_void_p()
    rc = capi.lib().dfx_gconv_create(ctypes.byref(desc), ctypes.byref(h))
    msg = capi.lib().dfx_last_error().decode()
    if rc == 0:
        assert capi.lib().dfx_gconv_destroy(h) == 0
    else:
        assert not h.value
    return rc, msg


def _admitted(**kw):
    """a valid descriptor gets past validation: it creates with a device and fails with NO_DEVICE without one"""
    rc, msg = _create(**kw)
    assert rc in (0, NO_DEVICE), (kw, rc, msg)


def test_descriptor_validation_needs_no_device():
    for bad in ("bs", "ic", "ih", "iw", "oc", "oh", "ow", "kh", "kw", "sh", "sw"):
        assert _create(**{bad: 0})[0] == INVALID, bad
        assert _create(**{bad: -3})[0] == INVALID, bad
    assert _create(pad_t=-1)[0] == INVALID and _create(pad_l=-1)[0] == INVALID
    _admitted(pad_t=0, pad_l=0, oh=7, ow=9)
    # groups: at least 1, dividing ic and oc
    assert _create(groups=0)[0] == INVALID and _create(groups=-1)[0] == INVALID
    _admitted(groups=1)
    _admitted(groups=32)
    assert _create(groups=3)[0] == INVALID                              # divides neither
    _admitted(ic=24, oc=32, groups=8)                                   # 8 divides ic = 24 and oc = 32 ...
    assert _create(ic=24, oc=36, groups=8, nscales=1)[0] == INVALID     # ... but not oc = 36
    assert _create(ic=36, oc=24, groups=8)[0] == INVALID                # ... nor ic = 36
    _admitted(ic=24, oc=36, groups=3)
    # kh * kw * ic / groups <= 65025 = 255^2: the last admitted and the first rejected value
    _admitted(ic=255, oc=255, groups=1, kh=15, kw=17, pad_t=7, pad_l=8)                     # 15 * 17 * 255 = 65025
    assert _create(ic=255, oc=255, groups=1, kh=15, kw=17 + 1, pad_t=7, pad_l=8)[0] == INVALID
    _admitted(ic=7225 * 2, oc=2, groups=2)                                                  # 9 * 7225 = 65025
    assert _create(ic=7226 * 2, oc=2, groups=2)[0] == INVALID
    _admitted(ic=2, oc=2, groups=2, kh=255, kw=255, pad_t=127, pad_l=127)
    assert _create(ic=2, oc=2, groups=2, kh=255, kw=256, pad_t=127, pad_l=127)[0] == INVALID
    # (oh - 1) * sh - pad_t <= ih - 1, likewise in x: the last admitted and the first rejected output size
    _admitted(oh=10, ow=12)                                             # 9 * 1 - 1 = 8
    assert _create(oh=11)[0] == INVALID                                 # 10 * 1 - 1 = 9 > 8
    assert _create(ow=13)[0] == INVALID
    _admitted(sh=2, sw=2, pad_t=0, pad_l=0, oh=5, ow=6)                 # 4 * 2 = 8
    assert _create(sh=2, sw=2, pad_t=0, pad_l=0, oh=6, ow=6)[0] == INVALID      # 5 * 2 = 10 > 8
    assert _create(dst_dt=capi.DFX_UNDEF)[0] == INVALID
    assert _create(dst_dt=9)[0] == INVALID
    assert _create(bia_dt=7)[0] == INVALID
    assert _create(bia_dt=-1)[0] == INVALID
    assert _create(round_mode=2)[0] == INVALID
    assert _create(nscales=0)[0] == INVALID
    assert _create(nscales=4)[0] == INVALID                             # (the group count is no scale count)
    _admitted(nscales=32)
    assert _create(force_path=2)[0] == INVALID
    assert _create(force_path=-2)[0] == INVALID
    # fewer than 2^31 pixels on either side: the last admitted and the first rejected count, src and dst on their own
    _admitted(bs=(1 << 31) - 1, ih=1, iw=1, oh=1, ow=1)                                     # 2^31 - 1 on both sides
    assert _create(bs=1 << 11, ih=1 << 10, iw=1 << 10, oh=1, ow=1)[0] == INVALID            # src: exactly 2^31
    _admitted(bs=(1 << 11) - 1, ih=1 << 10, iw=1 << 10, oh=1 << 10, ow=1 << 10)
    rc, msg = _create(bs=1 << 30, ih=1, iw=1, oh=2, ow=1)                                   # dst: exactly 2^31 (src 2^30)
    assert rc == INVALID and "pixel count" in msg, (rc, msg)
    _admitted(bs=(1 << 30) - 1, ih=1, iw=1, oh=2, ow=1)
    assert _create(bs=1 << 12, ih=1 << 10, iw=1 << 10, oh=1 << 10, ow=1 << 10)[0] == INVALID     # 2^32 pixels
    # force_path = MFMA outside its class: every clause of the class
    for kw in (dict(kh=5, kw=5, pad_t=2, pad_l=2), dict(kh=1, kw=1, pad_t=0, pad_l=0), dict(kh=3, kw=1, pad_l=0),  # window
               dict(sh=1, sw=2, ow=6), dict(sh=3, sw=3, oh=3, ow=4),                                              # stride
               dict(oc=64), dict(ic=64, groups=8),                                                                # ic != oc
               dict(ic=48, oc=48, groups=6),                                                                      # c % 32
               dict(groups=16), dict(groups=32), dict(ic=96, oc=96, groups=8), dict(ic=128, oc=128, groups=1),    # cpg 2, 1, 12, 128
               dict(bs=1, ic=1 << 20, oc=1 << 20, groups=1 << 18, ih=64, iw=64, oh=64, ow=64),        # a source image of 2^32 bytes
               dict(bs=1, ic=1 << 18, oc=1 << 18, groups=1 << 16, ih=64, iw=64, oh=64, ow=64, dst_dt=capi.DFX_S32)):  # a dst image
        rc, msg = _create(force_path=capi.GCONV_MFMA, **kw)
        assert rc == UNSUPPORTED and "MFMA kernel's class" in msg, (kw, rc, msg)
        _admitted(**kw)                                                  # on auto the op is total
    # one image below 2^31 bytes on either side: exactly 2^31 is outside the class, the largest size a multiple of 32
    # channels can form below it is inside (src: 2^31 - 32; dst, 4-byte: 2^31 - 128)
    big = dict(bs=1, ic=32, oc=32, groups=8, ih=1)
    for out, ok in ((dict(iw=1 << 26, oh=1, ow=1), dict(iw=(1 << 26) - 1, oh=1, ow=1)),
                    (dict(iw=1 << 26, oh=1, ow=1 << 26), dict(iw=(1 << 26) - 1, oh=1, ow=(1 << 26) - 1)),      # u8 dst as well
                    (dict(iw=1 << 24, oh=1, ow=1 << 24, dst_dt=capi.DFX_S32), dict(iw=1 << 24, oh=1, ow=(1 << 24) - 1, dst_dt=capi.DFX_S32)),
                    (dict(iw=1 << 24, oh=1, ow=1 << 24, dst_dt=capi.DFX_F32), dict(iw=1 << 24, oh=1, ow=(1 << 24) - 1, dst_dt=capi.DFX_F32))):
        rc, msg = _create(force_path=capi.GCONV_MFMA, **big, **out)
        assert rc == UNSUPPORTED and "MFMA kernel's class" in msg and "2^31 bytes" in msg, (out, rc, msg)
        _admitted(**big, **out)
        _admitted(force_path=capi.GCONV_MFMA, **big, **ok)
    for kw in (dict(), dict(sh=2, sw=2, oh=5, ow=6), dict(groups=8), dict(groups=2), dict(groups=1),
               dict(ic=64, oc=64, groups=1), dict(ic=96, oc=96, groups=3)):
        _admitted(force_path=capi.GCONV_MFMA, **kw)                      # every admitted value of each clause
    # null arguments
    L = capi.lib()
    assert L.dfx_gconv_create(None, ctypes.byref(ctypes.c_void_p())) == INVALID
    assert L.dfx_gconv_create(ctypes.byref(capi.GConvDesc()), None) == INVALID
    assert L.dfx_gconv_submit(None, None, None, None) == INVALID
    assert L.dfx_gconv_submit_host(None, None, None) == INVALID
    assert L.dfx_gconv_set_weights(None, None, None, None) == INVALID
    assert L.dfx_gconv_query(None, None) == INVALID
    assert L.dfx_debug_gconv_requant(None, None) == INVALID
    assert L.dfx_gconv_destroy(None) == 0
    # a bad descriptor is refused through the Python class as well
    with pytest.raises(dfa.DfxError) as e:
        dfa.GroupConv((1, 4, 4, 32), 32, 4, (3, 3), nscales=5)
    assert "dfx error 1" in str(e.value)


VALID = [
    dict(),                                                                         # MFMA class
    dict(sh=2, sw=2, pad_t=0, pad_l=0, oh=5, ow=6, relu=1, round_mode=capi.ROUND_DOWN),     # windows hang over
    dict(ic=128, oc=128, groups=2, dst_dt=capi.DFX_S32, bia_dt=capi.DFX_F32, nscales=128),  # cpg 64
    dict(force_path=capi.GCONV_MFMA),
    dict(force_path=capi.GCONV_GENERIC),
    dict(ic=24, oc=36, groups=3, nscales=36),                                       # outside it: the generic path
    dict(groups=1), dict(groups=32), dict(kh=7, kw=7, pad_t=3, pad_l=3), dict(kh=1, kw=3, pad_t=0), dict(sh=1, sw=2, ow=6),
    dict(ic=20, oc=20, groups=5),
    dict(pad_t=5, pad_l=4, oh=14, ow=15),                                           # windows entirely in the padding
]


def test_valid_descriptors_and_no_cpu_fallback():
    """valid descriptors pass validation, inside and outside the MFMA class: with a device they create and destroy
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
            dfa.GroupConv((1, 4, 4, 32), 32, 4, (3, 3))
        assert "dfx error 4" in str(e.value) and "no HIP device" in str(e.value)


def test_gconv_structs_match_the_header(tmp_path):
    """dfx_gconv_desc / dfx_gconv_info compiled by gcc have the sizes and field offsets of the ctypes mirrors"""
    pairs = {"dfx_gconv_desc": capi.GConvDesc, "dfx_gconv_info": capi.GConvInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dfx.h"', 'int main(void) {']
    for cname, ct in pairs.items():
        lines.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in ct._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines.append('printf("path mfma %d\\n", DFX_GCONV_MFMA); printf("path generic %d\\n", DFX_GCONV_GENERIC);')
    lines.append('printf("dfx_conv_desc size %zu\\n", sizeof(dfx_conv_desc));')
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
    assert seen[("path", "mfma")] == capi.GCONV_MFMA == R.MFMA and seen[("path", "generic")] == capi.GCONV_GENERIC == R.GENERIC
    assert capi.GCONV_AUTO == -1
    assert [n for n, _ in capi.GConvDesc._fields_] == ["bs", "ic", "ih", "iw", "oc", "oh", "ow", "groups", "kh", "kw", "sh",
                                                       "sw", "pad_t", "pad_l", "dst_dt", "bia_dt", "relu", "round_mode",
                                                       "nscales", "force_path"]
    assert [n for n, _ in capi.GConvInfo._fields_] == [n for n, _ in capi.DwConvInfo._fields_]
    assert ctypes.sizeof(capi.GConvInfo) == ctypes.sizeof(capi.DwConvInfo)
    # the conv's descriptor is untouched
    assert ctypes.sizeof(capi.ConvDesc) == 100 == seen[("dfx_conv_desc", "size")] and len(capi.ConvDesc._fields_) == 25


def test_library_exports_the_gconv_entry_points():
    L = capi.lib()
    for s in ("dfx_gconv_create", "dfx_gconv_set_weights", "dfx_gconv_submit", "dfx_gconv_submit_host",
              "dfx_gconv_query", "dfx_gconv_destroy", "dfx_debug_gconv_requant"):
        assert s in dfa.declared_symbols() and hasattr(L, s), s
    assert not [s for s in dfa.declared_symbols() if not hasattr(L, s)]
    for name in ("GroupConv", "GConvDesc", "GConvInfo", "GCONV_AUTO", "GCONV_MFMA", "GCONV_GENERIC"):
        assert hasattr(dfa, name), name


def test_dropin_layer_exports_grouped_conv_and_tools_are_built():
    so = os.path.join(PKG, "libdeepfusion.so")
    assert os.path.exists(so), "run __graft_entry__.build() first"
    syms = subprocess.check_output(["nm", "-D", "-C", "--defined-only", so]).decode()
    assert "deepfusion::grouped_conv(" in syms
    for tool in ("gconv_check", "bench_gconv"):
        exe = os.path.join(PKG, "tools", tool)
        assert os.path.exists(exe) and os.access(exe, os.X_OK), tool


def test_tables_cover_what_they_claim():
    m, o, g = R.mfma_table(), R.options_table(), R.generic_table()
    assert all(c.mfma_class for c in m + o) and not any(c.mfma_class for c in g)
    assert all(c.bs == 2 for c in m)
    # every cpg with full and partial 128-channel chunks; cpg 64 with one, two and three groups
    for cpg in (4, 8, 16, 32):
        assert {c.c for c in m if c.cpg == cpg} >= {32, 96, 128, 160, 256}, cpg
    assert {c.c for c in m if c.cpg == 64} == {64, 128, 192}
    assert {c.cpg for c in m} == set(R.MFMA_CPG)
    assert any(c.c % 128 for c in m) and any(c.c % 128 == 0 for c in m) and any(c.c > 128 and c.c % 128 for c in m)
    geoms = {(c.stride, c.pad, c.ih, c.iw, c.out_hw) for c in m}
    for ihw in ((1, 1), (3, 3), (7, 7), (5, 9), (13, 37), (3, 200)):
        assert ((1, 1), (1, 1)) + ihw + (None,) in geoms, ihw
    assert ((1, 1), (0, 0), 5, 6, None) in geoms and ((1, 1), (2, 2), 4, 5, None) in geoms
    for ihw in ((8, 8), (7, 7), (9, 14)):
        assert ((2, 2), (1, 1)) + ihw + (None,) in geoms, ihw
    assert ((2, 2), (0, 0), 8, 8, (4, 4)) in geoms and ((2, 2), (0, 0), 7, 10, (4, 5)) in geoms
    # every geometry meets every (c, cpg)
    per_geom = {}
    for c in m:
        if c.name != "s1p1-long":
            per_geom.setdefault((c.stride, c.pad, c.ih, c.iw, c.out_hw), set()).add((c.c, c.cpg))
    assert len(per_geom) == 12 and all(v == set(R.MFMA_CHANNELS) for v in per_geom.values())
    assert len(o) == 2 * len(R.OPTIONS) and {c.stride for c in o} == {(1, 1), (2, 2)} and {(c.c, c.cpg) for c in o} == {(96, 8)}
    for t in (o, m, m + g):
        assert {c.dst_dt for c in t} == {C.U8, C.S8, C.S32, C.F32}
        assert {c.bia_dt for c in t} == {C.UNDEF, C.F32, C.S32, C.S8, C.U8}
        assert {c.per_channel for c in t} == {True, False} and {c.rm for c in t} == {0, 1} and {c.relu for c in t} == {True, False}
        assert any(c.wide for c in t)
    assert {(c.c, c.oc, c.groups) for c in g} >= {(24, 36, 3), (240, 60, 3), (32, 64, 4)}
    assert {c.k for c in g} >= {(1, 1), (5, 5), (7, 7), (1, 3)} and {c.stride for c in g} >= {(1, 2), (2, 1)}
    assert {c.cpg for c in g} >= {1, 2, 3, 12, 24} and any(c.groups == 1 for c in g) and any(c.c == 20 for c in g)
    assert len({c.ident() for c in R.all_tables()}) == len(R.all_tables())


@pytest.mark.parametrize("impl", ["scalar_mt", "avx512"])
def test_reference_equals_the_oracles_dense_conv_with_block_diagonal_weights(oracle, impl):
    """every table case the dense conv can express: this pins the reference of the GPU tests"""
    if impl == "avx512" and not oracle.have_avx512_vnni():
        impl = "scalar"       # the oracle's other implementation on a host without AVX-512 VNNI
    tables = R.all_tables()
    n = 0
    for case in tables:
        if not case.dense_expressible:
            continue
        data = R.generate(case)
        want = hipref.oracle_conv(oracle, R.dense_case(case), R.dense_data(case, data), impl=impl)
        hipref.assert_bit_equal(R.gconv_ref(case, data), want, "%s vs oracle %s" % (case.ident(), impl))
        n += 1
    assert n >= len([c for c in tables if c.c % 16 == 0 and c.oc % 16 == 0 and c.out_hw is None]) > 200


def test_block_diag_weights_are_the_headers_formula():
    case = R.GCase("bd", 1, 24, 3, 3, 36, 3)
    w = R.generate(case)["w"]
    d = R.block_diag_weights(w, 3)
    assert d.shape == (36, 24, 3, 3)
    for o in range(36):
        g = o // 12
        for j in range(24):
            want = w[o, j - g * 8] if g * 8 <= j < (g + 1) * 8 else 0
            assert np.array_equal(d[o, j], np.broadcast_to(want, (3, 3))), (o, j)


@pytest.mark.parametrize("c,cpg", [(128, 4), (128, 64), (24, 8)])
def test_group_isolation_on_the_reference(c, cpg):
    """with the source non-zero only in the channels of groups != g, group g's outputs are the bias alone"""
    for g in range(c // cpg):
        case, data, want = R.isolation_case(c, cpg, g)
        ref = R.gconv_ref(case, data)
        assert (ref[..., g * cpg:(g + 1) * cpg] == want).all(), g
        other = np.delete(ref, np.s_[g * cpg:(g + 1) * cpg], axis=3) - np.delete(data["bia"], np.s_[g * cpg:(g + 1) * cpg])
        assert other.any()


def test_wide_cases_reach_both_ends_of_the_range():
    """a "wide" 1-byte case's expected output holds both ends of what its dtype and ReLU flag can reach"""
    n = 0
    for case in R.all_tables():                     # every wide 1-byte case, the 1x1 images (2 pixels) included
        if not case.wide or case.dst_dt not in (C.U8, C.S8):
            continue
        ref = R.gconv_ref(case, R.generate(case))
        lo = 0 if (case.relu or case.dst_dt == C.U8) else -128
        hi = 255 if case.dst_dt == C.U8 else 127
        assert ref.min() == lo and ref.max() == hi, (case.ident(), ref.min(), ref.max())
        n += 1
    assert n >= 8


def test_nan_and_inf_scales_give_the_x86_results():
    """NaN -> 0x80000000 -> u8 255 / s8 -128; +inf * positive likewise (out of range), on the reference"""
    for dst_dt, bad in ((C.U8, 255), (C.S8, -128)):
        case = R.GCase("nan", 1, 32, 4, 4, 32, 4, dst_dt=dst_dt, bia_dt=C.UNDEF, relu=False, per_channel=True)
        data = R.generate(case)
        data["scales"][3] = np.nan
        data["scales"][7] = np.inf
        data["src"][...] = np.maximum(data["src"], 1)
        data["w"][7] = np.abs(data["w"][7]) + 1
        ref = R.gconv_ref(case, data)
        assert (ref[..., 3] == bad).all() and (ref[..., 7] == bad).all()


@pytest.mark.parametrize("edge", R.EDGES, ids=lambda e: e.name)
def test_edge_data_attains_the_bound_the_proof_uses(edge):
    """(255 * max(P, N) + |bias|) * scale is exactly 2^30 at the last admitted value, one scale step beyond at the first
    rejected one, the prescribed weights sit on several input channels of the group, and the centre pixel's accumulator
    is exactly 255 P / -255 N"""
    case, data = R.edge_case(edge, C.S32)
    assert case.mfma_class
    w = data["w"][R.EDGE_CHANNEL]
    assert sorted(w.flatten().tolist()) == sorted(edge.weights + (0,) * 27)
    assert len([i for i in range(R.EDGE_CPG) if w[i].any()]) >= 2
    acc, bound, P, N = R.edge_attained(edge, case, data)
    assert acc == bound and abs(bound) == 255 * max(P, N)
    reach = (255 * max(P, N) + abs(edge.bias)) * edge.scale
    assert reach == (R.LIMIT if edge.fast else R.LIMIT + edge.scale)
    assert float(np.float32(edge.bias)) == edge.bias and float(np.float32(edge.scale)) == edge.scale     # exact in f32
    ref = R.gconv_ref(case, data)
    img = 0 if edge.which == "max" else 1
    sign = 1 if edge.which == "max" else -1
    assert int(ref[img, 1, 1, R.EDGE_CHANNEL]) == sign * int(reach)            # the s32 result shows it: no saturation yet
