"""CPU-only checks of the depthwise + pointwise conv op: the C ABI validates descriptors before it touches a device, the
ctypes mirrors match the header, the symbols are exported, the drop-in layer and its tools are built, the numpy
reference the GPU tests compare against equals the C oracle (dw_ref to u8 then the oracle's unfused 1x1 conv, and the
oracle's FUSED conv with block-diagonal conv0 weights), and the test data keeps the promises the GPU tests rely on."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

import cases as C
import dwpw_ref as R
import hipref

dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-fusion_amd")
INVALID, UNSUPPORTED, NO_DEVICE = 1, 2, 4


def _create(**kw):
    d = dict(bs=2, c=32, ih=9, iw=11, oh=9, ow=11, kh=3, kw=3, sh=1, sw=1, pad_t=1, pad_l=1, oc=64, dst_dt=capi.DFX_U8,
             bia0_dt=capi.DFX_UNDEF, bia1_dt=capi.DFX_UNDEF, relu=0, round_mode0=capi.ROUND_NEAREST,
             round_mode1=capi.ROUND_NEAREST, nscales0=1, nscales1=1, force_path=capi.DWPW_AUTO)
    d.update(kw)
    desc = capi.DwPwDesc(**d)
    h = ctypes.c_void_p()
    rc = capi.lib().dfx_dwpw_create(ctypes.byref(desc), ctypes.byref(h))
    msg = capi.lib().dfx_last_error().decode()
    if rc == 0:
        assert capi.lib().dfx_dwpw_destroy(h) == 0
    else:
        assert not h.value
    return rc, msg


def test_descriptor_validation_needs_no_device():
    for bad in ("bs", "c", "ih", "iw", "oh", "ow", "kh", "kw", "sh", "sw", "oc"):
        assert _create(**{bad: 0})[0] == INVALID, bad
        assert _create(**{bad: -3})[0] == INVALID, bad
    assert _create(pad_t=-1)[0] == INVALID
    assert _create(pad_l=-1)[0] == INVALID
    assert _create(kh=256, pad_t=128)[0] == INVALID
    assert _create(kw=256, pad_l=128)[0] == INVALID
    assert _create(oh=11)[0] == INVALID                                # 10 * 1 - 1 = 9 > 8
    assert _create(ow=13)[0] == INVALID
    assert _create(sh=2, sw=2, pad_t=0, pad_l=0, oh=6, ow=6)[0] == INVALID
    assert _create(dst_dt=capi.DFX_UNDEF)[0] == INVALID
    assert _create(dst_dt=9)[0] == INVALID
    for b in ("bia0_dt", "bia1_dt"):
        assert _create(**{b: 7})[0] == INVALID
        assert _create(**{b: -1})[0] == INVALID
    assert _create(round_mode0=2)[0] == INVALID
    assert _create(round_mode1=2)[0] == INVALID
    assert _create(nscales0=0)[0] == INVALID
    assert _create(nscales0=64)[0] == INVALID                          # oc, not c
    assert _create(nscales1=0)[0] == INVALID
    assert _create(nscales1=32)[0] == INVALID                          # c, not oc
    assert _create(force_path=2)[0] == INVALID
    assert _create(force_path=-2)[0] == INVALID
    assert _create(bs=1 << 12, ih=1 << 10, iw=1 << 10, oh=1 << 10, ow=1 << 10)[0] == INVALID     # 2^32 pixels
    # force_path = FUSED outside the class: every clause of the class
    for kw in (dict(c=48), dict(c=16), dict(c=288), dict(c=512), dict(oc=96), dict(oc=32), dict(oc=512),
               dict(kh=5, kw=5, pad_t=2, pad_l=2), dict(kh=1, kw=1, pad_t=0, pad_l=0), dict(kh=3, kw=5, pad_l=2),
               dict(sh=1, sw=2, ow=6), dict(sh=3, sw=3, oh=3, ow=4),
               dict(bs=1, c=256, ih=2048, iw=4096, oh=2048, ow=4096),                       # one source image of 2^31 bytes
               dict(bs=1, c=32, ih=2048, iw=2048, oh=2048, ow=2048, oc=256, dst_dt=capi.DFX_S32),   # one dst image of 2^32 bytes
               # one image of the u8 tensor BETWEEN the stages of 2^31 bytes (src and dst images are smaller): pad 2
               dict(bs=1, c=256, ih=4094, iw=2046, oh=4096, ow=2048, pad_t=2, pad_l=2, oc=64)):
        rc, msg = _create(force_path=capi.DWPW_FUSED, **kw)
        assert rc == UNSUPPORTED and "fused kernel's class" in msg, (kw, rc, msg)
    # null arguments
    L = capi.lib()
    assert L.dfx_dwpw_create(None, ctypes.byref(ctypes.c_void_p())) == INVALID
    assert L.dfx_dwpw_submit(None, None, None, None) == INVALID
    assert L.dfx_dwpw_submit_host(None, None, None) == INVALID
    assert L.dfx_dwpw_set_weights(None, None, None, None, None, None, None) == INVALID
    assert L.dfx_dwpw_query(None, None) == INVALID
    assert L.dfx_debug_dwpw_requant(None, None) == INVALID
    assert L.dfx_dwpw_destroy(None) == 0
    with pytest.raises(dfa.DfxError) as e:
        dfa.DwPwConv((1, 4, 4, 32), (3, 3), 64, nscales1=5)
    assert "dfx error 1" in str(e.value)


VALID = [
    dict(),
    dict(sh=2, sw=2, oh=5, ow=6, dst_dt=capi.DFX_S32, bia0_dt=capi.DFX_F32, bia1_dt=capi.DFX_S8, nscales0=32, nscales1=64),
    dict(sh=2, sw=2, pad_t=0, pad_l=0, oh=5, ow=6, relu=1, round_mode0=capi.ROUND_DOWN, round_mode1=capi.ROUND_DOWN),
    dict(force_path=capi.DWPW_FUSED),
    dict(force_path=capi.DWPW_TWO_LAUNCH),
    dict(c=256, oc=256), dict(c=96, oc=128),
    dict(c=48), dict(c=512), dict(oc=96), dict(kh=5, kw=5, pad_t=2, pad_l=2), dict(sh=1, sw=2, ow=6),     # two launches
]


def test_valid_descriptors_and_no_cpu_fallback():
    import torch
    for kw in VALID:
        rc, msg = _create(**kw)
        if torch.cuda.is_available():
            assert rc == 0, (kw, msg)
        else:
            assert rc == NO_DEVICE and "no HIP device" in msg, (kw, rc, msg)
    if not torch.cuda.is_available():
        with pytest.raises(dfa.DfxError) as e:
            dfa.DwPwConv((1, 4, 4, 32), (3, 3), 64)
        assert "dfx error 4" in str(e.value)


def test_dwpw_structs_match_the_header(tmp_path):
    pairs = {"dfx_dwpw_desc": capi.DwPwDesc, "dfx_dwpw_info": capi.DwPwInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dfx.h"', 'int main(void) {']
    for cname, ct in pairs.items():
        lines.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in ct._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines.append('printf("path fused %d\\n", DFX_DWPW_FUSED); printf("path two %d\\n", DFX_DWPW_TWO_LAUNCH);')
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
    assert seen[("path", "fused")] == capi.DWPW_FUSED == R.FUSED and seen[("path", "two")] == capi.DWPW_TWO_LAUNCH == R.TWO_LAUNCH
    assert [n for n, _ in capi.DwPwDesc._fields_] == ["bs", "c", "ih", "iw", "oh", "ow", "kh", "kw", "sh", "sw", "pad_t", "pad_l",
                                                      "oc", "dst_dt", "bia0_dt", "bia1_dt", "relu", "round_mode0",
                                                      "round_mode1", "nscales0", "nscales1", "force_path"]
    assert [n for n, _ in capi.DwPwInfo._fields_] == [n for n, _ in capi.CatConvInfo._fields_]
    assert ctypes.sizeof(capi.DwPwInfo) == ctypes.sizeof(capi.CatConvInfo)
    assert ctypes.sizeof(capi.DwConvDesc) == 72 and ctypes.sizeof(capi.ConvDesc) == 100      # the others are untouched


def test_library_exports_the_dwpw_entry_points():
    L = capi.lib()
    for s in ("dfx_dwpw_create", "dfx_dwpw_set_weights", "dfx_dwpw_submit", "dfx_dwpw_submit_host", "dfx_dwpw_query",
              "dfx_dwpw_destroy", "dfx_debug_dwpw_requant"):
        assert s in dfa.declared_symbols() and hasattr(L, s), s
    assert not [s for s in dfa.declared_symbols() if not hasattr(L, s)]
    for name in ("DwPwConv", "DwPwDesc", "DwPwInfo", "DWPW_AUTO", "DWPW_FUSED", "DWPW_TWO_LAUNCH"):
        assert hasattr(dfa, name), name
    L.dfx_debug_set_tuning.restype = ctypes.c_int
    for key in (b"DFX_DWPW_GRID", b"DFX_DWPW_TH"):                    # known switches (an unknown key is refused)
        assert L.dfx_debug_set_tuning(key, b"1") == 0 and L.dfx_debug_set_tuning(key, None) == 0
    assert L.dfx_debug_set_tuning(b"DFX_DWPW_NOPE", b"1") != 0


def test_dropin_layer_exports_the_op_and_tools_are_built():
    so = os.path.join(PKG, "libdeepfusion.so")
    assert os.path.exists(so), "run __graft_entry__.build() first"
    syms = subprocess.check_output(["nm", "-D", "-C", "--defined-only", so]).decode()
    assert "deepfusion::depthwise_separable_conv(" in syms
    for tool in ("dwpw_check", "bench_dwpw"):
        exe = os.path.join(PKG, "tools", tool)
        assert os.path.exists(exe) and os.access(exe, os.X_OK), tool


def test_tables_cover_what_they_should():
    t, o, x = R.shape_table(), R.options_table(), R.outside_table()
    assert all(c.in_class for c in t + o) and not any(c.in_class for c in x)
    assert {(c.c, c.oc) for c in t} == {(c, oc) for c in R.CHANNELS for oc in R.OUT_CHANNELS}
    s1 = {(c.bs, c.ih, c.iw) for c in t if c.stride == (1, 1) and c.pad == (1, 1)}
    assert s1 >= {(1, 1, 1), (2, 2, 3), (3, 7, 7), (2, 9, 37), (1, 3, 130)} and {c.bs for c in t} == {1, 2, 3}
    assert any(c.out_hw == (4, 4) and (c.ih, c.iw) == (8, 8) and c.pad == (0, 0) for c in t)
    assert any(c.out_hw == (4, 5) and (c.ih, c.iw) == (7, 10) and c.pad == (0, 0) for c in t)
    assert any(c.stride == (2, 2) and c.pad == (1, 1) for c in t)
    tiles = [(c,) + R.tile_of(c) for c in t]
    assert {tw for _, _, tw in tiles} == {16, 32, 42, 128}
    for want_tw in (16, 32, 42, 128):        # a tile narrower than the image with a ragged last tile column
        assert any(tw == want_tw and c.ow > tw and c.ow % tw for c, th, tw in tiles), want_tw
    assert {th for c, th, tw in tiles if c.oh == th + 1} >= {8, 16}
    assert {(c.stride, c.oc, c.dst_dt) for c in t} == {(s_, oc, d) for s_ in ((1, 1), (2, 2)) for oc in R.OUT_CHANNELS
                                                       for d in (C.U8, C.S8, C.S32, C.F32)}      # all 24 kernel instances
    assert any(c.oh < th and c.ow < tw for c, th, tw in tiles)           # an image smaller than one tile
    assert any((th * tw) % 32 for c, th, tw in tiles)                    # a last 32-pixel block that is partly empty
    for tab in (o, t):
        assert {c.dst_dt for c in tab} == {C.U8, C.S8, C.S32, C.F32}
        assert {c.bia0_dt for c in tab} == {C.UNDEF, C.F32, C.S32, C.S8, C.U8} == {c.bia1_dt for c in tab}
        assert {c.pc0 for c in tab} == {c.pc1 for c in tab} == {c.relu for c in tab} == {True, False}
        assert {c.rm0 for c in tab} == {c.rm1 for c in tab} == {0, 1}
        assert any(c.wide for c in tab)
    assert {c.k for c in x} >= {(5, 5)} and {c.c for c in x} >= {48, 512} and {c.oc for c in x} >= {96} and (1, 2) in {c.stride for c in x}
    assert len({c.ident() for c in R.all_tables()}) == len(R.all_tables())
    # forcing the tile height: the case the GPU test uses admits every height of the list
    assert R.heights_that_fit(R.DwPwCase("th", 2, 128, 19, 37, 128)) == [16, 8, 4, 2]


@pytest.mark.parametrize("impl", ["scalar_mt", "avx512"])
def test_reference_equals_the_oracle(oracle, impl):
    """numpy reference == dw_ref to u8 then the oracle's unfused 1x1 conv, on every table case; == the oracle's FUSED
    conv with block-diagonal conv0 weights wherever a dense conv can express the case.  This pins the reference."""
    if impl == "avx512" and not oracle.have_avx512_vnni():
        impl = "scalar"
    n = m = 0
    for case in R.all_tables():
        if case.c % 16 or case.oc % 16:
            continue
        data = R.generate(case)
        want = R.ref(case, data)
        mid = R.mid_ref(case, data)
        two = hipref.oracle_conv(oracle, R.pw_case(case), R.pw_data(case, data, mid), impl=impl)
        hipref.assert_bit_equal(want, two, "%s vs dw_ref + oracle 1x1 %s" % (case.ident(), impl))
        n += 1
        if case.dense_expressible:
            fused = hipref.oracle_conv(oracle, R.fused_dense_case(case), R.fused_dense_data(data), impl=impl)
            hipref.assert_bit_equal(want, fused, "%s vs oracle fused %s" % (case.ident(), impl))
            m += 1
    assert n >= 90 and m >= 85, (n, m)


def test_wide_cases_reach_both_ends_of_the_range():
    """a "wide" case's tensor between the stages holds 0 and 255, and a 1-byte dst both ends of what it can reach"""
    n = 0
    for case in R.all_tables():
        if not case.wide or case.bs * case.oh * case.ow < 16:
            continue
        data = R.generate(case)
        mid = R.mid_ref(case, data)
        assert mid.min() == 0 and mid.max() == 255, case.ident()
        if case.dst_dt in (C.U8, C.S8):
            ref = R.ref(case, data)
            lo = 0 if (case.relu or case.dst_dt == C.U8) else -128
            hi = 255 if case.dst_dt == C.U8 else 127
            assert ref.min() == lo and ref.max() == hi, (case.ident(), ref.min(), ref.max())
            n += 1
    assert n >= 6


@pytest.mark.parametrize("edge", R.EDGES0, ids=lambda e: e.name)
def test_stage0_edge_data_attains_the_bound(edge):
    case, data = R.edge0_case(edge, C.S32)
    acc, bound, P, N = R.edge0_attained(edge, case, data)
    assert acc == bound and abs(bound) == 255 * max(P, N)
    reach = (255 * max(P, N) + abs(edge.bias)) * edge.scale
    assert reach == (R.LIMIT if edge.fast else R.LIMIT + edge.scale)
    assert float(np.float32(edge.bias)) == edge.bias and float(np.float32(edge.scale)) == edge.scale


@pytest.mark.parametrize("edge", R.EDGES1, ids=lambda e: e.name)
def test_stage1_edge_data_attains_the_bound(edge):
    """the depthwise stage drives the tensor between the stages to 255 / 0, so the edge channel's stage-1 accumulator
    is exactly 255 P / -255 N, and the s32 result shows the bound itself: no saturation yet"""
    case, data = R.edge1_case(edge, C.S32)
    mid = R.mid_ref(case, data)
    assert set(np.unique(mid)) == {0, 255}
    acc, bound, P, N = R.edge1_attained(edge, case, data)
    assert acc == bound and abs(bound) == 255 * max(P, N)
    reach = (255 * max(P, N) + abs(edge.bias)) * edge.scale
    assert reach == (R.LIMIT if edge.fast else R.LIMIT + edge.scale)
    assert float(np.float32(edge.bias)) == edge.bias and float(np.float32(edge.scale)) == edge.scale
    ref = R.ref(case, data)
    img = 0 if edge.which == "max" else 1
    sign = 1 if edge.which == "max" else -1
    assert (ref[img, :, :, R.EDGE_CHANNEL] == sign * int(reach)).all()


def test_nan_and_inf_give_the_x86_results_on_the_reference():
    for dst_dt, bad in ((C.U8, 255), (C.S8, -128)):
        case = R.DwPwCase("nan", 1, 32, 4, 4, 64, dst_dt=dst_dt, bia0_dt=C.UNDEF, bia1_dt=C.UNDEF, relu=False, pc0=True, pc1=True)
        data = R.generate(case)
        data["scales1"][3] = np.nan
        data["scales1"][7] = np.inf
        data["src"][...] = np.maximum(data["src"], 1)
        data["w"][...] = np.abs(data["w"]) + 1
        data["w1"][7] = np.abs(data["w1"][7]) + 1
        ref = R.ref(case, data)
        assert (ref[..., 3] == bad).all() and (ref[..., 7] == bad).all()
        data = R.generate(case)
        data["scales0"][5] = np.nan                                    # stage 0: the channel between the stages is 255
        assert (R.mid_ref(case, data)[..., 5] == 255).all()
