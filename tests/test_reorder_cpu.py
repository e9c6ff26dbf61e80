"""CPU-only checks of the activation reorder: the numpy reference agrees with an independent witness on the
whole case table, the C ABI validates descriptors before it touches a device, the ctypes mirror matches the
header, and the drop-in layer and its tools are built."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

import reorder_ref as R

dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-fusion_amd")


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("lay", R.LAYOUTS, ids=lambda l: "%s-%s" % (R.FMT_NAME[l[0]], R.FMT_NAME[l[1]]))
def test_reference_equals_witness_on_the_table(lay):
    cases = R.table(layouts=[lay])
    assert len(cases) > 300
    for c in cases:
        src, sc = R.generate(c), R.make_scales(c)
        a, b = R.reference(src, c, sc), R.witness(src, c, sc)
        assert a.dtype == b.dtype and a.shape == b.shape == c.dst_shape, c.ident()
        assert np.array_equal(_bits(a), _bits(b)), c.ident()


def test_table_covers_what_it_should():
    t = R.table()
    assert {(c.src_fmt, c.dst_fmt) for c in t} == set(R.LAYOUTS)
    assert {(c.src_dt, c.dst_dt) for c in t} == set(R.DTYPE_PAIRS)
    assert {c.shape for c in t} >= set(R.SHAPES)
    assert {(c.shape[1], c.dst_c) for c in t} >= {(3, 16), (3, 4), (17, 32), (64, 48), (16, 3)}
    for lay in R.LAYOUTS:
        for dts in R.DTYPE_PAIRS:
            sub = [c for c in t if (c.src_fmt, c.dst_fmt) == lay and (c.src_dt, c.dst_dt) == dts]
            assert {(c.scale_mode, c.rm) for c in sub} == {(s, r) for s in R.SCALE_MODES for r in R.ROUND_MODES}


def test_rounding_and_saturation_pins():
    """the points the semantics name: ties to even at +-0.5, 254.5, 255.5; NaN -> 0; saturation of the value"""
    x = np.array([0.5, -0.5, 1.5, 2.5, 254.5, 255.5, 300.0, -3.0, np.nan, np.inf, -np.inf, 127.5, -128.5],
                 dtype=np.float32).reshape(1, 13, 1, 1)
    c = R.ReorderCase((1, 13, 1, 1), 13, R.NCHW, R.NCHW, R.F32, R.U8)
    assert R.reference(x, c, None).reshape(-1).tolist() == [0, 0, 2, 2, 254, 255, 255, 0, 0, 255, 0, 128, 0]
    c = R.ReorderCase((1, 13, 1, 1), 13, R.NCHW, R.NCHW, R.F32, R.S8)
    assert R.reference(x, c, None).reshape(-1).tolist() == [0, 0, 2, 2, 127, 127, 127, -3, 0, 127, -128, 127, -128]
    c = R.ReorderCase((1, 13, 1, 1), 13, R.NCHW, R.NCHW, R.F32, R.S8, rm=R.DOWN)
    assert R.reference(x, c, None).reshape(-1).tolist() == [0, -1, 1, 2, 127, 127, 127, -3, 0, 127, -128, 127, -128]


def _create(scales=None, **kw):
    d = dict(bs=2, h=5, w=7, src_c=8, dst_c=8, src_fmt=capi.FMT_NCHW, dst_fmt=capi.FMT_NHWC, src_dt=capi.DFX_F32,
             dst_dt=capi.DFX_U8, round_mode=capi.ROUND_NEAREST, n_scales=0)
    d.update(kw)
    desc = capi.ReorderDesc(**d)
    sc = None if scales is None else np.ascontiguousarray(scales, dtype=np.float32)
    h = ctypes.c_void_p()
    rc = capi.lib().dfx_reorder_create(ctypes.byref(desc), None if sc is None else sc.ctypes.data_as(ctypes.c_void_p),
                                       ctypes.byref(h))
    msg = capi.lib().dfx_last_error().decode()
    if rc == 0:
        assert capi.lib().dfx_reorder_destroy(h) == 0
    return rc, msg


def test_descriptor_validation_needs_no_device():
    INVALID, UNSUPPORTED = 1, 2
    for bad in ("bs", "h", "w", "src_c", "dst_c"):
        assert _create(**{bad: 0})[0] == INVALID, bad
        assert _create(**{bad: -3})[0] == INVALID, bad
    assert _create(src_fmt=2)[0] == INVALID
    assert _create(dst_fmt=-1)[0] == INVALID
    assert _create(src_dt=capi.DFX_UNDEF)[0] == INVALID
    assert _create(src_dt=5)[0] == INVALID
    assert _create(dst_dt=capi.DFX_UNDEF)[0] == INVALID
    assert _create(dst_dt=9)[0] == INVALID
    assert _create(round_mode=2)[0] == INVALID
    assert _create(n_scales=3, scales=np.ones(3))[0] == INVALID
    assert _create(n_scales=2, scales=np.ones(2))[0] == INVALID
    assert _create(n_scales=1)[0] == INVALID                                   # scales missing
    assert _create(n_scales=1, scales=[np.nan])[0] == INVALID
    assert _create(n_scales=8, scales=[1, 2, 3, np.inf, 5, 6, 7, 8])[0] == INVALID
    rc, msg = _create(dst_dt=capi.DFX_S32)
    assert rc == UNSUPPORTED and "s32" in msg
    rc, msg = _create(h=1 << 15, w=1 << 15, src_c=2, dst_c=2)                  # one image of 2^31 elements
    assert rc == UNSUPPORTED
    # a bad descriptor is refused through the Python class as well
    with pytest.raises(dfa.DfxError) as e:
        dfa.Reorder((1, 8, 4, 4), np.float32, np.uint8, scales=np.ones(5, dtype=np.float32))
    assert "dfx error 1" in str(e.value)


def test_valid_descriptor_and_no_cpu_fallback():
    """a valid descriptor passes validation: with a device it creates and destroys cleanly, without one it
    fails at the first device call (there is no CPU path), as Conv does"""
    import torch
    for kw in (dict(), dict(n_scales=1, scales=[0.5]), dict(n_scales=8, scales=np.arange(1, 9)),
               dict(src_dt=capi.DFX_S32, dst_dt=capi.DFX_F32, dst_c=16), dict(src_fmt=capi.FMT_NHWC, dst_fmt=capi.FMT_NHWC)):
        rc, msg = _create(**kw)
        if torch.cuda.is_available():
            assert rc == 0, msg
        else:
            assert rc == 4 and "no HIP device" in msg, (rc, msg)
    if not torch.cuda.is_available():
        with pytest.raises(dfa.DfxError) as e:
            dfa.Reorder((1, 8, 4, 4), np.float32, np.uint8)
        assert "no HIP device" in str(e.value)


def test_reorder_structs_match_the_header(tmp_path):
    """dfx_reorder_desc / dfx_reorder_info compiled by gcc have the sizes and field offsets of the ctypes mirrors"""
    pairs = {"dfx_reorder_desc": capi.ReorderDesc, "dfx_reorder_info": capi.ReorderInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dfx.h"', 'int main(void) {']
    for cname, ct in pairs.items():
        lines.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in ct._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines.append('printf("fmt nhwc %d\\n", DFX_FMT_NHWC); printf("fmt nchw %d\\n", DFX_FMT_NCHW);')
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
    assert seen[("fmt", "nhwc")] == capi.FMT_NHWC and seen[("fmt", "nchw")] == capi.FMT_NCHW
    assert [n for n, _ in capi.ReorderDesc._fields_] == ["bs", "h", "w", "src_c", "dst_c", "src_fmt", "dst_fmt", "src_dt",
                                                         "dst_dt", "round_mode", "n_scales"]


def test_library_exports_the_reorder_entry_points():
    L = capi.lib()
    for s in ("dfx_reorder_create", "dfx_reorder_submit", "dfx_reorder_submit_host", "dfx_reorder_query",
              "dfx_reorder_destroy"):
        assert s in dfa.declared_symbols() and hasattr(L, s), s
    assert L.dfx_version() == 100


def test_dropin_layer_exports_reorder_and_tools_are_built():
    so = os.path.join(PKG, "libdeepfusion.so")
    assert os.path.exists(so), "run __graft_entry__.build() first"
    syms = subprocess.check_output(["nm", "-D", "-C", "--defined-only", so]).decode()
    assert "deepfusion::reorder(" in syms
    for tool in ("reorder_check", "bench_reorder"):
        exe = os.path.join(PKG, "tools", tool)
        assert os.path.exists(exe) and os.access(exe, os.X_OK), tool
