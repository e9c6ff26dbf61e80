"""CPU-only checks of the concat + pointwise conv op: the C ABI validates descriptors and submit arguments before it
touches a device, the ctypes mirrors match the header, the symbols are exported, and the drop-in layer and its
tools are built."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-fusion_amd")
INVALID, UNSUPPORTED, NO_DEVICE = 1, 2, 4


def _create(channels=(128, 128), **kw):
    d = dict(bs=2, h=5, w=7, oc=64, dst_dt=capi.DFX_U8, bia_dt=capi.DFX_UNDEF, relu=0, round_mode=capi.ROUND_NEAREST,
             nscales=1, force_path=capi.CATCONV_AUTO)
    d.update(kw)
    n = d.pop("n_inputs", None if channels is None else len(channels))
    ch = None if channels is None else (ctypes.c_int32 * len(channels))(*channels)
    desc = capi.CatConvDesc(n_inputs=n or 0, channels=ch, **d)
    h = ctypes.c_void_p()
    rc = capi.lib().dfx_catconv_create(ctypes.byref(desc), ctypes.byref(h))
    msg = capi.lib().dfx_last_error().decode()
    if rc == 0:
        assert capi.lib().dfx_catconv_destroy(h) == 0
    else:
        assert not h.value
    return rc, msg


def test_descriptor_validation_needs_no_device():
    for bad in ("bs", "h", "w", "oc"):
        assert _create(**{bad: 0})[0] == INVALID, bad
        assert _create(**{bad: -3})[0] == INVALID, bad
    assert _create(channels=(256,))[0] == INVALID                               # n_inputs 2 .. 16
    assert _create(channels=(16,) * 17)[0] == INVALID
    assert _create(n_inputs=0)[0] == INVALID
    assert _create(channels=None, n_inputs=2)[0] == INVALID                     # null channels
    rc, msg = _create(channels=(128, 24))
    assert rc == INVALID and "multiple of 16" in msg
    assert _create(channels=(128, 0))[0] == INVALID
    assert _create(channels=(128, -16))[0] == INVALID
    assert _create(dst_dt=capi.DFX_UNDEF)[0] == INVALID
    assert _create(dst_dt=9)[0] == INVALID
    assert _create(bia_dt=7)[0] == INVALID
    assert _create(bia_dt=-1)[0] == INVALID
    assert _create(round_mode=2)[0] == INVALID
    assert _create(nscales=0)[0] == INVALID
    assert _create(nscales=7)[0] == INVALID
    assert _create(force_path=2)[0] == INVALID
    assert _create(force_path=-2)[0] == INVALID
    assert _create(oc=72)[0] == INVALID                                         # what dfx_conv_create rejects: oc % 16
    assert _create(bs=1 << 12, h=1 << 10, w=1 << 10)[0] == INVALID              # 2^32 pixels
    # null arguments
    L = capi.lib()
    assert L.dfx_catconv_create(None, ctypes.byref(ctypes.c_void_p())) == INVALID
    assert L.dfx_catconv_submit(None, None, None, None) == INVALID
    assert L.dfx_catconv_submit_host(None, None, None) == INVALID
    assert L.dfx_catconv_set_weights(None, None, None, None) == INVALID
    assert L.dfx_catconv_query(None, None) == INVALID
    assert L.dfx_catconv_destroy(None) == 0
    # a bad descriptor is refused through the Python class as well
    with pytest.raises(dfa.DfxError) as e:
        dfa.ConcatConv(1, 4, 4, [128, 40], 64)
    assert "dfx error 1" in str(e.value)


def test_valid_descriptors_and_no_cpu_fallback():
    """valid descriptors pass validation, inside the fused class and outside it: with a device they create and
    destroy cleanly, without one they fail at the first device call (there is no CPU path)"""
    import torch
    for kw in (dict(), dict(channels=(64, 128, 32, 32), oc=128, dst_dt=capi.DFX_S32, bia_dt=capi.DFX_F32, nscales=128),
               dict(channels=(16, 48), oc=96, relu=1, round_mode=capi.ROUND_DOWN), dict(channels=(32,) * 16, oc=256),
               dict(force_path=capi.CATCONV_TWO_LAUNCH)):
        rc, msg = _create(**kw)
        if torch.cuda.is_available():
            assert rc == 0, msg
        else:
            assert rc == NO_DEVICE and "no HIP device" in msg, (rc, msg)
    if not torch.cuda.is_available():
        with pytest.raises(dfa.DfxError) as e:
            dfa.ConcatConv(1, 4, 4, [128, 128], 64)
        assert "no HIP device" in str(e.value)


def test_catconv_structs_match_the_header(tmp_path):
    """dfx_catconv_desc / dfx_catconv_info compiled by gcc have the sizes and field offsets of the ctypes mirrors"""
    pairs = {"dfx_catconv_desc": capi.CatConvDesc, "dfx_catconv_info": capi.CatConvInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dfx.h"', 'int main(void) {']
    for cname, ct in pairs.items():
        lines.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in ct._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines.append('printf("path fused %d\\n", DFX_CATCONV_FUSED); printf("path two %d\\n", DFX_CATCONV_TWO_LAUNCH);')
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
    assert seen[("path", "fused")] == capi.CATCONV_FUSED and seen[("path", "two")] == capi.CATCONV_TWO_LAUNCH
    assert [n for n, _ in capi.CatConvDesc._fields_] == ["n_inputs", "bs", "h", "w", "oc", "dst_dt", "bia_dt", "relu",
                                                         "round_mode", "nscales", "force_path", "channels"]
    assert [n for n, _ in capi.CatConvInfo._fields_] == ["path", "grid", "block", "lds_bytes", "device", "algorithmic_ops",
                                                         "algorithmic_bytes", "kernel_name"]


def test_library_exports_the_catconv_entry_points():
    L = capi.lib()
    for s in ("dfx_catconv_create", "dfx_catconv_set_weights", "dfx_catconv_submit", "dfx_catconv_submit_host",
              "dfx_catconv_query", "dfx_catconv_destroy"):
        assert s in dfa.declared_symbols() and hasattr(L, s), s
    assert L.dfx_version() == 100


def test_conv_descriptor_is_untouched(tmp_path):
    """the op has its own descriptor: dfx_conv_desc keeps its 25 int32 fields"""
    assert ctypes.sizeof(capi.ConvDesc) == 100 and len(capi.ConvDesc._fields_) == 25


def test_dropin_layer_exports_concat_conv_and_tools_are_built():
    so = os.path.join(PKG, "libdeepfusion.so")
    assert os.path.exists(so), "run __graft_entry__.build() first"
    syms = subprocess.check_output(["nm", "-D", "-C", "--defined-only", so]).decode()
    assert "deepfusion::concat_conv(" in syms
    for tool in ("catconv_check", "bench_catconv"):
        exe = os.path.join(PKG, "tools", tool)
        assert os.path.exists(exe) and os.access(exe, os.X_OK), tool
