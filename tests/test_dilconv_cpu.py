"""CPU-only checks of the dilated conv op: the C ABI validates descriptors before it touches a device, the ctypes mirrors
match the header, the symbols are exported, the drop-in layer and its tools are built, the weight packer is clean under
the host sanitizers (a stand-alone program), the numpy reference the GPU tests compare against (a gather) equals the C
oracle's dense conv on the zero-stuffed weights and the grouped conv's reference with groups = 1, and the test data
keeps the promises the GPU tests rely on."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

import cases as C
import dilconv_ref as R
import gconv_ref as G
import hipref

dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-fusion_amd")
INVALID, UNSUPPORTED, NO_DEVICE = 1, 2, 4


def _create(**kw):
    d = dict(bs=2, ic=32, ih=9, iw=10, oc=32, oh=9, ow=10, kh=3, kw=3, sh=1, sw=1, dh=2, dw=2, pad_t=2, pad_l=2,
             dst_dt=capi.DFX_U8, bia_dt=capi.DFX_UNDEF, relu=0, round_mode=capi.ROUND_NEAREST, nscales=1,
             force_path=capi.DILCONV_AUTO)
    d.update(kw)
    desc = capi.DilConvDesc(**d)
    h = ctypes.c_void_p()
    rc = capi.lib().dfx_dilconv_create(ctypes.byref(desc), ctypes.byref(h))
    msg = capi.lib().dfx_last_error().decode()
    if rc == 0:
        assert capi.lib().dfx_dilconv_destroy(h) == 0
    else:
        assert not h.value
    return rc, msg


def _admitted(**kw):
    """a valid descriptor gets past validation: it creates with a device and fails with NO_DEVICE without one"""
    rc, msg = _create(**kw)
    assert rc in (0, NO_DEVICE), (kw, rc, msg)


def test_descriptor_validation_needs_no_device():
    for bad in ("bs", "ic", "ih", "iw", "oc", "oh", "ow", "kh", "kw", "sh", "sw", "dh", "dw"):
        assert _create(**{bad: 0})[0] == INVALID, bad
        assert _create(**{bad: -3})[0] == INVALID, bad
    # any ic >= 1 and oc >= 1
    for c in (1, 3, 20, 33, 1000):
        _admitted(ic=c)
        _admitted(oc=c)
    # windows, strides and dilations 1 .. 255: the last admitted and the first refused value
    _admitted(kh=1, kw=1, pad_t=0, pad_l=0)
    _admitted(ic=1, kh=255, kw=255, dh=1, dw=1)
    rc, msg = _create(ic=1, kh=256, kw=1, pad_l=0)
    assert rc == INVALID and "window" in msg, (rc, msg)
    assert _create(ic=1, kh=1, kw=256, pad_t=0)[0] == INVALID
    _admitted(sh=255, sw=255, oh=1, ow=1)
    rc, msg = _create(sh=256, oh=1)
    assert rc == INVALID and "stride" in msg, (rc, msg)
    assert _create(sw=256, ow=1)[0] == INVALID
    _admitted(dh=255, dw=255)
    rc, msg = _create(dh=256)
    assert rc == INVALID and "dilation" in msg, (rc, msg)
    assert _create(dw=256)[0] == INVALID
    # 0 <= pad <= (k - 1) * d
    assert _create(pad_t=-1)[0] == INVALID and _create(pad_l=-1)[0] == INVALID
    _admitted(pad_t=0, pad_l=0)
    _admitted(pad_t=4, pad_l=4)                                                  # (3 - 1) * 2
    rc, msg = _create(pad_t=5)
    assert rc == INVALID and "padding" in msg, (rc, msg)
    assert _create(pad_l=5)[0] == INVALID
    _admitted(dh=18, dw=7, pad_t=36, pad_l=14)
    assert _create(dh=18, dw=7, pad_t=37, pad_l=14)[0] == INVALID
    assert _create(dh=18, dw=7, pad_t=36, pad_l=15)[0] == INVALID
    _admitted(kh=1, kw=1, pad_t=0, pad_l=0, dh=9, dw=9)                          # a 1x1 window admits no padding at all
    assert _create(kh=1, kw=1, pad_t=1, pad_l=0, dh=9, dw=9)[0] == INVALID
    # kh * kw * ic <= 65025 = 255^2, counted on the taps that exist: the dilation does not enter
    _admitted(ic=7225)                                                           # 9 * 7225 = 65025
    rc, msg = _create(ic=7226)
    assert rc == INVALID and "65025" in msg, (rc, msg)
    _admitted(ic=7225, dh=255, dw=255)
    _admitted(ic=1, kh=255, kw=255, dh=1, dw=1)
    assert _create(ic=2, kh=255, kw=255, dh=1, dw=1)[0] == INVALID
    _admitted(ic=2048, oc=256, dh=18, dw=18, pad_t=18, pad_l=18)                 # an ASPP branch of a ResNet backbone
    # (oh - 1) * sh - pad_t <= ih - 1, likewise in x: windows may hang over the bottom / right edge
    _admitted(oh=1, ow=1)
    _admitted(oh=11, ow=12)                                                      # 10 - 2 = 8 = ih - 1, 11 - 2 = 9 = iw - 1
    rc, msg = _create(oh=12)
    assert rc == INVALID and "starts below" in msg, (rc, msg)
    assert _create(ow=13)[0] == INVALID
    _admitted(pad_t=0, pad_l=0, oh=9, ow=10)
    assert _create(pad_t=0, oh=10)[0] == INVALID
    assert _create(pad_l=0, ow=11)[0] == INVALID
    _admitted(sh=2, sw=3, oh=6, ow=4)                                            # 5 * 2 - 2 = 8, 3 * 3 - 2 = 7 <= 9
    assert _create(sh=2, oh=7)[0] == INVALID
    assert _create(sw=3, ow=5)[0] == INVALID                                     # 4 * 3 - 2 = 10 > 9
    assert _create(dst_dt=capi.DFX_UNDEF)[0] == INVALID
    assert _create(dst_dt=9)[0] == INVALID
    for dt in (capi.DFX_F32, capi.DFX_S32, capi.DFX_S8, capi.DFX_U8):
        _admitted(dst_dt=dt)
        _admitted(bia_dt=dt)
    assert _create(bia_dt=7)[0] == INVALID
    assert _create(bia_dt=-1)[0] == INVALID
    assert _create(round_mode=2)[0] == INVALID and _create(round_mode=-1)[0] == INVALID
    _admitted(round_mode=capi.ROUND_DOWN)
    assert _create(nscales=0)[0] == INVALID
    assert _create(nscales=3)[0] == INVALID
    _admitted(nscales=32)
    assert _create(force_path=2)[0] == INVALID
    assert _create(force_path=-2)[0] == INVALID
    # fewer than 2^31 pixels on either side: the last admitted and the first refused count, src and dst on their own
    one = dict(ic=1, kh=1, kw=1, dh=1, dw=1, pad_t=0, pad_l=0)
    _admitted(**one, bs=(1 << 31) - 1, ih=1, iw=1, oh=1, ow=1)
    assert _create(**one, bs=1 << 11, ih=1 << 10, iw=1 << 10, oh=1, ow=1)[0] == INVALID           # src: exactly 2^31
    rc, msg = _create(bs=1 << 30, ih=1, iw=1, oh=2, ow=1)                                          # dst: exactly 2^31 (src 2^30)
    assert rc == INVALID and "pixel count" in msg, (rc, msg)
    _admitted(bs=(1 << 30) - 1, ih=1, iw=1, oh=2, ow=1)
    # force_path = MFMA outside its class: every clause of the class
    for kw in (dict(ic=16), dict(ic=48), dict(ic=1), dict(oc=16), dict(oc=48), dict(oc=7),                       # channels
               dict(sh=2, sw=2, oh=5, ow=5), dict(sh=2, sw=1, oh=5), dict(sh=1, sw=2, ow=5),                     # stride
               dict(kh=1, kw=1, pad_t=0, pad_l=0), dict(kh=5, kw=5), dict(kh=3, kw=1, pad_l=0), dict(kh=2, kw=3),  # window
               dict(bs=1, ic=1024, ih=1 << 11, iw=1 << 10, oh=1, ow=1),                                          # a source image of 2^31 bytes
               dict(bs=1, ih=1 << 13, iw=1 << 13, oh=1 << 13, ow=1 << 13),                                       # a dst image of 2^31 bytes
               dict(bs=1, ih=1 << 12, iw=1 << 12, oh=1 << 12, ow=1 << 12, dst_dt=capi.DFX_S32)):
        rc, msg = _create(force_path=capi.DILCONV_MFMA, **kw)
        assert rc == UNSUPPORTED and "MFMA kernel's class" in msg, (kw, rc, msg)
        _admitted(**kw)                                                  # on auto the op is total
    for kw in (dict(), dict(dh=1, dw=1, pad_t=1, pad_l=1), dict(dh=18, dw=18, pad_t=18, pad_l=18), dict(dh=3, dw=1, pad_t=1, pad_l=0),
               dict(dh=255, dw=255, pad_t=510, pad_l=0), dict(pad_t=0, pad_l=0, oh=5, ow=6), dict(oh=1, ow=1), dict(oh=11, ow=12),
               dict(oc=160), dict(oc=1024), dict(ic=96), dict(ic=320, oc=256), dict(ic=2048, oc=256), dict(ic=7200),
               dict(bs=1, ic=1024, ih=(1 << 11) - 1, iw=1 << 10, oh=1, ow=1),
               dict(bs=1, ih=(1 << 13) - 1, iw=1 << 13, oh=(1 << 13) - 1, ow=1 << 13)):
        _admitted(force_path=capi.DILCONV_MFMA, **kw)                    # every admitted value of each clause: NO cap on ic
    # null arguments
    L = capi.lib()
    assert L.dfx_dilconv_create(None, ctypes.byref(ctypes.c_void_p())) == INVALID
    assert L.dfx_dilconv_create(ctypes.byref(capi.DilConvDesc()), None) == INVALID
    assert L.dfx_dilconv_submit(None, None, None, None) == INVALID
    assert L.dfx_dilconv_submit_host(None, None, None) == INVALID
    assert L.dfx_dilconv_set_weights(None, None, None, None) == INVALID
    assert L.dfx_dilconv_query(None, None) == INVALID
    assert L.dfx_debug_dilconv_requant(None, None) == INVALID
    assert L.dfx_dilconv_destroy(None) == 0
    # a bad descriptor is refused through the Python class as well
    with pytest.raises(dfa.DfxError) as e:
        dfa.DilatedConv((1, 4, 4, 32), 32, (3, 3), dilation=(2, 2), pad=(2, 2), nscales=5)
    assert "dfx error 1" in str(e.value)
    with pytest.raises(dfa.DfxError) as e:
        dfa.DilatedConv((1, 4, 4, 32), 32, (3, 3), dilation=(2, 2), pad=(5, 2))
    assert "dfx error 1" in str(e.value)


VALID = [
    dict(), dict(dh=1, dw=1, pad_t=1, pad_l=1), dict(dh=18, dw=18, pad_t=18, pad_l=18),    # MFMA class
    dict(oh=8, ow=7, relu=1, round_mode=capi.ROUND_DOWN),                                  # cropped
    dict(oc=128, dst_dt=capi.DFX_S32, bia_dt=capi.DFX_F32, nscales=128),
    dict(ic=2048, oc=256),
    dict(force_path=capi.DILCONV_MFMA),
    dict(force_path=capi.DILCONV_GENERIC),
    dict(ic=1), dict(ic=3), dict(oc=7, nscales=7), dict(kh=5, kw=5, pad_t=4, pad_l=4, oh=5, ow=6),   # outside it: the generic path
    dict(sh=2, sw=2, oh=5, ow=5), dict(kh=1, kw=3, pad_t=0),
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
            dfa.DilatedConv((1, 4, 4, 32), 32, (3, 3), dilation=(2, 2), pad=(2, 2))
        assert "dfx error 4" in str(e.value) and "no HIP device" in str(e.value)


def test_dilconv_structs_match_the_header(tmp_path):
    """dfx_dilconv_desc / dfx_dilconv_info compiled by gcc have the sizes and field offsets of the ctypes mirrors"""
    pairs = {"dfx_dilconv_desc": capi.DilConvDesc, "dfx_dilconv_info": capi.DilConvInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dfx.h"', 'int main(void) {']
    for cname, ct in pairs.items():
        lines.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in ct._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines.append('printf("path mfma %d\\n", DFX_DILCONV_MFMA); printf("path generic %d\\n", DFX_DILCONV_GENERIC);')
    lines.append('printf("dfx_conv_desc size %zu\\n", sizeof(dfx_conv_desc));')
    lines.append('printf("dfx_gconv_desc size %zu\\n", sizeof(dfx_gconv_desc));')
    lines.append('printf("dfx_deconv_desc size %zu\\n", sizeof(dfx_deconv_desc));')
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
    assert seen[("path", "mfma")] == capi.DILCONV_MFMA == R.MFMA and seen[("path", "generic")] == capi.DILCONV_GENERIC == R.GENERIC
    assert capi.DILCONV_AUTO == -1
    # dfx_deconv_desc with the dilation after the stride
    names = [n for n, _ in capi.DeconvDesc._fields_]
    at = names.index("sw") + 1
    assert [n for n, _ in capi.DilConvDesc._fields_] == names[:at] + ["dh", "dw"] + names[at:]
    assert [n for n, _ in capi.DilConvInfo._fields_] == [n for n, _ in capi.DeconvInfo._fields_]
    # the other descriptors are untouched
    assert ctypes.sizeof(capi.ConvDesc) == 100 == seen[("dfx_conv_desc", "size")]
    assert ctypes.sizeof(capi.GConvDesc) == 80 == seen[("dfx_gconv_desc", "size")]
    assert ctypes.sizeof(capi.DeconvDesc) == 76 == seen[("dfx_deconv_desc", "size")]
    assert ctypes.sizeof(capi.DilConvDesc) == 84


def test_library_exports_the_dilconv_entry_points():
    L = capi.lib()
    for s in ("dfx_dilconv_create", "dfx_dilconv_set_weights", "dfx_dilconv_submit", "dfx_dilconv_submit_host",
              "dfx_dilconv_query", "dfx_dilconv_destroy", "dfx_debug_dilconv_requant"):
        assert s in dfa.declared_symbols() and hasattr(L, s), s
    assert not [s for s in dfa.declared_symbols() if not hasattr(L, s)]
    for name in ("DilatedConv", "DilConvDesc", "DilConvInfo", "DILCONV_AUTO", "DILCONV_MFMA", "DILCONV_GENERIC", "dilconv_out_hw"):
        assert hasattr(dfa, name), name
    assert dfa.dilconv_out_hw(33, 33, (3, 3), (1, 1), (12, 12), (12, 12)) == (33, 33)
    assert dfa.dilconv_out_hw(15, 14, (5, 5), (2, 2), (3, 3), (6, 6)) == (8, 7)
    # the two tuning keys are known to the library (an unknown key is refused)
    for key in ("DFX_DILCONV_GRID", "DFX_DILCONV_SLAB"):
        capi.set_tuning(key, "1")
        capi.set_tuning(key, None)


def test_dropin_layer_exports_dilated_conv_and_tools_are_built():
    so = os.path.join(PKG, "libdeepfusion.so")
    assert os.path.exists(so), "run __graft_entry__.build() first"
    syms = subprocess.check_output(["nm", "-D", "-C", "--defined-only", so]).decode()
    assert "deepfusion::dilated_conv(" in syms
    for tool in ("dilconv_check", "dilconv_pack_check", "bench_dilconv"):
        exe = os.path.join(PKG, "tools", tool)
        assert os.path.exists(exe) and os.access(exe, os.X_OK), tool


def test_dilconv_pack_check_is_clean_under_the_host_sanitizers(tmp_path):
    """tools/dilconv_pack_check.cc, a stand-alone host program over csrc/dilconv_pack.h, built with ASan + UBSan: for
    every (ic, oc, slab) of its table -- ic 96 at 2 K-steps per slab and oc 160 among them -- the (chunk, slab) pieces
    tile the image, unpacking them in the kernel's reading order reproduces the weights, no byte of the image is left
    unwritten and none outside it is touched.  Nothing here is loaded into Python."""
    src = os.path.join(PKG, "tools", "dilconv_pack_check.cc")
    assert os.path.exists(src), "tools/dilconv_pack_check.cc is missing"
    probe = tmp_path / "probe.cc"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++"] + flags + [str(probe), "-o", str(tmp_path / "probe")], stdout=subprocess.DEVNULL,
                      stderr=subprocess.DEVNULL).returncode != 0:
        pytest.skip("this compiler has no sanitizer runtime")
    exe = tmp_path / "dilconv_pack_check"
    subprocess.check_call(["g++"] + flags + [src, "-o", str(exe)])
    p = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    assert "all 11 cases unpacked to the weights they were packed from" in out, out
    assert "ic   96 oc  32 slab 2:" in out and "in 1 chunks x 2 slabs" in out, out       # an uneven last slab
    assert "ic   96 oc 160 slab 2:" in out and "ic   32 oc 160 slab 1:" in out and "in 2 chunks" in out, out   # chunks of 4 + 1
    assert "ic 2048 oc  32 slab 3:" in out, out


def test_tables_cover_what_they_claim():
    m, g = R.mfma_table(), R.generic_table()
    assert all(c.mfma_class for c in m) and not any(c.mfma_class for c in g)
    assert len(m) == len(R.MFMA_GEOMS) * len(R.OPTIONS) and sum(len(R.mfma_table(n[0])) for n in R.MFMA_GEOMS) == len(m)
    by = {n[0]: R.mfma_case(n[0]) for n in R.MFMA_GEOMS}
    px = lambda c: c.bs * c.oh * c.ow                                                      # noqa: E731
    assert (by["base"].bs, by["base"].ih, by["base"].iw, by["base"].c, by["base"].oc, by["base"].dil, by["base"].pad) == (1, 8, 8, 32, 32, (2, 2), (2, 2))
    assert px(by["base"]) == 64
    assert px(by["rows-d1"]) == px(by["rows-d2"]) == 70 and by["rows-d1"].dil == (1, 1) and by["rows-d2"].dil == (2, 2)   # ragged: 70 = 2 * 32 + 6
    far = by["far-d18"]                                                                    # only the centre tap is ever inside
    assert far.dil == (18, 18) and far.pad == (18, 18) and far.ih <= 18 and far.iw <= 18 and px(far) == 70
    assert {(c.dil, c.pad) for c in m if c.name.startswith("aniso")} == {((3, 1), (1, 0)), ((3, 1), (0, 0)), ((2, 5), (1, 0)), ((2, 5), (0, 0))}
    assert (by["aniso31-p00"].oh, by["aniso31-p00"].ow) == (5, 7) and (by["aniso31-p10"].oh, by["aniso31-p10"].ow) == (7, 7)
    assert by["aniso25-p10"].out_hw == (8, 4) and by["aniso25-p00"].out_hw == (6, 3)       # cropped rows; a window wider than the image
    assert by["aniso25-p00"].ext == (5, 11) and by["aniso25-p00"].iw == 9
    assert by["slabs"].c == 96 and by["slabs-oc160"].c == 96 and by["slabs-oc160"].oc == 160
    assert by["chunks"].oc == 160 and by["chunks"].c == 32
    assert by["strips"].oc == 160 and px(by["strips"]) == 312 and -(-312 // 32) == 10 > R.WAVES and 312 % 32
    # the slab plans the GPU tests reach through DFX_DILCONV_SLAB: one K-step per slab (two buffers), an uneven last slab
    # with two buffers (one block) and with one (a chunk of four), all K-steps in one slab
    assert R.lds_plan(96, 32, 1)[:2] == (1, 2) and R.lds_plan(96, 32, 2)[:2] == (2, 2) and R.lds_plan(96, 32, 8)[:2] == (3, 1)
    assert R.lds_plan(96, 160, 1)[:2] == (1, 2) and R.lds_plan(96, 160, 2)[:2] == (2, 1) and R.lds_plan(96, 160, 8)[:2] == (3, 1)
    assert R.lds_plan(32, 32)[:2] == (1, 1)
    assert all(R.lds_plan(c, 256, s)[2] <= R.LDS_LIMIT for c in (32, 96, 2048, 7200) for s in (None, 1, 2, 3, 8, 1000))
    assert R.lds_plan(320, 256) == R.lds_plan(2048, 256) == R.lds_plan(7200, 256)          # the plan does not depend on ic
    for t in (m, g):
        assert {c.dst_dt for c in t} == {C.U8, C.S8, C.S32, C.F32}
        assert {c.bia_dt for c in t} == {C.UNDEF, C.F32, C.S32, C.S8, C.U8}
        assert {c.per_channel for c in t} == {True, False} and {c.rm for c in t} == {0, 1} and {c.relu for c in t} == {True, False}
        assert any(c.wide for c in t)
    for n in R.MFMA_GEOMS:                                                                 # every geometry under every option
        t = R.mfma_table(n[0])
        assert {c.dst_dt for c in t} == {C.U8, C.S8, C.S32, C.F32} and {c.rm for c in t} == {0, 1}
        assert {c.bia_dt == C.UNDEF for c in t} == {True, False} and {c.relu for c in t} == {True, False}
    assert ((5, 5), (2, 2), (3, 3)) in {(c.k, c.stride, c.dil) for c in g}
    assert {(c.c, c.oc) for c in g} >= {(ic, oc) for ic in (3, 20) for oc in (5, 48)}
    assert any(c.k == (3, 3) and c.stride == (1, 1) and c.c % 32 for c in g) and any(c.k == (3, 3) and c.stride == (2, 2) and c.c % 32 == 0 for c in g)
    assert all(c.stuffed_expressible for c in R.all_tables())
    assert any(c.dense_expressible for c in m) and any(not c.dense_expressible for c in m)
    assert len({c.ident() for c in R.all_tables()}) == len(R.all_tables())
    for c in R.all_tables():                                                               # what dfx_dilconv_create validates
        assert 0 <= c.pad[0] <= (c.k[0] - 1) * c.dil[0] and 0 <= c.pad[1] <= (c.k[1] - 1) * c.dil[1]
        assert c.oh >= 1 and c.ow >= 1 and (c.oh - 1) * c.stride[0] - c.pad[0] <= c.ih - 1 and (c.ow - 1) * c.stride[1] - c.pad[1] <= c.iw - 1


@pytest.mark.parametrize("impl", ["scalar_mt", "avx512"])
def test_reference_equals_the_oracles_dense_conv_on_the_stuffed_weights(oracle, impl):
    """defining property 2 on the reference: every table case with ic and oc multiples of 16 and the derived output
    size, against the C oracle's dense conv with the zero-stuffed ((k-1)d+1)^2 window: this pins the reference of the GPU
    tests"""
    if impl == "avx512" and not oracle.have_avx512_vnni():
        impl = "scalar"       # the oracle's other implementation on a host without AVX-512 VNNI
    n, seen = 0, set()
    for case in R.all_tables():
        if not case.dense_expressible:
            continue
        data = R.generate(case)
        want = hipref.oracle_conv(oracle, R.dense_case(case), R.dense_data(case, data), impl=impl)
        hipref.assert_bit_equal(R.dilconv_ref(case, data), want, "%s vs oracle %s" % (case.ident(), impl))
        n += 1
        seen.add(case.dil)
    assert n >= 60 and seen >= {(1, 1), (2, 2), (18, 18), (3, 1), (2, 1), (3, 3)}, (n, seen)


def _gcase(case, k):
    return G.GCase(case.name, case.bs, case.c, case.ih, case.iw, case.oc, 1, k=k, stride=case.stride, pad=case.pad,
                   out_hw=(case.oh, case.ow), dst_dt=case.dst_dt, bia_dt=case.bia_dt, relu=case.relu, rm=case.rm,
                   per_channel=case.per_channel, wide=case.wide, seed=case.seed)


def test_reference_equals_the_grouped_reference_on_the_stuffed_weights():
    """defining property 1 on the reference, for every table case (anisotropic dilation, cropped outputs, windows that
    hang over, strides, channel counts that are no multiple of 16 included), and property 3 where dh = dw = 1"""
    n1 = 0
    for case in R.all_tables():
        data = R.generate(case)
        ref = R.dilconv_ref(case, data)
        hipref.assert_bit_equal(ref, G.gconv_ref(_gcase(case, case.ext), dict(data, w=R.stuff_weights(data["w"], case.dil))), case.ident())
        if case.dil == (1, 1):
            hipref.assert_bit_equal(ref, G.gconv_ref(_gcase(case, case.k), data), case.ident())
            n1 += 1
    assert n1 >= len(R.OPTIONS)


def test_hand_written_values():
    """one channel, a 5x5 image of distinct values, d 2: the centre output sums the nine pixels at even coordinates; a
    corner output reaches four taps; and at d 18 pad 18 on a 7x5 image an output pixel is the centre tap alone"""
    src = np.arange(1, 26, dtype=np.uint8).reshape(1, 5, 5, 1)
    w = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9], dtype=np.int8).reshape(1, 1, 3, 3)
    acc = R.dilconv_acc(src, w, (1, 1), (2, 2), (2, 2), (5, 5))[0, :, :, 0]
    img = src[0, :, :, 0].astype(np.int64)
    assert acc[2, 2] == sum(int(w[0, 0, ky, kx]) * int(img[2 * ky, 2 * kx]) for ky in range(3) for kx in range(3)) == 1 * 1 + 2 * 3 + 3 * 5 + 4 * 11 + 5 * 13 + 6 * 15 + 7 * 21 + 8 * 23 + 9 * 25
    assert acc[0, 0] == 5 * 1 + 6 * 3 + 8 * 11 + 9 * 13                       # taps (1,1), (1,2), (2,1), (2,2)
    assert acc[4, 1] == 2 * 12 + 3 * 14 + 5 * 22 + 6 * 24                     # rows 2 and 4 (ky 0, 1), columns 1 and 3 (kx 1, 2)
    # pad 0: the output shrinks to one pixel
    assert R.dilconv_acc(src, w, (1, 1), (2, 2), (0, 0), (1, 1))[0, 0, 0, 0] == acc[2, 2]
    # only the centre tap reaches: d 18 on 7x5
    case = R.mfma_case("far-d18", 2)                                          # s32, no bias, scale alone
    data = R.generate(case)
    acc = R.dilconv_acc(data["src"], data["w"], case.stride, case.dil, case.pad, (case.oh, case.ow))
    centre = np.einsum('nyxi,oi->nyxo', data["src"].astype(np.int64), data["w"][:, :, 1, 1].astype(np.int64))
    assert np.array_equal(acc, centre)
    # two input channels, two output channels, dh != dw, by hand
    src2 = np.zeros((1, 4, 3, 2), dtype=np.uint8)
    src2[0, 0, 0] = (2, 3)
    src2[0, 3, 2] = (5, 7)
    w2 = np.zeros((2, 2, 2, 2), dtype=np.int8)
    w2[0, :, 0, 0] = (1, 10)
    w2[0, :, 1, 1] = (2, 20)
    w2[1, :, 1, 1] = (-1, -3)
    acc = R.dilconv_acc(src2, w2, (1, 1), (3, 2), (0, 0), (1, 1))               # taps (0,0) at (0,0) and (1,1) at (3,2)
    assert acc[0, 0, 0].tolist() == [2 * 1 + 3 * 10 + 5 * 2 + 7 * 20, -5 - 21]
    # the formula of include/dfx.h on a few pixels of a generic table case (5x5, stride 2, d 3)
    case = [c for c in R.generic_table() if c.k == (5, 5) and c.c == 3 and c.oc == 5][0]
    data = R.generate(case)
    acc = R.dilconv_acc(data["src"], data["w"], case.stride, case.dil, case.pad, (case.oh, case.ow))
    for n, oy, ox, o in ((0, 0, 0, 0), (1, 7, 6, 4), (0, 4, 3, 2), (1, 5, 0, 3)):
        want = 0
        for ky in range(5):
            for kx in range(5):
                y, x = oy * 2 - case.pad[0] + ky * 3, ox * 2 - case.pad[1] + kx * 3
                if 0 <= y < case.ih and 0 <= x < case.iw:
                    want += int(np.dot(data["src"][n, y, x].astype(np.int64), data["w"][o, :, ky, kx].astype(np.int64)))
        assert int(acc[n, oy, ox, o]) == want, (n, oy, ox, o)


def test_rows_of_the_reference_are_the_rows_of_the_whole():
    case = R.DlCase("rows", 2, 32, 9, 7, 32, dil=(3, 2), pad=(3, 2), seed=45000, **R.OPTIONS[0])
    data = R.generate(case)
    whole = R.dilconv_ref(case, data)
    hipref.assert_bit_equal(R.dilconv_ref(case, data, rows=(0, 4, 8)), np.ascontiguousarray(whole[:, [0, 4, 8]]), "rows")


@pytest.mark.parametrize("geom", [g[0] for g in R.MFMA_GEOMS])
def test_permutation_case_has_distinct_weights(geom):
    """at every (i, ky, kx) the output channels of a 32-block are distinct; within an output channel any 255 taps that
    are consecutive in (i, ky, kx) order are distinct, so the nine taps of one input channel, the 16 channel bytes a
    lane loads and the taps on either side of a K-step or slab boundary are"""
    case, data = R.permutation_case(geom)
    assert case.mfma_class
    w = data["w"].reshape(case.oc, -1).astype(np.int64)
    taps = w.shape[1]
    for b in range(case.oc // 32):
        assert all(len(set(col.tolist())) == 32 for col in w[32 * b:32 * b + 32].T)
    for row in w[::7]:
        assert all(len(set(row[t:t + 255].tolist())) == min(255, taps - t) for t in range(0, taps, 64))
    assert len(np.unique(data["src"])) > 200
    assert R.dilconv_ref(case, data).dtype == np.int32


def test_wide_cases_reach_both_ends_of_the_range():
    """a "wide" 1-byte case's expected output holds both ends of what its dtype and ReLU flag can reach"""
    n = 0
    for case in R.all_tables():
        if not case.wide or case.dst_dt not in (C.U8, C.S8) or case.bs * case.oh * case.ow * case.oc < 2000:
            continue
        ref = R.dilconv_ref(case, R.generate(case))
        lo = 0 if (case.relu or case.dst_dt == C.U8) else -128
        hi = 255 if case.dst_dt == C.U8 else 127
        assert ref.min() == lo and ref.max() == hi, (case.ident(), ref.min(), ref.max())
        n += 1
    assert n >= 8


@pytest.mark.parametrize("edge", R.EDGES, ids=lambda e: e.name)
def test_edge_data_attains_the_bound_the_proof_uses(edge):
    """(255 * max(P, N) + |bias|) * scale is exactly 2^30 at the last admitted value, one scale step beyond at the first
    rejected one; the prescribed weights sit on nine (tap, input channel) positions, one per tap and on both K-steps,
    every other weight of the channel is zero, and EDGE_PIXEL's accumulator is exactly 255 P / -255 N"""
    case, data = R.edge_case(edge, C.S32)
    assert case.mfma_class and case.c == 64
    w = data["w"][R.EDGE_CHANNEL]
    assert len(set(R.EDGE_POSITIONS)) == 9 and [(ky, kx) for ky, kx, i in R.EDGE_POSITIONS] == [(a, b) for a in range(3) for b in range(3)]
    assert {i // 32 for ky, kx, i in R.EDGE_POSITIONS} == {0, 1}
    assert tuple(int(w[i, ky, kx]) for ky, kx, i in R.EDGE_POSITIONS) == edge.weights
    rest = w.copy()
    for ky, kx, i in R.EDGE_POSITIONS:
        rest[i, ky, kx] = 0
    assert not rest.any()
    acc, bound, P, N = R.edge_attained(edge, case, data)
    assert acc == bound and abs(bound) == 255 * max(P, N)
    reach = (255 * max(P, N) + abs(edge.bias)) * edge.scale
    assert reach == (R.LIMIT if edge.fast else R.LIMIT + edge.scale)
    ref = R.dilconv_ref(case, data)
    img = 0 if edge.which == "max" else 1
    sign = 1 if edge.which == "max" else -1
    assert int(ref[img, R.EDGE_PIXEL[0], R.EDGE_PIXEL[1], R.EDGE_CHANNEL]) == sign * int(reach)
