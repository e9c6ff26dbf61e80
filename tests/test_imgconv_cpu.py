"""CPU-only checks of the first-layer conv op: the C ABI validates descriptors before it touches a device, the ctypes
mirrors match the header, the symbols are exported, the drop-in layer and its tools are built, the weight packer is
clean under the host sanitizers, the numpy reference the GPU tests compare against equals the C oracle's dense conv on
the image zero-padded to 16 channels and the grouped conv's reference with groups = 1, and the test data keeps the
promises the GPU tests rely on."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

import cases as C
import gconv_ref as G
import hipref
import imgconv_ref as R

dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-fusion_amd")
INVALID, UNSUPPORTED, NO_DEVICE = 1, 2, 4


def _create(**kw):
    d = dict(bs=2, ic=3, ih=9, iw=11, oc=32, oh=9, ow=11, kh=3, kw=3, sh=1, sw=1, pad_t=1, pad_l=1,
             dst_dt=capi.DFX_U8, bia_dt=capi.DFX_UNDEF, relu=0, round_mode=capi.ROUND_NEAREST, nscales=1,
             force_path=capi.IMGCONV_AUTO)
    d.update(kw)
    desc = capi.ImgConvDesc(**d)
    h = ctypes.c_void_p()
    rc = capi.lib().dfx_imgconv_create(ctypes.byref(desc), ctypes.byref(h))
    msg = capi.lib().dfx_last_error().decode()
    if rc == 0:
        assert capi.lib().dfx_imgconv_destroy(h) == 0
    else:
        assert not h.value
    return rc, msg


def _admitted(**kw):
    """a valid descriptor gets past validation: it creates with a device and fails with NO_DEVICE without one"""
    rc, msg = _create(**kw)
    assert rc in (0, NO_DEVICE), (kw, rc, msg)


K7 = dict(kh=7, kw=7, sh=2, sw=2, pad_t=3, pad_l=3, oh=5, ow=6)         # (9 + 6 - 7) // 2 + 1, (11 + 6 - 7) // 2 + 1
K3S2 = dict(sh=2, sw=2, oh=5, ow=6)


def test_descriptor_validation_needs_no_device():
    for bad in ("bs", "ic", "ih", "iw", "oc", "oh", "ow", "kh", "kw", "sh", "sw"):
        assert _create(**{bad: 0})[0] == INVALID, bad
        assert _create(**{bad: -3})[0] == INVALID, bad
    assert _create(pad_t=-1)[0] == INVALID and _create(pad_l=-1)[0] == INVALID
    _admitted(pad_t=0, pad_l=0, oh=7, ow=9)
    # 1 <= ic <= 4: every admitted value and the first rejected one
    for ic in (1, 2, 3, 4):
        _admitted(ic=ic)
    rc, msg = _create(ic=5)
    assert rc == INVALID and "beyond 4" in msg, (rc, msg)
    assert _create(ic=16)[0] == INVALID
    # any oc >= 1
    for oc in (1, 7, 33, 1000):
        _admitted(oc=oc)
    # windows 1 .. 255; kh * kw * ic <= 65025 = 255^2: the last admitted and the first rejected value
    _admitted(kh=1, kw=1, pad_t=0, pad_l=0)
    _admitted(ic=1, kh=255, kw=255, pad_t=127, pad_l=127)                                # 255 * 255 * 1 = 65025
    assert _create(ic=1, kh=255, kw=256, pad_t=127, pad_l=127)[0] == INVALID             # the window
    assert _create(ic=1, kh=256, kw=1, pad_t=127, pad_l=0)[0] == INVALID
    rc, msg = _create(ic=2, kh=255, kw=255, pad_t=127, pad_l=127)                        # the accumulator
    assert rc == INVALID and "65025" in msg, (rc, msg)
    _admitted(ic=3, kh=85, kw=255, pad_t=42, pad_l=127)                                  # 85 * 255 * 3 = 65025
    assert _create(ic=3, kh=86, kw=255, pad_t=42, pad_l=127)[0] == INVALID
    _admitted(ic=4, kh=127, kw=128, pad_t=63, pad_l=63)                                  # 65024
    assert _create(ic=4, kh=128, kw=128, pad_t=63, pad_l=63)[0] == INVALID               # 65536
    # (oh - 1) * sh - pad_t <= ih - 1, likewise in x: the last admitted and the first rejected output size
    _admitted(oh=10, ow=12)                                             # 9 * 1 - 1 = 8
    assert _create(oh=11)[0] == INVALID                                 # 10 * 1 - 1 = 9 > 8
    assert _create(ow=13)[0] == INVALID
    _admitted(sh=2, sw=2, pad_t=0, pad_l=0, oh=5, ow=6)                 # 4 * 2 = 8
    assert _create(sh=2, sw=2, pad_t=0, pad_l=0, oh=6, ow=6)[0] == INVALID      # 5 * 2 = 10 > 8
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
    assert _create(nscales=3)[0] == INVALID                             # (the channel count of src is no scale count)
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
    # force_path = MFMA outside its class: every clause of the class
    for kw in (dict(ic=1), dict(ic=2),                                                                    # ic
               dict(kh=5, kw=5, pad_t=2, pad_l=2), dict(kh=1, kw=1, pad_t=0, pad_l=0), dict(kh=3, kw=1, pad_l=0),
               dict(kh=7, kw=3, pad_t=3), dict(kh=11, kw=11, sh=4, sw=4, pad_t=2, pad_l=2, oh=1, ow=2),   # window
               dict(sh=1, sw=2, ow=6), dict(sh=3, sw=3, oh=3, ow=4),                                      # stride
               dict(kh=7, kw=7, pad_t=3, pad_l=3), dict(kh=7, kw=7, sh=1, sw=2, pad_t=3, pad_l=3, ow=6),  # 7x7 at stride 1
               dict(pad_t=3, oh=11), dict(pad_l=3, ow=13), dict(K7, pad_t=7, oh=7), dict(K7, pad_l=7, ow=8),      # pad > k - 1
               dict(oc=16), dict(oc=48), dict(oc=7), dict(oc=160), dict(oc=256),                          # oc
               dict(bs=1, ic=4, ih=1 << 15, iw=1 << 14, oh=1, ow=1),                                       # a source image of 2^31 bytes
               dict(bs=1, ih=1, iw=1 << 24, oh=1, ow=1 << 24, oc=128),                                     # a dst image
               dict(bs=1, ih=1, iw=1 << 24, oh=1, ow=1 << 24, dst_dt=capi.DFX_S32)):
        rc, msg = _create(force_path=capi.IMGCONV_MFMA, **kw)
        assert rc == UNSUPPORTED and "MFMA kernel's class" in msg, (kw, rc, msg)
        _admitted(**kw)                                                  # on auto the op is total
    # one image below 2^31 bytes on either side: exactly 2^31 is outside the class, the largest size below it inside
    big = dict(bs=1, ih=1, oh=1)
    for out, ok in ((dict(ic=4, iw=1 << 29, ow=1), dict(ic=4, iw=(1 << 29) - 1, ow=1)),
                    (dict(iw=1 << 26, ow=1 << 26), dict(iw=1 << 26, ow=(1 << 26) - 1)),                     # u8 dst, oc 32
                    (dict(iw=1 << 24, ow=1 << 24, dst_dt=capi.DFX_F32), dict(iw=1 << 24, ow=(1 << 24) - 1, dst_dt=capi.DFX_F32))):
        rc, msg = _create(force_path=capi.IMGCONV_MFMA, **big, **out)
        assert rc == UNSUPPORTED and "2^31 bytes" in msg, (out, rc, msg)
        _admitted(**big, **out)
        _admitted(force_path=capi.IMGCONV_MFMA, **big, **ok)
    for kw in (dict(), dict(ic=4), K3S2, K7, dict(K7, ic=4), dict(oc=64), dict(oc=96), dict(oc=128),
               dict(pad_t=0, pad_l=0, oh=7, ow=9), dict(pad_t=2, pad_l=2, oh=11, ow=13), dict(K3S2, pad_t=0, pad_l=0, oh=4, ow=5),
               dict(K7, pad_t=6, pad_l=6, oh=8, ow=9), dict(K7, pad_t=0, pad_l=0, oh=2, ow=3)):
        _admitted(force_path=capi.IMGCONV_MFMA, **kw)                    # every admitted value of each clause
    # null arguments
    L = capi.lib()
    assert L.dfx_imgconv_create(None, ctypes.byref(ctypes.c_void_p())) == INVALID
    assert L.dfx_imgconv_create(ctypes.byref(capi.ImgConvDesc()), None) == INVALID
    assert L.dfx_imgconv_submit(None, None, None, None) == INVALID
    assert L.dfx_imgconv_submit_host(None, None, None) == INVALID
    assert L.dfx_imgconv_set_weights(None, None, None, None) == INVALID
    assert L.dfx_imgconv_query(None, None) == INVALID
    assert L.dfx_debug_imgconv_requant(None, None) == INVALID
    assert L.dfx_imgconv_destroy(None) == 0
    # a bad descriptor is refused through the Python class as well
    with pytest.raises(dfa.DfxError) as e:
        dfa.ImageConv((1, 4, 4, 3), 32, (3, 3), nscales=5)
    assert "dfx error 1" in str(e.value)
    with pytest.raises(dfa.DfxError) as e:
        dfa.ImageConv((1, 4, 4, 16), 32, (3, 3))
    assert "dfx error 1" in str(e.value)


VALID = [
    dict(), dict(ic=4), K7, K3S2,                                                           # MFMA class
    dict(K3S2, pad_t=0, pad_l=0, relu=1, round_mode=capi.ROUND_DOWN),                       # windows hang over
    dict(oc=128, dst_dt=capi.DFX_S32, bia_dt=capi.DFX_F32, nscales=128),
    dict(force_path=capi.IMGCONV_MFMA),
    dict(force_path=capi.IMGCONV_GENERIC),
    dict(ic=1), dict(ic=2), dict(oc=7, nscales=7), dict(kh=5, kw=5, pad_t=2, pad_l=2),      # outside it: the generic path
    dict(kh=11, kw=11, sh=4, sw=4, pad_t=2, pad_l=2, oh=1, ow=2), dict(kh=1, kw=3, pad_t=0), dict(sh=1, sw=2, ow=6),
    dict(pad_t=5, pad_l=4, oh=14, ow=15),                                                   # windows entirely in the padding
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
            dfa.ImageConv((1, 4, 4, 3), 32, (3, 3))
        assert "dfx error 4" in str(e.value) and "no HIP device" in str(e.value)


def test_imgconv_structs_match_the_header(tmp_path):
    """dfx_imgconv_desc / dfx_imgconv_info compiled by gcc have the sizes and field offsets of the ctypes mirrors"""
    pairs = {"dfx_imgconv_desc": capi.ImgConvDesc, "dfx_imgconv_info": capi.ImgConvInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dfx.h"', 'int main(void) {']
    for cname, ct in pairs.items():
        lines.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in ct._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines.append('printf("path mfma %d\\n", DFX_IMGCONV_MFMA); printf("path generic %d\\n", DFX_IMGCONV_GENERIC);')
    lines.append('printf("dfx_conv_desc size %zu\\n", sizeof(dfx_conv_desc));')
    lines.append('printf("dfx_gconv_desc size %zu\\n", sizeof(dfx_gconv_desc));')
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
    assert seen[("path", "mfma")] == capi.IMGCONV_MFMA == R.MFMA and seen[("path", "generic")] == capi.IMGCONV_GENERIC == R.GENERIC
    assert capi.IMGCONV_AUTO == -1
    # dfx_gconv_desc without `groups`
    assert [n for n, _ in capi.ImgConvDesc._fields_] == [n for n, _ in capi.GConvDesc._fields_ if n != "groups"]
    assert [n for n, _ in capi.ImgConvInfo._fields_] == [n for n, _ in capi.GConvInfo._fields_]
    assert ctypes.sizeof(capi.ImgConvInfo) == ctypes.sizeof(capi.GConvInfo)
    # the other descriptors are untouched
    assert ctypes.sizeof(capi.ConvDesc) == 100 == seen[("dfx_conv_desc", "size")]
    assert ctypes.sizeof(capi.GConvDesc) == 80 == seen[("dfx_gconv_desc", "size")]


def test_library_exports_the_imgconv_entry_points():
    L = capi.lib()
    for s in ("dfx_imgconv_create", "dfx_imgconv_set_weights", "dfx_imgconv_submit", "dfx_imgconv_submit_host",
              "dfx_imgconv_query", "dfx_imgconv_destroy", "dfx_debug_imgconv_requant"):
        assert s in dfa.declared_symbols() and hasattr(L, s), s
    assert not [s for s in dfa.declared_symbols() if not hasattr(L, s)]
    for name in ("ImageConv", "ImgConvDesc", "ImgConvInfo", "IMGCONV_AUTO", "IMGCONV_MFMA", "IMGCONV_GENERIC"):
        assert hasattr(dfa, name), name


def test_dropin_layer_exports_image_conv_and_tools_are_built():
    so = os.path.join(PKG, "libdeepfusion.so")
    assert os.path.exists(so), "run __graft_entry__.build() first"
    syms = subprocess.check_output(["nm", "-D", "-C", "--defined-only", so]).decode()
    assert "deepfusion::image_conv(" in syms
    for tool in ("imgconv_check", "imgconv_pack_check", "bench_imgconv"):
        exe = os.path.join(PKG, "tools", tool)
        assert os.path.exists(exe) and os.access(exe, os.X_OK), tool


def test_imgconv_pack_check_is_clean_under_the_host_sanitizers(tmp_path):
    """tools/imgconv_pack_check.cc, a stand-alone host program over csrc/imgconv_pack.h, built with ASan + UBSan: every
    (o, c, ky, kx) lands where the K layout says, every dead byte is zero, no byte outside the image is touched"""
    src = os.path.join(PKG, "tools", "imgconv_pack_check.cc")
    assert os.path.exists(src), "tools/imgconv_pack_check.cc is missing"
    probe = tmp_path / "probe.cc"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++"] + flags + [str(probe), "-o", str(tmp_path / "probe")], stdout=subprocess.DEVNULL,
                      stderr=subprocess.DEVNULL).returncode != 0:
        pytest.skip("this compiler has no sanitizer runtime")
    exe = tmp_path / "imgconv_pack_check"
    subprocess.check_call(["g++"] + flags + [src, "-o", str(exe)])
    p = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0, p.stdout.decode()
    assert b"all 16 shapes packed, every dead byte zero" in p.stdout, p.stdout.decode()


def test_tables_cover_what_they_claim():
    m, g = R.mfma_table(), R.generic_table()
    assert all(c.mfma_class for c in m) and not any(c.mfma_class for c in g)
    assert len(m) == 2 * 4 * 4 * 6 and sum(len(R.mfma_table(n)) for n, _, _, _ in R.MFMA_GEOMS) == len(m)
    assert {(c.k, c.stride, c.pad) for c in m} == {((7, 7), (2, 2), (3, 3)), ((3, 3), (1, 1), (1, 1)), ((3, 3), (2, 2), (1, 1)),
                                                   ((3, 3), (2, 2), (0, 0))}
    assert {c.bs for c in m} == {1, 3}
    per_geom = {}
    for c in m:
        per_geom.setdefault((c.k, c.stride, c.pad, c.ih, c.iw), set()).add((c.c, c.oc))
    assert len(per_geom) == 24 and all(v == {(ic, oc) for ic in (3, 4) for oc in R.MFMA_OC} for v in per_geom.values())
    assert {(c.ih, c.iw) for c in m} == {(5, 5), (9, 9), (17, 23), (33, 70), (2, 131), (10, 12)}
    assert any(c.ih < 7 and c.k == (7, 7) for c in m)                                   # smaller than the window
    assert any((c.iw * c.c) % 4 for c in m)                                             # odd row bytes
    assert any(c.ow > 32 and c.ow % 32 for c in m)                                      # a partial strip behind a whole one
    for c in m:                                                                         # windows that hang over
        if c.out_hw:
            assert (c.oh - 1) * c.stride[0] - c.pad[0] + c.k[0] > c.ih or (c.ow - 1) * c.stride[1] - c.pad[1] + c.k[1] > c.iw
    assert {(c.k, c.stride, c.pad) for c in m if c.out_hw and (c.ih, c.iw) == (10, 12)} == {(c.k, c.stride, c.pad) for c in m}
    for t in (m, g):
        assert {c.dst_dt for c in t} == {C.U8, C.S8, C.S32, C.F32}
        assert {c.bia_dt for c in t} == {C.UNDEF, C.F32, C.S32, C.S8, C.U8}
        assert {c.per_channel for c in t} == {True, False} and {c.rm for c in t} == {0, 1} and {c.relu for c in t} == {True, False}
        assert any(c.wide for c in t)
    assert {(c.c, c.k, c.stride, c.oc) for c in g} == {(ic, k, s, oc) for ic in (1, 2, 3) for oc in (7, 16, 48)
                                                       for k, s in (((5, 5), (1, 1)), ((11, 11), (4, 4)))}
    assert len({c.ident() for c in R.all_tables()}) == len(R.all_tables())


@pytest.mark.parametrize("impl", ["scalar_mt", "avx512"])
def test_reference_equals_the_oracles_dense_conv_on_the_padded_image(oracle, impl):
    """every table case with oc % 16 == 0 and the conv's output size, on the image zero-padded to 16 channels with
    zero weights on the channels >= ic: this pins the reference of the GPU tests"""
    if impl == "avx512" and not oracle.have_avx512_vnni():
        impl = "scalar"       # the oracle's other implementation on a host without AVX-512 VNNI
    tables = R.all_tables()
    n = 0
    for case in tables:
        if not case.dense_expressible:
            continue
        data = R.generate(case)
        want = hipref.oracle_conv(oracle, R.dense_case(case), R.dense_data(case, data), impl=impl)
        hipref.assert_bit_equal(R.imgconv_ref(case, data), want, "%s vs oracle %s" % (case.ident(), impl))
        n += 1
    assert n == len([c for c in tables if c.oc % 16 == 0 and c.out_hw is None]) > 150


def test_reference_equals_the_grouped_reference_with_one_group():
    for case in R.all_tables():
        data = R.generate(case)
        gcase = G.GCase(case.name, case.bs, case.c, case.ih, case.iw, case.oc, 1, k=case.k, stride=case.stride, pad=case.pad,
                        out_hw=(case.oh, case.ow), dst_dt=case.dst_dt, bia_dt=case.bia_dt, relu=case.relu, rm=case.rm,
                        per_channel=case.per_channel, wide=case.wide, seed=case.seed)
        hipref.assert_bit_equal(R.imgconv_ref(case, data), G.gconv_ref(gcase, data), case.ident())


def test_rows_of_the_reference_are_the_rows_of_the_whole():
    case = R.ICase("rows", 2, 3, 20, 17, 32, k=(7, 7), stride=(2, 2), pad=(3, 3), seed=25000, **R.OPTIONS[0])
    data = R.generate(case)
    whole = R.imgconv_ref(case, data)
    hipref.assert_bit_equal(R.imgconv_ref(case, data, rows=(0, 4, 9)), np.ascontiguousarray(whole[:, [0, 4, 9]]), "rows")


@pytest.mark.parametrize("k,stride", R.MFMA_WINDOWS)
@pytest.mark.parametrize("c", [3, 4])
def test_permutation_case_has_distinct_weights(k, stride, c):
    """within an output channel every (c, ky, kx) weight is distinct and at every (c, ky, kx) the output channels'
    weights are distinct; the reference agrees with a plain loop over (o, c, ky, kx) on a few pixels"""
    case, data = R.permutation_case(k, stride, c)
    w = data["w"].reshape(32, -1).astype(np.int64)
    assert all(len(set(row.tolist())) == w.shape[1] for row in w)
    assert all(len(set(col.tolist())) == 32 for col in w.T)
    ref = R.imgconv_ref(case, data)
    assert ref.dtype == np.int32
    src, w4 = data["src"].astype(np.int64), data["w"].astype(np.int64)
    for n, oy, ox, o in ((0, 0, 0, 0), (1, 2, 3, 17), (0, case.oh - 1, case.ow - 1, 31), (1, 1, case.ow - 1, 5)):
        acc = 0
        for ci in range(c):
            for ky in range(k[0]):
                for kx in range(k[1]):
                    y, x = oy * stride[0] - case.pad[0] + ky, ox * stride[1] - case.pad[1] + kx
                    if 0 <= y < case.ih and 0 <= x < case.iw:
                        acc += int(src[n, y, x, ci]) * int(w4[o, ci, ky, kx])
        assert int(ref[n, oy, ox, o]) == acc, (n, oy, ox, o)


def test_wide_cases_reach_both_ends_of_the_range():
    """a "wide" 1-byte case's expected output holds both ends of what its dtype and ReLU flag can reach"""
    n = 0
    for case in R.all_tables():
        if not case.wide or case.dst_dt not in (C.U8, C.S8) or case.bs * case.oh * case.ow < 8:
            continue
        ref = R.imgconv_ref(case, R.generate(case))
        lo = 0 if (case.relu or case.dst_dt == C.U8) else -128
        hi = 255 if case.dst_dt == C.U8 else 127
        assert ref.min() == lo and ref.max() == hi, (case.ident(), ref.min(), ref.max())
        n += 1
    assert n >= 8


def test_nan_and_inf_scales_and_biases_give_the_x86_results():
    """NaN -> 0x80000000 -> u8 255 / s8 -128; +inf * positive likewise (out of range), on the reference"""
    for dst_dt, bad in ((C.U8, 255), (C.S8, -128)):
        case = R.ICase("nan", 1, 3, 4, 4, 32, dst_dt=dst_dt, bia_dt=C.UNDEF, relu=False, per_channel=True)
        data = R.generate(case)
        data["scales"][3] = np.nan
        data["scales"][7] = np.inf
        data["src"][...] = np.maximum(data["src"], 1)
        data["w"][7] = np.abs(data["w"][7]) + 1
        ref = R.imgconv_ref(case, data)
        assert (ref[..., 3] == bad).all() and (ref[..., 7] == bad).all()
        case = R.ICase("nanbias", 1, 3, 4, 4, 32, dst_dt=dst_dt, bia_dt=C.F32, relu=False, per_channel=True)
        data = R.generate(case)
        data["bia"] = data["bia"].copy()
        data["bia"][5] = np.nan
        data["bia"][9] = np.inf
        ref = R.imgconv_ref(case, data)
        assert (ref[..., 5] == bad).all() and (ref[..., 9] == bad).all()


@pytest.mark.parametrize("edge", R.EDGES, ids=lambda e: e.name)
def test_edge_data_attains_the_bound_the_proof_uses(edge):
    """(255 * max(P, N) + |bias|) * scale is exactly 2^30 at the last admitted value, one scale step beyond at the first
    rejected one, the prescribed weights sit on the channel's first nine taps, and the centre pixel's accumulator is
    exactly 255 P / -255 N"""
    case, data = R.edge_case(edge, C.S32)
    assert case.mfma_class
    w = data["w"][R.EDGE_CHANNEL]
    assert tuple(w.flatten()[:9].tolist()) == edge.weights and not w.flatten()[9:].any()
    acc, bound, P, N = R.edge_attained(edge, case, data)
    assert acc == bound and abs(bound) == 255 * max(P, N)
    reach = (255 * max(P, N) + abs(edge.bias)) * edge.scale
    assert reach == (R.LIMIT if edge.fast else R.LIMIT + edge.scale)
    assert float(np.float32(edge.bias)) == edge.bias and float(np.float32(edge.scale)) == edge.scale     # exact in f32
    ref = R.imgconv_ref(case, data)
    img = 0 if edge.which == "max" else 1
    sign = 1 if edge.which == "max" else -1
    assert int(ref[img, 1, 1, R.EDGE_CHANNEL]) == sign * int(reach)            # the s32 result shows it: no saturation yet
