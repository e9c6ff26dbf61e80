"""CPU-only checks of the transposed conv op: the C ABI validates descriptors before it touches a device, the ctypes
mirrors match the header, the symbols are exported, the drop-in layer and its tools are built, the weight packer is
clean under the host sanitizers, the numpy reference the GPU tests compare against (a scatter) equals the C oracle's
dense conv on the zero-stuffed tensor with flipped weights and the grouped conv's reference with groups = 1, and the test
data keeps the promises the GPU tests rely on."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

import cases as C
import deconv_ref as R
import gconv_ref as G
import hipref

dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-fusion_amd")
INVALID, UNSUPPORTED, NO_DEVICE = 1, 2, 4


def _create(**kw):
    d = dict(bs=2, ic=32, ih=5, iw=6, oc=32, oh=10, ow=12, kh=2, kw=2, sh=2, sw=2, pad_t=0, pad_l=0,
             dst_dt=capi.DFX_U8, bia_dt=capi.DFX_UNDEF, relu=0, round_mode=capi.ROUND_NEAREST, nscales=1,
             force_path=capi.DECONV_AUTO)
    d.update(kw)
    desc = capi.DeconvDesc(**d)
    h = ctypes.c_void_p()
    rc = capi.lib().dfx_deconv_create(ctypes.byref(desc), ctypes.byref(h))
    msg = capi.lib().dfx_last_error().decode()
    if rc == 0:
        assert capi.lib().dfx_deconv_destroy(h) == 0
    else:
        assert not h.value
    return rc, msg


def _admitted(**kw):
    """a valid descriptor gets past validation: it creates with a device and fails with NO_DEVICE without one"""
    rc, msg = _create(**kw)
    assert rc in (0, NO_DEVICE), (kw, rc, msg)


K4 = dict(kh=4, kw=4, pad_t=1, pad_l=1)                  # (5 - 1) * 2 - 2 + 4 = 10, (6 - 1) * 2 - 2 + 4 = 12
K3 = dict(kh=3, kw=3, pad_t=1, pad_l=1)                  # output_padding 1: 10 x 12 = (in - 1) * 2 + 3 - 1, the limit


def test_descriptor_validation_needs_no_device():
    for bad in ("bs", "ic", "ih", "iw", "oc", "oh", "ow", "kh", "kw", "sh", "sw"):
        assert _create(**{bad: 0})[0] == INVALID, bad
        assert _create(**{bad: -3})[0] == INVALID, bad
    # any ic >= 1 and oc >= 1
    for c in (1, 3, 20, 33, 1000):
        _admitted(ic=c)
        _admitted(oc=c)
    # windows and strides 1 .. 255: the last admitted and the first refused value
    _admitted(kh=1, kw=1, sh=1, sw=1, oh=5, ow=6)
    _admitted(ic=1, kh=255, kw=255, oh=263, ow=265)                              # (in - 1) * 2 + 255
    assert _create(ic=1, kh=256, kw=1, oh=10, ow=11)[0] == INVALID
    assert _create(ic=1, kh=1, kw=256, oh=9, ow=12)[0] == INVALID
    _admitted(sh=255, sw=255, oh=1022, ow=1277)                                  # 4 * 255 + 2, 5 * 255 + 2
    rc, msg = _create(sh=256, oh=10)
    assert rc == INVALID and "stride" in msg, (rc, msg)
    assert _create(sw=256, ow=12)[0] == INVALID
    # 0 <= pad <= k - 1
    assert _create(pad_t=-1)[0] == INVALID and _create(pad_l=-1)[0] == INVALID
    _admitted(pad_t=1, pad_l=1, oh=9, ow=11)                                     # k - 1 = 1
    rc, msg = _create(pad_t=2, oh=8)
    assert rc == INVALID and "padding" in msg, (rc, msg)
    assert _create(pad_l=2, ow=10)[0] == INVALID
    _admitted(kh=4, kw=4, pad_t=3, pad_l=3, oh=9, ow=11)                         # (in - 1) * 2 + 4 - 3
    assert _create(kh=4, kw=4, pad_t=4, pad_l=3, oh=8, ow=11)[0] == INVALID
    assert _create(kh=4, kw=4, pad_t=3, pad_l=4, oh=9, ow=10)[0] == INVALID
    # kh * kw * ic <= 65025 = 255^2
    _admitted(ic=1, kh=255, kw=255, oh=1, ow=1)
    rc, msg = _create(ic=2, kh=255, kw=255, oh=1, ow=1)
    assert rc == INVALID and "65025" in msg, (rc, msg)
    _admitted(ic=16256, oh=1, ow=1)                                              # 4 * 16256 = 65024
    assert _create(ic=16257, oh=1, ow=1)[0] == INVALID                           # 65028
    _admitted(ic=255, kh=15, kw=17, oh=1, ow=1)                                  # 65025
    assert _create(ic=255, kh=16, kw=16, oh=1, ow=1)[0] == INVALID               # 65280
    # 1 <= oh <= (ih - 1) * sh + kh - pad_t, likewise in x
    _admitted(oh=1, ow=1)
    _admitted(oh=10, ow=12)
    rc, msg = _create(oh=11)
    assert rc == INVALID and "output size" in msg, (rc, msg)
    assert _create(ow=13)[0] == INVALID
    _admitted(**K4, oh=11, ow=13)                                                # 8 + 4 - 1, 10 + 4 - 1
    assert _create(**K4, oh=12, ow=13)[0] == INVALID
    assert _create(**K4, oh=11, ow=14)[0] == INVALID
    _admitted(**K3)
    assert _create(**K3, oh=11)[0] == INVALID
    _admitted(kh=2, kw=2, sh=3, sw=3, oh=14, ow=17)                              # holes: 4 * 3 + 2, 5 * 3 + 2
    assert _create(kh=2, kw=2, sh=3, sw=3, oh=15, ow=17)[0] == INVALID
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
    one = dict(ic=1, kh=1, kw=1, sh=1, sw=1)
    _admitted(**one, bs=(1 << 31) - 1, ih=1, iw=1, oh=1, ow=1)
    assert _create(**one, bs=1 << 11, ih=1 << 10, iw=1 << 10, oh=1, ow=1)[0] == INVALID          # src: exactly 2^31
    rc, msg = _create(bs=1 << 30, ih=1, iw=1, oh=2, ow=1)                                         # dst: exactly 2^31 (src 2^30)
    assert rc == INVALID and "pixel count" in msg, (rc, msg)
    _admitted(bs=(1 << 30) - 1, ih=1, iw=1, oh=2, ow=1)
    # force_path = MFMA outside its class: every clause of the class
    for kw in (dict(ic=16), dict(ic=48), dict(ic=1), dict(oc=16), dict(oc=48), dict(oc=7),                     # channels
               dict(sh=1, sw=1, oh=6, ow=7), dict(sh=2, sw=1, ow=7), dict(sh=1, sw=2, oh=6), dict(sh=3, sw=3),  # stride
               dict(kh=1, kw=1, oh=9, ow=11), dict(kh=5, kw=5), dict(kh=2, kw=4), dict(kh=4, kw=3), dict(kh=3, kw=2),  # window
               dict(pad_t=1, oh=9), dict(pad_l=1, ow=11),                                                       # 2x2 with padding
               dict(ic=1120, oh=1, ow=1),                                                                       # LDS: 2x2, 35 K-steps
               dict(K4, ic=288), dict(K3, ic=288),                                                              # LDS: 4x4 / 3x3, 9 K-steps
               dict(bs=1, ic=1024, ih=1 << 11, iw=1 << 10, oh=1, ow=1),                                         # a source image of 2^31 bytes
               dict(bs=1, ih=1 << 12, iw=1 << 12, oh=1 << 13, ow=1 << 13),                                      # a dst image of 2^31 bytes
               dict(bs=1, ih=1 << 11, iw=1 << 11, oh=1 << 12, ow=1 << 12, dst_dt=capi.DFX_S32)):
        rc, msg = _create(force_path=capi.DECONV_MFMA, **kw)
        assert rc == UNSUPPORTED and "MFMA kernel's class" in msg, (kw, rc, msg)
        _admitted(**kw)                                                  # on auto the op is total
    for kw in (dict(), K4, K3, dict(K4, pad_t=0, pad_l=0), dict(K4, pad_t=3, pad_l=3, oh=9, ow=11), dict(K4, pad_t=2, pad_l=0),
               dict(K3, pad_t=0, pad_l=2, oh=11, ow=11), dict(K3, pad_t=2, pad_l=2, oh=9, ow=11),
               dict(ic=1088, oh=1, ow=1), dict(K4, ic=256), dict(K3, ic=256), dict(oc=160), dict(oc=1024),
               dict(oh=9, ow=11), dict(oh=1, ow=1), dict(K4, oh=9, ow=11),
               dict(bs=1, ic=1024, ih=(1 << 11) - 1, iw=1 << 10, oh=1, ow=1),
               dict(bs=1, ih=1 << 12, iw=1 << 12, oh=(1 << 13) - 1, ow=1 << 13)):
        _admitted(force_path=capi.DECONV_MFMA, **kw)                     # every admitted value of each clause
    # null arguments
    L = capi.lib()
    assert L.dfx_deconv_create(None, ctypes.byref(ctypes.c_void_p())) == INVALID
    assert L.dfx_deconv_create(ctypes.byref(capi.DeconvDesc()), None) == INVALID
    assert L.dfx_deconv_submit(None, None, None, None) == INVALID
    assert L.dfx_deconv_submit_host(None, None, None) == INVALID
    assert L.dfx_deconv_set_weights(None, None, None, None) == INVALID
    assert L.dfx_deconv_query(None, None) == INVALID
    assert L.dfx_debug_deconv_requant(None, None) == INVALID
    assert L.dfx_deconv_destroy(None) == 0
    # a bad descriptor is refused through the Python class as well
    with pytest.raises(dfa.DfxError) as e:
        dfa.Deconv((1, 4, 4, 32), 32, (2, 2), nscales=5)
    assert "dfx error 1" in str(e.value)
    with pytest.raises(dfa.DfxError) as e:
        dfa.Deconv((1, 4, 4, 32), 32, (2, 2), out_hw=(9, 8))
    assert "dfx error 1" in str(e.value)


VALID = [
    dict(), K4, K3, dict(K4, pad_t=0, pad_l=0),                                            # MFMA class
    dict(oh=9, ow=11, relu=1, round_mode=capi.ROUND_DOWN),                                 # cropped
    dict(oc=128, dst_dt=capi.DFX_S32, bia_dt=capi.DFX_F32, nscales=128),
    dict(force_path=capi.DECONV_MFMA),
    dict(force_path=capi.DECONV_GENERIC),
    dict(ic=1), dict(ic=3), dict(oc=7, nscales=7), dict(kh=5, kw=5, pad_t=2, pad_l=2),     # outside it: the generic path
    dict(sh=1, sw=1, oh=6, ow=7), dict(sh=3, sw=3, oh=14, ow=17), dict(sh=2, sw=1, ow=7),
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
            dfa.Deconv((1, 4, 4, 32), 32, (2, 2))
        assert "dfx error 4" in str(e.value) and "no HIP device" in str(e.value)


def test_deconv_structs_match_the_header(tmp_path):
    """dfx_deconv_desc / dfx_deconv_info compiled by gcc have the sizes and field offsets of the ctypes mirrors"""
    pairs = {"dfx_deconv_desc": capi.DeconvDesc, "dfx_deconv_info": capi.DeconvInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dfx.h"', 'int main(void) {']
    for cname, ct in pairs.items():
        lines.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in ct._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines.append('printf("path mfma %d\\n", DFX_DECONV_MFMA); printf("path generic %d\\n", DFX_DECONV_GENERIC);')
    lines.append('printf("dfx_conv_desc size %zu\\n", sizeof(dfx_conv_desc));')
    lines.append('printf("dfx_gconv_desc size %zu\\n", sizeof(dfx_gconv_desc));')
    lines.append('printf("dfx_imgconv_desc size %zu\\n", sizeof(dfx_imgconv_desc));')
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
    assert seen[("path", "mfma")] == capi.DECONV_MFMA == R.MFMA and seen[("path", "generic")] == capi.DECONV_GENERIC == R.GENERIC
    assert capi.DECONV_AUTO == -1
    # dfx_gconv_desc without `groups`
    assert [n for n, _ in capi.DeconvDesc._fields_] == [n for n, _ in capi.GConvDesc._fields_ if n != "groups"]
    assert [n for n, _ in capi.DeconvInfo._fields_] == [n for n, _ in capi.GConvInfo._fields_]
    # the other descriptors are untouched
    assert ctypes.sizeof(capi.ConvDesc) == 100 == seen[("dfx_conv_desc", "size")]
    assert ctypes.sizeof(capi.GConvDesc) == 80 == seen[("dfx_gconv_desc", "size")]
    assert ctypes.sizeof(capi.ImgConvDesc) == 76 == seen[("dfx_imgconv_desc", "size")]


def test_library_exports_the_deconv_entry_points():
    L = capi.lib()
    for s in ("dfx_deconv_create", "dfx_deconv_set_weights", "dfx_deconv_submit", "dfx_deconv_submit_host",
              "dfx_deconv_query", "dfx_deconv_destroy", "dfx_debug_deconv_requant"):
        assert s in dfa.declared_symbols() and hasattr(L, s), s
    assert not [s for s in dfa.declared_symbols() if not hasattr(L, s)]
    for name in ("Deconv", "DeconvDesc", "DeconvInfo", "DECONV_AUTO", "DECONV_MFMA", "DECONV_GENERIC", "deconv_out_hw"):
        assert hasattr(dfa, name), name
    assert dfa.deconv_out_hw(5, 6, (4, 4), (2, 2), (1, 1)) == (10, 12)
    assert dfa.deconv_out_hw(5, 6, (3, 3), (2, 2), (1, 1), (1, 1)) == (10, 12)


def test_dropin_layer_exports_deconvolution_and_tools_are_built():
    so = os.path.join(PKG, "libdeepfusion.so")
    assert os.path.exists(so), "run __graft_entry__.build() first"
    syms = subprocess.check_output(["nm", "-D", "-C", "--defined-only", so]).decode()
    assert "deepfusion::deconvolution(" in syms
    for tool in ("deconv_check", "deconv_pack_check", "bench_deconv"):
        exe = os.path.join(PKG, "tools", tool)
        assert os.path.exists(exe) and os.access(exe, os.X_OK), tool


def test_deconv_pack_check_is_clean_under_the_host_sanitizers(tmp_path):
    """tools/deconv_pack_check.cc, a stand-alone host program over csrc/deconv_pack.h, built with ASan + UBSan: every
    packed byte is the weight the layout formula names, the zero row / column of a 3x3 window is zero, no source weight
    is lost or doubled, no byte outside the image is touched"""
    src = os.path.join(PKG, "tools", "deconv_pack_check.cc")
    assert os.path.exists(src), "tools/deconv_pack_check.cc is missing"
    probe = tmp_path / "probe.cc"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++"] + flags + [str(probe), "-o", str(tmp_path / "probe")], stdout=subprocess.DEVNULL,
                      stderr=subprocess.DEVNULL).returncode != 0:
        pytest.skip("this compiler has no sanitizer runtime")
    exe = tmp_path / "deconv_pack_check"
    subprocess.check_call(["g++"] + flags + [src, "-o", str(exe)])
    p = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0, p.stdout.decode()
    assert b"all 27 shapes packed, every dead byte zero" in p.stdout, p.stdout.decode()


def test_tables_cover_what_they_claim():
    m, g = R.mfma_table(), R.generic_table()
    assert all(c.mfma_class for c in m) and not any(c.mfma_class for c in g)
    assert len(m) == 4 * 5 * 4 and sum(len(R.mfma_table(n)) for n, _, _, _ in R.MFMA_GEOMS) == len(m)
    assert {(c.k, c.pad) for c in m} == {((2, 2), (0, 0)), ((4, 4), (1, 1)), ((3, 3), (1, 1)), ((4, 4), (0, 0))}
    assert {c.stride for c in m} == {(2, 2)} and {c.bs for c in m} == {1, 3}
    assert {(c.ih, c.iw) for c in m} == {(1, 1), (3, 5), (2, 33), (5, 70), (4, 6)}
    assert {(c.c, c.oc) for c in m} == {(32, 32), (64, 96), (160, 64), (32, 160)}
    for c in m:
        if c.k == (3, 3) and (c.ih, c.iw) != (4, 6):
            assert (c.oh, c.ow) == (2 * c.ih, 2 * c.iw)                                # output_padding 1
        if (c.ih, c.iw) == (4, 6):
            assert (c.oh, c.ow) == (7, 11)                                             # cropped to odd sizes
        assert 1 <= c.oh <= (c.ih - 1) * 2 + c.k[0] - c.pad[0] and 1 <= c.ow <= (c.iw - 1) * 2 + c.k[1] - c.pad[1]
    assert any(c.oc // 32 > c.lds_blocks for c in m)                                   # a second weight chunk
    assert any(c.c // 32 >= 5 for c in m)                                              # several K-steps
    assert any(c.dense_expressible for c in m) and any(not c.dense_expressible for c in m)
    for t in (m, g):
        assert {c.dst_dt for c in t} == {C.U8, C.S8, C.S32, C.F32}
        assert {c.bia_dt for c in t} == {C.UNDEF, C.F32, C.S32, C.S8, C.U8}
        assert {c.per_channel for c in t} == {True, False} and {c.rm for c in t} == {0, 1} and {c.relu for c in t} == {True, False}
        assert any(c.wide for c in t)
    assert {(c.k, c.stride) for c in g} == {((3, 3), (1, 1)), ((2, 2), (3, 3)), ((3, 3), (2, 1)), ((5, 5), (2, 2))}
    assert {(c.c, c.oc) for c in g} == {(ic, oc) for ic in (1, 3, 20) for oc in (1, 7, 48)}
    assert len({c.ident() for c in R.all_tables()}) == len(R.all_tables())


@pytest.mark.parametrize("impl", ["scalar_mt", "avx512"])
def test_reference_equals_the_oracles_dense_conv_on_the_stuffed_tensor(oracle, impl):
    """defining property 2 on the reference: every table case with ic and oc multiples of 16, the same twin padding on
    both axes and the derived output size, against the C oracle's dense stride-1 conv on the zero-stuffed tensor with
    the flipped weights: this pins the reference of the GPU tests"""
    if impl == "avx512" and not oracle.have_avx512_vnni():
        impl = "scalar"       # the oracle's other implementation on a host without AVX-512 VNNI
    n, seen = 0, set()
    for case in R.all_tables():
        if not case.dense_expressible:
            continue
        data = R.generate(case)
        want = hipref.oracle_conv(oracle, R.dense_case(case), R.dense_data(case, data), impl=impl)
        hipref.assert_bit_equal(R.deconv_ref(case, data), want, "%s vs oracle %s" % (case.ident(), impl))
        n += 1
        seen.add((case.k, case.stride, case.pad))
    assert n >= 36 and seen == {((2, 2), (2, 2), (0, 0)), ((4, 4), (2, 2), (1, 1)), ((4, 4), (2, 2), (0, 0))}


def _gcase(case):
    return G.GCase(case.name, case.bs, case.c, (case.ih - 1) * case.stride[0] + 1, (case.iw - 1) * case.stride[1] + 1, case.oc, 1,
                   k=case.k, stride=(1, 1), pad=R.twin_pad(case), out_hw=(case.oh, case.ow), dst_dt=case.dst_dt, bia_dt=case.bia_dt,
                   relu=case.relu, rm=case.rm, per_channel=case.per_channel, wide=case.wide, seed=case.seed)


def test_reference_equals_the_grouped_reference_on_the_stuffed_tensor():
    """defining property 1 on the reference, for every table case (output_padding, cropped outputs, holes, mixed
    strides, channel counts that are no multiple of 16 included)"""
    for case in R.all_tables():
        data = R.generate(case)
        gdata = dict(data, src=R.stuff(data["src"], case.stride), w=R.flip(data["w"]))
        hipref.assert_bit_equal(R.deconv_ref(case, data), G.gconv_ref(_gcase(case), gdata), case.ident())


def test_hand_written_values():
    """a 1x1 input: the output is the kernel itself times the pixel; and stride 3 with a 2x2 window: every third row and
    column is reached by no tap and holds requant(0)"""
    w = np.arange(-6, 6, dtype=np.int8).reshape(1, 1, 3, 4)
    src = np.array([[[[7]]]], dtype=np.uint8)
    acc = R.deconv_acc(src, w, (2, 2), (0, 0), (3, 4))
    assert np.array_equal(acc[0, :, :, 0], 7 * w[0, 0].astype(np.int64))
    acc = R.deconv_acc(src, w, (2, 2), (1, 2), (2, 2))                     # the canvas from (1, 2) on
    assert np.array_equal(acc[0, :, :, 0], 7 * w[0, 0, 1:, 2:].astype(np.int64))
    # two input channels, two output channels, by hand
    w2 = np.array([[[[1, 2], [3, 4]], [[10, 20], [30, 40]]], [[[-1, -2], [-3, -4]], [[0, 0], [0, 5]]]], dtype=np.int8)   # {2, 2, 2, 2}
    src2 = np.array([[[[2, 3]]]], dtype=np.uint8)
    acc = R.deconv_acc(src2, w2, (2, 2), (0, 0), (2, 2))
    assert acc[0, :, :, 0].tolist() == [[32, 64], [96, 128]] and acc[0, :, :, 1].tolist() == [[-2, -4], [-6, 7]]
    # holes
    case = R.DCase("holes", 1, 1, 2, 2, 1, k=(2, 2), stride=(3, 3), pad=(0, 0), dst_dt=C.S32, bia_dt=C.S32, relu=False)
    assert (case.oh, case.ow) == (5, 5)
    data = dict(src=np.array([[[[1], [2]], [[3], [4]]]], dtype=np.uint8), w=np.array([[[[1, 2], [3, 4]]]], dtype=np.int8),
                bia=np.array([9], dtype=np.int32), scales=np.array([1.0], dtype=np.float32))
    ref = R.deconv_ref(case, data)[0, :, :, 0]
    assert ref.tolist() == [[10, 11, 9, 11, 13], [12, 13, 9, 15, 17], [9, 9, 9, 9, 9], [12, 15, 9, 13, 17], [18, 21, 9, 21, 25]]
    # the gather formula of include/dfx.h on a few pixels of a table case
    case = [c for c in R.generic_table() if c.k == (5, 5) and c.c == 3 and c.oc == 7][0]
    data = R.generate(case)
    acc = R.deconv_acc(data["src"], data["w"], case.stride, case.pad, (case.oh, case.ow))
    for n, oy, ox, o in ((0, 0, 0, 0), (1, 9, 7, 6), (0, 4, 3, 2), (1, 5, 0, 3)):
        want = 0
        for ky in range(5):
            for kx in range(5):
                ty, tx = oy + case.pad[0] - ky, ox + case.pad[1] - kx
                if ty % 2 == 0 and tx % 2 == 0 and 0 <= ty // 2 < case.ih and 0 <= tx // 2 < case.iw:
                    want += int(np.dot(data["src"][n, ty // 2, tx // 2].astype(np.int64), data["w"][o, :, ky, kx].astype(np.int64)))
        assert int(acc[n, oy, ox, o]) == want, (n, oy, ox, o)


def test_rows_of_the_reference_are_the_rows_of_the_whole():
    case = R.DCase("rows", 2, 32, 6, 5, 32, k=(4, 4), pad=(1, 1), seed=35000, **R.OPTIONS[0])
    data = R.generate(case)
    whole = R.deconv_ref(case, data)
    hipref.assert_bit_equal(R.deconv_ref(case, data, rows=(0, 5, 11)), np.ascontiguousarray(whole[:, [0, 5, 11]]), "rows")


@pytest.mark.parametrize("geom", [g[0] for g in R.MFMA_GEOMS])
def test_permutation_case_has_distinct_weights(geom):
    """at every (i, ky, kx) the 32 output channels' weights are distinct; within an output channel any 255 taps that are
    consecutive in (i, ky, kx) order are distinct (all of them for the 2x2 window), so the taps of one input channel and
    the 32 input channels of one (ky, kx) are"""
    case, data = R.permutation_case(geom)
    assert case.mfma_class
    w = data["w"].reshape(32, -1).astype(np.int64)
    taps = w.shape[1]
    assert all(len(set(col.tolist())) == 32 for col in w.T)
    for row in w:
        assert all(len(set(row[t:t + 255].tolist())) == min(255, taps - t) for t in range(0, taps, 64))
    w4 = data["w"].astype(np.int64)
    for ky in range(case.k[0]):
        for kx in range(case.k[1]):
            assert all(len(set(w4[o, :, ky, kx].tolist())) == 32 for o in range(32))
    assert R.deconv_ref(case, data).dtype == np.int32


def test_wide_cases_reach_both_ends_of_the_range():
    """a "wide" 1-byte case's expected output holds both ends of what its dtype and ReLU flag can reach"""
    n = 0
    for case in R.all_tables():
        if not case.wide or case.dst_dt not in (C.U8, C.S8) or case.bs * case.oh * case.ow * case.oc < 2000:
            continue
        ref = R.deconv_ref(case, R.generate(case))
        lo = 0 if (case.relu or case.dst_dt == C.U8) else -128
        hi = 255 if case.dst_dt == C.U8 else 127
        assert ref.min() == lo and ref.max() == hi, (case.ident(), ref.min(), ref.max())
        n += 1
    assert n >= 8


@pytest.mark.parametrize("edge", R.EDGES, ids=lambda e: e.name)
def test_edge_data_attains_the_bound_the_proof_uses(edge):
    """(255 * max(P, N) + |bias|) * scale is exactly 2^30 at the last admitted value, one scale step beyond at the first
    rejected one; the prescribed weights sit on nine (tap, input channel) positions of ONE parity, every other weight of
    the channel is zero, and EDGE_PIXEL's accumulator is exactly 255 P / -255 N"""
    case, data = R.edge_case(edge, C.S32)
    assert case.mfma_class
    w = data["w"][R.EDGE_CHANNEL]
    assert len(set(R.EDGE_POSITIONS)) == 9 and {(ky % 2, kx % 2) for ky, kx, i in R.EDGE_POSITIONS} == {(0, 0)}
    assert tuple(int(w[i, ky, kx]) for ky, kx, i in R.EDGE_POSITIONS) == edge.weights
    rest = w.copy()
    for ky, kx, i in R.EDGE_POSITIONS:
        rest[i, ky, kx] = 0
    assert not rest.any()
    acc, bound, P, N = R.edge_attained(edge, case, data)
    assert acc == bound and abs(bound) == 255 * max(P, N)
    reach = (255 * max(P, N) + abs(edge.bias)) * edge.scale
    assert reach == (R.LIMIT if edge.fast else R.LIMIT + edge.scale)
    ref = R.deconv_ref(case, data)
    img = 0 if edge.which == "max" else 1
    sign = 1 if edge.which == "max" else -1
    assert int(ref[img, R.EDGE_PIXEL[0], R.EDGE_PIXEL[1], R.EDGE_CHANNEL]) == sign * int(reach)
