"""CPU-only checks of the activation resize op: the numpy reference the GPU tests compare against (tests/resize_ref.py)
equals a scalar loop of the formula, lies within the final rounding of the exact rational interpolation, follows torch's
coordinate conventions and has the op's defining properties (2x2 average pooling, identity, transposed conv with identity
weights, resize then eltwise-sum); the library's own tables (csrc/resize_plan.h, printed by tools/resize_plan_check,
also built under the host sanitizers as a stand-alone program) equal the numpy tables bit for bit; the C ABI validates
descriptors before it touches a device, the ctypes mirrors match the header, the symbols are exported and the drop-in
layer and tools are built."""
import ctypes
import importlib
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import deconv_ref as D
import refmath
import resize_ref as R

dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-fusion_amd")
INVALID, UNSUPPORTED, NO_DEVICE = 1, 2, 4
MODES = [(a, c) for a in (R.NEAREST, R.BILINEAR) for c in (R.HALF_PIXEL, R.ALIGN_CORNERS, R.ASYMMETRIC)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---- 1. independent formulation -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", R.GEOMS, ids=lambda g: "%dx%d-%dx%d" % g)
def test_reference_equals_the_scalar_loop(geom):
    ih, iw, oh, ow = geom
    for dtype in (np.uint8, np.int8, np.float32):
        src = R.random_src((2, ih, iw, 3), dtype, seed=ih * 100 + ow)
        for algo, coord in MODES:
            got, want = R.resize(src, (oh, ow), algo, coord), R.resize_scalar(src, (oh, ow), algo, coord)
            assert got.dtype == want.dtype == src.dtype and got.shape == (2, oh, ow, 3)
            assert np.array_equal(_bits(got), _bits(want)), (geom, dtype, algo, coord)
    src = R.random_src((1, ih, iw, 2), np.int32, seed=5)
    for coord in (R.HALF_PIXEL, R.ALIGN_CORNERS, R.ASYMMETRIC):
        assert np.array_equal(R.resize(src, (oh, ow), R.NEAREST, coord), R.resize_scalar(src, (oh, ow), R.NEAREST, coord))


# ---- 2. exact rational ---------------------------------------------------------------------------------------------------
def _exact(src, out_hw, coord):
    """the bilinear interpolation in exact rationals: the same integer index plan, weights num % den / den as Fractions"""
    bs, ih, iw, c = src.shape

    def axis(n, m):
        num, den = R.num_den(n, m, coord)
        out = []
        for v in num:
            v = max(int(v), 0)
            i0 = min(v // den, n - 1)
            out.append((i0, min(i0 + 1, n - 1), Fraction(v % den, den)))
        return out
    ys, xs = axis(ih, out_hw[0]), axis(iw, out_hw[1])
    res = np.empty((bs, out_hw[0], out_hw[1], c), dtype=object)
    for n in range(bs):
        for oy, (y0, y1, wy) in enumerate(ys):
            for ox, (x0, x1, wx) in enumerate(xs):
                for k in range(c):
                    top = int(src[n, y0, x0, k]) * (1 - wx) + int(src[n, y0, x1, k]) * wx
                    bot = int(src[n, y1, x0, k]) * (1 - wx) + int(src[n, y1, x1, k]) * wx
                    res[n, oy, ox, k] = top * (1 - wy) + bot * wy
    return res


@pytest.mark.parametrize("geom", R.GEOMS + [(5, 7, 13, 9)], ids=lambda g: "%dx%d-%dx%d" % g)
def test_integer_results_are_the_rounded_exact_interpolation(geom):
    """the f32 error of three rounded products and sums of values <= 255 is below 2^-10, so only the final rounding
    separates the reference from the exact rational value: |ref - exact| <= 0.5 + 2^-10"""
    ih, iw, oh, ow = geom
    bound = Fraction(1, 2) + Fraction(1, 1024)
    worst = Fraction(0)
    for dtype in (np.uint8, np.int8):
        src = R.random_src((1, ih, iw, 2), dtype, seed=11)
        for coord in (R.HALF_PIXEL, R.ALIGN_CORNERS, R.ASYMMETRIC):
            ref, exact = R.resize(src, (oh, ow), R.BILINEAR, coord), _exact(src, (oh, ow), coord)
            err = max(abs(int(r) - e) for r, e in zip(ref.reshape(-1), exact.reshape(-1)))
            worst = max(worst, err)
    print("worst |reference - exact| on %s: %.4f" % (geom, float(worst)))
    assert worst <= bound, (geom, float(worst))


# ---- 3. / 4. conventions against torch on the CPU -------------------------------------------------------------------------
def _torch_nearest_index(n, m, mode):
    import torch
    import torch.nn.functional as F
    x = torch.arange(n, dtype=torch.float32).reshape(1, 1, 1, n)
    return F.interpolate(x, size=(1, m), mode=mode).reshape(-1).to(torch.int64).numpy()


def test_nearest_conventions_are_torchs():
    """ASYMMETRIC nearest is torch's legacy 'nearest' on all 897 pairs; HALF_PIXEL nearest is 'nearest-exact' on all but
    three pairs, where torch's float index is off by one and the integer arithmetic is asserted by hand"""
    off = {}
    pairs = 0
    for n in range(1, 24):
        for m in range(1, 40):
            pairs += 1
            i0 = R.tables(n, m, R.NEAREST, R.ASYMMETRIC)[0]
            assert np.array_equal(i0, _torch_nearest_index(n, m, "nearest")), (n, m)
            i0 = R.tables(n, m, R.NEAREST, R.HALF_PIXEL)[0]
            t = _torch_nearest_index(n, m, "nearest-exact")
            if not np.array_equal(i0, t):
                off[(n, m)] = np.flatnonzero(i0 != t).tolist()
    assert pairs == 897
    assert sorted(off) == [(6, 37), (12, 37), (14, 23)], off
    # floor((2o+1) * in / (2 * out)) by hand at the output index where torch differs: the quotient is an exact integer
    # there ((2o+1) * in is a multiple of 2 * out), which torch's f32 product (o + 0.5) * (in / out) falls just short of
    for (n, m), where in off.items():
        for o in where:
            assert ((2 * o + 1) * n) % (2 * m) == 0, (n, m, o)
            assert R.tables(n, m, R.NEAREST, R.HALF_PIXEL)[0][o] == ((2 * o + 1) * n) // (2 * m)
    assert R.tables(6, 37, R.NEAREST, R.HALF_PIXEL)[0][18] == 3        # 37 * 6 / 74
    assert R.tables(12, 37, R.NEAREST, R.HALF_PIXEL)[0][18] == 6       # 37 * 12 / 74
    assert R.tables(14, 23, R.NEAREST, R.HALF_PIXEL)[0][11] == 7       # 23 * 14 / 46


def test_bilinear_f32_is_torchs_bilinear_within_rounding():
    import torch
    import torch.nn.functional as F
    worst = 0.0
    rng = np.random.default_rng(3)
    for ih, iw, oh, ow in R.GEOMS:
        src = rng.standard_normal((2, ih, iw, 3)).astype(np.float32)
        t = torch.from_numpy(src).permute(0, 3, 1, 2).contiguous()
        for coord, ac in ((R.HALF_PIXEL, False), (R.ALIGN_CORNERS, True)):
            want = F.interpolate(t, size=(oh, ow), mode="bilinear", align_corners=ac).permute(0, 2, 3, 1).numpy()
            got = R.resize(src, (oh, ow), R.BILINEAR, coord)
            worst = max(worst, float(np.abs(got - want).max()))
    print("largest |reference - torch bilinear|: %.3g" % worst)
    assert worst <= R.TORCH_BILINEAR_TOL, worst


# ---- 5. defining properties on the reference alone -----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.int8])
def test_bilinear_half_pixel_at_half_size_is_the_2x2_average_pooling(dtype):
    info = np.iinfo(dtype)
    src = R.random_src((2, 8, 12, 5), dtype, seed=21)
    src[0, 0:2, 0:2, :] = info.min                                  # all-min and all-max windows
    src[0, 0:2, 2:4, :] = info.max
    src[0, 2:4, 0:2, 0] = [[1, 2], [3, 4]]                          # sum 10: 2.5 -> 2
    src[0, 2:4, 2:4, 0] = [[1, 2], [3, 8]]                          # sum 14: 3.5 -> 4
    src[0, 2:4, 4:6, 0] = [[info.max, info.max], [info.max, info.max - 2]]   # x.5 just below the top
    got = R.resize(src, (4, 6), R.BILINEAR, R.HALF_PIXEL)
    want = refmath.avgpool(src, (2, 2), (2, 2), (0, 0), (4, 6), include_padding=True)
    assert np.array_equal(got, want)
    assert got[0, 1, 0, 0] == 2 and got[0, 1, 1, 0] == 4 and got[0, 0, 0, 0] == info.min and got[0, 0, 1, 0] == info.max


def test_identity_size_is_a_copy_of_integer_tensors():
    for dtype in (np.uint8, np.int8):
        src = R.random_src((2, 5, 7, 3), dtype, seed=4)
        for algo, coord in MODES:
            assert np.array_equal(R.resize(src, (5, 7), algo, coord), src), (dtype, algo, coord)
    # f32: nearest is a bit copy, NaN payloads included; bilinear is not (-0 * 1 + x * 0 is +0, Inf * 0 is NaN)
    src = np.array([-0.0, 1.5, 2.0, -3.0], dtype=np.float32).reshape(1, 2, 2, 1)
    nan = np.array([0x7fc12345, 0xffc00001, 0x7f800000, 0x00000001], dtype=np.uint32).view(np.float32).reshape(1, 2, 2, 1)
    for coord in (R.HALF_PIXEL, R.ALIGN_CORNERS, R.ASYMMETRIC):
        assert np.array_equal(_bits(R.resize(src, (2, 2), R.NEAREST, coord)), _bits(src))
        assert np.array_equal(_bits(R.resize(nan, (2, 2), R.NEAREST, coord)), _bits(nan))
        bil = R.resize(src, (2, 2), R.BILINEAR, coord)
        assert np.array_equal(bil, src) and not np.signbit(bil[0, 0, 0, 0]) and not np.array_equal(_bits(bil), _bits(src))
    row = np.array([np.inf, 1.0], dtype=np.float32).reshape(1, 1, 2, 1)
    bil = R.resize(row, (1, 2), R.BILINEAR, R.HALF_PIXEL)
    assert np.isnan(bil[0, 0, 0, 0]) and bil[0, 0, 1, 0] == 1.0


@pytest.mark.parametrize("s", [2, 3])
def test_nearest_at_an_integer_factor_is_the_transposed_conv_with_identity_weights(s):
    c = 5
    src = R.random_src((2, 4, 3, c), np.uint8, seed=s)
    w = np.zeros((c, c, s, s), dtype=np.int8)
    for k in range(c):
        w[k, k] = 1
    case = D.DCase("ident", 2, c, 4, 3, c, k=(s, s), stride=(s, s), pad=(0, 0), dst_dt=D.U8, bia_dt=D.UNDEF, relu=False)
    want = D.deconv_ref(case, dict(src=src, w=w, bia=None, scales=np.array([1.0], dtype=np.float32)))
    for coord in (R.ASYMMETRIC, R.HALF_PIXEL):
        assert np.array_equal(R.resize(src, (4 * s, 3 * s), R.NEAREST, coord), want), coord


def test_fused_add_is_resize_then_the_oracles_eltwise_sum(oracle):
    for dtype in (np.uint8, np.int8, np.float32, np.int32):
        src = R.random_src((2, 5, 7, 3), dtype, seed=8)
        add = R.random_src((2, 10, 14, 3), dtype, seed=9)
        for algo in (R.NEAREST,) if dtype == np.int32 else (R.NEAREST, R.BILINEAR):
            for relu in (False, True):
                got = R.resize_add(src, add, (10, 14), algo, R.HALF_PIXEL, relu)
                want = oracle.eltwise_sum([R.resize(src, (10, 14), algo, R.HALF_PIXEL), add], post_relu=relu)
                assert np.array_equal(_bits(got), _bits(want)), (dtype, algo, relu)


# ---- 6. the library's tables --------------------------------------------------------------------------------------------
def _tool_tables(exe, n, m, algo, coord):
    out = subprocess.check_output([exe, str(n), str(m), algo, coord], timeout=120).decode().split("\n")
    rows = [ln.split() for ln in out if ln]
    assert [int(r[0]) for r in rows] == list(range(m))
    return ([int(r[1]) for r in rows], [int(r[2]) for r in rows], [float.fromhex(r[3]) for r in rows],
            [float.fromhex(r[4]) for r in rows])


def _assert_tables(exe):
    for n, m in R.PLAN_PAIRS:
        for aname, algo in R.ALGOS.items():
            for cname, coord in R.COORDS.items():
                i0, i1, w0, w1 = _tool_tables(exe, n, m, aname, cname)
                r0, r1, v0, v1 = R.tables(n, m, algo, coord)
                assert i0 == r0.tolist() and i1 == r1.tolist(), (n, m, aname, cname)
                # float.fromhex of a printed f32 is exact, and so is float(np.float32): equality is bit equality
                assert w0 == [float(v) for v in v0] and w1 == [float(v) for v in v1], (n, m, aname, cname)


def test_the_librarys_tables_are_the_numpy_tables():
    exe = os.path.join(PKG, "tools", "resize_plan_check")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    _assert_tables(exe)


def test_resize_plan_check_is_clean_under_the_host_sanitizers(tmp_path):
    """tools/resize_plan_check.cc, a stand-alone host program over csrc/resize_plan.h, built with ASan + UBSan: its own
    walk over 1944 axis plans (65535 among the sizes) and the printed tables of every pair.  Nothing is loaded into Python."""
    src = os.path.join(PKG, "tools", "resize_plan_check.cc")
    assert os.path.exists(src), "tools/resize_plan_check.cc is missing"
    probe = tmp_path / "probe.cc"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(["g++"] + flags + [str(probe), "-o", str(tmp_path / "probe")], stdout=subprocess.DEVNULL,
                      stderr=subprocess.DEVNULL).returncode != 0:
        pytest.skip("this compiler has no sanitizer runtime")
    exe = tmp_path / "resize_plan_check"
    subprocess.check_call(["g++"] + flags + [src, "-o", str(exe)])
    p = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()
    assert "all 1944 axis plans keep their indices inside the source" in p.stdout.decode()
    _assert_tables(str(exe))
    assert subprocess.run([str(exe), "0", "4", "nearest", "half_pixel"], stderr=subprocess.DEVNULL).returncode == 2
    assert subprocess.run([str(exe), "4", "65536", "bilinear", "asymmetric"], stderr=subprocess.DEVNULL).returncode == 2


# ---- 7. descriptor and build checks -------------------------------------------------------------------------------------
def _create(**kw):
    d = dict(bs=2, c=16, ih=5, iw=7, oh=10, ow=14, dt=capi.DFX_U8, algo=capi.RESIZE_BILINEAR, coord=capi.COORD_HALF_PIXEL,
             add=0, post_relu=0, force_path=capi.RESIZE_AUTO)
    d.update(kw)
    desc = capi.ResizeDesc(**d)
    h = ctypes.c_void_p()
    rc = capi.lib().dfx_resize_create(ctypes.byref(desc), ctypes.byref(h))
    msg = capi.lib().dfx_last_error().decode()
    if rc == 0:
        assert capi.lib().dfx_resize_destroy(h) == 0
    else:
        assert not h.value
    return rc, msg


def _admitted(**kw):
    """a valid descriptor gets past validation: it creates with a device and fails with NO_DEVICE without one"""
    rc, msg = _create(**kw)
    assert rc in (0, NO_DEVICE), (kw, rc, msg)


def test_descriptor_validation_needs_no_device():
    for bad in ("bs", "c", "ih", "iw", "oh", "ow"):
        assert _create(**{bad: 0})[0] == INVALID, bad
        assert _create(**{bad: -3})[0] == INVALID, bad
    for size in ("ih", "iw", "oh", "ow"):
        assert _create(**{size: 65536})[0] == INVALID, size
        _admitted(**{size: 65535, "c": 1, "bs": 1})
    for c in (1, 3, 5, 21, 1000):
        _admitted(c=c)
    for key, bad in (("dt", 0), ("dt", 5), ("algo", -1), ("algo", 2), ("coord", -1), ("coord", 3), ("add", 2), ("post_relu", 2),
                     ("post_relu", -1), ("force_path", -2), ("force_path", 2)):
        assert _create(**{key: bad, **({"add": 1} if key == "post_relu" else {})})[0] == INVALID, (key, bad)
    rc, msg = _create(post_relu=1, add=0)
    assert rc == INVALID and "post_relu without add" in msg
    # bilinear on s32; nearest takes it
    rc, msg = _create(dt=capi.DFX_S32)
    assert rc == UNSUPPORTED and "s32" in msg, (rc, msg)
    _admitted(dt=capi.DFX_S32, algo=capi.RESIZE_NEAREST)
    # force_path = BAND outside the class: c * element size no multiple of 16
    for kw in (dict(c=5), dict(c=24), dict(c=3, dt=capi.DFX_F32), dict(c=21)):
        rc, msg = _create(force_path=capi.RESIZE_BAND, **kw)
        assert rc == UNSUPPORTED and "class" in msg, (kw, rc, msg)
        _admitted(force_path=capi.RESIZE_GENERIC, **kw)
        _admitted(**kw)
    for kw in (dict(c=16), dict(c=48), dict(c=4, dt=capi.DFX_F32), dict(c=4, dt=capi.DFX_S32, algo=capi.RESIZE_NEAREST)):
        _admitted(force_path=capi.RESIZE_BAND, **kw)
    # ... or one image of 2^31 bytes or more
    rc, msg = _create(bs=1, c=32, ih=8192, iw=8192, oh=4, ow=4, force_path=capi.RESIZE_BAND)
    assert rc == UNSUPPORTED, (rc, msg)
    # a tensor of more than 2^40 elements, on either side: refused before any size product can leave 64 bits
    big = 2 ** 31 - 1
    for kw in (dict(c=big, ih=65535, iw=65535), dict(c=big, oh=65535, ow=65535), dict(bs=big, c=big),
               dict(bs=big, c=big, ih=65535, iw=65535, oh=65535, ow=65535, dt=capi.DFX_F32),
               dict(bs=2 ** 20, c=2 ** 20 + 1, ih=1, iw=1, oh=1, ow=1), dict(bs=1, c=257, ih=65535, iw=65535)):
        rc, msg = _create(**kw)
        assert rc == INVALID and "2^40" in msg, (kw, rc, msg)
    _admitted(bs=2 ** 20, c=2 ** 20, ih=1, iw=1, oh=1, ow=1)
    _admitted(bs=1, c=256, ih=65535, iw=65535, oh=1, ow=1)
    # an invalid field is reported before an unsupported combination
    assert _create(dt=capi.DFX_S32, coord=7)[0] == INVALID
    lib = capi.lib()
    assert lib.dfx_resize_create(None, None) == INVALID
    assert lib.dfx_resize_submit(None, None, None, None, None) == INVALID
    assert lib.dfx_resize_submit_host(None, None, None, None) == INVALID
    assert lib.dfx_resize_query(None, None) == INVALID
    assert lib.dfx_resize_destroy(None) == 0


def test_valid_descriptors_and_no_cpu_fallback():
    import torch
    for kw in (dict(), dict(add=1, post_relu=1), dict(c=5, dt=capi.DFX_S8, coord=capi.COORD_ALIGN_CORNERS),
               dict(algo=capi.RESIZE_NEAREST, coord=capi.COORD_ASYMMETRIC, dt=capi.DFX_S32, c=4)):
        rc, msg = _create(**kw)
        if torch.cuda.is_available():
            assert rc == 0, (kw, msg)
        else:
            assert rc == NO_DEVICE and "no HIP device" in msg, (kw, rc, msg)
    if not torch.cuda.is_available():
        with pytest.raises(dfa.DfxError) as e:
            dfa.Resize((1, 4, 4, 16), (8, 8), np.uint8)
        assert "dfx error 4" in str(e.value) and "no HIP device" in str(e.value)


def test_resize_structs_match_the_header(tmp_path):
    """dfx_resize_desc / dfx_resize_info compiled by gcc have the sizes and field offsets of the ctypes mirrors"""
    pairs = {"dfx_resize_desc": capi.ResizeDesc, "dfx_resize_info": capi.ResizeInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dfx.h"', 'int main(void) {']
    for cname, ct in pairs.items():
        lines.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in ct._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    for name in ("DFX_RESIZE_BAND", "DFX_RESIZE_GENERIC", "DFX_RESIZE_NEAREST", "DFX_RESIZE_BILINEAR", "DFX_COORD_HALF_PIXEL",
                 "DFX_COORD_ALIGN_CORNERS", "DFX_COORD_ASYMMETRIC", "DFX_VERSION"):
        lines.append('printf("enum %s %%d\\n", %s);' % (name, name))
    lines.append('printf("dfx_dilconv_desc size %zu\\n", sizeof(dfx_dilconv_desc));')
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
    assert [n for n, _ in capi.ResizeDesc._fields_] == ["bs", "c", "ih", "iw", "oh", "ow", "dt", "algo", "coord", "add",
                                                        "post_relu", "force_path"]
    assert seen[("enum", "DFX_RESIZE_BAND")] == capi.RESIZE_BAND == R.BAND
    assert seen[("enum", "DFX_RESIZE_GENERIC")] == capi.RESIZE_GENERIC == R.GENERIC
    assert seen[("enum", "DFX_RESIZE_NEAREST")] == capi.RESIZE_NEAREST == R.NEAREST
    assert seen[("enum", "DFX_RESIZE_BILINEAR")] == capi.RESIZE_BILINEAR == R.BILINEAR
    assert seen[("enum", "DFX_COORD_HALF_PIXEL")] == capi.COORD_HALF_PIXEL == R.HALF_PIXEL
    assert seen[("enum", "DFX_COORD_ALIGN_CORNERS")] == capi.COORD_ALIGN_CORNERS == R.ALIGN_CORNERS
    assert seen[("enum", "DFX_COORD_ASYMMETRIC")] == capi.COORD_ASYMMETRIC == R.ASYMMETRIC
    assert seen[("enum", "DFX_VERSION")] == 100 and capi.RESIZE_AUTO == -1
    assert ctypes.sizeof(capi.ResizeDesc) == 48
    assert ctypes.sizeof(capi.DilConvDesc) == 84 == seen[("dfx_dilconv_desc", "size")]      # the others are untouched


def test_library_exports_the_resize_entry_points():
    L = capi.lib()
    for s in ("dfx_resize_create", "dfx_resize_submit", "dfx_resize_submit_host", "dfx_resize_query", "dfx_resize_destroy",
              "dfx_debug_resize_launches"):
        assert s in dfa.declared_symbols() and hasattr(L, s), s
    assert not [s for s in dfa.declared_symbols() if not hasattr(L, s)]
    assert L.dfx_debug_resize_launches(None) == INVALID and min(capi.resize_launches()) >= 0     # needs no device
    for name in ("Resize", "ResizeDesc", "ResizeInfo", "RESIZE_AUTO", "RESIZE_BAND", "RESIZE_GENERIC", "RESIZE_NEAREST",
                 "RESIZE_BILINEAR", "COORD_HALF_PIXEL", "COORD_ALIGN_CORNERS", "COORD_ASYMMETRIC"):
        assert hasattr(dfa, name), name
    assert not hasattr(dfa, "resize_tables") and not hasattr(capi, "resize_tables")   # the package stays plumbing
    for key in ("DFX_RESIZE_ROWS", "DFX_RESIZE_MAX_GRID"):      # known to the library (an unknown key is refused)
        capi.set_tuning(key, "1")
        capi.set_tuning(key, None)


def test_dropin_layer_exports_resize_and_tools_are_built():
    so = os.path.join(PKG, "libdeepfusion.so")
    assert os.path.exists(so), "run __graft_entry__.build() first"
    syms = subprocess.check_output(["nm", "-D", "-C", "--defined-only", so]).decode()
    assert "deepfusion::resize(" in syms and "deepfusion::resize_add(" in syms
    for tool in ("resize_check", "resize_plan_check", "bench_resize"):
        exe = os.path.join(PKG, "tools", tool)
        assert os.path.exists(exe) and os.access(exe, os.X_OK), tool
