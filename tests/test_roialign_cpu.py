"""CPU-only checks of RoIAlign (dfx_roialign_*): the numpy reference of tests/roialign_ref.py against its pure-Python witness bit
for bit and against float64 within the bound its docstring derives, the pins against ops that already exist (a crop,
refmath.avgpool, resize_ref.resize) wherever the sample points fall on exact dyadic positions, roi_level_thresholds against
torchvision's LevelMapper in float64, the host plan of csrc/roialign_plan.h (tools/roialign_plan_check, also under the host
sanitizers as a stand-alone program), and the ctypes structs against the header."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import refmath
import resize_ref
import roialign_ref as R

dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "deep-fusion_amd", "tools")
F = np.float32


def _maps(rng, dtype, bs, shapes, c):
    if np.dtype(dtype) == np.float32:
        return [rng.standard_normal((bs, h, w, c)).astype(np.float32) * F(50) for h, w in shapes]
    info = np.iinfo(dtype)
    return [rng.integers(info.min, info.max + 1, (bs, h, w, c)).astype(dtype) for h, w in shapes]


def _boxes(rng, n, w, h, spread=0.3):
    """boxes around a w x h image, some reaching outside"""
    x = np.sort(rng.uniform(-spread * w, (1 + spread) * w, (n, 2)), axis=1)
    y = np.sort(rng.uniform(-spread * h, (1 + spread) * h, (n, 2)), axis=1)
    return np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], axis=1).astype(np.float32)


PLANTED = np.array([
    [-50, -50, -20, -20], [30, 2, 60, 9], [2, -40, 9, -20], [2, 30, 9, 60],        # wholly outside on each side
    [-3, 2, 4, 9], [12, 2, 25, 9], [3, -3, 9, 4], [3, 9, 9, 20],                    # straddling each border
    [-1.5, -1.5, 0.5, 0.5], [15, 11, 19, 15], [2, 3, 6, 7], [4, 4, 4, 4], [9, 9, 3, 2],
    [-800, -600, 900, 700], [np.nan, 1, 5, 5], [1, 1, np.inf, 5], [-np.inf, 1, 5, 5], [1e30, 1e30, 2e30, 2e30],
    [-1e30, 0, 1e30, 5], [1e-40, 1e-40, 3e-40, 2e-40], [0, 0, 17, 13]], dtype=np.float32)


@pytest.mark.parametrize("dtype", [np.uint8, np.int8, np.float32])
def test_reference_equals_the_scalar_witness(dtype):
    rng = np.random.default_rng(3)
    shapes = [(13, 17), (7, 9), (2, 2)]
    levels = _maps(rng, dtype, 2, shapes, 3)
    thr = np.array([30.0, 120.0], dtype=np.float32)
    scales = [1.0, 0.5, 0.125]
    for S, aligned, out_hw in ((1, True, (2, 3)), (2, False, (3, 2)), (3, True, (1, 1)), (4, False, (2, 2))):
        boxes = np.concatenate([PLANTED, _boxes(rng, 2 * 14 - len(PLANTED), 17, 13)]).reshape(2, 14, 4)
        count = np.array([14, 9])
        a = R.roi_align(levels, boxes, out_hw, scales, S, aligned, thr, count=count)
        b = R.roi_align_scalar(levels, boxes, out_hw, scales, S, aligned, thr, count=count)
        assert a.dtype == np.dtype(dtype) and a.shape == (28, out_hw[0], out_hw[1], 3)
        assert np.array_equal(a.view(np.uint8 if a.itemsize == 1 else np.uint32), b.view(np.uint8 if b.itemsize == 1 else np.uint32))
        assert not a[14 + 9:].any()                          # rows behind the count
        assert not a[0].any() and a[20].any()                # wholly outside; the whole map
    idx = np.array([1, -1, 0, 2, 1], dtype=np.int32)
    boxes = _boxes(rng, 5, 17, 13)
    a = R.roi_align(levels, boxes, (2, 2), scales, 2, True, thr, mode=R.LIST, batch_idx=idx)
    b = R.roi_align_scalar(levels, boxes, (2, 2), scales, 2, True, thr, mode=R.LIST, batch_idx=idx)
    assert np.array_equal(a, b, equal_nan=True) and not a[1].any() and not a[3].any() and a[0].any()


def test_f32_inf_under_a_zero_weight_is_nan():
    """a sample is left out only by its valid bits: a sample exactly on a pixel has zero weights on three corners, and an Inf
    there gives 0 * Inf = NaN"""
    m = np.ones((1, 4, 4, 1), dtype=np.float32)
    m[0, 2, 3, 0] = np.inf
    box = np.array([[[2.0, 2.0, 3.0, 3.0]]], dtype=np.float32)  # aligned, S 1: the sample is at (2, 2) exactly
    for fn in (R.roi_align, R.roi_align_scalar):
        assert np.isnan(fn([m], box, (1, 1), [1.0], 1, True)[0, 0, 0, 0])
    box[0, 0] = [0, 0, 1, 1]
    assert R.roi_align([m], box, (1, 1), [1.0], 1, True)[0, 0, 0, 0] == 1.0


@pytest.mark.parametrize("dtype", [np.uint8, np.int8, np.float32])
def test_reference_against_float64_within_the_derived_bound(dtype):
    rng = np.random.default_rng(11)
    levels = _maps(rng, dtype, 2, [(13, 17)], 4)
    vmax = float(np.abs(levels[0].astype(np.float64)).max())
    checked = 0
    for S, aligned, out_hw, scale in ((2, True, (7, 7), 1.0), (1, False, (2, 3), 0.25), (4, True, (3, 3), 1.0), (3, False, (5, 1), 0.5)):
        boxes = (_boxes(rng, 2 * 40, 17, 13) / F(scale)).reshape(2, 40, 4)
        mc = 2.0 * float(np.abs(boxes.astype(np.float64) * scale).max()) + 2.0
        out64, margin = R.roi_align_f64(levels, boxes, out_hw, [scale], S, aligned)
        assert margin > R.coord_margin(mc), "a sample sits on a validity border: choose other boxes"
        got = R.roi_align(levels, boxes, out_hw, [scale], S, aligned)
        bound = R.error_bound(S, mc, vmax)
        assert bound < 0.1                                    # (the bound means something: far below one u8 step)
        if np.dtype(dtype) == np.float32:
            assert np.abs(got.astype(np.float64) - out64).max() <= bound
        else:
            info = np.iinfo(dtype)
            want = np.clip(np.rint(out64), info.min, info.max)
            diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
            assert diff.max() <= 1
            frac = np.abs(out64 - np.floor(out64) - 0.5)      # distance of the float64 value from a rounding tie
            assert (frac[diff == 1] <= bound).all()
        checked += got.size
    assert checked > 10000


# ---- pins: the sample points are exact dyadic positions, so every product and sum is exact before the conversion --------------
@pytest.mark.parametrize("dtype", [np.uint8, np.int8, np.float32])
def test_pin_crop(dtype):
    rng = np.random.default_rng(5)
    src = _maps(rng, dtype, 2, [(13, 17)], 5)[0]
    for (x0, y0, ph, pw) in ((0, 0, 13, 17), (3, 2, 7, 7), (16, 12, 1, 1), (5, 0, 2, 3)):
        box = np.tile(np.array([x0, y0, x0 + pw, y0 + ph], dtype=np.float32), (2, 1, 1))
        got = R.roi_align([src], box, (ph, pw), [1.0], 1, True)
        assert np.array_equal(got, src[:, y0:y0 + ph, x0:x0 + pw])
        # scale 0.5 with the box doubled
        got = R.roi_align([src], box * F(2), (ph, pw), [0.5], 1, True)
        assert np.array_equal(got, src[:, y0:y0 + ph, x0:x0 + pw])


@pytest.mark.parametrize("dtype", [np.uint8, np.int8])
def test_pin_avgpool_2x2(dtype):
    rng = np.random.default_rng(6)
    src = _maps(rng, dtype, 2, [(13, 17)], 4)[0]
    for (x0, y0, ph, pw) in ((0, 0, 6, 8), (1, 1, 6, 8), (3, 2, 2, 3), (15, 11, 1, 1)):
        box = np.tile(np.array([x0, y0, x0 + 2 * pw, y0 + 2 * ph], dtype=np.float32), (2, 1, 1))
        got = R.roi_align([src], box, (ph, pw), [1.0], 2, True)
        crop = np.ascontiguousarray(src[:, y0:y0 + 2 * ph, x0:x0 + 2 * pw])
        want = refmath.avgpool(crop, (2, 2), (2, 2), (0, 0), (ph, pw), True)
        assert np.array_equal(got, want.astype(dtype))


@pytest.mark.parametrize("dtype", [np.uint8, np.int8])
def test_pin_bilinear_resize_x2(dtype):
    rng = np.random.default_rng(7)
    for (h, w) in ((5, 7), (1, 5), (5, 1), (2, 2), (13, 17)):
        src = _maps(rng, dtype, 2, [(h, w)], 3)[0]
        box = np.tile(np.array([0, 0, w, h], dtype=np.float32), (2, 1, 1))
        got = R.roi_align([src], box, (2 * h, 2 * w), [1.0], 1, True)
        want = resize_ref.resize(src, (2 * h, 2 * w), resize_ref.BILINEAR, resize_ref.HALF_PIXEL)
        assert np.array_equal(got, want)


# ---- level thresholds ----------------------------------------------------------------------------------------------------------
def test_level_thresholds_reproduce_the_level_mapper():
    thr = dfa.roi_level_thresholds(2, 5)
    assert thr.dtype == np.float32 and thr.shape == (3,) and (np.diff(thr) > 0).all()
    assert np.allclose(thr, [112.0 ** 2, 224.0 ** 2, 448.0 ** 2], rtol=1e-5)
    rng = np.random.default_rng(9)
    area = np.exp(rng.uniform(np.log(10.0), np.log(4e6), 40000)).astype(np.float32)
    far = np.all(np.abs(area[:, None].astype(np.float64) / thr[None, :].astype(np.float64) - 1.0) > 1e-4, axis=1)
    area = area[far][:10000]
    assert area.size == 10000
    want = R.level_mapper_f64(area, 2, 5)
    got = np.array([R.level_of(np.array([0, 0, a, 1], dtype=np.float32), thr) for a in area])
    assert np.array_equal(got, want) and set(got) == {0, 1, 2, 3}
    # >= at an area exactly equal to a threshold; just below it; a NaN area
    for i, t in enumerate(thr):
        assert R.level_of(np.array([0, 0, t, 1], dtype=np.float32), thr) == i + 1
        assert R.level_of(np.array([0, 0, np.nextafter(t, F(0)), 1], dtype=np.float32), thr) == i
    assert R.level_of(np.array([0, 0, np.nan, 1], dtype=np.float32), thr) == 0
    assert R.level_of(np.array([np.inf, 0, np.inf, 1], dtype=np.float32), thr) == 0   # inf - inf
    assert dfa.roi_level_thresholds(4, 4).size == 0
    other = dfa.roi_level_thresholds(3, 6, canonical_scale=160, canonical_level=5, eps=1e-3)
    a = np.array([100.0, 160.0 ** 2 * 0.26, 160.0 ** 2 * 1.1, 1e7], dtype=np.float32)
    assert np.array_equal([R.level_of(np.array([0, 0, v, 1], dtype=np.float32), other) for v in a],
                          R.level_mapper_f64(a, 3, 6, 160, 5, 1e-3))


# ---- the host plan ---------------------------------------------------------------------------------------------------------------
def _plan_check_output(exe):
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = p.stdout.decode()
    assert p.returncode == 0 and text.rstrip().endswith("roialign_plan_check: ok"), text
    return text


def test_plan_check_tool():
    text = _plan_check_output(os.path.join(TOOLS, "roialign_plan_check"))
    assert re.search(r"plan: \d{4,} descriptors, \d{5,} workgroups walked", text), text
    assert re.search(r"validation: \d{2,} refusals", text), text


def test_plan_check_tool_under_the_host_sanitizers(tmp_path):
    """ASan + UBSan on host code: built apart and run as a stand-alone program"""
    exe = str(tmp_path / "roialign_plan_check_san")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(TOOLS, "roialign_plan_check.cc")])
    _plan_check_output(exe)


# ---- the boundary ----------------------------------------------------------------------------------------------------------------
def test_ctypes_structs_match_the_header(tmp_path):
    pairs = {"dfx_roialign_desc": capi.RoiAlignDesc, "dfx_roialign_io": capi.RoiAlignIo, "dfx_roialign_info": capi.RoiAlignInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dfx.h"', 'int main(void) {']
    for cname, ct in pairs.items():
        lines.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in ct._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
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
    assert {"dfx_roialign_create", "dfx_roialign_submit", "dfx_roialign_query", "dfx_roialign_destroy",
            "dfx_debug_roialign_launches"} <= set(dfa.declared_symbols())
    assert (capi.ROIALIGN_TILE, capi.ROIALIGN_GENERIC, capi.ROI_BATCHED, capi.ROI_LIST) == (0, 1, 0, 1)


def test_validation_comes_before_the_device():
    """an invalid descriptor is DFX_ERR_INVALID (1) and adaptive sampling DFX_ERR_UNSUPPORTED (2), with or without a GPU"""
    def err(**kw):
        args = dict(bs=1, n=3, level_shapes=[(5, 5)], c=16, dtype=np.uint8, out_hw=(7, 7), spatial_scales=[1.0])
        args.update(kw)
        with pytest.raises(dfa.DfxError) as e:
            dfa.RoiAlign(**args)
        return str(e.value)
    assert "dfx error 2" in err(sampling_ratio=0)
    assert "dfx error 1" in err(sampling_ratio=5)
    assert "dfx error 1" in err(out_hw=(65, 7))
    assert "dfx error 1" in err(spatial_scales=[0.0])
    assert "dfx error 1" in err(dtype=np.int32)
    assert "dfx error 1" in err(c=20, force_path=dfa.ROIALIGN_TILE)
    assert "dfx error 1" in err(level_shapes=[(5, 5), (3, 3), (2, 2)], spatial_scales=[1, .5, .25], level_area_thr=[9.0, 4.0])
    assert "dfx error 2" in err(level_shapes=[(65535, 65535)], dtype=np.float32, c=4)
