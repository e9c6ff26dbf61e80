"""CPU-only checks of the net head (channel top-k / argmax and table softmax): the numpy reference the GPU tests compare
against (tests/head_ref.py) equals an independent pure-Python witness on the whole case table, bit for bit, and a handful of
hand-computed values; the generators plant what they promise; the C ABI validates descriptors before it touches a device,
the ctypes mirrors match the header, the symbols are exported and bound, the drop-in layer and the tools are built, and the
op's host-side plan (csrc/head_plan.h) is clean under the host sanitizers as a stand-alone program."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

import head_ref as H

dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-fusion_amd")
INVALID, UNSUPPORTED, HIP, NO_DEVICE, STATE = 1, 2, 3, 4, 5
TABLE = H.table() + [H.tie_case(255.0), H.tie_case(1.0), H.tie_case(255.0, H.F32)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _f32(*bits):
    return np.array(bits, dtype=np.uint32).view(np.float32).reshape(1, -1)


# ---- 1. independent formulations ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TABLE, ids=lambda c: c.ident())
def test_reference_equals_the_witness(case):
    assert dfa.HEAD_GENERIC == H.GENERIC                      # (the package knows the op at all)
    src = H.make_src(case)
    assert src.shape == (case.rows, case.ld) and src.dtype == H.NP_OF[case.src_dt]
    got, want = H.reference(case, src), H.witness(case, src)
    if case.mode == H.TOPK:
        assert got[0].dtype == want[0].dtype == H.NP_OF[case.dst_dt] and got[0].shape == (case.rows, case.k)
        assert got[1].dtype == want[1].dtype == H.NP_OF[case.src_dt]
        assert np.array_equal(got[0], want[0]), case.ident()
        assert np.array_equal(_bits(got[1]), _bits(want[1])), case.ident()
    else:
        assert got.dtype == want.dtype == H.NP_OF[case.dst_dt] and got.shape == (case.rows, case.c)
        assert np.array_equal(_bits(got), _bits(want)), case.ident()


def test_hand_computed_values():
    assert dfa.HEAD_TOPK == H.TOPK and dfa.HEAD_SOFTMAX == H.SOFTMAX
    # an all-equal row gives idx 0 .. k-1
    for dt in (np.uint8, np.int8, np.int32, np.float32):
        idx, val = H.reference_topk(np.full((2, 12), 7, dtype=dt), 9, 5)
        assert idx.tolist() == [[0, 1, 2, 3, 4]] * 2 and (val == 7).all()
    # -0 < +0
    idx, val = H.reference_topk(_f32(0x80000000, 0x00000000, 0x80000000), 3, 3)
    assert idx.tolist() == [[1, 0, 2]] and _bits(val).view(np.uint32).reshape(-1).tolist() == [0x00000000, 0x80000000, 0x80000000]
    # +NaN beats +Inf, -NaN loses to -Inf; payloads order the NaNs and come back verbatim
    row = _f32(0x7F800000, 0x7FC00001, 0xFF800000, 0xFFC00001, 0x7FC00002, 0x3F800000)
    idx, val = H.reference_topk(row, 6, 6)
    assert idx.tolist() == [[4, 1, 0, 5, 2, 3]]
    assert _bits(val).view(np.uint32).reshape(-1).tolist() == [0x7FC00002, 0x7FC00001, 0x7F800000, 0x3F800000, 0xFF800000, 0xFFC00001]
    # denormals order by magnitude on both sides of zero
    assert H.reference_topk(_f32(0x80000001, 0x00000001, 0x00000000, 0x80000000), 4, 4)[0].tolist() == [[1, 2, 3, 0]]
    # INT32_MIN / MAX, s8 and u8 extremes
    lo, hi = -2 ** 31, 2 ** 31 - 1
    idx, val = H.reference_topk(np.array([[lo, hi, 0, hi, lo]], dtype=np.int32), 5, 5)
    assert idx.tolist() == [[1, 3, 2, 0, 4]] and val.tolist() == [[hi, hi, 0, lo, lo]]
    assert H.reference_topk(np.array([[-128, 127, -1, 0]], dtype=np.int8), 4, 2)[0].tolist() == [[1, 3]]
    assert H.reference_topk(np.array([[128, 127, 255, 0]], dtype=np.uint8), 4, 2)[0].tolist() == [[2, 0]]
    # pad channels never take part
    assert H.reference_topk(np.array([[1, 5, 2, 9, 9]], dtype=np.uint8), 3, 1)[0].tolist() == [[1]]
    # a two-maxima row under the one-hot table: p = 0.5 at both maxima, 0 elsewhere; u8: 127.5 ties to even -> 128; 0.5 -> 0
    for scale, want in ((255.0, 128), (1.0, 0)):
        case = H.tie_case(scale)
        src = H.tie_src(case)
        p = H.reference(H.tie_case(scale, H.F32), src)
        q = H.reference(case, src)
        for r in range(case.rows):
            hot = sorted({r % case.c, (r + 16) % case.c})
            assert len(hot) == 2
            assert p[r, hot].tolist() == [0.5, 0.5] and p[r].sum() == 1.0
            assert q[r, hot].tolist() == [want, want] and int(q[r].sum()) == 2 * want
    # the table recipe: E[0] * c stays within u32 and dfa ships the same numbers
    for c in (1, 21, 150, 1000, 65535):
        e = dfa.softmax_table(0.0625, c)
        assert e.dtype == np.uint32 and e.shape == (256,) and np.array_equal(e, H.softmax_table(0.0625, c))
        assert int(e[0]) == (2 ** 32 - 1) // c and int(e.max()) * c <= 2 ** 32 - 1 and (np.diff(e.astype(np.int64)) <= 0).all()
    with pytest.raises(ValueError):
        dfa.softmax_table(0.1, 65536)
    # within 1e-6 of a float64 softmax
    case = H.HeadCase("acc", H.SOFTMAX, 8, 150, 160, H.S8, H.F32)
    src = H.generate(case)
    x = src[:, :150].astype(np.float64) * 0.0625
    ex = np.exp(x - x.max(axis=1, keepdims=True))
    assert np.abs(H.reference(case, src).astype(np.float64) - ex / ex.sum(axis=1, keepdims=True)).max() < 1e-6


# ---- 2. the generators plant what they promise ---------------------------------------------------------------------------
def test_generators_plant_what_they_promise():
    assert hasattr(dfa, "Head")
    seen_seam = 0
    for case in H.pixel_cases() + H.row_cases() + H.generic_cases():
        src = H.generate(case)
        c, per = case.c, H.seam(case.src_dt) + 1
        if case.ld > c:                                         # pad channels hold values LARGER than every valid one
            key = H.key_u32(src)
            assert (key[:, c:].min(axis=1) > key[:, :c].max(axis=1)).all(), case.ident()
        idx, _ = H.reference_topk(src, c, min(2, c))
        rows = case.rows
        assert idx[0, 0] == 0                                   # the maximum at channel 0
        if rows > 1:
            assert idx[1, 0] == c - 1 or (src[1, :c] == src[1, c - 1]).sum() > 1   # ... at c - 1
        if rows > 2 and c > per:
            assert idx[2].tolist() == [per - 1, per]            # ... twice, across the first 16-byte seam
            seen_seam += 1
        if rows > 3:
            assert (src[3, :c] == src[3, 0]).all() and idx[3].tolist() == list(range(min(2, c)))   # all equal
        if rows > 4:
            assert idx[4, 0] == (c - 1) // per * per or c > 63 * per    # the last group (or lane 63's first, if lower)
        if rows > 5 and c > 1:
            m = src[5, :c].max()
            assert (src[5, :c] == m).sum() >= 2, case.ident()   # duplicates of the maximum
    assert seen_seam > 10
    big = [c for c in H.row_cases() if c.c > 63 * 16 and c.rows > 4 and c.mode == H.TOPK and H.SIZE_OF[c.src_dt] == 1]
    assert big and all(H.reference_topk(H.generate(c), c.c, 1)[0][4, 0] == 63 * 16 for c in big)   # lane 63's first group
    t = H.table()
    assert {c.src_dt for c in t if c.mode == H.TOPK} == {H.U8, H.S8, H.S32, H.F32}
    assert {c.k for c in t} >= {1, 5, 7, 8} and {c.rows for c in t} >= {1, 3, 70, 130, 193}
    geos = {(21, 32), (19, 32), (16, 16), (1, 16), (33, 48), (64, 64), (150, 160), (161, 176)}
    px = H.pixel_cases()
    assert {(c.c, c.ld) for c in px} == geos
    # every geometry at both row counts: argmax of u8 and s8 with u8 and s32 idx; softmax of u8 and s8 to f32 and u8 with
    # dst_ld = c and dst_ld = ld
    for geo in geos:
        for rows in (70, 193):
            here = [c for c in px if (c.c, c.ld) == geo and c.rows == rows]
            assert {(c.src_dt, c.dst_dt) for c in here if c.mode == H.TOPK and c.k == 1} == {(s, i) for s in (H.U8, H.S8) for i in (H.U8, H.S32)}, geo
            assert {(c.src_dt, c.dst_dt, c.out_ld) for c in here if c.mode == H.SOFTMAX} == \
                {(s, d, o) for s in (H.U8, H.S8) for d in (H.F32, H.U8) for o in (geo[0], geo[1])}, geo
    rc = H.row_cases()
    for c in (1, 7, 15, 16, 17, 1000, 1023, 1024, 1025, 4097):
        assert {x.rows for x in rc if x.c == c and x.mode == H.TOPK} >= {1, 3, 130}, c
        assert {x.k for x in rc if x.c == c and x.mode == H.TOPK and x.rows == 130} >= {1, min(5, c), min(8, c)}, c
    for c in (1, 15, 16, 17, 1000, 1023, 1024, 1025, 4097):
        assert {x.rows for x in rc if x.c == c and x.mode == H.SOFTMAX} >= {1, 3, 130}, c
    assert {c.c for c in H.row_cases()} >= {1, 15, 16, 17, 1000, 1023, 1024, 1025, 4097, 65535}
    for path in (H.PIXEL, H.ROW, H.GENERIC):
        assert sum(H.in_class(c, path) for c in t) > 20
    assert not H.in_class(H.HeadCase("x", H.TOPK, 4, 161, 176, H.U8, H.U8), H.PIXEL)
    assert H.in_class(H.HeadCase("x", H.TOPK, 4, 150, 160, H.U8, H.U8), H.PIXEL)
    b = [c for c in t if c.table == "bound"][0]
    assert int(H.make_table(b).max()) * b.c == 2 ** 32 - 1
    for dt in (H.F32, H.S32, H.U8, H.S8):
        s = H.special_rows(dt, 20, 32)
        assert s.shape == (6, 32)
    f = H.special_rows(H.F32, 20, 32).view(np.uint32)
    assert {0x7FC00001, 0xFFC00123, 0x7F800000, 0xFF800000, 0x80000000, 0, 1, 0x80000001} <= set(f[:, :20].reshape(-1).tolist())
    K = H.HeadCase
    assert H.auto_path(K("a", H.TOPK, 70, 21, 32, H.U8, H.U8)) == H.PIXEL and H.auto_path(K("a", H.TOPK, 70, 21, 32, H.U8, H.U8, k=2)) == H.GENERIC
    assert H.auto_path(K("a", H.TOPK, 3, 1000, 1008, H.S8, H.S32, k=5)) == H.ROW and H.auto_path(K("a", H.TOPK, 3, 37, 40, H.F32, H.S32)) == H.ROW
    assert H.auto_path(K("a", H.TOPK, 3, 21, 36, H.F32, H.S32)) == H.GENERIC and H.auto_path(K("a", H.SOFTMAX, 3, 161, 176, H.S8, H.U8)) == H.ROW
    assert H.auto_path(K("a", H.SOFTMAX, 3, 21, 21, H.S8, H.U8)) == H.GENERIC
    assert H.auto_path(K("a", H.SOFTMAX, 3, 150, 160, H.S8, H.U8)) == H.ROW and H.auto_path(K("a", H.TOPK, 3, 150, 160, H.S8, H.U8)) == H.PIXEL
    assert H.auto_path(K("a", H.SOFTMAX, 3, 130, 144, H.S8, H.U8)) == H.PIXEL
    assert H.planned_grid(70, H.PIXEL) == 1 and H.planned_grid(257, H.GENERIC) == 2 and H.planned_grid(130, H.ROW) == 33
    assert H.planned_grid(10 ** 9, H.ROW) == 2048 and H.planned_grid(10 ** 9, H.PIXEL, 1) == 1


# ---- 3. the plan under the host sanitizers -------------------------------------------------------------------------------
def test_head_plan_check_is_clean_under_the_host_sanitizers(tmp_path):
    """tools/head_plan_check.cc, a stand-alone host program over csrc/head_plan.h, built with the flags of the host
    Makefile's SAN=1 rule (ASan + UBSan) into a scratch directory and run directly.  Nothing is loaded into Python."""
    src = os.path.join(PKG, "tools", "head_plan_check.cc")
    assert os.path.exists(src), "tools/head_plan_check.cc is missing"
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert "$(TOOLS)/head_plan_check: $(TOOLS)/head_plan_check.cc ../csrc/head_plan.h" in mk
    exe = tmp_path / "head_plan_check"
    flags = ["-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++"] + flags + [src, "-o", str(exe)])
    p = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()
    assert "head plans: validation, classes, table bounds, grids and the 2^40 limit hold" in p.stdout.decode()


# ---- 4. descriptor and build checks -------------------------------------------------------------------------------------
def _desc(**kw):
    d = dict(rows=70, mode=capi.HEAD_TOPK, src_dt=capi.DFX_U8, dst_dt=capi.DFX_U8, c=21, src_ld=32, dst_ld=21, idx_ld=0, k=1,
             out_scale=255.0, force_path=capi.HEAD_AUTO)
    d.update(kw)
    if d["idx_ld"] == 0:
        d["idx_ld"] = max(d["k"], 1)
    desc = capi.HeadDesc()
    for k, v in d.items():
        setattr(desc, k, v)
    return desc


def _create(**kw):
    desc = _desc(**kw)
    h = ctypes.c_void_p()
    rc = capi.lib().dfx_head_create(ctypes.byref(desc), ctypes.byref(h))
    msg = capi.lib().dfx_last_error().decode()
    if rc == 0:
        assert capi.lib().dfx_head_destroy(h) == 0
    else:
        assert not h.value
    return rc, msg


def _admitted(**kw):
    rc, msg = _create(**kw)
    assert rc in (0, NO_DEVICE), (kw, rc, msg)


SOFTMAX = dict(mode=capi.HEAD_SOFTMAX, dst_dt=capi.DFX_F32)


def test_descriptor_validation_needs_no_device():
    for kw, word in ((dict(k=0), "k"), (dict(k=9), "k"), (dict(k=8, c=7, src_ld=16), "k above c"), (dict(c=257, src_ld=272), "u8 idx"),
                     (dict(c=0), "c must"), (dict(c=65536, src_ld=65536, dst_dt=capi.DFX_S32), "65535"), (dict(src_ld=20), "src_ld"),
                     (dict(force_path=3), "force_path"), (dict(force_path=-2), "force_path"), (dict(rows=0), "rows"),
                     (dict(mode=2), "mode"), (dict(k=3, idx_ld=2), "idx_ld"), (dict(src_dt=0), "src dtype"), (dict(dst_dt=capi.DFX_F32), "idx")):
        rc, msg = _create(**kw)
        assert rc == INVALID and word in msg, (kw, rc, msg)
    for kw in (dict(k=8), dict(k=8, c=8, src_ld=8), dict(c=256, src_ld=256), dict(c=257, src_ld=272, dst_dt=capi.DFX_S32),
               dict(c=65535, src_ld=65535, dst_dt=capi.DFX_S32, k=8), dict(src_ld=21), dict(src_dt=capi.DFX_F32, k=5, dst_dt=capi.DFX_S32)):
        _admitted(**kw)
    # softmax: 1-byte src only; dst f32 or u8; dst_ld >= c; a finite out_scale for u8
    rc, msg = _create(src_dt=capi.DFX_S32, **SOFTMAX)
    assert rc == UNSUPPORTED and "reorder" in msg, (rc, msg)
    assert _create(src_dt=capi.DFX_F32, **SOFTMAX)[0] == UNSUPPORTED
    assert _create(src_dt=capi.DFX_S32, src_ld=20, **SOFTMAX)[0] == INVALID          # invalid is reported before unsupported
    assert _create(mode=capi.HEAD_SOFTMAX, dst_dt=capi.DFX_S32)[0] == INVALID
    assert _create(dst_ld=20, **SOFTMAX)[0] == INVALID
    assert _create(mode=capi.HEAD_SOFTMAX, dst_dt=capi.DFX_U8, out_scale=float("inf"))[0] == INVALID
    assert _create(mode=capi.HEAD_SOFTMAX, dst_dt=capi.DFX_U8, out_scale=float("nan"))[0] == INVALID
    _admitted(**SOFTMAX)
    _admitted(mode=capi.HEAD_SOFTMAX, dst_dt=capi.DFX_U8, src_dt=capi.DFX_S8, dst_ld=32)
    _admitted(k=0, **SOFTMAX)                                                       # k is ignored
    # rows * max(src_ld, out_ld) <= 2^40
    _admitted(rows=2 ** 35)
    rc, msg = _create(rows=2 ** 35 + 1)
    assert rc == INVALID and "2^40" in msg, (rc, msg)
    assert _create(rows=2 ** 35, dst_ld=64, **SOFTMAX)[0] == INVALID
    # a forced path outside its class
    for kw in (dict(force_path=capi.HEAD_PIXEL, k=2, c=21), dict(force_path=capi.HEAD_PIXEL, src_ld=176, c=161),
               dict(force_path=capi.HEAD_PIXEL, src_ld=24), dict(force_path=capi.HEAD_PIXEL, src_dt=capi.DFX_S32, dst_dt=capi.DFX_S32),
               dict(force_path=capi.HEAD_ROW, src_ld=21), dict(force_path=capi.HEAD_ROW, src_dt=capi.DFX_F32, src_ld=22, dst_dt=capi.DFX_S32)):
        rc, msg = _create(**kw)
        assert rc == UNSUPPORTED and "class" in msg, (kw, rc, msg)
        kw["force_path"] = capi.HEAD_GENERIC
        _admitted(**kw)
    for kw in (dict(force_path=capi.HEAD_PIXEL), dict(force_path=capi.HEAD_PIXEL, src_ld=160, c=150), dict(force_path=capi.HEAD_ROW, k=8),
               dict(force_path=capi.HEAD_PIXEL, **SOFTMAX), dict(force_path=capi.HEAD_ROW, src_dt=capi.DFX_F32, src_ld=24, dst_dt=capi.DFX_S32)):
        _admitted(**kw)
    lib = capi.lib()
    assert lib.dfx_head_create(None, None) == INVALID
    assert lib.dfx_head_set_table(None, None) == INVALID
    assert lib.dfx_head_submit(None, None, None, None, None) == INVALID
    assert lib.dfx_head_query(None, None) == INVALID
    assert lib.dfx_debug_head_launches(None) == INVALID
    assert lib.dfx_head_destroy(None) == 0
    assert "null" in lib.dfx_last_error().decode()


def test_valid_descriptors_and_no_cpu_fallback():
    import torch
    for kw in (dict(), dict(k=5, src_dt=capi.DFX_S8, dst_dt=capi.DFX_S32, c=1000, src_ld=1008), dict(**SOFTMAX)):
        rc, msg = _create(**kw)
        if torch.cuda.is_available():
            assert rc == 0, (kw, msg)
        else:
            assert rc == NO_DEVICE and "no HIP device" in msg, (kw, rc, msg)
    if not torch.cuda.is_available():
        with pytest.raises(dfa.DfxError) as e:
            dfa.TopK(70, 21, np.uint8, np.uint8, src_ld=32)
        assert "dfx error 4" in str(e.value) and "no HIP device" in str(e.value)
        with pytest.raises(dfa.DfxError):
            dfa.Softmax(70, 21, np.int8, np.float32, src_ld=32, table=dfa.softmax_table(0.1, 21))


def test_head_structs_match_the_header(tmp_path):
    """dfx_head_desc / dfx_head_info compiled by gcc have the sizes and field offsets of the ctypes mirrors"""
    pairs = {"dfx_head_desc": capi.HeadDesc, "dfx_head_info": capi.HeadInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dfx.h"', 'int main(void) {']
    for cname, ct in pairs.items():
        lines.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in ct._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    enums = ("DFX_HEAD_TOPK", "DFX_HEAD_SOFTMAX", "DFX_HEAD_PIXEL", "DFX_HEAD_ROW", "DFX_HEAD_GENERIC", "DFX_HEAD_MAX_K", "DFX_HEAD_MAX_C",
             "DFX_VERSION")
    for name in enums:
        lines.append('printf("enum %s %%d\\n", %s);' % (name, name))
    lines.append('printf("dfx_wsum_desc size %zu\\n", sizeof(dfx_wsum_desc));')
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
    assert [n for n, _ in capi.HeadDesc._fields_] == ["rows", "mode", "src_dt", "dst_dt", "c", "src_ld", "dst_ld", "idx_ld", "k", "out_scale",
                                                      "force_path"]
    assert [n for n, _ in capi.HeadInfo._fields_] == ["path", "grid", "block", "lds_bytes", "device", "algorithmic_bytes", "kernel_name"]
    assert seen[("enum", "DFX_HEAD_TOPK")] == capi.HEAD_TOPK == H.TOPK == 0 and seen[("enum", "DFX_HEAD_SOFTMAX")] == capi.HEAD_SOFTMAX == H.SOFTMAX == 1
    assert seen[("enum", "DFX_HEAD_PIXEL")] == capi.HEAD_PIXEL == H.PIXEL == 0 and seen[("enum", "DFX_HEAD_ROW")] == capi.HEAD_ROW == H.ROW == 1
    assert seen[("enum", "DFX_HEAD_GENERIC")] == capi.HEAD_GENERIC == H.GENERIC == 2 and capi.HEAD_AUTO == -1
    assert seen[("enum", "DFX_HEAD_MAX_K")] == 8 and seen[("enum", "DFX_HEAD_MAX_C")] == 65535 and seen[("enum", "DFX_VERSION")] == 100
    assert ctypes.sizeof(capi.HeadDesc) == 48
    assert ctypes.sizeof(capi.WsumDesc) == seen[("dfx_wsum_desc", "size")]            # the others are untouched


def test_library_exports_the_head_entry_points():
    L = capi.lib()
    for s in ("dfx_head_create", "dfx_head_set_table", "dfx_head_submit", "dfx_head_query", "dfx_head_destroy", "dfx_debug_head_launches"):
        assert s in dfa.declared_symbols() and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s                                # bound with a signature
    assert not [s for s in dfa.declared_symbols() if not hasattr(L, s)]
    for name in ("Head", "TopK", "Softmax", "HeadDesc", "HeadInfo", "HEAD_AUTO", "HEAD_PIXEL", "HEAD_ROW", "HEAD_GENERIC", "HEAD_TOPK",
                 "HEAD_SOFTMAX", "softmax_table", "head_launches"):
        assert hasattr(dfa, name), name
    capi.set_tuning("DFX_HEAD_GRID", "1")                                           # known to the library
    capi.set_tuning("DFX_HEAD_GRID", None)
    with pytest.raises(dfa.DfxError):
        capi.set_tuning("DFX_HEAD_ROWS", "1")


def test_dropin_layer_exports_the_head_ops_and_tools_are_built():
    so = os.path.join(PKG, "libdeepfusion.so")
    assert os.path.exists(so), "run __graft_entry__.build() first"
    syms = subprocess.check_output(["nm", "-D", "-C", "--defined-only", so]).decode()
    for fn in ("deepfusion::argmax(", "deepfusion::top_k(", "deepfusion::softmax("):
        assert fn in syms, fn
    for tool in ("head_check", "head_plan_check", "bench_head"):
        exe = os.path.join(PKG, "tools", tool)
        assert os.path.exists(exe) and os.access(exe, os.X_OK), tool
    p = subprocess.run([os.path.join(PKG, "tools", "head_plan_check")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0 and "the 2^40 limit hold" in p.stdout.decode(), p.stdout.decode()
    ignore = open(os.path.join(ROOT, ".gitignore")).read().split()
    for tool in ("head_check", "head_plan_check", "bench_head"):
        assert "deep-fusion_amd/tools/" + tool in ignore, tool
    # the trace stub knows the new C-ABI calls: coherence_check links against it
    stub = open(os.path.join(PKG, "tools", "dfx_trace_stub.cc")).read()
    for s in ("dfx_head_create", "dfx_head_set_table", "dfx_head_submit", "dfx_head_destroy"):
        assert "int %s(" % s in stub, s
