"""CPU-only checks of the image-wide top-K (dfx_select_*): the numpy reference of tests/select_ref.py against a pure-Python
witness (loops and sorted() on tuples), the regimes the case tables are meant to hold, the host plan of csrc/select_plan.h
(tools/select_plan_check, a plain host program) against the Python mirror, the ctypes structs against the header, and the
order of the validation: everything invalid is refused before a device is asked for."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import select_ref as S

dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "deep-fusion_amd", "tools")


# ---- the witness -----------------------------------------------------------------------------------------------------------
def witness(case, src, k):
    """idx, val, count as nested lists, by the definition of include/dfx.h read literally"""
    idx, val, count = [], [], []
    mv = S.min_val_of(case)
    for r in range(case.bs):
        img = src[r].tolist()
        cand = []
        for y in range(case.h):
            for x in range(case.w):
                for ch in range(case.c):
                    v = img[y][x][ch]
                    if v < mv:
                        continue
                    if case.peak == S.PEAK3 and any(
                            img[y + dy][x + dx][ch] > v for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                            if 0 <= y + dy < case.h and 0 <= x + dx < case.w):
                        continue
                    cand.append((-v, (y * case.w + x) * case.c + ch))
        best = sorted(cand)[:k]
        count.append(len(best))
        idx.append([e for _, e in best] + [-1] * (k - len(best)))
        val.append([-v for v, _ in best] + [0] * (k - len(best)))
    return idx, val, count, [len(cand)]


def planted_cases():
    K = S.SelectCase
    return [K("equal", 2, 5, 7, 3, 16, S.U8, S.PEAK3, None, "equal"), K("two", 2, 6, 8, 2, 16, S.S8, S.ALL, None, "two"),
            K("plateau", 2, 9, 11, 3, 16, S.U8, S.PEAK3, None, "plateau", 3), K("extremes", 2, 5, 7, 4, 16, S.S8, S.PEAK3, None, "extremes"),
            K("extremes", 2, 5, 7, 4, 16, S.U8, S.ALL, 255, "extremes"), K("count", 2, 4, 5, 3, 16, S.U8, S.ALL, 255, "count17")]


def test_reference_matches_the_pure_python_witness():
    maps = [c for i, c in enumerate(S.table_maps()) if c.h * c.w * c.c <= 3000 or i % 7 == 0] + planted_cases()
    assert len(maps) > 200
    for case in maps:
        src, order = S.problem(case)
        n0 = len(order[0])
        for k in {1, 7, max(1, n0 - 1), n0 + 1}:
            idx, val, count = S.reference(case, src, k, order)[:3]
            widx, wval, wcount, _ = witness(case, src, k)
            assert idx.tolist() == widx and val.tolist() == wval and count.tolist() == wcount, S.ident(case, k)
            assert idx.dtype == np.int32 and count.dtype == np.int32 and val.dtype == S.NP_OF[case.dt]


def test_the_pad_channels_never_take_part():
    """the pad channels hold the dtype's maximum: were they read, they would be the best candidates everywhere"""
    for case in S.table_maps():
        src = S.problem(case)[0]
        if case.ld > case.c:
            assert (src[..., case.c:] == S.DT_MAX[case.dt]).all()
        assert (src[..., :case.c].astype(np.int32) < S.DT_MAX[case.dt]).all()


def test_gather_reference():
    case = S.SelectCase("g", 2, 5, 7, 3, 16, S.U8, S.PEAK3)
    src, order = S.problem(case)
    rng = np.random.default_rng(5)
    g = rng.integers(0, 256, (2, 5, 7, 12), dtype=np.uint8)
    k = len(order[0]) + 2
    idx, _, count, rows = S.reference(case, src, k, order, [g], [(8, 12)])
    for r in range(2):
        for j in range(k):
            if j < count[r]:
                p = idx[r, j] // case.c
                assert rows[r, j].tolist() == g[r, p // 7, p % 7, :8].tolist()
            else:
                assert not rows[r, j].any() and idx[r, j] == -1


# ---- the regimes of the table ----------------------------------------------------------------------------------------------
def test_the_table_holds_every_regime():
    """per map and k the regime of every image -- no candidate, fewer than k, exactly k, k + 1, more -- is what the case
    is meant to have; all five occur, under both peak modes, both dtypes and on both kernel classes"""
    maps = S.table_maps()
    assert len(maps) == 5 * 6 * 2 * 2 * 3
    seen = set()
    for case in maps:
        _, order = S.problem(case)
        counts = [len(o) for o in order]
        n0 = counts[0]
        if case.min_val == S.DT_MAX[case.dt]:
            assert counts == [0] * case.bs, S.ident(case)          # above every element
        elif case.min_val is None and case.peak == S.ALL:
            assert counts == [case.h * case.w * case.c] * case.bs   # all
        elif case.min_val is None:
            assert all(1 <= n <= case.h * case.w * case.c for n in counts)  # every channel of an image has a maximum
        ks = S.table_ks(n0)
        assert set(S.FIXED_K) <= set(ks)
        for k in ks:
            meant = {n0: "equal", n0 - 1: "plus1", n0 + 1: "fewer"}.get(k) if n0 else "zero"
            got = S.regime(n0, k)
            if meant:
                assert got == meant, S.ident(case, k)
            for n in counts:
                seen.add((S.regime(n, k), case.peak, case.dt, S.hist_class(case)))
    for reg in S.REGIMES:
        for peak in (S.ALL, S.PEAK3):
            for dt in (S.U8, S.S8):
                for hist in (False, True):
                    assert (reg, peak, dt, hist) in seen, (reg, peak, dt, hist)


def test_threshold_mirror_against_a_sort():
    rng = np.random.default_rng(3)
    for trial in range(300):
        total = np.zeros(256, dtype=np.int64)
        for b in rng.integers(0, 256, 6):
            total[b] += rng.integers(0, 5)
        keys = sorted(np.repeat(np.arange(256), total).tolist(), reverse=True)
        for k in (1, 3, len(keys), len(keys) + 1, 4096):
            if k < 1:
                continue
            t, n_gt, quota, count = S.threshold(total.tolist(), k)
            taken = keys[:k]
            assert count == len(taken) and n_gt + quota == count
            if taken:
                assert t == taken[-1] and n_gt == sum(1 for x in taken if x > t)
            else:
                assert (t, n_gt, quota) == (0, 0, 0)


# ---- the host plan -----------------------------------------------------------------------------------------------------------
def test_plan_check_tool_matches_the_python_mirror():
    """tools/select_plan_check (plain host C++ over csrc/select_plan.h): the scan against a brute-force sort, the validation,
    and one printed plan per point of select_ref.plan_points(), equal to the mirror"""
    p = subprocess.run([os.path.join(TOOLS, "select_plan_check")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    text = p.stdout.decode()
    assert p.returncode == 0 and text.rstrip().endswith("select_plan_check: ok"), text
    assert re.search(r"scan: \d{4,} cases against the brute-force sort", text), text
    got = []
    for ln in text.splitlines():
        m = re.match(r"plan bs=(\d+) px=(\d+) ld=(\d+) cus=(\d+) forced=(\d+) : chunk_px=(\d+) chunks=(\d+) items=(\d+) grid=(\d+) scratch=(\d+)$", ln)
        if m:
            got.append(tuple(int(v) for v in m.groups()))
    want = []
    for bs, px, ld, cus, forced in S.plan_points():
        pl = S.plan(bs, px, ld, cus, forced)
        want.append((bs, px, ld, cus, forced, pl.chunk_px, pl.chunks, pl.items, pl.grid, S.scratch_bytes(bs, pl.chunks, 100)))
    assert got == want
    assert "lds hist=%d generic=%d launches hist=%d generic=%d" % (S.lds_bytes(S.HIST), S.lds_bytes(S.GENERIC), S.launches(S.HIST),
                                                                    S.launches(S.GENERIC)) in text
    # the points hold every 16-byte shape of the table under the three chunk settings
    for case in S.table_maps():
        if S.hist_class(case):
            for forced in S.chunk_settings(case):
                assert (case.bs, case.h * case.w, case.ld, 256, forced or 0) in [w[:5] for w in want]


def test_chunk_settings_cut_the_table_as_meant():
    """1 pixel per chunk: every 3x3 window crosses chunks; two rows minus a pixel: chunk borders fall inside rows and a
    window spans up to three chunks; with 13x16 and k up to 4096 a tie bin spans many chunks"""
    for case in S.table_maps():
        px = case.h * case.w
        one, rows2, _ = S.chunk_settings(case)
        assert S.plan(case.bs, px, case.ld, 256, one).chunks == px
        pl = S.plan(case.bs, px, case.ld, 256, rows2)
        assert pl.chunk_px == min(px, 2 * case.w - 1)
        if case.h >= 5 and case.w > 1:
            assert pl.chunks >= 3 and pl.chunk_px % case.w != 0


# ---- the binding ---------------------------------------------------------------------------------------------------------------
def test_ctypes_structs_match_the_header(tmp_path):
    pairs = {"dfx_select_desc": capi.SelectDesc, "dfx_select_info": capi.SelectInfo}
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
    assert (capi.SELECT_MAX_K, capi.SELECT_MAX_GATHER) == (4096, 4)


def test_symbols_are_declared_and_exported():
    syms = dfa.declared_symbols()
    for s in ("dfx_select_create", "dfx_select_submit", "dfx_select_query", "dfx_select_destroy", "dfx_debug_select_launches"):
        assert s in syms and hasattr(dfa.lib(), s), s
    assert all(v >= 0 for v in dfa.select_launches())
    capi.set_tuning("DFX_SELECT_CHUNK", "1")                                        # known to the library
    capi.set_tuning("DFX_SELECT_CHUNK", None)


def _error(**kw):
    args = dict(bs=2, h=5, w=7, c=21, src_dtype=np.uint8, k=100, src_ld=32)
    args.update(kw)
    with pytest.raises(dfa.DfxError) as e:
        dfa.SelectTopK(**args)
    return str(e.value)


def test_validation_comes_before_the_device():
    """DFX_ERR_INVALID (1) and DFX_ERR_UNSUPPORTED (2) are reported with or without a GPU; "no HIP device" only for a valid
    descriptor"""
    for kw in (dict(bs=0), dict(h=0), dict(c=0), dict(c=33), dict(src_ld=65536, c=1), dict(k=0), dict(k=4097), dict(idx_ld=99),
               dict(peak=2), dict(force_path=2), dict(min_val=256), dict(min_val=-1), dict(src_dtype=np.int8, min_val=128),
               dict(src_dtype=9), dict(h=65536, w=32768, c=1, src_ld=1), dict(bs=3, h=32768, w=32768, c=1, src_ld=512),
               dict(gather=[(8, 8)] * 5), dict(gather=[(0, 8)]), dict(gather=[(1025, 2048)]), dict(gather=[(8, 7)]),
               dict(src_dtype=np.float32, k=0)):
        assert "dfx error 1" in _error(**kw), kw
    for kw in (dict(src_dtype=np.int32), dict(src_dtype=np.float32), dict(src_ld=21, force_path=dfa.SELECT_HIST),
               dict(c=5, src_ld=7, force_path=dfa.SELECT_HIST)):
        assert "dfx error 2" in _error(**kw), kw
    assert "radix" in _error(src_dtype=np.float32)
    import torch
    if not torch.cuda.is_available():
        assert "no HIP device" in _error()
        assert "no HIP device" in _error(src_ld=21)
