"""CPU-only checks of the box decode + greedy NMS (dfx_nms_*): the numpy reference of tests/nms_ref.py against a pure-Python
witness (loops over np.float32 scalars) and against exact rational arithmetic on grid-aligned boxes, box_tables against
float64, the host plan of csrc/nms_plan.h (tools/nms_plan_check, a plain host program, also under the host sanitizers)
against the Python mirror, the ctypes structs against the header, the order of the validation, and the regimes the GPU case
tables are meant to hold."""
import ctypes
import importlib
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import nms_ref as S

dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "deep-fusion_amd", "tools")
F = np.float32


# ---- the witnesses -----------------------------------------------------------------------------------------------------------
def w_suppresses(a, b, thr):
    """the definition of include/dfx.h read literally, on np.float32 scalars; a is the box of the lower position"""
    with np.errstate(all="ignore"):
        area_a = (a[2] - a[0]) * (a[3] - a[1])
        area_b = (b[2] - b[0]) * (b[3] - b[1])
        xx1 = a[0] if a[0] > b[0] else b[0]
        yy1 = a[1] if a[1] > b[1] else b[1]
        xx2 = a[2] if a[2] < b[2] else b[2]
        yy2 = a[3] if a[3] < b[3] else b[3]
        w = xx2 - xx1
        w = w if w > F(0) else F(0)
        h = yy2 - yy1
        h = h if h > F(0) else F(0)
        inter = w * h
        u = (area_a + area_b) - inter
        q = inter / u
        assert all(type(v) is F for v in (area_a, w, h, inter, u, q))
        return bool(q > F(thr))


def w_decode(e, row, anchors, tab_c, tab_s, classes, apx, clip):
    g = e // classes
    a = g % apx
    q = [int(row[4 * a + i]) for i in range(4)]
    ax1, ay1, ax2, ay2 = (anchors[g, i] for i in range(4))
    half = F(0.5)
    with np.errstate(all="ignore"):
        aw, ah = ax2 - ax1, ay2 - ay1
        acx, acy = ax1 + half * aw, ay1 + half * ah
        cx, cy = acx + tab_c[q[0]] * aw, acy + tab_c[q[1]] * ah
        w, hh = aw * tab_s[q[2]], ah * tab_s[q[3]]
        box = [cx - half * w, cy - half * hh, cx + half * w, cy + half * hh]
    if clip is not None and clip[0] > 0:
        for i, hi in ((0, clip[0]), (2, clip[0]), (1, clip[1]), (3, clip[1])):
            x = box[i]
            x = F(0) if x < F(0) else x
            box[i] = F(hi) if x > F(hi) else x
    assert all(type(v) is F for v in box)
    return box


def witness(case, max_out, boxes=None, idx=None, deltas=None, anchors=None, tabs=None, count_in=None, over=w_suppresses):
    keeps, boxes_of = [], []
    for r, nv in enumerate(S.n_valid(count_in, case.bs, case.n)):
        bx, lab = [], []
        for j in range(case.n):
            e = int(idx[r, j]) if (case.mode == S.DECODE or case.per_class) else 0
            ok = 0 <= e < S.n_anchors_of(case) * case.classes
            lab.append(-1 if not ok else e % case.classes if case.per_class else 0)
            if case.mode == S.BOXES:
                bx.append([boxes[r, j, i] for i in range(4)])
            else:
                bx.append(w_decode(e, deltas[r, j], anchors, tabs[0], tabs[1], case.classes, case.apx, case.clip) if ok else [F(0)] * 4)
        keep = []
        for j in range(nv):
            if len(keep) == max_out:
                break
            if lab[j] < 0:
                continue
            if not any(lab[i] == lab[j] and over(bx[i], bx[j], case.thr) for i in keep):
                keep.append(j)
        keeps.append(keep)
        boxes_of.append(bx)
    return keeps, boxes_of


def assert_same(case, max_out, ref, wit):
    keep, count, bout, dec = ref
    keeps, boxes_of = wit
    for r in range(case.bs):
        k = keeps[r]
        assert count[r] == len(k) and keep[r].tolist() == k + [-1] * (max_out - len(k)), S.ident(case, max_out)
        for o, j in enumerate(k):
            assert [v.view(np.uint32) for v in bout[r, o]] == [F(v).view(np.uint32) for v in boxes_of[r][j]], (S.ident(case), r, j)
        assert not bout[r, len(k):].any()


def test_reference_matches_the_pure_python_witness():
    n_cases = 0
    for pc, classes, thr in S.RANDOM:
        case, boxes, idx = S.random_problem(pc, classes, thr, n=90)
        for max_out in (1, 17, 90):
            for count_in in (None, np.array([70, 0], dtype=np.int32)):
                assert_same(case, max_out, S.reference(case, max_out, boxes=boxes, idx=idx, count_in=count_in),
                            witness(case, max_out, boxes=boxes, idx=idx, count_in=count_in))
                n_cases += 1
    for name in S.PLANTED:
        boxes, thr = S.planted(name)
        case = S.NmsCase(name, 1, boxes.shape[1], S.BOXES, 0, 1, 1, None, None, thr)
        assert_same(case, case.n, S.reference(case, case.n, boxes=boxes), witness(case, case.n, boxes=boxes))
        n_cases += 1
    for dt, apx, classes, clip in S.DECODES[::3]:
        case, idx, deltas, anchors, tabs = S.decode_case(dt, apx, classes, clip, 0.5, n=140)
        ref = S.reference(case, 100, idx=idx, deltas=deltas, anchors=anchors, tabs=tabs)
        wit = witness(case, 100, idx=idx, deltas=deltas, anchors=anchors, tabs=tabs)
        assert_same(case, 100, ref, wit)
        for r in range(case.bs):   # every decoded box, kept or not
            assert ref[3][r].view(np.uint32).tolist() == [[F(v).view(np.uint32) for v in b] for b in wit[1][r]]
        n_cases += 1
    assert n_cases > 40


def test_grid_aligned_boxes_against_exact_arithmetic():
    """coordinates multiples of 1/4 below 2^10: differences, products (at most 24 bits) and sums before the division are exact
    in f32, and inter / u > thr is decided exactly: rounding to nearest is monotonic and thr is itself an f32, so
    fl(inter / u) > thr iff inter / u > thr, unless inter / u rounds down onto thr -- which needs thr < inter / u < thr + ulp
    and is looked for explicitly (no such pair may be among the cases)"""
    rng = np.random.default_rng(8)
    hits = 0
    for thr in (0.25, 0.5, 0.7):
        t = Fraction(float(F(thr)))
        boxes = S.grid_aligned_boxes(rng, 120, extent=20)[None]   # dense: many overlaps
        # plant exact ties and near ties: IoU exactly 1/4, 1/2
        boxes[0, 0], boxes[0, 1], boxes[0, 2] = [0, 0, 2, 2], [0, 0, 2, 1], [0, 0, 1, 1]
        assert (boxes * 4 == np.round(boxes * 4)).all() and np.abs(boxes).max() < 1024

        def exact(a, b, thr_):
            fa, fb = [Fraction(float(v)) for v in a], [Fraction(float(v)) for v in b]
            w = max(Fraction(0), min(fa[2], fb[2]) - max(fa[0], fb[0]))
            h = max(Fraction(0), min(fa[3], fb[3]) - max(fa[1], fb[1]))
            inter = w * h
            u = (fa[2] - fa[0]) * (fa[3] - fa[1]) + (fb[2] - fb[0]) * (fb[3] - fb[1]) - inter
            if u == 0:
                return False   # 0 / 0
            q = inter / u
            up = Fraction(float(np.nextafter(F(thr_), F(2))))
            assert not (t < q < up), "a quotient strictly between thr and the next float: not decidable this way"
            return q > t

        case = S.NmsCase("grid", 1, boxes.shape[1], S.BOXES, 0, 1, 1, None, None, thr)
        ref = S.reference(case, case.n, boxes=boxes)
        wit = witness(case, case.n, boxes=boxes, over=exact)
        assert ref[0][0, :ref[1][0]].tolist() == wit[0][0]
        hits += case.n - len(wit[0][0])
    assert hits > 30   # suppressions did happen


def test_box_tables_against_float64():
    for dt, zp in ((np.uint8, 128), (np.uint8, 0), (np.int8, 0), (np.int8, -3)):
        for scale, wxy, wwh in ((1 / 32, 10.0, 5.0), (0.1, 1.0, 1.0), (0.05, 10.0, 5.0)):
            tc, ts = dfa.box_tables(scale, zp, wxy, wwh, dtype=dt)
            assert tc.dtype == F and ts.dtype == F and tc.shape == ts.shape == (256,)
            for raw in range(256):
                q = raw if dt == np.uint8 else (raw - 256 if raw >= 128 else raw)
                d = (q - zp) * scale
                assert tc[raw] == F(d / wxy), (dt, raw)
                assert ts[raw] == F(math.exp(min(d / wwh, math.log(1000.0 / 16)))), (dt, raw)
    assert dfa.box_tables(1.0, 0, 1.0, 1.0)[1].max() == F(1000.0 / 16)          # the clip of torchvision's BoxCoder
    assert dfa.box_tables(1.0, 0, 1.0, 1.0, clip=1.0)[1].max() == F(math.e)


# ---- the host plan -------------------------------------------------------------------------------------------------------------
def _plan_check_output(exe):
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = p.stdout.decode()
    assert p.returncode == 0 and text.rstrip().endswith("nms_plan_check: ok"), text
    return text


def test_plan_check_tool_matches_the_python_mirror():
    text = _plan_check_output(os.path.join(TOOLS, "nms_plan_check"))
    assert re.search(r"scan: \d{4,} cases against the brute-force greedy walk", text), text
    assert "tiles: ok" in text and re.search(r"validation: \d{2,} refusals", text), text
    got = []
    for ln in text.splitlines():
        m = re.match(r"plan bs=(\d+) n=(\d+) : blocks=(\d+) tiles=(\d+) prep=(\d+) mask=(\d+) scan=(\d+) scratch=(\d+)$", ln)
        if m:
            got.append(tuple(int(v) for v in m.groups()))
    want = [(bs, n, S.blocks(n), S.tiles(n), S.prep_grid(bs, n), S.mask_grid(bs, n), bs, S.scratch_bytes(bs, n)) for bs, n in S.plan_points()]
    assert got == want
    assert "lds mask=%d generic=%d launches mask=%d generic=%d auto_min_n=%d auto_min_out=%d" % (
        S.lds_bytes(S.MASK), S.lds_bytes(S.GENERIC), S.launches(S.MASK), S.launches(S.GENERIC), S.MASK_AUTO_MIN_N, S.MASK_AUTO_MIN_OUT) in text
    assert {n for _, n in S.plan_points()} >= {1, 63, 64, 65, 128, 130, 1000, 4096}


def test_plan_check_tool_under_the_host_sanitizers(tmp_path):
    """the SAN=1 build of host/Makefile (ASan + UBSan on host code), built apart and run as a program"""
    exe = str(tmp_path / "nms_plan_check_san")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(TOOLS, "nms_plan_check.cc")])
    _plan_check_output(exe)


def test_block_scan_mirror_against_brute_force():
    rng = np.random.default_rng(2)
    for trial in range(400):
        den = int(rng.integers(2, 30))
        diag = [sum(1 << c for c in range(t + 1, 64) if rng.integers(0, den) == 0) for t in range(64)]
        cand = int(rng.integers(0, 2 ** 63)) * 2 + int(rng.integers(0, 2)) if trial % 5 else [0, 2 ** 64 - 1][trial % 2]
        for budget in (1, 5, 64):
            kept, rem = [], 0
            for t in range(64):
                if len(kept) < budget and cand >> t & 1 and not rem >> t & 1:
                    kept.append(t)
                    rem |= diag[t]
            assert S.block_scan(diag, cand, budget) == sum(1 << t for t in kept)
    assert S.enumerate_tiles(130) == [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


# ---- the binding ---------------------------------------------------------------------------------------------------------------
def test_ctypes_structs_match_the_header(tmp_path):
    pairs = {"dfx_nms_desc": capi.NmsDesc, "dfx_nms_io": capi.NmsIo, "dfx_nms_info": capi.NmsInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dfx.h"', 'int main(void) {']
    for cname, ct in pairs.items():
        lines.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in ct._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines.append('printf("enum mask %d\\n", DFX_NMS_MASK); printf("enum generic %d\\n", DFX_NMS_GENERIC);')
    lines.append('printf("enum decode %d\\n", DFX_NMS_DECODE); printf("enum max_n %d\\n", DFX_NMS_MAX_N);')
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
    assert (seen[("enum", "mask")], seen[("enum", "generic")], seen[("enum", "decode")], seen[("enum", "max_n")]) == (
        capi.NMS_MASK, capi.NMS_GENERIC, capi.NMS_DECODE, capi.NMS_MAX_N)


def test_symbols_are_declared_and_exported():
    syms = dfa.declared_symbols()
    for s in ("dfx_nms_create", "dfx_nms_submit", "dfx_nms_query", "dfx_nms_destroy", "dfx_debug_nms_launches"):
        assert s in syms and hasattr(dfa.lib(), s), s
    assert all(v >= 0 for v in dfa.nms_launches())


def _error(**kw):
    args = dict(bs=2, n=100, max_out=50, iou_thr=0.5, mode=dfa.NMS_DECODE, per_class=True, classes=80, anchors_per_pixel=9, n_anchors=1000)
    args.update(kw)
    with pytest.raises(dfa.DfxError) as e:
        dfa.BoxNms(**args)
    return str(e.value)


def test_validation_comes_before_the_device():
    """DFX_ERR_INVALID (1) is reported with or without a GPU; "no HIP device" only for a valid descriptor"""
    for kw in (dict(bs=0), dict(n=0), dict(n=4097), dict(max_out=0), dict(max_out=101), dict(keep_ld=49), dict(mode=2), dict(per_class=2),
               dict(force_path=2), dict(classes=0), dict(anchors_per_pixel=0), dict(n_anchors=0), dict(n_anchors=26843546),
               dict(iou_thr=float("inf")), dict(iou_thr=float("nan")), dict(idx_ld=99), dict(row_bytes=35), dict(clip=(float("nan"), 1.0)),
               dict(clip=(10.0, -1.0)), dict(mode=dfa.NMS_BOXES, idx_ld=99)):
        assert "dfx error 1" in _error(**kw), kw
    import torch
    if not torch.cuda.is_available():
        assert "no HIP device" in _error()
        assert "no HIP device" in _error(mode=dfa.NMS_BOXES, per_class=False, idx_ld=0, row_bytes=0)


# ---- the regimes of the GPU tables ---------------------------------------------------------------------------------------------
def test_the_size_table_holds_every_kept_count_regime():
    """kept count 0, 1, below max_out, equal to max_out and cut off by max_out all occur, and differing count_in per image"""
    seen = set()
    for n in S.SIZES:
        for bs in (1, 3):
            case = S.NmsCase("size", bs, n)
            boxes = S.size_problem(n, bs)
            cis = S.count_ins(n, bs)
            assert cis[0] is None and {int(v) for c in cis[1:] for v in c} >= ({-1, 0, 1, n, n + 5} if bs == 1 or n > 1 else {0})
            if bs == 3:
                assert all(len(set(c.tolist())) > 1 for c in cis[1:] if n > 1)
            for count_in in cis:
                full = S.reference(case, n, boxes=boxes, count_in=count_in)
                kept0 = int(full[1][0])
                for max_out in S.max_outs(kept0, n):
                    for kept in full[1]:
                        seen.add("zero" if kept == 0 else "one" if kept == 1 else "below" if kept < max_out else "equal" if kept == max_out else "cut")
                    got = S.cut(full, max_out)
                    direct = S.reference(case, max_out, boxes=boxes, count_in=count_in)
                    assert all((a == b).all() for a, b in zip(got[:3], direct[:3]))   # cutting the full walk is the definition
            if n <= 130:
                assert set(S.max_outs(kept0, n)) >= {1, n}
    assert seen == {"zero", "one", "below", "equal", "cut"}


def test_the_tables_hold_cross_block_suppressions_and_chains():
    """in the size / random tables: a suppression whose i and j lie in different 64-blocks, and a chain -- B suppressed by a
    kept A, and a kept C that B alone would have suppressed; in the planted cases: exactly what each was built to show"""
    def facts(boxes, labels, thr):
        Sm = S.suppress_matrix(boxes, labels, thr)
        keep = S.greedy(boxes, labels, boxes.shape[0], thr, boxes.shape[0])
        kept = np.zeros(boxes.shape[0], dtype=bool)
        kept[keep] = True
        i, j = np.nonzero(Sm & kept[:, None])
        cross = bool(((i // 64) != (j // 64)).any())
        by_kept = (Sm & kept[:, None]).any(axis=0)
        chain = bool((Sm[~kept & by_kept][:, kept]).any())     # a suppressed B overlaps a kept C behind it
        return keep, cross, chain

    for n in (128, 130, 1000):
        _, cross, chain = facts(S.size_problem(n, 1)[0], np.zeros(n, dtype=np.int64), 0.5)
        assert cross and chain, n
    for pc, classes, thr in S.RANDOM:
        case, boxes, idx = S.random_problem(pc, classes, thr)
        _, cross, chain = facts(boxes[0], S.labels_of(case, idx[0] if pc else None), thr)
        assert cross or classes == 80, (pc, classes, thr)
        assert chain or classes == 80 or thr == 0.7, (pc, classes, thr)

    def kept_of(name):
        b, thr = S.planted(name)
        return facts(b[0], np.zeros(b.shape[1], dtype=np.int64), thr)[0], b[0], thr

    n = 130
    assert kept_of("identical")[0] == [0]
    assert kept_of("disjoint")[0] == list(range(n))
    keep, b, thr = kept_of("chain")
    assert keep == [j for j in range(n) if j != 64]
    assert w_suppresses(b[0], b[64], thr) and w_suppresses(b[64], b[129], thr) and not w_suppresses(b[0], b[129], thr)
    assert kept_of("first_last")[0] == list(range(n - 1))
    assert kept_of("zero_area")[0] == list(range(n))                  # 0 / 0 does not suppress, not even an identical box
    keep, b, thr = kept_of("inverted")
    assert 2 in keep and 8 in keep and 66 in keep                      # negative areas, empty intersections
    keep, b, thr = kept_of("nan_inf")
    assert 3 not in keep and {1, 2, 5, 6, 10, 100} <= set(keep)        # a NaN neither suppresses nor is suppressed
    assert 64 in kept_of("at_thr")[0] and 64 not in kept_of("below_thr")[0]
    a, c = F([0, 0, 2, 2]), F([0, 0, 2, 1])
    assert Fraction(2, 4) == Fraction(1, 2) and not w_suppresses(a, c, 0.5) and w_suppresses(a, c, float(np.nextafter(F(0.5), F(0))))


def test_the_decode_table_runs_every_byte_through_both_tables():
    for dt, apx, classes, clip in S.DECODES:
        case, idx, deltas, anchors, tabs = S.decode_case(dt, apx, classes, clip, 0.5)
        for r in range(case.bs):
            ok = (idx[r] >= 0) & (idx[r].astype(np.int64) < case.n_anchors * classes)
            assert (~ok).sum() == 3
            a = (np.where(ok, idx[r], 0) // classes) % apx
            rows = np.arange(case.n)
            for slot in range(4):
                assert set(deltas[r, rows, 4 * a + slot][ok].tolist()) == set(range(256)), (dt, apx, slot)
            assert apx == 1 or len(set(a[ok].tolist())) == apx
        assert case.row_bytes > 4 * apx and (tabs[0] != 0).sum() >= 254 and len(set(tabs[1].tolist())) > 200
        if clip:
            dec = S.reference(case, case.n, idx=idx, deltas=deltas, anchors=anchors, tabs=tabs)[3]
            unclipped = S.reference(case._replace(clip=None), case.n, idx=idx, deltas=deltas, anchors=anchors, tabs=tabs)[3]
            assert (dec != unclipped).any() and dec.min() == 0 and dec[..., 0].max() == clip[0] and dec[..., 1].max() == clip[1]
