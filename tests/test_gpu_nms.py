"""GPU: the box decode + greedy NMS (dfx_nms_*, deepfusion::box_nms) against the numpy reference of tests/nms_ref.py, bit
for bit (tests/test_nms_cpu.py pins that reference against a pure-Python witness and an exact-arithmetic one).  Everything
goes through the C ABI; keep, count and boxes_out of a submit lie in ONE allocation between guard bands with poison fill,
keep_ld = max_out + 3 with the pad columns still poison.  Every case runs on auto, on the generic kernel and on the mask
path, all runs are compared with one another, and the plan is asserted from info()."""
import importlib
import os
import subprocess
import threading

import numpy as np
import pytest

import hipref
import nms_ref as S
import select_ref as SEL

pytestmark = pytest.mark.gpu
dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "deep-fusion_amd", "tools")
GUARD = 1 << 12       # guard bytes around every output
PAD_COLS = 3          # keep_ld = max_out + 3: elements max_out .. keep_ld-1 must keep their poison
PATHS = (-1, S.GENERIC, S.MASK)


def on_device(a, offset=0):
    """the bytes of numpy array `a` on the device, `offset` bytes off a 16-byte boundary -> uint8 tensor (None stays None)"""
    import torch
    if a is None:
        return None
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf = torch.empty(raw.size + offset + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + raw.size]
    view.copy_(torch.from_numpy(raw.copy()))
    return view


class Outputs:
    """keep | count | boxes_out of one submit, each `offsets[name]` bytes off a 16-byte boundary, in one allocation with GUARD
    bytes before, between and behind them; poisoned.  fetch() checks the guards and returns the arrays."""

    def __init__(self, bs, max_out, with_boxes=True, offsets=None):
        import torch
        self.bs, self.max_out, self.ld = bs, max_out, max_out + PAD_COLS
        offsets = offsets or {}
        want = [("keep", bs * self.ld * 4), ("count", bs * 4)]
        if with_boxes:
            want.append(("boxes_out", bs * max_out * 16))
        self.at, pos = {}, 0
        for name, n in want:
            start = pos + GUARD + offsets.get(name, 0)
            self.at[name] = (start, n)
            pos = (start + n + 15) // 16 * 16
        self.template = np.full(pos + GUARD, hipref.GUARD_BYTE, dtype=np.uint8)
        for start, n in self.at.values():
            self.template[start:start + n] = hipref.POISON_BYTE
        self.buf = torch.from_numpy(self.template.copy()).cuda()
        assert self.buf.data_ptr() % 16 == 0

    def dev(self, name):
        if name not in self.at:
            return None
        start, n = self.at[name]
        return self.buf[start:start + n]

    def raw(self):
        return self.buf.cpu().numpy()

    def fetch(self, what):
        got = self.raw()
        outside = np.ones(got.size, dtype=bool)
        for start, n in self.at.values():
            outside[start:start + n] = False
        assert (got[outside] == hipref.GUARD_BYTE).all(), what + ": a guard band was overwritten"
        out = {}
        for name, (start, n) in self.at.items():
            b = got[start:start + n].copy()
            out[name] = (b.view(np.int32).reshape(self.bs, self.ld) if name == "keep" else b.view(np.int32) if name == "count"
                         else b.view(np.float32).reshape(self.bs, self.max_out, 4))
        return out


def make_op(case, max_out, force_path=-1, idx_ld=None, keep_ld=None):
    return dfa.BoxNms(case.bs, case.n, max_out, case.thr, mode=case.mode, per_class=bool(case.per_class), classes=case.classes,
                      anchors_per_pixel=case.apx, n_anchors=case.n_anchors, row_bytes=case.row_bytes, idx_ld=idx_ld,
                      keep_ld=max_out + PAD_COLS if keep_ld is None else keep_ld, clip=case.clip, force_path=force_path)


def to_device(prob, offsets=None):
    """the inputs of a problem (a dict of numpy arrays: boxes, idx, deltas, anchors, tab_c, tab_s, count_in) on the device"""
    offsets = offsets or {}
    return {k: on_device(v, offsets.get(k, 0)) for k, v in prob.items()}


def submit(op, dev, outs, stream=None):
    op.submit(outs.dev("keep"), outs.dev("count"), boxes_out=outs.dev("boxes_out"), stream=stream, **dev)


def compare(got, want, max_out, what):
    keep, count, bout = want[:3]
    hipref.assert_bit_equal(got["count"], count, what + " count")
    hipref.assert_bit_equal(np.ascontiguousarray(got["keep"][:, :max_out]), keep, what + " keep")
    assert (np.ascontiguousarray(got["keep"][:, max_out:]).view(np.uint8) == hipref.POISON_BYTE).all(), what + ": keep elements max_out .. keep_ld-1 were written"
    if "boxes_out" in got:
        hipref.assert_bit_equal(got["boxes_out"], bout, what + " boxes_out")


def assert_plan(case, max_out, info, path):
    what = "%s [%s]" % (S.ident(case, max_out), info.kernel_name.decode())
    assert info.path == path and info.kernel_name.decode() == S.kernel_name(case, path), what
    if path == S.MASK:
        assert (info.tiles, info.grid_prep, info.grid_mask, info.grid_scan) == (S.tiles(case.n), S.prep_grid(case.bs, case.n),
                                                                                 S.mask_grid(case.bs, case.n), case.bs), what
        assert (info.block_prep, info.block_mask, info.block_scan) == (S.PREP_THREADS, S.MASK_THREADS, S.SCAN_THREADS), what
        assert info.scratch_bytes == S.scratch_bytes(case.bs, case.n), what
    else:
        assert (info.tiles, info.grid_prep, info.grid_mask, info.grid_scan, info.scratch_bytes) == (0, 0, 0, case.bs, 0), what
        assert (info.block_prep, info.block_mask, info.block_scan) == (0, 0, S.GENERIC_THREADS), what
    assert info.lds_bytes == S.lds_bytes(path) and info.launches == S.launches(path), what
    assert info.algorithmic_bytes == S.algorithmic_bytes(case, max_out), what
    return what


def ref_args(prob):
    a = {k: prob.get(k) for k in ("boxes", "idx", "deltas", "anchors", "count_in")}
    a["tabs"] = (prob["tab_c"], prob["tab_s"]) if "tab_c" in prob else None
    return a


def check_every_path(case, prob, max_outs=None, full=None, with_boxes=True):
    """the case under each max_out on auto, generic and mask: the plan from info(), the bytes against the reference, all runs
    equal.  full: reference(case, n, ...) when the caller has it.  -> full"""
    full = S.reference(case, case.n, **ref_args(prob)) if full is None else full
    dev = to_device(prob)
    for max_out in (S.max_outs(int(full[1][0]), case.n) if max_outs is None else max_outs):
        want = S.cut(full, max_out)
        raws = []
        for force in PATHS:
            op = make_op(case, max_out, force)
            try:
                what = assert_plan(case, max_out, op.info(), S.auto_path(case, max_out) if force == -1 else force)
                outs = Outputs(case.bs, max_out, with_boxes)
                submit(op, dev, outs)
                compare(outs.fetch(what), want, max_out, what)
                raws.append(outs.raw().tobytes())
            finally:
                op.close()
        assert len(set(raws)) == 1, S.ident(case, max_out)
    return full


# ---- 1. sizes, count_in, max_out ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", S.SIZES)
def test_sizes_counts_and_max_out(n):
    """n around the 64-box tile and at 1000, bs 1 and 3, count_in absent and -1 / 0 / 1 / n / n + 5 differing per image,
    max_out 1, kept - 1, kept, kept + 1 and n: kept counts 0, 1, below, at and cut off by max_out all occur"""
    for bs in (1, 3):
        case = S.NmsCase("size", bs, n)
        boxes = S.size_problem(n, bs)
        for count_in in S.count_ins(n, bs):
            prob = {"boxes": boxes}
            if count_in is not None:
                prob["count_in"] = count_in
            check_every_path(case, prob)


@pytest.mark.parametrize("mode", ["boxes", "decode"])
def test_n_4096(mode):
    """the largest n, one case per mode: 64 blocks, 2080 tiles, every lane of the scan's wave holds a word"""
    n = S.MAX_N
    if mode == "boxes":
        case = S.NmsCase("max", 1, n)
        rng = np.random.default_rng(4096)
        prob = {"boxes": S.clustered_boxes(rng, n, clusters=300)[None]}
    else:
        case, idx, deltas, anchors, tabs = S.decode_case(np.uint8, 3, 80, (400.0, 300.0), 0.5, n=n, bs=1)
        prob = {"idx": idx, "deltas": deltas, "anchors": anchors, "tab_c": tabs[0], "tab_s": tabs[1]}
    full = S.reference(case, n, **ref_args(prob))
    assert 64 < full[1][0] < n
    check_every_path(case, prob, max_outs=(int(full[1][0]) - 1, n), full=full)


def test_auto_follows_the_measured_rule():
    """the AUTO RULE of include/dfx.h (DFX_NMS_AUTO_NOTE): the mask path from n = 200 and max_out = 100 on, the generic
    kernel below either"""
    for n, max_out, path in ((200, 100, S.MASK), (199, 100, S.GENERIC), (200, 99, S.GENERIC), (4096, 4096, S.MASK), (1000, 20, S.GENERIC),
                             (64, 64, S.GENERIC)):
        case = S.NmsCase("auto", 2, n)
        assert S.auto_path(case, max_out) == path, (n, max_out)
        op = make_op(case, max_out)
        try:
            assert op.info().path == path, (n, max_out)
        finally:
            op.close()


# ---- 2. random and planted cases ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc,classes,thr", S.RANDOM)
def test_random_clustered(pc, classes, thr):
    case, boxes, idx = S.random_problem(pc, classes, thr)
    prob = {"boxes": boxes}
    if pc:
        prob["idx"] = idx
    check_every_path(case, prob)


@pytest.mark.parametrize("name", S.PLANTED)
def test_planted(name):
    """identical, disjoint, the A-B-C chain over positions 0 / 64 / 129, block 0 against the last block, zero-area and inverted
    boxes, NaN and Inf, an IoU equal to the threshold (tests/test_nms_cpu.py asserts what each shows)"""
    boxes, thr = S.planted(name)
    case = S.NmsCase(name, 1, boxes.shape[1], S.BOXES, 0, 1, 1, None, None, thr)
    full = check_every_path(case, {"boxes": boxes})
    kept = full[0][0, :full[1][0]].tolist()
    if name == "chain":
        assert 0 in kept and 64 not in kept and 129 in kept
    if name == "at_thr":
        assert 64 in kept
    if name == "below_thr":
        assert 64 not in kept


# ---- 3. decode --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,apx,classes,clip", S.DECODES, ids=lambda v: getattr(v, "__name__", str(v)))
def test_decode(dt, apx, classes, clip):
    """all 256 byte values through both tables, u8 and s8 deltas, A 1 / 3 / 9, classes 1 / 80, clip on and off, idx entries of
    -1 and out of range inside the count.  With a threshold nothing exceeds, boxes_out holds every decoded box: the decode
    alone, bit for bit; then the same inputs under thr 0.5."""
    for thr in (2.0, 0.5):
        case, idx, deltas, anchors, tabs = S.decode_case(dt, apx, classes, clip, thr)
        prob = {"idx": idx, "deltas": deltas, "anchors": anchors, "tab_c": tabs[0], "tab_s": tabs[1]}
        full = check_every_path(case, prob, max_outs=None if thr < 1 else (case.n,))
        if thr > 1:
            assert full[1].tolist() == [case.n - 3, case.n - 3]   # the invalid entries, and only they, are missing
            ok = np.ones(case.n, dtype=bool)
            ok[[5, 70, 71]] = False
            hipref.assert_bit_equal(np.ascontiguousarray(full[2][0, :case.n - 3]), np.ascontiguousarray(full[3][0][ok]), "all decoded boxes")


# ---- 4. fallback, errors, optional output ------------------------------------------------------------------------------------------
def test_misaligned_pointers_fall_back_to_generic_for_that_submit():
    """boxes, idx, keep, count or boxes_out 4 bytes off a 16-byte boundary: the forced mask handle runs the generic kernel for
    that submit (dfx_debug_nms_launches), info() keeps the plan, the bytes are the same"""
    case, boxes, idx = S.random_problem(1, 3, 0.5)
    max_out = 60
    want = S.cut(S.reference(case, case.n, boxes=boxes, idx=idx), max_out)
    op = make_op(case, max_out, force_path=S.MASK)
    try:
        for in_off, out_off in (({"boxes": 4}, {}), ({"idx": 4}, {}), ({}, {"keep": 4}), ({}, {"count": 4}), ({}, {"boxes_out": 4}),
                                ({"boxes": 4, "idx": 4}, {"keep": 4, "count": 4, "boxes_out": 4}), ({}, {})):
            before = dfa.nms_launches()
            outs = Outputs(case.bs, max_out, offsets=out_off)
            submit(op, to_device({"boxes": boxes, "idx": idx}, in_off), outs)
            got = outs.fetch("offset")
            after = dfa.nms_launches()
            ran = S.GENERIC if (in_off or out_off) else S.MASK
            assert [after[p] - before[p] for p in range(2)] == [int(p == ran) for p in range(2)], (in_off, out_off)
            assert op.info().path == S.MASK
            compare(got, want, max_out, "offset %s %s" % (in_off, out_off))
    finally:
        op.close()


def test_errors_launch_nothing():
    """null pointers, a 4-byte pointer off its element, any output overlapping an input or another output: DFX_ERR_INVALID,
    nothing is launched, every output keeps its poison"""
    import torch
    case, idx, deltas, anchors, tabs = S.decode_case(np.uint8, 3, 80, None, 0.5, n=140)
    dev = to_device({"idx": idx, "deltas": deltas, "anchors": anchors, "tab_c": tabs[0], "tab_s": tabs[1], "count_in": np.array([140, 3], dtype=np.int32)})
    bcase, boxes, bidx = S.random_problem(1, 3, 0.5, n=70)
    bdev = to_device({"boxes": boxes, "idx": bidx})
    max_out = 20
    before = dfa.nms_launches()
    for path in (S.MASK, S.GENERIC):
        op = make_op(case, max_out, force_path=path, keep_ld=max_out)
        bop = make_op(bcase, max_out, force_path=path, keep_ld=max_out)
        try:
            outs = Outputs(case.bs, max_out)
            keep, count, bo = outs.dev("keep"), outs.dev("count"), outs.dev("boxes_out")
            good = dict(dev, keep_dev=keep, count_dev=count, boxes_out=bo)
            for name in ("idx", "deltas", "anchors", "tab_c", "tab_s", "keep_dev", "count_dev"):                 # null
                with pytest.raises(dfa.DfxError, match="dfx error 1"):
                    op.submit(**dict(good, **{name: None}))
            for name in ("idx", "anchors", "tab_c", "tab_s", "count_in", "keep_dev", "count_dev", "boxes_out"):  # off their element
                with pytest.raises(dfa.DfxError, match="dfx error 1"):
                    op.submit(**dict(good, **{name: good[name][2:]}))
            for name in ("idx", "deltas", "anchors", "tab_c", "tab_s", "count_in"):                              # an output over an input
                for out in ("keep_dev", "count_dev", "boxes_out"):
                    with pytest.raises(dfa.DfxError, match="dfx error 1"):
                        op.submit(**dict(good, **{out: dev[name]}))
            for a, b in (("keep_dev", count), ("count_dev", keep[4:]), ("boxes_out", keep), ("boxes_out", count)):  # two outputs
                with pytest.raises(dfa.DfxError, match="dfx error 1"):
                    op.submit(**dict(good, **{a: b}))
            bgood = dict(bdev, keep_dev=keep, count_dev=count, boxes_out=bo)
            for bad in (dict(boxes=None), dict(idx=None), dict(boxes=bdev["boxes"][2:]), dict(keep_dev=bdev["boxes"]), dict(boxes_out=bdev["boxes"][16:]),
                        dict(count_dev=bdev["idx"])):
                with pytest.raises(dfa.DfxError, match="dfx error 1"):
                    bop.submit(**dict(bgood, **bad))
            torch.cuda.synchronize()
            assert (outs.raw() == outs.template).all()
        finally:
            op.close()
            bop.close()
    assert dfa.nms_launches() == before


def test_boxes_out_is_optional_and_idx_is_ignored_when_agnostic():
    case, boxes, idx = S.random_problem(0, 1, 0.5)
    full = S.reference(case, case.n, boxes=boxes)
    check_every_path(case, {"boxes": boxes}, max_outs=(40,), full=full, with_boxes=False)
    check_every_path(case, {"boxes": boxes, "idx": np.full_like(idx, -1)}, max_outs=(40,), full=full)   # BOXES / agnostic never reads idx


# ---- 5. threads and streams ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [S.MASK, S.GENERIC], ids=["mask", "generic"])
def test_one_handle_from_two_threads_and_on_three_streams(path):
    """two host threads, each on its own stream, and a third stream, four submits each on alternating inputs: every output
    holds the result of ITS input.  On the mask path the submits share the handle's scratch, so this is what shows that they
    are serialised on the device."""
    import torch
    probs = [S.random_problem(1, 3, 0.5, n=600, bs=2), S.random_problem(1, 3, 0.3, n=600, bs=2)]
    case = probs[0][0]
    max_out = 300
    devs = [to_device({"boxes": b, "idx": i}) for _, b, i in probs]
    wants = [S.cut(S.reference(case, case.n, boxes=b, idx=i), max_out) for _, b, i in probs]
    assert wants[0][0].tolist() != wants[1][0].tolist()
    op = make_op(case, max_out, force_path=path)
    try:
        streams = [torch.cuda.Stream() for _ in range(3)]
        outs = [[Outputs(case.bs, max_out) for _ in range(4)] for _ in range(3)]
        torch.cuda.synchronize()
        errors = []

        def work(i):
            try:
                for j, o in enumerate(outs[i]):
                    submit(op, devs[(i + j) % 2], o, stream=streams[i])
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        for t in threads:
            t.start()
        work(2)
        for t in threads:
            t.join()
        torch.cuda.synchronize()
        assert not errors, errors
        for i, per_stream in enumerate(outs):
            for j, o in enumerate(per_stream):
                compare(o.fetch("stream %d submit %d" % (i, j)), wants[(i + j) % 2], max_out, "stream %d submit %d" % (i, j))
    finally:
        op.close()


# ---- 6. the chain -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nms_path", PATHS, ids=["auto", "generic", "mask"])
def test_select_then_nms_on_the_device(nms_path):
    """SelectTopK over a score map {bs, h, w, A * classes}, gathering the pixel rows of a delta map {bs, h, w, 4 A}, feeds
    BoxNms (DECODE) with its idx, count and gather destination on the device, nothing touching the host in between;
    against select_ref -> nms_ref"""
    import torch
    bs, h, w, apx, classes, k, max_out = 2, 9, 11, 3, 5, 150, 120
    c = apx * classes
    sel = SEL.SelectCase("chain", bs, h, w, c, 16, SEL.U8, SEL.ALL, 230, "random", 3)
    src, order = SEL.problem(sel)
    rng = np.random.default_rng(77)
    dmap = rng.integers(96, 160, (bs, h, w, 4 * apx), dtype=np.uint8)
    gather = ((4 * apx, 4 * apx),)
    sidx, _, scount, rows = SEL.reference(sel, src, k, order, [dmap], gather)
    assert 0 < scount.min() and scount.max() < k   # fill rows and idx -1 behind the count
    na = h * w * apx
    cy, cx = np.divmod(np.arange(h * w), w)
    base = np.stack([cx * 16.0, cy * 16.0], axis=1).repeat(apx, axis=0)
    half = np.tile(np.array([[16.0, 16.0], [24.0, 12.0], [12.0, 24.0]]), (h * w, 1))
    anchors = np.concatenate([base - half, base + half], axis=1).astype(np.float32)
    tabs = capi.box_tables(1.0 / 32, 128, 10.0, 5.0)
    case = S.NmsCase("chain", bs, k, S.DECODE, 1, classes, apx, na, 4 * apx, 0.4, (float(w * 16), float(h * 16)))
    want = S.reference(case, max_out, idx=sidx, deltas=rows, anchors=anchors, tabs=tabs, count_in=scount)
    assert 1 < want[1].min() and (want[1] < np.minimum(scount, max_out)).all()   # suppressions in every image, not the cut
    select = dfa.SelectTopK(bs, h, w, c, np.uint8, k, src_ld=16, min_val=230, gather=gather)
    nms = make_op(case, max_out, nms_path, idx_ld=k)
    try:
        idx_d = torch.full((bs, k), -7, dtype=torch.int32, device="cuda")
        cnt_d = torch.full((bs,), -7, dtype=torch.int32, device="cuda")
        rows_d = torch.full((bs, k, 4 * apx), 0xCD, dtype=torch.uint8, device="cuda")
        outs = Outputs(bs, max_out)
        select.submit(on_device(src), idx_d, cnt_d, gather_src=[on_device(dmap)], gather_dst=[rows_d])
        submit(nms, to_device({"anchors": anchors, "tab_c": tabs[0], "tab_s": tabs[1]}) | {"idx": idx_d, "deltas": rows_d, "count_in": cnt_d}, outs)
        compare(outs.fetch("chain"), want, max_out, "select -> nms")
    finally:
        select.close()
        nms.close()


# ---- 7. the C++ API ----------------------------------------------------------------------------------------------------------------
def test_nms_check_tool():
    """tools/nms_check: box_nms() of the drop-in layer against a scalar loop, conv() -> select_top_k() -> box_nms() chained on
    the device with two frames in flight"""
    p = subprocess.run([os.path.join(TOOLS, "nms_check")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = p.stdout.decode()
    assert p.returncode == 0, text
    lines = [ln for ln in text.splitlines() if ln.startswith("nms_check ")]
    assert len(lines) >= 6 and all(ln.endswith(": ok") for ln in lines), text
    assert "every case identical to the scalar reference" in text
