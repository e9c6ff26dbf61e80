"""GPU: the image-wide top-K with peak filter (dfx_select_*, deepfusion::select_top_k) against the numpy reference of
tests/select_ref.py, bit for bit (tests/test_select_cpu.py pins that reference against a pure-Python witness), and against
dfx_head TOPK and dfx_pool MAX, the ops of the library that define a top-k and a 3x3 maximum on the device.  Everything goes
through the C ABI; idx, val, count and the gather rows lie in ONE allocation between guard bands with poison fill; path,
chunks, grids, blocks, LDS bytes, scratch bytes, launches, algorithmic bytes and kernel name are asserted from info().  Every
case runs on auto and on every forced path whose class holds it, the histogram path under three chunk sizes, and all runs are
compared with one another."""
import functools
import importlib
import os
import subprocess
import threading

import numpy as np
import pytest

import hipref
import select_ref as S

pytestmark = pytest.mark.gpu
dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "deep-fusion_amd", "tools")
GUARD = 1 << 12       # guard bytes around every output
PAD_COLS = 3          # idx_ld = k + 3: elements k .. idx_ld-1 must keep their poison


@functools.lru_cache(maxsize=None)
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def on_device(a, offset=0):
    """the bytes of numpy array `a` on the device, `offset` bytes off a 16-byte boundary -> uint8 tensor"""
    import torch
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf = torch.empty(raw.size + offset + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + raw.size]
    view.copy_(torch.from_numpy(raw.copy()))
    return view


class Outputs:
    """idx | val | count | gather rows of one submit, each `offset[name]` bytes off a 16-byte boundary, in one allocation
    with GUARD bytes before, between and behind them; poisoned.  fetch() checks the guards and returns the arrays."""

    def __init__(self, case, k, with_val=True, gather=(), offsets=None):
        import torch
        self.case, self.k, self.ld = case, k, k + PAD_COLS
        offsets = offsets or {}
        want = [("idx", case.bs * self.ld * 4), ("count", case.bs * 4)]
        if with_val:
            want.append(("val", case.bs * self.ld))
        want += [("g%d" % i, case.bs * k * rb) for i, (rb, _) in enumerate(gather)]
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

    def gather_dev(self):
        return [self.dev(n) for n in sorted(self.at) if n.startswith("g")]

    def raw(self):
        return self.buf.cpu().numpy()

    def fetch(self, what):
        """-> dict of numpy arrays: idx / val {bs, idx_ld} (pad columns included), count {bs}, g<i> {bs, k, rb}"""
        got = self.raw()
        outside = np.ones(got.size, dtype=bool)
        for start, n in self.at.values():
            outside[start:start + n] = False
        assert (got[outside] == hipref.GUARD_BYTE).all(), what + ": a guard band was overwritten"
        case, out = self.case, {}
        for name, (start, n) in self.at.items():
            b = got[start:start + n]
            if name == "idx":
                out[name] = b.copy().view(np.int32).reshape(case.bs, self.ld)
            elif name == "count":
                out[name] = b.copy().view(np.int32)
            elif name == "val":
                out[name] = b.copy().view(S.NP_OF[case.dt]).reshape(case.bs, self.ld)
            else:
                out[name] = b.copy().reshape(case.bs, self.k, -1)
        return out


def make_op(case, k, force_path=-1, gather=(), idx_ld=None):
    return dfa.SelectTopK(case.bs, case.h, case.w, case.c, S.NP_OF[case.dt], k, src_ld=case.ld, idx_ld=k + PAD_COLS if idx_ld is None else idx_ld,
                          peak=case.peak, min_val=case.min_val, gather=gather, force_path=force_path)


def submit(op, src_dev, outs, gather_src=(), stream=None):
    op.submit(src_dev, outs.dev("idx"), outs.dev("count"), outs.dev("val"), gather_src, outs.gather_dev(), stream=stream)


def compare(case, k, got, want, what, with_val=True):
    idx, val, count = want[:3]
    hipref.assert_bit_equal(got["count"], count, what + " count")
    hipref.assert_bit_equal(np.ascontiguousarray(got["idx"][:, :k]), idx, what + " idx")
    assert (np.ascontiguousarray(got["idx"][:, k:]).view(np.uint8) == hipref.POISON_BYTE).all(), what + ": idx elements k .. idx_ld-1 were written"
    if with_val:
        hipref.assert_bit_equal(np.ascontiguousarray(got["val"][:, :k]), val, what + " val")
        assert (np.ascontiguousarray(got["val"][:, k:]).view(np.uint8) == hipref.POISON_BYTE).all(), what + ": val elements k .. idx_ld-1 were written"
    for i, rows in enumerate(want[3:]):
        hipref.assert_bit_equal(got["g%d" % i], rows, what + " gather %d" % i)


def assert_plan(case, k, info, path, chunk, gather=()):
    px = case.h * case.w
    what = "%s [%s]" % (S.ident(case, k), info.kernel_name.decode())
    assert info.path == path and info.kernel_name.decode() == S.kernel_name(case, k, path), what
    if path == S.HIST:
        pl = S.plan(case.bs, px, case.ld, cus(), chunk or 0)
        assert (info.chunks, info.chunk_pixels, info.grid, info.block) == (pl.chunks, pl.chunk_px, pl.grid, S.THREADS), what
        assert info.scratch_bytes == S.scratch_bytes(case.bs, pl.chunks, k), what
    else:
        assert (info.chunks, info.chunk_pixels, info.grid, info.block, info.scratch_bytes) == (1, px, case.bs, S.SORT_THREADS, 0), what
    assert (info.grid_image, info.block_image) == (case.bs, S.SORT_THREADS), what
    assert info.lds_bytes == S.lds_bytes(path) and info.launches == S.launches(path), what
    assert info.algorithmic_bytes == S.algorithmic_bytes(case, k, gather), what
    return what


def check(case, k, src_dev, want, force_path=-1, chunk=None):
    """one guarded submit of `case` under k; the plan from info() and the bytes against the reference -> the raw bytes"""
    capi.set_tuning("DFX_SELECT_CHUNK", chunk)
    try:
        op = make_op(case, k, force_path)
    finally:
        capi.set_tuning("DFX_SELECT_CHUNK", None)
    try:
        path = S.auto_path(case) if force_path == -1 else force_path
        what = assert_plan(case, k, op.info(), path, chunk)
        outs = Outputs(case, k)
        submit(op, src_dev, outs)
        compare(case, k, outs.fetch(what), want, what)
        return outs.raw().tobytes()
    finally:
        op.close()


def check_every_path(case, ks=None, chunks=None):
    """auto, the generic kernel and, where its class holds the case, the histogram path under each chunk setting"""
    src, order = S.problem(case)
    src_dev = on_device(src)
    for k in (S.table_ks(len(order[0])) if ks is None else ks):
        want = S.reference(case, src, k, order)
        outs = [check(case, k, src_dev, want), check(case, k, src_dev, want, force_path=S.GENERIC)]
        if S.hist_class(case):
            for chunk in (S.chunk_settings(case) if chunks is None else chunks):
                outs.append(check(case, k, src_dev, want, force_path=S.HIST, chunk=chunk))
        else:
            with pytest.raises(dfa.DfxError, match="dfx error 2"):
                make_op(case, k, force_path=S.HIST)
        assert len(set(outs)) == 1, S.ident(case, k)


def groups(cases, n):
    return [tuple(cases[i::n]) for i in range(n)]


# ---- 1. the table against the numpy reference -----------------------------------------------------------------------------
@pytest.mark.parametrize("group", groups(S.table_maps(), 24), ids=lambda g: "tab%d" % len(g))
def test_table(group):
    """the whole product (tests/test_select_cpu.py asserts it and its regimes): bs 3 x 5x7, 1x1, 1x9, 9x1, 13x16; c / src_ld
    80/80, 21/32, 1/16, 91/96 and 3/3, 5/7 (generic only), the pad channels at the dtype's maximum; u8 and s8; both peak modes;
    min_val at the dtype's minimum, in the middle and above every element; k in 1, 7, 100, 4096, the candidate count of image
    0 and that +- 1; DFX_SELECT_CHUNK at 1 pixel, two image rows minus a pixel and default"""
    for case in group:
        check_every_path(case)


def test_auto_follows_the_measured_rule():
    """the AUTO RULE of include/dfx.h (DFX_SELECT_AUTO_NOTE): the histogram path in its class from images of 4096 bytes
    (h * w * src_ld) on, the generic kernel below that and outside the class"""
    K = S.SelectCase
    for case, path in ((K("auto", 2, 8, 8, 64, 64, S.U8, S.PEAK3), S.HIST), (K("auto", 2, 1, 1, 1000, 1008, S.S8, S.ALL), S.GENERIC),
                       (K("auto", 2, 1, 1, 4090, 4096, S.S8, S.ALL), S.HIST), (K("auto", 2, 5, 51, 3, 16, S.U8, S.ALL), S.GENERIC),
                       (K("auto", 2, 16, 16, 1, 16, S.U8, S.PEAK3), S.HIST), (K("auto", 2, 16, 17, 15, 15, S.U8, S.ALL), S.GENERIC),
                       (K("auto", 2, 13, 16, 21, 32, S.U8, S.PEAK3), S.HIST)):
        assert S.auto_path(case) == path, S.ident(case)
        src, order = S.problem(case)
        check(case, 10, on_device(src), S.reference(case, src, 10, order))


# ---- 2. planted maps ---------------------------------------------------------------------------------------------------------
def test_all_equal_map_the_lowest_indices_win():
    """every element is a peak and a tie: idx is 0 .. k-1; with 4 pixels x 3 channels per chunk, k ends one before, at and
    one behind a chunk boundary, and at the image's size and beyond"""
    case = S.SelectCase("equal", 2, 5, 7, 3, 16, S.U8, S.PEAK3, None, "equal")
    src, order = S.problem(case)
    n = case.h * case.w * case.c
    assert [o.tolist() for o in order] == [list(range(n))] * 2
    check_every_path(case, ks=(11, 12, 13, 23, 24, 25, n - 1, n, n + 1), chunks=(4, 1, None))
    for k in (12, 25):
        assert S.reference(case, src, k, order)[0].tolist() == [list(range(k))] * 2


def test_two_valued_map_whose_tie_bin_spans_three_chunks():
    """three elements of the higher value, everything else ties: with 16 pixels x 2 channels per chunk the quota of the tie
    bin ends in the first, the second and the third chunk"""
    for dt in (S.S8, S.U8):
        case = S.SelectCase("two", 2, 6, 8, 2, 16, dt, S.ALL, None, "two")
        assert S.plan(case.bs, 48, 16, cus(), 16).chunks == 3
        check_every_path(case, ks=(2, 3, 4, 3 + 29, 3 + 30, 3 + 31, 3 + 61, 3 + 62, 96, 97), chunks=(16, 5, None))


def test_plateaus():
    """flat plateaus, some at the border: every element of a plateau that no higher neighbour touches is a peak"""
    for dt in (S.U8, S.S8):
        case = S.SelectCase("plateau", 2, 9, 11, 3, 16, dt, S.PEAK3, None, "plateau", 3)
        n0 = len(S.problem(case)[1][0])
        assert n0 > 12
        check_every_path(case, ks=(5, n0 - 1, n0, n0 + 1, 4096), chunks=(1, 21, None))


@pytest.mark.parametrize("dt", [S.S8, S.U8], ids=["s8", "u8"])
def test_extremes(dt):
    """maps of the dtype's minimum and maximum only, min_val at both ends"""
    for peak in (S.ALL, S.PEAK3):
        for mv in (None, S.DT_MAX[dt]):
            case = S.SelectCase("extremes", 2, 5, 7, 4, 16, dt, peak, mv, "extremes")
            check_every_path(case, ks=(1, 30, 140, 141), chunks=(1, 13, None))


@pytest.mark.parametrize("n", [4096, 4097])
def test_exactly_4096_and_4097_candidates_under_k_4096(n):
    case = S.SelectCase("count", 2, 13, 16, 21, 32, S.U8, S.ALL, 255, "count%d" % n)
    assert [len(o) for o in S.problem(case)[1]] == [n, n]
    check_every_path(case, ks=(4096,), chunks=(1, 31, None))


# ---- 3. pins by ops the library has ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,c,ld", [(S.S8, 1000, 1008), (S.U8, 21, 32)], ids=["s8-1000", "u8-21"])
def test_row_matrix_equals_dfx_head_topk(dt, c, ld):
    """peak = ALL, h = w = 1, k <= 8: idx and val equal dfx_head TOPK (s32 idx) on the same device buffer"""
    import torch
    bs = 5
    case = S.SelectCase("head", bs, 1, 1, c, ld, dt, S.ALL)
    src_dev = on_device(S.problem(case)[0])
    for k in (1, 5, 8):
        head = dfa.TopK(bs, c, S.NP_OF[dt], np.int32, k=k, src_ld=ld)
        try:
            hidx = torch.empty(bs * k * 4, dtype=torch.uint8, device="cuda")
            hval = torch.empty(bs * k, dtype=torch.uint8, device="cuda")
            head.submit(src_dev, hidx, hval)
            torch.cuda.synchronize()
            want_idx = hidx.cpu().numpy().view(np.int32).reshape(bs, k)
            want_val = hval.cpu().numpy().view(S.NP_OF[dt]).reshape(bs, k)
        finally:
            head.close()
        for path in S.paths(case):
            op = make_op(case, k, force_path=path)
            try:
                outs = Outputs(case, k)
                submit(op, src_dev, outs)
                got = outs.fetch("head pin")
                hipref.assert_bit_equal(np.ascontiguousarray(got["idx"][:, :k]), want_idx, "idx against dfx_head, path %d k %d" % (path, k))
                hipref.assert_bit_equal(np.ascontiguousarray(got["val"][:, :k]), want_val, "val against dfx_head, path %d k %d" % (path, k))
                assert got["count"].tolist() == [k] * bs
            finally:
                op.close()


@pytest.mark.parametrize("dt", [S.U8, S.S8], ids=["u8", "s8"])
def test_peak_set_equals_dfx_pool_max_3x3(dt):
    """peak = PEAK3 with k >= the number of peaks: the returned index set equals {e : dfx_pool MAX 3x3 / 1 pad 1 of src ==
    src}, computed from dfa.Pool's output on the device"""
    import torch
    case = S.SelectCase("pool", 3, 13, 16, 21, 32, dt, S.PEAK3, None, "random", 77)
    src, order = S.problem(case)
    src_dev = on_device(src)
    pool = dfa.Pool(case.bs, case.ld, case.h, case.w, case.h, case.w, (3, 3), (1, 1), (1, 1), S.NP_OF[dt])
    try:
        pooled = torch.empty(src.size, dtype=torch.uint8, device="cuda")
        pool.submit(src_dev, pooled)
        torch.cuda.synchronize()
        same = (pooled == src_dev).cpu().numpy().reshape(src.shape)[..., :case.c].reshape(case.bs, -1)
    finally:
        pool.close()
    peaks = [set(np.nonzero(same[r])[0].tolist()) for r in range(case.bs)]
    k = max(len(p) for p in peaks) + 1
    assert 8 < k <= S.MAX_K and min(len(p) for p in peaks) < case.h * case.w * case.c // 2
    for path in S.paths(case):
        op = make_op(case, k, force_path=path)
        try:
            outs = Outputs(case, k)
            submit(op, src_dev, outs)
            got = outs.fetch("pool pin")
            for r in range(case.bs):
                n = int(got["count"][r])
                assert n == len(peaks[r]) and set(got["idx"][r, :n].tolist()) == peaks[r], (path, r)
        finally:
            op.close()


# ---- 4. gather ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("peak,k", [(S.PEAK3, 50), (S.ALL, 4096)], ids=["peak3-k50", "all-k4096"])
def test_gather_rows(peak, k):
    """two sources, 2 x f32 in a 12-byte pixel and 4 x u8 in a 6-byte pixel: the rows of the selected pixels against numpy
    fancy indexing (select_ref.reference), zero rows from the count on"""
    case = S.SelectCase("gather", 3, 13, 16, 21, 32, S.U8, peak, 100 if peak == S.ALL else None, "random", 5)
    src, order = S.problem(case)
    gather = ((8, 12), (4, 6))
    rng = np.random.default_rng(11)
    gsrc = [rng.integers(0, 256, (case.bs, case.h, case.w, st), dtype=np.uint8) for _, st in gather]
    want = S.reference(case, src, k, order, gsrc, gather)
    assert 0 < want[2].min() and (peak == S.PEAK3 or want[2].max() < k)   # real rows everywhere; fill rows in the second case
    src_dev, g_dev = on_device(src), [on_device(g) for g in gsrc]
    raws = []
    for path in S.paths(case):
        op = make_op(case, k, force_path=path, gather=gather)
        try:
            what = assert_plan(case, k, op.info(), path, None, gather)
            outs = Outputs(case, k, gather=gather)
            submit(op, src_dev, outs, g_dev)
            compare(case, k, outs.fetch(what), want, what)
            raws.append(outs.raw().tobytes())
        finally:
            op.close()
    assert len(set(raws)) == 1


# ---- 5. fallback and errors --------------------------------------------------------------------------------------------------
def test_misaligned_pointers_fall_back_to_generic_for_that_submit():
    """src and val 1 byte, or every pointer 4 bytes, off a 16-byte boundary: the forced histogram handle runs the generic
    kernel for that submit (dfx_debug_select_launches), info() keeps the plan, the bytes are the same"""
    case = S.SelectCase("off", 3, 13, 16, 21, 32, S.S8, S.PEAK3, None, "random", 9)
    src, order = S.problem(case)
    k = 40
    want = S.reference(case, src, k, order)
    op = make_op(case, k, force_path=S.HIST)
    try:
        for src_off, offsets in ((1, {"val": 1}), (4, {"idx": 4, "val": 4, "count": 4}), (0, {"count": 4}), (0, {})):
            before = dfa.select_launches()
            outs = Outputs(case, k, offsets=offsets)
            submit(op, on_device(src, src_off), outs)
            got = outs.fetch("offset")
            after = dfa.select_launches()
            ran = S.GENERIC if (src_off or offsets) else S.HIST
            assert [after[p] - before[p] for p in range(2)] == [int(p == ran) for p in range(2)], (src_off, offsets)
            assert op.info().path == S.HIST
            compare(case, k, got, want, "offset %d %s" % (src_off, offsets))
    finally:
        op.close()


def test_errors_launch_nothing():
    """null pointers, an idx or count off its element, any output overlapping src, a gather source or another output:
    DFX_ERR_INVALID, nothing is launched, every output keeps its poison"""
    import torch
    case = S.SelectCase("err", 2, 5, 7, 21, 32, S.U8, S.PEAK3)
    src_dev = on_device(S.problem(case)[0])
    k, gather = 10, ((8, 8),)
    g_dev = on_device(np.zeros((2, 5, 7, 8), dtype=np.uint8))
    before = dfa.select_launches()
    for path in (S.HIST, S.GENERIC):
        op = make_op(case, k, force_path=path, gather=gather, idx_ld=k)
        plain = make_op(case, k, force_path=path, idx_ld=k)
        try:
            outs = Outputs(case, k, gather=gather)
            idx, val, count, rows = outs.dev("idx"), outs.dev("val"), outs.dev("count"), outs.dev("g0")
            bad = [(0, idx, count, val, [g_dev], [rows]), (src_dev, 0, count, val, [g_dev], [rows]), (src_dev, idx, 0, val, [g_dev], [rows]),
                   (src_dev, idx, count, val, [0], [rows]), (src_dev, idx, count, val, [g_dev], [0]), (src_dev, idx, count, val, [], []),
                   (src_dev, idx[2:], count, val, [g_dev], [rows]), (src_dev, idx, count[1:], val, [g_dev], [rows]),   # off their element
                   (src_dev, src_dev, count, val, [g_dev], [rows]), (src_dev, idx, src_dev[64:], val, [g_dev], [rows]),  # overlap src
                   (src_dev, idx, count, src_dev[8:], [g_dev], [rows]), (src_dev, idx, count, val, [g_dev], [src_dev]),
                   (src_dev, idx, count, val, [g_dev], [g_dev]), (src_dev, g_dev, count, val, [g_dev], [rows]),        # overlap a gather source
                   (src_dev, idx, count, idx, [g_dev], [rows]), (src_dev, idx, idx[4:], val, [g_dev], [rows]),           # two outputs
                   (src_dev, idx, count, val, [g_dev], [idx]), (src_dev, idx, count, rows, [g_dev], [rows])]
            for a in bad:
                with pytest.raises(dfa.DfxError, match="dfx error 1"):
                    op.submit(a[0], a[1], a[2], a[3], a[4], a[5])
            with pytest.raises(dfa.DfxError, match="dfx error 1"):
                plain.submit(src_dev, idx, count, count)                                                                # val overlaps count
            torch.cuda.synchronize()
            assert (outs.raw() == outs.template).all()
        finally:
            op.close()
            plain.close()
    assert dfa.select_launches() == before


def test_val_is_optional():
    case = S.SelectCase("noval", 3, 13, 16, 21, 32, S.U8, S.PEAK3, None, "random", 4)
    src, order = S.problem(case)
    k = 60
    want = S.reference(case, src, k, order)
    src_dev = on_device(src)
    for path in S.paths(case):
        op = make_op(case, k, force_path=path)
        try:
            outs = Outputs(case, k, with_val=False)
            submit(op, src_dev, outs)
            compare(case, k, outs.fetch("no val"), want, "no val path %d" % path, with_val=False)
        finally:
            op.close()


# ---- 6. threads and streams ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [S.HIST, S.GENERIC], ids=["hist", "generic"])
def test_one_handle_from_two_threads_and_on_three_streams(path):
    """two host threads, each on its own stream, and a third stream, four submits each on alternating maps: every output holds
    the result of ITS map.  On the histogram path the submits share the handle's scratch, so this is what shows that they are
    serialised on the device."""
    import torch
    cases = [S.SelectCase("mt", 3, 13, 16, 21, 32, S.U8, S.PEAK3, None, "random", seed) for seed in (21, 22)]
    k = 300
    srcs = [on_device(S.problem(c)[0]) for c in cases]
    wants = [S.reference(c, S.problem(c)[0], k, S.problem(c)[1]) for c in cases]
    assert wants[0][0].tolist() != wants[1][0].tolist()
    capi.set_tuning("DFX_SELECT_CHUNK", 7)
    try:
        op = make_op(cases[0], k, force_path=path)
    finally:
        capi.set_tuning("DFX_SELECT_CHUNK", None)
    try:
        streams = [torch.cuda.Stream() for _ in range(3)]
        outs = [[Outputs(cases[0], k) for _ in range(4)] for _ in range(3)]
        torch.cuda.synchronize()
        errors = []

        def work(i):
            try:
                for j, o in enumerate(outs[i]):
                    submit(op, srcs[(i + j) % 2], o, stream=streams[i])
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
                compare(cases[0], k, o.fetch("stream %d submit %d" % (i, j)), wants[(i + j) % 2], "stream %d submit %d" % (i, j))
    finally:
        op.close()


# ---- 7. the C++ API ----------------------------------------------------------------------------------------------------------------
def test_select_check_tool():
    """tools/select_check: select_top_k() of the drop-in layer against a scalar reference, conv() -> select_top_k() chained on
    the device with two select ops in flight"""
    p = subprocess.run([os.path.join(TOOLS, "select_check")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = p.stdout.decode()
    assert p.returncode == 0, text
    lines = [ln for ln in text.splitlines() if ln.startswith("select_check ")]
    assert len(lines) == 8 and all(ln.endswith(": ok") for ln in lines), text
    assert "every case identical to the scalar reference (8 cases)" in text
