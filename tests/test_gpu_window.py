"""GPU: the window partition / reverse op (dfx_window_*) against the numpy reference of tests/window_ref.py, byte for byte.
Everything goes through the C ABI.  Every case runs a partition and a reverse on both forced kernels (where the row kernel's
class admits it; outside it a forced row path is DFX_ERR_UNSUPPORTED) and on auto.  Every destination is pre-filled with a
sentinel, carries guard rows behind its last row and sits between two guard bands; the WHOLE storage is compared, so columns
c .. ld-1 and the guards are proved untouched.  Tokens are random bytes and pairwise distinct, so a misplaced token cannot
compare equal.  Path, grid, block, algorithmic bytes and kernel name are asserted from info(), the kernel that ran from
window_launches()."""
import functools
import importlib

import numpy as np
import pytest

import hipref
import window_ref as W

pytestmark = pytest.mark.gpu
dfa = importlib.import_module("deep-fusion_amd")
GUARD = 1 << 12       # guard bytes on each side of every output
assert W.SENTINEL == hipref.POISON_BYTE


@functools.lru_cache(maxsize=None)
def problem(case):
    """(grid tokens, window tokens): computed once per case and shared; never written to"""
    grid, win = W.grid_tokens(case), W.window_tokens(case)
    back = W.reversed_tokens(case, win)
    assert np.array_equal(back, grid), case.ident()                      # the reference's own round trip
    for a in (grid, win):
        a.setflags(write=False)
    return grid, win


def make_op(case, direction, force_path=W.AUTO):
    return dfa.WindowOp(direction, case.bs, case.h, case.w, case.c, case.window, shift=case.shift, order=case.order, dtype=W.NP_OF[case.dt],
                        grid_ld=case.gld, win_ld=case.wld, pad_value=case.pad_value, force_path=force_path)


def on_device(a, offset=0):
    """the bytes of numpy array `a` on the device, `offset` bytes off a 16-byte boundary -> uint8 tensor"""
    import torch
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf = torch.empty(raw.size + offset + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + raw.size]
    view.copy_(torch.from_numpy(raw.copy()))
    return view


def guarded(nbytes, offset=0):
    """-> (buf, out): out (sentinel-filled, `offset` bytes off a 16-byte boundary) between two GUARD-byte bands"""
    import torch
    buf = torch.empty(GUARD + offset + nbytes + GUARD, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf.fill_(hipref.GUARD_BYTE)
    mid = buf[GUARD + offset:GUARD + offset + nbytes]
    mid.fill_(hipref.POISON_BYTE)
    return buf, mid


def sides(case, direction):
    """(source tokens, their ld, expected destination tokens, their ld)"""
    grid, win = problem(case)
    return (grid, case.gld, win, case.wld) if direction == W.PARTITION else (win, case.wld, grid, case.gld)


def run(op, case, direction, offset=0, stream=None):
    """one guarded submit -> the destination's whole storage {rows + guard rows, ld} as a raw numpy array"""
    import torch
    src, sld, want, dld = sides(case, direction)
    what = "%s [%s]" % (case.ident(), op.info().kernel_name.decode())
    src_dev = on_device(W.storage(case, src, sld), offset)
    rows = want.shape[0] + W.GUARD_ROWS
    buf, out = guarded(rows * dld * case.esize, offset)
    torch.cuda.synchronize()
    op.submit(src_dev, out, stream=stream)
    torch.cuda.synchronize()
    lo, hi = buf[:GUARD + offset], buf[GUARD + offset + out.numel():]
    assert bool((lo == hipref.GUARD_BYTE).all()) and bool((hi == hipref.GUARD_BYTE).all()), what + ": a guard band was overwritten"
    got = out.cpu().numpy().view(W.RAW_OF[case.esize]).reshape(rows, dld)
    hipref.assert_bit_equal(got, W.storage(case, want, dld), what)
    return got


def check(case, direction, force_path, path, grid_cap=0, offset=0):
    op = make_op(case, direction, force_path)
    try:
        info = op.info()
        what = "%s [%s]" % (case.ident(), info.kernel_name.decode())
        assert info.path == path, what
        assert info.kernel_name.decode() == W.kernel_name(case, direction, path), what
        assert info.grid == W.planned_grid(case, direction, path, grid_cap), (what, info.grid)
        assert info.block == 256 and info.algorithmic_bytes == W.algorithmic_bytes(case, direction), what
        assert op.n_windows == case.n_windows and op.win_rows == case.win_rows
        before = dfa.window_launches()
        got = run(op, case, direction, offset)
        after = dfa.window_launches()
        ran = path if offset % 16 == 0 else W.GENERIC
        assert [after[p] - before[p] for p in range(2)] == [int(p == ran) for p in range(2)], what
        assert op.info().path == path, what                              # a fallback leaves the plan alone
        return got
    finally:
        op.close()


def check_every_path(case, grid_cap=0):
    for direction in (W.PARTITION, W.REVERSE):
        outs = [check(case, direction, force, path, grid_cap) for force, path in case.paths()]
        assert len({o.tobytes() for o in outs}) == 1, case.ident()
        if not case.row_class:
            with pytest.raises(dfa.DfxError, match="dfx error 2"):
                make_op(case, direction, W.ROW)


# ---- 1. the case tables: both directions, every kernel, the whole storage ------------------------------------------------------
@pytest.mark.parametrize("case", W.ALL_CASES, ids=lambda c: c.ident())
def test_partition_and_reverse(case):
    check_every_path(case)


# ---- 2. REVERSE(PARTITION(x)) == x on the device, pad tokens never read ------------------------------------------------------
@pytest.mark.parametrize("path", [W.ROW, W.GENERIC], ids=["row", "generic"])
def test_round_trip_on_the_device(path):
    """the windows a partition wrote go straight into a reverse (no host step): the grid comes back, whatever the pad tokens
    hold -- they are overwritten with other bytes in between, since a reverse must not read them"""
    import torch
    for case in [c for c in W.ALL_CASES if c.row_class][::7] + W.swin_cases()[:3]:
        grid, win = problem(case)
        part, rev = make_op(case, W.PARTITION, path), make_op(case, W.REVERSE, path)
        try:
            src = on_device(W.storage(case, grid, case.gld))
            _, mid = guarded((case.win_rows + W.GUARD_ROWS) * case.wld * case.esize)
            _, back = guarded((case.grid_rows + W.GUARD_ROWS) * case.gld * case.esize)
            part.submit(src, mid)
            torch.cuda.synchronize()
            rows = mid.view(case.win_rows + W.GUARD_ROWS, case.wld * case.esize)
            pads = torch.from_numpy(np.flatnonzero(W.pad_mask(case))).cuda()
            rows[pads] = 0x5A                                             # whole pad rows, pad columns included
            rev.submit(mid, back)
            torch.cuda.synchronize()
            got = back.cpu().numpy().view(W.RAW_OF[case.esize]).reshape(case.grid_rows + W.GUARD_ROWS, case.gld)
            hipref.assert_bit_equal(got, W.storage(case, grid, case.gld), case.ident())
        finally:
            part.close()
            rev.close()


# ---- 3. misaligned pointers, overlap ------------------------------------------------------------------------------------------------
def test_misaligned_pointers_take_the_generic_kernel_for_that_submit():
    for case in (W.WinCase("mis", 3, 10, 13, 96, (7, 7), (3, 3), W.ROW_MAJOR, W.S8, win_ld=112, pad_value=0x80, seed=31),
                 W.WinCase("mis", 1, 7, 7, 24, (4, 4), (2, 0), W.COL_MAJOR, W.F32, grid_ld=28, pad_value=0x3FC01234, seed=32)):
        for direction in (W.PARTITION, W.REVERSE):
            for offset in (0, case.esize, 8, 16):
                check(case, direction, W.ROW, W.ROW, offset=offset)
                check(case, direction, W.GENERIC, W.GENERIC, offset=offset)


def test_overlapping_and_misaligned_submits_are_refused():
    import torch
    case = W.WinCase("overlap", 2, 7, 7, 16, (7, 7), (3, 3), W.ROW_MAJOR, W.F32, seed=33)
    grid, win = problem(case)
    nbytes = case.grid_rows * case.c * 4
    assert case.grid_rows == case.win_rows
    op = make_op(case, W.PARTITION)
    try:
        big = torch.empty(3 * nbytes, dtype=torch.uint8, device="cuda")
        big[:nbytes].copy_(torch.from_numpy(np.ascontiguousarray(grid).view(np.uint8).reshape(-1).copy()))
        before = dfa.window_launches()
        for dst in (big, big[nbytes - 4:], big[16:]):                     # in place, the last element, shifted by a lane
            with pytest.raises(dfa.DfxError, match="dfx error 1.*overlaps"):
                op.submit(big, dst)
        with pytest.raises(dfa.DfxError, match="dfx error 1.*overlaps"):
            op.submit(big[nbytes:], big[4:])                              # dst in front of src, its last element inside
        with pytest.raises(dfa.DfxError, match="dfx error 1.*aligned"):
            op.submit(big, big[nbytes + 2:])
        with pytest.raises(dfa.DfxError, match="dfx error 1.*null"):
            op.submit(0, big)
        assert dfa.window_launches() == before                            # nothing was launched
        op.submit(big, big[nbytes:])                                      # right behind src: no overlap
        torch.cuda.synchronize()
        got = big[nbytes:2 * nbytes].cpu().numpy().view(np.uint32).reshape(case.win_rows, case.c)
        hipref.assert_bit_equal(got, win, "behind src")
    finally:
        op.close()


# ---- 4. DFX_WINDOW_GRID ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [1, 3])
def test_grid_cap(tuning, cap):
    """dozens of trips and a ragged last one under a cap of 1 and of 3 workgroups: a trip of the row kernel starts in the
    middle of a token, of a window and of an image"""
    tuning.setenv("DFX_WINDOW_GRID", cap)
    for case in (W.WinCase("cap", 3, 10, 13, 96, (7, 7), (3, 3), W.ROW_MAJOR, W.S8, pad_value=0x80, seed=41),
                 W.WinCase("cap", 2, 16, 12, 68, (2, 2), (0, 0), W.COL_MAJOR, W.S32, win_ld=72, seed=42),
                 W.WinCase("cap", 5, 3, 200, 16, (3, 5), (2, 199), W.ROW_MAJOR, W.U8, grid_ld=32, seed=43)):
        assert W.planned_grid(case, W.REVERSE, W.ROW) >= 2 and W.planned_grid(case, W.PARTITION, W.ROW, cap) == cap
        check_every_path(case, grid_cap=cap)


# ---- 5. streams ------------------------------------------------------------------------------------------------------------------
def test_submits_follow_their_stream():
    import torch
    case = W.swin_cases()[1]
    op = make_op(case, W.PARTITION, W.ROW)
    try:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            run(op, case, W.PARTITION, stream=s)
    finally:
        op.close()
