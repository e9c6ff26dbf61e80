"""GPU: the net head (dfx_head_*, deepfusion::argmax / top_k / softmax) against the numpy reference of tests/head_ref.py,
bit for bit (tests/test_head_cpu.py pins that reference against a pure-Python witness), and against dfx_pool MAX, the op of
the library that defines a row maximum on the device.  Everything goes through the C ABI; every idx, val and dst sits between
guard bands with poison fill; path, grid, block, LDS bytes, algorithmic bytes and kernel name are asserted from info().  Every
case runs on every path whose class holds it (forced) and on auto, and the paths are compared with one another."""
import functools
import importlib
import os
import subprocess
import threading

import numpy as np
import pytest

import head_ref as H
import hipref

pytestmark = pytest.mark.gpu
dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "deep-fusion_amd", "tools")
GUARD = 1 << 12       # guard bytes on each side of every output


@functools.lru_cache(maxsize=None)
def problem(case):
    """(src, reference): computed once per case and shared; never written to"""
    src = H.make_src(case)
    want = H.reference(case, src)
    for a in (src,) + (want if isinstance(want, tuple) else (want,)):
        a.setflags(write=False)
    return src, want


def make_op(case, force_path=-1):
    if case.mode == H.TOPK:
        return dfa.TopK(case.rows, case.c, H.NP_OF[case.src_dt], H.NP_OF[case.dst_dt], k=case.k, src_ld=case.ld, force_path=force_path)
    return dfa.Softmax(case.rows, case.c, H.NP_OF[case.src_dt], H.NP_OF[case.dst_dt], table=H.make_table(case), src_ld=case.ld,
                       dst_ld=case.out_ld, out_scale=case.out_scale, force_path=force_path)


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
    """-> (buf, out): out (poisoned, `offset` bytes off a 16-byte boundary) between two GUARD-byte bands"""
    import torch
    buf = torch.empty(GUARD + offset + nbytes + GUARD, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf.fill_(hipref.GUARD_BYTE)
    mid = buf[GUARD + offset:GUARD + offset + nbytes]
    mid.fill_(hipref.POISON_BYTE)
    return buf, mid


def assert_guards(buf, offset, nbytes, what):
    lo, hi = buf[:GUARD + offset], buf[GUARD + offset + nbytes:]
    assert bool((lo == hipref.GUARD_BYTE).all()) and bool((hi == hipref.GUARD_BYTE).all()), what + ": a guard band was overwritten"


def run_guarded(op, case, src_dev, offset=0, stream=None, with_val=True):
    """one submit into guarded outputs -> (idx, val) or dst as numpy arrays of `out_ld` columns (pad columns included)"""
    import torch
    rows, old = case.rows, case.out_ld
    what = op.info().kernel_name.decode()
    obuf, out = guarded(rows * old * H.SIZE_OF[case.dst_dt], offset)
    vbuf = val = None
    if case.mode == H.TOPK and with_val:
        vbuf, val = guarded(rows * old * H.SIZE_OF[case.src_dt], offset)
    torch.cuda.synchronize()
    op.submit(src_dev, out, val, stream=stream)
    torch.cuda.synchronize()
    assert_guards(obuf, offset, out.numel(), what)
    got = out.cpu().numpy().view(H.NP_OF[case.dst_dt]).reshape(rows, old)
    if case.mode == H.SOFTMAX:
        return got
    if val is None:
        return got, None
    assert_guards(vbuf, offset, val.numel(), what)
    return got, val.cpu().numpy().view(H.NP_OF[case.src_dt]).reshape(rows, old)


def compare(case, got, want, what, with_val=True):
    if case.mode == H.TOPK:
        hipref.assert_bit_equal(got[0], want[0], what + " idx")
        if with_val:
            hipref.assert_bit_equal(got[1], want[1], what + " val")
        return
    hipref.assert_bit_equal(np.ascontiguousarray(got[:, :case.c]), want, what)
    pad = np.ascontiguousarray(got[:, case.c:]).view(np.uint8)
    assert (pad == hipref.POISON_BYTE).all(), what + ": elements c .. dst_ld-1 were written"


def check(case, path, force_path=-1, grid_cap=0, offset=0):
    """one guarded submit of `case`; the plan from info() and the bytes against the reference"""
    src, want = problem(case)
    op = make_op(case, force_path)
    try:
        info = op.info()
        what = "%s [%s]" % (case.ident(), info.kernel_name.decode())
        assert info.path == path, what
        assert info.kernel_name.decode() == H.kernel_name(case, path), what
        assert info.grid == H.planned_grid(case.rows, path, grid_cap), (what, info.grid)
        assert info.block == 256 and info.lds_bytes == H.lds_bytes(case, path), (what, info.lds_bytes)
        assert info.algorithmic_bytes == H.algorithmic_bytes(case), what
        got = run_guarded(op, case, on_device(src, offset), offset)
        compare(case, got, want, what)
        return got
    finally:
        op.close()


def as_bytes(got):
    return b"".join(np.ascontiguousarray(g).tobytes() for g in (got if isinstance(got, tuple) else (got,)))


def check_every_path(case, grid_cap=0):
    outs = [check(case, H.auto_path(case), grid_cap=grid_cap)]
    for path in (H.PIXEL, H.ROW, H.GENERIC):
        if H.in_class(case, path):
            outs.append(check(case, path, force_path=path, grid_cap=grid_cap))
        else:
            with pytest.raises(dfa.DfxError, match="dfx error 2"):
                make_op(case, force_path=path)
    assert len({as_bytes(o) for o in outs}) == 1, case.ident()


def chunks(cases, n):
    return [tuple(cases[i::n]) for i in range(n)]


# ---- 1. the tables against the numpy reference -----------------------------------------------------------------------------
@pytest.mark.parametrize("group", chunks(H.pixel_cases(), 12), ids=lambda g: "px%d" % len(g))
def test_pixel_table(group):
    """the whole product, 192 cases (tests/test_head_cpu.py asserts it): rows 2*5*7 (a partial last wave) and 64*3+1; c / ld
    21/32, 19/32, 16/16, 1/16, 33/48, 64/64, 150/160 (the largest src_ld of the pixel class) and 161/176 (the first outside
    it: row and generic only); u8 and s8; k = 1 with u8 and s32 idx; softmax to f32 and u8 with dst_ld = c and dst_ld = ld,
    the pad elements still poison"""
    for case in group:
        check_every_path(case)


@pytest.mark.parametrize("group", chunks(H.row_cases(), 12), ids=lambda g: "row%d" % len(g))
def test_row_table(group):
    """c in 1, 7, 15, 16, 17, 1000, 1023, 1024, 1025 (the first c whose row no longer stays in a wave's registers), 4097 at
    bs 1, 3, 130 (rows packed four per workgroup, a tail wave, a masked tail group); k in 1, 5, 8, c; all four dtypes;
    softmax at c = 1000 and at c = 65535 with the table at the u32 bound"""
    for case in group:
        check_every_path(case)


@pytest.mark.parametrize("case", H.generic_cases(), ids=lambda c: c.ident())
def test_odd_leading_dimensions_run_generic(case):
    """src_ld 21 / 1001 / 7 / 11: outside the classes of both fast paths"""
    assert H.paths(case) == [H.GENERIC]
    check_every_path(case)


@pytest.mark.parametrize("group", chunks(H.special_cases(), 4), ids=lambda g: "sp%d" % len(g))
def test_planted_rows(group):
    """f32 rows of +-NaN with payloads, +-0, +-Inf and denormals; s32, s8 and u8 extremes; all-equal rows: idx by the total
    order with the lower channel first, val the bits verbatim, on every path"""
    for case in group:
        check_every_path(case)


@pytest.mark.parametrize("out_scale,want", [(255.0, 128), (1.0, 0)])
def test_the_tie_row(out_scale, want):
    """two maxima under the one-hot table: p = 0.5 at both, u8 128 at out_scale 255 (127.5 ties to even), 0 at out_scale 1"""
    for dst_dt in (H.U8, H.F32):
        case = H.tie_case(out_scale, dst_dt, rows=70)
        check_every_path(case)
        got = problem(case)[1]
        assert got[3, 3] == (want if dst_dt == H.U8 else 0.5) and got[3, 19] == got[3, 3]


@pytest.mark.parametrize("case", [H.HeadCase("cap", H.TOPK, 64 * 3 + 1 + 512, 21, 32, H.S8, H.U8),
                                  H.HeadCase("cap", H.SOFTMAX, 64 * 3 + 1 + 512, 33, 48, H.U8, H.U8, dst_ld=48),
                                  H.HeadCase("cap", H.TOPK, 130, 1000, 1008, H.S8, H.S32, k=5),
                                  H.HeadCase("cap", H.TOPK, 130, 1000, 1000, H.F32, H.S32, k=8),
                                  H.HeadCase("cap", H.SOFTMAX, 130, 1025, 1040, H.S8, H.F32)], ids=lambda c: c.ident())
def test_grid_cap(tuning, case):
    """DFX_HEAD_GRID=1: every lane (pixel, generic) and every wave (row) makes several passes with a ragged last one"""
    tuning.setenv("DFX_HEAD_GRID", 1)
    check_every_path(case, grid_cap=1)


def test_auto_follows_the_measured_rule():
    """the AUTO RULE of include/dfx.h (DFX_HEAD_AUTO_NOTE): pixel everywhere in its class, but a softmax of 160-byte rows on
    the row kernel; else row in its class from rows of 160 bytes on; else generic"""
    K = H.HeadCase
    for case, path in ((K("auto", H.TOPK, 70, 21, 32, H.U8, H.U8), H.PIXEL), (K("auto", H.SOFTMAX, 70, 150, 160, H.S8, H.U8), H.ROW),
                       (K("auto", H.SOFTMAX, 70, 130, 144, H.S8, H.U8), H.PIXEL), (K("auto", H.TOPK, 70, 150, 160, H.S8, H.U8), H.PIXEL),
                       (K("auto", H.TOPK, 70, 21, 32, H.U8, H.U8, k=2), H.GENERIC), (K("auto", H.TOPK, 70, 150, 160, H.U8, H.U8, k=2), H.ROW),
                       (K("auto", H.TOPK, 70, 140, 144, H.U8, H.U8, k=2), H.GENERIC), (K("auto", H.TOPK, 9, 37, 40, H.S32, H.U8), H.ROW),
                       (K("auto", H.TOPK, 9, 33, 36, H.F32, H.U8), H.GENERIC), (K("auto", H.SOFTMAX, 9, 161, 176, H.U8, H.F32), H.ROW),
                       (K("auto", H.SOFTMAX, 9, 1000, 1001, H.S8, H.F32), H.GENERIC)):
        assert H.auto_path(case) == path, case.ident()
        check(case, path)


# ---- 2. the per-submit fallback ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [H.HeadCase("off", H.TOPK, 70, 21, 32, H.U8, H.U8), H.HeadCase("off", H.SOFTMAX, 70, 21, 32, H.S8, H.U8),
                                  H.HeadCase("off", H.TOPK, 3, 1000, 1000, H.F32, H.S32, k=5)], ids=lambda c: c.ident())
def test_misaligned_pointers_fall_back_to_generic_for_that_submit(case):
    """pointers 1 byte (4 for f32) and 4 bytes off a 16-byte boundary: the forced fast path's handle launches the generic
    kernel for that submit (dfx_debug_head_launches), info() keeps the plan, the bytes are the same"""
    src, want = problem(case)
    for path in [p for p in H.paths(case) if p != H.GENERIC]:
        op = make_op(case, force_path=path)
        try:
            for offset in (H.SIZE_OF[case.src_dt], 4, 0):
                before = dfa.head_launches()
                got = run_guarded(op, case, on_device(src, offset), offset)
                after = dfa.head_launches()
                ran = H.GENERIC if offset else path
                assert [after[p] - before[p] for p in range(3)] == [int(p == ran) for p in range(3)], (case.ident(), path, offset)
                assert op.info().path == path
                compare(case, got, want, "%s path %d offset %d" % (case.ident(), path, offset))
        finally:
            op.close()


# ---- 3. the defining property against dfx_pool -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,c,ld", [(np.uint8, 21, 32), (np.int8, 150, 160), (np.int32, 37, 40), (np.uint8, 1000, 1008)])
def test_val_of_k1_is_the_max_pooling_of_the_row(dtype, c, ld):
    """val of k = 1 equals dfx_pool MAX over the {1, rows, ld, 1} NHWC view of src with a 1 x c window (stride ld).  Integer
    dtypes only: for f32 the head orders by totalOrder (NaN above Inf, -0 below +0) where the pooling's maximum follows the
    reference's comparison, by design."""
    import torch
    rows = 193
    case = H.HeadCase("pool", H.TOPK, rows, c, ld, capi._DT[np.dtype(dtype)], H.S32)
    src = problem(case)[0]
    dev = on_device(src)
    pool = dfa.Pool(1, 1, rows, ld, rows, 1, (1, c), (1, ld), (0, 0), dtype)
    try:
        pooled = torch.empty(rows * src.itemsize, dtype=torch.uint8, device="cuda")
        pool.submit(dev, pooled)
        torch.cuda.synchronize()
        want = pooled.cpu().numpy().view(dtype).reshape(rows, 1)
    finally:
        pool.close()
    assert not np.array_equal(want[:, 0], src[:, c:].max(axis=1))            # (the pad channels are larger and stay out)
    for path in H.paths(case):
        op = make_op(case, force_path=path)
        try:
            _, val = run_guarded(op, case, dev)
            hipref.assert_bit_equal(val, want, "val against dfx_pool, path %d" % path)
        finally:
            op.close()


# ---- 4. state errors -----------------------------------------------------------------------------------------------------------
def test_state_errors_launch_nothing():
    """submit before set_table is DFX_ERR_STATE; a null src, a val given to a softmax, an output that overlaps src or the
    other output are DFX_ERR_INVALID; nothing is launched and the outputs keep their poison"""
    import torch
    case = H.HeadCase("state", H.SOFTMAX, 70, 21, 32, H.U8, H.U8)
    src = on_device(problem(case)[0])
    before = dfa.head_launches()
    op = dfa.Softmax(case.rows, case.c, np.uint8, np.uint8, src_ld=case.ld)
    try:
        buf, dst = guarded(case.rows * case.c)
        with pytest.raises(dfa.DfxError, match="dfx error 5"):
            op.submit(src, dst)
        with pytest.raises(dfa.DfxError, match="dfx error 1"):
            op.set_table(np.zeros(256, dtype=np.uint32))                              # E[0] == 0
        with pytest.raises(dfa.DfxError, match="dfx error 1"):
            op.set_table(np.full(256, (2 ** 32 - 1) // case.c + 1, dtype=np.uint32))  # c * max(E) > 2^32 - 1
        with pytest.raises(dfa.DfxError, match="dfx error 5"):
            op.submit(src, dst)                                                       # a refused table does not count
        op.set_table(np.full(256, (2 ** 32 - 1) // case.c, dtype=np.uint32))          # the last admitted value
        with pytest.raises(dfa.DfxError, match="dfx error 1"):
            op.submit(0, dst)
        with pytest.raises(dfa.DfxError, match="dfx error 1"):
            op.submit(src, 0)
        with pytest.raises(dfa.DfxError, match="dfx error 1"):
            op.submit(src, dst, dst)                                                  # a softmax has no val
        with pytest.raises(dfa.DfxError, match="dfx error 1"):
            op.submit(src, src[16:])                                                  # dst overlaps src
        torch.cuda.synchronize()
        assert bool((dst == hipref.POISON_BYTE).all())
    finally:
        op.close()
    tk = dfa.TopK(case.rows, case.c, np.uint8, np.uint8, src_ld=case.ld)
    try:
        with pytest.raises(dfa.DfxError, match="dfx error 1"):
            tk.set_table(np.ones(256, dtype=np.uint32))                               # not a softmax handle
        buf, idx = guarded(case.rows)
        with pytest.raises(dfa.DfxError, match="dfx error 1"):
            tk.submit(src, idx, idx)                                                  # val overlaps idx
        with pytest.raises(dfa.DfxError, match="dfx error 1"):
            tk.submit(src, src)
        torch.cuda.synchronize()
        assert bool((idx == hipref.POISON_BYTE).all())
    finally:
        tk.close()
    assert dfa.head_launches() == before


def test_val_is_optional():
    import torch
    for case in (H.HeadCase("noval", H.TOPK, 70, 21, 32, H.U8, H.U8), H.HeadCase("noval", H.TOPK, 3, 1000, 1008, H.S8, H.S32, k=5)):
        src, want = problem(case)
        for path in H.paths(case):
            op = make_op(case, force_path=path)
            try:
                got = run_guarded(op, case, on_device(src), with_val=False)
                compare(case, got, want, case.ident(), with_val=False)
            finally:
                op.close()
    torch.cuda.synchronize()


# ---- 5. threads and streams ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,path", [(H.HeadCase("mt", H.SOFTMAX, 193, 21, 32, H.U8, H.U8, dst_ld=32), H.PIXEL),
                                       (H.HeadCase("mt", H.TOPK, 130, 1000, 1000, H.F32, H.S32, k=5), H.ROW),
                                       (H.HeadCase("mt", H.TOPK, 193, 21, 21, H.S8, H.U8, k=3), H.GENERIC)], ids=["pixel", "row", "generic"])
def test_one_handle_from_two_threads_and_on_three_streams(case, path):
    """submit never writes to the handle: two host threads, each on its own stream, and a third stream give the same bytes"""
    import torch
    src, want = problem(case)
    dev = on_device(src)
    op = make_op(case, force_path=path)
    try:
        streams = [torch.cuda.Stream() for _ in range(3)]
        outs = [[guarded(case.rows * case.out_ld * H.SIZE_OF[case.dst_dt]) for _ in range(4)] for _ in range(3)]
        torch.cuda.synchronize()
        errors = []

        def work(i):
            try:
                for _, o in outs[i]:
                    op.submit(dev, o, None, stream=streams[i])
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
        for per_stream in outs:
            for buf, o in per_stream:
                assert_guards(buf, 0, o.numel(), case.ident())
                got = o.cpu().numpy().view(H.NP_OF[case.dst_dt]).reshape(case.rows, case.out_ld)
                compare(case, (got, None) if case.mode == H.TOPK else got, want, case.ident(), with_val=False)
    finally:
        op.close()


# ---- 6. the C++ API ----------------------------------------------------------------------------------------------------------------
def test_head_check_tool():
    """tools/head_check: argmax / top_k / softmax of the drop-in layer against a scalar reference, inner_product -> top_k and
    resize -> argmax chained on the device, two ops in flight"""
    p = subprocess.run([os.path.join(TOOLS, "head_check")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = p.stdout.decode()
    assert p.returncode == 0, text
    lines = [ln for ln in text.splitlines() if ln.startswith("head_check ")]
    assert len(lines) == 14 and all(ln.endswith(": ok") for ln in lines), text
    assert "every case identical to the scalar reference (14 cases)" in text
