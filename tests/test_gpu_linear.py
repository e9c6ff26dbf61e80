"""GPU: the int8 token linear op (dfx_linear_*, dfa.Linear) against the numpy reference of tests/linear_ref.py, bit for bit
(tests/test_linear_cpu.py pins that reference against an element-by-element witness and against fc_ref), and against the ops
the library already has: dfx_fc (dfa.InnerProduct), dfx_bmm (dfa.MatMul) and dfx_wsum's table (dfa.ScaledSum).  Everything
goes through the C ABI.  dst's whole storage sits between guard bands and is poisoned: the comparison of the whole storage
shows that the elements n .. dst_ld-1 of every row are not written.  The pad columns of src hold 0xFF and the rows behind
`rows` are poisoned.  The tile kernel is forced at both tile heights, on the fast and on the exact route, then the generic
kernel is forced: all against the one reference."""
import functools
import importlib
import threading

import numpy as np
import pytest

import hipref
import linear_ref as R

pytestmark = pytest.mark.gpu
dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
GUARD = 1 << 12       # guard bytes on each side of dst
BEHIND = 1 << 12      # poisoned bytes behind src's last row


@pytest.fixture(autouse=True)
def tuning():
    """no switch of one test reaches the next"""
    keys = []

    class T:
        def setenv(self, k, v):
            keys.append(k)
            capi.set_tuning(k, v)
    yield T()
    for k in keys:
        capi.set_tuning(k, None)


@functools.lru_cache(maxsize=None)
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def src_on_device(data, offset=0):
    """src's storage on the device, `offset` bytes off a 16-byte boundary, poison behind its last row -> uint8 tensor"""
    import torch
    raw = np.ascontiguousarray(data["src"]).view(np.uint8).reshape(-1)
    buf = torch.empty(offset + raw.size + BEHIND, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf.fill_(hipref.POISON_BYTE)
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


def make_op(case, force_path, data=None):
    op = dfa.Linear(case.rows, case.k, case.n, src_dtype=R.NP_OF[case.src_dt], dst_dtype=R.NP_OF[case.dst_dt], bia_dt=case.bia_dt,
                    relu=case.relu, rm=case.rm, nscales=case.nscales, src_ld=case.sld, dst_ld=case.dld,
                    table=None if case.lut_in == R.UNDEF else case.lut_in, force_path=force_path)
    if data is not None:
        op.set_weights(data["w"], data["scales"], data["bia"])
        if data["lut"] is not None:
            op.set_table(data["lut"])
    return op


def dst_bytes(case):
    return R.dst_storage(case) * R.SIZE_OF[case.dst_dt]


def run(op, case, src_dev, dst_offset=0, stream=None):
    """one submit into a guarded, poisoned dst -> dst's whole storage as bytes"""
    import torch
    n = dst_bytes(case)
    buf, dst = guarded(n, dst_offset)
    torch.cuda.synchronize()
    op.submit(src_dev, dst, stream=stream)
    torch.cuda.synchronize()
    assert_guards(buf, dst_offset, n, case.ident())
    return dst.cpu().numpy()


def same(got, want, case, what):
    """whole-storage comparison, reported per element of dst's dtype; NaNs by place and payload (the bits)"""
    if not np.array_equal(got, want):
        dt = {R.F32: np.uint32}.get(case.dst_dt, R.NP_OF[case.dst_dt])
        hipref.assert_bit_equal(got.view(dt), want.view(dt), "%s %s" % (case.ident(), what))


def check_case(case, data, paths=(R.TILE, R.GENERIC), bms=R.BMS, grid_cap=0, want=None, tuning=None):
    """the case on the forced tile kernel at every tile height in `bms` (the route the weights prove, then the exact route) and
    on the forced generic kernel; path, route, kernel name, grid, block, LDS and the algorithmic counts from the handle"""
    want = R.reference(case, data) if want is None else want
    src_dev = src_on_device(data)
    d = R.desc_of(case)
    outs = []
    for path in paths:
        for bm in (bms if path == R.TILE else (None,)):
            if bm is not None:
                capi.set_tuning("DFX_LINEAR_BM", bm)
            try:
                op = make_op(case, path)
            finally:
                capi.set_tuning("DFX_LINEAR_BM", None)
            try:
                routes = ((None, int(R.fast_ok(case, data))), ("1", 0)) if path == R.TILE else ((None, 0),)
                for no_fast, route in routes:
                    if no_fast:
                        capi.set_tuning("DFX_NO_FAST", no_fast)
                    try:
                        op.set_weights(data["w"], data["scales"], data["bia"])
                    finally:
                        if no_fast:
                            capi.set_tuning("DFX_NO_FAST", None)
                    if data["lut"] is not None:
                        op.set_table(data["lut"])
                    info = op.info()
                    what = "[%s]" % info.kernel_name.decode()
                    pbm = R.planned_bm(d, cus(), bm or 0)
                    assert info.path == path and op.requant() == route, (case.ident(), what, op.requant(), route)
                    assert info.kernel_name.decode() == R.kernel_name(case, path, pbm, route), (case.ident(), what)
                    assert info.grid == R.planned_grid(d, path, pbm, cus(), grid_cap) and info.block == 256, (case.ident(), what, info.grid)
                    assert info.lds_bytes == R.lds_bytes(path, pbm), (case.ident(), what)
                    assert info.algorithmic_ops == R.algorithmic_ops(d) and info.algorithmic_bytes == R.algorithmic_bytes(d), (case.ident(), what)
                    before = dfa.linear_launches()
                    got = run(op, case, src_dev)
                    after = dfa.linear_launches()
                    assert [after[p] - before[p] for p in range(2)] == [int(p == path) for p in range(2)], (case.ident(), what)
                    same(got, want, case, what)
                    outs.append(got)
            finally:
                op.close()
    return outs


# ---- 1. the grid of tails ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src_dt", [R.U8, R.S8], ids=["u8", "s8"])
@pytest.mark.parametrize("bm", R.BMS)
@pytest.mark.parametrize("part", range(4))
def test_grid_of_tails_on_the_tile_kernel(bm, src_dt, part):
    """rows in 1, BM-1, BM, BM+1, 2BM+2 x n in 1, 3, 4, 127, 128, 129, 264 x k in 1, 15, 16, 17, 63, 64, 65, 136, 200 as a pairwise
    cover (linear_ref.shape_grid), on the forced tile kernel of height BM, fast and exact route; dst dtypes, dst pitches (vector
    and element stores), bias dtypes, ReLU, round modes and per-channel scales rotating"""
    for case in R.shape_grid(bm, src_dt)[part::4]:
        check_case(case, R.generate(case), paths=(R.TILE,), bms=(bm,))


@pytest.mark.parametrize("src_dt", [R.U8, R.S8], ids=["u8", "s8"])
@pytest.mark.parametrize("part", range(2))
def test_grid_of_tails_on_the_generic_kernel(src_dt, part):
    """the same cover (the one of BM = 64) on the forced generic kernel"""
    for case in R.shape_grid(64, src_dt)[part::2]:
        check_case(case, R.generate(case), paths=(R.GENERIC,))


# ---- 2. compensation at depth ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [200, R.KMAX])
def test_compensation(k):
    """u8 rows of all 255 and all 0 against weight rows of all -128 and all 127 at k = 200 and 65025: s32 dst and scale 1, so
    nothing is hidden by saturation"""
    seen = 0
    for case, data in R.compensation_cases():
        if case.k != k:
            continue
        vals = R.values(case, data)
        assert R.accumulate(case, data).tolist() == [[255 * -128 * k, 255 * 127 * k], [0, 0]]
        if k == 200:                                                 # (f32 rounds the deepest sums: there the reference decides)
            assert vals.tolist() == [[255 * -128 * k, 255 * 127 * k], [0, 0]]
        else:
            assert abs(int(vals[0, 0])) > 2 ** 30 and abs(int(vals[0, 1])) > 2 ** 30
        check_case(case, data)
        seen += 1
    assert seen == 1


# ---- 3. the lane map ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bm", R.BMS)
def test_lane_map(bm):
    """identity-like src rows against asymmetric weights: element (m, o) is one weight times a small factor, so a transposed,
    swapped or shifted fragment shows everywhere"""
    case, data = R.lane_map_case(bm)
    m, o = np.arange(case.rows).reshape(-1, 1), np.arange(case.n).reshape(1, -1)
    assert np.array_equal(R.values(case, data), (1 + m // case.k) * data["w"].astype(np.int32)[o, m % case.k])
    check_case(case, data, bms=(bm,))


# ---- 4. bias, scales, ties, non-finite scales ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.bias_cases(), ids=lambda c: c.ident())
def test_bias_of_every_dtype_and_per_channel_scales(case):
    check_case(case, R.generate(case))


@pytest.mark.parametrize("case", R.tie_cases(), ids=lambda c: c.ident())
def test_ties_at_scale_one_half(case):
    """every odd accumulator is a tie: nearest-even and floor differ there, and both routes must agree with the reference"""
    data = R.generate(case)
    acc = R.accumulate(case, data)
    assert (acc % 2 != 0).mean() > 0.25
    check_case(case, data)


@pytest.mark.parametrize("case", R.nonfinite_cases(), ids=lambda c: c.ident())
def test_nonfinite_scales_take_the_exact_route(case):
    """a scale of inf or NaN is never called fast; the exact route gives the x86 0x80000000 pattern and its saturations"""
    data = R.generate(case)
    assert not R.fast_ok(case, data)
    check_case(case, data)


# ---- 5. the table --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.table_cases(), ids=lambda c: c.ident())
def test_table_behind_the_requant(case):
    """u8 and s8 index types with a random permutation table; the result equals the same op with dst_dt = lut_in_dt and no
    table followed by dfa.ScaledSum (one input, scale 1, that table)"""
    import torch
    data = R.generate(case)
    assert sorted(data["lut"].tolist()) == list(range(256))
    got = check_case(case, data)[0]
    plain = R.with_dst(case, dst_dt=case.lut_in, lut_in=R.UNDEF, dst_ld=case.n)
    pdata = dict(data, lut=None)
    mid = check_case(plain, pdata, paths=(R.GENERIC,))[0]
    ws = dfa.ScaledSum((1, 1, case.rows, case.n), [R.NP_OF[case.lut_in]], R.NP_OF[case.dst_dt], [1], lut_in=R.NP_OF[case.lut_in])
    try:
        ws.set_params([np.ones(1, dtype=np.float32)], lut=data["lut"])
        mid_dev = torch.from_numpy(mid.copy()).cuda()
        out = torch.empty(case.rows * case.n, dtype=torch.uint8, device="cuda")
        ws.submit([mid_dev], out)
        torch.cuda.synchronize()
        chained = out.cpu().numpy().reshape(case.rows, case.n)
    finally:
        ws.close()
    idx = np.arange(case.rows).reshape(-1, 1) * case.dld + np.arange(case.n).reshape(1, -1)
    assert np.array_equal(got[idx], chained), case.ident()


def test_gelu_table_behind_fc1():
    """dfa.gelu_table as the table of an s8 -> s8 linear layer: the reference applies the same bytes"""
    case = R.GELU_CASE
    data = dict(R.generate(case))
    data["lut"] = dfa.gelu_table(0.05, 0.04, np.int8, np.int8)
    vals = R.values(case, data)
    assert len(np.unique(vals)) > 20 and vals.min() < 0 < vals.max()
    check_case(case, data)


# ---- 6. pitched operands -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.pitched_cases(), ids=lambda c: c.ident())
def test_pitched_operands(case):
    """src_ld > k (a slice of a wider tensor: the columns behind k hold 0xFF), dst_ld > n (the pad stays poisoned), and a
    projection written into a third of a QKV-shaped tensor"""
    check_case(case, R.generate(case))


def test_three_projections_fill_one_qkv_tensor():
    """Q, K and V written by three handles into the thirds of one {rows, 3C} tensor: together they leave no byte unwritten and
    overwrite nothing of each other"""
    import torch
    base = R.QKV_CASES[0]
    c, rows = base.n, base.rows
    src_dev = None
    out = torch.empty(rows * 3 * c, dtype=torch.uint8, device="cuda")
    out.fill_(hipref.POISON_BYTE)
    want = np.empty((rows, 3 * c), dtype=np.int8)
    for path in (R.TILE, R.GENERIC):
        for third in range(3):
            case = R.QKV_CASES[third]
            data = dict(R.generate(case))
            if third:
                data["src"] = R.generate(base)["src"]
            src_dev = src_on_device(data)
            want[:, third * c:(third + 1) * c] = R.values(case, data)
            op = make_op(case, path, data)
            try:
                op.submit(src_dev, out[third * c:])
                torch.cuda.synchronize()
            finally:
                op.close()
        assert np.array_equal(out.cpu().numpy().view(np.int8).reshape(rows, 3 * c), want), path


# ---- 7. DFX_LINEAR_GRID -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [1, 3])
def test_grid_cap(cap, tuning):
    """DFX_LINEAR_GRID = 1 and 3 on 12 tiles of 64 x 128: workgroups loop over several tiles, across n-blocks"""
    case = R.GRID_CAP_CASE
    assert R.tiles(R.desc_of(case), 64) == 12
    tuning.setenv("DFX_LINEAR_GRID", cap)
    check_case(case, R.generate(case), grid_cap=cap)


# ---- 8. the per-submit fallback, state and submit errors ------------------------------------------------------------------
def test_misaligned_pointers_fall_back_per_submit():
    """a src that is not 16-byte aligned takes the generic kernel for that submit (dfx_debug_linear_launches); a dst that is
    only element-aligned keeps the tile kernel, which then stores element by element; the bytes are the same"""
    for case in R.MISALIGNED_CASES:
        data = R.generate(case)
        want = R.reference(case, data)
        op = make_op(case, R.TILE, data)
        try:
            for src_off, dst_off, ran in ((0, 0, R.TILE), (4, 0, R.GENERIC), (0, R.SIZE_OF[case.dst_dt], R.TILE), (1, 3 * R.SIZE_OF[case.dst_dt], R.GENERIC)):
                src_dev = src_on_device(data, src_off)
                before = dfa.linear_launches()
                got = run(op, case, src_dev, dst_offset=dst_off)
                after = dfa.linear_launches()
                assert [after[p] - before[p] for p in range(2)] == [int(p == ran) for p in range(2)], (case.ident(), src_off, dst_off)
                assert op.info().path == R.TILE
                same(got, want, case, "offsets %d, %d" % (src_off, dst_off))
        finally:
            op.close()


def test_state_and_submit_errors_launch_nothing():
    import torch
    case, tcase = R.ERROR_CASES
    data, tdata = R.generate(case), R.generate(tcase)
    src_dev = src_on_device(data)
    buf, dst = guarded(dst_bytes(case))
    before = dfa.linear_launches()
    op, top = make_op(case, R.TILE), make_op(tcase, R.TILE)
    try:
        for h, args in ((op, (src_dev, dst)), (top, (src_dev, dst))):
            with pytest.raises(dfa.DfxError, match="dfx error 5"):
                h.submit(*args)                                       # before set_weights
        top.set_weights(tdata["w"], tdata["scales"], tdata["bia"])
        with pytest.raises(dfa.DfxError, match="dfx error 5.*set_table"):
            top.submit(src_dev, dst)                                  # a table handle before set_table
        with pytest.raises(dfa.DfxError, match="dfx error 1"):
            op.set_table(tdata["lut"])                                # a handle created without a table
        op.set_weights(data["w"], data["scales"], data["bia"])
        with pytest.raises(dfa.DfxError, match="dfx error 1.*aligned"):
            op.submit(src_dev, buf[GUARD + 2:])                       # an f32 dst off its element
        with pytest.raises(dfa.DfxError, match="dfx error 1.*overlaps"):
            op.submit(src_dev, src_dev[16:])
        with pytest.raises(dfa.DfxError, match="dfx error 1.*null"):
            op.submit(0, dst)
        torch.cuda.synchronize()
        assert dfa.linear_launches() == before
        assert bool((dst == hipref.POISON_BYTE).all())
    finally:
        op.close()
        top.close()


def test_submit_host():
    """dfx_linear_submit_host: densely packed host tensors in and out, synchronous, on both paths; pitched operands are refused"""
    case = R.HOST_CASE
    data = R.generate(case)
    for path in (R.TILE, R.GENERIC):
        op = make_op(case, path, data)
        try:
            before = dfa.linear_launches()
            got = op.submit_host(data["src"].reshape(case.rows, case.k))
            after = dfa.linear_launches()
            assert [after[p] - before[p] for p in range(2)] == [int(p == path) for p in range(2)]
            assert got.dtype == np.int32 and np.array_equal(got, R.values(case, data)), path
        finally:
            op.close()
    pitched = R.with_dst(case, dst_ld=52)
    op = make_op(pitched, R.GENERIC, R.generate(pitched))
    try:
        with pytest.raises(dfa.DfxError, match="dfx error 2.*densely"):
            op.submit_host(data["src"].reshape(case.rows, case.k))
    finally:
        op.close()


# ---- 9. one handle, two threads, two streams -------------------------------------------------------------------------------
def test_one_handle_from_two_threads_on_two_streams():
    import torch
    case = R.THREADS_CASE
    data = R.generate(case)
    want = R.reference(case, data)
    for path in (R.TILE, R.GENERIC):
        op = make_op(case, path, data)
        src_dev = src_on_device(data)
        outs, errs = {}, []

        def work(i):
            try:
                st = torch.cuda.Stream()
                res = []
                for _ in range(8):
                    buf, dst = guarded(dst_bytes(case))
                    st.wait_stream(torch.cuda.current_stream())
                    op.submit(src_dev, dst, stream=st)
                    res.append((buf, dst))
                st.synchronize()
                outs[i] = res
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        try:
            torch.cuda.synchronize()
            ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
            for t in ts:
                t.start()
            for t in ts:
                t.join()
            assert not errs, errs
            for i in range(2):
                for buf, dst in outs[i]:
                    assert_guards(buf, 0, dst_bytes(case), case.ident())
                    same(dst.cpu().numpy(), want, case, "thread %d" % i)
        finally:
            op.close()


# ---- 10. auto ---------------------------------------------------------------------------------------------------------------
def test_auto_rule():
    """the AUTO RULE of include/dfx.h (DFX_LINEAR_AUTO_NOTE), mirrored by linear_ref.auto_path: on both sides of each bound --
    rows, n, k, the tile count, the multiply-adds and the class; the forced paths are honoured"""
    want = {(1576, 768, 768, 768): R.TILE, (1575, 768, 768, 768): R.GENERIC,             # rows
            (9408, 256, 96, 256): R.TILE, (9408, 256, 95, 256): R.GENERIC,               # n
            (9408, 96, 288, 96): R.TILE, (9408, 95, 288, 96): R.GENERIC,                 # k
            (3393, 512, 128, 512): R.TILE, (3392, 512, 128, 512): R.GENERIC,             # 54 tiles of 64 x 128
            (1700, 256, 256, 256): R.TILE, (1699, 256, 256, 256): R.GENERIC,             # 1700 * 256 * 256 multiply-adds
            (1576, 768, 2304, 784): R.TILE, (1576, 768, 2304, 776): R.GENERIC,           # the class
            (1, 16, 1, 16): R.GENERIC, (130, 64, 128, 64): R.GENERIC, (12608, 3072, 768, 3072): R.TILE}
    for (rows, k, n, sld), path in want.items():
        case = R.LinCase("auto", rows, k, n, src_ld=sld)
        d = R.desc_of(case)
        op = make_op(case, -1)
        try:
            info = op.info()
            bm = R.planned_bm(d, cus())
            assert info.path == R.auto_path(d) == path and info.lds_bytes == R.lds_bytes(path, bm), (d, info.path)
            assert info.kernel_name.decode() == R.kernel_name(case, path, bm, 0).replace(" exact", " (no weights)")
            assert info.grid == R.planned_grid(d, path, bm, cus())
        finally:
            op.close()
        if R.tile_class(d):
            op = make_op(case, R.TILE)
            try:
                assert op.info().path == R.TILE
            finally:
                op.close()
        else:
            with pytest.raises(dfa.DfxError, match="dfx error 2"):
                make_op(case, R.TILE)
        op = make_op(case, R.GENERIC)
        try:
            assert op.info().path == R.GENERIC
        finally:
            op.close()


def test_auto_takes_the_tile_kernel_at_a_measured_point_and_gives_the_reference():
    """the smallest measured point (DETR 256 -> 256, 1700 rows) on auto: the tile kernel runs and the bytes are the reference's"""
    case = R.AUTO_POINT_CASE
    data = R.generate(case)
    op = make_op(case, -1, data)
    try:
        assert op.info().path == R.TILE
        before = dfa.linear_launches()
        got = run(op, case, src_on_device(data))
        after = dfa.linear_launches()
        assert (after[R.TILE] - before[R.TILE], after[R.GENERIC] - before[R.GENERIC]) == (1, 0)
        same(got, R.reference(case, data), case, "auto")
    finally:
        op.close()


# ---- 11. against the ops the library already has -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.fc_twin_cases(), ids=lambda c: c.ident())
def test_equals_inner_product(case):
    """u8 src, src_ld = k, dst_ld = n: dfa.InnerProduct with ih = iw = 1, ic = k, bs = rows gives the same bytes"""
    import torch
    data = R.generate(case)
    got = check_case(case, data)[0]
    fc = dfa.InnerProduct((case.rows, 1, 1, case.k), case.n, dst_dt=case.dst_dt, bia_dt=case.bia_dt, relu=case.relu, rm=case.rm,
                          nscales=case.nscales)
    try:
        fc.set_weights(data["w"].reshape(case.n, case.k, 1, 1), data["scales"], data["bia"])
        src_dev = src_on_device(data)
        buf, dst = guarded(dst_bytes(case))
        fc.submit(src_dev, dst)
        torch.cuda.synchronize()
        same(dst.cpu().numpy(), got, case, "against " + fc.info().kernel_name.decode())
    finally:
        fc.close()


@pytest.mark.parametrize("case", R.bmm_twin_cases(), ids=lambda c: c.ident())
def test_equals_matmul(case):
    """no bias: dfa.MatMul (trans_b, one matrix, the weights uploaded as B) gives the same bytes, dense and pitched"""
    import torch
    data = R.generate(case)
    got = check_case(case, data)[0]
    ldb = R.up(case.k, 16)
    b = np.zeros((case.n, ldb), dtype=np.int8)
    b[:, :case.k] = data["w"]
    mm = dfa.MatMul(1, case.rows, case.n, case.k, a_dtype=R.NP_OF[case.src_dt], dst_dtype=R.NP_OF[case.dst_dt], trans_b=True,
                    a_strides=(0, 0, case.sld), b_strides=(0, 0, ldb), c_strides=(0, 0, case.dld), relu=case.relu, rm=case.rm,
                    nscales=case.nscales, scales=data["scales"])
    try:
        src_dev = src_on_device(data)
        b_dev = torch.from_numpy(b.view(np.uint8).reshape(-1).copy()).cuda()
        buf, dst = guarded(dst_bytes(case))
        mm.submit(src_dev, b_dev, dst)
        torch.cuda.synchronize()
        same(dst.cpu().numpy(), got, case, "against " + mm.info().kernel_name.decode())
    finally:
        mm.close()
