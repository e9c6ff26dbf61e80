"""GPU: the batched int8 matrix product (dfx_bmm_*, dfa.MatMul) against the numpy reference of tests/bmm_ref.py, bit for bit
(tests/test_bmm_cpu.py pins that reference against a pure-Python witness and against fc_ref), and against the ops the library
already has: dfx_fc (dfa.InnerProduct) and the table softmax of dfx_head in an int8 attention chain.  Everything goes through
the C ABI.  C's whole storage sits between guard bands and is poisoned: the comparison of the whole storage shows that the
elements N .. ldc-1 of every row (and whatever lies between the matrices) are not written.  The pad columns of A hold 0xFF,
those of B random non-zero bytes.  The MFMA kernel is forced, on the fast and
on the exact route, then the generic kernel is forced: all against the one reference."""
import functools
import importlib
import threading

import numpy as np
import pytest

import bmm_ref as R
import head_ref as H
import hipref

pytestmark = pytest.mark.gpu
dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
GUARD = 1 << 12       # guard bytes on each side of C


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


def make_op(case, force_path, scales=None):
    return dfa.MatMul(case.batch, case.m, case.n, case.k, a_dtype=R.NP_OF[case.a_dt], dst_dtype=R.NP_OF[case.dst_dt], trans_b=case.trans_b,
                      a_strides=case.strides("a"), b_strides=case.strides("b"), c_strides=case.strides("c"), relu=case.relu, rm=case.rm,
                      nscales=case.n if case.per_channel else 1, force_path=force_path, scales=scales)


def c_bytes(case):
    return R.storage_elems(case, "c") * R.SIZE_OF[case.dst_dt]


def run(op, case, a_dev, b_dev, c_offset=0, stream=None):
    """one submit into a guarded, poisoned C -> C's whole storage as bytes"""
    import torch
    n = c_bytes(case)
    buf, c = guarded(n, c_offset)
    torch.cuda.synchronize()
    op.submit(a_dev, b_dev, c, stream=stream)
    torch.cuda.synchronize()
    assert_guards(buf, c_offset, n, case.ident())
    return c.cpu().numpy()


def same(got, want, case, what):
    """whole-storage comparison, reported per element of dst's dtype"""
    if not np.array_equal(got, want):
        dt = R.NP_OF[case.dst_dt]
        hipref.assert_bit_equal(got.view(dt), want.view(dt), "%s %s" % (case.ident(), what))


def check_case(case, data, paths=(R.MFMA, R.GENERIC), grid_cap=0, want=None):
    """the case on the forced MFMA kernel (the route the shape proves, then the exact route) and on the forced generic kernel;
    path, route, kernel name, grid, block, LDS and the algorithmic counts from the handle"""
    want = R.reference(case, data) if want is None else want
    a_dev, b_dev = on_device(data["a"]), on_device(data["b"])
    d = R.desc_of(case)
    outs = []
    for path in paths:
        op = make_op(case, path)
        try:
            routes = ((None, int(path == R.MFMA and R.fast_ok(d, data["scales"]))), ("1", 0)) if path == R.MFMA else ((None, 0),)
            for no_fast, route in routes:
                if no_fast:
                    capi.set_tuning("DFX_NO_FAST", no_fast)
                try:
                    op.set_scales(data["scales"])
                finally:
                    if no_fast:
                        capi.set_tuning("DFX_NO_FAST", None)
                info = op.info()
                what = "[%s]" % info.kernel_name.decode()
                assert info.path == path and op.requant() == route, (case.ident(), what, op.requant(), route)
                assert info.kernel_name.decode() == R.kernel_name(case, path, route), (case.ident(), what)
                assert info.grid == R.planned_grid(d, path, cus(), grid_cap) and info.block == 256, (case.ident(), what, info.grid)
                assert info.lds_bytes == R.lds_bytes(d, path), (case.ident(), what)
                assert info.algorithmic_ops == R.algorithmic_ops(d) and info.algorithmic_bytes == R.algorithmic_bytes(d), (case.ident(), what)
                before = dfa.bmm_launches()
                got = run(op, case, a_dev, b_dev)
                after = dfa.bmm_launches()
                assert [after[p] - before[p] for p in range(2)] == [int(p == path) for p in range(2)], (case.ident(), what)
                same(got, want, case, what)
                outs.append(got)
        finally:
            op.close()
    return outs


def chunks(cases, n):
    return [tuple(cases[i::n]) for i in range(n)]


# ---- 1. the shape grid -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", chunks(R.shape_grid(), 36), ids=lambda g: "grid%d" % len(g))
def test_shape_grid(group):
    """M, N in 1, 31, 32, 33, 65, 130 x K in 1, 15, 16, 17, 63, 64, 65, 96, 200, both forms, both A dtypes, the dst dtypes,
    ReLU, round modes, per-channel scales and C's alignment rotating; leading dimensions of A and B rounded up to 16"""
    for case in group:
        check_case(case, R.generate(case))


# ---- 2. batches and strides ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.batch_cases(), ids=lambda c: c.ident())
def test_batches_and_strides(case):
    """(1,1) and (2,3) batches; head-sliced A and B (dfa.attention_strides); C interleaved back into {bs, T, heads * d}, the
    bytes of the other heads checked as part of the whole tensor; B broadcast with a batch stride of 0"""
    hs = dfa.attention_strides(R.BS, R.HEADS, R.T, R.D, R.HEADS * R.D)
    assert hs == R.attention_strides(R.BS, R.HEADS, R.T, R.D) == (R.T * R.HEADS * R.D, R.D, R.HEADS * R.D)
    if case.name == "heads-qk":
        assert case.strides("a") == hs and case.strides("b") == hs
    if case.name == "heads-pv":
        assert case.strides("b") == hs and case.strides("c") == hs
    check_case(case, R.generate(case))


# ---- 3. the compensation of the u8 operand ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [200, R.KMAX])
def test_compensation(k):
    """u8 A all 255 / all 0 / random against B all -128 / all 127 / random at K = 200 and K = 65025 (M = N = 33, one batch):
    s32 dst and scale 1, so nothing is hidden by saturation; 255 * 127 * 65025 and 255 * -128 * 65025 are reached"""
    seen = 0
    for case, data in R.compensation_cases():
        if case.k != k:
            continue
        acc = R.accumulate(case, data["a"], data["b"])
        if case.name == "comp-a255-b127":
            assert (acc == 255 * 127 * k).all()
        if case.name == "comp-a255-b-128":
            assert (acc == 255 * -128 * k).all()
        check_case(case, data)
        seen += 1
    assert seen == 18


# ---- 4. the lane map -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans_b", [True, False], ids=["nt", "nn"])
def test_lane_map(trans_b):
    """A = identity-like rows and an asymmetric B ((3 n + 5 k) mod 251 - 125): C is B transposed, exactly"""
    case, data, want_vals = R.lane_map_case(trans_b)
    assert not np.array_equal(want_vals, want_vals.T)
    for got in check_case(case, data):
        vals = got.view(np.int32)[R.index(case, "c").reshape(-1)].reshape(case.m, case.n)
        hipref.assert_bit_equal(vals, want_vals, case.ident())


# ---- 5. ties and the conversion --------------------------------------------------------------------------------------------
def test_ties():
    """scale 0.5 on odd accumulators: nearest-even against floor on every value, u8 / s8 / s32 dst, both forms"""
    for case, data in R.tie_cases():
        acc = R.accumulate(case, data["a"], data["b"])
        assert (acc % 2 != 0).all()
        check_case(case, data)


@pytest.mark.parametrize("case", R.nonfinite_cases(), ids=lambda c: c.ident())
def test_nonfinite_scales_take_the_exact_route(case):
    """a scale of inf or NaN is never called fast; the exact route gives the x86 0x80000000 pattern and its saturations"""
    data = R.generate(case)
    assert not R.fast_ok(R.desc_of(case), data["scales"])
    vals = R.values(case, data)
    if case.dst_dt == R.S32:
        assert (vals == -2 ** 31).mean() > 0.4
    elif case.dst_dt == R.S8:
        assert (vals == -128).mean() > 0.4
    elif case.dst_dt == R.U8:
        assert (vals == 255).mean() > 0.4
    check_case(case, data)


# ---- 6. the grid cap -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("trans_b", [True, False], ids=["nt", "nn"])
def test_grid_cap(tuning, cap, trans_b):
    """DFX_BMM_GRID = 1 and 3 on 30 tiles (8 units of four): workgroups loop over several units, the last one ragged"""
    from dataclasses import replace
    case = replace(R.GRID_CAP_CASE, trans_b=trans_b)
    assert R.tiles(R.desc_of(case)) == 30
    tuning.setenv("DFX_BMM_GRID", cap)
    check_case(case, R.generate(case), grid_cap=cap)


def test_auto_follows_the_measured_rule():
    """the AUTO RULE of include/dfx.h (DFX_BMM_AUTO_NOTE): the MFMA kernel in its class from M 49, N 32, K 32,
    192 * 49 * 49 * 32 multiply-adds and 384 tiles of 32 x 32 on, the generic kernel below any of the five and outside the class"""
    K = R.BmmCase
    for case, path in ((K("auto", 49, 49, 32, batch=(64, 3), a_dt=R.S8), R.MFMA), (K("auto", 49, 32, 49, trans_b=False, batch=(64, 3)), R.MFMA),
                       (K("auto", 48, 49, 32, batch=(64, 3), a_dt=R.S8), R.GENERIC), (K("auto", 49, 49, 32, batch=(63, 3), a_dt=R.S8), R.GENERIC),
                       (K("auto", 197, 197, 31, batch=(8, 12)), R.GENERIC), (K("auto", 197, 31, 197, trans_b=False, batch=(8, 12)), R.GENERIC),
                       (K("auto", 49, 49, 32, batch=(64, 3), a_strides=(3 * 49 * 40, 49 * 40, 40)), R.GENERIC),
                       (K("auto", 49, 32, 20000), R.GENERIC),                      # 2 tiles under a deep K: never timed
                       (K("auto", 384, 1024, 64), R.MFMA), (K("auto", 384, 992, 64), R.GENERIC)):   # 384 and 372 tiles
        d = R.desc_of(case)
        assert R.auto_path(d) == path, case.ident()
        data = R.generate(case)
        op = make_op(case, -1, data["scales"])
        try:
            assert op.info().path == path, case.ident()
            same(run(op, case, on_device(data["a"]), on_device(data["b"])), R.reference(case, data), case, "auto")
        finally:
            op.close()


# ---- 7. the per-submit fallback --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans_b", [True, False], ids=["nt", "nn"])
def test_misaligned_operands_fall_back_to_generic_for_that_submit(trans_b):
    """a, then b, 4 bytes off a 16-byte boundary: the forced MFMA handle launches the generic kernel for that submit
    (dfx_debug_bmm_launches), info() keeps the plan, the bytes are the same; a misaligned C only loses the vector stores"""
    case = R.BmmCase("off", 33, 40, 50, trans_b=trans_b, a_dt=R.U8, dst_dt=R.S8, c_ld=48, seed=37000)
    data = R.generate(case)
    want = R.reference(case, data)
    op = make_op(case, R.MFMA, data["scales"])
    try:
        for off_a, off_b, off_c in ((4, 0, 0), (0, 4, 0), (0, 0, 1), (0, 0, 0)):
            before = dfa.bmm_launches()
            got = run(op, case, on_device(data["a"], off_a), on_device(data["b"], off_b), off_c)
            after = dfa.bmm_launches()
            ran = R.GENERIC if (off_a or off_b) else R.MFMA
            assert [after[p] - before[p] for p in range(2)] == [int(p == ran) for p in range(2)], (off_a, off_b, off_c)
            assert op.info().path == R.MFMA
            same(got, want, case, "offsets %d %d %d" % (off_a, off_b, off_c))
    finally:
        op.close()


# ---- 8. submit checks ------------------------------------------------------------------------------------------------------
def test_submit_checks_launch_nothing():
    """DFX_ERR_STATE before set_scales; a null pointer, a misaligned 4-byte C and a C that overlaps A or B are DFX_ERR_INVALID;
    nothing is launched, C keeps its poison and the guard bands are untouched"""
    import torch
    case = R.BmmCase("state", 33, 40, 50, a_dt=R.U8, dst_dt=R.S32, c_ld=40, seed=37100)
    data = R.generate(case)
    a_dev, b_dev = on_device(data["a"]), on_device(data["b"])
    for path in (R.MFMA, R.GENERIC):
        op = make_op(case, path)
        try:
            n = c_bytes(case)
            buf, c = guarded(n)
            before = dfa.bmm_launches()
            with pytest.raises(dfa.DfxError, match="dfx error 5"):
                op.submit(a_dev, b_dev, c)
            with pytest.raises(dfa.DfxError, match="dfx error 5"):
                op.requant()
            op.set_scales(data["scales"])
            for args in ((None, b_dev, c), (a_dev, None, c), (a_dev, b_dev, None)):
                with pytest.raises(dfa.DfxError, match="dfx error 1"):
                    capi._check(capi.lib().dfx_bmm_submit(op._h, *[None if x is None else capi._dev_ptr(x) for x in args], None))
            with pytest.raises(dfa.DfxError, match="dfx error 1"):
                op.submit(a_dev, b_dev, c[2:])                                    # a 4-byte C off its element
            # C over A: A sits in the middle of a guarded buffer large enough for C
            abuf, amid = guarded(max(n, a_dev.numel()) + 64)
            amid[:a_dev.numel()].copy_(a_dev)
            with pytest.raises(dfa.DfxError, match="overlaps"):
                op.submit(amid, b_dev, amid)
            d = R.desc_of(case)
            a_span = R.span(1, 1, 0, 0, d["lda"], case.m, case.k)                 # A's byte range ends behind its last VALID element
            with pytest.raises(dfa.DfxError, match="overlaps"):
                op.submit(amid, b_dev, amid[(a_span - 1) // 4 * 4:])              # C's first element over A's last byte
            with pytest.raises(dfa.DfxError, match="overlaps"):
                op.submit(a_dev, amid, amid[16:])                                 # C over B
            torch.cuda.synchronize()
            assert dfa.bmm_launches() == before
            assert_guards(buf, 0, n, "state")
            assert_guards(abuf, 0, amid.numel(), "state")
            assert bool((c == hipref.POISON_BYTE).all())
            assert bool((amid[:a_dev.numel()] == a_dev).all())
            op.submit(a_dev, b_dev, c)                                            # a valid submit still works
            torch.cuda.synchronize()
            same(c.cpu().numpy(), R.reference(case, data), case, "after the refusals")
        finally:
            op.close()


def test_two_streams_submit_one_handle_at_once():
    """no scratch, one launch with its own arguments: two host threads on two streams, one handle, the same bits"""
    import torch
    case = R.BmmCase("streams", 130, 130, 200, trans_b=False, a_dt=R.U8, dst_dt=R.S8, batch=(2, 3), c_ld=144, seed=37200)
    data = R.generate(case)
    want = R.reference(case, data)
    a_dev, b_dev = on_device(data["a"]), on_device(data["b"])
    for path in (R.MFMA, R.GENERIC):
        op = make_op(case, path, data["scales"])
        try:
            streams = [torch.cuda.Stream(), torch.cuda.Stream()]
            outs = [[guarded(c_bytes(case)) for _ in range(4)] for _ in streams]
            torch.cuda.synchronize()
            errors = []

            def work(i):
                try:
                    for _, c in outs[i]:
                        op.submit(a_dev, b_dev, c, stream=streams[i])
                except Exception as e:  # noqa: BLE001
                    errors.append(e)

            threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
            torch.cuda.synchronize()
            assert not errors, errors
            for per in outs:
                for buf, c in per:
                    assert_guards(buf, 0, c.numel(), "streams")
                    same(c.cpu().numpy(), want, case, "path %d" % path)
        finally:
            op.close()


# ---- 9. defining properties against the ops the library already has -----------------------------------------------------------
@pytest.mark.parametrize("k,m,n", R.FC_TWIN)
def test_equals_the_fully_connected_op(k, m, n):
    """batch 1, NT, u8 A: identical to dfa.InnerProduct with w = B, for every dst dtype, with relu on and off"""
    import torch
    for dst in R.DST_ROTATION:
        for relu in (False, True):
            case = R.BmmCase("fc", m, n, k, trans_b=True, a_dt=R.U8, dst_dt=dst, relu=relu, c_ld=n, seed=38000 + k + m + n)
            data = R.generate(case)
            assert case.strides("a")[2] == k and case.strides("b")[2] == k
            fc = dfa.InnerProduct((m, 1, 1, k), n, dst_dt=dst, bia_dt=dfa.DFX_UNDEF, relu=relu)
            try:
                fc.set_weights(data["b"].reshape(n, k, 1, 1), data["scales"])
                dst_dev = torch.empty(m * n * R.SIZE_OF[dst] + 16, dtype=torch.uint8, device="cuda")
                fc.submit(on_device(data["a"]), dst_dev)
                torch.cuda.synchronize()
                want = dst_dev.cpu().numpy()[:m * n * R.SIZE_OF[dst]]
            finally:
                fc.close()
            same(R.reference(case, data), want, case, "reference against dfx_fc")
            check_case(case, data, want=want)


@pytest.mark.parametrize("a_dt", [R.U8, R.S8], ids=["u8", "s8"])
def test_nn_equals_nt_on_the_transposed_operand(a_dt):
    """NN on B equals NT on B.T made contiguous on the host"""
    from dataclasses import replace
    nn = R.BmmCase("nn", 65, 70, 100, trans_b=False, a_dt=a_dt, dst_dt=R.S8, batch=(1, 2), c_ld=80, seed=38500)
    data = R.generate(nn)
    nt = replace(nn, trans_b=True)
    bt = np.swapaxes(data["b"][R.index(nn, "b")], 2, 3)                           # {1, 2, n, k}
    b_nt = np.full(R.storage_elems(nt, "b"), 0x55, dtype=np.uint8).view(np.int8)
    b_nt[R.index(nt, "b").reshape(-1)] = bt.reshape(-1)
    outs = check_case(nn, data) + check_case(nt, dict(data, b=b_nt))
    assert len({o.tobytes() for o in outs}) == 1


def test_attention_chain():
    """bs 2, heads 2, T 37 (logit rows 48 apart), d 32: MatMul (s8 x s8 -> s8), dfx_head's table softmax (u8, dst_ld 48),
    MatMul (u8 x s8 NN -> s8, K = 37 over rows 48 apart whose pad holds poison), the context interleaved back into
    {bs, T, heads * d}; against the same chain of bmm_ref and head_ref, tensor by tensor"""
    import torch
    bs, heads, t, d, ld = 2, 2, 37, 32, 48
    hs = dfa.attention_strides(bs, heads, t, d, heads * d)
    ls = (heads * t * ld, t * ld, ld)
    qk = R.BmmCase("chain-qk", t, t, d, trans_b=True, a_dt=R.S8, dst_dt=R.S8, batch=(bs, heads), a_strides=hs, b_strides=hs, c_strides=ls,
                   seed=39000)
    pv = R.BmmCase("chain-pv", t, d, t, trans_b=False, a_dt=R.U8, dst_dt=R.S8, batch=(bs, heads), a_strides=ls, b_strides=hs, c_strides=hs,
                   scale=1.0 / 256.0, seed=39001)
    qdata = R.generate(qk)                                                        # a = Q, b = K
    v = R.generate(pv)["b"]
    table = dfa.softmax_table(0.0625, t)
    rows = bs * heads * t
    # the reference chain
    logits = R.reference(qk, qdata)                                               # bytes, {bs, heads, T, 48} minus the last row's pad
    logits_full = np.full(rows * ld, hipref.POISON_BYTE, dtype=np.uint8)
    logits_full[:logits.size] = logits
    probs = H.reference_softmax(logits_full.view(np.int8).reshape(rows, ld), t, table, H.U8, 255.0)   # (rows, t) u8
    probs_full = np.full((rows, ld), hipref.POISON_BYTE, dtype=np.uint8)
    probs_full[:, :t] = probs
    pdata = dict(a=probs_full.reshape(-1), b=v, scales=R.make_scales(pv))
    context = R.reference(pv, pdata)
    assert 0.0 < (probs > 0).mean() and R.saturated_fraction(pv, R.values(pv, pdata)) < 0.1
    for path in (R.MFMA, R.GENERIC):
        op1, op2 = make_op(qk, path, qdata["scales"]), make_op(pv, path, pdata["scales"])
        sm = dfa.Softmax(rows, t, np.int8, np.uint8, table=table, src_ld=ld, dst_ld=ld)
        try:
            lbuf, ldev = guarded(rows * ld)
            pbuf, pdev = guarded(rows * ld)
            cbuf, cdev = guarded(c_bytes(pv))
            torch.cuda.synchronize()
            op1.submit(on_device(qdata["a"]), on_device(qdata["b"]), ldev)
            sm.submit(ldev, pdev)
            op2.submit(pdev, on_device(v), cdev)
            torch.cuda.synchronize()
            for buf, dev in ((lbuf, ldev), (pbuf, pdev), (cbuf, cdev)):
                assert_guards(buf, 0, dev.numel(), "chain")
            same(ldev.cpu().numpy(), logits_full, qk, "logits, path %d" % path)
            hipref.assert_bit_equal(pdev.cpu().numpy().reshape(rows, ld), probs_full, "probabilities, path %d" % path)
            same(cdev.cpu().numpy(), context, pv, "context, path %d" % path)
        finally:
            op1.close()
            op2.close()
            sm.close()
