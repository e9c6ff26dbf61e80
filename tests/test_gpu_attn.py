"""GPU: the fused int8 attention (dfx_attn_*, dfa.Attention) against the numpy reference of tests/attn_ref.py, bit for bit.  That
reference is nothing but bmm_ref -> head_ref's softmax -> bmm_ref (tests/test_attn_cpu.py pins it against the pure-Python
witnesses).  Everything goes through the C ABI.  O's whole storage sits between guard bands and is poisoned: the comparison of
the whole storage shows that the elements dv .. ldo-1 of every row (and whatever lies between the matrices) are not written.
Q's pad columns hold 0xFF, K's and V's random non-zero bytes.  The fused kernel is forced, on the routes the shape proves and
on the exact routes, then the chain is forced: all against the one reference."""
import functools
import importlib
import threading
from dataclasses import replace

import numpy as np
import pytest

import attn_ref as A
import bmm_ref as R
import hipref

pytestmark = pytest.mark.gpu
dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
GUARD = 1 << 12       # guard bytes on each side of O


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


def make_op(case, force_path, data=None):
    op = dfa.Attention(case.batch, case.tq, case.tk, case.d, case.dv, q_dtype=A.NP_OF[case.q_dt], dst_dtype=A.NP_OF[case.dst_dt],
                       q_strides=case.strides("q"), k_strides=case.strides("k"), v_strides=case.strides("v"), o_strides=case.strides("o"),
                       relu=case.relu, rm=case.rm, nscales=case.dv if case.per_channel else 1, prob_scale=case.prob_scale, force_path=force_path)
    if data is not None:
        op.set_table(data["table"])
        op.set_scales(data["logit_scale"][0], data["out_scales"])
    return op


def o_bytes(case):
    return A.storage_elems(case, "o") * A.SIZE_OF[case.dst_dt]


def run(op, case, dev, o_offset=0, stream=None):
    """one submit into a guarded, poisoned O -> O's whole storage as bytes"""
    import torch
    n = o_bytes(case)
    buf, o = guarded(n, o_offset)
    torch.cuda.synchronize()
    op.submit(dev["q"], dev["k"], dev["v"], o, stream=stream)
    torch.cuda.synchronize()
    assert_guards(buf, o_offset, n, case.ident())
    return o.cpu().numpy()


def same(got, want, case, what):
    """whole-storage comparison, reported per element of dst's dtype"""
    if not np.array_equal(got, want):
        dt = A.NP_OF[case.dst_dt]
        hipref.assert_bit_equal(got.view(dt), want.view(dt), "%s %s" % (case.ident(), what))


def to_device(data):
    return {w: on_device(data[w]) for w in "qkv"}


def check_case(case, data, paths=(A.FUSED, A.CHAIN), grid_cap=0, want=None):
    """the case on the forced fused kernel (the routes the shape proves, then both exact) and on the forced chain; path, routes,
    kernel name, grid, block, LDS, scratch and the algorithmic counts from the handle"""
    want = A.reference(case, data) if want is None else want
    dev = to_device(data)
    d = A.desc_of(case)
    outs = []
    for path in paths:
        op = make_op(case, path)
        try:
            op.set_table(data["table"])
            proved = (int(A.fast_logits(d, data["logit_scale"])), int(A.fast_context(d, data["out_scales"])))
            for no_fast, routes in ((None, proved), ("1", (0, 0))) if path == A.FUSED else ((None, proved),):
                if no_fast:
                    capi.set_tuning("DFX_NO_FAST", no_fast)
                try:
                    op.set_scales(data["logit_scale"][0], data["out_scales"])
                finally:
                    if no_fast:
                        capi.set_tuning("DFX_NO_FAST", None)
                info = op.info()
                what = "[%s]" % info.kernel_name.decode()
                assert info.path == path and op.requant() == routes, (case.ident(), what, op.requant(), routes)
                assert info.kernel_name.decode() == A.kernel_name(case, path, *routes), (case.ident(), what)
                if path == A.FUSED:
                    assert info.grid == A.planned_grid(d, cus(), grid_cap) and info.block == 256, (case.ident(), what, info.grid)
                    assert info.lds_bytes == A.lds_bytes(d), (case.ident(), what)
                else:
                    assert (info.grid, info.block, info.lds_bytes) == (0, 0, 0), (case.ident(), what)
                # (a fused handle holds no L / P until a submit falls back to the chain)
                assert info.scratch_bytes == (A.scratch_bytes(d) if path == A.CHAIN else 0), (case.ident(), what)
                assert info.algorithmic_ops == A.algorithmic_ops(d) and info.algorithmic_bytes == A.algorithmic_bytes(d), (case.ident(), what)
                before = dfa.attn_launches()
                got = run(op, case, dev)
                after = dfa.attn_launches()
                assert [after[p] - before[p] for p in range(2)] == [int(p == path) for p in range(2)], (case.ident(), what)
                same(got, want, case, what)
                outs.append(got)
        finally:
            op.close()
    return outs


def chunks(cases, n):
    return [tuple(cases[i::n]) for i in range(n)]


# ---- 1. the covering table -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", chunks(A.shape_grid(), 12), ids=lambda g: "grid%d" % len(g))
def test_shape_grid(group):
    """tq in 1, 31, 32, 33, 65 x tk in 1 .. 200 x d in 1 .. 256 x dv in 1 .. 130, every value of an axis against at least two of
    each other axis; both Q dtypes, the dst dtypes, ReLU, round modes, per-channel out scales and O's alignment rotating"""
    for case in group:
        check_case(case, A.generate(case))


# ---- 2. batches and strides ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", A.batch_cases(), ids=lambda c: c.ident())
def test_batches_and_strides(case):
    """(2,3) batches; (bs 2, heads 2, T 37, d 32) head-sliced with the context interleaved back into {bs, T, heads * d}, the bytes
    of the other heads checked as part of the whole tensor; K and V broadcast with batch strides of 0"""
    if case.name == "heads":
        hs = dfa.attention_strides(A.BS, A.HEADS, A.T, A.D)
        assert all(case.strides(w) == hs for w in "qkvo")
    check_case(case, A.generate(case))


# ---- 3. softmax edges, ties, non-finite scales -------------------------------------------------------------------------------
def test_softmax_edges():
    """a row of equal logits (S = tk * E[0]); logits on both saturation bounds (distance 255), also with a table whose E[255]
    is 0; tk = 1, where P = 255 against all -128 / all 127 V with s32 out: the u8 compensation's extreme"""
    seen = set()
    for case, data in A.softmax_edge_cases():
        logits, probs, _ = A.chain(case, data)
        lv = logits[:, :case.tk]
        if case.name == "equal":
            assert (lv == 0).all() and len(np.unique(probs[:, :case.tk])) == 1
        if case.name.startswith("bounds"):
            assert (lv.max(axis=1) == 127).all() and (lv.min(axis=1) == -128).all()
        if case.name.startswith("tk1"):
            assert (probs[:, :1] == 255).all()
            fill = -128 if "v-128" in case.name else 127
            assert (A.o_values(case, data, probs) == 255 * fill).all()
        seen.add(case.name)
        check_case(case, data)
    assert seen == {"equal", "bounds", "bounds-e255", "tk1-v-128", "tk1-v127"}


def test_ties():
    """scale 0.5 on odd accumulators of the context (tk = 1, P = 1) and of the logits: nearest-even against floor"""
    for case, data in A.tie_cases():
        acc = R.accumulate(A.qk_case(case), data["q"], data["k"]) if case.name == "ties-logits" else \
            R.accumulate(A.pv_case(case), A.chain(case, data)[1].reshape(-1), data["v"])
        assert (acc % 2 != 0).all(), case.ident()
        check_case(case, data)


@pytest.mark.parametrize("case", A.nonfinite_cases(), ids=lambda c: c.ident())
def test_nonfinite_scales_take_the_exact_route(case):
    """a logit or out scale of inf or NaN is never called fast; the exact route gives the x86 0x80000000 pattern's saturations"""
    data = A.generate(case)
    d = A.desc_of(case)
    assert not (A.fast_logits(d, data["logit_scale"]) and A.fast_context(d, data["out_scales"]))
    check_case(case, data)


# ---- 4. the class bound, the grid cap, the auto rule ---------------------------------------------------------------------------
def test_class_bound():
    """tk at the plan's maximum (tq 33, d 16, dv 32, one matrix: the strip takes 141.5 KiB of LDS); at maximum + 1 auto plans the
    chain and a forced fused path is DFX_ERR_UNSUPPORTED"""
    case = A.CLASS_BOUND_CASE
    assert case.tk == A.TK_MAX and A.fused_class(A.desc_of(case)) and A.lds_bytes(A.desc_of(case)) == 144896
    check_case(case, A.generate(case))
    over = replace(case, tk=A.TK_MAX + 1)
    assert not A.fused_class(A.desc_of(over))
    with pytest.raises(dfa.DfxError, match="dfx error 2"):
        make_op(over, A.FUSED)
    data = A.generate(over)
    op = make_op(over, -1, data)
    try:
        assert op.info().path == A.CHAIN
        same(run(op, over, to_device(data)), A.reference(over, data), over, "auto")
    finally:
        op.close()


@pytest.mark.parametrize("cap", [1, 3])
def test_grid_cap(tuning, cap):
    """DFX_ATTN_GRID = 1 and 3 on a dozen strips: workgroups loop over several strips and reuse their LDS"""
    case = A.GRID_CAP_CASE
    assert A.strips(A.desc_of(case)) == 12
    tuning.setenv("DFX_ATTN_GRID", cap)
    check_case(case, A.generate(case), paths=(A.FUSED,), grid_cap=cap)


def test_auto_follows_the_measured_rule():
    """the AUTO RULE of include/dfx.h (DFX_ATTN_AUTO_NOTE) at both sides of each of its bounds: the fused kernel in its class for
    tq >= 49, tk in 49 .. 850, d and dv in 32 .. 64 and at least 384 strips, the chain below or above any of them and outside
    the class; both give the reference's bits"""
    for case, path in A.auto_cases():
        d = A.desc_of(case)
        assert A.auto_path(d) == path, case.ident()
        data = A.generate(case)
        op = make_op(case, -1, data)
        try:
            assert op.info().path == path, case.ident()
            before = dfa.attn_launches()
            got = run(op, case, to_device(data))
            after = dfa.attn_launches()
            assert [after[p] - before[p] for p in range(2)] == [int(p == path) for p in range(2)], case.ident()
            same(got, A.reference(case, data), case, "auto")
        finally:
            op.close()
    outside = A.AttnCase("auto", 65, 70, A.D_MAX + 1, 64, batch=(2, 2), seed=57050)
    assert not A.fused_class(A.desc_of(outside))
    with pytest.raises(dfa.DfxError, match="dfx error 2"):
        make_op(outside, A.FUSED)


# ---- 5. the per-submit fallback, submit checks, streams ------------------------------------------------------------------------
def test_misaligned_operands_fall_back_to_the_chain_for_that_submit():
    """q, then k, then v 4 bytes off a 16-byte boundary: the forced fused handle runs the chain for that submit
    (dfx_debug_attn_launches), info() keeps the plan, the bytes are the same; a misaligned O only loses the vector stores"""
    case = A.OFFSET_CASE
    data = A.generate(case)
    want = A.reference(case, data)
    op = make_op(case, A.FUSED, data)
    fell_back = False
    try:
        for offs in ((0, 0, 0, 0), (4, 0, 0, 0), (0, 4, 0, 0), (0, 0, 4, 0), (0, 0, 0, 1), (0, 0, 0, 0)):
            dev = {w: on_device(data[w], off) for w, off in zip("qkv", offs)}
            before = dfa.attn_launches()
            got = run(op, case, dev, offs[3])
            after = dfa.attn_launches()
            ran = A.CHAIN if any(offs[:3]) else A.FUSED
            assert [after[p] - before[p] for p in range(2)] == [int(p == ran) for p in range(2)], offs
            assert op.info().path == A.FUSED
            fell_back = fell_back or ran == A.CHAIN                                 # the chain and its scratch are made then
            assert op.info().scratch_bytes == (A.scratch_bytes(A.desc_of(case)) if fell_back else 0), offs
            same(got, want, case, "offsets %s" % (offs,))
    finally:
        op.close()


def test_submit_checks_launch_nothing():
    """DFX_ERR_STATE before set_table / set_scales; a null pointer, a misaligned 4-byte O and an O that overlaps Q, K or V are
    DFX_ERR_INVALID; a table that could overflow the sum is refused; nothing is launched, O keeps its poison"""
    import torch
    case = A.STATE_CASE
    data = A.generate(case)
    dev = to_device(data)
    for path in (A.FUSED, A.CHAIN):
        op = make_op(case, path)
        try:
            n = o_bytes(case)
            buf, o = guarded(n)
            before = dfa.attn_launches()
            assert op.requant() == (-1, -1)
            with pytest.raises(dfa.DfxError, match="dfx error 5"):
                op.submit(dev["q"], dev["k"], dev["v"], o)
            op.set_table(data["table"])
            with pytest.raises(dfa.DfxError, match="dfx error 5"):
                op.submit(dev["q"], dev["k"], dev["v"], o)
            op.set_scales(data["logit_scale"][0], data["out_scales"])
            bad = data["table"].copy()
            bad[0] = 0
            with pytest.raises(dfa.DfxError, match="dfx error 1"):
                op.set_table(bad)
            with pytest.raises(dfa.DfxError, match="dfx error 1"):
                op.set_table(np.full(256, 2 ** 32 // case.tk + 1, dtype=np.uint32))
            for hole in range(4):
                args = [dev["q"], dev["k"], dev["v"], o]
                args[hole] = None
                with pytest.raises(dfa.DfxError, match="dfx error 1"):
                    capi._check(capi.lib().dfx_attn_submit(op._h, *[None if x is None else capi._dev_ptr(x) for x in args], None))
            with pytest.raises(dfa.DfxError, match="dfx error 1"):
                op.submit(dev["q"], dev["k"], dev["v"], o[2:])                     # a 4-byte O off its element
            for which in "qkv":
                src = dev[which]
                abuf, amid = guarded(max(n, src.numel()) + 64)
                amid[:src.numel()].copy_(src)
                args = dict(dev, **{which: amid})
                with pytest.raises(dfa.DfxError, match="overlaps"):
                    op.submit(args["q"], args["k"], args["v"], amid)
            torch.cuda.synchronize()
            assert dfa.attn_launches() == before
            assert_guards(buf, 0, n, "state")
            assert bool((o == hipref.POISON_BYTE).all())
            op.submit(dev["q"], dev["k"], dev["v"], o)                             # a valid submit still works
            torch.cuda.synchronize()
            same(o.cpu().numpy(), A.reference(case, data), case, "after the refusals")
        finally:
            op.close()


def test_two_streams_submit_one_handle_at_once():
    """two host threads on two streams, one handle, on both paths: the fused launches are independent; the chain's submits share
    L and P and are serialised on the device by the handle"""
    import torch
    case = A.STREAMS_CASE
    data = A.generate(case)
    want = A.reference(case, data)
    dev = to_device(data)
    for path in (A.FUSED, A.CHAIN):
        op = make_op(case, path, data)
        try:
            streams = [torch.cuda.Stream(), torch.cuda.Stream()]
            outs = [[guarded(o_bytes(case)) for _ in range(4)] for _ in streams]
            torch.cuda.synchronize()
            errors = []

            def work(i):
                try:
                    for _, o in outs[i]:
                        op.submit(dev["q"], dev["k"], dev["v"], o, stream=streams[i])
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
                for buf, o in per:
                    assert_guards(buf, 0, o.numel(), "streams")
                    same(o.cpu().numpy(), want, case, "path %d" % path)
        finally:
            op.close()


# ---- 6. the defining property: the three ops run by the test itself ---------------------------------------------------------------
@pytest.mark.parametrize("q_dt", [A.S8, A.U8], ids=["s8", "u8"])
def test_fused_equals_chain_equals_the_three_ops(q_dt):
    """FUSED == CHAIN == dfa.MatMul -> dfa.Softmax -> dfa.MatMul run here over the head-sliced tensors, O's whole storage"""
    import torch
    case = A.three_ops_case(q_dt)
    assert all(case.strides(w) == dfa.attention_strides(A.BS, A.HEADS, A.T, A.D) for w in "qkvo")
    data = A.generate(case)
    dev = to_device(data)
    qk, pv = A.qk_case(case), A.pv_case(case)
    rows, ld = case.g * case.tq, case.ldl
    mk = lambda c, s: dfa.MatMul(c.batch, c.m, c.n, c.k, a_dtype=R.NP_OF[c.a_dt], dst_dtype=R.NP_OF[c.dst_dt], trans_b=c.trans_b,  # noqa: E731
                                 a_strides=c.strides("a"), b_strides=c.strides("b"), c_strides=c.strides("c"), relu=c.relu, rm=c.rm, scales=s)
    op1, op2 = mk(qk, data["logit_scale"]), mk(pv, data["out_scales"])
    sm = dfa.Softmax(rows, case.tk, np.int8, np.uint8, table=data["table"], src_ld=ld, dst_ld=ld)
    try:
        _, ldev = guarded(rows * ld)
        _, pdev = guarded(rows * ld)
        obuf, odev = guarded(o_bytes(case))
        torch.cuda.synchronize()
        op1.submit(dev["q"], dev["k"], ldev)
        sm.submit(ldev, pdev)
        op2.submit(pdev, dev["v"], odev)
        torch.cuda.synchronize()
        assert_guards(obuf, 0, odev.numel(), "three ops")
        three = odev.cpu().numpy()
    finally:
        op1.close()
        op2.close()
        sm.close()
    same(three, A.reference(case, data), case, "the three ops against the reference")
    outs = check_case(case, data, want=three)
    assert len(outs) == 3 and len({o.tobytes() for o in outs}) == 1
