"""GPU: the logit bias of the int8 attention (dfx_attn_set_bias, dfa.Attention.set_bias) against the numpy reference of
tests/attn_bias_ref.py, bit for bit: the biased matrix product -> head_ref's softmax -> bmm_ref's product
(tests/test_attn_bias_cpu.py pins it against the witnesses).  The harness is test_gpu_attn's: O's whole storage between guard
bands and poisoned.  The fused kernel is forced, on the routes the shape and the bias prove and on the exact routes, then the
chain is forced, then the three Python ops (MatMul with the bias -> Softmax -> MatMul) run here: all against the one reference."""
import importlib
import threading

import numpy as np
import pytest

import attn_bias_ref as R
import attn_ref as A
import bmm_ref as B
import hipref
import test_gpu_attn as G

pytestmark = pytest.mark.gpu
dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")


def set_bias(op, bias, bd):
    op.set_bias(bd["table"], periods=bias.periods, strides=bd["layout"])


def routes_of(case, data, bias, bd):
    return int(R.attn_fast_logits(case, data, bias, bd)), int(A.fast_context(A.desc_of(case), data["out_scales"]))


def check_case(case, data, bias, bd, paths=(A.FUSED, A.CHAIN), want=None):
    """the biased case on the forced fused kernel (the routes proved with the bias, then both exact) and on the forced chain"""
    want = R.attn_reference(case, data, bias, bd) if want is None else want
    dev = G.to_device(data)
    d = A.desc_of(case)
    proved = routes_of(case, data, bias, bd)
    outs = []
    for path in paths:
        op = G.make_op(case, path)
        try:
            op.set_table(data["table"])
            set_bias(op, bias, bd)                                                  # before the scales
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
                assert info.kernel_name.decode() == A.kernel_name(case, path, *routes) + " +bias", (case.ident(), what)
                assert info.lds_bytes == (A.lds_bytes(d) if path == A.FUSED else 0), (case.ident(), what)       # the LDS plan does not change
                assert info.algorithmic_bytes == A.algorithmic_bytes(d) + R.distinct_bytes(A.bmm_desc_logits(d), R.layout_dict(bias, case.tq, case.tk)), what
                before = dfa.attn_launches()
                got = G.run(op, case, dev)
                after = dfa.attn_launches()
                assert [after[p] - before[p] for p in range(2)] == [int(p == path) for p in range(2)], (case.ident(), what)
                G.same(got, want, case, what + " biased")
                outs.append(got)
        finally:
            op.close()
    return outs


def three_ops(case, data, bias, bd):
    """dfa.MatMul with the bias -> dfa.Softmax -> dfa.MatMul run here -> (P {G*tq, ldl} uint8, O's whole storage)"""
    import torch
    dev = G.to_device(data)
    qk, pv = A.qk_case(case), A.pv_case(case)
    rows, ld = case.g * case.tq, case.ldl
    mk = lambda c, s, **kw: dfa.MatMul(c.batch, c.m, c.n, c.k, a_dtype=B.NP_OF[c.a_dt], dst_dtype=B.NP_OF[c.dst_dt], trans_b=c.trans_b,  # noqa: E731
                                       a_strides=c.strides("a"), b_strides=c.strides("b"), c_strides=c.strides("c"), relu=c.relu, rm=c.rm,
                                       nscales=len(s), scales=s, **kw)
    op1 = mk(qk, data["logit_scale"], bias=(bd["table"], bias.periods, bd["layout"]))
    op2 = mk(pv, data["out_scales"])
    sm = dfa.Softmax(rows, case.tk, np.int8, np.uint8, table=data["table"], src_ld=ld, dst_ld=ld)
    try:
        _, ldev = G.guarded(rows * ld)
        _, pdev = G.guarded(rows * ld)
        obuf, odev = G.guarded(G.o_bytes(case))
        torch.cuda.synchronize()
        op1.submit(dev["q"], dev["k"], ldev)
        sm.submit(ldev, pdev)
        op2.submit(pdev, dev["v"], odev)
        torch.cuda.synchronize()
        G.assert_guards(obuf, 0, odev.numel(), "three ops")
        return pdev.cpu().numpy().reshape(rows, ld), odev.cpu().numpy()
    finally:
        op1.close()
        op2.close()
        sm.close()


# ---- 1. the defining property on the issue's four shapes ---------------------------------------------------------------------------
@pytest.mark.parametrize("case,bias", R.attn_cases(), ids=lambda c: c.ident() if hasattr(c, "ident") else c.mask)
def test_fused_equals_chain_equals_the_three_ops_equals_numpy(case, bias):
    """Swin 49 x 49, d 32, batch (4,3), periods (2,3) with the shifted-window mask; tq 33, tk 70, d 40, dv 24 (tails, split keys);
    tk 197, d 64 with a key-padding row (ld = 0); a causal 40 x 40.  The finite mask (fast logits) and -inf (exact logits) give
    the same bits on every path."""
    data = A.generate(case)
    bd = R.attn_bias_data(case, data, bias)
    want = R.attn_reference(case, data, bias, bd)
    probs, three = three_ops(case, data, bias, bd)
    G.same(three, want, case, "the three ops against the reference")
    assert np.array_equal(probs[:, :case.tk], R.attn_chain(case, data, bias, bd)[1][:, :case.tk])
    outs = check_case(case, data, bias, bd, want=three)
    assert len(outs) == 3 and len({o.tobytes() for o in outs}) == 1
    assert routes_of(case, data, bias, bd)[0] == 1                                   # the finite mask: the fast route, proved
    ninf = R.with_ninf(bias)
    nd = R.attn_bias_data(case, data, ninf)
    assert routes_of(case, data, ninf, nd)[0] == 0 and np.isneginf(nd["values"]).any()
    for o in check_case(case, data, ninf, nd, want=three):                           # -inf: the exact route, the same bits
        assert o.tobytes() == three.tobytes()


def test_a_fully_masked_row_is_uniform():
    """row 0 of every matrix masks all 70 keys: every logit is -128, the probabilities are uniform (torch: NaN), O is the
    requantised mean of V; finite mask and -inf alike"""
    case, bias = R.FULL_ROW
    data = A.generate(case)
    for b in (bias, R.with_ninf(bias)):
        bd = R.attn_bias_data(case, data, b)
        probs, three = three_ops(case, data, b, bd)
        rows0 = probs[::case.tq, :case.tk]
        assert rows0.shape == (case.g, case.tk) and len(np.unique(rows0)) == 1 and rows0[0, 0] > 0
        check_case(case, data, b, bd, want=three)
        G.same(three, R.attn_reference(case, data, b, bd), case, "fully masked rows")


# ---- 2. the setters ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [A.FUSED, A.CHAIN], ids=["fused", "chain"])
def test_clear_reset_and_both_setter_orders(path):
    """set_bias(None) gives the unbiased bits back; another table replaces the first; set_bias after set_scales proves the logits'
    route again; a refused table leaves the handle as it was"""
    case, bias = R.attn_cases()[1]
    data = A.generate(case)
    bd = R.attn_bias_data(case, data, bias)
    other = R.Bias(periods=(1, 1), one_row=True, mask="keypad", mask_value="ninf", seed=76000)
    od = R.attn_bias_data(case, data, other)
    dev = G.to_device(data)
    plain = A.reference(case, data)
    op = G.make_op(case, path, data)
    try:
        assert op.requant()[0] == 1
        G.same(G.run(op, case, dev), plain, case, "before any bias")
        set_bias(op, bias, bd)                                                       # after the scales
        assert op.requant()[0] == 1 and op.info().kernel_name.decode().endswith(" +bias")
        G.same(G.run(op, case, dev), R.attn_reference(case, data, bias, bd), case, "set after the scales")
        set_bias(op, other, od)
        assert op.requant()[0] == 0
        G.same(G.run(op, case, dev), R.attn_reference(case, data, other, od), case, "set again")
        bad = od["table"].copy()
        bad[-1] = np.nan
        for table, periods, strides in ((bad, other.periods, od["layout"]), (np.zeros(4096, dtype=np.float32), (2, 1), od["layout"]),
                                        (np.zeros(4096, dtype=np.float32), (1, 1), (0, 0, case.tk - 1))):
            with pytest.raises(dfa.DfxError, match="dfx error 1"):
                op.set_bias(table, periods=periods, strides=strides)
        G.same(G.run(op, case, dev), R.attn_reference(case, data, other, od), case, "after the refusals")
        op.set_scales(data["logit_scale"][0], data["out_scales"])
        assert op.requant()[0] == 0                                                  # the scales again: -inf keeps the exact route
        op.set_bias(None)
        assert op.requant()[0] == 1 and op.info().kernel_name.decode() == A.kernel_name(case, path, *op.requant())
        assert op.info().algorithmic_bytes == A.algorithmic_bytes(A.desc_of(case))
        G.same(G.run(op, case, dev), plain, case, "cleared")
    finally:
        op.close()
    op = dfa.Attention(case.batch, case.tq, case.tk, case.d, case.dv, q_dtype=A.NP_OF[case.q_dt], dst_dtype=A.NP_OF[case.dst_dt], force_path=path,
                       q_strides=case.strides("q"), k_strides=case.strides("k"), v_strides=case.strides("v"), o_strides=case.strides("o"),
                       table=data["table"], logit_scale=data["logit_scale"][0], out_scales=data["out_scales"], bias=(bd["values"], bias.periods))
    try:
        G.same(G.run(op, case, dev), R.attn_reference(case, data, bias, bd), case, "bias= keyword")
    finally:
        op.close()


# ---- 3. the grid cap, the per-submit fallback, streams, the auto rule --------------------------------------------------------------------
def test_grid_cap_of_one(tuning):
    """DFX_ATTN_GRID = 1: one workgroup walks the strips of all four matrices and so changes its bias table on the way"""
    case, bias = R.GRID_CAP
    assert A.strips(A.desc_of(case)) == 12 and bias.periods == (2, 2)
    tuning.setenv("DFX_ATTN_GRID", 1)
    data = A.generate(case)
    bd = R.attn_bias_data(case, data, bias)
    op = G.make_op(case, A.FUSED, data)
    try:
        assert op.info().grid == 1
    finally:
        op.close()
    check_case(case, data, bias, bd, paths=(A.FUSED,))


def test_a_misaligned_q_falls_back_to_the_chain_with_the_bias():
    """a forced fused handle with a bias: Q 4 bytes off a 16-byte boundary runs the chain for that submit -- the chain the handle
    makes then gets the table, the scales AND the bias -- and gives the same bytes; a bias set after that reaches both"""
    case, bias = R.OFFSET
    data = A.generate(case)
    bd = R.attn_bias_data(case, data, bias)
    want = R.attn_reference(case, data, bias, bd)
    op = G.make_op(case, A.FUSED, data)
    try:
        set_bias(op, bias, bd)
        for off, ran in ((0, A.FUSED), (4, A.CHAIN), (0, A.FUSED)):
            dev = {w: G.on_device(data[w], off if w == "q" else 0) for w in "qkv"}
            before = dfa.attn_launches()
            got = G.run(op, case, dev)
            after = dfa.attn_launches()
            assert [after[p] - before[p] for p in range(2)] == [int(p == ran) for p in range(2)], off
            assert op.info().path == A.FUSED
            G.same(got, want, case, "q offset %d" % off)
        other = R.Bias(periods=(1, 1), mask="random", seed=77000)                   # the chain exists now: set_bias forwards to it
        od = R.attn_bias_data(case, data, other)
        set_bias(op, other, od)
        for off in (4, 0):
            dev = {w: G.on_device(data[w], off if w == "q" else 0) for w in "qkv"}
            G.same(G.run(op, case, dev), R.attn_reference(case, data, other, od), case, "another table, q offset %d" % off)
        op.set_bias(None)
        dev = {w: G.on_device(data[w], 4 if w == "q" else 0) for w in "qkv"}
        G.same(G.run(op, case, dev), A.reference(case, data), case, "cleared, on the chain")
    finally:
        op.close()


def test_two_streams_submit_one_biased_handle_at_once():
    import torch
    case, bias = R.STREAMS
    data = A.generate(case)
    bd = R.attn_bias_data(case, data, bias)
    want = R.attn_reference(case, data, bias, bd)
    dev = G.to_device(data)
    for path in (A.FUSED, A.CHAIN):
        op = G.make_op(case, path, data)
        try:
            set_bias(op, bias, bd)
            streams = [torch.cuda.Stream(), torch.cuda.Stream()]
            outs = [[G.guarded(G.o_bytes(case)) for _ in range(3)] for _ in streams]
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
                    G.assert_guards(buf, 0, o.numel(), "streams")
                    G.same(o.cpu().numpy(), want, case, "path %d" % path)
        finally:
            op.close()


def test_biased_auto_follows_the_measured_rule():
    """the rule recorded in include/dfx.h (DFX_ATTN_AUTO_NOTE) and DESIGN.md section 4.22: the biased fused kernel won against the
    biased chain at every point of the unbiased rule's box and lost where the unbiased one loses, so a bias does not change a
    handle's plan: the Swin stage on auto stays on the fused kernel with a bias set and after it is cleared, a shape below the box
    stays on the chain; a forced fused handle stays fused"""
    below, bbias = R.attn_cases()[3]                                                 # the causal 40 x 40: below the box
    assert A.auto_path(A.desc_of(below)) == A.CHAIN
    bdata = A.generate(below)
    bbd = R.attn_bias_data(below, bdata, bbias)
    op = G.make_op(below, -1, bdata)
    try:
        set_bias(op, bbias, bbd)
        assert op.info().path == A.CHAIN and op.info().kernel_name.decode().startswith("attn_chain")
        before = dfa.attn_launches()
        got = G.run(op, below, G.to_device(bdata))
        assert [dfa.attn_launches()[p] - before[p] for p in range(2)] == [0, 1]
        G.same(got, R.attn_reference(below, bdata, bbias, bbd), below, "auto below the box, biased")
    finally:
        op.close()
    case, bias = R.AUTO
    assert A.auto_path(A.desc_of(case)) == A.FUSED
    data = A.generate(case)
    bd = R.attn_bias_data(case, data, bias)
    dev = G.to_device(data)
    op = G.make_op(case, -1, data)
    try:
        for biased, path in ((False, A.FUSED), (True, A.FUSED), (False, A.FUSED)):
            if biased:
                set_bias(op, bias, bd)
            else:
                op.set_bias(None)
            info = op.info()
            assert info.path == path and info.kernel_name.decode().startswith("attn_fused" if path == A.FUSED else "attn_chain"), info.kernel_name
            before = dfa.attn_launches()
            got = G.run(op, case, dev)
            after = dfa.attn_launches()
            assert [after[p] - before[p] for p in range(2)] == [int(p == path) for p in range(2)], biased
            G.same(got, R.attn_reference(case, data, bias if biased else None, bd), case, "auto, biased %d" % biased)
    finally:
        op.close()
    forced = G.make_op(case, A.FUSED, data)
    try:
        set_bias(forced, bias, bd)
        assert forced.info().path == A.FUSED
        G.same(G.run(forced, case, dev), R.attn_reference(case, data, bias, bd), case, "forced fused, biased")
    finally:
        forced.close()
    assert hipref.POISON_BYTE == A.POISON
