"""GPU: the logit bias of the batched int8 matrix product (dfx_bmm_set_bias, dfa.MatMul.set_bias) against the numpy reference of
tests/attn_bias_ref.py, bit for bit (tests/test_attn_bias_cpu.py pins that reference against its witness).  The harness is
test_gpu_bmm's: C's whole storage between guard bands and poisoned, A's pad columns 0xFF, B's random non-zero bytes.  The host
table holds NaN in every float its layout does not address.  The MFMA kernel is forced, on the route the shape and the bias
prove and on the exact route, then the generic kernel is forced: all against the one reference."""
import importlib

import numpy as np
import pytest

import attn_bias_ref as R
import bmm_ref as B
import test_gpu_bmm as G

pytestmark = pytest.mark.gpu
dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")


def bias_of(case, data, bias):
    return R.make_bias(bias, case.m, case.n, data["scales"][0], R.acc_bound(case.a_dt, case.k))


def set_bias(op, bias, bd):
    op.set_bias(bd["table"], periods=bias.periods, strides=bd["layout"])


def check_case(case, data, bias, bd, paths=(B.MFMA, B.GENERIC)):
    """the biased case on the forced MFMA kernel (the route proved with the bias, then the exact route) and on the forced generic
    kernel; the route, the name's suffix and the table's bytes from the handle"""
    want = R.bmm_reference(case, data, bias, bd)
    a_dev, b_dev = G.on_device(data["a"]), G.on_device(data["b"])
    d = B.desc_of(case)
    proved = int(R.bmm_fast(case, data, bias, bd))
    outs = []
    for path in paths:
        op = G.make_op(case, path)
        try:
            set_bias(op, bias, bd)                                                  # before the scales: set_scales proves the route with it
            for no_fast, route in (((None, proved), ("1", 0)) if path == B.MFMA else ((None, 0),)):
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
                assert info.kernel_name.decode() == B.kernel_name(case, path, route) + " +bias", (case.ident(), what)
                assert info.algorithmic_bytes == B.algorithmic_bytes(d) + R.distinct_bytes(d, R.layout_dict(bias, case.m, case.n)), (case.ident(), what)
                before = dfa.bmm_launches()
                got = G.run(op, case, a_dev, b_dev)
                after = dfa.bmm_launches()
                assert [after[p] - before[p] for p in range(2)] == [int(p == path) for p in range(2)], (case.ident(), what)
                G.same(got, want, case, what + " biased")
                outs.append(got)
        finally:
            op.close()
    return outs


# ---- 1. every tail, both forms, both A dtypes, every dst, vector and element stores ----------------------------------------------
@pytest.mark.parametrize("group", G.chunks(R.bmm_tail_cases(), 4), ids=lambda g: "tails%d" % len(g))
def test_every_tail_form_and_dst(group):
    """m 33, n 37, k 40, batch (2,3): NT and NN, A u8 / s8, all four dst types, C's rows 41 (element stores) and 48 (vector stores)
    apart; periods, one-row tables, ReLU, round modes, per-channel scales and a random finite mask rotate"""
    for case, bias in group:
        data = B.generate(case)
        check_case(case, data, bias, bias_of(case, data, bias))


# ---- 2. periods, layouts, n = 1 and m = 1, -inf, several tiles -----------------------------------------------------------------
@pytest.mark.parametrize("case,bias", R.bmm_layout_cases(), ids=lambda c: c.ident() if hasattr(c, "ident") else "p%dx%d-row%d" % (c.periods + (c.one_row,)))
def test_periods_layouts_and_edges(case, bias):
    """batch (2,3) with periods (1,1), (1,3), (2,1), (2,3), whole tables and one row (ld = 0); host strides with gaps (NaN between
    the rows and the tables) and tables that share their floats (s0 = 0); n = 1 and m = 1; -inf entries (the exact route: -128 on
    s8, the x86 pattern on s32, 0 behind u8's ReLU); 3 x 5 tiles per matrix with a causal mask"""
    data = B.generate(case)
    bd = bias_of(case, data, bias)
    if bias.mask_value == "ninf":
        assert not R.bmm_fast(case, data, bias, bd) and np.isneginf(bd["values"]).any()
    if bias.strides is not None and bias.strides[0] != 0:
        assert np.isnan(bd["table"]).any()
    check_case(case, data, bias, bd)


# ---- 3. the setters: clear, set again, either order, refusals --------------------------------------------------------------------
def test_clear_reset_and_both_setter_orders():
    """set_bias(None) gives the unbiased bits and name back; another table replaces the first; set_bias after set_scales proves the
    route again (a -inf table drops a fast handle to exact, a finite one brings it back); a refused table leaves the handle as it was"""
    case, bias = R.bmm_layout_cases()[3]                                             # periods (1,3), one row
    assert bias.periods == (1, 3) and bias.one_row
    data = B.generate(case)
    bd = bias_of(case, data, bias)
    other = R.Bias(periods=(2, 3), mask="random", mask_value="ninf", seed=75000)
    od = bias_of(case, data, other)
    a_dev, b_dev = G.on_device(data["a"]), G.on_device(data["b"])
    plain = B.reference(case, data)
    op = G.make_op(case, B.MFMA, data["scales"])
    try:
        assert op.requant() == 1 and "+bias" not in op.info().kernel_name.decode()
        G.same(G.run(op, case, a_dev, b_dev), plain, case, "before any bias")
        set_bias(op, bias, bd)                                                       # after the scales
        assert op.requant() == 1 and op.info().kernel_name.decode().endswith("fast +bias")
        G.same(G.run(op, case, a_dev, b_dev), R.bmm_reference(case, data, bias, bd), case, "set after the scales")
        set_bias(op, other, od)                                                      # again, another layout, with -inf
        assert op.requant() == 0 and op.info().kernel_name.decode().endswith("exact +bias")
        G.same(G.run(op, case, a_dev, b_dev), R.bmm_reference(case, data, other, od), case, "set again")
        bad = bd["table"].copy()
        bad[0] = np.inf
        room = np.zeros(4096, dtype=np.float32)                                      # (enough floats for any of these layouts)
        for table, periods, strides in ((bad, bias.periods, bd["layout"]), (room, (3, 3), bd["layout"]), (room, (1, 4), bd["layout"]),
                                        (room, (1, 3), (0, 37, 36)), (room, (1, 3), (-1, 37, 37))):
            with pytest.raises(dfa.DfxError, match="dfx error 1"):
                op.set_bias(table, periods=periods, strides=strides)
        G.same(G.run(op, case, a_dev, b_dev), R.bmm_reference(case, data, other, od), case, "after the refusals")
        op.set_scales(data["scales"])                                                # the scales again: still exact
        assert op.requant() == 0
        op.set_bias(None)
        assert op.requant() == 1 and op.info().kernel_name.decode() == B.kernel_name(case, B.MFMA, 1)
        assert op.info().algorithmic_bytes == B.algorithmic_bytes(B.desc_of(case))
        G.same(G.run(op, case, a_dev, b_dev), plain, case, "cleared")
        op.set_bias(None)                                                            # clearing twice is fine
        huge = R.Bias(periods=(1, 1), finite=False, seed=75001)
        hd = bias_of(case, data, huge)
        hd["table"][:] = np.float32(2.0 ** 30 / data["scales"][0])                   # beyond the bound: exact
        set_bias(op, huge, hd)
        assert op.requant() == 0
    finally:
        op.close()
    op = dfa.MatMul(case.batch, case.m, case.n, case.k, a_dtype=B.NP_OF[case.a_dt], dst_dtype=B.NP_OF[case.dst_dt], trans_b=case.trans_b,
                    a_strides=case.strides("a"), b_strides=case.strides("b"), c_strides=case.strides("c"), force_path=B.GENERIC, scales=data["scales"],
                    bias=(bd["values"], bias.periods))                              # the constructor keyword, a dense {p0, p1, n} table
    try:
        G.same(G.run(op, case, a_dev, b_dev), R.bmm_reference(case, data, bias, bd), case, "bias= keyword")
    finally:
        op.close()


def test_a_misaligned_operand_takes_the_generic_kernel_with_the_bias():
    case, bias = R.bmm_layout_cases()[6]                                             # periods (2,3), whole tables
    data = B.generate(case)
    bd = bias_of(case, data, bias)
    op = G.make_op(case, B.MFMA, data["scales"])
    try:
        set_bias(op, bias, bd)
        before = dfa.bmm_launches()
        got = G.run(op, case, G.on_device(data["a"], 4), G.on_device(data["b"]))
        after = dfa.bmm_launches()
        assert [after[p] - before[p] for p in range(2)] == [0, 1]
        G.same(got, R.bmm_reference(case, data, bias, bd), case, "a 4 bytes off")
    finally:
        op.close()
