"""GPU: a Swin stage on the device -- a W-MSA block, an SW-MSA block and patch merging -- bs 2, a 16 x 12 map of C 64, heads 2,
d 32, window 7 (padded to 21 x 14: 6 windows per image, padding on both axes), MLP 256, built from the library's ops with
dfa.WindowOp producing the windows and taking them back:

    LayerNorm -> WindowOp(PARTITION) -> Linear (QKV) -> Attention over batch (bs * nW, heads), Q / K / V head-sliced in place out
    of the one QKV tensor (attention_strides with ld = 3C), relative-position bias (and, shifted, the window mask) ->
    Linear (proj) -> WindowOp(REVERSE) -> ScaledSum (residual) -> LayerNorm -> Linear (fc1 + GELU table) -> Linear (fc2) ->
    ScaledSum (residual)

then WindowOp(PARTITION, 2 x 2, COL_MAJOR, win_ld = C) read as {bs * 8 * 6, 4C} -> LayerNorm(4C) -> Linear(4C -> 2C).
Every intermediate tensor is compared bit for bit with the chained numpy references (lnorm_ref, linear_ref, attn_ref /
attn_bias_ref, wsum_ref, window_ref), on auto, with every WindowOp forced to each kernel and with every Attention forced to
each path.  No tensor leaves the device between the first and the last op."""
import importlib

import numpy as np
import pytest

import attn_bias_ref as AB
import attn_ref as A
import linear_ref as R
import lnorm_ref as L
import window_ref as WR
import wsum_ref as W

pytestmark = pytest.mark.gpu
dfa = importlib.import_module("deep-fusion_amd")
BS, H, WD, HEADS, D, WIN, SHIFT = 2, 16, 12, 2, 32, 7, 3
C, MLP = HEADS * D, 256
HP, WP = 21, 14
NW, T = 6, WIN * WIN
GROWS, WROWS = BS * H * WD, BS * HP * WP
MROWS = BS * (H // 2) * (WD // 2)                      # merged tokens: rows of 4C
EPS = 0.5
GELU_IN, GELU_OUT = 0.05, 0.04
RES = (0.75, 0.625)       # the residual sums' scales
LOGIT_STEP = 0.05         # the s8 logits' quantisation step, for the real-valued relative-position bias
STAGES = ("n1", "w1", "qkv", "ctx", "proj", "rv", "r1", "n2", "h", "fc2", "y")
WIDTH = dict(qkv=3 * C, h=MLP)
WIN_SIDE = ("w1", "qkv", "ctx", "proj")


def _weights(rng, n, k, in_sd, bias=True):
    """random s8 weights, an s32 bias and the scale that gives an output of standard deviation about 40"""
    w = rng.integers(-128, 128, (n, k)).astype(np.int8)
    sd = in_sd * 74.0 * np.sqrt(k)
    bia = np.rint(rng.standard_normal(n) * sd / 4).astype(np.int32) if bias else None
    return dict(w=w, bia=bia, scales=np.array([40.0 / sd], dtype=np.float32), lut=None)


def _norm_params(rng, c=C):
    return (30.0 + 4.0 * rng.standard_normal(c)).astype(np.float32), (3.0 * rng.standard_normal(c)).astype(np.float32)


def _linear_ref(src2d, p, n, lut_in=R.UNDEF):
    rows, k = src2d.shape
    case = R.LinCase("swin", rows, k, n, src_dt=R.S8, dst_dt=R.S8, bia_dt=R.UNDEF if p["bia"] is None else R.S32, src_ld=k, lut_in=lut_in)
    return R.values(case, dict(p, src=np.ascontiguousarray(src2d).reshape(-1)))


def _partition_ref(x2d, window, shift, order):
    x = np.ascontiguousarray(x2d).view(np.uint8).reshape(BS, H, WD, C)
    return WR.partition(x, window, shift, order, 0).view(np.int8)


def _block_reference(rng, x, shift):
    """one block: -> (ref, par, attention case, attention data, bias table, periods)"""
    ref = {"x": x}
    par = dict(ln1=_norm_params(rng), ln2=_norm_params(rng), qkv=_weights(rng, 3 * C, C, 30.0), proj=_weights(rng, C, C, 40.0),
               fc1=_weights(rng, MLP, C, 30.0), fc2=_weights(rng, C, MLP, 25.0, bias=False))
    par["fc1"]["lut"] = dfa.gelu_table(GELU_IN, GELU_OUT, np.int8, np.int8)
    ref["n1"] = L.convert(L.reference_values(x, C, par["ln1"][0], par["ln1"][1], None, EPS, L.LAYER), L.S8)
    ref["w1"] = _partition_ref(ref["n1"], (WIN, WIN), (shift, shift), WR.ROW_MAJOR)
    assert ref["w1"].shape == (WROWS, C)
    ref["qkv"] = _linear_ref(ref["w1"], par["qkv"], 3 * C)
    hs3, hs1 = dfa.attention_strides(BS * NW, HEADS, T, D, 3 * C), dfa.attention_strides(BS * NW, HEADS, T, D, C)
    acase = A.AttnCase("swin", T, T, D, D, q_dt=A.S8, dst_dt=A.S8, batch=(BS * NW, HEADS), q_strides=hs3, k_strides=hs3, v_strides=hs3, o_strides=hs1,
                       logit_scale=40.0 / (40.0 * 40.0 * np.sqrt(D)), out_scale=1.0 / 256.0)
    flat = ref["qkv"].reshape(-1)
    adata = dict(q=flat, k=flat[C:], v=flat[2 * C:], logit_scale=np.array([acase.logit_scale], dtype=np.float32),
                 out_scales=np.array([acase.out_scale], dtype=np.float32), table=A.make_table(acase))
    rel_table = (rng.standard_normal(((2 * WIN - 1) ** 2, HEADS)) * 0.5).astype(np.float32)
    mask = dfa.swin_shift_mask(H, WD, WIN, shift) if shift else None
    table, periods = dfa.attention_bias(rel_bias=dfa.swin_relative_bias(rel_table, WIN), mask=mask, logit_step=LOGIT_STEP,
                                        logit_scale=float(adata["logit_scale"][0]), acc_bound=AB.acc_bound(A.S8, D))
    assert periods == ((NW, HEADS) if shift else (1, HEADS)) and table.shape == periods + (T, T)
    ctx = AB.attn_reference(acase, adata, AB.Bias(periods=periods), dict(values=table))
    assert ctx.size == WROWS * C
    ref["ctx"] = ctx.view(np.int8).reshape(WROWS, C)
    ref["proj"] = _linear_ref(ref["ctx"], par["proj"], C)
    rv = WR.reverse(ref["proj"].view(np.uint8), BS, H, WD, (WIN, WIN), (shift, shift), WR.ROW_MAJOR)
    ref["rv"] = rv.view(np.int8).reshape(GROWS, C)
    wcase = W.WsumCase("res", (BS, H * WD, 1, C), (W.S8, W.S8), W.S8, (False, False))
    scales = [np.array([s], dtype=np.float32) for s in RES]
    shape = (BS, H * WD, 1, C)
    ref["r1"] = W.reference(wcase, [x.reshape(shape), ref["rv"].reshape(shape)], scales, None, None).reshape(GROWS, C)
    ref["n2"] = L.convert(L.reference_values(ref["r1"], C, par["ln2"][0], par["ln2"][1], None, EPS, L.LAYER), L.S8)
    ref["h"] = _linear_ref(ref["n2"], par["fc1"], MLP, lut_in=R.S8)
    ref["fc2"] = _linear_ref(ref["h"], par["fc2"], C)
    ref["y"] = W.reference(wcase, [ref["r1"].reshape(shape), ref["fc2"].reshape(shape)], scales, None, None).reshape(GROWS, C)
    return dict(ref=ref, par=par, adata=adata, table=table, periods=periods, mask=mask)


def _build_reference():
    rng = np.random.default_rng(7070)
    x = rng.integers(-128, 128, (GROWS, C)).astype(np.int8)
    b0 = _block_reference(rng, x, 0)
    b1 = _block_reference(rng, b0["ref"]["y"], SHIFT)
    mref = {}
    mpar = dict(ln=_norm_params(rng, 4 * C), red=_weights(rng, 2 * C, 4 * C, 30.0, bias=False))
    mref["m"] = _partition_ref(b1["ref"]["y"], (2, 2), (0, 0), WR.COL_MAJOR).reshape(MROWS, 4 * C)
    mref["n3"] = L.convert(L.reference_values(mref["m"], 4 * C, mpar["ln"][0], mpar["ln"][1], None, EPS, L.LAYER), L.S8)
    mref["red"] = _linear_ref(mref["n3"], mpar["red"], 2 * C)
    return b0, b1, dict(ref=mref, par=mpar)


_BUILT = []


def built():
    """the chained reference, computed once and shared by all runs; left unchanged"""
    if not _BUILT:
        _BUILT.append(_build_reference())
        b0, b1, mg = _BUILT[0]
        for blk, names in ((b0, STAGES), (b1, STAGES), (mg, ("m", "n3", "red"))):          # no stage is degenerate
            for name in names:
                v = blk["ref"][name].astype(np.int64)
                assert v.std() > 4 and len(np.unique(v)) > 20, (name, v.std())
                assert ((v == -128) | (v == 127)).mean() < 0.1, name
        for blk in (b0, b1):
            assert (blk["ref"]["h"] < 0).any() and blk["ref"]["h"].min() >= -5               # GELU's dip, and nothing below it
        # the shifted block's mask: some logit row is partly masked, none is fully masked (a property of the mask)
        mask = b1["mask"]
        assert b0["mask"] is None and mask.shape == (NW, T, T) and mask.any(axis=2).any() and not mask.all(axis=2).any()
        masked_value = b1["table"].min()
        assert ((b1["table"] == masked_value).any(axis=3) & ~(b1["table"] == masked_value).all(axis=3)).any()
        assert np.array_equal(b1["table"] == masked_value, np.broadcast_to(mask[:, None], b1["table"].shape))
    return _BUILT[0]


RUNS = [("auto", dfa.WINDOW_AUTO, dfa.ATTN_AUTO), ("window-row", dfa.WINDOW_ROW, dfa.ATTN_AUTO), ("window-generic", dfa.WINDOW_GENERIC, dfa.ATTN_AUTO),
        ("attn-fused", dfa.WINDOW_AUTO, dfa.ATTN_FUSED), ("attn-chain", dfa.WINDOW_AUTO, dfa.ATTN_CHAIN)]


@pytest.mark.parametrize("name,wpath,apath", RUNS, ids=[r[0] for r in RUNS])
def test_swin_stage_on_the_device(name, wpath, apath):
    import torch
    b0, b1, mg = built()

    def fresh(rows, width):
        return torch.full((rows * width,), -51, dtype=torch.int8, device="cuda")

    def lin(rows, k, n, p, table=None):
        op = dfa.Linear(rows, k, n, np.int8, np.int8, bia_dt=dfa.DFX_UNDEF if p["bia"] is None else dfa.DFX_S32, table=table)
        op.set_weights(p["w"], p["scales"], p["bia"])
        if table is not None:
            op.set_table(p["lut"])
        return op

    def norm(rows, c, p):
        op = dfa.LayerNorm(rows, c, np.int8, np.int8, EPS)
        op.set_params(p[0], p[1])
        return op

    def resid():
        op = dfa.ScaledSum((BS, H * WD, 1, C), [np.int8, np.int8], np.int8, [1, 1])
        op.set_params([np.array([s], dtype=np.float32) for s in RES])
        return op

    def window(direction, win, shift=0, order=dfa.WINDOW_ROW_MAJOR):
        return dfa.WindowOp(direction, BS, H, WD, C, win, shift=shift, order=order, dtype=np.int8, pad_value=0, force_path=wpath)

    hs3, hs1 = dfa.attention_strides(BS * NW, HEADS, T, D, 3 * C), dfa.attention_strides(BS * NW, HEADS, T, D, C)
    ops, devs = [], []
    try:
        def block_ops(blk, shift):
            par, adata = blk["par"], blk["adata"]
            o = dict(ln1=norm(GROWS, C, par["ln1"]), part=window(dfa.WINDOW_PARTITION, WIN, shift), qkv=lin(WROWS, C, 3 * C, par["qkv"]),
                     attn=dfa.Attention((BS * NW, HEADS), T, T, D, D, q_strides=hs3, k_strides=hs3, v_strides=hs3, o_strides=hs1, table=adata["table"],
                                        logit_scale=adata["logit_scale"][0], out_scales=adata["out_scales"], bias=(blk["table"], blk["periods"]),
                                        force_path=apath),
                     proj=lin(WROWS, C, C, par["proj"]), rev=window(dfa.WINDOW_REVERSE, WIN, shift), r1=resid(), ln2=norm(GROWS, C, par["ln2"]),
                     fc1=lin(GROWS, C, MLP, par["fc1"], table=np.int8), fc2=lin(GROWS, MLP, C, par["fc2"]), r2=resid())
            ops.extend(o.values())
            return o

        o0, o1 = block_ops(b0, 0), block_ops(b1, SHIFT)
        om = dict(part=window(dfa.WINDOW_PARTITION, 2, 0, dfa.WINDOW_COL_MAJOR), ln=norm(MROWS, 4 * C, mg["par"]["ln"]),
                  red=lin(MROWS, 4 * C, 2 * C, mg["par"]["red"]))
        ops.extend(om.values())
        want_w = dfa.WINDOW_GENERIC if wpath == dfa.WINDOW_AUTO else wpath
        for op in (o0["part"], o0["rev"], o1["part"], o1["rev"], om["part"]):
            assert op.info().path == want_w
        assert o1["part"].n_windows == NW and o1["part"].win_rows == WROWS and om["part"].win_rows == 4 * MROWS
        if apath != dfa.ATTN_AUTO:
            assert o0["attn"].info().path == apath and o1["attn"].info().path == apath

        def run_block(o, x_dev):
            d = {k: fresh(WROWS if k in WIN_SIDE else GROWS, WIDTH.get(k, C)) for k in STAGES}
            o["ln1"].submit(x_dev, d["n1"])
            o["part"].submit(d["n1"], d["w1"])
            o["qkv"].submit(d["w1"], d["qkv"])
            o["attn"].submit(d["qkv"], d["qkv"][C:], d["qkv"][2 * C:], d["ctx"])
            o["proj"].submit(d["ctx"], d["proj"])
            o["rev"].submit(d["proj"], d["rv"])
            o["r1"].submit([x_dev, d["rv"]], d["r1"])
            o["ln2"].submit(d["r1"], d["n2"])
            o["fc1"].submit(d["n2"], d["h"])
            o["fc2"].submit(d["h"], d["fc2"])
            o["r2"].submit([d["r1"], d["fc2"]], d["y"])
            return d

        x_dev = torch.from_numpy(b0["ref"]["x"].reshape(-1).copy()).cuda()
        before = dfa.window_launches()
        d0 = run_block(o0, x_dev)
        d1 = run_block(o1, d0["y"])
        dm = dict(m=fresh(MROWS, 4 * C), n3=fresh(MROWS, 4 * C), red=fresh(MROWS, 2 * C))
        om["part"].submit(d1["y"], dm["m"])
        om["ln"].submit(dm["m"], dm["n3"])
        om["red"].submit(dm["n3"], dm["red"])
        torch.cuda.synchronize()
        devs.extend([d0, d1, dm])
        after = dfa.window_launches()
        assert [after[p] - before[p] for p in range(2)] == [5 * int(p == want_w) for p in range(2)]
        for what, blk, d in (("W-MSA", b0, d0), ("SW-MSA", b1, d1), ("merging", mg, dm)):
            for k in d:
                ref = blk["ref"][k]
                got = d[k].cpu().numpy().reshape(ref.shape)
                assert np.array_equal(got, ref), "%s %s differs in %d of %d elements" % (what, k, int((got != ref).sum()), got.size)
    finally:
        for op in ops:
            op.close()
