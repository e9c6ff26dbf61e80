"""GPU: one ViT-style encoder block on the device, bs 2, T 50, heads 2, d 32 (C 64, MLP 256), built from the library's ops with
dfa.Linear as its four weight multiplies:

    LayerNorm -> Linear (QKV, s8, bias) -> Attention reading Q / K / V head-sliced in place out of the one QKV tensor
    (attention_strides with ld = 3C) -> Linear (proj, reading the head-interleaved context) -> ScaledSum (residual) ->
    LayerNorm -> Linear (fc1 + GELU table) -> Linear (fc2) -> ScaledSum (residual)

Every intermediate tensor is compared bit for bit with the chained numpy references (lnorm_ref, linear_ref, attn_ref,
wsum_ref), on auto and with every Linear forced to each path.  No tensor leaves the device between the first and the last op."""
import importlib

import numpy as np
import pytest

import attn_ref as A
import linear_ref as R
import lnorm_ref as L
import wsum_ref as W

pytestmark = pytest.mark.gpu
dfa = importlib.import_module("deep-fusion_amd")
BS, T, HEADS, D = 2, 50, 2, 32
C, MLP, ROWS = HEADS * D, 256, BS * T
EPS = 0.5
GELU_IN, GELU_OUT = 0.05, 0.04
RES = (0.75, 0.625)       # the residual sums' scales


def _weights(rng, n, k, in_sd, bias=True):
    """random s8 weights, an s32 bias and the scale that gives an output of standard deviation about 40"""
    w = rng.integers(-128, 128, (n, k)).astype(np.int8)
    sd = in_sd * 74.0 * np.sqrt(k)
    bia = np.rint(rng.standard_normal(n) * sd / 4).astype(np.int32) if bias else None
    return dict(w=w, bia=bia, scales=np.array([40.0 / sd], dtype=np.float32), lut=None)


def _norm_params(rng):
    return (30.0 + 4.0 * rng.standard_normal(C)).astype(np.float32), (3.0 * rng.standard_normal(C)).astype(np.float32)


def _linear_ref(src2d, p, n, dst_dt=R.S8, lut_in=R.UNDEF):
    rows, k = src2d.shape
    case = R.LinCase("block", rows, k, n, src_dt=R.S8, dst_dt=dst_dt, bia_dt=R.UNDEF if p["bia"] is None else R.S32, src_ld=k, lut_in=lut_in)
    return case, R.values(case, dict(p, src=np.ascontiguousarray(src2d).reshape(-1)))


def _build_reference():
    rng = np.random.default_rng(4242)
    ref = {}
    ref["x"] = rng.integers(-128, 128, (ROWS, C)).astype(np.int8)
    par = dict(ln1=_norm_params(rng), ln2=_norm_params(rng), qkv=_weights(rng, 3 * C, C, 30.0), proj=_weights(rng, C, C, 40.0),
               fc1=_weights(rng, MLP, C, 30.0), fc2=_weights(rng, C, MLP, 25.0, bias=False))
    par["fc1"]["lut"] = dfa.gelu_table(GELU_IN, GELU_OUT, np.int8, np.int8)
    ref["n1"] = L.convert(L.reference_values(ref["x"], C, par["ln1"][0], par["ln1"][1], None, EPS, L.LAYER), L.S8)
    _, ref["qkv"] = _linear_ref(ref["n1"], par["qkv"], 3 * C)
    hs3, hs1 = dfa.attention_strides(BS, HEADS, T, D, 3 * C), dfa.attention_strides(BS, HEADS, T, D, C)
    acase = A.AttnCase("block", T, T, D, D, q_dt=A.S8, dst_dt=A.S8, batch=(BS, HEADS), q_strides=hs3, k_strides=hs3, v_strides=hs3, o_strides=hs1,
                       logit_scale=40.0 / (40.0 * 40.0 * np.sqrt(D)), out_scale=1.0 / 256.0)
    flat = ref["qkv"].reshape(-1)
    adata = dict(q=flat, k=flat[C:], v=flat[2 * C:], logit_scale=np.array([acase.logit_scale], dtype=np.float32),
                 out_scales=np.array([acase.out_scale], dtype=np.float32), table=A.make_table(acase))
    ctx = A.reference(acase, adata)
    assert ctx.size == ROWS * C
    ref["ctx"] = ctx.view(np.int8).reshape(ROWS, C)
    _, ref["proj"] = _linear_ref(ref["ctx"], par["proj"], C)
    wcase = W.WsumCase("res", (BS, T, 1, C), (W.S8, W.S8), W.S8, (False, False))
    scales = [np.array([s], dtype=np.float32) for s in RES]
    ref["r1"] = W.reference(wcase, [ref["x"].reshape(BS, T, 1, C), ref["proj"].reshape(BS, T, 1, C)], scales, None, None).reshape(ROWS, C)
    ref["n2"] = L.convert(L.reference_values(ref["r1"], C, par["ln2"][0], par["ln2"][1], None, EPS, L.LAYER), L.S8)
    _, ref["h"] = _linear_ref(ref["n2"], par["fc1"], MLP, lut_in=R.S8)
    _, ref["fc2"] = _linear_ref(ref["h"], par["fc2"], C)
    ref["y"] = W.reference(wcase, [ref["r1"].reshape(BS, T, 1, C), ref["fc2"].reshape(BS, T, 1, C)], scales, None, None).reshape(ROWS, C)
    return ref, par, acase, adata


_BUILT = []


def built():
    """the chained reference, computed once and shared by the three runs; left unchanged"""
    if not _BUILT:
        _BUILT.append(_build_reference())
        ref = _BUILT[0][0]
        for name in ("n1", "qkv", "ctx", "proj", "r1", "n2", "h", "fc2", "y"):          # no stage of the block is degenerate
            v = ref[name].astype(np.int64)
            assert v.std() > 4 and len(np.unique(v)) > 20, (name, v.std())
            assert ((v == -128) | (v == 127)).mean() < 0.1, name
        assert (ref["h"] < 0).any() and ref["h"].min() >= -5                            # GELU's dip, and nothing below it
    return _BUILT[0]


@pytest.mark.parametrize("path", [dfa.LINEAR_AUTO, dfa.LINEAR_TILE, dfa.LINEAR_GENERIC], ids=["auto", "tile", "generic"])
def test_encoder_block_on_the_device(path):
    import torch
    ref, par, acase, adata = built()
    dev = {k: torch.full((ROWS * (3 * C if k == "qkv" else MLP if k == "h" else C),), -51, dtype=torch.int8, device="cuda")
           for k in ("n1", "qkv", "ctx", "proj", "r1", "n2", "h", "fc2", "y")}
    dev["x"] = torch.from_numpy(ref["x"].reshape(-1).copy()).cuda()

    def lin(k, n, p, table=None):
        op = dfa.Linear(ROWS, k, n, np.int8, np.int8, bia_dt=dfa.DFX_UNDEF if p["bia"] is None else dfa.DFX_S32, table=table, force_path=path)
        op.set_weights(p["w"], p["scales"], p["bia"])
        if table is not None:
            op.set_table(p["lut"])
        return op

    def norm(p):
        op = dfa.LayerNorm(ROWS, C, np.int8, np.int8, EPS)
        op.set_params(p[0], p[1])
        return op

    def resid():
        op = dfa.ScaledSum((BS, T, 1, C), [np.int8, np.int8], np.int8, [1, 1])
        op.set_params([np.array([s], dtype=np.float32) for s in RES])
        return op

    hs3, hs1 = dfa.attention_strides(BS, HEADS, T, D, 3 * C), dfa.attention_strides(BS, HEADS, T, D, C)
    ops = dict(ln1=norm(par["ln1"]), qkv=lin(C, 3 * C, par["qkv"]),
               attn=dfa.Attention((BS, HEADS), T, T, D, D, q_strides=hs3, k_strides=hs3, v_strides=hs3, o_strides=hs1, table=adata["table"],
                                  logit_scale=adata["logit_scale"][0], out_scales=adata["out_scales"]),
               proj=lin(C, C, par["proj"]), r1=resid(), ln2=norm(par["ln2"]), fc1=lin(C, MLP, par["fc1"], table=np.int8), fc2=lin(MLP, C, par["fc2"]),
               r2=resid())
    try:
        want_path = dfa.LINEAR_GENERIC if path == dfa.LINEAR_AUTO else path
        for k in ("qkv", "proj", "fc1", "fc2"):
            assert ops[k].info().path == want_path, k
        before = dfa.linear_launches()
        ops["ln1"].submit(dev["x"], dev["n1"])
        ops["qkv"].submit(dev["n1"], dev["qkv"])
        ops["attn"].submit(dev["qkv"], dev["qkv"][C:], dev["qkv"][2 * C:], dev["ctx"])
        ops["proj"].submit(dev["ctx"], dev["proj"])
        ops["r1"].submit([dev["x"], dev["proj"]], dev["r1"])
        ops["ln2"].submit(dev["r1"], dev["n2"])
        ops["fc1"].submit(dev["n2"], dev["h"])
        ops["fc2"].submit(dev["h"], dev["fc2"])
        ops["r2"].submit([dev["r1"], dev["fc2"]], dev["y"])
        torch.cuda.synchronize()
        after = dfa.linear_launches()
        assert [after[p] - before[p] for p in range(2)] == [4 * int(p == want_path) for p in range(2)]
        for k in ("n1", "qkv", "ctx", "proj", "r1", "n2", "h", "fc2", "y"):
            got = dev[k].cpu().numpy().reshape(ref[k].shape)
            assert np.array_equal(got, ref[k]), "%s differs in %d of %d elements" % (k, int((got != ref[k]).sum()), got.size)
    finally:
        for op in ops.values():
            op.close()
