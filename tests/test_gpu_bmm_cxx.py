"""GPU: deepfusion::matmul of the drop-in C++ layer, driven by tools/bmm_check on files this test writes from tests/bmm_ref.py:
the int8 attention chain (matmul -> softmax -> matmul, asynchronous, no host step in between) of tests/test_gpu_bmm.py and two
points of the shape grid.  bmm_check compares every valid element with the expected storage and with its own scalar
restatement."""
import os
import subprocess

import numpy as np
import pytest

import bmm_ref as R
import head_ref as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "deep-fusion_amd", "tools", "bmm_check")


def _write_case(d, name, case, data):
    desc = R.desc_of(case)
    # the tool's tensors end where bmm_ref's storage does: the last row's valid columns rounded up to 16
    data["a"].tofile(os.path.join(d, name + ".a"))
    data["b"].tofile(os.path.join(d, name + ".b"))
    data["scales"].astype(np.float32).tofile(os.path.join(d, name + ".scales"))
    R.reference(case, data).tofile(os.path.join(d, name + ".c"))
    keys = ("batch0", "batch1", "m", "n", "k", "trans_b", "a_dt", "dst_dt", "relu", "round_mode", "nscales", "a_s0", "a_s1", "lda", "b_s0", "b_s1",
            "ldb", "c_s0", "c_s1", "ldc")
    return "case %s %s\n" % (name, " ".join(str(int(desc[k])) for k in keys))


def test_bmm_check_on_the_chain_and_two_grid_points(tmp_path):
    assert os.path.exists(TOOL), "run __graft_entry__.build() first"
    d = str(tmp_path)
    lines = []
    grid = R.shape_grid()
    picks = [c for c in grid if (c.m, c.n, c.k) == (65, 130, 200) and c.trans_b and c.a_dt == R.U8][:1] + \
            [c for c in grid if (c.m, c.n, c.k) == (33, 31, 17) and not c.trans_b and c.a_dt == R.S8][:1]
    assert len(picks) == 2
    for i, case in enumerate(picks):
        lines.append(_write_case(d, "grid%d" % i, case, R.generate(case)))
    # the chain of tests/test_gpu_bmm.py::test_attention_chain in the tool's layout: logit rows up16(t) apart
    bs, heads, t, dd, ld = 2, 2, 37, 32, 48
    hs = R.attention_strides(bs, heads, t, dd)
    ls = (heads * t * ld, t * ld, ld)
    qk = R.BmmCase("chain-qk", t, t, dd, trans_b=True, a_dt=R.S8, dst_dt=R.S8, batch=(bs, heads), a_strides=hs, b_strides=hs, c_strides=ls, seed=39000)
    pv = R.BmmCase("chain-pv", t, dd, t, trans_b=False, a_dt=R.U8, dst_dt=R.S8, batch=(bs, heads), a_strides=ls, b_strides=hs, c_strides=hs,
                   scale=1.0 / 256.0, seed=39001)
    qdata = R.generate(qk)
    v = R.generate(pv)["b"]
    rows = bs * heads * t
    table = H.softmax_table(0.0625, t)
    logits = np.full(rows * ld, R.POISON, dtype=np.uint8)
    ref = R.reference(qk, qdata)
    logits[:ref.size] = ref
    probs = np.full((rows, ld), R.POISON, dtype=np.uint8)
    probs[:, :t] = H.reference_softmax(logits.view(np.int8).reshape(rows, ld), t, table, H.U8, 255.0)
    pdata = dict(a=probs.reshape(-1), b=v, scales=R.make_scales(pv))
    context = R.reference(pv, pdata)
    n_tensor = bs * t * heads * dd
    for ext, arr in (("q", qdata["a"]), ("k", qdata["b"]), ("v", v)):
        assert arr.size == n_tensor
        arr.tofile(os.path.join(d, "chain." + ext))
    table.astype(np.uint32).tofile(os.path.join(d, "chain.table"))
    logits.tofile(os.path.join(d, "chain.logits"))
    probs.tofile(os.path.join(d, "chain.probs"))
    assert context.size == n_tensor
    context.tofile(os.path.join(d, "chain.context"))
    lines.append("chain chain %d %d %d %d %r %r\n" % (bs, heads, t, dd, float(qdata["scales"][0]), float(pdata["scales"][0])))
    with open(os.path.join(d, "cases.txt"), "w") as f:
        f.writelines(lines)
    p = subprocess.run([TOOL, d], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    assert "bmm_check: 3 entries, all ok" in out and "DIFFERENT" not in out, out
    assert out.count(" ok") >= 5, out
