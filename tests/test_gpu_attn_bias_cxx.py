"""GPU: the logit_bias overloads of deepfusion::attention and deepfusion::matmul of the drop-in C++ layer, driven by
tools/attn_bias_check on files this test writes from tests/attn_bias_ref.py: an attention with per-(window, head) tables and a
random mask, and a matrix product with one bias row per head, each submitted synchronously and asynchronously.
attn_bias_check compares every valid element with the expected storage and runs the same case without the bias, which must
then differ."""
import os
import subprocess

import numpy as np
import pytest

import attn_bias_ref as R
import attn_ref as A
import bmm_ref as B

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "deep-fusion_amd", "tools", "attn_bias_check")


def _bias_words(d, name, bias, bd):
    bd["table"].astype(np.float32).tofile(os.path.join(d, name + ".bias"))
    return "%d %d %d %d %d" % (bias.periods + tuple(bd["layout"]))


def _write_attn(d, name, case, bias, use_async):
    data = A.generate(case)
    bd = R.attn_bias_data(case, data, bias)
    desc = A.desc_of(case)
    for ext in "qkv":
        data[ext].tofile(os.path.join(d, "%s.%s" % (name, ext)))
    data["table"].astype(np.uint32).tofile(os.path.join(d, name + ".table"))
    data["out_scales"].astype(np.float32).tofile(os.path.join(d, name + ".scales"))
    R.attn_reference(case, data, bias, bd).tofile(os.path.join(d, name + ".o"))
    head = ("batch0", "batch1", "tq", "tk", "d", "dv", "q_dt", "dst_dt", "relu", "round_mode", "nscales")
    tail = ("q_s0", "q_s1", "ldq", "k_s0", "k_s1", "ldk", "v_s0", "v_s1", "ldv", "o_s0", "o_s1", "ldo")
    return "attn %s %s %d %r %r %s %s %s\n" % (name, " ".join(str(int(desc[k])) for k in head), int(use_async), float(case.prob_scale),
                                               float(data["logit_scale"][0]), " ".join(str(int(desc[k])) for k in tail),
                                               " ".join(str(A.storage_elems(case, w)) for w in "qkvo"), _bias_words(d, name, bias, bd))


def _write_bmm(d, name, case, bias, use_async):
    data = B.generate(case)
    bd = R.make_bias(bias, case.m, case.n, data["scales"][0], R.acc_bound(case.a_dt, case.k))
    desc = B.desc_of(case)
    for ext in "ab":
        data[ext].tofile(os.path.join(d, "%s.%s" % (name, ext)))
    data["scales"].astype(np.float32).tofile(os.path.join(d, name + ".scales"))
    R.bmm_reference(case, data, bias, bd).tofile(os.path.join(d, name + ".c"))
    head = ("batch0", "batch1", "m", "n", "k", "trans_b", "a_dt", "dst_dt", "relu", "round_mode", "nscales")
    tail = ("a_s0", "a_s1", "lda", "b_s0", "b_s1", "ldb", "c_s0", "c_s1", "ldc")
    return "bmm %s %s %d %s %s %s\n" % (name, " ".join(str(int(desc[k])) for k in head), int(use_async), " ".join(str(int(desc[k])) for k in tail),
                                        " ".join(str(B.storage_elems(case, w)) for w in "abc"), _bias_words(d, name, bias, bd))


def test_attn_bias_check_on_both_overloads_sync_and_async(tmp_path):
    assert os.path.exists(TOOL), "run __graft_entry__.build() first"
    d = str(tmp_path)
    attn, bmm = R.cxx_cases()
    lines = []
    for use_async in (0, 1):
        for case, bias in attn:
            lines.append(_write_attn(d, "attn-%s%d" % (case.name, use_async), case, bias, use_async))
        for case, bias in bmm:
            lines.append(_write_bmm(d, "bmm-%s%d" % (case.name, use_async), case, bias, use_async))
    with open(os.path.join(d, "cases.txt"), "w") as f:
        f.writelines(lines)
    p = subprocess.run([TOOL, d], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    assert "attn_bias_check: 4 entries, all ok" in out and "DIFFERENT" not in out, out
    assert out.count(" sync ") == 2 and out.count(" async ") == 2, out
