"""GPU: deepfusion::attention of the drop-in C++ layer, driven by tools/attn_check on files this test writes from
tests/attn_ref.py: the head-sliced block (bs 2, heads 2, T 37, d 32, context interleaved back) and a ragged dense shape with a
u8 Q, per-channel out scales and an s32 O, each submitted synchronously and asynchronously.  attn_check compares every valid
element with the expected storage and with its own scalar restatement of the chain."""
import os
import subprocess

import numpy as np
import pytest

import attn_ref as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "deep-fusion_amd", "tools", "attn_check")


def _write_case(d, name, case, data, use_async):
    desc = A.desc_of(case)
    for ext in "qkv":
        data[ext].tofile(os.path.join(d, "%s.%s" % (name, ext)))
    data["table"].astype(np.uint32).tofile(os.path.join(d, name + ".table"))
    data["out_scales"].astype(np.float32).tofile(os.path.join(d, name + ".scales"))
    A.reference(case, data).tofile(os.path.join(d, name + ".o"))
    head = ("batch0", "batch1", "tq", "tk", "d", "dv", "q_dt", "dst_dt", "relu", "round_mode", "nscales")
    tail = ("q_s0", "q_s1", "ldq", "k_s0", "k_s1", "ldk", "v_s0", "v_s1", "ldv", "o_s0", "o_s1", "ldo")
    return "case %s %s %d %r %r %s\n" % (name, " ".join(str(int(desc[k])) for k in head), int(use_async), float(case.prob_scale),
                                         float(data["logit_scale"][0]), " ".join(str(int(desc[k])) for k in tail))


def test_attn_check_on_two_shapes_sync_and_async(tmp_path):
    assert os.path.exists(TOOL), "run __graft_entry__.build() first"
    d = str(tmp_path)
    cases = A.cxx_cases()
    assert [c.name for c in cases] == ["heads", "ragged"]
    lines = []
    for case in cases:
        data = A.generate(case)
        for use_async in (0, 1):
            lines.append(_write_case(d, "%s%d" % (case.name, use_async), case, data, use_async))
    with open(os.path.join(d, "cases.txt"), "w") as f:
        f.writelines(lines)
    p = subprocess.run([TOOL, d], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    assert "attn_check: 4 entries, all ok" in out and "DIFFERENT" not in out, out
    assert out.count(" sync ") == 2 and out.count(" async ") == 2, out
