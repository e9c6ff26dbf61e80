"""GPU: deepfusion::linear of the drop-in C++ layer, driven by tools/linear_check: its own cases against the scalar reference
inside the tool (QKV with bias, a k_valid slice, fc1 with a table, u8 src, odd sizes, a padded f32 dst, 1 x 1 x 1, and a
layer_norm -> linear -> linear chain on the device, asynchronous), then the cases this test writes from tests/linear_ref.py --
two points of the grid of tails and the fc1 + table case, each submitted synchronously and asynchronously -- which the tool
compares with the expected storage from numpy AND with its scalar reference."""
import os
import subprocess

import numpy as np
import pytest

import linear_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "deep-fusion_amd", "tools", "linear_check")


def _write_case(d, name, case, bs, h, w, use_async):
    assert bs * h * w == case.rows
    data = R.generate(case)
    full = np.full((case.rows, case.dld * R.SIZE_OF[case.dst_dt]), 0xCD, dtype=np.uint8).view(R.NP_OF[case.dst_dt]).reshape(case.rows, case.dld).copy()
    full[:, :case.n] = R.values(case, data)
    data["src"].view(np.uint8).tofile(os.path.join(d, name + ".src"))
    data["w"].tofile(os.path.join(d, name + ".wei"))
    data["scales"].tofile(os.path.join(d, name + ".scales"))
    full.tofile(os.path.join(d, name + ".dst"))
    if data["bia"] is not None:
        data["bia"].tofile(os.path.join(d, name + ".bia"))
    if data["lut"] is not None:
        data["lut"].tofile(os.path.join(d, name + ".lut"))
    return "case %s %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n" % (
        name, bs, case.sld, h, w, case.k, case.n, case.dld, case.src_dt, case.dst_dt, case.bia_dt, int(case.relu), case.rm, case.nscales, case.lut_in,
        int(use_async))


def test_linear_check_own_cases_and_three_written_shapes_sync_and_async(tmp_path):
    assert os.path.exists(TOOL), "run __graft_entry__.build() first"
    d = str(tmp_path)
    grid = R.shape_grid(64, R.U8)
    # (a pairwise cover holds every pair of tails: rows BM + 1 with n = BN + 1 at BM 64, rows 2 BM + 2 with k = 200 at BM 128)
    tails = [c for c in grid if (c.rows, c.n) == (65, 129)][:1] + [c for c in R.shape_grid(128, R.S8) if (c.rows, c.k) == (258, 200)][:1]
    assert len(tails) == 2, [c.ident() for c in tails]
    fc1 = R.CXX_FC1_CASE
    lines = []
    for use_async in (0, 1):
        lines.append(_write_case(d, "tail-a%d" % use_async, tails[0], 5, 13, 1, use_async))
        lines.append(_write_case(d, "tail-b%d" % use_async, tails[1], 2, 43, 3, use_async))
        lines.append(_write_case(d, "fc1-lut%d" % use_async, fc1, 2, 50, 1, use_async))
    with open(os.path.join(d, "cases.txt"), "w") as f:
        f.writelines(lines)
    p = subprocess.run([TOOL, d], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    assert "linear_check: 6 entries from" in out and "DIFFERENT" not in out, out
    assert "linear_check: every case identical to the reference (15 cases)" in out, out
    assert out.count(" sync") >= 3 and out.count(" async") >= 3 and out.count("+table") >= 3, out
