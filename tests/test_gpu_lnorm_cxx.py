"""GPU: deepfusion::layer_norm of the drop-in C++ layer, driven by tools/lnorm_check: its own cases against the scalar
reference inside the tool (shapes of Swin / ViT, c_valid below C, odd leading dimensions, one channel, c = 16384, a
layer_norm -> inner_product chain on the device, two norms in flight), then the cases this test writes from
tests/lnorm_ref.py -- a ViT-like block with shifts and a ragged shape with c_valid < C, an f32 dst and no beta, each
submitted synchronously and asynchronously -- which the tool compares with the expected storage from numpy AND with its
scalar reference."""
import os
import subprocess

import numpy as np
import pytest

import lnorm_ref as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "deep-fusion_amd", "tools", "lnorm_check")


def _write_case(d, name, case, bs, h, w, with_beta, use_async):
    assert bs * h * w == case.rows
    src = L.make_src(case)
    gamma, beta, shift = L.make_params(case)
    if not with_beta:
        beta = None
    want = L.reference(case, src, (gamma, beta, shift))
    full = np.full((case.rows, case.dst_ld * L.SIZE_OF[case.dst_dt]), 0xCD, dtype=np.uint8).view(L.NP_OF[case.dst_dt]).reshape(case.rows, case.dst_ld).copy()
    full[:, :case.c] = want
    src.tofile(os.path.join(d, name + ".src"))
    gamma.tofile(os.path.join(d, name + ".gamma"))
    full.tofile(os.path.join(d, name + ".dst"))
    if beta is not None:
        beta.tofile(os.path.join(d, name + ".beta"))
    if shift is not None:
        shift.tofile(os.path.join(d, name + ".shift"))
    eps_bits = int(np.array([case.eps], dtype=np.float32).view(np.uint32)[0])
    return "case %s %d %d %d %d %d %d %d %d %d %d %d %d %x\n" % (name, bs, case.src_ld, h, w, case.c, case.dst_ld, case.src_dt, case.dst_dt, case.mode,
                                                                 int(beta is not None), int(shift is not None), int(use_async), eps_bits)


def test_lnorm_check_own_cases_and_two_written_shapes_sync_and_async(tmp_path):
    assert os.path.exists(TOOL), "run __graft_entry__.build() first"
    d = str(tmp_path)
    vit = L.LnCase("vit", 2 * 197, 768, L.S8, L.S8, shift=True, eps=1e-5 / 0.04 ** 2)
    ragged = L.LnCase("ragged", 3 * 5 * 7, 100, L.U8, L.F32, mode=L.RMS, src_ld=112, dst_ld=101, eps=0.5)
    lines = []
    for use_async in (0, 1):
        lines.append(_write_case(d, "vit%d" % use_async, vit, 2, 197, 1, True, use_async))
        lines.append(_write_case(d, "ragged%d" % use_async, ragged, 3, 5, 7, False, use_async))
    with open(os.path.join(d, "cases.txt"), "w") as f:
        f.writelines(lines)
    p = subprocess.run([TOOL, d], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    assert "lnorm_check: 4 entries from" in out and "DIFFERENT" not in out, out
    assert "lnorm_check: every case identical to the reference (14 cases)" in out, out
    assert out.count(" sync") >= 2 and out.count(" async") >= 2, out
