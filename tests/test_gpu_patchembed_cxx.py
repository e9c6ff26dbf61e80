"""GPU: deepfusion::patch_embed of the drop-in C++ layer, driven by tools/patchembed_check: its own cases against the scalar
restatement inside the tool (a ViT /16 stem with class token and position table, a Swin 4 x 4 stem, an s8 2 x 2 downsample, two
prefix rows with slack, a /14 stem outside the tile class, a padded f32 dst, 1 x 1 x 1, and a patch_embed -> layer_norm -> linear
chain on the device, asynchronous), then the cases this test writes from tests/patchembed_ref.py -- two points of the pairwise
cover and the class-token case, each submitted synchronously and asynchronously -- which the tool compares with the expected
storage from numpy AND with its scalar restatement.  Once on one device and once as two batch shards of the same device."""
import os
import subprocess

import numpy as np
import pytest

import patchembed_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "deep-fusion_amd", "tools", "patchembed_check")


def _write_case(d, name, case, use_async):
    assert not case.extra_h and not case.extra_w                     # (the C++ layer takes th, tw from the image's size)
    data = R.generate(case)
    data["src"].view(np.uint8).tofile(os.path.join(d, name + ".src"))
    data["w"].tofile(os.path.join(d, name + ".wei"))
    data["scales"].tofile(os.path.join(d, name + ".scales"))
    R.reference(case, data).tofile(os.path.join(d, name + ".dst"))
    if data["bia"] is not None:
        data["bia"].tofile(os.path.join(d, name + ".bia"))
    if data["table"] is not None:
        data["table"].tofile(os.path.join(d, name + ".table"))
    if data["prefix"] is not None:
        data["prefix"].tofile(os.path.join(d, name + ".prefix"))
    return "case %s %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n" % (
        name, case.bs, case.ic, case.ih, case.iw, case.ph, case.pw, case.oc, case.dld, case.img_rows, 1, case.t0, case.src_dt, case.dst_dt, case.bia_dt,
        int(case.relu), case.rm, case.nscales, int(case.table), int(data["prefix"] is not None), int(use_async))


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    """the case files, written once and shared by both runs; left unchanged"""
    d = str(tmp_path_factory.mktemp("patchembed_cxx"))
    # (a pairwise cover holds every pair: BM + 1 tokens with oc = BN + 1 at BM 64, 2 BM + 2 tokens with the L 80 geometry at BM 128)
    tails = [c for c in R.shape_grid(64, R.U8) if (c.rows, c.oc) == (65, 129)][:1] + [c for c in R.shape_grid(128, R.S8) if (c.rows, c.ph, c.pw, c.ic) == (258, 3, 5, 16)][:1]
    assert len(tails) == 2 and tails[1].bs == 3, [c.ident() for c in tails]
    lines = []
    for use_async in (0, 1):
        lines.append(_write_case(d, "tail-a%d" % use_async, tails[0], use_async))
        lines.append(_write_case(d, "tail-b%d" % use_async, tails[1], use_async))
        lines.append(_write_case(d, "cls-tok%d" % use_async, R.CXX_CASE, use_async))
    with open(os.path.join(d, "cases.txt"), "w") as f:
        f.writelines(lines)
    return d


@pytest.mark.parametrize("shards", [1, 2], ids=["one-device", "two-shards"])
def test_patchembed_check_own_cases_and_three_written_shapes_sync_and_async(written, shards):
    assert os.path.exists(TOOL), "run __graft_entry__.build() first"
    env = dict(os.environ)
    env.pop("DEEPFUSION_DEVICES", None)
    if shards > 1:
        env["DEEPFUSION_DEVICES"] = str(shards)
    p = subprocess.run([TOOL, written], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, env=env)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    assert "patchembed_check: 6 entries from" in out and "DIFFERENT" not in out, out
    assert "patchembed_check: every case identical to the reference (14 cases)" in out, out
    assert out.count(" sync") >= 3 and out.count(" async") >= 3 and out.count("+table") >= 3 and out.count("+prefix") >= 3, out
