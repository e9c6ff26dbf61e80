"""GPU: every op class of include/deepfusion.h chained through the C++ API with the tensors staying on the device
(tools/pipeline_check over tools/pipeline_net.h), bit for bit against the chained numpy / oracle references of
tests/pipeline_ref.py.  synchronous submits name a wrong link; one asynchronous frame and four frames in flight run the
stream ordering of host/deepfusion.cc for real (tests/test_coherence_cpu.py is the authoritative check of that ordering:
a race can pass here by luck); batch shards must give the single-device bytes.  Each run is a fresh child process."""
import os
import subprocess

import pytest

import hipref
import pipeline_ref as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "deep-fusion_amd", "tools", "pipeline_check")


@pytest.fixture(scope="module")
def net(oracle, tmp_path_factory):
    """inputs on disk, and the reference of every tensor of every frame, computed once"""
    p = P.generate()
    indir = tmp_path_factory.mktemp("pipeline_in")
    P.write_inputs(str(indir), p)
    return str(indir), [P.reference(oracle, p, p["x_%d" % f]) for f in range(P.FRAMES)]


def _run(mode, indir, outdir, shards=None):
    assert os.path.exists(EXE), "run __graft_entry__.build() first"
    env = {k: v for k, v in os.environ.items() if k not in ("DEEPFUSION_DEVICES", "DEEPFUSION_PROFILE")}
    if shards:
        env["DEEPFUSION_DEVICES"] = shards
    os.makedirs(str(outdir), exist_ok=True)
    r = subprocess.run([EXE, mode, indir, str(outdir)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, "pipeline_check %s exited with %d:\n%s" % (mode, r.returncode, r.stdout.decode())
    return str(outdir)


def test_sync_every_link(net, tmp_path):
    indir, frames = net
    out = _run("sync", indir, tmp_path)
    for name in P.ORDER:        # in pipeline order: the first name that fails is the broken link
        hipref.assert_bit_equal(P.load(out, name), frames[0][name], "sync: " + name)


def test_async_one_frame(net, tmp_path):
    indir, frames = net
    out = _run("async", indir, tmp_path)
    for name in ("k",) + tuple(n for n in P.ORDER if n not in ("k", "e0")):     # (e0 is overwritten in place)
        hipref.assert_bit_equal(P.load(out, name), frames[0][name], "async: " + name)


def test_four_frames_in_flight(net, tmp_path):
    indir, frames = net
    out = _run("frames", indir, tmp_path)
    for f in range(P.FRAMES):
        hipref.assert_bit_equal(P.load(out, "k", "k_%d.bin" % f), frames[f]["k"], "frames: k_%d" % f)


def test_two_batch_shards_give_the_same_bytes(net, tmp_path):
    """DEEPFUSION_DEVICES=2, batch 3 = 2 + 1: every file of the synchronous run equals the single-device run's"""
    indir, frames = net
    one, two = _run("sync", indir, tmp_path / "one"), _run("sync", indir, tmp_path / "two", shards="2")
    names = sorted(os.listdir(one))
    assert names == sorted(os.listdir(two)) == sorted(n + ".bin" for n in P.ORDER)
    for n in names:
        with open(os.path.join(one, n), "rb") as a, open(os.path.join(two, n), "rb") as b:
            assert a.read() == b.read(), n
    hipref.assert_bit_equal(P.load(two, "k"), frames[0]["k"], "two shards: k")


def test_two_batch_shards_stepwise_async(net, tmp_path):
    """the documented contract of batch shards: submit_async() with the producer's wait() before every consumer --
    including the two op classes that are not sharded (conv_relu_pool, eltwise_sum) between sharded neighbours"""
    indir, frames = net
    out = _run("stepwise", indir, tmp_path, shards="2")
    for name in P.ORDER:
        hipref.assert_bit_equal(P.load(out, name), frames[0][name], "two shards, stepwise: " + name)
