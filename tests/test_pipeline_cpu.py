"""No GPU: the chained reference of tests/pipeline_ref.py is a test that can see a broken link.  A chain of saturated
tensors would pass whatever the ops in the middle do, so the reference itself is checked here, on the CPU: every u8
tensor lives inside (0, 255), the output depends on the frame and on the class, the tensors with several readers change
with the input -- and the whole chain is pinned against one recorded result, so that it cannot drift silently."""
import os

import numpy as np
import pytest

import hipref
import pipeline_ref as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pipeline_k.bin")


@pytest.fixture(scope="module")
def chain(oracle):
    p = P.generate()
    return p, [P.reference(oracle, p, p["x_%d" % f]) for f in range(P.FRAMES)]


def test_shapes_and_dtypes_are_the_tools(chain):
    _, frames = chain
    for t in frames:
        assert sorted(t) == sorted(P.TENSORS)
        for name, (dt, shape) in P.TENSORS.items():
            assert t[name].dtype == dt and t[name].shape == shape, name


def test_no_intermediate_is_saturated(chain):
    """in every u8 intermediate of every frame at least a quarter of the bytes lie strictly between 0 and 255"""
    _, frames = chain
    for f, t in enumerate(frames):
        for name in P.ORDER:
            v = t[name]
            if v.dtype != np.uint8:
                continue
            inside = float(np.mean((v > 0) & (v < 255)))
            print("frame %d %-3s %.2f of the bytes inside (0, 255)" % (f, name, inside))
            assert inside >= 0.25, (f, name, inside)


def test_output_depends_on_class_and_frame(chain):
    _, frames = chain
    ks = [t["k"] for t in frames]
    for f, k in enumerate(ks):
        assert np.all(np.isfinite(k))
        for n in range(P.N):
            assert np.unique(k[n]).size > 1, "k is constant over its classes (frame %d, image %d)" % (f, n)
    for a in range(P.FRAMES):
        for b in range(a + 1, P.FRAMES):
            assert not np.array_equal(ks[a].view(np.uint32), ks[b].view(np.uint32)), (a, b)


def test_shared_tensors_change_with_the_frame(chain):
    """b, c, d and e are the tensors several streams read (and e the one updated in place): a frame that found one of
    them still holding another frame's bytes must be visible"""
    _, frames = chain
    for name in ("b", "c", "d", "e"):
        for a in range(P.FRAMES):
            for b in range(a + 1, P.FRAMES):
                differ = float(np.mean(frames[a][name] != frames[b][name]))
                assert differ > 0.05, (name, a, b, differ)


def test_in_place_link_is_not_the_identity(chain):
    _, frames = chain
    for t in frames:
        assert float(np.mean(t["e"] != t["e0"])) > 0.5


def test_chain_matches_the_recorded_result(chain):
    """k of the four frames, 480 bytes recorded from this very chain when it was written"""
    _, frames = chain
    got = np.stack([t["k"] for t in frames])
    want = np.fromfile(GOLDEN, dtype=np.float32).reshape(got.shape)
    hipref.assert_bit_equal(got, want, "chained reference against tests/golden/pipeline_k.bin")
