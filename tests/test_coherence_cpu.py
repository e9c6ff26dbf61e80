"""No GPU: the host/device coherence protocol of host/deepfusion.cc is free of data races when every op class is
chained with the tensors staying on the device.  tools/coherence_check is host/deepfusion.cc over a recording fake of
the C ABI (tools/dfx_trace_stub.cc): it drives two networks through include/deepfusion.h -- the one of
tools/pipeline_net.h (14 op classes, scenarios a - f) and token_net of tools/coherence_check.cc (the other ten, scenarios
g and h) -- and checks the recorded trace with vector clocks: for every two accesses to overlapping bytes of one buffer,
at least one of them a write, one must happen-before the other.  Its --dump, every call of the C ABI in call order, is
compared with tests/golden/coherence/.  One process per scenario (DEEPFUSION_DEVICES is read once)."""
import difflib
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "deep-fusion_amd", "tools", "coherence_check")

# scenario -> (environment, launches the trace must hold).  One frame is 14 ops = 14 launches of the fake (its handles
# are one launch each); two batch shards double the eleven sharded op classes and leave conv_relu_pool and eltwise_sum.
SCENARIOS = {
    "a": ({}, 14),                                                    # every op with submit()
    "b": ({}, 14),                                                    # one frame of submit_async(), one wait()
    "c": ({}, 4 * 14),                                                # four frames in flight
    "d": ({}, 2 * 14),                                                # synchronous and asynchronous submits mixed
    "e": ({}, 18),                                                    # ops destroyed while their launch is in flight
    "f": ({"DEEPFUSION_DEVICES": "2", "DFX_TRACE_DEVICES": "2"}, 2 * (2 * 12 + 2)),   # batch 3 over two shards
    # token_net is 10 ops = 10 launches.  g: one frame of submit(), two of submit_async(), then scaled_sum, matmul,
    # squeeze_excite and head once more around the two in-flight destructions
    "g": ({}, 3 * 10 + 4),
    # h: a frame of submit() and one of submit_async(); two shards double layer_norm, scaled_sum, squeeze_excite and head
    "h": ({"DEEPFUSION_DEVICES": "2", "DFX_TRACE_DEVICES": "2"}, 2 * (2 * 4 + 6)),
}
GOLDEN = os.path.join(ROOT, "tests", "golden", "coherence")
# golden file -> (scenario, environment on top of the scenario's own)
DUMPS = dict({s: (s, {}) for s in SCENARIOS}, a_profile=("a", {"DEEPFUSION_PROFILE": "1"}))


def _run(scenario, *args, **more_env):
    assert os.path.exists(EXE), "run __graft_entry__.build() first"
    env = {k: v for k, v in os.environ.items() if k not in ("DEEPFUSION_DEVICES", "DFX_TRACE_DEVICES", "DEEPFUSION_PROFILE")}
    env.update(SCENARIOS[scenario][0])
    env.update(more_env)
    p = subprocess.run([EXE, scenario] + list(args), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    return p.returncode, p.stdout.decode()


def _counts(out):
    m = re.search(r"records (\d+) launches (\d+) copies (\d+) syncs (\d+) waits (\d+) races (\d+) stub_errors (\d+)", out)
    assert m, out
    return dict(zip(("records", "launches", "copies", "syncs", "waits", "races", "stub_errors"), map(int, m.groups())))


@pytest.mark.parametrize("scenario", sorted(SCENARIOS))
def test_scenario_is_race_free(scenario):
    rc, out = _run(scenario)
    assert rc == 0 and "RACE" not in out and "STUB ERROR" not in out, out
    n = _counts(out)
    assert n["races"] == 0 and n["stub_errors"] == 0, out
    assert n["launches"] == SCENARIOS[scenario][1], out      # the scenario really ran all of its ops
    assert "scenario %s: race-free" % scenario in out, out


def test_synchronous_submit_orders_by_its_own_syncs_alone():
    """submit() uploads, launches, downloads and waits: one frame of it needs no stream-to-stream edge at all, and the
    ordering added for asynchronous chains must not cost it one (nor a copy or a wait more than an op has: per op one
    upload per input, one download, one sync; set_weights syncs once more for each of the ten ops with weights)."""
    n = _counts(_run("a")[1])
    assert n["waits"] == 0
    inputs = 1 + (1 + 1 + 1 + 1 + 1 + 1 + 2 + 2 + 1 + 2 + 1 + 3) + 1      # sources of reorder, the twelve, inner_product
    assert n["copies"] == inputs + 14
    assert n["syncs"] == 14 + 10


def test_the_trace_names_what_it_orders():
    """--dump: the multi-frame trace shows the write-after-read edges themselves -- the first op of a later frame waits
    for the reader of q before it overwrites q, and an in-place op never waits for its own stream"""
    rc, out = _run("c", "--dump")
    assert rc == 0, out
    lines = out.splitlines()
    waits = [re.match(r"dfx_stream_wait_stream stream (\d+) waits for stream (\d+)", ln) for ln in lines]
    waits = [m for m in waits if m]
    assert waits and all(m.group(1) != m.group(2) for m in waits), out
    stream_of = {}
    for ln in lines:
        m = re.match(r"(dfx_\w+_submit) stream (\d+)", ln)
        if m:
            stream_of.setdefault(m.group(1), []).append(m.group(2))
    reorders, imgconv = stream_of["dfx_reorder_submit"], stream_of["dfx_imgconv_submit"][0]
    assert len(set(reorders)) == 4                       # four first ops, four streams
    for s in reorders[1:]:                               # frames 1..3 overwrite q behind image_conv's read of it
        assert any(m.group(1) == s and m.group(2) == imgconv for m in waits), (s, imgconv)


@pytest.mark.parametrize("name", sorted(DUMPS))
def test_dump_equals_the_recorded_call_sequence(name):
    """--dump is every call host/deepfusion.cc makes into the C ABI, in call order: device switches, creates, allocations,
    copies, launches, waits, syncs, destroys (and, under DEEPFUSION_PROFILE=1, the event calls and the name() strings).
    It must equal tests/golden/coherence/<name>.txt byte for byte.  The files were recorded from the commit before the 24
    op classes of host/deepfusion.cc shared one skeleton (built with make DEEPFUSION_CC=<that revision's file>), so they
    pin that the shared skeleton calls what the 24 copies called.  A deliberate change of the call sequence regenerates
    them, one --dump run per file in the file's environment:
        coherence_check <a..e, g> --dump > tests/golden/coherence/<s>.txt
        DEEPFUSION_DEVICES=2 DFX_TRACE_DEVICES=2 coherence_check <f, h> --dump > tests/golden/coherence/<s>.txt
        DEEPFUSION_PROFILE=1 coherence_check a --dump > tests/golden/coherence/a_profile.txt"""
    scenario, env = DUMPS[name]
    rc, out = _run(scenario, "--dump", **env)
    assert rc == 0, out[-2000:]
    with open(os.path.join(GOLDEN, name + ".txt")) as f:
        want = f.read()
    if out != want:
        diff = list(difflib.unified_diff(want.splitlines(), out.splitlines(), "golden/%s.txt" % name, "coherence_check --dump", lineterm="", n=5))
        end = next((i for i, ln in enumerate(diff[3:], 3) if ln.startswith("@@")), len(diff))      # the first differing region
        pytest.fail("the call sequence differs from the recorded one\n" + "\n".join(diff[:min(end, 80)]), pytrace=False)


def _selftest(mode):
    p = subprocess.run([EXE, mode], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    return p.returncode, p.stdout.decode()


def test_the_checker_sees_races_when_the_edges_are_missing():
    """the checker itself, on a hand-made trace through the fake's C ABI: a write, a read on another stream, a rewrite of
    half the buffer, a host write of the uploaded bytes.  With a wait or a sync between each pair it is race-free; without
    them it reports read-after-write, write-after-read and both host-against-upload pairs, and the wait on a stream that
    was destroyed."""
    rc, out = _selftest("selftest-ordered")
    assert rc == 0 and "RACE" not in out and _counts(out)["races"] == 0, out
    rc, out = _selftest("selftest-race")
    n = _counts(out)
    assert rc == 1 and n["races"] == 4 and n["stub_errors"] == 1, out
    races = [ln for ln in out.splitlines() if ln.startswith("RACE")]
    assert "dfx_memcpy_h2d (stream 1, write" in races[0] and "dfx_memcpy_d2h (stream 2, read" in races[0], out    # RAW
    assert "dfx_memcpy_d2h (stream 2, read" in races[1] and "dfx_memcpy_h2d (stream 1, write" in races[1], out    # WAR
    assert all("host rewrites h1 (host, write" in r for r in races[2:]), out
    assert "stream 2 was destroyed" in out, out
