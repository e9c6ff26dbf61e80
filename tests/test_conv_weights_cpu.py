"""CPU-only checks of the conv op's weight packing and requant-route proofs (csrc/conv_weights.h over conv_plan.h, conv_geom.h
and requant_host.h): the header compiles as plain C++11 without any HIP include path; tools/conv_weights_check.cc, a
stand-alone host program over it, is clean under the host sanitizers, holds its self-check (every byte of every weight image
is the weight its layout comment names) and prints, for every case of tests/golden/conv_weights.json
(tests/conv_weights_golden.py), exactly the line that was recorded on an MI355X from the commit before this code left
dfx_api.hip: routes, roles, block, region sizes, the hash of each region, the kernel's name.  The golden's case list is
held to what it is there for: every family, every route, every proof deciding alone on either side of its bounds."""
import os
import subprocess

import numpy as np
import pytest

import conv_plan_golden as PG
import conv_weights_golden as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-fusion_amd")
SAN_FLAGS = ["-std=c++11", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def san_tool(tmp_path_factory):
    """tools/conv_weights_check.cc built with the flags of the host Makefile's SAN=1 rule (ASan + UBSan) into a temporary
    directory; it is run directly, as its own program.  Nothing is loaded into Python."""
    src = os.path.join(PKG, "tools", "conv_weights_check.cc")
    assert os.path.exists(src), "tools/conv_weights_check.cc is missing"
    exe = tmp_path_factory.mktemp("conv_weights") / "conv_weights_check"
    subprocess.check_call(["g++"] + SAN_FLAGS + [src, "-o", str(exe)])
    return str(exe)


@pytest.fixture(scope="module")
def golden():
    return G.load()


@pytest.fixture(scope="module")
def inputs(golden):
    """{case name: generated inputs}, made once"""
    return {c["name"]: G.generate(c["desc"], c["recipe"]) for c in golden["cases"]}


def _run(tool, text):
    p = subprocess.run([tool], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    assert not p.stderr, p.stderr.decode()                               # (a sanitizer report that did not end the run)
    return p.stdout.decode().splitlines()


def test_header_needs_no_hip(tmp_path):
    src = tmp_path / "only_weights.cc"
    src.write_text('#include "conv_weights.h"\nint main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(PKG, "csrc"), str(src)])
    text = open(os.path.join(PKG, "csrc", "conv_weights.h")).read()
    assert "#include <hip" not in text and "hipMalloc" not in text and "hipMemcpy" not in text and "getenv" not in text
    api = open(os.path.join(PKG, "csrc", "dfx_api.hip")).read()
    assert api.count("conv_pack_weights(") == 1                          # ONE call, in dfx_conv_set_weights
    for gone in ("fast_ok_channel", "stream_consts", "set_weights_stream", "set_weights_direct", "d_wei1", "d_consts"):
        assert gone not in api, gone


def test_build_rules_know_the_tool():
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert ("$(TOOLS)/conv_weights_check: $(TOOLS)/conv_weights_check.cc ../csrc/conv_weights.h ../csrc/conv_plan.h ../csrc/conv_geom.h "
            "../csrc/requant_host.h") in mk
    assert mk.count("$(TOOLS)/conv_weights_check ") >= 2                   # built by `all`, removed by `clean`
    hdrs = [ln for ln in open(os.path.join(PKG, "csrc", "Makefile")).read().splitlines() if ln.startswith("HDRS")][0]
    assert " conv_weights.h " in hdrs
    assert "deep-fusion_amd/tools/conv_weights_check" in open(os.path.join(ROOT, ".gitignore")).read().split()
    exe = os.path.join(PKG, "tools", "conv_weights_check")
    assert os.path.exists(exe) and os.access(exe, os.X_OK), "run __graft_entry__.build() first"


def test_self_check_is_clean_under_the_host_sanitizers(san_tool):
    p = subprocess.run([san_tool], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    assert "every byte is the weight its layout names, sizes are the plan's, the switches cap the routes" in out


def test_every_golden_line_is_reproduced(san_tool, golden):
    cases = golden["cases"]
    assert len(cases) >= 150 and len({c["name"] for c in cases}) == len(cases)
    lines = _run(san_tool, "".join(G.tool_line(c, golden["ncu"]) for c in cases))
    assert len(lines) == len(cases)
    for c, ln in zip(cases, lines):
        assert ln == c["line"], c["name"]


def test_python_generates_the_tools_inputs(san_tool, golden, inputs):
    """tests/test_gpu_conv_weights.py hands the library what the golden was recorded with"""
    lines = _run(san_tool, "".join(G.tool_line(c, golden["ncu"], "@inputs=1") for c in golden["cases"]))
    for c, ln in zip(golden["cases"], lines):
        assert ln == "inputs=" + G.inputs_hash(inputs[c["name"]]), c["name"]


def test_descs_are_the_plan_goldens(golden):
    plans = {c["name"]: c for c in PG.load()["cases"]}
    free = [G.DESC_FIELDS.index(k) for k in G.FREE_FIELDS]
    for c in golden["cases"]:
        o = plans[c["origin"]]
        assert not o["plan"].startswith("rc="), c["name"]
        assert [v for i, v in enumerate(c["desc"]) if i not in free] == [v for i, v in enumerate(o["desc"]) if i not in free], c["name"]
        assert c["per_cu"] == o["per_cu"] and all(c["tuning"].get(k) == v for k, v in o["tuning"].items()), c["name"]
        assert set(c["tuning"]) - set(o["tuning"]) <= {"DFX_NO_FAST", "DFX_NO_MAGIC"}, c["name"]   # (switches planning never reads)
        assert G.fields(c["line"])["name"].split("/")[0].split("<")[0] in (PG.fields(o["plan"])["name"].split("<")[0], "conv_mfma_roles_kernel")


_PLANS = {}


def _plan(origin):
    if not _PLANS:
        _PLANS.update({p["name"]: p for p in PG.load()["cases"]})
    return PG.fields(_PLANS[origin]["plan"])


def _family(c):
    """-> (family, the proofs that decide each stage's route there)"""
    d = dict(zip(G.DESC_FIELDS, c["desc"]))
    name, fused = G.fields(c["line"])["name"], d["oc1x1"] > 0
    roles_ok = _plan(c["origin"])["roles_ok"]
    if name.startswith("conv_mfma_"):
        s0 = ["fast_magnitude", "magic0"] + (["fma0"] if roles_ok else []) if fused else ["fast_magnitude", "magic1"]
        return ("resident_fused" if fused else "resident_unfused"), {0: s0, 1: ["fast_magnitude", "magic1"] + (["fma1"] if roles_ok else [])}
    if name.startswith("conv_stream_kernel"):
        return ("stream_fused" if fused else "stream_unfused"), {0: ["fast_fold"], 1: ["fast_fold"]}
    if name.startswith("conv_pw_kernel"):
        return "pointwise", {0: ["fast_fold", "fma0"]}
    if name.startswith("conv_direct_kernel"):
        return ("direct_fused" if fused else "direct_unfused"), {0: ["fast_fold", "fma0"], 1: ["fast_fold", "magic1", "fma1"]}
    assert name.startswith("conv_generic_kernel"), name
    return "generic", {0: [], 1: []}


def test_golden_covers_families_and_routes(golden):
    routes, names = {}, set()
    for c in golden["cases"]:
        fam, _ = _family(c)
        f = G.fields(c["line"])
        routes.setdefault(fam, set()).add(f["routes"])
        names.add(f["name"])
        if fam == "direct_fused" and f["name"].split("<")[1].split(",")[2] == "4" and f["name"].split("<")[1].split(",")[4] == str(G.U8):
            names.add("direct G4 u8")                                    # (conv_direct_kernel<nw, wo, G, wo1, dst, ...>)
    per_stage = lambda fam, s: {r[s] for r in routes[fam]}
    assert per_stage("resident_fused", 0) == {0, 1, 2, 3} and per_stage("resident_fused", 1) == {0, 1, 2, 3}
    assert routes["resident_unfused"] == {(0, -1), (1, -1), (2, -1)}
    assert routes["stream_fused"] == {(0, 0), (1, 1)} and routes["stream_unfused"] == {(0, -1), (1, -1)}
    assert per_stage("direct_fused", 0) == {0, 1, 3} and per_stage("direct_fused", 1) == {0, 1, 2, 3}
    assert routes["direct_unfused"] == {(0, -1), (1, -1), (3, -1)} and routes["pointwise"] == {(0, -1), (1, -1), (3, -1)}
    assert routes["generic"] == {(0, 0), (0, -1)}
    assert "direct G4 u8" in names
    assert any(n.startswith("conv_mfma_roles_kernel<") and n.endswith("/fma") for n in names)
    assert any(n.startswith("conv_mfma_roles_kernel<") and n.endswith("/magic") for n in names)
    # the roles decision changes block and name together; everything else keeps the plan's
    for c in golden["cases"]:
        f = G.fields(c["line"])
        assert f["roles"] == int(f["name"].startswith("conv_mfma_roles_kernel<")), c["name"]


def test_golden_pairs_straddle_every_bound(golden, inputs):
    """each tagged pair: the named proof holds in the :pass case and not in the :fail case, every other proof that decides
    the stage's route in that family holds alike in both, and the recorded routes of the stage differ"""
    pairs = {}
    for c in golden["cases"]:
        for t in c["tag"].split():
            if t.count(":") == 3:
                proof, bound, stage, side = t.split(":")
                pairs.setdefault((c["name"].rsplit("-", 1)[0], proof, bound, int(stage)), {})[side] = c
    seen = set()
    for (name, proof, bound, stage), p in pairs.items():
        assert set(p) == {"pass", "fail"}, name
        fam, used = _family(p["pass"])
        assert _family(p["fail"])[0] == fam and proof in used[stage], name
        holds = {side: G.proofs(inputs[c["name"]], stage) for side, c in p.items()}
        assert holds["pass"][proof] and not holds["fail"][proof], (name, holds)
        for other in used[stage]:
            assert other == proof or holds["pass"][other] == holds["fail"][other], (name, other)
        r = {side: G.fields(c["line"])["routes"][stage] for side, c in p.items()}
        assert r["pass"] > r["fail"], (name, r)
        seen.add((proof, bound))
    for want in (("fast_magnitude", "2^31"), ("fast_fold", "2^24"), ("fast_fold", "2^31"), ("magic0", "+2^22"), ("magic0", "-2^22"),
                 ("magic1", "MAGIC1_LO"), ("magic1", "2^24"), ("magic1", "scale*2^26"), ("fma0", "+2^23"), ("fma0", "-2^23"),
                 ("fma0", "scale>=0"), ("fma0", "scale*2^23"), ("fma1", "exact")):
        assert want in seen, want
    # MAGIC1_HI cannot decide alone (conv_weights_golden.py says why): one case lies beyond it
    beyond = [c for c in golden["cases"] if any(127 * int(p) + 128 * int(n) > G.MAGIC1_HI for p, n in zip(*G._pn(inputs[c["name"]]["w0"])))]
    assert beyond and all(G.fields(c["line"])["routes"][0] < 2 for c in beyond)


def test_golden_covers_scales_biases_modes_and_switches(golden, inputs):
    idx = {k: i for i, k in enumerate(G.DESC_FIELDS)}
    cases = golden["cases"]
    fused = [c for c in cases if c["desc"][idx["oc1x1"]]]
    assert {c["desc"][idx["bia0_dt"]] for c in cases} == {0, 1, 2, 3, 4} and {c["desc"][idx["bia1_dt"]] for c in fused} == {0, 1, 2, 3, 4}
    for k in ("conv0_round_mode", "conv1_round_mode"):
        assert {c["desc"][idx[k]] for c in fused} == {0, 1}, k
    assert {c["desc"][idx["conv0_nscales"]] > 1 for c in cases} == {False, True} and {c["desc"][idx["conv1_nscales"]] > 1 for c in fused} == {False, True}
    for sw in ("DFX_NO_FAST", "DFX_NO_MAGIC"):
        fams = {_family(c)[0] for c in cases if c["tuning"].get(sw) == "1"}
        assert {"resident_fused", "resident_unfused", "stream_fused", "direct_fused", "direct_unfused", "pointwise"} <= fams, (sw, fams)
    scales = [s for c in cases for k in ("scales0", "scales1") if inputs[c["name"]][k] is not None for s in inputs[c["name"]][k]]
    pow2 = lambda s: s > 0 and np.frexp(s)[0] == 0.5
    assert any(pow2(s) for s in scales) and any(s > 0 and not pow2(s) for s in scales) and any(s < 0 for s in scales) and any(s > 1e20 for s in scales)
    nonint = [c for c in cases for k in ("bia0", "bia1") if inputs[c["name"]][k] is not None and inputs[c["name"]][k].dtype == np.float32
              and (inputs[c["name"]][k] != np.floor(inputs[c["name"]][k])).any()]
    assert {_family(c)[0] for c in nonint} >= {"resident_fused", "resident_unfused", "stream_fused", "direct_fused", "generic"}
    gpu = [c for c in cases if c["tag"].startswith("gpu")]
    assert 8 <= len(gpu) <= 12 and sum(c["tag"] == "gpu+submit" for c in gpu) == 2
