"""CPU-only checks of the conv op's planner (csrc/conv_plan.h over csrc/conv_geom.h): both headers compile as plain C++11
without any HIP include path; tools/conv_plan_check.cc, a stand-alone host program over them, is clean under the host
sanitizers, holds its self-check (unit counts, magic numbers, LDS layouts, the hand-out rules of hipref.check_sched) and
prints, for every case of tests/golden/conv_plans.json (tests/conv_plan_golden.py), exactly the plan that was recorded on
an MI355X from the commit before the planner was moved out of dfx_api.hip -- or the recorded refusal."""
import os
import subprocess

import pytest

import conv_plan_golden as G
import hipref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-fusion_amd")
SAN_FLAGS = ["-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def san_tool(tmp_path_factory):
    """tools/conv_plan_check.cc built with the flags of the host Makefile's SAN=1 rule (ASan + UBSan) into a temporary
    directory; it is run directly, as its own program.  Nothing is loaded into Python."""
    src = os.path.join(PKG, "tools", "conv_plan_check.cc")
    assert os.path.exists(src), "tools/conv_plan_check.cc is missing"
    exe = tmp_path_factory.mktemp("conv_plan") / "conv_plan_check"
    subprocess.check_call(["g++"] + SAN_FLAGS + [src, "-o", str(exe)])
    return str(exe)


def test_planner_headers_need_no_hip(tmp_path):
    src = tmp_path / "only_plan.cc"
    src.write_text('#include "conv_plan.h"\nint main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(PKG, "csrc"), str(src)])
    for name in ("conv_plan.h", "conv_geom.h"):
        text = open(os.path.join(PKG, "csrc", name)).read()
        assert "#include <hip" not in text and "hipMalloc" not in text and "hipGet" not in text, name


def test_build_rules_know_the_planner():
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert "$(TOOLS)/conv_plan_check: $(TOOLS)/conv_plan_check.cc ../csrc/conv_plan.h ../csrc/conv_geom.h" in mk
    assert mk.count("$(TOOLS)/conv_plan_check ") >= 2                      # built by `all`, removed by `clean`
    hdrs = [ln for ln in open(os.path.join(PKG, "csrc", "Makefile")).read().splitlines() if ln.startswith("HDRS")][0]
    assert " conv_geom.h " in hdrs and " conv_plan.h " in hdrs
    assert "deep-fusion_amd/tools/conv_plan_check" in open(os.path.join(ROOT, ".gitignore")).read().split()
    exe = os.path.join(PKG, "tools", "conv_plan_check")
    assert os.path.exists(exe) and os.access(exe, os.X_OK), "run __graft_entry__.build() first"


def test_self_check_is_clean_under_the_host_sanitizers(san_tool):
    p = subprocess.run([san_tool], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    assert "unit counts, magic numbers, LDS layouts and the hand-out rules hold" in out


def test_every_golden_plan_is_reproduced(san_tool):
    g = G.load()
    cases = g["cases"]
    assert len(cases) >= 400 and len({c["name"] for c in cases}) == len(cases)
    text = "".join(" ".join([str(v) for v in c["desc"]] + [str(g["ncu"]), str(c["per_cu"])] + ["%s=%s" % kv for kv in c["tuning"].items()]) + "\n"
                   for c in cases)
    p = subprocess.run([san_tool], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    assert not p.stderr, p.stderr.decode()                               # (a sanitizer report that did not end the run)
    lines = p.stdout.decode().splitlines()
    assert len(lines) == len(cases)
    for c, ln in zip(cases, lines):
        if c["plan"].startswith("rc="):
            assert ln == c["plan"], c["name"]
            continue
        assert not ln.startswith("rc="), (c["name"], ln)
        head, name = ln.split(" name=", 1)
        got = dict(kv.split("=", 1) for kv in head.split(" "))           # every printed field, under the name the tool gives it
        want = G.fields(c["plan"])
        assert list(got) == [k for k in want if k != "name"], c["name"]
        got = {k: int(v) for k, v in got.items()}
        got["name"] = name
        assert got == want, (c["name"], {k: (got[k], want[k]) for k in want if got[k] != want[k]})


def test_golden_covers_what_it_is_there_for():
    """the recorded hand-outs satisfy hipref.check_sched, and every kernel family, refusal and rule of the case list occurs"""
    kinds = set()
    for c in G.load()["cases"]:
        if c["plan"].startswith("rc="):
            kinds.add(c["plan"].split(" ", 1)[1])
            continue
        p = G.fields(c["plan"])
        _, s, upx = G.hooks(p)
        if s is not None:
            class _Case:
                name, bs = c["name"], c["desc"][0]
            hipref.check_sched(_Case, dict(zip(hipref._SCHED_FIELDS, s)))
            kinds.add("resident" + ("+roles" if p["roles_ok"] else "") + ("+halves" if s[6] < s[5] else "") +
                      ("+runs" if upx else "") + ("+pool" if s[9] else "") + ("+lazy" if s[8] else ""))
        else:
            kinds.add(p["name"].split("<")[0] + (":pxb%d:occ_par%d" % (p["pxb"], p["s.occ_par"]) if "s.ni" in p else ""))
        if "[dst >= 4 GiB" in p["name"]:
            kinds.add("4 GiB")
    for k in ("conv_pw_kernel", "conv_direct_kernel", "conv_generic_kernel", "conv_stream_kernel:pxb1:occ_par0", "conv_stream_kernel:pxb2:occ_par0",
              "conv_stream_kernel:pxb1:occ_par1", "resident+roles", "resident+halves+lazy", "resident+runs+lazy", "resident+pool", "4 GiB",
              "conv_create: shape not covered by the MFMA variant", "conv_create: shape does not fit the streamed MFMA variant",
              "conv_create: fused pooling needs an unfused 3x3 stride-1 conv with 32/64 channels and even output size",
              "conv: non-positive dimension", "conv: bad dst dtype", "conv: bad bias dtype", "conv: bad bias1x1 dtype",
              "conv: ic and oc must be multiples of 16", "conv: output image size do not match", "conv: conv0 scales count must be 1 or oc",
              "conv: oc1x1 must be a multiple of 16", "conv: conv1 scales count must be 1 or oc1x1", "conv: bad round mode"):
        assert k in kinds, k
