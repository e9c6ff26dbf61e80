"""CPU-only checks of the squeeze-and-excitation op: the numpy reference the GPU tests compare against (tests/se_ref.py)
equals a scalar loop of the formula, its first stage is refmath's average pooling with the window of the image and its two
layers are fc_ref's fully-connected layer; the data of every table case keeps each stage away from degeneracy; the C ABI
validates descriptors before it touches a device, the ctypes mirrors match the header, the symbols are exported, the
drop-in layer and the tools are built, and the squeeze kernel's plan (csrc/se_plan.h) is clean under the host sanitizers
as a stand-alone program."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

import fc_ref
import refmath
import se_ref as S

dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-fusion_amd")
INVALID, UNSUPPORTED, HIP, NO_DEVICE = 1, 2, 3, 4
TABLE = S.table()
EXTRA = [S.SLICE_CASE] + S.GRID_CASES


# ---- 1. independent formulations ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in S.small_table() if c.bs * c.px * c.c <= 6000], ids=lambda c: c.ident())
def test_reference_equals_the_scalar_loop(case):
    data, st = S.generate(case)
    want = S.scalar_stages(case, data)
    for k in ("z", "h", "t", "g", "dst"):
        assert st[k].dtype == want[k].dtype and np.array_equal(st[k], want[k]), (case.ident(), k)


@pytest.mark.parametrize("case", TABLE + EXTRA, ids=lambda c: c.ident())
def test_squeeze_is_average_pooling_and_the_layers_are_fc(case):
    data, st = S.generate(case)
    z = refmath.avgpool(data["src"], (case.ih, case.iw), (1, 1), (0, 0), (1, 1), include_padding=False)
    assert z.dtype == np.uint8 and np.array_equal(z.reshape(case.bs, case.c), st["z"])
    f1 = fc_ref.FcCase("fc1", case.bs, case.c, 1, 1, case.cr, dst_dt=S.U8, bia_dt=case.bia1_dt, relu=True, rm=case.rm)
    h = fc_ref.fc_ref(f1, dict(src=st["z"].reshape(case.bs, 1, 1, case.c), w=data["w1"].reshape(case.cr, case.c, 1, 1),
                               bia=data["bia1"], scales=data["scales1"]))
    assert h.dtype == np.uint8 and np.array_equal(h, st["h"])
    f2 = fc_ref.FcCase("fc2", case.bs, case.cr, 1, 1, case.c, dst_dt=S.S8, bia_dt=case.bia2_dt, relu=False, rm=case.rm)
    t = fc_ref.fc_ref(f2, dict(src=st["h"].reshape(case.bs, 1, 1, case.cr), w=data["w2"].reshape(case.c, case.cr, 1, 1),
                               bia=data["bia2"], scales=data["scales2"]))
    assert t.dtype == np.int8 and np.array_equal(t, st["t"])
    assert np.array_equal(data["lut"][t.astype(np.int64) + 128], st["g"])


# ---- 2. the cases are not degenerate -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TABLE + EXTRA, ids=lambda c: c.ident())
def test_case_conditions_hold(case):
    data, st = S.generate(case)
    h, t, g, dst, src = st["h"], st["t"], st["g"], st["dst"], data["src"]
    assert np.mean(h == 0) <= 0.85
    assert np.mean(h == 255) <= 0.10
    assert np.mean((t == -128) | (t == 127)) <= 0.10
    assert len(np.unique(g)) >= min(12, case.bs * case.c / 2)
    if case.wide:
        assert case.px * case.c < 64 or np.any(dst == 255)       # the saturation the wide set is there for
    else:
        assert np.mean((dst == 0) | (dst == 255)) <= 0.20
    assert np.mean(dst != src) >= 0.5
    assert S.conditions(case, data, st) == []


@pytest.mark.parametrize("k", S.TIE_LOG2)
@pytest.mark.parametrize("rm", [0, 1])
def test_rescale_tie_data_holds_ties_and_the_reference_rounds_them_as_integers_say(k, rm):
    """tie_data's thresholds hold (it asserts them), the ties are what integer arithmetic says they are, and on them the
    reference gives the even neighbour (rm 0) or the floor (rm 1)"""
    case, data, st, n = S.tie_data(k, rm)
    print("SE TIES 2^-%d rm %d: %r of %d" % (k, rm, n, st["dst"].size))
    assert case.band_class and float(data["out_scales"][0]) == 2.0 ** -k and data["out_scales"].size == 1
    m = data["src"].astype(np.int64) * st["g"].astype(np.int64)[:, None, None, :]
    fl = m >> k
    tie = ((m & ((1 << k) - 1)) == (1 << (k - 1))) & (fl < 255)
    assert int(tie.sum()) == n["total"] >= 50 and n["below"] >= 15 and n["above"] >= 15
    want = fl if rm else fl + (fl & 1)
    assert np.array_equal(st["dst"][tie], want[tie].astype(np.uint8))
    if rm == 0:
        assert np.any(st["dst"][tie] == fl[tie]) and np.any(st["dst"][tie] == (fl + 1)[tie])


def test_table_covers_its_axes():
    assert {c.c for c in TABLE} == set(S.BAND_C + S.GENERIC_C)
    assert {c.cr for c in TABLE} == set(S.CRS) and {c.bs for c in TABLE} == set(S.BATCHES)
    for c in S.BAND_C + S.GENERIC_C:
        assert {(k.ih, k.iw) for k in TABLE if k.c == c} == set(S.IMAGES), c
    assert {c.rm for c in TABLE} == {0, 1} and any(c.wide for c in TABLE) and any(c.per_channel for c in TABLE)
    assert {c.bia1_dt for c in TABLE} == {S.S32, S.F32, S.UNDEF} == {c.bia2_dt for c in TABLE}
    assert all(c.band_class == (c.c % 16 == 0) for c in TABLE)
    lut = S.sigmoid_table()
    assert lut[128] == 128 and lut[0] == 1 and lut[255] == 254 and np.all(np.diff(lut.astype(int)) >= 0)
    assert S.hard_sigmoid_table()[0] == 0 and S.hard_sigmoid_table()[255] == 255


def test_planned_slices():
    """the mirror of se_plan.h: two workgroups per CU where the image allows it, 64 pixels per slice at least"""
    K = S.SeCase
    assert S.planned_slices(K("p", 64, 112, 112, 32, 8), 256) == 8          # 64 images -> 512 workgroups
    assert S.planned_slices(K("p", 1, 112, 112, 32, 8), 256) == 196         # 12544 / 64
    assert S.planned_slices(K("p", 1, 7, 7, 1152, 48), 256) == 1
    assert S.planned_slices(K("p", 1024, 56, 56, 96, 4), 256) == 1
    assert S.planned_slices(S.SLICE_CASE, 256, forced=10 ** 6) == 561 and S.planned_slices(S.SLICE_CASE, 256, forced=7) == 7


# ---- 3. the plan under the host sanitizers -------------------------------------------------------------------------------
def test_se_plan_check_is_clean_under_the_host_sanitizers(tmp_path):
    """tools/se_plan_check.cc, a stand-alone host program over csrc/se_plan.h, built by the host Makefile's SAN=1 rule
    (ASan + UBSan) into a scratch directory and run directly.  Nothing is loaded into Python."""
    src = os.path.join(PKG, "tools", "se_plan_check.cc")
    assert os.path.exists(src), "tools/se_plan_check.cc is missing"
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert "$(TOOLS)/se_plan_check: $(TOOLS)/se_plan_check.cc ../csrc/se_plan.h" in mk and "$(if $(SAN),-fsanitize=address$(comma)undefined" in mk
    exe = tmp_path / "se_plan_check"
    flags = ["-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++"] + flags + [src, "-o", str(exe)])
    p = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()
    assert "squeeze plans cover every pixel exactly once, leave no slice empty and flush within 257 pixels" in p.stdout.decode()


# ---- 4. descriptor and build checks -------------------------------------------------------------------------------------
def _create(**kw):
    d = dict(bs=2, c=32, ih=5, iw=7, cr=8, mode=capi.SE_SCALE, bia1_dt=capi.DFX_S32, bia2_dt=capi.DFX_UNDEF,
             round_mode=capi.ROUND_NEAREST, nscales1=1, nscales2=1, nscales_out=1, force_path=capi.SE_AUTO)
    d.update(kw)
    desc = capi.SeDesc(**d)
    h = ctypes.c_void_p()
    rc = capi.lib().dfx_se_create(ctypes.byref(desc), ctypes.byref(h))
    msg = capi.lib().dfx_last_error().decode()
    if rc == 0:
        assert capi.lib().dfx_se_destroy(h) == 0
    else:
        assert not h.value
    return rc, msg


def _admitted(huge=False, **kw):
    """a valid descriptor gets past validation: it creates with a device and fails with NO_DEVICE without one (huge: with
    a device, its scratch may be more than the device has -- a HIP error that names the buffers, not a refusal)"""
    rc, msg = _create(**kw)
    assert rc in (0, NO_DEVICE) or (huge and rc == HIP and "buffers" in msg), (kw, rc, msg)


def test_descriptor_validation_needs_no_device():
    for bad in ("bs", "c", "ih", "iw", "cr"):
        assert _create(**{bad: 0})[0] == INVALID, bad
        assert _create(**{bad: -3})[0] == INVALID, bad
        _admitted(**{bad: 1})
    # every cap at the last admitted value and the first refused one
    _admitted(bs=1, c=16, ih=4096, iw=2048)                                  # ih * iw = 2^23
    rc, msg = _create(bs=1, c=16, ih=4096, iw=2049)
    assert rc == INVALID and "2^23" in msg, (rc, msg)
    assert _create(bs=1, c=1, ih=2 ** 23 + 1, iw=1)[0] == INVALID
    _admitted(bs=1, c=1, ih=1, iw=2 ** 23)
    assert _create(bs=1, c=1, ih=65536, iw=65536)[0] == INVALID             # (the product does not fit an int)
    _admitted(c=16384, ih=1, iw=1)
    rc, msg = _create(c=16385, ih=1, iw=1)
    assert rc == INVALID and "16384" in msg, (rc, msg)
    _admitted(cr=16384, ih=1, iw=1)
    assert _create(cr=16385, ih=1, iw=1)[0] == INVALID
    _admitted(huge=True, bs=2 ** 26 - 1, c=16384, ih=1, iw=1)                          # bs * ih * iw * c = 2^40 - 2^14
    rc, msg = _create(bs=2 ** 26, c=16384, ih=1, iw=1)
    assert rc == INVALID and "2^40" in msg, (rc, msg)
    _admitted(huge=True, bs=7, c=16384, ih=4096, iw=2048, force_path=capi.SE_GENERIC)   # 7 * 2^37
    assert _create(bs=8, c=16384, ih=4096, iw=2048)[0] == INVALID
    assert _create(bs=2 ** 31 - 1, c=16384, ih=4096, iw=2048)[0] == INVALID
    for key, bad in (("mode", -1), ("mode", 3), ("bia1_dt", -1), ("bia1_dt", 5), ("bia2_dt", -1), ("bia2_dt", 5), ("round_mode", -1),
                     ("round_mode", 2), ("nscales1", 0), ("nscales1", 2), ("nscales1", 32), ("nscales2", 0), ("nscales2", 8),
                     ("nscales2", 31), ("nscales_out", 0), ("nscales_out", 8), ("nscales_out", 33), ("force_path", -2), ("force_path", 2)):
        assert _create(**{key: bad})[0] == INVALID, (key, bad)
    for kw in (dict(nscales1=8), dict(nscales2=32), dict(nscales_out=32), dict(nscales1=8, nscales2=32, nscales_out=32)):
        _admitted(**kw)
    for dt in (capi.DFX_UNDEF, capi.DFX_F32, capi.DFX_S32, capi.DFX_S8, capi.DFX_U8):
        _admitted(bia1_dt=dt, bia2_dt=dt)
    for mode in (capi.SE_SCALE, capi.SE_GATE, capi.SE_SQUEEZE):
        _admitted(mode=mode)
    # force_path = BAND outside the class: c no multiple of 16, or one image of 2^31 bytes or more
    for kw in (dict(c=1), dict(c=17), dict(c=40), dict(c=72), dict(c=120), dict(bs=1, c=256, ih=4096, iw=2048)):
        rc, msg = _create(force_path=capi.SE_BAND, **kw)
        assert rc == UNSUPPORTED and "class" in msg, (kw, rc, msg)
        _admitted(force_path=capi.SE_GENERIC, **kw)
        _admitted(**kw)
    for kw in (dict(c=16), dict(c=48), dict(c=1152), dict(bs=1, c=240, ih=4096, iw=2048)):
        _admitted(force_path=capi.SE_BAND, **kw)
    # an invalid field is reported before an unsupported combination
    assert _create(c=17, force_path=capi.SE_BAND, mode=9)[0] == INVALID
    lib = capi.lib()
    assert lib.dfx_se_create(None, None) == INVALID
    assert lib.dfx_se_set_weights(None, None, None, None, None, None, None, None, None) == INVALID
    assert lib.dfx_se_submit(None, None, None, None) == INVALID
    assert lib.dfx_se_submit_host(None, None, None) == INVALID
    assert lib.dfx_se_query(None, None) == INVALID
    assert lib.dfx_se_destroy(None) == 0


def test_valid_descriptors_and_no_cpu_fallback():
    import torch
    for kw in (dict(), dict(mode=capi.SE_GATE, c=17, cr=5), dict(mode=capi.SE_SQUEEZE, c=1152, cr=1), dict(round_mode=capi.ROUND_DOWN)):
        rc, msg = _create(**kw)
        if torch.cuda.is_available():
            assert rc == 0, (kw, msg)
        else:
            assert rc == NO_DEVICE and "no HIP device" in msg, (kw, rc, msg)
    if not torch.cuda.is_available():
        with pytest.raises(dfa.DfxError) as e:
            dfa.SqueezeExcite((1, 4, 4, 16), 4)
        assert "dfx error 4" in str(e.value) and "no HIP device" in str(e.value)


def test_se_structs_match_the_header(tmp_path):
    """dfx_se_desc / dfx_se_info compiled by gcc have the sizes and field offsets of the ctypes mirrors"""
    pairs = {"dfx_se_desc": capi.SeDesc, "dfx_se_info": capi.SeInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dfx.h"', 'int main(void) {']
    for cname, ct in pairs.items():
        lines.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in ct._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    for name in ("DFX_SE_BAND", "DFX_SE_GENERIC", "DFX_SE_SCALE", "DFX_SE_GATE", "DFX_SE_SQUEEZE", "DFX_VERSION"):
        lines.append('printf("enum %s %%d\\n", %s);' % (name, name))
    lines.append('printf("dfx_resize_desc size %zu\\n", sizeof(dfx_resize_desc));')
    lines.append("return 0; }")
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = {}
    for ln in subprocess.check_output([str(exe)]).decode().splitlines():
        a, b, c = ln.split()
        seen[(a, b)] = int(c)
    for cname, ct in pairs.items():
        assert seen[(cname, "size")] == ctypes.sizeof(ct), cname
        for fname, _ in ct._fields_:
            assert seen[(cname, fname)] == getattr(ct, fname).offset, (cname, fname)
    assert [n for n, _ in capi.SeDesc._fields_] == ["bs", "c", "ih", "iw", "cr", "mode", "bia1_dt", "bia2_dt", "round_mode", "nscales1",
                                                    "nscales2", "nscales_out", "force_path"]
    assert [n for n, _ in capi.SeInfo._fields_] == ["path", "slices", "grid", "block", "lds_bytes", "device", "algorithmic_bytes",
                                                    "kernel_name"]
    assert seen[("enum", "DFX_SE_BAND")] == capi.SE_BAND == S.BAND
    assert seen[("enum", "DFX_SE_GENERIC")] == capi.SE_GENERIC == S.GENERIC
    assert seen[("enum", "DFX_SE_SCALE")] == capi.SE_SCALE == S.SCALE == 0
    assert seen[("enum", "DFX_SE_GATE")] == capi.SE_GATE == S.GATE == 1
    assert seen[("enum", "DFX_SE_SQUEEZE")] == capi.SE_SQUEEZE == S.SQUEEZE == 2
    assert seen[("enum", "DFX_VERSION")] == 100 and capi.SE_AUTO == -1
    assert ctypes.sizeof(capi.SeDesc) == 52
    assert ctypes.sizeof(capi.ResizeDesc) == 48 == seen[("dfx_resize_desc", "size")]      # the others are untouched


def test_library_exports_the_se_entry_points():
    L = capi.lib()
    for s in ("dfx_se_create", "dfx_se_set_weights", "dfx_se_submit", "dfx_se_submit_host", "dfx_se_query", "dfx_se_destroy"):
        assert s in dfa.declared_symbols() and hasattr(L, s), s
    assert not [s for s in dfa.declared_symbols() if not hasattr(L, s)]
    for name in ("SqueezeExcite", "SeDesc", "SeInfo", "SE_AUTO", "SE_BAND", "SE_GENERIC", "SE_SCALE", "SE_GATE", "SE_SQUEEZE"):
        assert hasattr(dfa, name), name
    for key in ("DFX_SE_SLICES", "DFX_SE_GRID"):      # known to the library (an unknown key is refused)
        capi.set_tuning(key, "1")
        capi.set_tuning(key, None)
    with pytest.raises(dfa.DfxError):
        capi.set_tuning("DFX_SE_ROWS", "1")


def test_dropin_layer_exports_se_and_tools_are_built():
    so = os.path.join(PKG, "libdeepfusion.so")
    assert os.path.exists(so), "run __graft_entry__.build() first"
    syms = subprocess.check_output(["nm", "-D", "-C", "--defined-only", so]).decode()
    assert "deepfusion::squeeze_excite(" in syms and "deepfusion::global_avg_pool(" in syms
    for tool in ("se_check", "se_plan_check", "bench_se"):
        exe = os.path.join(PKG, "tools", tool)
        assert os.path.exists(exe) and os.access(exe, os.X_OK), tool
    p = subprocess.run([os.path.join(PKG, "tools", "se_plan_check")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0 and "flush within 257 pixels" in p.stdout.decode(), p.stdout.decode()
    ignore = open(os.path.join(ROOT, ".gitignore")).read().split()
    for tool in ("se_check", "se_plan_check", "bench_se"):
        assert "deep-fusion_amd/tools/" + tool in ignore, tool
