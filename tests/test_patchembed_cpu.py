"""CPU-only checks of the int8 patch-embedding op (dfx_patchembed_*): the numpy reference the GPU tests compare against
(tests/patchembed_ref.py) equals an element-by-element witness that indexes the image and the oihw weights directly, and
linear_ref on the patch matrix gathered on the host; the case tables hold the regime they are meant to hold; the op's host-side
plan and packer (csrc/patchembed_plan.h, patchembed_pack.h) agree with their Python mirror, byte for byte, and are clean under the
host sanitizers as a stand-alone program; the C ABI validates descriptors in the documented order before it touches a device; the
ctypes mirrors match the header; both libraries export the op and the tools exist; the two Python helpers follow their formulas."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

import linear_ref as L
import patchembed_ref as R

dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-fusion_amd")
INVALID, UNSUPPORTED, HIP, NO_DEVICE, STATE = 1, 2, 3, 4, 5


# ---- 1. the reference ------------------------------------------------------------------------------------------------------------
def _narrow(c, oc, **kw):
    """the case with fewer channels and the same pad elements behind them"""
    return R.with_case(c, oc=oc, dst_ld=oc + c.dld - c.oc, **kw)


def _small_cases():
    out = [c for bm in R.BMS for dt in (R.U8, R.S8) for c in R.shape_grid(bm, dt) if c.rows * c.oc * c.k <= 40000][::3]
    out += [_narrow(c, 11, bs=1) for c in R.table_cases() + R.tie_cases()[:4] + R.nonfinite_cases() + R.prefix_cases()]
    out += [_narrow(c, 5) for c in R.leftover_cases() + R.imgconv_twin_cases() + R.linear_twin_cases()]
    out += [_narrow(c, 3) for dt in (R.U8, R.S8) for c in R.shape_grid(64, dt) if c.bia_dt in (R.S8, R.U8) and c.k <= 768][:6]
    return out


def test_reference_equals_the_witness():
    """whole storage, bytes: every dst dtype, bias dtype, round mode, ReLU, per-channel scales, pitches, tables, prefix rows,
    leftover pixels, inf / NaN scales"""
    cases = _small_cases()
    assert len(cases) > 60
    seen = set()
    for case in cases:
        data = R.generate(case)
        assert np.array_equal(R.reference(case, data), R.witness(case, data)), case.ident()
        seen.add((case.src_dt, case.dst_dt, case.bia_dt, case.rm, case.table, case.prefix, bool(case.extra_h or case.extra_w)))
    assert {s[0] for s in seen} == {R.U8, R.S8} and {s[1] for s in seen} == {R.U8, R.S8, R.S32, R.F32}
    assert {s[2] for s in seen} == {R.UNDEF, R.U8, R.S8, R.S32, R.F32} and {s[3] for s in seen} == {0, 1}
    assert {s[4] for s in seen} == {False, True} and {s[5] for s in seen} == {False, True} and {s[6] for s in seen} == {False, True}
    for case, data in R.lane_map_cases(64):
        small = R.with_case(case, bs=1, oc=3)
        sdata = dict(data, src=data["src"][:1], w=data["w"][:3])
        assert np.array_equal(R.reference(small, sdata), R.witness(small, sdata)), case.ident()


def test_reference_equals_linear_ref_on_the_gathered_patch_matrix():
    """without a table the op is dfx_linear on the host-gathered patches with the weights in K order (ky, kx, i)"""
    cases = [c for c in R.linear_twin_cases() + R.imgconv_twin_cases() + R.leftover_cases() + list(R.shape_grid(64, R.S8))[::9] if not c.table]
    assert len(cases) >= 12
    for case in cases:
        data = R.generate(case)
        lc = R.lin_case(case)
        ldata = dict(src=R.gather(case, data).reshape(-1), w=R.permute_weights(case, data["w"]), bia=data["bia"], scales=data["scales"], lut=None)
        want = L.values(lc, ldata)
        got = R.values(case, data).reshape(case.rows, case.oc)
        assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), case.ident()
    # the gather itself, spelled out on one case: row (b, ty, tx), column (ky * pw + kx) * ic + i
    case = R.leftover_cases()[2]
    data = R.generate(case)
    g, img = R.gather(case, data), data["src"]
    for b, ty, tx, ky, kx, i in ((0, 0, 0, 0, 0, 0), (2, 1, 6, 3, 2, 1), (1, 0, 3, 2, 3, 2)):
        assert g[(b * case.th + ty) * case.tw + tx, (ky * case.pw + kx) * case.ic + i] == img[b, ty * case.ph + ky, tx * case.pw + kx, i]


def test_tables_hold_their_regime():
    """for every generated case the GPU files use: at most 10 % of the requant's outputs on a saturation bound
    (linear_ref.saturated_fraction's definition), except in the cases built to saturate, and no case all zero.  The data rule is
    the issue's; a few-channel case may draw its next seed (patchembed_ref.generate), which at most 2 % of the cases do."""
    cases = R.generated_cases()
    assert len(cases) > 400
    built = redrawn = 0
    for case in cases:
        data = R.generate(case)
        t = R.values(case, data)
        sat = R.saturated_fraction(case, t)
        redrawn += R.redraws(case) > 0
        if case.saturating:
            built += 1
            assert sat > 0.4 or case.dst_dt == R.F32, case.ident()
            continue
        assert sat <= R.SAT_CAP, (case.ident(), sat)
        assert t.view(np.uint8).any(), case.ident()
        if t.size >= 64:
            assert len(np.unique(t)) > 2, case.ident()
        if case.extra_h or case.extra_w:                                        # the leftover pixels hold 0xFF
            img = data["src"].view(np.uint8)
            assert (img[:, case.th * case.ph:] == 0xFF).all() and (img[:, :, case.tw * case.pw:] == 0xFF).all()
    assert built == 8 and redrawn <= len(cases) // 50, redrawn
    for bm in R.BMS:                                                            # the grid is a pairwise cover of the issue's axes
        rs = R.token_counts(bm)
        for dt in (R.U8, R.S8):
            g = R.shape_grid(bm, dt)
            geo = lambda c: (c.ph, c.pw, c.ic)  # noqa: E731
            assert {(c.rows, c.oc) for c in g} == {(r, n) for r in rs for n in R.OCS}
            assert {(c.rows, geo(c)) for c in g} == {(r, x) for r in rs for x in R.GEOMETRIES}
            assert {(c.oc, geo(c)) for c in g} == {(n, x) for n in R.OCS for x in R.GEOMETRIES}
            assert {c.bs for c in g} == {1, 2, 3} and {c.t0 for c in g} == {0, 1, 2} and {c.slack for c in g} == {0, 1, 2}
            assert {c.dst_dt for c in g} == {R.U8, R.S8, R.S32, R.F32} and {c.dld % 4 == 0 for c in g} == {True, False}
            assert {(c.table, c.bia_dt != R.UNDEF) for c in g} == {(True, False), (False, True), (False, False)}
            assert {(c.t0 > 0, c.prefix) for c in g} == {(False, False), (True, False), (True, True)}
            assert {c.granule for c in g} == {4, 16} and {c.rm for c in g} == {0, 1} and {c.relu for c in g} == {False, True}
    assert [R.granule(pw * ic, pw * ic) for ph, pw, ic in R.GEOMETRIES] == [16, 4, 16, 16, 16, 16, 16]
    assert [ph * pw * ic for ph, pw, ic in R.GEOMETRIES] == [768, 48, 16, 128, 240, 384, 4080]
    # the hand-built cases
    comp = R.compensation_cases()
    assert [c.k for c, _ in comp] == [R.KMAX, 65024] and [c.granule for c, _ in comp] == [0, 16]
    for case, data in comp:
        assert abs(R.accumulate(case, data)).max() == 255 * 128 * case.k and R.values(case, data).any()
    for bm in R.BMS:
        for case, data in R.lane_map_cases(bm):
            assert R.saturated_fraction(case, R.values(case, data)) == 0.0 and case.rows > bm and case.oc > R.BN
        assert {c.granule for c, _ in R.lane_map_cases(bm)} == {4, 16}
    assert R.tiles(R.desc_of(R.GRID_CAP_CASE), 64) == 12
    assert {c.granule for c in R.leftover_cases()} == {4, 16}
    assert (R.FRONT_CASE.bs, R.FRONT_CASE.ih, R.FRONT_CASE.iw, R.FRONT_CASE.ic, R.FRONT_CASE.ph, R.FRONT_CASE.oc, R.FRONT_CASE.t0) == (2, 32, 32, 3, 4, 64, 1)


# ---- 2. the plan and the packer against their mirror ------------------------------------------------------------------------------
# bs, ih, iw, ic, ph, pw, th, tw, oc, table, t0, cus, forced_bm, cap: n and K tails, both granules, leftover pixels
PLAN_SHAPES = [(1, 4, 4, 4, 4, 4, 1, 1, 1, 0, 0, 256, 0, 0), (3, 9, 20, 3, 4, 4, 2, 5, 133, 1, 1, 256, 0, 0), (3, 9, 24, 3, 4, 4, 2, 5, 133, 1, 2, 4, 0, 0),
               (8, 224, 224, 3, 16, 16, 14, 14, 768, 1, 1, 256, 0, 0), (8, 224, 224, 3, 16, 16, 14, 14, 768, 0, 0, 200, 0, 7),
               (2, 7, 26, 16, 3, 5, 2, 5, 129, 1, 0, 256, 128, 0), (2, 8, 9, 32, 2, 2, 4, 4, 127, 0, 3, 256, 64, 3), (5, 255, 3, 16, 255, 1, 1, 3, 3, 1, 0, 2, 0, 0)]


def _plan_tool(tmp_path, exe, shape, seed):
    bs, ih, iw, ic, ph, pw, th, tw, oc = shape[:9]
    w = np.random.default_rng(seed).integers(-128, 128, (oc, ic, ph, pw)).astype(np.int8)
    wf, imf = tmp_path / "w.bin", tmp_path / "img.bin"
    w.tofile(str(wf))
    out = subprocess.check_output([str(exe), "plan"] + [str(v) for v in shape] + [str(wf), str(imf)]).decode()
    plan = {ln.split()[0]: int(ln.split()[1]) for ln in out.splitlines() if len(ln.split()) == 2}
    return w, plan, np.fromfile(str(imf), dtype=np.uint8)


def _check_plans(tmp_path, exe):
    grans = set()
    for i, shape in enumerate(PLAN_SHAPES):
        bs, ih, iw, ic, ph, pw, th, tw, oc, table, t0, cus, forced, cap = shape
        w, plan, img = _plan_tool(tmp_path, exe, shape, 100 + i)
        case = R.PeCase("plan", bs, th, tw, ph, pw, ic, oc, table=bool(table), t0=t0, extra_h=ih - th * ph, extra_w=iw - tw * pw)
        d = R.desc_of(case, force_path=R.TILE)
        assert plan["validate"] == R.validate(d) == 0, shape
        bm = R.planned_bm(d, cus, forced)
        offs = R.image_offsets(d)
        assert plan["path"] == R.auto_path(d) == R.TILE and plan["granule"] == R.desc_granule(d) and plan["bm"] == bm and plan["tiles"] == R.tiles(d, bm), (shape, plan)
        assert plan["grid_tile"] == R.planned_grid(d, R.TILE, bm, cus, cap) and plan["grid_generic"] == R.planned_grid(d, R.GENERIC, bm, cus, cap), (shape, plan)
        assert plan["lds"] == R.lds_bytes(R.TILE, bm) and plan["fast"] == 1, (shape, plan)
        assert (plan["off_comp"], plan["off_bias"], plan["off_scale"], plan["off_ktab"], plan["off_table"], plan["off_prefix"], plan["bytes"]) == offs, (shape, plan)
        packed, comp = L.pack_weights(R.permute_weights(case, w))
        assert img.size == offs[5]
        assert np.array_equal(img[:offs[0]], packed), shape                                    # the weight section, byte for byte
        assert np.array_equal(img[offs[0]:offs[1]].view(np.int32), comp), shape                # the compensation
        assert not img[offs[1]:offs[2]].any(), shape                                           # no bias (and none with a table)
        scale = img[offs[2]:offs[3]].view(np.float32)
        assert (scale[:oc] == 1.0).all() and not scale[oc:].any(), shape
        kt = R.ktab(d)
        assert np.array_equal(img[offs[3]:offs[3] + 4 * kt.size].view(np.int32), kt) and not img[offs[3] + 4 * kt.size:offs[4]].any(), shape
        if table:
            t = img[offs[4]:offs[5]].view(np.float32).reshape(th * tw, R.table_ld(oc))
            assert (t[:, :oc] == 0.5).all() and not t[:, oc:].any(), shape
        grans.add(plan["granule"])
    assert grans == {4, 16}
    # one offset, spelled out: 4 x 4 x 3 patches in a 24-pixel-wide RGB image, granule 4: byte 28 of K is row 2 (28 // 12), byte 4
    d = R.desc_of(R.PeCase("k", 1, 2, 5, 4, 4, 3, 8, extra_w=4))
    assert R.desc_granule(d) == 4 and R.ktab(d)[7] == 2 * 24 * 3 + 4 and R.ktab(d).size == 16 and not R.ktab(d)[12:].any()


def test_patchembed_plan_check_is_clean_under_the_host_sanitizers_and_agrees_with_the_mirror(tmp_path):
    """tools/patchembed_plan_check.cc, a stand-alone host program over csrc/patchembed_plan.h and patchembed_pack.h, built with the
    flags of the host Makefile's SAN=1 rule (ASan + UBSan) into a scratch directory and run directly: its own checks, then plans
    and images of shapes with n and K tails and both granules against the Python mirror.  Nothing is loaded into Python."""
    src = os.path.join(PKG, "tools", "patchembed_plan_check.cc")
    assert os.path.exists(src), "tools/patchembed_plan_check.cc is missing"
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert "$(TOOLS)/patchembed_plan_check: $(TOOLS)/patchembed_plan_check.cc ../csrc/patchembed_plan.h ../csrc/patchembed_pack.h" in mk
    exe = tmp_path / "patchembed_plan_check"
    flags = ["-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++"] + flags + [src, "-o", str(exe)])
    p = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()
    assert "patchembed plans: validation order, granules, the auto rule, tile heights, grids, LDS, image sections, the K offset table, the packer" in p.stdout.decode()
    _check_plans(tmp_path, exe)


def test_mirror_validation_agrees_with_the_header_order():
    base = R.desc_of(R.PeCase("v", 2, 3, 5, 4, 4, 4, 40))
    assert R.validate(base) == 0 and R.desc_granule(base) == 16
    for kw in (dict(bs=0), dict(ic=0), dict(ph=0), dict(ph=256, ih=256 * 3), dict(pw=256, iw=256 * 5), dict(th=4), dict(th=0), dict(tw=6), dict(oc=0, dst_ld=1),
               dict(ph=255, pw=255, ic=2, ih=255 * 3, iw=255 * 5), dict(src_dt=R.F32), dict(dst_dt=0), dict(bia_dt=5), dict(round_mode=2), dict(nscales=2),
               dict(table=2), dict(table=1, bia_dt=R.S32), dict(tok_offset=-1), dict(force_path=2), dict(img_rows=14), dict(dst_ld=39), dict(bs=2 ** 40 // (12 * 20 * 4) + 1),
               dict(bs=2 ** 20, img_rows=2 ** 10, dst_ld=2 ** 10 + 1)):
        assert R.validate(dict(base, **kw)) == R.INVALID, kw
    odd = dict(base, ic=3)                                                              # 4 x 4 x 3 in a 20-pixel row: granule 4
    assert R.desc_granule(odd) == 4 and R.validate(dict(odd, force_path=R.TILE)) == 0
    out = dict(base, ic=3, pw=3, iw=15)
    assert R.desc_granule(out) == 0 and R.validate(dict(out, force_path=R.TILE)) == R.UNSUPPORTED and R.validate(out) == 0
    assert R.validate(dict(out, force_path=R.TILE, nscales=3)) == R.INVALID
    assert R.validate(dict(base, table=1, th=1, tw=1, oc=1, dst_ld=1, ih=2 ** 14, iw=2 ** 14, ph=1, pw=1)) == 0


# ---- 3. descriptor and build checks ------------------------------------------------------------------------------------------------
def _desc(**kw):
    d = dict(bs=2, ih=12, iw=20, ic=4, ph=4, pw=4, th=3, tw=5, oc=40, src_dt=capi.DFX_U8, dst_dt=capi.DFX_S8, bia_dt=capi.DFX_UNDEF, relu=0, round_mode=0,
             nscales=1, table=0, tok_offset=0, force_path=capi.PATCHEMBED_AUTO, img_rows=15, dst_ld=40)
    d.update(kw)
    desc = capi.PatchEmbedDesc()
    for k, v in d.items():
        setattr(desc, k, v)
    return desc


def _create(**kw):
    desc = _desc(**kw)
    h = ctypes.c_void_p()
    rc = capi.lib().dfx_patchembed_create(ctypes.byref(desc), ctypes.byref(h))
    msg = capi.lib().dfx_last_error().decode()
    if rc == 0:
        assert capi.lib().dfx_patchembed_destroy(h) == 0
    else:
        assert not h.value
    return rc, msg


def _admitted(**kw):
    rc, msg = _create(**kw)
    assert rc in (0, NO_DEVICE), (kw, rc, msg)


def test_descriptor_validation_needs_no_device():
    # every refusal, in the order of the checks: a descriptor with faults i and j > i reports i
    faults = [(dict(bs=0), "bs, ih"), (dict(ph=0), "ph, pw"), (dict(th=4), "th must"), (dict(tw=6), "tw must"), (dict(oc=0), "oc must"),
              (dict(src_dt=capi.DFX_F32), "src dtype"), (dict(dst_dt=5), "dst dtype"), (dict(bia_dt=5), "bias dtype"), (dict(round_mode=2), "round mode"),
              (dict(nscales=2), "scales count"), (dict(table=2), "table must"), (dict(tok_offset=-1), "tok_offset"), (dict(force_path=2), "force_path"),
              (dict(img_rows=14), "img_rows"), (dict(dst_ld=39), "dst_ld")]
    for i, (kw, word) in enumerate(faults):
        rc, msg = _create(**kw)
        assert rc == INVALID and word in msg, (kw, rc, msg)
        for kw2, _ in faults[i + 1:]:
            both = dict(kw2)
            both.update(kw)
            rc, msg = _create(**both)
            assert rc == INVALID and word in msg, (both, rc, msg)
    rc, msg = _create(table=1, bia_dt=capi.DFX_S32)
    assert rc == INVALID and "fold the bias" in msg
    rc, msg = _create(table=1, bia_dt=capi.DFX_S32, force_path=2)                        # the table's clause comes before force_path's
    assert rc == INVALID and "fold the bias" in msg
    for kw, word in ((dict(ih=0), "bs, ih"), (dict(iw=-1), "bs, ih"), (dict(ic=0), "bs, ih"), (dict(ph=256, ih=768), "ph, pw"), (dict(pw=-1), "ph, pw"),
                     (dict(th=0), "th must"), (dict(tw=0), "tw must"), (dict(ph=255, pw=255, ic=2, ih=765, iw=1275), "65025"),
                     (dict(oc=2 ** 31 - 127, dst_ld=2 ** 31), "oc must"), (dict(src_dt=0), "src dtype"), (dict(dst_dt=0), "dst dtype"), (dict(bia_dt=-1), "bias dtype"),
                     (dict(round_mode=-1), "round mode"), (dict(nscales=0), "scales count"), (dict(nscales=41), "scales count"), (dict(table=-1), "table must"),
                     (dict(force_path=-2), "force_path"), (dict(tok_offset=1), "img_rows"), (dict(bs=2 ** 40 // 960 + 1), "2^40"),
                     (dict(bs=2 ** 20, img_rows=2 ** 10, dst_ld=2 ** 10 + 1), "2^40"), (dict(ih=128, ph=128, th=1, iw=2 ** 22, img_rows=5), "2^31"),
                     (dict(table=1, ih=2 ** 12 + 1, iw=2 ** 14, ph=1, pw=1, th=2 ** 12 + 1, tw=2 ** 14, oc=1, dst_ld=1, img_rows=2 ** 27, ic=1, bs=1), "2^30")):
        rc, msg = _create(**kw)
        assert rc == INVALID and word in msg, (kw, rc, msg)
    for kw in (dict(), dict(ph=255, pw=255, ic=1, ih=765, iw=1275), dict(bs=1, ih=1, iw=1, ic=1, ph=1, pw=1, th=1, tw=1, oc=1, img_rows=1, dst_ld=1),
               dict(src_dt=capi.DFX_S8, dst_dt=capi.DFX_F32), dict(nscales=40), dict(bia_dt=capi.DFX_U8, dst_dt=capi.DFX_S32), dict(table=1), dict(th=1, tw=1),
               dict(tok_offset=2, img_rows=17), dict(tok_offset=2, img_rows=30, dst_ld=99), dict(round_mode=1, relu=1), dict(bs=2 ** 40 // 960),
               dict(force_path=capi.PATCHEMBED_TILE), dict(force_path=capi.PATCHEMBED_GENERIC), dict(force_path=capi.PATCHEMBED_TILE, ic=3),
               dict(table=1, ih=2 ** 12, iw=2 ** 14, ph=1, pw=1, th=2 ** 12, tw=2 ** 14, oc=1, dst_ld=1, img_rows=2 ** 26, ic=1, bs=1)):
        _admitted(**kw)
    # a forced path outside its class: unsupported, and only after everything invalid
    for kw in (dict(force_path=capi.PATCHEMBED_TILE, ic=3, pw=3, iw=15), dict(force_path=capi.PATCHEMBED_TILE, ic=3, iw=21), dict(force_path=capi.PATCHEMBED_TILE, ic=1, pw=2, iw=10)):
        rc, msg = _create(**kw)
        assert rc == UNSUPPORTED and "class" in msg, (kw, rc, msg)
        assert _create(dst_ld=39, **kw)[0] == INVALID
        assert _create(img_rows=2 ** 40, **kw)[0] == INVALID
        kw["force_path"] = capi.PATCHEMBED_GENERIC
        _admitted(**kw)
        kw["force_path"] = capi.PATCHEMBED_AUTO
        _admitted(**kw)
    lib = capi.lib()
    assert lib.dfx_patchembed_create(None, None) == INVALID
    assert lib.dfx_patchembed_set_weights(None, None, None, None) == INVALID
    assert lib.dfx_patchembed_set_table(None, None, 0) == INVALID
    assert lib.dfx_patchembed_set_prefix(None, None) == INVALID
    assert lib.dfx_patchembed_submit(None, None, None, None) == INVALID
    assert lib.dfx_patchembed_submit_host(None, None, None) == INVALID
    assert lib.dfx_patchembed_query(None, None) == INVALID
    assert lib.dfx_debug_patchembed_launches(None) == INVALID
    assert lib.dfx_debug_patchembed_requant(None, None) == INVALID
    assert lib.dfx_patchembed_destroy(None) == 0
    assert "null" in lib.dfx_last_error().decode()


def test_valid_descriptors_and_no_cpu_fallback():
    import torch
    for kw in (dict(), dict(src_dt=capi.DFX_S8, dst_dt=capi.DFX_F32, table=1), dict(force_path=capi.PATCHEMBED_TILE)):
        rc, msg = _create(**kw)
        if torch.cuda.is_available():
            assert rc == 0, (kw, msg)
        else:
            assert rc == NO_DEVICE and "no HIP device" in msg, (kw, rc, msg)
    if not torch.cuda.is_available():
        with pytest.raises(dfa.DfxError) as e:
            dfa.PatchEmbed((2, 12, 20, 4), 40, (4, 4))
        assert "dfx error 4" in str(e.value) and "no HIP device" in str(e.value)


def test_patchembed_structs_match_the_header(tmp_path):
    """dfx_patchembed_desc / dfx_patchembed_info compiled by gcc have the sizes and field offsets of the ctypes mirrors, and the
    prototypes of the header compile against calls with the documented argument types"""
    pairs = {"dfx_patchembed_desc": capi.PatchEmbedDesc, "dfx_patchembed_info": capi.PatchEmbedInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dfx.h"',
             'static int (*p_create)(const dfx_patchembed_desc *, dfx_patchembed_t **) = dfx_patchembed_create;',
             'static int (*p_weights)(dfx_patchembed_t *, const int8_t *, const void *, const float *) = dfx_patchembed_set_weights;',
             'static int (*p_table)(dfx_patchembed_t *, const float *, int64_t) = dfx_patchembed_set_table;',
             'static int (*p_prefix)(dfx_patchembed_t *, const void *) = dfx_patchembed_set_prefix;',
             'static int (*p_submit)(dfx_patchembed_t *, const void *, void *, dfx_stream_t) = dfx_patchembed_submit;',
             'static int (*p_host)(dfx_patchembed_t *, const void *, void *) = dfx_patchembed_submit_host;',
             'static int (*p_query)(const dfx_patchembed_t *, dfx_patchembed_info *) = dfx_patchembed_query;',
             'static int (*p_destroy)(dfx_patchembed_t *) = dfx_patchembed_destroy;',
             'static int (*p_launches)(int64_t *) = dfx_debug_patchembed_launches;',
             'static int (*p_requant)(const dfx_patchembed_t *, int32_t *) = dfx_debug_patchembed_requant;',
             'int main(void) {',
             '(void)p_create; (void)p_weights; (void)p_table; (void)p_prefix; (void)p_submit; (void)p_host; (void)p_query; (void)p_destroy; (void)p_launches; (void)p_requant;']
    for cname, ct in pairs.items():
        lines.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in ct._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    for name in ("DFX_PATCHEMBED_TILE", "DFX_PATCHEMBED_GENERIC", "DFX_VERSION"):
        lines.append('printf("enum %s %%d\\n", %s);' % (name, name))
    lines.append('printf("dfx_linear_desc size %zu\\n", sizeof(dfx_linear_desc));')
    lines.append("return 0; }")
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-c", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "abi.o")])
    body = "\n".join(ln for ln in lines if not ln.startswith("static int (*p_") and not ln.startswith("(void)p_"))
    src.write_text(body)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = {}
    for ln in subprocess.check_output([str(exe)]).decode().splitlines():
        a, b, c = ln.split()
        seen[(a, b)] = int(c)
    for cname, ct in pairs.items():
        assert seen[(cname, "size")] == ctypes.sizeof(ct), cname
        for fname, _ in ct._fields_:
            assert seen[(cname, fname)] == getattr(ct, fname).offset, (cname, fname)
    assert [n for n, _ in capi.PatchEmbedDesc._fields_] == ["bs", "ih", "iw", "ic", "ph", "pw", "th", "tw", "oc", "src_dt", "dst_dt", "bia_dt", "relu", "round_mode",
                                                            "nscales", "table", "tok_offset", "force_path", "img_rows", "dst_ld"]
    assert [n for n, _ in capi.PatchEmbedInfo._fields_] == ["path", "grid", "block", "lds_bytes", "device", "granule", "algorithmic_ops", "algorithmic_bytes",
                                                            "kernel_name"]
    assert seen[("enum", "DFX_PATCHEMBED_TILE")] == capi.PATCHEMBED_TILE == R.TILE == 0
    assert seen[("enum", "DFX_PATCHEMBED_GENERIC")] == capi.PATCHEMBED_GENERIC == R.GENERIC == 1
    assert capi.PATCHEMBED_AUTO == -1 and seen[("enum", "DFX_VERSION")] == 100
    assert ctypes.sizeof(capi.PatchEmbedDesc) == 88
    assert ctypes.sizeof(capi.LinearDesc) == seen[("dfx_linear_desc", "size")]            # the others are untouched


def test_library_exports_the_patchembed_entry_points():
    lib = capi.lib()
    for s in ("dfx_patchembed_create", "dfx_patchembed_set_weights", "dfx_patchembed_set_table", "dfx_patchembed_set_prefix", "dfx_patchembed_submit",
              "dfx_patchembed_submit_host", "dfx_patchembed_query", "dfx_patchembed_destroy", "dfx_debug_patchembed_launches", "dfx_debug_patchembed_requant"):
        assert s in dfa.declared_symbols() and hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s                              # bound with a signature
    assert not [s for s in dfa.declared_symbols() if not hasattr(lib, s)]
    for name in ("PatchEmbed", "PatchEmbedDesc", "PatchEmbedInfo", "PATCHEMBED_AUTO", "PATCHEMBED_TILE", "PATCHEMBED_GENERIC", "patchembed_launches",
                 "patch_embed_table", "patch_embed_prefix"):
        assert hasattr(dfa, name), name
    for key in ("DFX_PATCHEMBED_GRID", "DFX_PATCHEMBED_BM"):                         # known to the library
        capi.set_tuning(key, "1")
        capi.set_tuning(key, None)
    with pytest.raises(dfa.DfxError):
        capi.set_tuning("DFX_PATCHEMBED_TILES", "1")
    header = open(os.path.join(ROOT, "include", "dfx.h")).read()
    assert "DFX_PATCHEMBED_AUTO_NOTE" in header and "Parity unpinned: the reference has no such op" in header[header.index("int8 patch embedding"):]
    # the plan rests on linear_plan.h and the packer on linear_pack.h, which this op does not edit
    plan = open(os.path.join(PKG, "csrc", "patchembed_plan.h")).read()
    pack = open(os.path.join(PKG, "csrc", "patchembed_pack.h")).read()
    assert '#include "linear_plan.h"' in plan and '#include "linear_pack.h"' in pack and "lin_pack(" in pack and "hip" not in (plan + pack).replace("HIP", "").lower()


def test_dropin_layer_exports_patch_embed_and_tools_are_built():
    so = os.path.join(PKG, "libdeepfusion.so")
    assert os.path.exists(so), "run __graft_entry__.build() first"
    syms = subprocess.check_output(["nm", "-D", "-C", "--defined-only", so]).decode()
    assert "deepfusion::patch_embed(" in syms
    for tool in ("patchembed_check", "patchembed_plan_check", "bench_patchembed"):
        exe = os.path.join(PKG, "tools", tool)
        assert os.path.exists(exe) and os.access(exe, os.X_OK), tool
    p = subprocess.run([os.path.join(PKG, "tools", "patchembed_plan_check")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0 and "the route's proof hold" in p.stdout.decode(), p.stdout.decode()
    ignore = open(os.path.join(ROOT, ".gitignore")).read().split()
    for tool in ("patchembed_check", "patchembed_plan_check", "bench_patchembed"):
        assert "deep-fusion_amd/tools/" + tool in ignore, tool
    # the trace stub knows the new C-ABI calls: coherence_check links against it; the op is in neither recorded network
    stub = open(os.path.join(PKG, "tools", "dfx_trace_stub.cc")).read()
    for s in ("dfx_patchembed_create", "dfx_patchembed_set_weights", "dfx_patchembed_set_table", "dfx_patchembed_set_prefix", "dfx_patchembed_submit",
              "dfx_patchembed_destroy"):
        assert "int %s(" % s in stub, s
    assert "patch_embed" not in open(os.path.join(PKG, "tools", "pipeline_net.h")).read()


# ---- 4. the Python helpers ---------------------------------------------------------------------------------------------------------
def test_patch_embed_table_and_prefix_follow_their_formulas():
    """at their ends and at a tie"""
    pos = np.array([[0.5, -1.0, 3.0], [2.0, 0.0, -7.5]])
    t = dfa.patch_embed_table([1.0, 2.0, -3.0], pos, [0.5, 0.25, 2.0])
    assert t.dtype == np.float32 and t.shape == (2, 3)
    assert np.array_equal(t, np.array([[3.0, 4.0, 0.0], [6.0, 8.0, -5.25]], dtype=np.float32))
    assert np.array_equal(dfa.patch_embed_table(None, pos, 0.5), (pos * 2).astype(np.float32))
    # one rounding: (bias + pos) / step in float64, then to f32 -- not f32(bias) + f32(pos)
    b, p, s = 1.0, 2.0 ** -30, 3.0
    one = dfa.patch_embed_table([b], [[p]], s)[0, 0]
    assert one == np.float32((b + p) / s) and one.dtype == np.float32
    big = dfa.patch_embed_table([1e30], [[1e30]], 1e-10)                                  # beyond f32: inf, which set_table refuses
    assert np.isinf(big[0, 0])
    for bad in (dict(conv_bias=[1.0, 2.0], pos_embed=pos, acc_step=1.0), dict(conv_bias=None, pos_embed=pos, acc_step=[1.0, 2.0]),
                dict(conv_bias=None, pos_embed=pos, acc_step=0.0), dict(conv_bias=None, pos_embed=pos[0], acc_step=1.0),
                dict(conv_bias=None, pos_embed=pos, acc_step=float("nan"))):
        with pytest.raises(ValueError):
            dfa.patch_embed_table(**bad)
    # the prefix: ties to even, clamped at both ends of both dtypes
    cls = np.array([[0.5, 1.5, 2.5, -0.5, -1.5, 1000.0, -1000.0, 127.4]])
    r = dfa.patch_embed_prefix(cls, None, 1.0, np.int8)
    assert r.dtype == np.int8 and r.shape == (1, 8) and r.tolist() == [[0, 2, 2, 0, -2, 127, -128, 127]]
    u = dfa.patch_embed_prefix(cls, None, 1.0, np.uint8)
    assert u.dtype == np.uint8 and u.tolist() == [[0, 2, 2, 0, 0, 255, 0, 127]]
    two = dfa.patch_embed_prefix([[1.0, 2.0], [3.0, 4.0]], [[0.25, 0.5], [-3.0, 1.0]], 0.5)
    assert two.tolist() == [[2, 5], [0, 10]]                                              # 2.5 -> 2 (even), 5.0, 0.0, 10.0
    assert dfa.patch_embed_prefix([1.0, 3.0], None, 2.0).tolist() == [[0, 2]]              # {oc} is one row; 0.5 -> 0, 1.5 -> 2
    for bad in ((0.0, np.int8), (-1.0, np.int8), (float("inf"), np.int8), (1.0, np.int32)):
        with pytest.raises(ValueError):
            dfa.patch_embed_prefix(cls, None, *bad)
