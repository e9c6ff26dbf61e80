"""Pixel-run units of the resident-weight kernel (conv_mfma.cuh, MfmaGeom::upx): a unit is a
run of U consecutive pixels of one image in row-major order instead of whole rows, so that every 32-pixel tile but an
image's last is full.

GPU tests: every case forces the mode with DFX_UNIT_PX (and DFX_STORE_BOUND_BYTES / DFX_NO_ROLES where the shape needs
it), asserts Conv.unit_px() == U on a handle created under the same switches, compares the WHOLE output bit for bit
with the CPU oracle through hipref.hip_conv_guarded (guard bands, poisoned dst, check_sched), and asserts that a run
with DFX_UNIT_PX=0 -- row units, the kernel as it was -- gives identical bytes.

Two cases of the list this file was written from cannot reach the mode as stated, and say so instead of silently
testing something else:
  * "unfused, oc = 128": the resident kernel takes oc in {32, 64} only, an unfused oc = 128 op runs on another kernel
    family.  test_unfused runs oc = 64 (pixel runs asserted) AND oc = 128 (unit_px() == 0 asserted, oracle compared).
  * "5 x 200, U = 128": its halo tile (4 rows x 202 columns x 2 chunks = 1616 granules) is larger than the 1408 the
    loader wave holds in registers.  The planner keeps such tiles out of the DEFAULT rule (speed), but a forced
    DFX_UNIT_PX admits them when they fit the ring slot; the rest of the tile is staged by the loader's synchronous
    path (write_rest), which this case therefore covers for pixel runs.

CPU test (no GPU marker): dfx_conv_create needs a device (it sizes the grid from the device's CU count), so the host
arithmetic is checked against a pure-Python restatement of the planner's rule (_plan below), not against
Conv.sched(); the GPU cases tie the two together (uy / ntu-derived fields of Conv.sched() are compared with _plan)."""
from dataclasses import replace

import numpy as np
import pytest

import cases as C

MFMA_LC = 22          # conv_mfma.cuh: 16-byte granules per loader lane
LDS_MAX = 163840


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import hipref
    return hipref


# ---- the planner's rule, restated (dfx_api.hip: pick_geometry) ------------------------------------------------------
def _tile_max(ic, oc, oc1, ctrl=128):
    cst = (3 * oc + 5 * oc1) if oc1 else 5 * oc
    fixed = (oc // 32) * 9 * (ic // 32) * 1024 + (oc1 // 32) * (oc // 32) * 1024 + (cst * 4 + 15) // 16 * 16 + ctrl
    return (LDS_MAX - fixed) // 4


def _plan(bs, oh, ow, ic, oc, oc1, U, forced=True):
    """-> dict(rmax, uy, ntu, total_units, tile_chunks) or None where U is illegal (row units then)"""
    if U < 32 or U % 32 or U >= 32768 or ow < 2 or ow >= 65536 or oh * ow * ow >= 1 << 31:
        return None
    rmax = -(-(ow - 1 + U) // ow)
    chunks = (rmax + 2) * (ow + 2) * (ic // 16)
    if (chunks + 63) // 64 * 1024 + 1024 > _tile_max(ic, oc, oc1):
        return None
    if not forced and chunks > 64 * MFMA_LC:
        return None
    uy = -(-(oh * ow) // U)
    return dict(rmax=rmax, uy=uy, ntu=U // 32, total_units=bs * uy, tile_chunks=chunks)


def test_unit_table_host_arithmetic():
    """random (oh, ow, ic, U): the unit table the rule implies covers every pixel of an image exactly once, no unit
    touches more than rmax rows, uy / ntu / total_units are as defined, the tile count is the output's own
    (only an image's last tile may be partial), and the multiply-high division the kernel uses for a run's first
    row is exact.  Pure-Python restatement: creating a handle needs a device (module docstring)."""
    rng = np.random.default_rng(7)
    seen_legal = seen_illegal = 0
    shapes = [(56, 56, 64, 96), (56, 56, 64, 128), (56, 56, 64, 160), (56, 56, 64, 192), (55, 56, 64, 128),
              (7, 7, 32, 64), (5, 200, 32, 128), (20, 24, 32, 96), (28, 60, 32, 96)]
    for _ in range(300):
        shapes.append((int(rng.integers(1, 130)), int(rng.integers(2, 260)), int(rng.choice([32, 64])),
                       32 * int(rng.integers(1, 12))))
    for oh, ow, ic, U in shapes:
        bs = 3
        p = _plan(bs, oh, ow, ic, 64, 256, U)
        if (oh, ow, ic, U) == (56, 56, 64, 192):
            assert _plan(bs, oh, ow, ic, 64, 256, U, forced=False) is None   # 7 halo rows: not by default
        if p is None:
            seen_illegal += 1
            continue
        seen_legal += 1
        opx = oh * ow
        assert p["rmax"] == -(-(ow - 1 + U) // ow) and p["ntu"] * 32 == U
        assert p["uy"] == -(-opx // U) and p["total_units"] == bs * p["uy"]
        cover = np.zeros(opx, dtype=np.int32)
        magic = ((1 << 32) + ow - 1) // ow
        tiles = 0
        for u in range(p["uy"]):
            p0 = u * U
            n = min(U, opx - p0)
            assert n > 0
            cover[p0:p0 + n] += 1
            y0 = (p0 * magic) >> 32
            assert y0 == p0 // ow, (oh, ow, U, u)
            xs = p0 - y0 * ow
            rows = (xs + n - 1) // ow + 1
            assert rows <= p["rmax"], (oh, ow, U, u, rows, p)
            assert y0 + rows <= oh
            for ti in range(p["ntu"]):              # the tile decode of the compute waves
                if 32 * ti >= n:
                    continue
                tiles += 1
                nvalid = min(32, n - 32 * ti)
                assert nvalid == 32 or (u == p["uy"] - 1 and 32 * ti + nvalid == n)
                pc = xs + 32 * ti + nvalid - 1
                assert (pc * magic) >> 32 == pc // ow and pc // ow < p["rmax"]
        assert (cover == 1).all()
        assert tiles == -(-opx // 32)
    assert seen_legal > 50 and seen_illegal > 5
    h = _plan(128, 56, 56, 64, 64, 256, 128, forced=False)       # the headline: 25 units and 98 tiles per image
    assert h["uy"] == 25 and h["total_units"] == 3200 and h["rmax"] == 4 and h["ntu"] == 4


# ---- GPU cases -----------------------------------------------------------------------------------------------------
def _unit_px(hip, case, data):
    op = hip.make_conv(case, data)
    try:
        return op.unit_px()
    finally:
        op.close()


class _Ref:
    def __init__(self, hip, oracle, case, data):
        import torch
        self.np = hip.oracle_conv(oracle, case, data)
        self.dev = torch.from_numpy(self.np).cuda()


def _run(hip, case, data, ref, what):
    got, info, s = hip.hip_conv_guarded(case, data, on_device=True)
    hip.assert_dev_bit_equal(got, ref.np, "%s %s %r" % (what, info.kernel_name.decode(), case), ref.dev)
    return got, info, s


def _check_case(hip, oracle, tuning, case, U, switches=(), ref=None, data=None):
    """the mode forced to U: unit_px, Conv.sched() against _plan, oracle parity; then DFX_UNIT_PX=0: same bytes"""
    import torch
    data = C.generate(case) if data is None else data
    ref = _Ref(hip, oracle, case, data) if ref is None else ref
    for k, v in switches:
        tuning.setenv(k, v)
    tuning.setenv("DFX_UNIT_PX", str(U))
    assert _unit_px(hip, case, data) == U, (case, U, switches)
    got, info, s = _run(hip, case, data, ref, "DFX_UNIT_PX=%d %r" % (U, switches))
    assert info.kernel_name.decode().startswith("conv_mfma_fused_kernel"), info.kernel_name
    p = _plan(case.bs, case.oh, case.ow, case.ic, case.oc, case.oc1x1, U)
    assert p is not None
    assert (s.th, s.tw, s.linear, s.uy, s.ux, s.total_units) == (p["rmax"], case.ow, 1, p["uy"], 1, p["total_units"]), (s, p)
    assert s.half_from >= s.total_units and s.roles == 0, s
    tuning.setenv("DFX_UNIT_PX", "0")
    assert _unit_px(hip, case, data) == 0
    got0, _, s0 = _run(hip, case, data, ref, "DFX_UNIT_PX=0 %r" % (switches,))
    assert torch.equal(got.view(torch.uint8), got0.view(torch.uint8)), "pixel runs and row units differ"
    tuning.undo()
    return got, s


PX56 = C.ConvCase("px56", 3, 64, 56, 56, 64, 256, dst_dt=C.S32)
NARROW = C.ConvCase("px20x24", 2, 32, 20, 24, 32, 128, dst_dt=C.F32, relu1=False)

gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("U", [128, 96])
def test_headline_shape(hip, oracle, tuning, U):
    """56 x 56, 64 -> 64 -> 256 s32, three images: units start mid-row, an image's last unit is short (64 / 64 px)"""
    _, s = _check_case(hip, oracle, tuning, PX56, U)
    assert s.uy == (25 if U == 128 else 33)


@gpu
def test_partial_last_tile(hip, oracle, tuning):
    """55 x 56: 3080 pixels = 24 units of 128 + one of 8 pixels, i.e. one partial tile per image"""
    _, s = _check_case(hip, oracle, tuning, C.ConvCase("px55", 2, 64, 55, 56, 64, 256, dst_dt=C.S32), 128)
    assert s.uy == 25 and 55 * 56 - 24 * 128 == 8


@gpu
def test_narrow_rows_rmax(hip, oracle, tuning):
    """20 x 24, f32 without the final ReLU, U = 96: a unit spans 4 to 5 rows (rmax = 5, 7 halo rows)"""
    _, s = _check_case(hip, oracle, tuning, NARROW, 96)
    assert s.th == 5


@gpu
def test_wide_rows(hip, oracle, tuning):
    """5 x 200, U = 128: units lie inside one row or cross one row end, tiles cross a row end; the halo tile is
    larger than the loader's registers (module docstring), so the synchronous rest path runs too"""
    case = C.ConvCase("px5x200", 2, 32, 5, 200, 32, 128, dst_dt=C.S32)
    _, s = _check_case(hip, oracle, tuning, case, 128)
    assert s.th == 2 and _plan(2, 5, 200, 32, 32, 128, 128, forced=False) is None


@gpu
def test_image_smaller_than_unit(hip, oracle, tuning):
    """7 x 7 (49 pixels), five images, U = 64: one short unit per image, rmax (10) beyond the image's rows"""
    _, s = _check_case(hip, oracle, tuning, C.ConvCase("px7", 5, 32, 7, 7, 32, 64, dst_dt=C.S32), 64)
    assert s.uy == 1 and s.total_units == 5


@gpu
def test_no_padding(hip, oracle, tuning):
    """pad = (0, 0): 30 x 62 in, 28 x 60 out, f32"""
    _check_case(hip, oracle, tuning, C.ConvCase("pxp0", 2, 32, 30, 62, 32, 64, pad=(0, 0), dst_dt=C.F32), 96)


@gpu
def test_per_channel_scales(hip, oracle, tuning):
    _check_case(hip, oracle, tuning, replace(NARROW, name="pxpc", dst_dt=C.S32, relu1=True, per_channel1=True,
                                             per_channel0=True), 64)


@gpu
def test_unfused(hip, oracle, tuning):
    """unfused s32: oc = 64 on the resident kernel with pixel runs; oc = 128 is not this kernel's (module docstring)"""
    _check_case(hip, oracle, tuning, C.ConvCase("pxu64", 2, 64, 20, 24, 64, 0, dst_dt=C.S32), 96)
    case = C.ConvCase("pxu128", 2, 64, 20, 24, 128, 0, dst_dt=C.S32)
    data = C.generate(case)
    want = hip.oracle_conv(oracle, case, data)
    for v in ("96", "0"):
        tuning.setenv("DFX_UNIT_PX", v)
        assert _unit_px(hip, case, data) == 0
        got, info = hip.hip_conv(case, data)
        assert not info.kernel_name.decode().startswith("conv_mfma_"), info.kernel_name
        hip.assert_bit_equal(got, want, "unfused oc=128 DFX_UNIT_PX=" + v)


U8_ROLES_SHAPE = C.ConvCase("pxu8", 2, 64, 56, 56, 64, 256, dst_dt=C.U8)


@gpu
def test_u8_without_roles(hip, oracle, tuning):
    """a 1-byte output on conv_mfma.cuh's kernel (DFX_NO_ROLES=1): not store-bound, the switch alone forces the mode"""
    _check_case(hip, oracle, tuning, U8_ROLES_SHAPE, 128, switches=(("DFX_NO_ROLES", "1"),))


@gpu
def test_roles_shape_keeps_row_units(hip, oracle, tuning):
    """a shape the role-specialised kernel takes never gets pixel runs: that kernel has no decode for them"""
    import torch
    case, data = U8_ROLES_SHAPE, C.generate(U8_ROLES_SHAPE)
    ref = _Ref(hip, oracle, case, data)
    assert _unit_px(hip, case, data) == 0
    got, info, s = _run(hip, case, data, ref, "roles default")
    tuning.setenv("DFX_UNIT_PX", "128")
    assert _unit_px(hip, case, data) == 0
    got2, info2, s2 = _run(hip, case, data, ref, "roles DFX_UNIT_PX=128")
    assert info2.kernel_name == info.kernel_name and s2 == s and s.roles == 1, (info.kernel_name, info2.kernel_name, s, s2)
    assert torch.equal(got, got2)


@gpu
@pytest.mark.parametrize("switch", ["DFX_NO_MAGIC", "DFX_NO_FAST"])
def test_requant_routes(hip, oracle, tuning, switch):
    """the fast and the exact requant route under pixel runs (mid-row starts, a partial last tile)"""
    _check_case(hip, oracle, tuning, C.ConvCase("px55r", 1, 64, 55, 56, 64, 256, dst_dt=C.S32), 128,
                switches=((switch, "1"),))


@gpu
def test_scheduling_modes(hip, oracle, tuning):
    """bs = 24, 56 x 56 s32, U = 128 (600 units): however the units reach the loaders -- all from the queue, one
    static round, all static, eager draws -- the bytes are those of the default hand-out"""
    import torch
    case = replace(PX56, name="px56b24", bs=24)
    data = C.generate(case)
    ref = _Ref(hip, oracle, case, data)
    base, _ = _check_case(hip, oracle, tuning, case, 128, ref=ref, data=data)
    for key, val in (("DFX_STATIC_ROUNDS", "0"), ("DFX_STATIC_ROUNDS", "1"), ("DFX_STATIC_ROUNDS", "99"),
                     ("DFX_NO_LAZY", "1")):
        tuning.setenv("DFX_UNIT_PX", "128")
        tuning.setenv(key, val)
        assert _unit_px(hip, case, data) == 128
        got, _, s = _run(hip, case, data, ref, "%s=%s" % (key, val))
        tuning.undo()
        assert s.total_units == 600, s
        assert torch.equal(got, base), "%s=%s changes the result" % (key, val)


@gpu
def test_forced_geometry_wins(hip, oracle, tuning):
    """DFX_FORCE_GEOM=2,56 with DFX_UNIT_PX=128: a forced geometry stays row units"""
    case, data = PX56, C.generate(PX56)
    ref = _Ref(hip, oracle, case, data)
    tuning.setenv("DFX_FORCE_GEOM", "2,56")
    tuning.setenv("DFX_UNIT_PX", "128")
    assert _unit_px(hip, case, data) == 0
    _, _, s = _run(hip, case, data, ref, "forced geometry")
    assert (s.th, s.tw, s.uy) == (2, 56, 28), s


@gpu
def test_illegal_unit_px_falls_back(hip, oracle, tuning):
    """an illegal U (no multiple of 32; 7 halo rows do not fit the ring slot check of the headline shape) never fails
    dfx_conv_create: row units"""
    case, data = replace(PX56, bs=1), C.generate(replace(PX56, bs=1))
    ref = _Ref(hip, oracle, case, data)
    for v in ("100", "-32", "4096"):
        tuning.setenv("DFX_UNIT_PX", v)
        assert _unit_px(hip, case, data) == 0, v
        _run(hip, case, data, ref, "DFX_UNIT_PX=" + v)
        tuning.undo()
