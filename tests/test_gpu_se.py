"""GPU: the squeeze-and-excitation op (dfx_se_*, deepfusion::squeeze_excite / global_avg_pool) against the numpy reference of
tests/se_ref.py, bit for bit (tests/test_se_cpu.py pins that reference against a scalar loop, refmath's average pooling and
fc_ref), and against the ops that define it on the device: dfx_pool with the window of the image, dfx_fc twice and a table
lookup.  Everything goes through the C ABI; every dst sits between guard bands with poison fill; path, slices and kernel
name are asserted from info()."""
import importlib
import os
import subprocess
from dataclasses import replace

import numpy as np
import pytest

import hipref
import se_ref as S

pytestmark = pytest.mark.gpu
dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "deep-fusion_amd", "tools")
GUARD = 1 << 16       # guard bytes on each side of dst
MAX_GRID = 2048       # workgroups of an uncapped launch
SQUEEZE_LDS = 4 * (256 * 17 + 256)
MODE_NAME = {S.SCALE: "scale", S.GATE: "gate", S.SQUEEZE: "squeeze"}
RESULT = {S.SCALE: "dst", S.GATE: "g", S.SQUEEZE: "z"}


def cus():
    import torch
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def make_op(case, data, mode=S.SCALE, force_path=-1, weights=True):
    op = dfa.SqueezeExcite((case.bs, case.ih, case.iw, case.c), case.cr, mode=mode, bia1_dt=case.bia1_dt, bia2_dt=case.bia2_dt,
                           nscales1=data["scales1"].size, nscales2=data["scales2"].size, nscales_out=data["out_scales"].size,
                           rm=case.rm, force_path=force_path)
    if weights and mode != S.SQUEEZE:
        op.set_weights(data["w1"], data["scales1"], data["w2"], data["scales2"], data["lut"], data["out_scales"], bia1=data["bia1"],
                       bia2=data["bia2"])
    return op


def guarded(nbytes, shape, offset=0):
    """-> (buf, dst): dst (poisoned with 0xCD, `offset` bytes off a 16-byte boundary) between two GUARD-byte bands of 0xA5"""
    import torch
    buf = torch.empty(GUARD + offset + nbytes + GUARD, dtype=torch.uint8, device="cuda")
    buf.fill_(hipref.GUARD_BYTE)
    mid = buf[GUARD + offset:GUARD + offset + nbytes]
    mid.fill_(hipref.POISON_BYTE)
    return buf, mid.view(shape)


def assert_guards(buf, offset, nbytes, what):
    lo, hi = buf[:GUARD + offset], buf[GUARD + offset + nbytes:]
    assert bool((lo == hipref.GUARD_BYTE).all()) and bool((hi == hipref.GUARD_BYTE).all()), what + ": a guard band was overwritten"


def submit_guarded(op, src_dev, offset=0, stream=None):
    import torch
    nbytes = int(np.prod(op.dst_shape))
    buf, dst = guarded(nbytes, op.dst_shape, offset)
    torch.cuda.synchronize()
    op.submit(src_dev, dst, stream=stream)
    torch.cuda.synchronize()
    assert_guards(buf, offset, nbytes, op.info().kernel_name.decode())
    return dst.cpu().numpy()


def want_name(case, mode, path, slices):
    if path == S.BAND:
        return "se_band<%s> c%d cr%d slices%d" % (MODE_NAME[mode], case.c, case.cr, slices)
    return "se_generic<%s> c%d cr%d" % (MODE_NAME[mode], case.c, case.cr)


def check(case, mode, path, force_path=-1, forced_slices=None, grid_cap=None, data_st=None):
    """one guarded submit of `case` in `mode`; the plan from info() and the bytes against the reference"""
    import torch
    data, st = data_st or S.generate(case)
    op = make_op(case, data, mode, force_path)
    try:
        info = op.info()
        what = "%s [%s]" % (case.ident(), info.kernel_name.decode())
        assert info.path == path, what
        slices = S.planned_slices(case, cus(), forced_slices) if path == S.BAND else 1
        assert info.slices == slices, (what, info.slices, slices)
        assert info.kernel_name.decode() == want_name(case, mode, path, slices), what
        groups = case.c // 16
        items = case.bs * slices * -(-groups // 256) if path == S.BAND else -(-case.bs * case.c // 256)
        assert info.grid == min(items, grid_cap or MAX_GRID), (what, info.grid, items)
        assert info.block == 256 and info.lds_bytes == (SQUEEZE_LDS if path == S.BAND else 0), what
        src_b, dst_b = case.bs * case.px * case.c, int(np.prod(op.dst_shape))
        assert info.algorithmic_bytes == (2 * src_b + dst_b if mode == S.SCALE else src_b + dst_b), what
        got = submit_guarded(op, torch.from_numpy(data["src"]).cuda())
        hipref.assert_bit_equal(got, st[RESULT[mode]], what)
        return info
    finally:
        op.close()


# ---- 1. the table ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", S.MODES, ids=lambda m: MODE_NAME[m])
@pytest.mark.parametrize("c", S.BAND_C + S.GENERIC_C)
def test_table(c, mode):
    """every channel count with every image size (1x1 ... 33x17); cr, bs, biases, scale sets and round mode rotate; band
    shapes run on both paths"""
    table = [k for k in S.table() if k.c == c]
    assert len(table) == len(S.IMAGES)
    for case in table:
        if case.band_class:
            check(case, mode, S.BAND)
            check(case, mode, S.BAND, force_path=S.BAND)
            check(case, mode, S.GENERIC, force_path=S.GENERIC)
        else:
            check(case, mode, S.GENERIC)
            with pytest.raises(dfa.DfxError, match="dfx error 2"):
                make_op(case, S.generate(case)[0], mode, force_path=S.BAND)


# ---- 2. the packed accumulators' flush and the s32 bound ------------------------------------------------------------------
def _flush_case(px, c):
    return S.SeCase("flush", 1, px, 1, c, 4, seed=6000 + c)


@pytest.mark.parametrize("c, pixels", [(16, S.FLUSH_PIXELS), (64, S.FLUSH_PIXELS), (4096, (256, 257, 258, 561)),
                                       (1152, (768, 771, 772, 774, 1683))], ids=lambda v: str(v))
def test_flush_of_the_packed_accumulators(tuning, c, pixels):
    """all-255 images: every channel's sum is 255 * pixels and z exactly 255.  With c = 16 / 64 a workgroup spreads a
    slice over 256 / 64 lanes per channel group; with c = 4096 a lane walks every pixel of its slice and with c = 1152
    every third one, so 258 (774) pixels in ONE slice are the first count past a flush at 257.  Then the same image
    with zeros sprinkled in, and the gate the sums lead to, against the reference."""
    import torch
    tuning.setenv("DFX_SE_SLICES", 1)
    for px in pixels:
        case = _flush_case(px, c)
        data = dict(S._draw(case, case.seed))
        for variant in ("all-255", "sprinkled"):
            src = np.full((1, px, 1, c), 255, dtype=np.uint8)
            if variant == "sprinkled":
                rng = np.random.default_rng(px + c)
                src[0, rng.integers(0, px, 3 * px // 4), 0, rng.integers(0, c, 3 * px // 4)] = 0
            data["src"] = src
            st = S.gate_stages(case, data)
            if variant == "all-255":
                assert np.all(st["sum"] == 255 * px) and np.all(st["z"] == 255)
            for mode in (S.SQUEEZE, S.GATE):
                op = make_op(case, data, mode, force_path=S.BAND)
                try:
                    assert op.info().slices == 1
                    got = submit_guarded(op, torch.from_numpy(src).cuda())
                    hipref.assert_bit_equal(got, st[RESULT[mode]], "%s %s px %d c %d" % (variant, MODE_NAME[mode], px, c))
                finally:
                    op.close()


def test_accumulator_bound():
    """one image 4096 x 2048 x 16 of 255s: ih * iw = 2^23 is the last admitted pixel count and the channel sum
    2 139 095 040 stays in s32; squeeze mode, then scale mode in place"""
    import torch
    case = S.SeCase("bound", 1, 4096, 2048, 16, 4, seed=6500)
    assert case.px == S.MAX_PX and 255 * case.px == 2139095040 < 2 ** 31
    data = dict(S._draw(replace(case, ih=1, iw=1), case.seed))
    data["src"] = np.full((1, 1, 1, 16), 255, dtype=np.uint8)        # the same z, so the same gate
    st = S.stages(replace(case, ih=1, iw=1), data)
    assert np.all(st["z"] == 255) and len(np.unique(st["g"])) > 4
    src = torch.full((1, 4096, 2048, 16), 255, dtype=torch.uint8, device="cuda")
    op = make_op(case, data, S.SQUEEZE)
    try:
        assert op.info().path == S.BAND and op.info().slices == min(2 * cus(), case.px // 64)
        got = submit_guarded(op, src)
        hipref.assert_bit_equal(got, st["z"], "squeeze at the pixel bound")
    finally:
        op.close()
    op = make_op(case, data, S.SCALE)
    try:
        op.submit(src, src)
        torch.cuda.synchronize()
        want = torch.from_numpy(st["dst"].reshape(16)).cuda()
        assert bool((src.view(-1, 16) == want).all()), "scale in place at the pixel bound"
    finally:
        op.close()


# ---- 3. slices and grid caps ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slices", S.SLICE_VALUES)
def test_every_slice_count_gives_the_same_bits(tuning, slices):
    """DFX_SE_SLICES in {1, 2, 3, 7, ih * iw, 10^6 (clamped)} on 561 pixels: uneven last slices, one-pixel slices.  The sum
    of the slices is an integer sum."""
    tuning.setenv("DFX_SE_SLICES", slices)
    for mode in S.MODES:
        info = check(S.SLICE_CASE, mode, S.BAND, forced_slices=slices)
        assert info.slices == min(slices, S.SLICE_CASE.px)


@pytest.mark.parametrize("grid", S.GRID_VALUES)
def test_capped_grids_loop(tuning, grid):
    """DFX_SE_GRID in {1, 3}: every workgroup loop of every kernel takes a second pass"""
    tuning.setenv("DFX_SE_GRID", grid)
    for case in S.GRID_CASES:
        for mode in S.MODES:
            check(case, mode, S.BAND, grid_cap=grid)
            check(case, mode, S.GENERIC, force_path=S.GENERIC, grid_cap=grid)


def test_more_work_than_one_launch_holds(tuning):
    """uncapped launches of 2048 workgroups that loop: 2100 images (excite kernel; squeeze kernel: 2100 items), 4 x 561
    one-pixel slices (squeeze kernel), and a 70 MB tensor (scale kernels: more than 2048 * 256 lanes on either path),
    whose rescale is checked on the device against the same f32 operations in torch"""
    import torch
    check(S.SeCase("many", 2100, 1, 1, 16, 4, seed=6600), S.SCALE, S.BAND)
    tuning.setenv("DFX_SE_SLICES", 561)
    info = check(replace(S.SLICE_CASE, bs=4, seed=6700), S.GATE, S.BAND, forced_slices=561)
    assert info.grid == MAX_GRID < 4 * 561
    tuning.setenv("DFX_SE_SLICES", None)
    case = S.SeCase("large", 5, 384, 384, 96, 4, seed=6800)
    assert case.bs * -(-case.px // 8) * (case.c // 16) > MAX_GRID * 256
    data = dict(S._draw(replace(case, ih=48, iw=48), case.seed))
    data["src"] = np.tile(data["src"], (1, 8, 8, 1))               # (a 48 x 48 draw, tiled: quick to make)
    g = S.gate_stages(case, data)["g"]
    src = torch.from_numpy(data["src"]).cuda()
    f = (src.to(torch.int32) * torch.from_numpy(g).cuda().to(torch.int32)[:, None, None, :]).to(torch.float32)
    want = torch.clamp(torch.round(f * float(data["out_scales"][0])), 0, 255).to(torch.uint8)      # (round: half to even)
    for path in (S.BAND, S.GENERIC):
        op = make_op(case, data, S.SCALE, force_path=path)
        try:
            nbytes = src.numel()
            buf, dst = guarded(nbytes, op.dst_shape)
            op.submit(src, dst)
            torch.cuda.synchronize()
            assert_guards(buf, 0, nbytes, "large")
            assert torch.equal(dst, want), "the %s scale kernel on a looping launch" % ("band" if path == S.BAND else "generic")
        finally:
            op.close()


# ---- 4. scale sets and biases ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["scales1", "scales2", "out_scales"])
def test_per_channel_against_single_scales(which):
    """each of the three scale sets per channel on its own: against the reference, and -- filled with one value -- against
    the single-scale result"""
    for case in (S.SeCase("sc", 2, 5, 9, 48, 12, seed=7000), S.SeCase("sc", 2, 5, 9, 17, 5, seed=7100)):
        base, st = S.generate(case)
        n = case.cr if which == "scales1" else case.c
        for fill in ("varied", "uniform"):
            data = dict(base)
            mult = 0.8 + 0.4 * ((np.arange(n) * 5) % 7) / 7.0 if fill == "varied" else np.ones(n)
            data[which] = (base[which][0] * mult).astype(np.float32)
            want = S.stages(case, data)
            if fill == "uniform":
                assert all(np.array_equal(want[k], st[k]) for k in ("h", "t", "g", "dst"))
            elif which != "scales1":
                assert not np.array_equal(want["dst"], st["dst"])
            for mode in (S.SCALE, S.GATE):
                check(case, mode, S.BAND if case.band_class else S.GENERIC, data_st=(data, want))


@pytest.mark.parametrize("b1, b2", [(S.UNDEF, S.UNDEF), (S.F32, S.S32), (S.S32, S.F32), (S.UNDEF, S.S32), (S.F32, S.UNDEF)],
                         ids=lambda v: str(v))
def test_biases_absent_f32_s32(b1, b2):
    for case in (S.SeCase("bias", 3, 7, 7, 64, 12, bia1_dt=b1, bia2_dt=b2, seed=7200),
                 S.SeCase("bias", 2, 3, 3, 40, 5, bia1_dt=b1, bia2_dt=b2, rm=1, seed=7300)):
        check(case, S.SCALE, S.BAND if case.band_class else S.GENERIC)


def test_rescale_rounding_ties():
    """out_scale = 2^-8 and 2^-7 put hundreds of the products src * gate on k + 1/2 (se_ref.tie_data counts them; no
    out_scale of the table does): nearest-even (rm 0) and floor (rm 1) in sat_u8(cvt(src * gate * out_scale)) on the
    band and the generic path, bit for bit"""
    failures = []
    for k in S.TIE_LOG2:
        for rm in (0, 1):
            case, data, st, n = S.tie_data(k, rm)
            for path in (S.BAND, S.GENERIC):
                try:
                    check(case, S.SCALE, path, force_path=path, data_st=(data, st))
                except AssertionError as e:
                    failures.append("2^-%d rm %d path %d %r: %s" % (k, rm, path, n, str(e)[:600]))
    assert not failures, "%d:\n%s" % (len(failures), "\n".join(failures))


# ---- 5.the defining properties, on the device -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [S.SeCase("def", 3, 14, 14, 64, 12, seed=7400), S.SeCase("def", 2, 33, 17, 1152, 48, per_channel=True, seed=7500),
                                  S.SeCase("def", 2, 7, 7, 72, 5, rm=1, seed=7600), S.SeCase("def", 1, 5, 9, 17, 4, bia1_dt=S.F32, seed=7700)],
                         ids=lambda c: c.ident())
def test_defining_properties(case):
    """squeeze == dfx_pool (average, window = image); gate == that pool -> dfx_fc (relu, u8) -> dfx_fc (s8) -> table;
    scale == the reference"""
    import torch
    data, st = S.generate(case)
    src = torch.from_numpy(data["src"]).cuda()
    pool = dfa.Pool(case.bs, case.c, case.ih, case.iw, 1, 1, (case.ih, case.iw), (1, 1), (0, 0), np.uint8, algo=dfa.Pool.AVG_EXCLUDE_PADDING)
    fc1 = dfa.InnerProduct((case.bs, 1, 1, case.c), case.cr, dst_dt=S.U8, bia_dt=case.bia1_dt, relu=True, rm=case.rm,
                           nscales=data["scales1"].size)
    fc2 = dfa.InnerProduct((case.bs, 1, 1, case.cr), case.c, dst_dt=S.S8, bia_dt=case.bia2_dt, relu=False, rm=case.rm,
                           nscales=data["scales2"].size)
    ops = [pool, fc1, fc2]
    try:
        fc1.set_weights(data["w1"].reshape(case.cr, case.c, 1, 1), data["scales1"], bia=data["bia1"])
        fc2.set_weights(data["w2"].reshape(case.c, case.cr, 1, 1), data["scales2"], bia=data["bia2"])
        z = torch.empty((case.bs, 1, 1, case.c), dtype=torch.uint8, device="cuda")
        h = torch.empty((case.bs, case.cr), dtype=torch.uint8, device="cuda")
        t = torch.empty((case.bs, case.c), dtype=torch.int8, device="cuda")
        pool.submit(src, z)
        fc1.submit(z, h)
        fc2.submit(h, t)
        torch.cuda.synchronize()
        g = torch.from_numpy(data["lut"]).cuda()[t.to(torch.int64) + 128]
        for mode, want in ((S.SQUEEZE, z.view(case.bs, case.c)), (S.GATE, g)):
            op = make_op(case, data, mode)
            ops.append(op)
            got = submit_guarded(op, src)
            hipref.assert_bit_equal(got, want.cpu().numpy(), "%s %s against the ops that define it" % (case.ident(), MODE_NAME[mode]))
    finally:
        for op in ops:
            op.close()
    check(case, S.SCALE, S.BAND if case.band_class else S.GENERIC)


# ---- 6. pointers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [S.SeCase("ptr", 2, 14, 14, 48, 12, seed=7800), S.SeCase("ptr", 2, 5, 9, 40, 5, seed=7900)], ids=lambda c: c.ident())
def test_in_place_overlap_null_and_misaligned_pointers(case):
    import torch
    data, st = S.generate(case)
    n = data["src"].size
    op = make_op(case, data, S.SCALE)
    sq = make_op(case, data, S.SQUEEZE)
    try:
        path = op.info().path
        assert path == (S.BAND if case.band_class else S.GENERIC)
        # in place: src inside guard bands, overwritten with what the out-of-place submit gives
        buf, io = guarded(n, op.dst_shape)
        io.copy_(torch.from_numpy(data["src"]).cuda())
        torch.cuda.synchronize()
        op.submit(io, io)
        torch.cuda.synchronize()
        assert_guards(buf, 0, n, "in place")
        hipref.assert_bit_equal(io.cpu().numpy(), st["dst"], "in place")
        # a dst that overlaps src without being src is refused, nothing is launched: poison and guards stay
        buf, flat = guarded(2 * n, (2 * n,))
        flat[:n].copy_(torch.from_numpy(data["src"]).cuda().view(-1))
        torch.cuda.synchronize()
        before = buf.clone()
        for off in (16, n // 2 // 16 * 16, n - 16, 1, n - 1):
            with pytest.raises(dfa.DfxError, match="dfx error 1.*overlaps"):
                op.submit(flat[:n].view(op.dst_shape), flat[off:off + n].view(op.dst_shape))
            with pytest.raises(dfa.DfxError, match="dfx error 1.*overlaps"):
                op.submit(flat[off:off + n].view(op.dst_shape), flat[:n].view(op.dst_shape))
        for off in (0, 16, n - 1):          # the {bs, c} result of squeeze mode must lie apart from src altogether
            with pytest.raises(dfa.DfxError, match="dfx error 1.*overlaps"):
                sq.submit(flat[:n].view(op.dst_shape), flat[off:off + case.bs * case.c].view(sq.dst_shape))
        torch.cuda.synchronize()
        assert torch.equal(buf, before), "a refused submit wrote something"
        # null pointers
        lib = capi.lib()
        for s, d in ((None, io.data_ptr()), (io.data_ptr(), None), (None, None)):
            assert lib.dfx_se_submit(op._h, s, d, None) == 1 and "null" in lib.dfx_last_error().decode()
        # src and / or dst one byte off a 16-byte boundary: the generic kernels for that submit, the same bytes
        for so, do in ((1, 0), (0, 1), (1, 1)):
            sbuf = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
            s = sbuf[so:so + n].view(op.dst_shape)
            s.copy_(torch.from_numpy(data["src"]).cuda())
            assert s.data_ptr() % 16 == so
            got = submit_guarded(op, s, offset=do)
            hipref.assert_bit_equal(got, st["dst"], "src + %d, dst + %d" % (so, do))
            got = submit_guarded(sq, s, offset=do)
            hipref.assert_bit_equal(got, st["z"], "squeeze: src + %d, dst + %d" % (so, do))
            assert op.info().path == path and sq.info().path == path
    finally:
        op.close()
        sq.close()


# ---- 7. streams, weights, state ---------------------------------------------------------------------------------------------
def test_three_submits_on_two_streams():
    """one handle, two streams, three inputs: the handle's slab and gate are handed from submit to submit in order"""
    import torch
    case = S.SeCase("streams", 3, 33, 17, 96, 12, seed=8000)
    sets = [(S._draw(case, 8000 + k), None) for k in range(3)]
    data0 = sets[0][0]
    wants = [S.stages(case, dict(data0, src=d["src"]))["dst"] for d, _ in sets]
    assert not np.array_equal(wants[0], wants[1]) and not np.array_equal(wants[1], wants[2])
    op = make_op(case, data0, S.SCALE)
    try:
        srcs = [torch.from_numpy(d["src"]).cuda() for d, _ in sets]
        n = srcs[0].numel()
        outs = [guarded(n, op.dst_shape) for _ in range(3)]
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        for k in range(3):
            op.submit(srcs[k], outs[k][1], stream=streams[k % 2])
        torch.cuda.synchronize()
        for k in range(3):
            assert_guards(outs[k][0], 0, n, "submit %d" % k)
            hipref.assert_bit_equal(outs[k][1].cpu().numpy(), wants[k], "submit %d on stream %d" % (k, k % 2))
    finally:
        op.close()


def test_set_weights_again_and_state():
    import torch
    case = S.SeCase("again", 2, 7, 7, 32, 8, seed=8100)
    data, st = S.generate(case)
    src = torch.from_numpy(data["src"]).cuda()
    other = dict(data, lut=S.hard_sigmoid_table())
    want_other = S.stages(case, other)
    assert not np.array_equal(want_other["g"], st["g"])
    for mode in (S.SCALE, S.GATE):
        op = make_op(case, data, mode, weights=False)
        try:
            buf, dst = guarded(int(np.prod(op.dst_shape)), op.dst_shape)
            before = buf.clone()
            with pytest.raises(dfa.DfxError, match="dfx error 5"):
                op.submit(src, dst)
            with pytest.raises(dfa.DfxError, match="dfx error 5"):
                op.submit_host(data["src"])
            torch.cuda.synchronize()
            assert torch.equal(buf, before)
            for d, want in ((data, st), (other, want_other), (data, st)):
                op.set_weights(d["w1"], d["scales1"], d["w2"], d["scales2"], d["lut"], d["out_scales"], bia1=d["bia1"], bia2=d["bia2"])
                hipref.assert_bit_equal(submit_guarded(op, src), want[RESULT[mode]], MODE_NAME[mode])
                hipref.assert_bit_equal(op.submit_host(data["src"]), want[RESULT[mode]], MODE_NAME[mode] + " submit_host")
        finally:
            op.close()
    op = make_op(case, data, S.SQUEEZE)          # takes no weights: never DFX_ERR_STATE
    try:
        hipref.assert_bit_equal(submit_guarded(op, src), st["z"], "squeeze")
        hipref.assert_bit_equal(op.submit_host(data["src"]), st["z"], "squeeze submit_host")
    finally:
        op.close()


@pytest.mark.parametrize("shards", [None, "2", "3", "all"])
def test_se_check_tool(shards):
    """the drop-in C++ layer end to end: squeeze_excite() and global_avg_pool() against the tool's scalar loop, unsharded and
    with the batch split over DEEPFUSION_DEVICES shards (the op is per image: shards are independent)"""
    exe = os.path.join(TOOLS, "se_check")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    env = dict(os.environ)
    env.pop("DEEPFUSION_DEVICES", None)
    if shards:
        env["DEEPFUSION_DEVICES"] = shards
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, env=env)
    out = p.stdout.decode()
    assert p.returncode == 0 and "se_check: every layer identical to the scalar loop" in out, out
