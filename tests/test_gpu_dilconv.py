"""GPU: the dilated conv op (dfx_dilconv_*, deepfusion::dilated_conv) against the numpy gather reference of
tests/dilconv_ref.py, bit for bit (tests/test_dilconv_cpu.py pins that reference against the C oracle's dense conv on
the zero-stuffed weights and against the grouped conv's reference).  Everything goes through the C ABI; every output is
written between guard bands; every case runs under both requant routes (DFX_NO_FAST forces the exact one) and the route
is asserted from requant()."""
import ctypes
import importlib
import os
import subprocess
from dataclasses import replace

import numpy as np
import pytest

import cases as C
import dilconv_ref as R
import hipref

pytestmark = pytest.mark.gpu
dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "deep-fusion_amd", "tools")
BAND = 1 << 16       # guard bytes on each side of dst
EXACT, FAST = 0, 1
AUTO = -1


def auto_path(case):
    """the AUTO RULE of include/dfx.h (DFX_DILCONV_MFMA): auto takes the MFMA kernel everywhere in its class (it beats the
    generic path on every measured point, profiles/dilconv/)"""
    return R.MFMA


def make_op(case, data, force_path=AUTO):
    op = dfa.DilatedConv((case.bs, case.ih, case.iw, case.c), case.oc, case.k, dilation=case.dil, stride=case.stride,
                         pad=case.pad, out_hw=(case.oh, case.ow), dst_dt=case.dst_dt, bia_dt=case.bia_dt, relu=case.relu,
                         rm=case.rm, nscales=data["scales"].size, force_path=force_path)
    op.set_weights(data["w"], data["scales"], bia=data["bia"])
    return op


def guarded_dst(op, case):
    """-> (buf, dst): dst (poisoned with 0xCD) sits between two BAND-byte bands of 0xA5 inside one allocation"""
    import torch
    nbytes = int(np.prod(op.dst_shape)) * np.dtype(C.NP_OF[case.dst_dt]).itemsize
    buf = torch.empty(BAND + nbytes + BAND, dtype=torch.uint8, device="cuda")
    buf.fill_(hipref.GUARD_BYTE)
    mid = buf[BAND:BAND + nbytes]
    mid.fill_(hipref.POISON_BYTE)
    return buf, mid.view(hipref.torch_dtype(case.dst_dt)).view(op.dst_shape)


def run(case, data, force_path=AUTO, stream=None, on_device=False):
    """-> (dst, info, route): one submit into a guarded dst; the guard bands must survive"""
    import torch
    op = make_op(case, data, force_path)
    try:
        info, route = op.info(), op.requant()
        src = torch.from_numpy(data["src"]).cuda()
        buf, dst = guarded_dst(op, case)
        torch.cuda.synchronize()
        op.submit(src, dst, stream=stream)
        torch.cuda.synchronize()
        hipref.assert_guards(buf, BAND, "%s %s" % (info.kernel_name.decode(), case.ident()))
        return (dst if on_device else dst.cpu().numpy()), info, route
    finally:
        op.close()


_REF = {}


def reference(case, data=None):
    """computed once per case, shared, never written to"""
    if case not in _REF:
        data = data or R.generate(case)
        ref = R.dilconv_ref(case, data)
        ref.setflags(write=False)
        _REF[case] = (data, ref)
    return _REF[case]


def want_route(case, switch, path):
    """what set_weights must prove for reference-range and "wide" data: fast on the MFMA kernel with nearest rounding
    (everything is finite and far below 2^30), exact otherwise"""
    return FAST if (path == R.MFMA and case.rm == 0 and not switch) else EXACT


def want_name(case, path, route, slab=None, strips=R.DEFAULT_STRIPS):
    dt = C.NAME_OF[case.dst_dt]
    if path == R.MFMA:
        s, nbuf, _ = R.lds_plan(case.c, case.oc, slab)
        return "dilconv_mfma<3x3,d%dx%d,ic%d,oc%d,%s,slab%dx%d,r%d> %s" % (
            case.dil + (case.c, case.oc, dt, s, nbuf, strips, "fast" if route == FAST else "exact"))
    return "dilconv_generic<%dx%d,s%dx%d,d%dx%d,ic%d,oc%d,%s> exact" % (case.k + case.stride + case.dil + (case.c, case.oc, dt))


def check_table(table, force, switch, tuning, slab=None, strips=R.DEFAULT_STRIPS):
    if switch:
        tuning.setenv(switch, "1")
    names = set()
    for case in table:
        data, ref = reference(case)
        got, info, route = run(case, data, force_path=force)
        name = info.kernel_name.decode()
        what = "%s [%s] %s" % (case.ident(), name, switch)
        path = force if force != AUTO else (auto_path(case) if case.mfma_class else R.GENERIC)
        assert info.path == path, what
        assert route == want_route(case, switch, path), what
        assert name == want_name(case, path, route, slab, strips), what
        hipref.assert_bit_equal(got, ref, what)
        names.add(name.split(" ")[0])
    return names


@pytest.mark.parametrize("geom", [g[0] for g in R.MFMA_GEOMS])
@pytest.mark.parametrize("force", [R.MFMA, AUTO], ids=["forced", "auto"])
@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_mfma_shapes(tuning, switch, force, geom):
    """one geometry of the class table under every option row (all four dst types, with and without bias and ReLU, both
    round modes), forced onto the MFMA kernel and on auto"""
    table = R.mfma_table(geom)
    assert len(table) == len(R.OPTIONS)
    names = check_table(table, force, switch, tuning)
    assert {n.split(",")[4] for n in names} == {"u8", "s8", "s32", "f32"}


@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_generic_path(tuning, switch):
    """5x5 window at stride 2 and d 3, the class's window at stride 2, on ic 3 / 20 / 48 and oc 5 / 48, a row window, an
    even window with a given output size: info.path asserted"""
    names = check_table(R.generic_table(), AUTO, switch, tuning)
    assert all(n.startswith("dilconv_generic<") for n in names)


@pytest.mark.parametrize("geom", [g[0] for g in R.MFMA_GEOMS])
def test_permutation_case(geom):
    """distinct weights per (i, ky, kx) of a channel and per channel at every tap, activations over the whole range, the
    accumulators themselves (s32, scale 1): a swapped tap, channel, K-step, slab or block in the packer or the kernel
    changes the bytes"""
    case, data = R.permutation_case(geom)
    data, ref = reference(case, data)
    for path in (R.MFMA, R.GENERIC):
        got, info, route = run(case, data, force_path=path)
        assert info.path == path
        hipref.assert_bit_equal(got, ref, "permutation %s [%s]" % (case.ident(), info.kernel_name.decode()))


@pytest.mark.parametrize("geom", ["slabs", "slabs-oc160"])
@pytest.mark.parametrize("slab", [1, 2, 8])
@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_k_slabs(tuning, switch, slab, geom):
    """ic 96 = three K-steps under DFX_DILCONV_SLAB = 1 (a slab per K-step), 2 (an uneven last slab) and 8 (clamped to the
    three that exist: all in one); with one output block two slab buffers fit, with a chunk of four at slab 2 only one:
    every option row and the permutation case on each plan"""
    tuning.setenv("DFX_DILCONV_SLAB", slab)
    s, nbuf, lds = R.lds_plan(96, R.mfma_case(geom).oc, slab)
    assert (s, nbuf) == {("slabs", 1): (1, 2), ("slabs", 2): (2, 2), ("slabs", 8): (3, 1), ("slabs-oc160", 1): (1, 2),
                         ("slabs-oc160", 2): (2, 1), ("slabs-oc160", 8): (3, 1)}[(geom, slab)]
    check_table(R.mfma_table(geom), R.MFMA, switch, tuning, slab=slab)
    case, data = R.permutation_case(geom)
    data, ref = reference(case, data)
    got, info, route = run(case, data, force_path=R.MFMA)
    assert info.lds_bytes == lds and ("slab%dx%d" % (s, nbuf)) in info.kernel_name.decode(), info.kernel_name
    hipref.assert_bit_equal(got, ref, "permutation %s [%s]" % (case.ident(), info.kernel_name.decode()))


@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_more_work_items_than_workgroups(tuning, switch):
    """ten strips on eight waves and oc 160 (chunks of 4 + 1 blocks): uncapped, a workgroup per (chunk, slot) unit, the
    second slot's workgroup has TWO waves with a live strip -- the other six run the clamped strip through every
    barrier and store nothing; DFX_DILCONV_GRID = 1 makes one workgroup loop over all units (and, with one slot, over
    two passes of strips), 3 leaves one workgroup two units."""
    strips = R.DEFAULT_STRIPS
    table = R.mfma_table("strips")
    pcase, pdata = R.permutation_case("strips")
    pdata, pref = reference(pcase, pdata)
    op = make_op(pcase, pdata, R.MFMA)
    try:
        assert op.info().grid == 2 * -(-10 // (R.WAVES * strips))       # chunks x slots
    finally:
        op.close()
    for grid in (None, 1, 3):
        if grid:
            tuning.setenv("DFX_DILCONV_GRID", grid)
        check_table(table, R.MFMA, switch, tuning, strips=strips)
        got, info, route = run(pcase, pdata, force_path=R.MFMA)
        assert info.path == R.MFMA and (grid is None or info.grid == min(grid, 2 * -(-10 // (R.WAVES * strips)))), info.grid
        hipref.assert_bit_equal(got, pref, "%s grid %s [%s]" % (pcase.ident(), grid, info.kernel_name.decode()))


def _twin_cases():
    """geometries of the class table whose stuffed window the other ops accept, the option rows rotating"""
    return [R.mfma_case(name, j) for j, name in enumerate(("base", "rows-d2", "far-d18", "aniso31-p10", "aniso31-p00", "aniso25-p10",
                                                            "aniso25-p00", "slabs", "slabs-oc160", "chunks", "strips"))]


def _generic_twins():
    return [c for c in R.generic_table() if c.name == "gen"][::3]


@pytest.mark.parametrize("force", [R.MFMA, R.GENERIC])
@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_equal_to_group_conv_on_the_stuffed_weights_on_the_device(tuning, switch, force):
    """defining property 1: DilatedConv == GroupConv(groups = 1) with the zero-stuffed window, same stride, padding and
    output size, compared on the device (the generic path also on shapes outside the MFMA class)"""
    import torch
    if switch:
        tuning.setenv(switch, "1")
    for case in _twin_cases() + (_generic_twins() if force == R.GENERIC else []):
        assert case.stuffed_expressible
        data = R.generate(case)
        got, info, route = run(case, data, force_path=force if case.mfma_class else AUTO, on_device=True)
        assert info.path == force
        gc = dfa.GroupConv(data["src"].shape, case.oc, 1, case.ext, stride=case.stride, pad=case.pad, out_hw=(case.oh, case.ow),
                           dst_dt=case.dst_dt, bia_dt=case.bia_dt, relu=case.relu, rm=case.rm, nscales=data["scales"].size)
        try:
            gc.set_weights(R.stuff_weights(data["w"], case.dil), data["scales"], bia=data["bia"])
            src = torch.from_numpy(data["src"]).cuda()
            want = torch.empty(gc.dst_shape, dtype=hipref.torch_dtype(case.dst_dt), device="cuda")
            gc.submit(src, want)
            torch.cuda.synchronize()
            gname = gc.info().kernel_name.decode()
        finally:
            gc.close()
        assert tuple(got.shape) == tuple(want.shape)
        assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)), "%s: %s differs from %s" % (
            case.ident(), info.kernel_name.decode(), gname)


@pytest.mark.parametrize("force", [R.MFMA, R.GENERIC])
@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_equal_to_conv_on_the_stuffed_weights_on_the_device(tuning, switch, force):
    """defining property 2: DilatedConv == the unfused Conv with the zero-stuffed window, where the dense conv can
    express the layer, both run on the GPU"""
    import torch
    if switch:
        tuning.setenv(switch, "1")
    n = 0
    for case in _twin_cases():
        if not case.dense_expressible:
            continue
        data = R.generate(case)
        got, info, route = run(case, data, force_path=force, on_device=True)
        assert info.path == force
        ddata = R.dense_data(case, data)
        conv = hipref.make_conv(R.dense_case(case), ddata)
        try:
            src = torch.from_numpy(ddata["src"]).cuda()
            want = torch.empty(conv.dst_shape, dtype=hipref.torch_dtype(case.dst_dt), device="cuda")
            conv.submit(src, want)
            torch.cuda.synchronize()
            cname = conv.info().kernel_name.decode()
        finally:
            conv.close()
        assert tuple(got.shape) == tuple(want.shape)
        assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)), "%s: %s differs from %s" % (
            case.ident(), info.kernel_name.decode(), cname)
        n += 1
    assert n >= 8


@pytest.mark.parametrize("force", [R.MFMA, R.GENERIC])
@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_without_dilation_equal_to_group_conv_on_the_device(tuning, switch, force):
    """defining property 3: at dh = dw = 1 DilatedConv == GroupConv(groups = 1) on the same tensors, on the device"""
    import torch
    if switch:
        tuning.setenv(switch, "1")
    for j in range(len(R.OPTIONS)):
        case = R.mfma_case("rows-d1", j)
        data = R.generate(case)
        got, info, route = run(case, data, force_path=force, on_device=True)
        assert info.path == force
        gc = dfa.GroupConv(data["src"].shape, case.oc, 1, case.k, stride=case.stride, pad=case.pad, out_hw=(case.oh, case.ow),
                           dst_dt=case.dst_dt, bia_dt=case.bia_dt, relu=case.relu, rm=case.rm, nscales=data["scales"].size)
        try:
            gc.set_weights(data["w"], data["scales"], bia=data["bia"])
            want = torch.empty(gc.dst_shape, dtype=hipref.torch_dtype(case.dst_dt), device="cuda")
            gc.submit(torch.from_numpy(data["src"]).cuda(), want)
            torch.cuda.synchronize()
            gname = gc.info().kernel_name.decode()
        finally:
            gc.close()
        assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)), "%s: %s differs from %s" % (
            case.ident(), info.kernel_name.decode(), gname)


@pytest.mark.parametrize("geom", ["rows-d2", "aniso25-p10", "slabs-oc160", "strips"])
def test_forced_paths_agree(geom):
    import torch
    case = R.mfma_case(geom, 1, rm=0)        # s8, s8 bias, per-channel scales, nearest
    data, ref = reference(case)
    outs = []
    for path in (R.MFMA, R.GENERIC):
        got, info, route = run(case, data, force_path=path, on_device=True)
        assert info.path == path and (route == FAST) == (path == R.MFMA)
        hipref.assert_bit_equal(got.cpu().numpy(), ref, "forced path %d" % path)
        outs.append(got)
    assert torch.equal(outs[0], outs[1])


def test_nan_and_inf_scales_take_the_exact_route():
    """a NaN or an infinite scale must fail the fast route's proof; the bytes are the x86 ones: u8 255 / s8 -128"""
    for dst_dt, bad in ((C.U8, 255), (C.S8, -128)):
        case = R.DlCase("nan", 2, 64, 6, 5, 32, dil=(2, 2), pad=(2, 2), dst_dt=dst_dt, bia_dt=C.UNDEF, relu=False, per_channel=True,
                        seed=47100)
        for poison in (np.nan, np.inf, -np.inf):
            data = R.generate(case)
            data["scales"][19] = poison
            data["src"][...] = np.maximum(data["src"], 1)
            data["w"][19] = np.abs(data["w"][19]) + 1
            ref = R.dilconv_ref(case, data)
            got, info, route = run(case, data, force_path=R.MFMA)
            assert info.path == R.MFMA and route == EXACT and info.kernel_name.decode().endswith("exact"), (poison, info.kernel_name)
            hipref.assert_bit_equal(got, ref, "%s scale %r" % (case.ident(), poison))
            if not (poison == -np.inf and dst_dt == C.U8):       # (-inf through the u8 ReLU is 0)
                assert (got[..., 19] == bad).all(), (poison, dst_dt)


def test_nan_and_inf_bias_take_the_exact_route():
    """an f32 bias that is NaN or infinite must fail the fast route's proof on its own clause (the scale is ordinary);
    the exact route then gives the x86 results"""
    for dst_dt, bad in ((C.U8, 255), (C.S8, -128)):
        case = R.DlCase("nanbias", 2, 32, 6, 5, 32, dil=(2, 2), pad=(2, 2), dst_dt=dst_dt, bia_dt=C.F32, relu=False, per_channel=True,
                        seed=47150)
        for poison in (np.nan, np.inf, -np.inf):
            data = R.generate(case)
            data["bia"] = data["bia"].copy()
            data["bia"][21] = poison
            ref = R.dilconv_ref(case, data)
            got, info, route = run(case, data, force_path=R.MFMA)
            assert info.path == R.MFMA and route == EXACT and info.kernel_name.decode().endswith("exact"), (poison, info.kernel_name)
            hipref.assert_bit_equal(got, ref, "%s bias %r" % (case.ident(), poison))
            assert (got[..., 21] == (0 if (poison == -np.inf and dst_dt == C.U8) else bad)).all(), (poison, dst_dt)
            data["bia"][21] = 1.0       # the same numbers with that one bias finite are proven fast: the clause alone decided
            op = make_op(case, data, R.MFMA)
            try:
                assert op.requant() == FAST
            finally:
                op.close()


@pytest.mark.parametrize("edge", R.EDGES, ids=lambda e: e.name)
def test_fast_route_proof_edges(tuning, edge):
    """(255 * max(P, N) + |bias|) * |scale| <= 2^30 at the last value it admits and the first it rejects, with the bound
    attained by the data at one output pixel: the route, the bytes (every dst type), and the attained accumulator"""
    for dst_dt in (C.S32, C.U8, C.S8, C.F32):
        case, data = R.edge_case(edge, dst_dt)
        ref = R.dilconv_ref(case, data)
        got, info, route = run(case, data, force_path=R.MFMA)
        assert info.path == R.MFMA and route == (FAST if edge.fast else EXACT), (edge.name, dst_dt, info.kernel_name)
        hipref.assert_bit_equal(got, ref, "%s %s" % (edge.name, info.kernel_name.decode()))
    # the bound is attained: the accumulator itself, in numpy and (s32 dst, scale 1, no bias) on the device
    case, data = R.edge_case(edge, C.S32)
    acc, bound, P, N = R.edge_attained(edge, case, data)
    assert acc == bound
    neutral = dict(data, bia=None, scales=np.ones(1, dtype=np.float32))
    got, info, route = run(replace(case, bia_dt=C.UNDEF, per_channel=False), neutral, force_path=R.MFMA)
    assert int(got[0 if edge.which == "max" else 1, R.EDGE_PIXEL[0], R.EDGE_PIXEL[1], R.EDGE_CHANNEL]) == bound
    # round-down and DFX_NO_FAST reject whatever the numbers are
    case, data = R.edge_case(R.EDGES[0], C.U8)
    got, info, route = run(replace(case, rm=1), data, force_path=R.MFMA)
    assert route == EXACT
    tuning.setenv("DFX_NO_FAST", "1")
    got, info, route = run(case, data, force_path=R.MFMA)
    assert route == EXACT
    hipref.assert_bit_equal(got, R.dilconv_ref(case, data), "forced exact")


def test_info_reports_the_launch_and_the_unstuffed_counts():
    case = R.DlCase("info", 2, 64, 5, 70, 160, dil=(6, 6), pad=(6, 6), **R.OPTIONS[0])
    op = make_op(case, R.generate(case), R.MFMA)
    try:
        i = op.info()
        assert (case.oh, case.ow) == (5, 70)
        assert i.path == R.MFMA and i.block == 512 and i.device >= 0
        # 700 pixels -> 22 strips -> 3 slots of 8 waves; 5 output blocks -> 2 chunks; both K-steps of 4 blocks in one slab
        assert i.grid == 3 * 2, i.grid
        assert i.lds_bytes == 2 * 4 * 9 * 1024 + 3 * 128 * 4 + 8 * 32 * 144 == R.lds_plan(64, 160)[2], i.lds_bytes
        assert i.algorithmic_ops == 2 * 2 * 5 * 70 * 160 * 64 * 9                               # nine taps, not 13 x 13
        assert i.algorithmic_bytes == 2 * 5 * 70 * 64 + 160 * 64 * 9 + 2 * 5 * 70 * 160         # weights un-stuffed
        assert i.kernel_name.decode() == "dilconv_mfma<3x3,d6x6,ic64,oc160,u8,slab2x1,r1> fast"
    finally:
        op.close()
    case3 = R.DlCase("info3", 2, 3, 15, 14, 7, k=(5, 5), stride=(2, 2), dil=(3, 3), pad=(6, 6), dst_dt=C.S32, bia_dt=C.S32, relu=False)
    op = make_op(case3, R.generate(case3))
    try:
        i = op.info()
        assert (case3.oh, case3.ow) == (8, 7)
        assert i.path == R.GENERIC and i.block == 256 and i.lds_bytes == 0
        assert i.kernel_name.decode() == "dilconv_generic<5x5,s2x2,d3x3,ic3,oc7,s32> exact"
        assert i.algorithmic_ops == 2 * 2 * 8 * 7 * 7 * 3 * 25
        assert i.algorithmic_bytes == 2 * 15 * 14 * 3 + 7 * 3 * 25 + 2 * 8 * 7 * 7 * 4
    finally:
        op.close()


def test_the_mfma_class_has_no_ic_limit():
    """an ASPP branch of a ResNet backbone -- 33x33, 2048 -> 256, d 18 -- is created on the MFMA path, with the LDS plan
    of a 320-channel one; so is the largest ic the descriptor admits (9 * 7200 <= 65025).  From query alone: the layer
    is not run"""
    plans = {}
    for ic in (320, 2048, 7200):
        op = dfa.DilatedConv((1, 33, 33, ic), 256, (3, 3), dilation=(18, 18), pad=(18, 18), force_path=R.MFMA)
        try:
            i = op.info()
            assert i.path == R.MFMA and i.kernel_name.decode().startswith("dilconv_mfma<3x3,d18x18,ic%d,oc256,u8," % ic), i.kernel_name
            assert i.lds_bytes <= R.LDS_LIMIT and i.algorithmic_ops == 2 * 33 * 33 * 256 * ic * 9
            plans[ic] = (i.lds_bytes, i.grid, i.block)
        finally:
            op.close()
    assert plans[320] == plans[2048] == plans[7200] and plans[2048][0] == R.lds_plan(2048, 256)[2]
    # ... and auto takes it there
    op = dfa.DilatedConv((1, 33, 33, 2048), 256, (3, 3), dilation=(18, 18), pad=(18, 18))
    try:
        assert op.info().path == auto_path(None)
    finally:
        op.close()


def test_set_weights_again_takes_effect():
    import torch
    case = R.DlCase("reweigh", 2, 64, 7, 9, 64, dil=(2, 3), pad=(2, 3), seed=47400, **R.OPTIONS[0])
    data = R.generate(case)
    data2 = dict(R.generate(replace(case, seed=77, wide=True)), src=data["src"])
    ref1, ref2 = R.dilconv_ref(case, data), R.dilconv_ref(case, data2)
    assert not np.array_equal(ref1, ref2)
    op = make_op(case, data, R.MFMA)
    try:
        src = torch.from_numpy(data["src"]).cuda()
        dst = torch.full(op.dst_shape, hipref.POISON_BYTE, dtype=torch.uint8, device="cuda")
        op.submit(src, dst)
        torch.cuda.synchronize()
        hipref.assert_dev_bit_equal(dst, ref1, "first weights")
        op.set_weights(data2["w"], data2["scales"], bia=data2["bia"])
        op.submit(src, dst)
        torch.cuda.synchronize()
        hipref.assert_dev_bit_equal(dst, ref2, "second weights")
        # the route follows the numbers of the LAST set_weights
        assert op.requant() == FAST
        op.set_weights(data2["w"], np.array([np.inf], dtype=np.float32), bia=data2["bia"])
        assert op.requant() == EXACT and op.info().kernel_name.decode().endswith("exact")
        op.set_weights(data["w"], data["scales"], bia=data["bia"])
        assert op.requant() == FAST
        op.submit(src, dst)
        torch.cuda.synchronize()
        hipref.assert_dev_bit_equal(dst, ref1, "first weights again")
    finally:
        op.close()


@pytest.mark.parametrize("path", [R.MFMA, R.GENERIC])
def test_one_handle_on_three_streams(path):
    """different inputs per stream, 20 submits each, interleaved: every launch has its own copy of the arguments"""
    import torch
    case = R.DlCase("3streams", 2, 64, 10, 13, 64, dil=(2, 2), pad=(2, 2), dst_dt=C.U8, bia_dt=C.S32, per_channel=True, seed=47500)
    data = R.generate(case)
    streams = [torch.cuda.Stream() for _ in range(3)]
    devs, refs = [], []
    for k in range(3):
        dk = dict(data, src=R.generate(replace(case, seed=300 + k))["src"])
        devs.append(torch.from_numpy(dk["src"]).cuda())
        refs.append(R.dilconv_ref(case, dk))
    assert not np.array_equal(refs[0], refs[1]) and not np.array_equal(refs[1], refs[2])
    op = make_op(case, data, force_path=path)
    try:
        outs = [[torch.full(op.dst_shape, hipref.POISON_BYTE, dtype=torch.uint8, device="cuda") for _ in range(20)] for _ in range(3)]
        torch.cuda.synchronize()
        for it in range(20):
            for k, st in enumerate(streams):
                op.submit(devs[k], outs[k][it], stream=st)
        torch.cuda.synchronize()
        for k in range(3):
            ref_dev = torch.from_numpy(refs[k]).cuda()
            for it in range(20):
                hipref.assert_dev_bit_equal(outs[k][it], refs[k], "path %d stream %d launch %d" % (path, k, it), ref_dev=ref_dev)
    finally:
        op.close()


def test_null_and_misaligned_pointers_are_refused_and_nothing_is_launched():
    import torch
    L = capi.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    # MFMA path: src and dst 16-byte aligned
    case = R.DlCase("refuse", 1, 32, 3, 4, 32, dil=(2, 2), pad=(2, 2), bia_dt=C.UNDEF)
    op = make_op(case, R.generate(case), R.MFMA)
    try:
        n = 3 * 4 * 32
        a = torch.zeros(12 * 32 + 32, dtype=torch.uint8, device="cuda")
        dst = torch.full((n + 32,), 0x77, dtype=torch.uint8, device="cuda")
        assert L.dfx_dilconv_submit(op._h, None, ctypes.c_void_p(dst.data_ptr()), st) == 1       # null src
        assert L.dfx_dilconv_submit(op._h, ctypes.c_void_p(a.data_ptr()), None, st) == 1         # null dst
        assert L.dfx_dilconv_submit(None, ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(dst.data_ptr()), st) == 1
        for off_s, off_d in ((8, 0), (0, 8), (1, 0), (0, 4), (4, 4)):
            rc = L.dfx_dilconv_submit(op._h, ctypes.c_void_p(a.data_ptr() + off_s), ctypes.c_void_p(dst.data_ptr() + off_d), st)
            assert rc == 1 and b"16-byte aligned" in L.dfx_last_error(), (off_s, off_d, rc)
        with pytest.raises(dfa.DfxError):
            op.submit(a, dst.data_ptr() + 8)
        torch.cuda.synchronize()
        assert bool((dst == 0x77).all()), "a refused submit wrote to dst"
        op.submit(a.data_ptr() + 16, dst.data_ptr() + 16)
        torch.cuda.synchronize()
        assert bool((dst[:16] == 0x77).all()) and bool((dst[16 + n:] == 0x77).all()) and not bool((dst[16:16 + n] == 0x77).all())
    finally:
        op.close()
    # generic path: dst aligned to the element
    case = R.DlCase("refuse-gen", 1, 3, 3, 4, 5, dil=(2, 2), pad=(2, 2), dst_dt=C.S32, bia_dt=C.UNDEF, relu=False)
    op = make_op(case, R.generate(case))
    try:
        assert op.info().path == R.GENERIC
        n = 3 * 4 * 5 * 4
        a = torch.zeros(12 * 3 + 16, dtype=torch.uint8, device="cuda")
        dst = torch.full((n + 16,), 0x77, dtype=torch.uint8, device="cuda")
        for off_d in (1, 2, 3):
            rc = L.dfx_dilconv_submit(op._h, ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(dst.data_ptr() + off_d), st)
            assert rc == 1 and b"aligned to its element" in L.dfx_last_error(), (off_d, rc)
        torch.cuda.synchronize()
        assert bool((dst == 0x77).all()), "a refused submit wrote to dst"
        op.submit(a.data_ptr() + 5, dst.data_ptr() + 4)       # src at any byte address, dst at any element
        torch.cuda.synchronize()
        assert bool((dst[:4] == 0x77).all()) and bool((dst[4 + n:] == 0x77).all()) and not bool((dst[4:4 + n] == 0x77).all())
    finally:
        op.close()


@pytest.mark.parametrize("path", [R.MFMA, R.GENERIC])
def test_submit_before_set_weights_is_a_state_error(path):
    import torch
    op = dfa.DilatedConv((1, 4, 4, 32), 32, (3, 3), dilation=(2, 2), pad=(2, 2), force_path=path)
    try:
        a = torch.zeros(16 * 32, dtype=torch.uint8, device="cuda")
        dst = torch.zeros(16 * 32, dtype=torch.uint8, device="cuda")
        with pytest.raises(dfa.DfxError) as e:
            op.submit(a, dst)
        assert "dfx error 5" in str(e.value)
        with pytest.raises(dfa.DfxError) as e:
            op.submit_host(np.zeros((1, 4, 4, 32), dtype=np.uint8))
        assert "dfx error 5" in str(e.value)
        with pytest.raises(dfa.DfxError) as e:
            op.requant()
        assert "dfx error 5" in str(e.value)
        assert op.info().kernel_name.decode().endswith("(no weights)")
    finally:
        op.close()


@pytest.mark.parametrize("path", [R.MFMA, R.GENERIC])
def test_non_default_stream_and_submit_host(path):
    import torch
    case = R.DlCase("stream", 2, 32, 9, 7, 96, dil=(3, 2), pad=(3, 2), dst_dt=C.S32, bia_dt=C.S32, relu=False, per_channel=True,
                    seed=47600)
    data, ref = reference(case)
    got, info, route = run(case, data, force_path=path, stream=torch.cuda.Stream())
    hipref.assert_bit_equal(got, ref, "non-default stream path %d" % path)
    op = make_op(case, data, path)
    try:
        hipref.assert_bit_equal(op.submit_host(data["src"]), ref, "submit_host path %d" % path)
        hipref.assert_bit_equal(op.submit_host(data["src"]), ref, "submit_host again path %d" % path)
    finally:
        op.close()


def test_aspp_layer():
    """one real layer at bs 1: the d 12 branch of DeepLabv3's ASPP on MobileNetV2 -- 33 x 33 x 320 -> 256, pad 12, u8; ten
    K-steps streamed through LDS in four slabs (3 + 3 + 3 + 1), eight output blocks in two chunks, 35 strips; the MFMA path against the
    reference on every pixel"""
    case = R.DlCase("aspp-mnv2", 1, 320, 33, 33, 256, dil=(12, 12), pad=(12, 12), seed=47700, **R.OPTIONS[0])
    data = R.generate(case)
    ref = R.dilconv_ref(case, data)
    got, info, route = run(case, data, force_path=R.MFMA, on_device=True)
    assert info.path == R.MFMA and route == FAST and tuple(got.shape) == (1, 33, 33, 256), info.kernel_name
    hipref.assert_bit_equal(got.cpu().numpy(), ref, "ASPP [%s]" % info.kernel_name.decode())
    assert len(np.unique(ref)) > 100


# --- the C++ layer ------------------------------------------------------------------------------------------------------
_LAYERS = {  # dilconv_check.cc's layers: name -> (bs, ic, oc, ih, iw, k, s, (dh, dw), (pt, pl), out_hw, dst, bias, relu, per_channel, rm)
    "aspp_d2_u8": (3, 64, 32, 9, 7, 3, 1, (2, 2), (2, 2), None, C.U8, C.S32, False, False, 0),
    "aspp_d6_s8": (4, 32, 160, 8, 8, 3, 1, (6, 6), (6, 6), None, C.S8, C.UNDEF, True, True, 1),
    "slabs_s32": (5, 96, 32, 6, 5, 3, 1, (3, 1), (1, 0), None, C.S32, C.F32, False, True, 0),
    "crop_f32": (3, 32, 64, 11, 9, 3, 1, (2, 5), (0, 0), (6, 3), C.F32, C.S8, True, False, 0),
    "far_d18_u8": (2, 64, 32, 7, 5, 3, 1, (18, 18), (18, 18), None, C.U8, C.U8, False, True, 0),
    "s2_k5_d3_s8": (3, 3, 5, 15, 14, 5, 2, (3, 3), (6, 6), None, C.S8, C.S32, False, False, 0),
    "odd_k3_u8": (2, 20, 7, 6, 5, 3, 1, (2, 2), (2, 2), None, C.U8, C.UNDEF, False, False, 0),
}


def _run_check(outdir, shards=None):
    exe = os.path.join(TOOLS, "dilconv_check")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    env = {k: v for k, v in os.environ.items() if k != "DEEPFUSION_DEVICES"}
    if shards:
        env["DEEPFUSION_DEVICES"] = shards
    p = subprocess.run([exe, str(outdir)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0, p.stdout.decode()
    assert b"every one identical to grouped_conv() on the zero-stuffed window where that exists" in p.stdout, p.stdout.decode()
    # far_d18_u8: 37 x 37 x 64 taps are beyond what grouped_conv() accepts
    assert p.stdout.count(b": identical") == len(_LAYERS) - 1 and p.stdout.count(b"not expressible") == 1, p.stdout.decode()


def test_cpp_layer_gives_the_reference_bytes_on_any_device_count(tmp_path):
    """dilconv_check through deepfusion::dilated_conv: its dumped results equal the numpy reference of its dumped
    inputs, and DEEPFUSION_DEVICES = 1 and 2 give the same files"""
    dirs = {}
    for shards in ("1", "2"):
        d = tmp_path / ("dev" + shards)
        d.mkdir()
        _run_check(d, shards=shards)
        dirs[shards] = d
    names = sorted(os.listdir(str(dirs["1"])))
    assert len([n for n in names if n.endswith("_dst.bin")]) == len(_LAYERS)
    assert names == sorted(os.listdir(str(dirs["2"])))
    for n in names:
        assert (dirs["1"] / n).read_bytes() == (dirs["2"] / n).read_bytes(), n
    d = dirs["1"]
    for name, (bs, ic, oc, ih, iw, k, s, dil, pad, ohw, dst_dt, bia_dt, relu, pc, rm) in _LAYERS.items():
        case = R.DlCase(name, bs, ic, ih, iw, oc, k=(k, k), stride=(s, s), dil=dil, pad=pad, out_hw=ohw, dst_dt=dst_dt,
                        bia_dt=bia_dt, relu=relu, rm=rm, per_channel=pc)
        data = dict(src=np.fromfile(str(d / (name + "_src.bin")), dtype=np.uint8).reshape(bs, ih, iw, ic),
                    w=np.fromfile(str(d / (name + "_wei.bin")), dtype=np.int8).reshape(oc, ic, k, k),
                    bia=None if bia_dt == C.UNDEF else np.fromfile(str(d / (name + "_bia.bin")), dtype=C.NP_OF[bia_dt]),
                    scales=np.fromfile(str(d / (name + "_scales.bin")), dtype=np.float32))
        assert data["scales"].size == (oc if pc else 1)
        got = np.fromfile(str(d / (name + "_dst.bin")), dtype=C.NP_OF[dst_dt]).reshape(bs, case.oh, case.ow, oc)
        hipref.assert_bit_equal(got, R.dilconv_ref(case, data), "dilconv_check " + name)


def test_bench_dilconv_runs():
    out = subprocess.check_output([os.path.join(TOOLS, "bench_dilconv"), "-shape", "3", "-bs", "2", "-ih", "9", "-ic", "64", "-oc", "64",
                                   "-burning_iter", "1", "-iter", "2", "-rounds", "3", "-rotate_mb", "8"], timeout=120)
    for want in (b"(m) dilconv, MFMA path", b"(g) dilconv, generic path", b"(c) conv on 13x13 stuffed weights", b"HBM floor", b"matrix floor",
                 b"m/g", b"m/c", b"all legs byte-identical", b"auto picks MFMA"):
        assert want in out, out
    out = subprocess.check_output([os.path.join(TOOLS, "bench_dilconv"), "-shape", "5", "-bs", "1", "-ih", "5", "-ic", "64", "-oc", "32",
                                   "-burning_iter", "1", "-iter", "2", "-rounds", "3", "-rotate_mb", "8"], timeout=120)
    assert b"(c) not expressible: a 37x37 window on 64 channels is 87616 taps" in out, out
