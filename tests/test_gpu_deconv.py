"""GPU: the transposed conv op (dfx_deconv_*, deepfusion::deconvolution) against the numpy scatter reference of
tests/deconv_ref.py, bit for bit (tests/test_deconv_cpu.py pins that reference against the C oracle's dense conv on the
zero-stuffed tensor with flipped weights and against the grouped conv's reference).  Everything goes through the C ABI;
every output is written between guard bands; every case runs under both requant routes (DFX_NO_FAST forces the exact
one) and the route is asserted from requant()."""
import ctypes
import importlib
import os
import subprocess
from dataclasses import replace

import numpy as np
import pytest

import cases as C
import deconv_ref as R
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
    """the AUTO RULE of include/dfx.h (DFX_DECONV_MFMA): auto takes the MFMA kernel everywhere in its class (it is faster
    than the generic path and than conv() on the pre-stuffed tensor on every measured layer, profiles/deconv/)"""
    return R.MFMA


def make_op(case, data, force_path=AUTO):
    op = dfa.Deconv((case.bs, case.ih, case.iw, case.c), case.oc, case.k, stride=case.stride, pad=case.pad,
                    out_hw=(case.oh, case.ow), dst_dt=case.dst_dt, bia_dt=case.bia_dt, relu=case.relu, rm=case.rm,
                    nscales=data["scales"].size, force_path=force_path)
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
        ref = R.deconv_ref(case, data)
        ref.setflags(write=False)
        _REF[case] = (data, ref)
    return _REF[case]


def want_route(case, switch, path):
    """what set_weights must prove for reference-range and "wide" data: fast on the MFMA kernel with nearest rounding
    (everything is finite and far below 2^30), exact otherwise"""
    return FAST if (path == R.MFMA and case.rm == 0 and not switch) else EXACT


def want_name(case, path, route):
    dt = C.NAME_OF[case.dst_dt]
    if path == R.MFMA:
        return "deconv_mfma<%dx%d,s2,ic%d,oc%d,%s> %s" % (case.k + (case.c, case.oc, dt, "fast" if route == FAST else "exact"))
    return "deconv_generic<%dx%d,s%dx%d,ic%d,oc%d,%s> exact" % (case.k + case.stride + (case.c, case.oc, dt))


def check_table(table, force, switch, tuning):
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
        assert name == want_name(case, path, route), what
        hipref.assert_bit_equal(got, ref, what)
        names.add(name.split(" ")[0])
    return names


@pytest.mark.parametrize("geom", [g[0] for g in R.MFMA_GEOMS])
@pytest.mark.parametrize("force", [R.MFMA, AUTO], ids=["forced", "auto"])
@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_mfma_shapes(tuning, switch, force, geom):
    """one geometry of the class table, forced onto the MFMA kernel and on auto: a 1x1 image, odd sizes, a full strip plus
    one pixel, several strips, outputs cropped to odd sizes; one block, a partial chunk, several K-steps, a second weight
    chunk; bs 1 and 3; the option rows rotate"""
    table = R.mfma_table(geom)
    assert len(table) == 20
    names = check_table(table, force, switch, tuning)
    assert {n.split(",")[2] + "," + n.split(",")[3] for n in names} == {"ic%d,oc%d" % p for p in R.MFMA_CHANNELS}
    assert {n.split(",")[4] for n in names} == {"u8>", "s8>", "s32>", "f32>"}


@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_generic_path(tuning, switch):
    """stride 1, holes (stride 3 under a 2x2 window), mixed strides, 5x5 / 2 with output_padding; ic 1 / 3 / 20, oc 1 / 7 /
    48: info.path asserted.  A 4x4 window with ic beyond the LDS plan is outside the class, too."""
    big = R.DCase("lds", 1, 288, 2, 3, 32, k=(4, 4), pad=(1, 1), seed=32900, **R.OPTIONS[1])
    assert not big.mfma_class and replace(big, c=256).mfma_class
    names = check_table(R.generic_table() + [big], AUTO, switch, tuning)
    assert all(n.startswith("deconv_generic<") for n in names)


@pytest.mark.parametrize("geom", [g[0] for g in R.MFMA_GEOMS])
def test_permutation_case(geom):
    """distinct weights per (i, ky, kx) of a channel and per channel at every tap, the accumulators themselves (s32,
    scale 1): a swapped axis or a wrong flip in the packer or in the kernel's parity split shows"""
    case, data = R.permutation_case(geom)
    data, ref = reference(case, data)
    for path in (R.MFMA, R.GENERIC):
        got, info, route = run(case, data, force_path=path)
        assert info.path == path
        hipref.assert_bit_equal(got, ref, "permutation %s [%s]" % (case.ident(), info.kernel_name.decode()))


def _twin_cases():
    """every MFMA geometry at two channel pairs, cropped and uncropped, the option rows rotating"""
    out, j = [], 0
    for name, k, p, op in R.MFMA_GEOMS:
        for c, oc in ((32, 64), (64, 32)):
            ih, iw = 6, 9
            ohw = (2 * ih, 2 * iw) if op else (None if j % 2 == 0 else (2 * ih - 1, 2 * iw - 1))
            out.append(R.DCase("twin-" + name, 2, c, ih, iw, oc, k=k, pad=p, out_hw=ohw, seed=36200 + j, **R.OPTIONS[j % 6]))
            j += 1
    return out


@pytest.mark.parametrize("force", [R.MFMA, R.GENERIC])
@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_equal_to_group_conv_on_the_stuffed_tensor_on_the_device(tuning, switch, force):
    """defining property 1: Deconv == GroupConv(groups = 1, stride 1, padding k - 1 - pad) on the zero-stuffed tensor the
    test builds, with the flipped weights, compared on the device"""
    import torch
    if switch:
        tuning.setenv(switch, "1")
    for case in _twin_cases():
        data = R.generate(case)
        got, info, route = run(case, data, force_path=force, on_device=True)
        assert info.path == force
        stuffed = R.stuff(data["src"], case.stride)
        gc = dfa.GroupConv(stuffed.shape, case.oc, 1, case.k, stride=(1, 1), pad=R.twin_pad(case), out_hw=(case.oh, case.ow),
                           dst_dt=case.dst_dt, bia_dt=case.bia_dt, relu=case.relu, rm=case.rm, nscales=data["scales"].size)
        try:
            gc.set_weights(R.flip(data["w"]), data["scales"], bia=data["bia"])
            src = torch.from_numpy(stuffed).cuda()
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
def test_equal_to_conv_on_the_stuffed_tensor_on_the_device(tuning, switch, force):
    """defining property 2: Deconv == the unfused Conv on the same stuffed tensor and flipped weights, where the dense
    conv can express the layer, both run on the GPU"""
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
    assert n >= 3


@pytest.mark.parametrize("geom", [g[0] for g in R.MFMA_GEOMS])
def test_forced_paths_agree(geom):
    import torch
    _, k, p, op = [g for g in R.MFMA_GEOMS if g[0] == geom][0]
    case = R.DCase("forced", 2, 96, 7, 11, 96, k=k, pad=p, out_hw=(14, 22) if op else None, dst_dt=C.S8, bia_dt=C.S8, relu=False,
                   per_channel=True, seed=36300)
    data, ref = reference(case)
    outs = []
    for path in (R.MFMA, R.GENERIC):
        got, info, route = run(case, data, force_path=path, on_device=True)
        assert info.path == path and (route == FAST) == (path == R.MFMA)
        hipref.assert_bit_equal(got.cpu().numpy(), ref, "forced path %d" % path)
        outs.append(got)
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_more_work_items_than_workgroups(tuning, switch):
    """DFX_DECONV_GRID caps the grid at two workgroups (and at one and three): the workgroups loop over the (chunk, slot)
    units and their waves over the strips; oc 160 makes two weight chunks, so a workgroup reloads its LDS image"""
    if switch:
        tuning.setenv(switch, "1")
    todo = []
    for name, k, p, op in R.MFMA_GEOMS:
        case = R.DCase("loop-" + name, 3, 32, 9, 40, 160, k=k, pad=p, out_hw=(18, 80) if op else None, seed=37000, **R.OPTIONS[0])
        data, ref = reference(case)
        full = make_op(case, data, R.MFMA)
        try:
            units = full.info().grid                    # uncapped: one workgroup per (chunk, slot) unit
        finally:
            full.close()
        assert units >= 8 and units % 2 == 0, units
        todo.append((case, data, ref))
    for grid in (2, 1, 3):
        tuning.setenv("DFX_DECONV_GRID", grid)
        for case, data, ref in todo:
            got, info, route = run(case, data, force_path=R.MFMA)
            assert info.grid == grid and info.path == R.MFMA
            hipref.assert_bit_equal(got, ref, "%s grid %d [%s]" % (case.ident(), grid, info.kernel_name.decode()))


def test_nan_and_inf_scales_take_the_exact_route():
    """a NaN or an infinite scale must fail the fast route's proof; the bytes are the x86 ones: u8 255 / s8 -128"""
    for dst_dt, bad in ((C.U8, 255), (C.S8, -128)):
        case = R.DCase("nan", 2, 32, 4, 5, 32, k=(4, 4), pad=(1, 1), dst_dt=dst_dt, bia_dt=C.UNDEF, relu=False, per_channel=True,
                       seed=37100)
        for poison in (np.nan, np.inf, -np.inf):
            data = R.generate(case)
            data["scales"][19] = poison
            data["src"][...] = np.maximum(data["src"], 1)
            data["w"][19] = np.abs(data["w"][19]) + 1
            ref = R.deconv_ref(case, data)
            got, info, route = run(case, data, force_path=R.MFMA)
            assert info.path == R.MFMA and route == EXACT and info.kernel_name.decode().endswith("exact"), (poison, info.kernel_name)
            hipref.assert_bit_equal(got, ref, "%s scale %r" % (case.ident(), poison))
            if not (poison == -np.inf and dst_dt == C.U8):       # (-inf through the u8 ReLU is 0)
                assert (got[..., 19] == bad).all(), (poison, dst_dt)


def test_nan_and_inf_bias_take_the_exact_route():
    """an f32 bias that is NaN or infinite must fail the fast route's proof on its own clause (the scale is ordinary);
    the exact route then gives the x86 results"""
    for dst_dt, bad in ((C.U8, 255), (C.S8, -128)):
        case = R.DCase("nanbias", 2, 32, 4, 5, 32, dst_dt=dst_dt, bia_dt=C.F32, relu=False, per_channel=True, seed=37150)
        for poison in (np.nan, np.inf, -np.inf):
            data = R.generate(case)
            data["bia"] = data["bia"].copy()
            data["bia"][21] = poison
            ref = R.deconv_ref(case, data)
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
    attained by the data at one output pixel of one parity: the route, the bytes (every dst type), and the attained
    accumulator"""
    for dst_dt in (C.S32, C.U8, C.S8, C.F32):
        case, data = R.edge_case(edge, dst_dt)
        ref = R.deconv_ref(case, data)
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
    hipref.assert_bit_equal(got, R.deconv_ref(case, data), "forced exact")


def test_info_reports_the_launch_and_the_unstuffed_counts():
    case = R.DCase("info", 2, 64, 5, 70, 160, k=(4, 4), pad=(1, 1), **R.OPTIONS[0])
    op = make_op(case, R.generate(case), R.MFMA)
    try:
        i = op.info()
        assert (case.oh, case.ow) == (10, 140)
        assert i.path == R.MFMA and i.block == 256 and i.device >= 0
        # base grid: rows 0 .. 5, columns 0 .. 70 -> 2 * 6 * 71 = 852 base pixels, 27 strips, 7 slots of 4 waves; 5 output
        # blocks of 2 K-steps x 16 KB each, 4 in LDS at once -> 2 chunks
        assert i.grid == 7 * 2, i.grid
        assert i.lds_bytes == 4 * 2 * 16 * 1024 + 6 * 128 * 4 + 4 * 32 * 144, i.lds_bytes
        # every input pixel meets every tap, except those whose product falls outside the output: per axis, in * k taps
        # less the first row's ky = 0 and the last row's ky = 3 (pad 1)
        assert i.algorithmic_ops == 2 * 2 * 64 * 160 * (5 * 4 - 2) * (70 * 4 - 2)
        assert i.algorithmic_bytes == 2 * 5 * 70 * 64 + 160 * 64 * 16 + 2 * 10 * 140 * 160      # src un-stuffed
        assert i.kernel_name.decode() == "deconv_mfma<4x4,s2,ic64,oc160,u8> fast"
    finally:
        op.close()
    case3 = R.DCase("info3", 2, 3, 4, 5, 7, k=(2, 2), stride=(3, 3), dst_dt=C.S32, bia_dt=C.S32, relu=False)
    op = make_op(case3, R.generate(case3))
    try:
        i = op.info()
        assert (case3.oh, case3.ow) == (11, 14)
        assert i.path == R.GENERIC and i.block == 256 and i.lds_bytes == 0
        assert i.kernel_name.decode() == "deconv_generic<2x2,s3x3,ic3,oc7,s32> exact"
        assert i.algorithmic_ops == 2 * 2 * 3 * 7 * (4 * 2) * (5 * 2)                            # the holes cost nothing
        assert i.algorithmic_bytes == 2 * 4 * 5 * 3 + 7 * 3 * 4 + 2 * 11 * 14 * 7 * 4
    finally:
        op.close()


def test_set_weights_again_takes_effect():
    import torch
    case = R.DCase("reweigh", 2, 64, 7, 9, 64, k=(4, 4), pad=(1, 1), seed=37400, **R.OPTIONS[0])
    data = R.generate(case)
    data2 = dict(R.generate(replace(case, seed=77, wide=True)), src=data["src"])
    ref1, ref2 = R.deconv_ref(case, data), R.deconv_ref(case, data2)
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
    case = R.DCase("3streams", 2, 64, 10, 13, 64, k=(4, 4), pad=(1, 1), dst_dt=C.U8, bia_dt=C.S32, per_channel=True, seed=37500)
    data = R.generate(case)
    streams = [torch.cuda.Stream() for _ in range(3)]
    devs, refs = [], []
    for k in range(3):
        dk = dict(data, src=R.generate(replace(case, seed=300 + k))["src"])
        devs.append(torch.from_numpy(dk["src"]).cuda())
        refs.append(R.deconv_ref(case, dk))
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
    case = R.DCase("refuse", 1, 32, 3, 4, 32, bia_dt=C.UNDEF)
    op = make_op(case, R.generate(case), R.MFMA)
    try:
        n = 6 * 8 * 32
        a = torch.zeros(12 * 32 + 32, dtype=torch.uint8, device="cuda")
        dst = torch.full((n + 32,), 0x77, dtype=torch.uint8, device="cuda")
        assert L.dfx_deconv_submit(op._h, None, ctypes.c_void_p(dst.data_ptr()), st) == 1       # null src
        assert L.dfx_deconv_submit(op._h, ctypes.c_void_p(a.data_ptr()), None, st) == 1         # null dst
        assert L.dfx_deconv_submit(None, ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(dst.data_ptr()), st) == 1
        for off_s, off_d in ((8, 0), (0, 8), (1, 0), (0, 4), (4, 4)):
            rc = L.dfx_deconv_submit(op._h, ctypes.c_void_p(a.data_ptr() + off_s), ctypes.c_void_p(dst.data_ptr() + off_d), st)
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
    # generic path: pointers aligned to the element
    case = R.DCase("refuse-gen", 1, 3, 3, 4, 5, dst_dt=C.S32, bia_dt=C.UNDEF, relu=False)
    op = make_op(case, R.generate(case))
    try:
        assert op.info().path == R.GENERIC
        n = 6 * 8 * 5 * 4
        a = torch.zeros(12 * 3 + 16, dtype=torch.uint8, device="cuda")
        dst = torch.full((n + 16,), 0x77, dtype=torch.uint8, device="cuda")
        for off_d in (1, 2, 3):
            rc = L.dfx_deconv_submit(op._h, ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(dst.data_ptr() + off_d), st)
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
    op = dfa.Deconv((1, 4, 4, 32), 32, (2, 2), force_path=path)
    try:
        a = torch.zeros(16 * 32, dtype=torch.uint8, device="cuda")
        dst = torch.zeros(64 * 32, dtype=torch.uint8, device="cuda")
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
    case = R.DCase("stream", 2, 32, 9, 7, 96, k=(3, 3), pad=(1, 1), out_hw=(18, 14), dst_dt=C.S32, bia_dt=C.S32, relu=False,
                   per_channel=True, seed=37600)
    data, ref = reference(case)
    got, info, route = run(case, data, force_path=path, stream=torch.cuda.Stream())
    hipref.assert_bit_equal(got, ref, "non-default stream path %d" % path)
    op = make_op(case, data, path)
    try:
        hipref.assert_bit_equal(op.submit_host(data["src"]), ref, "submit_host path %d" % path)
        hipref.assert_bit_equal(op.submit_host(data["src"]), ref, "submit_host again path %d" % path)
    finally:
        op.close()


def test_pose_head_layer():
    """a pose / CenterNet head layer at bs 2: 16 x 12 x 256, 4x4 / 2 pad 1 -> 32 x 24 x 256, u8, eight K-steps and eight
    output blocks in chunks of one (its fragments fill the LDS); the reference on the output rows 0, 1, 15, 16, 30 and 31
    (both image edges, both parities), on both paths"""
    case = R.DCase("pose-head", 2, 256, 16, 12, 256, k=(4, 4), pad=(1, 1), seed=37700, **R.OPTIONS[0])
    rows = (0, 1, 15, 16, 30, 31)
    data = R.generate(case)
    ref = R.deconv_ref(case, data, rows=rows)
    assert case.lds_blocks == 1
    for path in (R.MFMA, R.GENERIC):
        got, info, route = run(case, data, force_path=path, on_device=True)
        assert info.path == path and tuple(got.shape) == (2, 32, 24, 256), info.kernel_name
        assert route == (FAST if path == R.MFMA else EXACT)
        hipref.assert_bit_equal(got[:, list(rows)].cpu().numpy(), ref, "pose head [%s]" % info.kernel_name.decode())
        assert not bool((got == hipref.POISON_BYTE).all(dim=3).any()), "an output pixel was not written"


# --- the C++ layer ------------------------------------------------------------------------------------------------------
_LAYERS = {  # deconv_check.cc's layers: name -> (bs, ic, oc, ih, iw, k, s, p, out_hw, dst, bias, relu, per_channel, rm)
    "unet_k2_u8": (3, 64, 32, 7, 9, 2, 2, 0, None, C.U8, C.S32, False, False, 0),
    "pose_k4_s8": (4, 32, 64, 5, 6, 4, 2, 1, None, C.S8, C.UNDEF, True, True, 1),
    "keras_k3_s32": (5, 32, 32, 6, 5, 3, 2, 1, (12, 10), C.S32, C.F32, False, True, 0),
    "gan_k4p0_f32": (3, 64, 96, 4, 4, 4, 2, 0, None, C.F32, C.S8, True, False, 0),
    "crop_k4_u8": (3, 32, 32, 5, 7, 4, 2, 1, (9, 13), C.U8, C.U8, False, True, 0),
    "holes_s3_s8": (3, 3, 7, 4, 5, 2, 3, 0, None, C.S8, C.S32, False, False, 0),
    "rgb_k5_u8": (2, 20, 3, 6, 5, 5, 2, 2, (12, 10), C.U8, C.UNDEF, False, False, 0),
}


def _run_check(outdir, shards=None):
    exe = os.path.join(TOOLS, "deconv_check")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    env = {k: v for k, v in os.environ.items() if k != "DEEPFUSION_DEVICES"}
    if shards:
        env["DEEPFUSION_DEVICES"] = shards
    p = subprocess.run([exe, str(outdir)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0, p.stdout.decode()
    assert b"every one identical to grouped_conv() on the stuffed tensor with flipped weights" in p.stdout, p.stdout.decode()
    assert p.stdout.count(b": identical") == len(_LAYERS), p.stdout.decode()


def test_cpp_layer_gives_the_reference_bytes_on_any_device_count(tmp_path):
    """deconv_check through deepfusion::deconvolution: its dumped results equal the numpy reference of its dumped
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
    for name, (bs, ic, oc, ih, iw, k, s, p, ohw, dst_dt, bia_dt, relu, pc, rm) in _LAYERS.items():
        case = R.DCase(name, bs, ic, ih, iw, oc, k=(k, k), stride=(s, s), pad=(p, p), out_hw=ohw, dst_dt=dst_dt,
                       bia_dt=bia_dt, relu=relu, rm=rm, per_channel=pc)
        data = dict(src=np.fromfile(str(d / (name + "_src.bin")), dtype=np.uint8).reshape(bs, ih, iw, ic),
                    w=np.fromfile(str(d / (name + "_wei.bin")), dtype=np.int8).reshape(oc, ic, k, k),
                    bia=None if bia_dt == C.UNDEF else np.fromfile(str(d / (name + "_bia.bin")), dtype=C.NP_OF[bia_dt]),
                    scales=np.fromfile(str(d / (name + "_scales.bin")), dtype=np.float32))
        assert data["scales"].size == (oc if pc else 1)
        got = np.fromfile(str(d / (name + "_dst.bin")), dtype=C.NP_OF[dst_dt]).reshape(bs, case.oh, case.ow, oc)
        hipref.assert_bit_equal(got, R.deconv_ref(case, data), "deconv_check " + name)


def test_bench_deconv_runs():
    out = subprocess.check_output([os.path.join(TOOLS, "bench_deconv"), "-shape", "3", "-bs", "2", "-burning_iter", "1", "-iter", "2",
                                   "-rounds", "3", "-rotate_mb", "48"], timeout=120)
    for want in (b"(a) deconv, auto", b"(b) deconv, generic path", b"(c) conv  on a pre-stuffed tensor", b"(m) deconv, MFMA path",
                 b"stuffing not timed", b"HBM floor", b"matrix floor", b"a/b", b"a/c", b"m/b", b"m/c", b"all legs byte-identical"):
        assert want in out, out
