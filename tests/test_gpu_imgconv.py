"""GPU: the first-layer conv op (dfx_imgconv_*, deepfusion::image_conv) against the numpy reference of
tests/imgconv_ref.py, bit for bit (tests/test_imgconv_cpu.py pins that reference against the C oracle's dense conv on the
image zero-padded to 16 channels and against the grouped conv's reference).  Everything goes through the C ABI; every
output is written between guard bands; every case runs under both requant routes (DFX_NO_FAST forces the exact one)
and the route is asserted from requant()."""
import ctypes
import importlib
import os
import subprocess
from dataclasses import replace

import numpy as np
import pytest

import cases as C
import hipref
import imgconv_ref as R

pytestmark = pytest.mark.gpu
dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "deep-fusion_amd", "tools")
BAND = 1 << 16       # guard bytes on each side of dst
EXACT, FAST = 0, 1


def make_op(case, data, force_path=-1):
    op = dfa.ImageConv((case.bs, case.ih, case.iw, case.c), case.oc, case.k, stride=case.stride, pad=case.pad,
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


def run(case, data, force_path=-1, stream=None, on_device=False, src_dev=None):
    """-> (dst, info, route): one submit into a guarded dst; the guard bands must survive.  src_dev: a device pointer
    to read the source from instead of an upload of data["src"]"""
    import torch
    op = make_op(case, data, force_path)
    try:
        info, route = op.info(), op.requant()
        src = torch.from_numpy(data["src"]).cuda() if src_dev is None else src_dev
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
        ref = R.imgconv_ref(case, data)
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
        return "imgconv_mfma<%dx%d,s%d,ic%d,oc%d,%s> %s" % (case.k + (case.stride[0], case.c, case.oc, dt, "fast" if route == FAST else "exact"))
    return "imgconv_generic<%dx%d,s%dx%d,ic%d,oc%d,%s> exact" % (case.k + case.stride + (case.c, case.oc, dt))


def check_table(table, path, switch, tuning):
    if switch:
        tuning.setenv(switch, "1")
    names = set()
    for case in table:
        data, ref = reference(case)
        got, info, route = run(case, data)
        name = info.kernel_name.decode()
        what = "%s [%s] %s" % (case.ident(), name, switch)
        assert info.path == path, what
        assert route == want_route(case, switch, path), what
        assert name == want_name(case, path, route), what
        hipref.assert_bit_equal(got, ref, what)
        names.add(name.split(" ")[0])
    return names


@pytest.mark.parametrize("geom", [g[0] for g in R.MFMA_GEOMS])
@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_mfma_shapes(tuning, switch, geom):
    """one geometry of the class table: ic 3 and 4, oc 32 .. 128, bs 1 and 3, an image smaller than the window, odd row
    bytes, output rows that end in a partial strip, two long rows, windows that hang over; the option rows rotate"""
    table = R.mfma_table(geom)
    assert len(table) == 48
    names = check_table(table, R.MFMA, switch, tuning)
    assert {n.split(",")[2] + "," + n.split(",")[3] for n in names} == {"ic%d,oc%d" % (c, oc) for c in (3, 4) for oc in R.MFMA_OC}
    assert {n.split(",")[4] for n in names} == {"u8>", "s8>", "s32>", "f32>"}


@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_generic_path(tuning, switch):
    """ic 1 / 2 / 3, windows 5x5 / 1 and 11x11 / 4, oc 7 / 16 / 48: info.path asserted"""
    names = check_table(R.generic_table(), R.GENERIC, switch, tuning)
    assert all(n.startswith("imgconv_generic<") for n in names)


@pytest.mark.parametrize("k,stride", R.MFMA_WINDOWS)
@pytest.mark.parametrize("c", [3, 4])
def test_permutation_case(k, stride, c):
    """distinct weights per (c, ky, kx) of a channel and per channel at every tap, the accumulators themselves (s32,
    scale 1): a swapped axis in the packer or in the kernel's K layout shows"""
    case, data = R.permutation_case(k, stride, c)
    data, ref = reference(case, data)
    for path in (R.MFMA, R.GENERIC):
        got, info, route = run(case, data, force_path=path)
        assert info.path == path
        hipref.assert_bit_equal(got, ref, "permutation %s [%s]" % (case.ident(), info.kernel_name.decode()))


@pytest.mark.parametrize("path", [R.MFMA, R.GENERIC])
@pytest.mark.parametrize("k,stride,pad", [((7, 7), (2, 2), (3, 3)), ((3, 3), (1, 1), (1, 1))])
def test_forced_paths_agree(path, k, stride, pad):
    case = R.ICase("forced", 2, 3, 17, 23, 96, k=k, stride=stride, pad=pad, dst_dt=C.S8, bia_dt=C.S8, relu=False, per_channel=True,
                   seed=26300)
    data, ref = reference(case)
    got, info, route = run(case, data, force_path=path)
    assert info.path == path and (route == FAST) == (path == R.MFMA)
    hipref.assert_bit_equal(got, ref, "forced path %d" % path)


def _twin_cases(oc):
    out, j = [], 0
    for c in (3, 4):
        for name, k, s, p in R.MFMA_GEOMS:
            out.append(R.ICase("twin-" + name, 2, c, 12, 20, oc, k=k, stride=s, pad=p, seed=26200 + j, **R.OPTIONS[j % 4]))
            j += 1
    return out


@pytest.mark.parametrize("oc", [32, 64])
@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_equal_to_group_conv_with_one_group_on_the_device(tuning, switch, oc):
    """defining property 1: ImageConv == GroupConv(groups = 1) on the same tensors, compared on the device"""
    import torch
    if switch:
        tuning.setenv(switch, "1")
    for case in _twin_cases(oc):
        data = R.generate(case)
        got, info, route = run(case, data, on_device=True)
        assert info.path == R.MFMA
        gc = dfa.GroupConv((case.bs, case.ih, case.iw, case.c), case.oc, 1, case.k, stride=case.stride, pad=case.pad,
                           out_hw=(case.oh, case.ow), dst_dt=case.dst_dt, bia_dt=case.bia_dt, relu=case.relu, rm=case.rm,
                           nscales=data["scales"].size)
        try:
            gc.set_weights(data["w"], data["scales"], bia=data["bia"])
            # (the grouped op wants a 16-byte aligned src: a fresh allocation is)
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


@pytest.mark.parametrize("oc", [32, 64])
@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_equal_to_reorder_and_conv_on_the_device(tuning, switch, oc):
    """defining property 2: ImageConv == the channel-padding Reorder (ic -> 16) followed by Conv with zero weights on
    the channels >= ic, both run on the GPU"""
    import torch
    if switch:
        tuning.setenv(switch, "1")
    for case in _twin_cases(oc):
        data = R.generate(case)
        got, info, route = run(case, data, on_device=True)
        assert info.path == R.MFMA
        ddata = R.dense_data(case, data)
        ro = dfa.Reorder((case.bs, case.c, case.ih, case.iw), np.uint8, np.uint8, src_fmt=dfa.FMT_NHWC, dst_fmt=dfa.FMT_NHWC, dst_c=16)
        conv = hipref.make_conv(R.dense_case(case), ddata)
        try:
            src = torch.from_numpy(data["src"]).cuda()
            src16 = torch.full((case.bs, case.ih, case.iw, 16), 0x77, dtype=torch.uint8, device="cuda")
            want = torch.empty(conv.dst_shape, dtype=hipref.torch_dtype(case.dst_dt), device="cuda")
            ro.submit(src, src16)
            conv.submit(src16, want)
            torch.cuda.synchronize()
            cname = conv.info().kernel_name.decode()
            assert torch.equal(src16.cpu(), torch.from_numpy(ddata["src"])), "the reorder did not pad with zeros"
        finally:
            ro.close()
            conv.close()
        assert tuple(got.shape) == tuple(want.shape)
        assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)), "%s: %s differs from reorder + %s" % (
            case.ident(), info.kernel_name.decode(), cname)


@pytest.mark.parametrize("path", [R.MFMA, R.GENERIC])
@pytest.mark.parametrize("c", [3, 4])
def test_byte_misaligned_src(path, c):
    """src at 1, 2 and 3 bytes into a larger buffer whose other bytes are 0xFF: a lane that read a neighbouring byte
    as a pixel (before the first, behind the last, or the 4th byte of a 3-byte pixel) would change the result.  The
    image is 17 x 23 (odd row bytes for ic = 3), windows clipped on every side."""
    import torch
    for k, stride, pad in (((7, 7), (2, 2), (3, 3)), ((3, 3), (1, 1), (1, 1)), ((3, 3), (2, 2), (0, 0))):
        case = R.ICase("misal", 2, c, 17, 23, 32, k=k, stride=stride, pad=pad, dst_dt=C.S32, bia_dt=C.UNDEF, relu=False,
                       seed=26400 + c)
        data, ref = reference(case)
        n = data["src"].size
        for off in (0, 1, 2, 3):
            big = torch.full((256 + n + 256,), 0xFF, dtype=torch.uint8, device="cuda")
            assert big.data_ptr() % 16 == 0
            big[128 + off:128 + off + n] = torch.from_numpy(data["src"].reshape(-1)).cuda()
            got, info, route = run(case, data, force_path=path, src_dev=big.data_ptr() + 128 + off)
            assert info.path == path
            hipref.assert_bit_equal(got, ref, "src + %d bytes, %s [%s]" % (off, case.ident(), info.kernel_name.decode()))


def test_image_of_a_few_bytes():
    """a 3 x 5 x 3 image, 45 bytes (no multiple of 4): the load groups of its last pixels cannot take whole dwords
    inside the tensor and go byte by byte"""
    import torch
    for k, stride, pad in (((7, 7), (2, 2), (3, 3)), ((3, 3), (1, 1), (1, 1))):
        case = R.ICase("tiny", 1, 3, 3, 5, 32, k=k, stride=stride, pad=pad, dst_dt=C.S32, bia_dt=C.UNDEF, relu=False, seed=26450)
        data, ref = reference(case)
        got, info, route = run(case, data)
        assert info.path == R.MFMA
        hipref.assert_bit_equal(got, ref, "tiny %s" % case.ident())


@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_more_work_items_than_workgroups(tuning, switch):
    """DFX_IMGCONV_GRID caps the grid at one workgroup and at three: the workgroups loop over the (image, band, column
    block) items -- 20, 60 and 20 of them, which three does not always divide"""
    if switch:
        tuning.setenv(switch, "1")
    todo = []
    for k, stride, pad in (((7, 7), (2, 2), (3, 3)), ((3, 3), (1, 1), (1, 1)), ((3, 3), (2, 2), (1, 1))):
        case = R.ICase("loop", 5, 3, 40, 150, 96, k=k, stride=stride, pad=pad, seed=27000, **R.OPTIONS[0])
        data, ref = reference(case)
        full = make_op(case, data)
        try:
            items = full.info().grid                    # uncapped: one workgroup per item
        finally:
            full.close()
        assert items >= 20, items
        todo.append((case, data, ref))
    for grid in (1, 3):
        tuning.setenv("DFX_IMGCONV_GRID", grid)
        for case, data, ref in todo:
            got, info, route = run(case, data)
            assert info.grid == grid and info.path == R.MFMA
            hipref.assert_bit_equal(got, ref, "%s grid %d [%s]" % (case.ident(), grid, info.kernel_name.decode()))


def test_nan_and_inf_scales_take_the_exact_route():
    """a NaN or an infinite scale must fail the fast route's proof; the bytes are the x86 ones: u8 255 / s8 -128"""
    for dst_dt, bad in ((C.U8, 255), (C.S8, -128)):
        case = R.ICase("nan", 2, 3, 6, 7, 32, dst_dt=dst_dt, bia_dt=C.UNDEF, relu=False, per_channel=True, seed=27100)
        for poison in (np.nan, np.inf, -np.inf):
            data = R.generate(case)
            data["scales"][19] = poison
            data["src"][...] = np.maximum(data["src"], 1)
            data["w"][19] = np.abs(data["w"][19]) + 1
            ref = R.imgconv_ref(case, data)
            got, info, route = run(case, data)
            assert info.path == R.MFMA and route == EXACT and info.kernel_name.decode().endswith("exact"), (poison, info.kernel_name)
            hipref.assert_bit_equal(got, ref, "%s scale %r" % (case.ident(), poison))
            if not (poison == -np.inf and dst_dt == C.U8):       # (-inf through the u8 ReLU is 0)
                assert (got[..., 19] == bad).all(), (poison, dst_dt)


def test_nan_and_inf_bias_take_the_exact_route():
    """an f32 bias that is NaN or infinite must fail the fast route's proof on its own clause (the scale is ordinary);
    the exact route then gives the x86 results"""
    for dst_dt, bad in ((C.U8, 255), (C.S8, -128)):
        case = R.ICase("nanbias", 2, 3, 6, 7, 32, dst_dt=dst_dt, bia_dt=C.F32, relu=False, per_channel=True, seed=27150)
        for poison in (np.nan, np.inf, -np.inf):
            data = R.generate(case)
            data["bia"] = data["bia"].copy()
            data["bia"][21] = poison
            ref = R.imgconv_ref(case, data)
            got, info, route = run(case, data)
            assert info.path == R.MFMA and route == EXACT and info.kernel_name.decode().endswith("exact"), (poison, info.kernel_name)
            hipref.assert_bit_equal(got, ref, "%s bias %r" % (case.ident(), poison))
            assert (got[..., 21] == (0 if (poison == -np.inf and dst_dt == C.U8) else bad)).all(), (poison, dst_dt)
            data["bia"][21] = 1.0       # the same numbers with that one bias finite are proven fast: the clause alone decided
            op = make_op(case, data)
            try:
                assert op.requant() == FAST
            finally:
                op.close()


@pytest.mark.parametrize("edge", R.EDGES, ids=lambda e: e.name)
def test_fast_route_proof_edges(tuning, edge):
    """(255 * max(P, N) + |bias|) * |scale| <= 2^30 at the last value it admits and the first it rejects, with the bound
    attained by the data: the route, the bytes (every dst type), and the attained accumulator"""
    for dst_dt in (C.S32, C.U8, C.S8, C.F32):
        case, data = R.edge_case(edge, dst_dt)
        ref = R.imgconv_ref(case, data)
        got, info, route = run(case, data)
        assert info.path == R.MFMA and route == (FAST if edge.fast else EXACT), (edge.name, dst_dt, info.kernel_name)
        hipref.assert_bit_equal(got, ref, "%s %s" % (edge.name, info.kernel_name.decode()))
    # the bound is attained: the accumulator itself (s32 dst, scale 1, no bias) on the device
    case, data = R.edge_case(edge, C.S32)
    neutral = dict(data, bia=None, scales=np.ones(1, dtype=np.float32))
    got, info, route = run(replace(case, bia_dt=C.UNDEF, per_channel=False), neutral)
    acc, bound, P, N = R.edge_attained(edge, case, data)
    assert int(got[0 if edge.which == "max" else 1, 1, 1, R.EDGE_CHANNEL]) == bound == acc
    # round-down and DFX_NO_FAST reject whatever the numbers are
    case, data = R.edge_case(R.EDGES[0], C.U8)
    got, info, route = run(replace(case, rm=1), data)
    assert route == EXACT
    tuning.setenv("DFX_NO_FAST", "1")
    got, info, route = run(case, data)
    assert route == EXACT
    hipref.assert_bit_equal(got, R.imgconv_ref(case, data), "forced exact")


def test_info_reports_the_launch_and_the_true_channel_traffic():
    case = R.ICase("info", 2, 3, 33, 70, 64, k=(7, 7), stride=(2, 2), pad=(3, 3), **R.OPTIONS[0])
    op = make_op(case, R.generate(case))
    try:
        i = op.info()
        opx = 2 * 17 * 35
        assert (case.oh, case.ow) == (17, 35)
        assert i.path == R.MFMA and i.block == 512 and i.device >= 0
        # one column block of 35, bands of 512 // 35 = 14 rows: 2 bands per image; halo 33 rows x 76 pixels
        assert i.grid == 2 * 2, i.grid
        assert i.lds_bytes == 2 * 7 * 1024 + 3 * 128 * 4 + 8 * 32 * 144 + 33 * 76 * 4, i.lds_bytes
        assert i.algorithmic_ops == 2 * 49 * 3 * opx * 64
        assert i.algorithmic_bytes == 2 * 33 * 70 * 3 + 64 * 3 * 49 + opx * 64        # 3 bytes per pixel, not 4 or 16
        assert i.kernel_name.decode() == "imgconv_mfma<7x7,s2,ic3,oc64,u8> fast"
    finally:
        op.close()
    case5 = R.ICase("info5", 2, 2, 13, 37, 7, k=(5, 5), pad=(2, 2), stride=(2, 2), dst_dt=C.S32, bia_dt=C.S32, relu=False)
    op = make_op(case5, R.generate(case5))
    try:
        i = op.info()
        assert i.path == R.GENERIC and i.block == 256 and i.lds_bytes == 0
        assert i.kernel_name.decode() == "imgconv_generic<5x5,s2x2,ic2,oc7,s32> exact"
        assert i.algorithmic_ops == 2 * 25 * 2 * 2 * 7 * 19 * 7
        assert i.algorithmic_bytes == 2 * 13 * 37 * 2 + 7 * 2 * 25 + 2 * 7 * 19 * 7 * 4
    finally:
        op.close()


def test_set_weights_again_takes_effect():
    import torch
    case = R.ICase("reweigh", 2, 3, 17, 23, 64, k=(7, 7), stride=(2, 2), pad=(3, 3), seed=27400, **R.OPTIONS[0])
    data = R.generate(case)
    data2 = dict(R.generate(replace(case, seed=77, wide=True)), src=data["src"])
    ref1, ref2 = R.imgconv_ref(case, data), R.imgconv_ref(case, data2)
    assert not np.array_equal(ref1, ref2)
    op = make_op(case, data)
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
    case = R.ICase("3streams", 2, 3, 40, 37, 64, k=(7, 7), stride=(2, 2), pad=(3, 3), dst_dt=C.U8, bia_dt=C.S32, per_channel=True,
                   seed=27500)
    data = R.generate(case)
    streams = [torch.cuda.Stream() for _ in range(3)]
    devs, refs = [], []
    for k in range(3):
        dk = dict(data, src=R.generate(replace(case, seed=300 + k))["src"])
        devs.append(torch.from_numpy(dk["src"]).cuda())
        refs.append(R.imgconv_ref(case, dk))
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
    case = R.ICase("refuse", 1, 3, 5, 7, 32, bia_dt=C.UNDEF)
    data = R.generate(case)
    op = make_op(case, data)
    try:
        n = 35 * 32
        a = torch.zeros(35 * 3 + 32, dtype=torch.uint8, device="cuda")
        dst = torch.full((n + 32,), 0x77, dtype=torch.uint8, device="cuda")
        L = capi.lib()
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert L.dfx_imgconv_submit(op._h, None, ctypes.c_void_p(dst.data_ptr()), st) == 1       # null src
        assert L.dfx_imgconv_submit(op._h, ctypes.c_void_p(a.data_ptr()), None, st) == 1         # null dst
        assert L.dfx_imgconv_submit(None, ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(dst.data_ptr()), st) == 1
        for od in (8, 1, 4, 2):                                                                  # dst: 16-byte aligned
            rc = L.dfx_imgconv_submit(op._h, ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(dst.data_ptr() + od), st)
            assert rc == 1 and b"16-byte aligned" in L.dfx_last_error(), (od, rc)
        with pytest.raises(dfa.DfxError):
            op.submit(a, dst.data_ptr() + 8)
        torch.cuda.synchronize()
        assert bool((dst == 0x77).all()), "a refused submit wrote to dst"
        op.submit(a.data_ptr() + 5, dst)             # src at any byte address goes through
        torch.cuda.synchronize()
        assert bool((dst[n:] == 0x77).all()) and not bool((dst[:n] == 0x77).all())
    finally:
        op.close()


def test_submit_before_set_weights_is_a_state_error():
    import torch
    op = dfa.ImageConv((1, 4, 4, 3), 32, (3, 3))
    try:
        a = torch.zeros(16 * 3, dtype=torch.uint8, device="cuda")
        dst = torch.zeros(16 * 32, dtype=torch.uint8, device="cuda")
        with pytest.raises(dfa.DfxError) as e:
            op.submit(a, dst)
        assert "dfx error 5" in str(e.value)
        with pytest.raises(dfa.DfxError) as e:
            op.submit_host(np.zeros((1, 4, 4, 3), dtype=np.uint8))
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
    case = R.ICase("stream", 2, 4, 20, 17, 96, k=(3, 3), stride=(2, 2), pad=(1, 1), dst_dt=C.S32, bia_dt=C.S32, relu=False,
                   per_channel=True, seed=27600)
    data, ref = reference(case)
    got, info, route = run(case, data, force_path=path, stream=torch.cuda.Stream())
    hipref.assert_bit_equal(got, ref, "non-default stream path %d" % path)
    op = make_op(case, data, path)
    try:
        hipref.assert_bit_equal(op.submit_host(data["src"]), ref, "submit_host path %d" % path)
        hipref.assert_bit_equal(op.submit_host(data["src"]), ref, "submit_host again path %d" % path)
    finally:
        op.close()


def test_resnet_conv1():
    """ResNet's conv1 at bs 2: 224 x 224 x 3, 7x7 / 2 pad 3 -> 112 x 112 x 64, u8; the reference on the output rows 0, 1,
    55, 56, 110 and 111 (both image edges and a seam between two bands)"""
    import torch
    case = R.ICase("resnet-conv1", 2, 3, 224, 224, 64, k=(7, 7), stride=(2, 2), pad=(3, 3), seed=27700, **R.OPTIONS[0])
    rows = (0, 1, 55, 56, 110, 111)
    data = R.generate(case)
    ref = R.imgconv_ref(case, data, rows=rows)
    got, info, route = run(case, data, on_device=True)
    assert info.path == R.MFMA and route == FAST and tuple(got.shape) == (2, 112, 112, 64), info.kernel_name
    hipref.assert_bit_equal(got[:, list(rows)].cpu().numpy(), ref, "resnet conv1 [%s]" % info.kernel_name.decode())
    assert not bool((got == hipref.POISON_BYTE).all(dim=3).any()), "an output pixel was not written"


# --- the C++ layer ------------------------------------------------------------------------------------------------------
_LAYERS = {  # imgconv_check.cc's layers: name -> (bs, ic, oc, ih, iw, k, s, p, out_hw, dst, bias, relu, per_channel, rm)
    "res_k7_u8": (3, 3, 64, 20, 23, 7, 2, 3, None, C.U8, C.S32, False, False, 0),
    "vgg_k3_s8": (4, 3, 64, 9, 11, 3, 1, 1, None, C.S8, C.UNDEF, True, True, 1),
    "mob_k3s2_s32": (5, 3, 32, 12, 9, 3, 2, 1, None, C.S32, C.F32, False, True, 0),
    "rgba_k7_f32": (3, 4, 96, 15, 15, 7, 2, 3, None, C.F32, C.S8, True, False, 0),
    "incep_p0_u8": (3, 3, 32, 15, 17, 3, 2, 0, None, C.U8, C.U8, False, True, 0),
    "same_u8": (3, 3, 32, 8, 7, 3, 2, 0, (4, 4), C.U8, C.U8, False, True, 0),
    "gray_k5_s8": (3, 1, 48, 9, 9, 5, 1, 2, None, C.S8, C.S32, False, False, 0),
    "alex_k11_u8": (2, 3, 7, 23, 27, 11, 4, 2, None, C.U8, C.UNDEF, False, False, 0),
}


def _run_check(outdir, shards=None):
    exe = os.path.join(TOOLS, "imgconv_check")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    env = {k: v for k, v in os.environ.items() if k != "DEEPFUSION_DEVICES"}
    if shards:
        env["DEEPFUSION_DEVICES"] = shards
    p = subprocess.run([exe, str(outdir)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0, p.stdout.decode()
    assert b"every dense twin identical to reorder() + conv() on the padded image" in p.stdout, p.stdout.decode()
    assert p.stdout.count(b": identical") == 6 and p.stdout.count(b"ran (no dense twin)") == 2, p.stdout.decode()


def test_cpp_layer_gives_the_reference_bytes_on_any_device_count(tmp_path):
    """imgconv_check through deepfusion::image_conv: its dumped results equal the numpy reference of its dumped inputs,
    and DEEPFUSION_DEVICES = 1, 2 and 3 give the same files"""
    dirs = {}
    for shards in ("1", "2", "3"):
        d = tmp_path / ("dev" + shards)
        d.mkdir()
        _run_check(d, shards=shards)
        dirs[shards] = d
    names = sorted(os.listdir(str(dirs["1"])))
    assert len([n for n in names if n.endswith("_dst.bin")]) == len(_LAYERS)
    for shards in ("2", "3"):
        assert names == sorted(os.listdir(str(dirs[shards])))
        for n in names:
            assert (dirs["1"] / n).read_bytes() == (dirs[shards] / n).read_bytes(), (shards, n)
    d = dirs["1"]
    for name, (bs, ic, oc, ih, iw, k, s, p, ohw, dst_dt, bia_dt, relu, pc, rm) in _LAYERS.items():
        case = R.ICase(name, bs, ic, ih, iw, oc, k=(k, k), stride=(s, s), pad=(p, p), out_hw=ohw, dst_dt=dst_dt,
                       bia_dt=bia_dt, relu=relu, rm=rm, per_channel=pc)
        data = dict(src=np.fromfile(str(d / (name + "_src.bin")), dtype=np.uint8).reshape(bs, ih, iw, ic),
                    w=np.fromfile(str(d / (name + "_wei.bin")), dtype=np.int8).reshape(oc, ic, k, k),
                    bia=None if bia_dt == C.UNDEF else np.fromfile(str(d / (name + "_bia.bin")), dtype=C.NP_OF[bia_dt]),
                    scales=np.fromfile(str(d / (name + "_scales.bin")), dtype=np.float32))
        assert data["scales"].size == (oc if pc else 1)
        got = np.fromfile(str(d / (name + "_dst.bin")), dtype=C.NP_OF[dst_dt]).reshape(bs, case.oh, case.ow, oc)
        hipref.assert_bit_equal(got, R.imgconv_ref(case, data), "imgconv_check " + name)


def test_bench_imgconv_runs():
    out = subprocess.check_output([os.path.join(TOOLS, "bench_imgconv"), "-shape", "2", "-burning_iter", "1", "-iter", "2", "-rounds", "3",
                                   "-rotate_mb", "48", "-cold_cache"], timeout=120)
    for want in (b"(a) imgconv, auto", b"(b) imgconv, generic path", b"(c) reorder 3->16 + conv", b"(d) conv on a padded tensor",
                 b"HBM floor", b"matrix floor", b"a/b", b"a/c", b"COLD"):
        assert want in out, out
