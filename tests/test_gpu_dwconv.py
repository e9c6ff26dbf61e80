"""GPU: the depthwise conv op (dfx_dwconv_*, deepfusion::depthwise_conv) against the numpy reference of
tests/dwconv_ref.py, bit for bit (tests/test_dwconv_cpu.py pins that reference against the C oracle's dense conv with
block-diagonal weights).  Everything goes through the C ABI; every output is written between guard bands; every case
runs under both requant routes (DFX_NO_FAST forces the exact one) and the route is asserted from requant()."""
import ctypes
import importlib
import os
import subprocess
from dataclasses import replace

import numpy as np
import pytest

import cases as C
import dwconv_ref as R
import hipref

pytestmark = pytest.mark.gpu
dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "deep-fusion_amd", "tools")
BAND = 1 << 16       # guard bytes on each side of dst
EXACT, FAST = 0, 1


def make_op(case, data, force_path=-1):
    op = dfa.DwConv((case.bs, case.ih, case.iw, case.c), case.k, stride=case.stride, pad=case.pad, out_hw=(case.oh, case.ow),
                    dst_dt=case.dst_dt, bia_dt=case.bia_dt, relu=case.relu, rm=case.rm, nscales=data["scales"].size,
                    force_path=force_path)
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


def run(case, data, force_path=-1, stream=None, on_device=False):
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
        ref = R.dw_ref(case, data)
        ref.setflags(write=False)
        _REF[case] = (data, ref)
    return _REF[case]


def want_route(case, switch, path):
    """what set_weights must prove for reference-range and "wide" data: fast on the window kernel with nearest
    rounding (everything is finite and far below 2^30), exact otherwise"""
    return FAST if (path == R.WINDOW and case.rm == 0 and not switch) else EXACT


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
        assert name.endswith("fast" if route == FAST else "exact"), what
        hipref.assert_bit_equal(got, ref, what)
        names.add(name.split(" ")[0])
    return names


@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_window_shapes(tuning, switch):
    """3x3 and 5x5, stride 1 and 2, every image size of the table with c = 16, 48, 144: clipped windows, windows that
    hang over, rows longer than a wave, channel groups that do not divide the launch, 5x5 beyond 64 groups"""
    names = check_table(R.window_table(), R.WINDOW, switch, tuning)
    assert {n.split(",")[0] + "," + n.split(",")[1] for n in names} == {"dwconv_window<3x3,s1", "dwconv_window<3x3,s2",
                                                                         "dwconv_window<5x5,s1", "dwconv_window<5x5,s2"}


@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_options_table(tuning, switch):
    check_table(R.options_table(), R.WINDOW, switch, tuning)


@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_generic_path(tuning, switch):
    """mixed strides, 7x7 / 1x3 / 3x1 windows, channel counts that are no multiple of 16: info.path asserted"""
    names = check_table(R.generic_table(), R.GENERIC, switch, tuning)
    assert all(n.startswith("dwconv_generic<") for n in names)


@pytest.mark.parametrize("band", [1, 8, 16])
def test_every_band_height(tuning, band):
    """the band (output rows per lane) is chosen from the tensor's size; the table's small tensors all get 4.  Other
    heights, forced: 1 (every row a band of its own), 8 and 16 (the last band partial, or the only one)"""
    tuning.setenv("DFX_DWCONV_BAND", band)
    for case in R.window_table():
        if case.ih < 7:
            continue
        data, ref = reference(case)
        got, info, route = run(case, data)
        assert (" band %d " % band) in info.kernel_name.decode(), info.kernel_name
        hipref.assert_bit_equal(got, ref, "%s [%s]" % (case.ident(), info.kernel_name.decode()))


@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_more_work_items_than_lanes(tuning, switch):
    """The kernel's outer loop iterates when a launch has fewer lanes than work items (info.grid x info.block against
    bs * bands * ow * c / 16).  The launch is sized from the device (4 workgroups per CU) and the band grows with the
    tensor, so the smallest tensor at which that happens by itself has 2^26 outputs: that one is
    test_more_work_items_than_lanes_uncapped, against the dense conv on the device.  Here DFX_DWCONV_GRID caps the grid
    (as DFX_STREAM_GRID does for the streamed conv kernel), at one workgroup and at three, so that the loop also runs
    against the numpy reference, under both routes, on 5x5, and with a step the uncapped launch cannot have: with
    c = 144 the 9 channel groups divide neither launch, so some lanes idle and a lane's step is not a multiple of a row."""
    for k, s, p in (((3, 3), (1, 1), (1, 1)), ((5, 5), (2, 2), (2, 2))):
        case = R.DwCase("loop", 4, 144, 13, 37, k=k, stride=s, pad=p, seed=6000, **R.OPTIONS[0])
        data, ref = reference(case)
        if switch:
            tuning.setenv(switch, "1")
        for grid in (1, 3):
            tuning.setenv("DFX_DWCONV_GRID", grid)
            got, info, route = run(case, data)
            bands = -(-case.oh // 4)
            items = case.bs * bands * case.ow * (case.c // 16)
            assert info.grid == grid and info.grid * info.block < items, (info.grid, info.block, items)
            hipref.assert_bit_equal(got, ref, "%s grid %d [%s]" % (case.ident(), grid, info.kernel_name.decode()))


def test_nan_and_inf_scales_take_the_exact_route():
    """a NaN or an infinite scale must fail the fast route's proof; the bytes are the x86 ones: u8 255 / s8 -128"""
    for dst_dt, bad in ((C.U8, 255), (C.S8, -128)):
        for k in ((3, 3), (5, 5)):
            case = R.DwCase("nan", 2, 32, 6, 7, k=k, pad=(k[0] // 2, k[1] // 2), dst_dt=dst_dt, bia_dt=C.UNDEF, relu=False,
                            per_channel=True, seed=6100)
            for poison in (np.nan, np.inf, -np.inf):
                data = R.generate(case)
                data["scales"][19] = poison
                data["src"][...] = np.maximum(data["src"], 1)
                data["w"][19] = np.abs(data["w"][19]) + 1
                ref = R.dw_ref(case, data)
                got, info, route = run(case, data)
                assert route == EXACT and info.kernel_name.decode().endswith("exact"), (poison, info.kernel_name)
                hipref.assert_bit_equal(got, ref, "%s scale %r" % (case.ident(), poison))
                if not (poison == -np.inf and dst_dt == C.U8):       # (-inf through the u8 ReLU is 0)
                    assert (got[..., 19] == bad).all(), (poison, dst_dt)


def test_more_work_items_than_lanes_uncapped():
    """The same, with nothing capped: the launch has at most 4 workgroups of 256 lanes per CU and the band is 16 rows
    once a tensor fills it, so 3x3 stride 1 on 256 x 256 x 16 (16 bands x 256 columns x 1 group = 4096 work items per
    image) needs one image more than lanes / 4096 -- 65 images on 256 CUs, 2^26 outputs.  Too large for the numpy
    reference: every byte is compared, on the device, with the dense conv with diagonal weights (the defining
    property), and the first and the last image with the reference as well."""
    import torch
    lanes = torch.cuda.get_device_properties(0).multi_processor_count * 4 * 256
    bs = lanes // 4096 + 1
    case = R.DwCase("uncapped", bs, 16, 256, 256, seed=6050, **R.OPTIONS[0])
    small = R.generate(replace(case, bs=1))
    g = torch.Generator(device="cuda").manual_seed(6051)
    src = torch.randint(0, 17, (bs, 256, 256, 16), dtype=torch.uint8, device="cuda", generator=g)
    op = make_op(case, small)
    conv = hipref.make_conv(R.dense_case(case), R.dense_data(dict(small, src=np.broadcast_to(np.uint8(0), tuple(src.shape)))))
    try:
        info = op.info()
        name = info.kernel_name.decode()
        assert info.path == R.WINDOW and op.requant() == FAST and " band 16 " in name, name
        items = bs * 16 * 256
        assert (bs - 1) * 16 * 256 <= info.grid * info.block < items, (info.grid, info.block, items)
        buf, dst = guarded_dst(op, case)
        want = torch.empty(conv.dst_shape, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        op.submit(src, dst)
        conv.submit(src, want)
        torch.cuda.synchronize()
        hipref.assert_guards(buf, BAND, name)
        assert torch.equal(dst, want), "%s differs from %s" % (name, conv.info().kernel_name.decode())
        for n in (0, bs - 1):
            ref = R.dw_ref(replace(case, bs=1), dict(small, src=src[n:n + 1].cpu().numpy()))
            hipref.assert_bit_equal(dst[n:n + 1].cpu().numpy(), ref, "image %d [%s]" % (n, name))
    finally:
        op.close()
        conv.close()


def test_nan_and_inf_bias_take_the_exact_route():
    """an f32 bias that is NaN or infinite must fail the fast route's proof on its own clause (the scale is ordinary);
    the exact route then gives the x86 results: NaN and +inf -> 0x80000000 -> u8 255 / s8 -128, -inf likewise for s8
    and 0 through the u8 ReLU"""
    for dst_dt, bad in ((C.U8, 255), (C.S8, -128)):
        for k in ((3, 3), (5, 5)):
            case = R.DwCase("nanbias", 2, 32, 6, 7, k=k, pad=(k[0] // 2, k[1] // 2), dst_dt=dst_dt, bia_dt=C.F32, relu=False,
                            per_channel=True, seed=6150)
            for poison in (np.nan, np.inf, -np.inf):
                data = R.generate(case)
                data["bia"] = data["bia"].copy()
                data["bia"][21] = poison
                ref = R.dw_ref(case, data)
                got, info, route = run(case, data)
                assert info.path == R.WINDOW and route == EXACT and info.kernel_name.decode().endswith("exact"), (poison, info.kernel_name)
                hipref.assert_bit_equal(got, ref, "%s bias %r" % (case.ident(), poison))
                assert (got[..., 21] == (0 if (poison == -np.inf and dst_dt == C.U8) else bad)).all(), (poison, dst_dt)
                # the same numbers with that one bias finite are proven fast: the clause alone decided
                data["bia"][21] = 1.0
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
        ref = R.dw_ref(case, data)
        got, info, route = run(case, data)
        assert route == (FAST if edge.fast else EXACT), (edge.name, dst_dt, info.kernel_name)
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
    hipref.assert_bit_equal(got, R.dw_ref(case, data), "forced exact")


@pytest.mark.parametrize("c", [32, 64])
@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_defining_property_on_the_device(tuning, switch, c):
    """DwConv == Conv with block-diagonal weights, compared on the device, 12 x 20, every dst type"""
    import torch
    if switch:
        tuning.setenv(switch, "1")
    for i, geom in enumerate((dict(), dict(stride=(2, 2)), dict(k=(5, 5), pad=(2, 2)))):
        for j, opt in enumerate(R.OPTIONS[:4]):
            case = R.DwCase("twin", 2, c, 12, 20, seed=6200 + 10 * i + j, **geom, **opt)
            data = R.generate(case)
            got, info, route = run(case, data, on_device=True)
            conv = hipref.make_conv(R.dense_case(case), R.dense_data(data))
            try:
                src = torch.from_numpy(data["src"]).cuda()
                want = torch.empty(conv.dst_shape, dtype=hipref.torch_dtype(case.dst_dt), device="cuda")
                conv.submit(src, want)
                torch.cuda.synchronize()
                cname = conv.info().kernel_name.decode()
            finally:
                conv.close()
            assert tuple(got.shape) == tuple(want.shape)
            same = torch.equal(got.view(torch.uint8), want.view(torch.uint8))
            assert same, "%s: %s differs from %s" % (case.ident(), info.kernel_name.decode(), cname)


def test_info_reports_the_launch_and_the_traffic():
    case = R.DwCase("info", 2, 48, 13, 37, **R.OPTIONS[0])
    data = R.generate(case)
    op = make_op(case, data)
    try:
        i = op.info()
        outs = 2 * 13 * 37 * 48
        assert i.path == R.WINDOW and i.block == 256 and i.grid >= 1 and i.lds_bytes == 0 and i.device >= 0
        assert i.algorithmic_ops == 2 * 9 * outs and i.algorithmic_bytes == outs + 48 * 9 + outs
        assert i.kernel_name.decode() == "dwconv_window<3x3,s1,u8> band 4 fast"
    finally:
        op.close()
    case5 = replace(case, k=(5, 5), pad=(2, 2), stride=(2, 2), dst_dt=C.S32)
    op = make_op(case5, R.generate(case5), force_path=R.GENERIC)
    try:
        i = op.info()
        assert i.path == R.GENERIC and i.kernel_name.decode() == "dwconv_generic<5x5,s2x2,s32> exact"
        assert i.algorithmic_bytes == 2 * 13 * 37 * 48 + 48 * 25 + 2 * 7 * 19 * 48 * 4
    finally:
        op.close()
    op = make_op(case5, R.generate(case5))
    try:
        i = op.info()
        assert i.path == R.WINDOW and i.lds_bytes == 53 * 3 * 16, i.lds_bytes
    finally:
        op.close()
    # the band grows with the tensor: N = 128, 56 x 56 x 128 gives every lane of the launch a work item at 8 rows
    # (nothing is launched here)
    big = dfa.DwConv((128, 56, 56, 128), (3, 3))
    try:
        i = big.info()
        assert " band 8 " in i.kernel_name.decode() and i.grid * i.block <= 128 * 7 * 56 * 8, (i.kernel_name, i.grid)
    finally:
        big.close()


@pytest.mark.parametrize("path", [R.WINDOW, R.GENERIC])
def test_forced_paths_agree(path):
    case = R.DwCase("forced", 2, 48, 9, 14, stride=(2, 2), dst_dt=C.S8, bia_dt=C.S8, relu=False, per_channel=True, seed=6300)
    data, ref = reference(case)
    got, info, route = run(case, data, force_path=path)
    assert info.path == path
    hipref.assert_bit_equal(got, ref, "forced path %d" % path)


def test_set_weights_again_takes_effect():
    import torch
    case = R.DwCase("reweigh", 2, 48, 9, 11, seed=6400, **R.OPTIONS[0])
    data = R.generate(case)
    data2 = dict(R.generate(replace(case, seed=77, wide=True)), src=data["src"])
    ref1, ref2 = R.dw_ref(case, data), R.dw_ref(case, data2)
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
    finally:
        op.close()


@pytest.mark.parametrize("path", [R.WINDOW, R.GENERIC])
def test_one_handle_on_three_streams(path):
    """different inputs per stream, 20 submits each, interleaved: every launch has its own copy of the arguments"""
    import torch
    case = R.DwCase("3streams", 2, 48, 40, 37, dst_dt=C.U8, bia_dt=C.S32, per_channel=True, seed=6500)
    data = R.generate(case)
    streams = [torch.cuda.Stream() for _ in range(3)]
    devs, refs = [], []
    for k in range(3):
        dk = dict(data, src=R.generate(replace(case, seed=300 + k))["src"])
        devs.append(torch.from_numpy(dk["src"]).cuda())
        refs.append(R.dw_ref(case, dk))
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


def test_misaligned_pointers_are_refused_and_nothing_is_launched():
    import torch
    case = R.DwCase("misal", 1, 32, 5, 7, bia_dt=C.UNDEF)
    data = R.generate(case)
    op = make_op(case, data)
    try:
        n = 35 * 32
        a = torch.zeros(n + 32, dtype=torch.uint8, device="cuda")
        dst = torch.full((n + 32,), 0x77, dtype=torch.uint8, device="cuda")
        L = capi.lib()
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for oa, od in ((8, 0), (0, 8), (1, 1), (4, 0), (0, 2)):
            rc = L.dfx_dwconv_submit(op._h, ctypes.c_void_p(a.data_ptr() + oa), ctypes.c_void_p(dst.data_ptr() + od), st)
            assert rc == 1 and b"16-byte aligned" in L.dfx_last_error(), (oa, od, rc)
        assert L.dfx_dwconv_submit(op._h, None, ctypes.c_void_p(dst.data_ptr()), st) == 1       # null src
        assert L.dfx_dwconv_submit(op._h, ctypes.c_void_p(a.data_ptr()), None, st) == 1         # null dst
        with pytest.raises(dfa.DfxError):
            op.submit(a.data_ptr() + 8, dst)
        torch.cuda.synchronize()
        assert bool((dst == 0x77).all()), "a refused submit wrote to dst"
        op.submit(a, dst)                            # the aligned call goes through
        torch.cuda.synchronize()
        assert bool((dst[n:] == 0x77).all()) and not bool((dst[:n] == 0x77).all())
    finally:
        op.close()


def test_submit_before_set_weights_is_a_state_error():
    import torch
    op = dfa.DwConv((1, 4, 4, 32), (3, 3))
    try:
        a = torch.zeros(16 * 32, dtype=torch.uint8, device="cuda")
        dst = torch.zeros(16 * 32, dtype=torch.uint8, device="cuda")
        with pytest.raises(dfa.DfxError) as e:
            op.submit(a, dst)
        assert "dfx error 5" in str(e.value)
        with pytest.raises(dfa.DfxError) as e:
            op.requant()
        assert "dfx error 5" in str(e.value)
    finally:
        op.close()


@pytest.mark.parametrize("path", [R.WINDOW, R.GENERIC])
def test_non_default_stream_and_submit_host(path):
    import torch
    case = R.DwCase("stream", 2, 48, 20, 17, k=(5, 5), pad=(2, 2), dst_dt=C.S32, bia_dt=C.S32, relu=False, per_channel=True, seed=6600)
    data, ref = reference(case)
    got, info, route = run(case, data, force_path=path, stream=torch.cuda.Stream())
    hipref.assert_bit_equal(got, ref, "non-default stream path %d" % path)
    op = make_op(case, data, path)
    try:
        hipref.assert_bit_equal(op.submit_host(data["src"]), ref, "submit_host path %d" % path)
        hipref.assert_bit_equal(op.submit_host(data["src"]), ref, "submit_host again path %d" % path)
    finally:
        op.close()


def test_mobilenet_layer():
    """N = 16, 56 x 56 x 128, 3x3 stride 1, u8: more waves than the chip holds at once, every byte against the
    reference on the device"""
    case = R.DwCase("mbv1", 16, 128, 56, 56, seed=6700, **R.OPTIONS[0])
    data = R.generate(case)
    ref = R.dw_ref(case, data)
    got, info, route = run(case, data, on_device=True)
    assert info.path == R.WINDOW and route == FAST, info.kernel_name
    hipref.assert_dev_bit_equal(got, ref, "mobilenet layer [%s]" % info.kernel_name.decode())


# --- the C++ layer ------------------------------------------------------------------------------------------------------
_LAYERS = {  # dwconv_check.cc's layers: name -> (bs, c, ih, iw, k, s, p, out_hw, dst, bias, relu, per_channel, rm)
    "k3s1_u8": (3, 32, 9, 11, 3, 1, 1, None, C.U8, C.S32, False, False, 0),
    "k3s2_s8": (4, 48, 8, 7, 3, 2, 1, None, C.S8, C.UNDEF, True, True, 1),
    "k5s1_s32": (5, 16, 6, 9, 5, 1, 2, None, C.S32, C.F32, False, True, 0),
    "k5s2_f32": (3, 64, 9, 9, 5, 2, 2, None, C.F32, C.S8, True, False, 0),
    "same_u8": (3, 32, 8, 7, 3, 2, 0, (4, 4), C.U8, C.U8, False, True, 0),
    "c24_s8": (3, 24, 7, 5, 3, 1, 1, None, C.S8, C.S32, False, False, 0),
    "k7_u8": (2, 16, 9, 9, 7, 1, 3, None, C.U8, C.UNDEF, False, False, 0),
}


def _run_check(outdir, shards=None):
    exe = os.path.join(TOOLS, "dwconv_check")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    env = {k: v for k, v in os.environ.items() if k != "DEEPFUSION_DEVICES"}
    if shards:
        env["DEEPFUSION_DEVICES"] = shards
    p = subprocess.run([exe, str(outdir)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode()
    assert b"every dense twin identical to conv() on diagonal weights" in p.stdout, p.stdout.decode()


def test_cpp_layer_gives_the_reference_bytes_on_any_device_count(tmp_path):
    """dwconv_check through deepfusion::depthwise_conv: its dumped results equal the numpy reference of its dumped
    inputs, and DEEPFUSION_DEVICES = 1, 2 and 3 give the same files"""
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
    for name, (bs, c, ih, iw, k, s, p, ohw, dst_dt, bia_dt, relu, pc, rm) in _LAYERS.items():
        case = R.DwCase(name, bs, c, ih, iw, k=(k, k), stride=(s, s), pad=(p, p), out_hw=ohw, dst_dt=dst_dt, bia_dt=bia_dt,
                        relu=relu, rm=rm, per_channel=pc)
        data = dict(src=np.fromfile(str(d / (name + "_src.bin")), dtype=np.uint8).reshape(bs, ih, iw, c),
                    w=np.fromfile(str(d / (name + "_wei.bin")), dtype=np.int8).reshape(c, k, k),
                    bia=None if bia_dt == C.UNDEF else np.fromfile(str(d / (name + "_bia.bin")), dtype=C.NP_OF[bia_dt]),
                    scales=np.fromfile(str(d / (name + "_scales.bin")), dtype=np.float32))
        assert data["scales"].size == (c if pc else 1)
        got = np.fromfile(str(d / (name + "_dst.bin")), dtype=C.NP_OF[dst_dt]).reshape(bs, case.oh, case.ow, c)
        hipref.assert_bit_equal(got, R.dw_ref(case, data), "dwconv_check " + name)


def test_bench_dwconv_runs():
    out = subprocess.check_output([os.path.join(TOOLS, "bench_dwconv"), "-shape", "5", "-burning_iter", "2", "-iter", "3", "-rounds", "3",
                                   "-rotate_mb", "48", "-cold_cache"])
    assert b"(a) dwconv" in out and b"(b) max pooling" in out and b"HBM floor" in out and b"a/b" in out and b"COLD" in out, out
