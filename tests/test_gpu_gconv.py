"""GPU: the grouped conv op (dfx_gconv_*, deepfusion::grouped_conv) against the numpy reference of tests/gconv_ref.py,
bit for bit (tests/test_gconv_cpu.py pins that reference against the C oracle's dense conv with block-diagonal
weights).  Everything goes through the C ABI; every output is written between guard bands; every case runs under both
requant routes (DFX_NO_FAST forces the exact one) and the route is asserted from requant()."""
import ctypes
import importlib
import os
import subprocess
from dataclasses import replace

import numpy as np
import pytest

import cases as C
import gconv_ref as R
import hipref

pytestmark = pytest.mark.gpu
dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "deep-fusion_amd", "tools")
BAND = 1 << 16       # guard bytes on each side of dst
EXACT, FAST = 0, 1


def make_op(case, data, force_path=-1):
    op = dfa.GroupConv((case.bs, case.ih, case.iw, case.c), case.oc, case.groups, case.k, stride=case.stride, pad=case.pad,
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
        ref = R.gconv_ref(case, data)
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
        return "gconv_mfma<3x3,s%d,cpg%d,%s> %s" % (case.stride[0], case.cpg, dt, "fast" if route == FAST else "exact")
    return "gconv_generic<%dx%d,s%dx%d,cpg%d,%s> exact" % (case.k + case.stride + (case.cpg, dt))


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
        assert name.endswith("fast" if route == FAST else "exact") and name == want_name(case, path, route), what
        hipref.assert_bit_equal(got, ref, what)
        names.add(name.split(" ")[0])
    return names


@pytest.mark.parametrize("cpg", R.MFMA_CPG)
@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_mfma_shapes(tuning, switch, cpg):
    """every geometry of the table (clipped windows, windows all padding, windows that hang over, images that end inside
    a strip, a row longer than a strip) with full and partial 128-channel chunks, for one cpg"""
    table = [c for c in R.mfma_table() if c.cpg == cpg]
    names = check_table(table, R.MFMA, switch, tuning)
    assert {n.split(",")[1] + "," + n.split(",")[2] for n in names} == {"s1,cpg%d" % cpg, "s2,cpg%d" % cpg}
    assert {n.split(",")[3] for n in names} == {"u8>", "s8>", "s32>", "f32>"}


@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_options_table(tuning, switch):
    check_table(R.options_table(), R.MFMA, switch, tuning)


@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_generic_path(tuning, switch):
    """ic != oc, other windows, mixed strides, cpg 1 / 2 / 3 / 12 / 24 / 80, groups = 1, c = 20: info.path asserted"""
    names = check_table(R.generic_table(), R.GENERIC, switch, tuning)
    assert all(n.startswith("gconv_generic<") for n in names)


@pytest.mark.parametrize("c,cpg", [(128, 4), (128, 64), (192, 64), (160, 16)])
def test_group_isolation_on_the_device(c, cpg):
    """the CPU test's inputs on the MFMA path: with the source non-zero only outside group g, group g's outputs are the
    bias alone -- a non-zero off-group byte in a packed tile would show"""
    for g in range(c // cpg):
        case, data, want = R.isolation_case(c, cpg, g)
        got, info, route = run(case, data)
        assert info.path == R.MFMA
        assert (got[..., g * cpg:(g + 1) * cpg] == want).all(), (g, info.kernel_name)
        hipref.assert_bit_equal(got, R.gconv_ref(case, data), "isolation group %d" % g)


@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_more_work_items_than_workgroups(tuning, switch):
    """DFX_GCONV_GRID caps the grid at one workgroup and at three: the workgroups loop over (chunk, slot) units and their
    waves over the strips.  c = 160 has a full and a partial chunk; three workgroups divide neither two chunks nor the
    strips."""
    for s in ((1, 1), (2, 2)):
        case = R.GCase("loop", 4, 160, 13, 37, 160, 20, stride=s, seed=17000, **R.OPTIONS[0])
        data, ref = reference(case)
        if switch:
            tuning.setenv(switch, "1")
        for grid in (1, 3):
            tuning.setenv("DFX_GCONV_GRID", grid)
            got, info, route = run(case, data)
            items = -(-case.bs * case.oh * case.ow // 32) * 2            # strips x chunks
            assert info.grid == grid and info.grid * (info.block // 64) < items, (info.grid, info.block, items)
            hipref.assert_bit_equal(got, ref, "%s grid %d [%s]" % (case.ident(), grid, info.kernel_name.decode()))


@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_lds_tile_variant_gives_the_same_bytes(tuning, switch):
    """DFX_GCONV_TILE=1 selects the variant of the MFMA kernel that stages its input as a halo tile in LDS (the A/B of
    DESIGN 4.9): every case of the MFMA and options tables (clipped bands and column blocks, windows all padding, windows
    that hang over, a 200-pixel row cut into column blocks of 64, partial chunks, cpg 64), and the grid capped at 1 and
    3 workgroups so that a workgroup loops over units and items"""
    tuning.setenv("DFX_GCONV_TILE", "1")
    if switch:
        tuning.setenv(switch, "1")
    for case in R.mfma_table() + R.options_table():
        data, ref = reference(case)
        got, info, route = run(case, data)
        name = info.kernel_name.decode()
        assert info.path == R.MFMA and name == want_name(case, R.MFMA, route).replace("gconv_mfma<", "gconv_mfma_tile<"), name
        assert route == want_route(case, switch, R.MFMA)
        hipref.assert_bit_equal(got, ref, "%s [%s] %s" % (case.ident(), name, switch))
    for s in ((1, 1), (2, 2)):
        case = R.GCase("loop", 4, 160, 13, 37, 160, 20, stride=s, seed=17000, **R.OPTIONS[0])
        data, ref = reference(case)
        for grid in (1, 3):
            tuning.setenv("DFX_GCONV_GRID", grid)
            got, info, route = run(case, data)
            assert info.grid == grid and info.kernel_name.decode().startswith("gconv_mfma_tile<")
            hipref.assert_bit_equal(got, ref, "%s tile grid %d" % (case.ident(), grid))


@pytest.mark.parametrize("c", [64, 128])
@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_defining_property_on_the_device(tuning, switch, c):
    """GroupConv == Conv with block-diagonal weights, compared on the device, 12 x 20, every dst type"""
    import torch
    if switch:
        tuning.setenv(switch, "1")
    for i, cpg in enumerate((4, 32, 64)):
        for s in (1, 2):
            for j, opt in enumerate(R.OPTIONS[:4]):
                case = R.GCase("twin", 2, c, 12, 20, c, c // cpg, stride=(s, s), seed=17200 + 100 * i + 10 * s + j, **opt)
                data = R.generate(case)
                got, info, route = run(case, data, on_device=True)
                assert info.path == R.MFMA
                conv = hipref.make_conv(R.dense_case(case), R.dense_data(case, data))
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


def test_nan_and_inf_scales_take_the_exact_route():
    """a NaN or an infinite scale must fail the fast route's proof; the bytes are the x86 ones: u8 255 / s8 -128"""
    for dst_dt, bad in ((C.U8, 255), (C.S8, -128)):
        case = R.GCase("nan", 2, 32, 6, 7, 32, 4, dst_dt=dst_dt, bia_dt=C.UNDEF, relu=False, per_channel=True, seed=17100)
        for poison in (np.nan, np.inf, -np.inf):
            data = R.generate(case)
            data["scales"][19] = poison
            data["src"][...] = np.maximum(data["src"], 1)
            data["w"][19] = np.abs(data["w"][19]) + 1
            ref = R.gconv_ref(case, data)
            got, info, route = run(case, data)
            assert info.path == R.MFMA and route == EXACT and info.kernel_name.decode().endswith("exact"), (poison, info.kernel_name)
            hipref.assert_bit_equal(got, ref, "%s scale %r" % (case.ident(), poison))
            if not (poison == -np.inf and dst_dt == C.U8):       # (-inf through the u8 ReLU is 0)
                assert (got[..., 19] == bad).all(), (poison, dst_dt)


def test_nan_and_inf_bias_take_the_exact_route():
    """an f32 bias that is NaN or infinite must fail the fast route's proof on its own clause (the scale is ordinary);
    the exact route then gives the x86 results"""
    for dst_dt, bad in ((C.U8, 255), (C.S8, -128)):
        case = R.GCase("nanbias", 2, 32, 6, 7, 32, 4, dst_dt=dst_dt, bia_dt=C.F32, relu=False, per_channel=True, seed=17150)
        for poison in (np.nan, np.inf, -np.inf):
            data = R.generate(case)
            data["bia"] = data["bia"].copy()
            data["bia"][21] = poison
            ref = R.gconv_ref(case, data)
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
        ref = R.gconv_ref(case, data)
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
    hipref.assert_bit_equal(got, R.gconv_ref(case, data), "forced exact")


def test_info_reports_the_launch_and_the_traffic():
    case = R.GCase("info", 2, 96, 13, 37, 96, 12, **R.OPTIONS[0])
    op = make_op(case, R.generate(case))
    try:
        i = op.info()
        px = 2 * 13 * 37
        assert i.path == R.MFMA and i.block == 512 and i.device >= 0
        assert i.grid == -(-(-(-px // 32)) // 8)                         # one chunk: ceil(strips / 8) workgroups
        assert i.lds_bytes == 3 * 9 * 1024 + 3 * 128 * 4 + 8 * 32 * 144, i.lds_bytes
        assert i.algorithmic_ops == 2 * 9 * 8 * px * 96 and i.algorithmic_bytes == px * 96 + 96 * 8 * 9 + px * 96
        assert i.kernel_name.decode() == "gconv_mfma<3x3,s1,cpg8,u8> fast"
    finally:
        op.close()
    case5 = R.GCase("info5", 2, 24, 13, 37, 36, 3, k=(5, 5), pad=(2, 2), stride=(2, 2), dst_dt=C.S32, bia_dt=C.S32, relu=False)
    op = make_op(case5, R.generate(case5))
    try:
        i = op.info()
        assert i.path == R.GENERIC and i.block == 256 and i.lds_bytes == 0
        assert i.kernel_name.decode() == "gconv_generic<5x5,s2x2,cpg8,s32> exact"
        assert i.algorithmic_ops == 2 * 25 * 8 * 2 * 7 * 19 * 36
        assert i.algorithmic_bytes == 2 * 13 * 37 * 24 + 36 * 8 * 25 + 2 * 7 * 19 * 36 * 4
    finally:
        op.close()
    # cpg 64: two input blocks per output block, twice the weight image (nothing is launched here)
    big = dfa.GroupConv((8, 7, 7, 256), 256, 4, (3, 3))
    try:
        i = big.info()
        assert i.lds_bytes == 4 * 18 * 1024 + 3 * 128 * 4 + 8 * 32 * 144 and i.grid == 2 * -(-(-(-8 * 49 // 32)) // 8), (i.lds_bytes, i.grid)
    finally:
        big.close()


@pytest.mark.parametrize("path", [R.MFMA, R.GENERIC])
def test_forced_paths_agree(path):
    case = R.GCase("forced", 2, 96, 9, 14, 96, 6, stride=(2, 2), dst_dt=C.S8, bia_dt=C.S8, relu=False, per_channel=True, seed=17300)
    data, ref = reference(case)
    got, info, route = run(case, data, force_path=path)
    assert info.path == path and (route == FAST) == (path == R.MFMA)
    hipref.assert_bit_equal(got, ref, "forced path %d" % path)


def test_set_weights_again_takes_effect():
    import torch
    case = R.GCase("reweigh", 2, 96, 9, 11, 96, 12, seed=17400, **R.OPTIONS[0])
    data = R.generate(case)
    data2 = dict(R.generate(replace(case, seed=77, wide=True)), src=data["src"])
    ref1, ref2 = R.gconv_ref(case, data), R.gconv_ref(case, data2)
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
    case = R.GCase("3streams", 2, 96, 40, 37, 96, 12, dst_dt=C.U8, bia_dt=C.S32, per_channel=True, seed=17500)
    data = R.generate(case)
    streams = [torch.cuda.Stream() for _ in range(3)]
    devs, refs = [], []
    for k in range(3):
        dk = dict(data, src=R.generate(replace(case, seed=300 + k))["src"])
        devs.append(torch.from_numpy(dk["src"]).cuda())
        refs.append(R.gconv_ref(case, dk))
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
    case = R.GCase("misal", 1, 32, 5, 7, 32, 4, bia_dt=C.UNDEF)
    data = R.generate(case)
    op = make_op(case, data)
    try:
        n = 35 * 32
        a = torch.zeros(n + 32, dtype=torch.uint8, device="cuda")
        dst = torch.full((n + 32,), 0x77, dtype=torch.uint8, device="cuda")
        L = capi.lib()
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for oa, od in ((8, 0), (0, 8), (1, 1), (4, 0), (0, 2)):
            rc = L.dfx_gconv_submit(op._h, ctypes.c_void_p(a.data_ptr() + oa), ctypes.c_void_p(dst.data_ptr() + od), st)
            assert rc == 1 and b"16-byte aligned" in L.dfx_last_error(), (oa, od, rc)
        assert L.dfx_gconv_submit(op._h, None, ctypes.c_void_p(dst.data_ptr()), st) == 1       # null src
        assert L.dfx_gconv_submit(op._h, ctypes.c_void_p(a.data_ptr()), None, st) == 1         # null dst
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
    op = dfa.GroupConv((1, 4, 4, 32), 32, 4, (3, 3))
    try:
        a = torch.zeros(16 * 32, dtype=torch.uint8, device="cuda")
        dst = torch.zeros(16 * 32, dtype=torch.uint8, device="cuda")
        with pytest.raises(dfa.DfxError) as e:
            op.submit(a, dst)
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
    case = R.GCase("stream", 2, 160, 20, 17, 160, 10, dst_dt=C.S32, bia_dt=C.S32, relu=False, per_channel=True, seed=17600)
    data, ref = reference(case)
    got, info, route = run(case, data, force_path=path, stream=torch.cuda.Stream())
    hipref.assert_bit_equal(got, ref, "non-default stream path %d" % path)
    op = make_op(case, data, path)
    try:
        hipref.assert_bit_equal(op.submit_host(data["src"]), ref, "submit_host path %d" % path)
        hipref.assert_bit_equal(op.submit_host(data["src"]), ref, "submit_host again path %d" % path)
    finally:
        op.close()


def test_resnext_layer():
    """N = 8, 56 x 56 x 128, 32 groups, 3x3 stride 1, u8 (ResNeXt-50's first stage): 784 strips on 98 workgroups, every
    byte against the reference on the device"""
    case = R.GCase("resnext", 8, 128, 56, 56, 128, 32, seed=17700, **R.OPTIONS[0])
    data = R.generate(case)
    ref = R.gconv_ref(case, data)
    got, info, route = run(case, data, on_device=True)
    assert info.path == R.MFMA and route == FAST and info.grid == 98, (info.kernel_name, info.grid)
    hipref.assert_dev_bit_equal(got, ref, "resnext layer [%s]" % info.kernel_name.decode())


# --- the C++ layer ------------------------------------------------------------------------------------------------------
_LAYERS = {  # gconv_check.cc's layers: name -> (bs, ic, oc, groups, ih, iw, k, s, p, out_hw, dst, bias, relu, per_channel, rm)
    "c128g32_u8": (3, 128, 128, 32, 9, 11, 3, 1, 1, None, C.U8, C.S32, False, False, 0),
    "c96g12s2_s8": (4, 96, 96, 12, 8, 7, 3, 2, 1, None, C.S8, C.UNDEF, True, True, 1),
    "c128g2_s32": (5, 128, 128, 2, 6, 9, 3, 1, 1, None, C.S32, C.F32, False, True, 0),
    "c64g2s2_f32": (3, 64, 64, 2, 9, 9, 3, 2, 1, None, C.F32, C.S8, True, False, 0),
    "same_u8": (3, 32, 32, 8, 8, 7, 3, 2, 0, (4, 4), C.U8, C.U8, False, True, 0),
    "ic24oc36_s8": (3, 24, 36, 3, 7, 5, 3, 1, 1, None, C.S8, C.S32, False, False, 0),
    "k5g4_u8": (2, 32, 64, 4, 9, 9, 5, 1, 2, None, C.U8, C.UNDEF, False, False, 0),
}


def _run_check(outdir, shards=None):
    exe = os.path.join(TOOLS, "gconv_check")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    env = {k: v for k, v in os.environ.items() if k != "DEEPFUSION_DEVICES"}
    if shards:
        env["DEEPFUSION_DEVICES"] = shards
    p = subprocess.run([exe, str(outdir)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0, p.stdout.decode()
    assert b"every dense twin identical to conv() on block-diagonal weights" in p.stdout, p.stdout.decode()
    assert p.stdout.count(b": identical") == 5 and p.stdout.count(b"ran (no dense twin)") == 2, p.stdout.decode()


def test_cpp_layer_gives_the_reference_bytes_on_any_device_count(tmp_path):
    """gconv_check through deepfusion::grouped_conv: its dumped results equal the numpy reference of its dumped inputs,
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
    for name, (bs, ic, oc, groups, ih, iw, k, s, p, ohw, dst_dt, bia_dt, relu, pc, rm) in _LAYERS.items():
        case = R.GCase(name, bs, ic, ih, iw, oc, groups, k=(k, k), stride=(s, s), pad=(p, p), out_hw=ohw, dst_dt=dst_dt,
                       bia_dt=bia_dt, relu=relu, rm=rm, per_channel=pc)
        data = dict(src=np.fromfile(str(d / (name + "_src.bin")), dtype=np.uint8).reshape(bs, ih, iw, ic),
                    w=np.fromfile(str(d / (name + "_wei.bin")), dtype=np.int8).reshape(oc, ic // groups, k, k),
                    bia=None if bia_dt == C.UNDEF else np.fromfile(str(d / (name + "_bia.bin")), dtype=C.NP_OF[bia_dt]),
                    scales=np.fromfile(str(d / (name + "_scales.bin")), dtype=np.float32))
        assert data["scales"].size == (oc if pc else 1)
        got = np.fromfile(str(d / (name + "_dst.bin")), dtype=C.NP_OF[dst_dt]).reshape(bs, case.oh, case.ow, oc)
        hipref.assert_bit_equal(got, R.gconv_ref(case, data), "gconv_check " + name)


def test_bench_gconv_runs():
    out = subprocess.check_output([os.path.join(TOOLS, "bench_gconv"), "-shape", "3", "-burning_iter", "2", "-iter", "3", "-rounds", "3",
                                   "-rotate_mb", "48", "-cold_cache"], timeout=120)
    assert b"(a) gconv" in out and b"(b) dense conv" in out and b"HBM floor" in out and b"a/b" in out and b"a/c" in out and b"COLD" in out and b"(t) gconv, input via LDS tile" in out and b"t/a" in out, out
