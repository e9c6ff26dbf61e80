"""GPU: the fully-connected op (dfx_fc_*, deepfusion::inner_product) against the numpy reference of tests/fc_ref.py, bit
for bit (tests/test_fc_cpu.py pins that reference against the C oracle's dense conv with the full-image window).
Everything goes through the C ABI; every output is written between guard bands; path, splitk, route and kernel name are
asserted from info() / requant(); the table cases run under both requant routes (DFX_NO_FAST forces the exact one)."""
import importlib
import os
import subprocess
from dataclasses import replace

import numpy as np
import pytest

import cases as C
import fc_ref as R
import hipref

pytestmark = pytest.mark.gpu
dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "deep-fusion_amd", "tools")
BAND = 1 << 16       # guard bytes on each side of dst
EXACT, FAST = 0, 1


def cus():
    import torch
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def make_op(case, data, force_path=-1):
    op = dfa.InnerProduct((case.bs, case.ih, case.iw, case.ic), case.oc, dst_dt=case.dst_dt, bia_dt=case.bia_dt, relu=case.relu,
                          rm=case.rm, nscales=data["scales"].size, force_path=force_path)
    op.set_weights(data["w"], data["scales"], bia=data["bia"])
    return op


def guarded_dst(op, case):
    """-> (buf, dst): dst (poisoned with 0xCD) sits between two BAND-byte bands of 0xA5 inside one allocation"""
    import torch
    nbytes = int(np.prod(op.dst_shape)) * np.dtype(C.NP_OF[case.dst_dt]).itemsize
    buf = torch.empty(BAND + nbytes + BAND, dtype=torch.uint8, device="cuda")      # (the band behind starts at dst's last byte)
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
        ref = R.fc_ref(case, data)
        ref.setflags(write=False)
        _REF[case] = (data, ref)
    return _REF[case]


def want_route(case, switch, path):
    """what set_weights must prove for reference-range and "wide" data: fast on the MFMA path with nearest rounding
    (everything is finite and far below 2^30), exact otherwise"""
    return FAST if (path == R.MFMA and case.rm == 0 and not switch) else EXACT


def want_name(case, path, route, splitk):
    dt = C.NAME_OF[case.dst_dt]
    if path == R.MFMA:
        return "fc_mfma<k%d,%s,sk%d> %s" % (case.K, dt, splitk, "fast" if route == FAST else "exact")
    return "fc_generic<%s> exact" % dt


def check(case, path, switch, forced_splitk=None, force_path=-1, grid=None):
    data, ref = reference(case)
    got, info, route = run(case, data, force_path=force_path)
    name = info.kernel_name.decode()
    what = "%s [%s] %s" % (case.ident(), name, switch)
    assert info.path == path, what
    splitk = R.planned_splitk(case, cus(), forced_splitk) if path == R.MFMA else 1
    assert info.splitk == splitk, (what, info.splitk, splitk)
    assert route == want_route(case, switch, path), what
    assert name == want_name(case, path, route, splitk), what
    if grid is not None:
        assert info.grid == grid, (what, info.grid)
    hipref.assert_bit_equal(got, ref, what)
    return info


@pytest.mark.parametrize("shape", R.MFMA_SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_mfma_shapes(tuning, switch, shape):
    """bs in {1, 2, 31, 32, 33, 130} x oc in {1, 10, 32, 33, 96, 130} for one (ih, iw, ic): partial column blocks, a
    second batch chunk with a partial tail, partial oc blocks, rows that are not 4-byte aligned; the options rotate"""
    if switch:
        tuning.setenv(switch, "1")
    table = [c for c in R.mfma_table() if (c.ih, c.iw, c.ic) == shape]
    assert len(table) == 36
    for case in table:
        info = check(case, R.MFMA, switch)
        assert info.block == 256 and info.lds_bytes == 512 * min(128, -(-case.bs // 32) * 32)


@pytest.mark.parametrize("grid", [None, 1])
@pytest.mark.parametrize("splitk", R.SPLITK_VALUES)
def test_every_splitk_gives_the_same_bits(tuning, splitk, grid):
    """DFX_FC_SPLITK in {1, 2, 3, 7, 64} on 7 and 49 k-steps: uneven slices, one step per slice, a clamp; with
    DFX_FC_GRID=1 one workgroup loops over all units.  The sum of the slices is an integer sum."""
    tuning.setenv("DFX_FC_SPLITK", splitk)
    if grid:
        tuning.setenv("DFX_FC_GRID", grid)
    for case in R.splitk_table():
        info = check(case, R.MFMA, None, forced_splitk=splitk, grid=grid)
        assert info.splitk == min(splitk, case.K // 64)
        units = -(-(-(-case.oc // 32)) // 4) * info.splitk * -(-case.bs // 128)
        assert info.grid == (1 if grid else units)


@pytest.mark.parametrize("forced", [1, None])
def test_accumulator_bounds(tuning, forced):
    """K = 65024: channel 0 all 127 / channel 1 all -128 against an image of 255s: 255 * 127 * 65024 and
    -255 * 128 * 65024 come out of the s32 accumulator, at splitk 1 and at the planner's own value"""
    if forced:
        tuning.setenv("DFX_FC_SPLITK", forced)
    case, data = R.bounds_case()
    data, ref = reference(case, data)
    got, info, route = run(case, data)
    assert info.path == R.MFMA and info.splitk == R.planned_splitk(case, cus(), forced), info.splitk
    assert forced or info.splitk > 1
    assert int(got[0, 0]) == 255 * 127 * 65024 == int(ref[0, 0]) and int(got[0, 1]) == -255 * 128 * 65024 == int(ref[0, 1])
    hipref.assert_bit_equal(got, ref, "bounds [%s]" % info.kernel_name.decode())


@pytest.mark.parametrize("edge", R.FC_EDGES, ids=lambda e: e.name)
def test_fast_route_proof_edges(tuning, edge):
    """(255 * max(P, N) + |bias|) * |scale| exactly 2^30 is admitted (fast), the next f32 scale above is rejected
    (exact), with the bound attained by the data: the route and the bytes, every dst type"""
    for dst_dt in (C.S32, C.U8, C.S8, C.F32):
        case, data = R.edge_case(edge, dst_dt)
        ref = R.fc_ref(case, data)
        got, info, route = run(case, data)
        assert info.path == R.MFMA and route == (FAST if edge.fast else EXACT), (edge.name, dst_dt, info.kernel_name)
        assert info.kernel_name.decode().endswith("fast" if edge.fast else "exact")
        hipref.assert_bit_equal(got, ref, "%s %s" % (edge.name, info.kernel_name.decode()))
    # the bound is attained: the accumulator itself (s32 dst, scale 1, no bias) on the device
    case, data = R.edge_case(edge, C.S32)
    neutral = dict(data, bia=None, scales=np.ones(1, dtype=np.float32))
    got, info, route = run(replace(case, bia_dt=C.UNDEF, per_channel=False), neutral)
    acc, bound, P, N = R.edge_attained(edge, case, data)
    assert int(got[0 if edge.which == "max" else 1, R.EDGE_CHANNEL]) == bound == acc
    # round-down and DFX_NO_FAST reject whatever the numbers are
    case, data = R.edge_case(R.FC_EDGES[0], C.U8)
    got, info, route = run(replace(case, rm=1), data)
    assert route == EXACT
    tuning.setenv("DFX_NO_FAST", "1")
    got, info, route = run(case, data)
    assert route == EXACT
    hipref.assert_bit_equal(got, R.fc_ref(case, data), "forced exact")


def test_nan_and_inf_scales_take_the_exact_route():
    """a NaN or an infinite scale must fail the fast route's proof; the bytes are the x86 ones: u8 255 / s8 -128"""
    for dst_dt, bad in ((C.U8, 255), (C.S8, -128)):
        case = R.FcCase("nan", 3, 64, 1, 1, 33, dst_dt=dst_dt, bia_dt=C.UNDEF, relu=False, per_channel=True, seed=27100)
        for poison in (np.nan, np.inf, -np.inf):
            data = R.generate(case)
            data["scales"][19] = poison
            data["src"][...] = np.maximum(data["src"], 1)
            data["w"][19] = np.abs(data["w"][19]) + 1
            ref = R.fc_ref(case, data)
            got, info, route = run(case, data)
            assert info.path == R.MFMA and route == EXACT and info.kernel_name.decode().endswith("exact"), (poison, info.kernel_name)
            hipref.assert_bit_equal(got, ref, "%s scale %r" % (case.ident(), poison))
            if not (poison == -np.inf and dst_dt == C.U8):       # (-inf through the u8 ReLU is 0)
                assert (got[:, 19] == bad).all(), (poison, dst_dt)


@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_generic_path(tuning, switch):
    """K = 100, 5 x 5 x 3 and K = 17 with oc in {7, 16}: auto takes the generic kernel, exact only"""
    if switch:
        tuning.setenv(switch, "1")
    for case in R.generic_table():
        info = check(case, R.GENERIC, switch)
        assert info.block == 256 and info.lds_bytes == 0


@pytest.mark.parametrize("i", range(4))
def test_forced_generic_equals_mfma(i):
    """one MFMA-class shape on both paths: the same bytes (and the reference's)"""
    case = R.FcCase("forced", 33, 64, 1, 3, 33, seed=27300 + i, **R.OPTIONS[(5 * i + 1) % len(R.OPTIONS)])
    data, ref = reference(case)
    a, ia, ra = run(case, data, force_path=R.MFMA)
    b, ib, rb = run(case, data, force_path=R.GENERIC)
    assert ia.path == R.MFMA and ib.path == R.GENERIC and rb == EXACT and ra == (FAST if case.rm == 0 else EXACT)
    assert ib.kernel_name.decode() == "fc_generic<%s> exact" % C.NAME_OF[case.dst_dt]
    hipref.assert_bit_equal(a, b, "generic against mfma, %s" % case.ident())
    hipref.assert_bit_equal(a, ref, "mfma against the reference, %s" % case.ident())


@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_conv_equivalence_on_the_device(tuning, switch):
    """InnerProduct == Conv with the full-image window (stride 1, no padding, oh = ow = 1), compared on the device:
    (1,1,256) -> 64, (3,3,32) -> 48 and (7,7,64) -> 32, every dst type"""
    import torch
    if switch:
        tuning.setenv(switch, "1")
    for case in R.twin_table():
        data, ref = reference(case)
        got, info, route = run(case, data, on_device=True)
        assert info.path == (R.MFMA if case.mfma_class else R.GENERIC)
        conv = hipref.make_conv(R.dense_case(case), R.dense_data(case, data))
        try:
            src = torch.from_numpy(data["src"]).cuda()
            want = torch.empty(conv.dst_shape, dtype=hipref.torch_dtype(case.dst_dt), device="cuda")
            conv.submit(src, want)
            torch.cuda.synchronize()
            cname = conv.info().kernel_name.decode()
        finally:
            conv.close()
        assert tuple(want.shape) == (case.bs, 1, 1, case.oc)
        same = torch.equal(got.contiguous().view(torch.uint8), want.view(case.bs, case.oc).contiguous().view(torch.uint8))
        assert same, "%s: %s differs from %s" % (case.ident(), info.kernel_name.decode(), cname)
        hipref.assert_dev_bit_equal(got, ref, case.ident())


def test_info_reports_the_launch_and_the_traffic():
    case = R.FcCase("info", 33, 64, 7, 7, 130, **R.OPTIONS[0])
    op = make_op(case, R.generate(case))
    try:
        i = op.info()
        sk = R.planned_splitk(case, cus())
        assert i.path == R.MFMA and i.block == 256 and i.device >= 0 and i.splitk == sk == min(cus() // 2, 7)
        assert i.grid == 2 * sk                                      # 5 oc blocks: two groups of four
        assert i.lds_bytes == 64 * 512
        assert i.algorithmic_ops == 2 * 33 * 3136 * 130 and i.algorithmic_bytes == 33 * 3136 + 130 * 3136 + 33 * 130
        assert i.kernel_name.decode() == "fc_mfma<k3136,u8,sk%d> fast" % sk
    finally:
        op.close()
    case = R.FcCase("info-g", 5, 3, 5, 5, 7, dst_dt=C.S32, bia_dt=C.S32, relu=False)
    op = make_op(case, R.generate(case))
    try:
        i = op.info()
        assert i.path == R.GENERIC and i.block == 256 and i.lds_bytes == 0 and i.splitk == 1 and i.grid == 1
        assert i.kernel_name.decode() == "fc_generic<s32> exact"
        assert i.algorithmic_ops == 2 * 5 * 75 * 7 and i.algorithmic_bytes == 5 * 75 + 7 * 75 + 5 * 7 * 4
    finally:
        op.close()


# --- contract -------------------------------------------------------------------------------------------------------------
def test_submit_before_set_weights_is_a_state_error():
    import torch
    for ic in (64, 100):
        op = dfa.InnerProduct((2, 1, 1, ic), 10)
        try:
            a = torch.zeros(2 * ic + 16, dtype=torch.uint8, device="cuda")
            dst = torch.zeros(32, dtype=torch.uint8, device="cuda")
            with pytest.raises(dfa.DfxError) as e:
                op.submit(a, dst)
            assert "dfx error 5" in str(e.value)
            with pytest.raises(dfa.DfxError) as e:
                op.submit_host(np.zeros((2, 1, 1, ic), dtype=np.uint8))
            assert "dfx error 5" in str(e.value)
            with pytest.raises(dfa.DfxError) as e:
                op.requant()
            assert "dfx error 5" in str(e.value)
            if ic == 64:
                assert op.info().kernel_name.decode().endswith("(no weights)")
        finally:
            op.close()


def test_misaligned_pointers_are_refused_and_nothing_is_launched():
    import ctypes
    import torch
    case = R.FcCase("misal", 2, 64, 1, 1, 16, bia_dt=C.UNDEF)
    op = make_op(case, R.generate(case))
    try:
        a = torch.zeros(2 * 64 + 32, dtype=torch.uint8, device="cuda")
        dst = torch.full((64,), 0x77, dtype=torch.uint8, device="cuda")
        L = capi.lib()
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for oa, od in ((8, 0), (0, 8), (1, 1), (4, 0), (0, 2)):
            rc = L.dfx_fc_submit(op._h, ctypes.c_void_p(a.data_ptr() + oa), ctypes.c_void_p(dst.data_ptr() + od), st)
            assert rc == 1 and b"16-byte aligned" in L.dfx_last_error(), (oa, od, rc)
        assert L.dfx_fc_submit(op._h, None, ctypes.c_void_p(dst.data_ptr()), st) == 1       # null src
        assert L.dfx_fc_submit(op._h, ctypes.c_void_p(a.data_ptr()), None, st) == 1         # null dst
        torch.cuda.synchronize()
        assert bool((dst == 0x77).all()), "a refused submit wrote to dst"
        op.submit(a, dst)                            # the aligned call goes through
        torch.cuda.synchronize()
        assert bool((dst[32:] == 0x77).all()) and not bool((dst[:32] == 0x77).all())
    finally:
        op.close()


@pytest.mark.parametrize("path", [R.MFMA, R.GENERIC])
def test_set_weights_again_takes_effect(path):
    import torch
    case = R.FcCase("reweigh", 33, 192, 1, 1, 33, seed=27400, **R.OPTIONS[0])
    data = R.generate(case)
    data2 = dict(R.generate(replace(case, seed=77, wide=True)), src=data["src"])
    ref1, ref2 = R.fc_ref(case, data), R.fc_ref(case, data2)
    assert not np.array_equal(ref1, ref2)
    op = make_op(case, data, force_path=path)
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
        if path == R.MFMA:       # the route follows the numbers of the LAST set_weights
            assert op.requant() == FAST
            op.set_weights(data2["w"], np.array([np.inf], dtype=np.float32), bia=data2["bia"])
            assert op.requant() == EXACT and op.info().kernel_name.decode().endswith("exact")
        op.set_weights(data["w"], data["scales"], bia=data["bia"])
        assert op.requant() == (FAST if path == R.MFMA else EXACT)
        op.submit(src, dst)
        torch.cuda.synchronize()
        hipref.assert_dev_bit_equal(dst, ref1, "first weights again")
    finally:
        op.close()


@pytest.mark.parametrize("path", [R.MFMA, R.GENERIC])
def test_one_handle_on_three_streams(tuning, path):
    """three different inputs, one per stream, ten rounds, submitted alternately on one handle: on the MFMA path the
    handle's one slab is handed from submit to submit, in order, on the device"""
    import torch
    tuning.setenv("DFX_FC_SPLITK", 3)
    case = R.FcCase("3streams", 130, 64, 7, 7, 130, dst_dt=C.U8, bia_dt=C.S32, per_channel=True, seed=27500)
    data = R.generate(case)
    streams = [torch.cuda.Stream() for _ in range(3)]
    devs, refs = [], []
    for k in range(3):
        dk = dict(data, src=R.generate(replace(case, seed=300 + k))["src"])
        devs.append(torch.from_numpy(dk["src"]).cuda())
        refs.append(R.fc_ref(case, dk))
    assert not np.array_equal(refs[0], refs[1]) and not np.array_equal(refs[1], refs[2])
    op = make_op(case, data, force_path=path)
    try:
        assert op.info().splitk == (3 if path == R.MFMA else 1)
        outs = [[torch.full(op.dst_shape, hipref.POISON_BYTE, dtype=torch.uint8, device="cuda") for _ in range(10)] for _ in range(3)]
        torch.cuda.synchronize()
        for it in range(10):
            for k, st in enumerate(streams):
                op.submit(devs[k], outs[k][it], stream=st)
        torch.cuda.synchronize()
        for k in range(3):
            ref_dev = torch.from_numpy(refs[k]).cuda()
            for it in range(10):
                hipref.assert_dev_bit_equal(outs[k][it], refs[k], "path %d stream %d launch %d" % (path, k, it), ref_dev=ref_dev)
    finally:
        op.close()


@pytest.mark.parametrize("path", [R.MFMA, R.GENERIC])
def test_non_default_stream_and_submit_host(path):
    import torch
    case = R.FcCase("stream", 33, 16, 2, 2, 130, dst_dt=C.S32, bia_dt=C.S32, relu=False, per_channel=True, seed=27600)
    data, ref = reference(case)
    got, info, route = run(case, data, force_path=path, stream=torch.cuda.Stream())
    hipref.assert_bit_equal(got, ref, "non-default stream path %d" % path)
    op = make_op(case, data, path)
    try:
        hipref.assert_bit_equal(op.submit_host(data["src"]), ref, "submit_host path %d" % path)
        hipref.assert_bit_equal(op.submit_host(data["src"]), ref, "submit_host again path %d" % path)
    finally:
        op.close()


def test_classifier_head():
    """bs 8, 2048 -> 1000, u8 -> s8 with s32 bias (ResNet-50's head): the planner's splitk, every byte on the device"""
    case = R.FcCase("head", 8, 2048, 1, 1, 1000, dst_dt=C.S8, bia_dt=C.S32, relu=False, per_channel=True, seed=27700)
    data = R.generate(case)
    ref = R.fc_ref(case, data)
    got, info, route = run(case, data, on_device=True)
    assert info.path == R.MFMA and route == FAST and info.splitk == R.planned_splitk(case, cus()), (info.kernel_name, info.splitk)
    hipref.assert_dev_bit_equal(got, ref, "classifier head [%s]" % info.kernel_name.decode())


# --- the C++ layer ------------------------------------------------------------------------------------------------------
def test_fc_check_exits_0():
    """tools/fc_check: deepfusion::inner_product end to end against a scalar loop in the tool"""
    exe = os.path.join(TOOLS, "fc_check")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    env = {k: v for k, v in os.environ.items() if k != "DEEPFUSION_DEVICES"}
    p = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0, p.stdout.decode()
    assert b"fc_check: every layer identical to the scalar loop" in p.stdout, p.stdout.decode()
