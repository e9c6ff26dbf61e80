"""GPU: the depthwise + pointwise conv op (dfx_dwpw_*, deepfusion::depthwise_separable_conv) against the numpy reference
of tests/dwpw_ref.py, bit for bit (tests/test_dwpw_cpu.py pins that reference against the C oracle).  Everything goes
through the C ABI; every output is written between guard bands; both requant routes are asserted from requant()
(DFX_NO_FAST forces the exact one); info.path is asserted."""
import ctypes
import importlib
import os
import subprocess
import threading
from dataclasses import replace

import numpy as np
import pytest

import cases as C
import dwpw_ref as R
import hipref

pytestmark = pytest.mark.gpu
dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "deep-fusion_amd", "tools")
BAND = 1 << 16       # guard bytes on each side of dst
EXACT, FAST = R.EXACT, R.FAST


def make_op(case, data, force_path=-1):
    op = dfa.DwPwConv((case.bs, case.ih, case.iw, case.c), case.k, case.oc, stride=case.stride, pad=case.pad,
                      out_hw=(case.oh, case.ow), dst_dt=case.dst_dt, bia0_dt=case.bia0_dt, bia1_dt=case.bia1_dt,
                      relu=case.relu, rm0=case.rm0, rm1=case.rm1, nscales0=data["scales0"].size,
                      nscales1=data["scales1"].size, force_path=force_path)
    op.set_weights(data["w"], data["scales0"], dfa.reorder_oihw_to_blocked(data["w1"]), data["scales1"], bia0=data["bia0"],
                   bia1=data["bia1"])
    return op


def guarded_dst(op, case):
    import torch
    nbytes = int(np.prod(op.dst_shape)) * np.dtype(C.NP_OF[case.dst_dt]).itemsize
    buf = torch.empty(BAND + nbytes + BAND, dtype=torch.uint8, device="cuda")
    buf.fill_(hipref.GUARD_BYTE)
    mid = buf[BAND:BAND + nbytes]
    mid.fill_(hipref.POISON_BYTE)
    return buf, mid.view(hipref.torch_dtype(case.dst_dt)).view(op.dst_shape)


def run(case, data, force_path=-1, stream=None, on_device=False):
    """-> (dst, info, routes): one submit into a guarded dst; the guard bands must survive"""
    import torch
    op = make_op(case, data, force_path)
    try:
        info, routes = op.info(), op.requant()
        src = torch.from_numpy(data["src"]).cuda()
        buf, dst = guarded_dst(op, case)
        torch.cuda.synchronize()
        op.submit(src, dst, stream=stream)
        torch.cuda.synchronize()
        hipref.assert_guards(buf, BAND, "%s %s" % (info.kernel_name.decode(), case.ident()))
        return (dst if on_device else dst.cpu().numpy()), info, routes
    finally:
        op.close()


_REF = {}


def reference(case):
    """computed once per case, shared, never written to"""
    if case not in _REF:
        data = R.generate(case)
        ref = R.ref(case, data)
        ref.setflags(write=False)
        _REF[case] = (data, ref)
    return _REF[case]


def want_routes(case, switch):
    """reference-range and "wide" data are finite and far below 2^30: fast with nearest rounding, per stage"""
    return (FAST if (case.rm0 == 0 and not switch) else EXACT, FAST if (case.rm1 == 0 and not switch) else EXACT)


def check_table(table, switch, tuning, force_path=R.FUSED):
    if switch:
        tuning.setenv(switch, "1")
    for case in table:
        data, ref = reference(case)
        got, info, routes = run(case, data, force_path)
        name = info.kernel_name.decode()
        what = "%s [%s] %s" % (case.ident(), name, switch)
        assert info.path == R.FUSED and name.startswith("dwpw_fused<3x3,s%d,c%d,oc%d," % (case.stride[0], case.c, case.oc)), what
        assert routes == want_routes(case, switch), what
        assert name.endswith("%s/%s" % tuple("fast" if r == FAST else "exact" for r in routes)), what
        th, tw = R.tile_of(case)
        assert (" th %d " % th) in name, what
        hipref.assert_bit_equal(got, ref, what)


@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_shape_table(tuning, switch):
    """every image size of the table x c in {32, 96, 128, 256} x oc in {64, 128, 256}: tiles narrower than the image
    with a ragged last column for every tile width, oh = TH + 1, images smaller than a tile, a partly empty last
    32-pixel block, windows that hang over (the CPU test asserts that the table holds all of it)"""
    check_table(R.shape_table(), switch, tuning)


@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_options_table(tuning, switch):
    check_table(R.options_table(), switch, tuning)


@pytest.mark.parametrize("th", [16, 8, 4, 2])
def test_every_tile_height(tuning, th):
    """the tile height is chosen from the LDS plan; forced here to every value the host can pick, on an image of
    19 rows (a partial last tile row for each) and a ragged tile column, stride 1 and 2"""
    tuning.setenv("DFX_DWPW_TH", th)
    for i, (stride, ih, iw) in enumerate((((1, 1), 19, 37), ((2, 2), 37, 70))):
        case = R.DwPwCase("th", 2, 128, ih, iw, 128, stride=stride, seed=7800 + i, **R.OPTIONS[i])
        data, ref = reference(case)
        got, info, routes = run(case, data, R.FUSED)
        assert (" th %d " % th) in info.kernel_name.decode(), info.kernel_name
        hipref.assert_bit_equal(got, ref, "%s [%s]" % (case.ident(), info.kernel_name.decode()))


@pytest.mark.parametrize("switch", [None, "DFX_NO_FAST"])
def test_more_tiles_than_workgroups(tuning, switch):
    """DFX_DWPW_GRID caps the grid at 1 and at 3 workgroups on a case with 10 tiles of 8 channel groups: the mid tile
    is reused, lanes loop, and 3 divides neither the tile count nor the group count"""
    case = R.DwPwCase("loop", 5, 128, 9, 37, 128, seed=7900, **R.OPTIONS[4])
    th, tw = R.tile_of(case)
    tiles = case.bs * -(-case.oh // th) * -(-case.ow // tw)
    assert tiles >= 7 and tiles % 3 != 0 and (case.c // 16) % 3 != 0, (tiles, case.c // 16)
    data, ref = reference(case)
    if switch:
        tuning.setenv(switch, "1")
    for grid in (1, 3):
        tuning.setenv("DFX_DWPW_GRID", grid)
        got, info, routes = run(case, data, R.FUSED)
        assert info.grid == grid, info.grid
        hipref.assert_bit_equal(got, ref, "%s grid %d [%s]" % (case.ident(), grid, info.kernel_name.decode()))


def test_fused_equals_two_launch_and_the_dense_fused_conv_on_the_device():
    """the same data through the fused path, the two-launch path and (c = 64) the fused dense Conv with block-diagonal
    conv0 weights: compared on the device"""
    import torch
    for i, opt in enumerate(R.OPTIONS[:4]):
        for stride in ((1, 1), (2, 2)):
            case = R.DwPwCase("twin", 2, 64, 12, 20, 128, stride=stride, seed=8000 + i, **opt)
            data = R.generate(case)
            a, ia, ra = run(case, data, R.FUSED, on_device=True)
            b, ib, rb = run(case, data, R.TWO_LAUNCH, on_device=True)
            assert ia.path == R.FUSED and ib.path == R.TWO_LAUNCH and ib.kernel_name.decode().startswith("dwpw_two_launch<")
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "%s: fused differs from two-launch" % case.ident()
            assert ib.algorithmic_bytes == ia.algorithmic_bytes + 2 * case.bs * case.oh * case.ow * case.c
            conv = hipref.make_conv(R.fused_dense_case(case), R.fused_dense_data(data))
            try:
                wbuf, want = guarded_dst(conv, case)
                conv.submit(torch.from_numpy(data["src"]).cuda(), want)
                torch.cuda.synchronize()
                cname = conv.info().kernel_name.decode()
                hipref.assert_guards(wbuf, BAND, cname)
            finally:
                conv.close()
            assert torch.equal(a.view(torch.uint8), want.view(torch.uint8)), "%s: %s differs from %s" % (
                case.ident(), ia.kernel_name.decode(), cname)


@pytest.mark.parametrize("edge", R.EDGES0, ids=lambda e: e.name)
def test_stage0_proof_edges(edge):
    for dst_dt in (C.S32, C.U8):
        case, data = R.edge0_case(edge, dst_dt)
        got, info, routes = run(case, data, R.FUSED)
        assert routes == (FAST if edge.fast else EXACT, FAST), (edge.name, info.kernel_name)
        hipref.assert_bit_equal(got, R.ref(case, data), "%s %s" % (edge.name, info.kernel_name.decode()))


@pytest.mark.parametrize("edge", R.EDGES1, ids=lambda e: e.name)
def test_stage1_proof_edges(tuning, edge):
    """the stage-1 clause at 2^30 exactly and one scale step beyond, with a tensor between the stages that the
    depthwise weights drive to 255 / 0: the routes, the bytes (every dst type), and the attained accumulator"""
    for dst_dt in (C.S32, C.U8, C.S8, C.F32):
        case, data = R.edge1_case(edge, dst_dt)
        got, info, routes = run(case, data, R.FUSED)
        assert routes == (FAST, FAST if edge.fast else EXACT), (edge.name, dst_dt, info.kernel_name)
        hipref.assert_bit_equal(got, R.ref(case, data), "%s %s" % (edge.name, info.kernel_name.decode()))
    case, data = R.edge1_case(edge, C.S32)
    neutral = dict(data, bia1=None, scales1=np.ones(1, dtype=np.float32))
    got, info, routes = run(replace(case, bia1_dt=C.UNDEF, pc1=False), neutral, R.FUSED)
    acc, bound, P, N = R.edge1_attained(edge, case, data)
    assert (got[0 if edge.which == "max" else 1, :, :, R.EDGE_CHANNEL] == bound).all() and bound == acc
    # round-down and DFX_NO_FAST reject whatever the numbers are, per stage
    case, data = R.edge1_case(R.EDGES1[0], C.U8)
    assert run(replace(case, rm1=1), data, R.FUSED)[2] == (FAST, EXACT)
    assert run(replace(case, rm0=1), data, R.FUSED)[2] == (EXACT, FAST)
    tuning.setenv("DFX_NO_FAST", "1")
    got, info, routes = run(case, data, R.FUSED)
    assert routes == (EXACT, EXACT)
    hipref.assert_bit_equal(got, R.ref(case, data), "forced exact")


def test_non_finite_scales_and_biases_give_the_x86_results():
    """NaN / +-inf scales and f32 biases, in either stage, fail that stage's proof alone; the bytes are the x86 ones"""
    for dst_dt in (C.U8, C.S8):
        case = R.DwPwCase("nan", 2, 32, 6, 7, 64, dst_dt=dst_dt, bia0_dt=C.F32, bia1_dt=C.F32, relu=False, pc0=True, pc1=True,
                          seed=8100)
        for poison in (np.nan, np.inf, -np.inf):
            for key, want in (("scales0", (EXACT, FAST)), ("bia0", (EXACT, FAST)), ("scales1", (FAST, EXACT)), ("bia1", (FAST, EXACT))):
                data = R.generate(case)
                data[key] = data[key].copy()
                data[key][19] = poison
                got, info, routes = run(case, data, R.FUSED)
                assert routes == want, (key, poison, info.kernel_name)
                hipref.assert_bit_equal(got, R.ref(case, data), "%s %s = %r" % (case.ident(), key, poison))
        data = R.generate(case)
        data["scales1"][19] = np.nan
        got, info, routes = run(case, data, R.FUSED)
        assert (got[..., 19] == (255 if dst_dt == C.U8 else -128)).all()


def test_outside_the_class_takes_two_launches_and_fused_is_refused():
    for case in R.outside_table():
        data, ref = reference(case)
        got, info, routes = run(case, data)
        assert info.path == R.TWO_LAUNCH, case.ident()
        hipref.assert_bit_equal(got, ref, "%s [%s]" % (case.ident(), info.kernel_name.decode()))
        with pytest.raises(dfa.DfxError) as e:
            make_op(case, data, R.FUSED)
        assert "dfx error 2" in str(e.value) and "fused kernel's class" in str(e.value)


def test_first_fused_launch_after_an_lds_scribble():
    import torch
    case = R.DwPwCase("first", 2, 96, 9, 45, 256, seed=8200, **R.OPTIONS[0])
    data, ref = reference(case)
    op = make_op(case, data, R.FUSED)
    try:
        src = torch.from_numpy(data["src"]).cuda()
        buf, dst = guarded_dst(op, case)
        st = torch.cuda.current_stream()
        assert capi.lib().dfx_debug_scribble_lds(0xFFFFFFFF, ctypes.c_void_p(st.cuda_stream)) == 0
        op.submit(src, dst)
        torch.cuda.synchronize()
        hipref.assert_guards(buf, BAND, "first launch")
        hipref.assert_bit_equal(dst.cpu().numpy(), ref, "first launch after scribble")
    finally:
        op.close()


def test_info_reports_the_launch_and_the_traffic():
    case = R.DwPwCase("info", 2, 128, 13, 37, 128, **R.OPTIONS[0])
    op = make_op(case, R.generate(case), R.FUSED)
    try:
        i = op.info()
        px = 2 * 13 * 37
        assert i.path == R.FUSED and i.block == 256 and 1 <= i.grid <= 2 * 1 * 2 and i.device >= 0
        assert i.lds_bytes == R.lds_plan(128, 128, C.U8, 16)
        assert i.algorithmic_ops == 2 * 9 * px * 128 + 2 * px * 128 * 128
        assert i.algorithmic_bytes == px * 128 + 128 * 9 + 128 * 128 + px * 128
        assert i.kernel_name.decode() == "dwpw_fused<3x3,s1,c128,oc128,u8> th 16 fast/fast"
    finally:
        op.close()


def test_set_weights_again_takes_effect():
    import torch
    case = R.DwPwCase("reweigh", 2, 32, 9, 11, 64, seed=8300, **R.OPTIONS[0])
    data = R.generate(case)
    data2 = dict(R.generate(replace(case, seed=77, wide=True)), src=data["src"])
    ref1, ref2 = R.ref(case, data), R.ref(case, data2)
    assert not np.array_equal(ref1, ref2)
    for path in (R.FUSED, R.TWO_LAUNCH):
        op = make_op(case, data, path)
        try:
            src = torch.from_numpy(data["src"]).cuda()
            buf, dst = guarded_dst(op, case)
            op.submit(src, dst)
            torch.cuda.synchronize()
            hipref.assert_dev_bit_equal(dst, ref1, "first weights")
            op.set_weights(data2["w"], data2["scales0"], dfa.reorder_oihw_to_blocked(data2["w1"]), data2["scales1"],
                           bia0=data2["bia0"], bia1=data2["bia1"])
            op.submit(src, dst)
            torch.cuda.synchronize()
            hipref.assert_dev_bit_equal(dst, ref2, "second weights")
            hipref.assert_guards(buf, BAND, "set_weights again path %d" % path)
            if path == R.FUSED:        # the routes follow the numbers of the LAST set_weights
                assert op.requant() == (FAST, FAST)
                op.set_weights(data2["w"], data2["scales0"], dfa.reorder_oihw_to_blocked(data2["w1"]),
                               np.array([np.inf], dtype=np.float32), bia0=data2["bia0"], bia1=data2["bia1"])
                assert op.requant() == (FAST, EXACT) and op.info().kernel_name.decode().endswith("fast/exact")
        finally:
            op.close()


@pytest.mark.parametrize("path", [R.FUSED, R.TWO_LAUNCH])
def test_one_handle_on_three_streams_and_two_threads(path):
    """different inputs per stream, 12 submits each, interleaved, then two host threads on their own streams: the
    fused launches are independent, the two-launch submits are serialised through the handle's one buffer"""
    import torch
    case = R.DwPwCase("3streams", 2, 64, 24, 37, 64, dst_dt=C.U8, bia0_dt=C.S32, bia1_dt=C.S32, pc1=True, seed=8400)
    data = R.generate(case)
    streams = [torch.cuda.Stream() for _ in range(3)]
    devs, refs = [], []
    for k in range(3):
        dk = dict(data, src=R.generate(replace(case, seed=300 + k))["src"])
        devs.append(torch.from_numpy(dk["src"]).cuda())
        refs.append(R.ref(case, dk))
    assert not np.array_equal(refs[0], refs[1]) and not np.array_equal(refs[1], refs[2])
    ref_devs = [torch.from_numpy(r).cuda() for r in refs]
    op = make_op(case, data, path)
    try:
        pairs = [[guarded_dst(op, case) for _ in range(12)] for _ in range(3)]
        outs = [[d for _, d in row] for row in pairs]
        torch.cuda.synchronize()
        for it in range(12):
            for k, st in enumerate(streams):
                op.submit(devs[k], outs[k][it], stream=st)
        torch.cuda.synchronize()
        for k in range(3):
            for it in range(12):
                hipref.assert_dev_bit_equal(outs[k][it], refs[k], "path %d stream %d launch %d" % (path, k, it), ref_dev=ref_devs[k])
                hipref.assert_guards(pairs[k][it][0], BAND, "path %d stream %d launch %d" % (path, k, it))
        pairs2 = [[guarded_dst(op, case) for _ in range(12)] for _ in range(2)]
        outs2 = [[d for _, d in row] for row in pairs2]
        errs = []

        def work(k):
            try:
                for it in range(12):
                    op.submit(devs[k], outs2[k][it], stream=streams[k])
            except Exception as e:      # noqa: BLE001
                errs.append(e)

        ts = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        torch.cuda.synchronize()
        assert not errs, errs
        for k in range(2):
            for it in range(12):
                hipref.assert_dev_bit_equal(outs2[k][it], refs[k], "path %d thread %d launch %d" % (path, k, it), ref_dev=ref_devs[k])
                hipref.assert_guards(pairs2[k][it][0], BAND, "path %d thread %d launch %d" % (path, k, it))
    finally:
        op.close()


def test_misaligned_and_null_pointers_are_refused_and_nothing_is_launched():
    import torch
    case = R.DwPwCase("misal", 1, 32, 5, 7, 64, bia0_dt=C.UNDEF, bia1_dt=C.UNDEF)
    data = R.generate(case)
    for path in (R.FUSED, R.TWO_LAUNCH):
        op = make_op(case, data, path)
        try:
            n = 35 * 64
            a = torch.zeros(35 * 32 + 32, dtype=torch.uint8, device="cuda")
            buf = torch.full((BAND + n + 32 + BAND,), hipref.GUARD_BYTE, dtype=torch.uint8, device="cuda")
            dst = buf[BAND:BAND + n + 32]
            dst.fill_(0x77)
            L = capi.lib()
            st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            for oa, od in ((8, 0), (0, 8), (1, 1), (4, 0), (0, 2)):
                rc = L.dfx_dwpw_submit(op._h, ctypes.c_void_p(a.data_ptr() + oa), ctypes.c_void_p(dst.data_ptr() + od), st)
                assert rc == 1 and b"16-byte aligned" in L.dfx_last_error(), (oa, od, rc)
            assert L.dfx_dwpw_submit(op._h, None, ctypes.c_void_p(dst.data_ptr()), st) == 1
            assert L.dfx_dwpw_submit(op._h, ctypes.c_void_p(a.data_ptr()), None, st) == 1
            with pytest.raises(dfa.DfxError):
                op.submit(a.data_ptr() + 8, dst)
            torch.cuda.synchronize()
            assert bool((dst == 0x77).all()), "a refused submit wrote to dst"
            op.submit(a, dst)
            torch.cuda.synchronize()
            hipref.assert_guards(buf, BAND, "misaligned")
            assert bool((dst[n:] == 0x77).all()) and not bool((dst[:n] == 0x77).all())
        finally:
            op.close()


def test_submit_before_set_weights_is_a_state_error():
    import torch
    op = dfa.DwPwConv((1, 4, 4, 32), (3, 3), 64)
    try:
        a = torch.zeros(16 * 32, dtype=torch.uint8, device="cuda")
        dst = torch.zeros(16 * 64, dtype=torch.uint8, device="cuda")
        with pytest.raises(dfa.DfxError) as e:
            op.submit(a, dst)
        assert "dfx error 5" in str(e.value)
        with pytest.raises(dfa.DfxError) as e:
            op.requant()
        assert "dfx error 5" in str(e.value)
        assert "(no weights)" in op.info().kernel_name.decode()
    finally:
        op.close()


@pytest.mark.parametrize("path", [R.FUSED, R.TWO_LAUNCH])
def test_non_default_stream_and_submit_host(path):
    import torch
    case = R.DwPwCase("stream", 2, 96, 20, 17, 128, stride=(2, 2), dst_dt=C.S32, bia0_dt=C.S32, bia1_dt=C.F32, relu=False,
                      pc0=True, pc1=True, seed=8500)
    data, ref = reference(case)
    got, info, routes = run(case, data, force_path=path, stream=torch.cuda.Stream())
    assert info.path == path
    hipref.assert_bit_equal(got, ref, "non-default stream path %d" % path)
    op = make_op(case, data, path)
    try:
        hipref.assert_bit_equal(op.submit_host(data["src"]), ref, "submit_host path %d" % path)
        hipref.assert_bit_equal(op.submit_host(data["src"]), ref, "submit_host again path %d" % path)
    finally:
        op.close()


def test_mobilenet_layer():
    """N = 8, 56 x 56, 128 -> 128, u8: more tiles than workgroups fit at once on a small part, every byte against the
    reference on the device"""
    case = R.DwPwCase("mbv1", 8, 128, 56, 56, 128, seed=8600, **R.OPTIONS[0])
    data = R.generate(case)
    got, info, routes = run(case, data, R.FUSED, on_device=True)
    assert info.path == R.FUSED and routes == (FAST, FAST), info.kernel_name
    hipref.assert_dev_bit_equal(got, R.ref(case, data), "mobilenet layer [%s]" % info.kernel_name.decode())


# --- the C++ layer ------------------------------------------------------------------------------------------------------
_LAYERS = {  # dwpw_check.cc's layers: name -> (bs, c, ih, iw, k, s, p, out_hw, oc, dst, bia0, bia1, relu, pc0, pc1, rm0, rm1)
    "s1_u8": (3, 32, 9, 11, 3, 1, 1, None, 64, C.U8, C.S32, C.S32, False, False, False, 0, 0),
    "s2_s8": (4, 64, 8, 7, 3, 2, 1, None, 128, C.S8, C.UNDEF, C.S8, True, True, True, 1, 0),
    "same_s32": (3, 32, 8, 7, 3, 2, 0, (4, 4), 64, C.S32, C.U8, C.F32, False, True, False, 0, 1),
    "c96_f32": (3, 96, 7, 45, 3, 1, 1, None, 256, C.F32, C.S8, C.S32, True, False, True, 0, 0),
    "k5_u8": (5, 48, 6, 9, 5, 1, 2, None, 32, C.U8, C.S32, C.UNDEF, False, False, False, 0, 0),
    "oc96_s8": (3, 32, 5, 5, 3, 1, 1, None, 96, C.S8, C.F32, C.S32, False, True, True, 0, 0),
}


def _run_check(outdir, shards=None):
    exe = os.path.join(TOOLS, "dwpw_check")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    env = {k: v for k, v in os.environ.items() if k != "DEEPFUSION_DEVICES"}
    if shards:
        env["DEEPFUSION_DEVICES"] = shards
    p = subprocess.run([exe, str(outdir)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode()
    assert b"every one identical to depthwise_conv() + conv()" in p.stdout, p.stdout.decode()


def test_cpp_layer_gives_the_reference_bytes_on_any_device_count(tmp_path):
    """dwpw_check through deepfusion::depthwise_separable_conv: its dumped results equal the numpy reference of its
    dumped inputs, and DEEPFUSION_DEVICES = 1, 2 and 3 give the same files"""
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
    for name, (bs, c, ih, iw, k, s, p, ohw, oc, dst_dt, b0, b1, relu, pc0, pc1, rm0, rm1) in _LAYERS.items():
        case = R.DwPwCase(name, bs, c, ih, iw, oc, k=(k, k), stride=(s, s), pad=(p, p), out_hw=ohw, dst_dt=dst_dt, bia0_dt=b0,
                          bia1_dt=b1, relu=relu, rm0=rm0, rm1=rm1, pc0=pc0, pc1=pc1)
        rd = lambda suffix, dt: np.fromfile(str(d / (name + suffix)), dtype=dt)      # noqa: E731
        data = dict(src=rd("_src.bin", np.uint8).reshape(bs, ih, iw, c), w=rd("_wdw.bin", np.int8).reshape(c, k, k),
                    w1=rd("_wpw.bin", np.int8).reshape(oc, c, 1, 1),
                    bia0=None if b0 == C.UNDEF else rd("_bia0.bin", C.NP_OF[b0]),
                    bia1=None if b1 == C.UNDEF else rd("_bia1.bin", C.NP_OF[b1]),
                    scales0=rd("_scales0.bin", np.float32), scales1=rd("_scales1.bin", np.float32))
        assert data["scales0"].size == (c if pc0 else 1) and data["scales1"].size == (oc if pc1 else 1)
        got = rd("_dst.bin", C.NP_OF[dst_dt]).reshape(bs, case.oh, case.ow, oc)
        hipref.assert_bit_equal(got, R.ref(case, data), "dwpw_check " + name)


def test_bench_dwpw_runs():
    out = subprocess.check_output([os.path.join(TOOLS, "bench_dwpw"), "-shape", "4", "-burning_iter", "2", "-iter", "3", "-rounds", "3",
                                   "-rotate_mb", "48", "-cold_cache"])
    for s in (b"(a) fused", b"(b) dwconv + conv", b"(c) dwconv alone", b"(d) the op's two-launch path", b"a/b", b"a/c", b"COLD"):
        assert s in out, out
