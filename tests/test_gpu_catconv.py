"""GPU: the concat + pointwise conv op (dfx_catconv_*, deepfusion::concat_conv) against the CPU oracle, bit for bit.
Expected output of every case: oracle.concat of the branches followed by the oracle conv of a cases.ConvCase with
k=(1,1), pad=(0,0) over the concatenated source (hipref.oracle_conv).  Both paths of the op (one fused launch;
concat + conv through the handle's buffer) must produce it, under the three requant routes."""
import ctypes
import importlib
import os
import subprocess
import threading
from dataclasses import replace

import numpy as np
import pytest

import cases as C
import hipref

pytestmark = pytest.mark.gpu
dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "deep-fusion_amd", "tools")
BAND = 1 << 16       # guard bytes on each side of dst
FUSED, TWO = 0, 1    # DFX_CATCONV_FUSED / DFX_CATCONV_TWO_LAUNCH

SPLITS = {
    "128+128": [128, 128],
    "inception3a": [64, 128, 32, 32],
    "densenet": [256] + [32] * 8,          # nine branches, ic 512
    "32x8": [32] * 8,
    "224+32": [224, 32],
}
PIXELS = {"px1": (1, 1, 1), "px297": (1, 11, 27), "px2960": (2, 40, 37)}   # 1; a partial last block; more blocks than waves
OPTIONS = [
    dict(oc=64, dst_dt=C.U8, bia0_dt=C.S32, per_channel0=False, rm0=0, relu0=True),
    dict(oc=128, dst_dt=C.S8, bia0_dt=C.S8, per_channel0=True, rm0=1, relu0=False),
    dict(oc=256, dst_dt=C.S32, bia0_dt=C.UNDEF, per_channel0=False, rm0=0, relu0=False),
    dict(oc=64, dst_dt=C.F32, bia0_dt=C.F32, per_channel0=True, rm0=0, relu0=True),
    dict(oc=128, dst_dt=C.U8, bia0_dt=C.U8, per_channel0=True, rm0=1, relu0=False),      # u8 dst forces the ReLU
    dict(oc=256, dst_dt=C.S8, bia0_dt=C.S32, per_channel0=False, rm0=0, relu0=True, wide=True),
    dict(oc=128, dst_dt=C.S32, bia0_dt=C.F32, per_channel0=True, rm0=1, relu0=True),
    dict(oc=64, dst_dt=C.U8, bia0_dt=C.UNDEF, per_channel0=False, rm0=0, relu0=False, wide=True),
    dict(oc=256, dst_dt=C.F32, bia0_dt=C.S8, per_channel0=False, rm0=1, relu0=False, wide=True),
    dict(oc=256, dst_dt=C.U8, bia0_dt=C.S32, per_channel0=True, rm0=0, relu0=True),
]


def make_case(name, channels, bs, h, w, seed=1234, **opt):
    ic = sum(channels)
    opt = dict(opt)
    if opt["oc"] * ic > 96 * 1024:          # the fused class: oc * ic <= 96 KB (ic 512 admits oc <= 192)
        opt["oc"] = 128
    oc = opt.pop("oc")
    return C.ConvCase(name, bs, ic, h, w, oc, 0, k=(1, 1), pad=(0, 0), seed=seed, **opt)


def table(split):
    out = []
    for pname, (bs, h, w) in PIXELS.items():
        for i, opt in enumerate(OPTIONS):
            out.append(make_case("%s-%s-o%d" % (split, pname, i), SPLITS[split], bs, h, w, seed=1000 + 17 * i + bs + h, **opt))
    return out


def branches_of(data, channels):
    """the case's NHWC source cut into contiguous per-branch tensors"""
    out, c0 = [], 0
    for c in channels:
        out.append(np.ascontiguousarray(data["src"][..., c0:c0 + c]))
        c0 += c
    return out


_EXPECTED = {}


def expected(oracle, case, data, branches, key=None):
    """oracle.concat of the branches, then the oracle's pointwise conv over the result"""
    key = key or case
    if key not in _EXPECTED:
        cat = oracle.concat(branches)
        assert cat.shape == (case.bs, case.ih, case.iw, case.ic)
        _EXPECTED[key] = hipref.oracle_conv(oracle, case, dict(data, src=cat))
    return _EXPECTED[key]


def make_op(case, data, channels, force_path=-1):
    op = dfa.ConcatConv(case.bs, case.ih, case.iw, channels, case.oc, dst_dt=case.dst_dt, bia_dt=case.bia0_dt,
                        relu=case.relu0, rm=case.rm0, nscales=data["scales0"].size, force_path=force_path)
    op.set_weights(dfa.reorder_oihw_to_blocked(data["w0"]), data["scales0"], bia=data["bia0"])
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


def run(case, data, channels, branches, force_path=-1, stream=None):
    """-> (dst ndarray, info): one submit into a guarded dst; the guard bands must survive"""
    import torch
    op = make_op(case, data, channels, force_path)
    try:
        info = op.info()
        dev = [torch.from_numpy(b).cuda() for b in branches]
        buf, dst = guarded_dst(op, case)
        torch.cuda.synchronize()
        op.submit(dev, dst, stream=stream)
        torch.cuda.synchronize()
        hipref.assert_guards(buf, BAND, "%s %s" % (info.kernel_name.decode(), case.ident()))
        return dst.cpu().numpy(), info
    finally:
        op.close()


@pytest.mark.parametrize("split", list(SPLITS))
@pytest.mark.parametrize("switch", [None, "DFX_NO_MAGIC", "DFX_NO_FAST"])
def test_case_table_both_paths(oracle, tuning, switch, split):
    """every case on the fused kernel and on the two-launch path, under the three requant routes (none: fma where the
    host can prove the ranges; DFX_NO_MAGIC: fast; DFX_NO_FAST: exact); on auto every case must pick the fused path"""
    if switch:
        tuning.setenv(switch, "1")
    channels = SPLITS[split]
    seen = set()
    for case in table(split):
        data = C.generate(case)
        br = branches_of(data, channels)
        ref = expected(oracle, case, data, br)
        for path in (FUSED, TWO):
            got, info = run(case, data, channels, br, force_path=path)
            what = "%s path %d [%s] %s" % (case.ident(), path, info.kernel_name.decode(), switch)
            assert info.path == path, what
            hipref.assert_bit_equal(got, ref, what)
            seen.add((path, info.kernel_name.decode().split(" ")[0]))
        op = make_op(case, data, channels)
        try:
            assert op.info().path == FUSED, "auto must take the fused path: " + case.ident()
            assert op.info().kernel_name.decode().startswith("catconv_pw_kernel<")
        finally:
            op.close()
    assert any(p == FUSED for p, _ in seen) and any(p == TWO for p, _ in seen)


def test_table_covers_what_it_should():
    t = [c for s in SPLITS for c in table(s)]
    assert {c.oc for c in t} == {64, 128, 256}
    assert {c.dst_dt for c in t} == {C.U8, C.S8, C.S32, C.F32}
    assert {c.bia0_dt for c in t} == {C.UNDEF, C.F32, C.S32, C.S8, C.U8}
    assert {c.per_channel0 for c in t} == {True, False} and {c.rm0 for c in t} == {0, 1} and {c.relu0 for c in t} == {True, False}
    assert {c.bs * c.ih * c.iw for c in t} == {1, 297, 2 * 40 * 37}
    assert {c.ic for c in t} == {256, 512}
    for s in SPLITS:
        assert {c.oc for c in table(s)} >= {64, 128}


OUTSIDE = {                                  # valid joins outside the fused class: the op must still be total
    "branch16": ([16, 240], 64),
    "branch48": ([48, 208], 128),
    "ic384": ([128, 256], 64),
    "oc96": ([128, 128], 96),
}


@pytest.mark.parametrize("which", list(OUTSIDE))
def test_outside_the_fused_class(oracle, which):
    """auto succeeds with the right bytes on the two-launch path; force_path = FUSED is DFX_ERR_UNSUPPORTED"""
    channels, oc = OUTSIDE[which]
    for dst_dt in (C.U8, C.S32):
        case = make_case(which, channels, 2, 9, 13, oc=oc, dst_dt=dst_dt, bia0_dt=C.S32, per_channel0=True, relu0=True)
        data = C.generate(case)
        br = branches_of(data, channels)
        got, info = run(case, data, channels, br)
        assert info.path == TWO, (which, info.kernel_name)
        hipref.assert_bit_equal(got, expected(oracle, case, data, br), "%s [%s]" % (case.ident(), info.kernel_name.decode()))
        ch = (ctypes.c_int32 * len(channels))(*channels)
        d = capi.CatConvDesc(len(channels), case.bs, case.ih, case.iw, oc, dst_dt, C.S32, 1, 0, oc, FUSED, ch)
        h = ctypes.c_void_p()
        rc = capi.lib().dfx_catconv_create(ctypes.byref(d), ctypes.byref(h))
        assert rc == 2 and not h.value, (which, rc, capi.lib().dfx_last_error())


def test_info_reports_the_launch_and_the_traffic():
    case = make_case("info", [128, 128], 2, 40, 37, oc=64, dst_dt=C.U8, bia0_dt=C.S32, per_channel0=False)
    data = C.generate(case)
    px = 2 * 40 * 37
    for path in (FUSED, TWO):
        op = make_op(case, data, [128, 128], path)
        try:
            i = op.info()
            assert i.path == path and i.block == 256 and i.grid >= 1 and i.lds_bytes >= 64 * 256 and i.device >= 0
            assert i.algorithmic_ops == 2 * px * 64 * 256
            assert i.algorithmic_bytes == px * 256 + 64 * 256 + px * 64 + (2 * px * 256 if path == TWO else 0)
            name = i.kernel_name.decode()
            assert name.startswith("catconv_pw_kernel<2,4>" if path == FUSED else "conv_pw_kernel<2,4>"), name
        finally:
            op.close()


@pytest.mark.parametrize("path", [FUSED, TWO])
def test_branches_are_views_at_odd_offsets_of_one_allocation(oracle, path):
    import torch
    channels = [64, 128, 32, 32]
    case = make_case("views", channels, 2, 13, 9, oc=128, dst_dt=C.S8, bia0_dt=C.S32, per_channel0=True, relu0=False)
    data = C.generate(case)
    br = branches_of(data, channels)
    sizes = [b.size for b in br]
    gaps = [16 * 3, 16 * 7, 16 * 1, 16 * 5]
    pool = torch.full((sum(sizes) + sum(gaps) + 256,), 0xEE, dtype=torch.uint8, device="cuda")
    assert pool.data_ptr() % 32 == 0
    views, off = [], 0
    for b, g in zip(br, gaps):
        off += g
        if (off // 16) % 2 == 0:
            off += 16
        v = pool[off:off + b.size]
        assert v.data_ptr() % 32 == 16                               # 16-byte aligned, nothing coarser
        v.copy_(torch.from_numpy(b.reshape(-1)))
        views.append(v)
        off += b.size
    op = make_op(case, data, channels, path)
    try:
        buf, dst = guarded_dst(op, case)
        torch.cuda.synchronize()
        op.submit(views, dst)
        torch.cuda.synchronize()
        hipref.assert_guards(buf, BAND, "views")
        hipref.assert_bit_equal(dst.cpu().numpy(), expected(oracle, case, data, br), "views path %d" % path)
    finally:
        op.close()


@pytest.mark.parametrize("path", [FUSED, TWO])
def test_the_same_buffer_as_two_branches(oracle, path):
    import torch
    channels = [128, 128]
    case = make_case("alias", channels, 1, 11, 27, oc=64, dst_dt=C.U8, bia0_dt=C.S32, per_channel0=False)
    data = C.generate(case)
    b = np.ascontiguousarray(data["src"][..., :128])
    ref = expected(oracle, case, data, [b, b], key=("alias", case))
    op = make_op(case, data, channels, path)
    try:
        dev = torch.from_numpy(b).cuda()
        buf, dst = guarded_dst(op, case)
        torch.cuda.synchronize()
        op.submit([dev, dev], dst)
        torch.cuda.synchronize()
        hipref.assert_guards(buf, BAND, "alias")
        hipref.assert_bit_equal(dst.cpu().numpy(), ref, "aliased branches path %d" % path)
    finally:
        op.close()


@pytest.mark.parametrize("path", [FUSED, TWO])
def test_misaligned_pointers_are_refused_and_nothing_is_launched(path):
    import torch
    channels = [128, 128]
    case = make_case("misal", channels, 1, 5, 7, oc=64, dst_dt=C.U8, bia0_dt=C.UNDEF, per_channel0=False)
    data = C.generate(case)
    op = make_op(case, data, channels, path)
    try:
        a = torch.zeros(35 * 128 + 32, dtype=torch.uint8, device="cuda")
        b = torch.zeros(35 * 128 + 32, dtype=torch.uint8, device="cuda")
        dst = torch.full((35 * 64 + 32,), 0x77, dtype=torch.uint8, device="cuda")
        L = capi.lib()
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for oa, ob, od in ((8, 0, 0), (0, 4, 0), (0, 0, 8), (1, 1, 1)):
            ptrs = (ctypes.c_void_p * 2)(a.data_ptr() + oa, b.data_ptr() + ob)
            rc = L.dfx_catconv_submit(op._h, ptrs, ctypes.c_void_p(dst.data_ptr() + od), st)
            assert rc == 1 and b"16-byte aligned" in L.dfx_last_error(), (oa, ob, od, rc)
        ptrs = (ctypes.c_void_p * 2)(a.data_ptr(), None)
        assert L.dfx_catconv_submit(op._h, ptrs, ctypes.c_void_p(dst.data_ptr()), st) == 1      # null branch
        assert L.dfx_catconv_submit(op._h, ptrs, None, st) == 1                                  # null dst
        with pytest.raises(dfa.DfxError):
            op.submit([a.data_ptr() + 8, b], dst)
        torch.cuda.synchronize()
        assert bool((dst == 0x77).all()), "a refused submit wrote to dst"
        op.submit([a, b], dst)                       # the aligned call goes through
        torch.cuda.synchronize()
        assert bool((dst[35 * 64:] == 0x77).all()) and not bool((dst[:35 * 64] == 0x77).all())
    finally:
        op.close()


def test_submit_before_set_weights_is_a_state_error():
    import torch
    op = dfa.ConcatConv(1, 4, 4, [128, 128], 64)
    try:
        a = torch.zeros(16 * 128, dtype=torch.uint8, device="cuda")
        dst = torch.zeros(16 * 64, dtype=torch.uint8, device="cuda")
        with pytest.raises(dfa.DfxError) as e:
            op.submit([a, a], dst)
        assert "dfx error 5" in str(e.value)
    finally:
        op.close()


@pytest.mark.parametrize("path", [FUSED, TWO])
def test_non_default_stream_and_submit_host(oracle, path):
    import torch
    channels = [224, 32]
    case = make_case("stream", channels, 2, 40, 37, oc=128, dst_dt=C.S32, bia0_dt=C.S32, per_channel0=True, relu0=False)
    data = C.generate(case)
    br = branches_of(data, channels)
    ref = expected(oracle, case, data, br)
    st = torch.cuda.Stream()
    got, info = run(case, data, channels, br, force_path=path, stream=st)
    hipref.assert_bit_equal(got, ref, "non-default stream path %d" % path)
    op = make_op(case, data, channels, path)
    try:
        hipref.assert_bit_equal(op.submit_host(br), ref, "submit_host path %d" % path)
        hipref.assert_bit_equal(op.submit_host(br), ref, "submit_host again path %d" % path)
    finally:
        op.close()


@pytest.mark.parametrize("path", [FUSED, TWO])
def test_one_handle_on_three_streams(oracle, path):
    """different inputs per stream, 20 submits each, interleaved; on the two-launch path the submits share the
    handle's one intermediate buffer and must be serialised by the handle"""
    import torch
    channels = [64, 128, 32, 32]
    case = make_case("3streams", channels, 2, 40, 37, oc=128, dst_dt=C.U8, bia0_dt=C.S32, per_channel0=True)
    data = C.generate(case)
    streams = [torch.cuda.Stream() for _ in range(3)]
    devs, refs = [], []
    for k in range(3):
        dk = dict(data, src=C.generate(replace(case, seed=300 + k))["src"])
        br = branches_of(dk, channels)
        devs.append([torch.from_numpy(b).cuda() for b in br])
        refs.append(expected(oracle, case, dk, br, key=("3streams", k)))
    assert not np.array_equal(refs[0], refs[1]) and not np.array_equal(refs[1], refs[2])
    op = make_op(case, data, channels, path)
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


@pytest.mark.parametrize("path", [FUSED, TWO])
def test_one_handle_from_two_host_threads(oracle, path):
    import torch
    channels = [128, 128]
    case = make_case("threads", channels, 2, 40, 37, oc=64, dst_dt=C.S8, bia0_dt=C.S8, per_channel0=False, relu0=False)
    data = C.generate(case)
    devs, refs, streams = [], [], []
    for k in range(2):
        dk = dict(data, src=C.generate(replace(case, seed=500 + k))["src"])
        br = branches_of(dk, channels)
        devs.append([torch.from_numpy(b).cuda() for b in br])
        refs.append(expected(oracle, case, dk, br, key=("threads", k)))
        streams.append(torch.cuda.Stream())
    op = make_op(case, data, channels, path)
    try:
        outs = [[torch.full(op.dst_shape, 0x11, dtype=torch.int8, device="cuda") for _ in range(25)] for _ in range(2)]
        torch.cuda.synchronize()
        errors = []

        def worker(k):
            try:
                for it in range(25):
                    op.submit(devs[k], outs[k][it], stream=streams[k])
            except Exception as e:      # noqa: BLE001 -- reported below, on the main thread
                errors.append(e)

        ts = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        torch.cuda.synchronize()
        assert not errors, errors
        for k in range(2):
            ref_dev = torch.from_numpy(refs[k]).cuda()
            for it in range(25):
                hipref.assert_dev_bit_equal(outs[k][it], refs[k], "path %d thread %d launch %d" % (path, k, it), ref_dev=ref_dev)
    finally:
        op.close()


@pytest.mark.parametrize("path", [FUSED, TWO])
def test_set_weights_again_takes_effect(oracle, path):
    import torch
    channels = [32] * 8
    case = make_case("reweigh", channels, 1, 11, 27, oc=64, dst_dt=C.U8, bia0_dt=C.S32, per_channel0=False)
    data = C.generate(case)
    data2 = dict(C.generate(replace(case, seed=77, wide=True)), src=data["src"])
    br = branches_of(data, channels)
    ref1 = expected(oracle, case, data, br)
    ref2 = expected(oracle, case, data2, br, key=("reweigh2", case))
    assert not np.array_equal(ref1, ref2)
    op = make_op(case, data, channels, path)
    try:
        dev = [torch.from_numpy(b).cuda() for b in br]
        dst = torch.full(op.dst_shape, hipref.POISON_BYTE, dtype=torch.uint8, device="cuda")
        op.submit(dev, dst)
        torch.cuda.synchronize()
        hipref.assert_dev_bit_equal(dst, ref1, "first weights path %d" % path)
        op.set_weights(dfa.reorder_oihw_to_blocked(data2["w0"]), data2["scales0"], bia=data2["bia0"])
        op.submit(dev, dst)
        torch.cuda.synchronize()
        hipref.assert_dev_bit_equal(dst, ref2, "second weights path %d" % path)
    finally:
        op.close()


def test_full_size_inception_join(oracle):
    """N = 128, 56 x 56, 128 + 128 -> 64 u8 on the fused path (auto), every byte against the oracle"""
    import torch
    channels = [128, 128]
    case = make_case("full", channels, 128, 56, 56, oc=64, dst_dt=C.U8, bia0_dt=C.S32, per_channel0=False, relu0=True)
    data = C.generate(case)
    br = branches_of(data, channels)
    ref = expected(oracle, case, data, br)
    op = make_op(case, data, channels)
    try:
        info = op.info()
        assert info.path == FUSED, info.kernel_name
        dev = [torch.from_numpy(b).cuda() for b in br]
        buf, dst = guarded_dst(op, case)
        torch.cuda.synchronize()
        op.submit(dev, dst)
        torch.cuda.synchronize()
        hipref.assert_guards(buf, BAND, "full size")
        hipref.assert_dev_bit_equal(dst, ref, "full size [%s]" % info.kernel_name.decode())
    finally:
        op.close()


def _run_check(outdir, shards=None):
    exe = os.path.join(TOOLS, "catconv_check")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    env = {k: v for k, v in os.environ.items() if k != "DEEPFUSION_DEVICES"}
    if shards:
        env["DEEPFUSION_DEVICES"] = shards
    p = subprocess.run([exe, str(outdir)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode()
    assert b"identical to concat() -> conv()" in p.stdout, p.stdout.decode()


def test_cpp_layer_equals_concat_then_conv(tmp_path):
    _run_check(tmp_path)


def test_cpp_layer_multi_device_same_bytes(tmp_path):
    """DEEPFUSION_DEVICES shards concat_conv by batch like conv and concat: every result file equals the unsharded run's"""
    one, many = tmp_path / "one", tmp_path / "many"
    one.mkdir()
    many.mkdir()
    _run_check(one)
    _run_check(many, shards="2")
    names = sorted(os.listdir(str(one)))
    assert names == sorted(os.listdir(str(many))) and len(names) == 7
    for n in names:
        assert (one / n).read_bytes() == (many / n).read_bytes(), n


def test_bench_catconv_runs():
    out = subprocess.check_output([os.path.join(TOOLS, "bench_catconv"), "-shape", "2", "-burning_iter", "2", "-iter", "3", "-rounds", "3"])
    assert b"byte-identical" in out and b"(a) fused op" in out and b"a/c" in out, out
