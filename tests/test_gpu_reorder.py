"""GPU: the activation reorder (dfx_reorder_*, deepfusion::reorder) against the numpy reference of
tests/reorder_ref.py, bit for bit; its stream / alignment rules; a reorder -> conv -> reorder chain that stays
on the device; the C++ layer; and its speed against the torch eager chain a user would write without it."""
import ctypes
import importlib
import os
import subprocess
from dataclasses import replace

import numpy as np
import pytest

import cases as C
import hipref
import reorder_ref as R

pytestmark = pytest.mark.gpu
dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "deep-fusion_amd", "tools")
BAND = 1 << 16       # guard bytes on each side of dst
POISON = 0xCD


def _torch_dt(dt):
    import torch
    return {R.F32: torch.float32, R.S32: torch.int32, R.S8: torch.int8, R.U8: torch.uint8}[dt]


def _make(case, scales):
    return dfa.Reorder(case.shape, case.src_dt, case.dst_dt, src_fmt=case.src_fmt, dst_fmt=case.dst_fmt,
                       dst_c=case.dst_c, scales=scales, round_mode=case.rm)


def _guarded(case):
    """-> (buf, dst): dst is a view into the middle of buf; all of buf holds 0xCD"""
    import torch
    nbytes = int(np.prod(case.dst_shape)) * np.dtype(R.NP_OF[case.dst_dt]).itemsize
    buf = torch.empty(BAND + nbytes + BAND, dtype=torch.uint8, device="cuda")
    buf.fill_(POISON)
    return buf, buf[BAND:BAND + nbytes].view(_torch_dt(case.dst_dt)).view(case.dst_shape)


def _assert_guards(buf, what):
    n = buf.numel()
    assert bool((buf[:BAND] == POISON).all()), what + ": bytes before dst were overwritten"
    assert bool((buf[n - BAND:] == POISON).all()), what + ": bytes behind dst were overwritten"


@pytest.mark.parametrize("dts", R.DTYPE_PAIRS, ids=lambda d: "%s-%s" % (R.NAME_OF[d[0]], R.NAME_OF[d[1]]))
@pytest.mark.parametrize("lay", R.LAYOUTS, ids=lambda l: "%s-%s" % (R.FMT_NAME[l[0]], R.FMT_NAME[l[1]]))
def test_table_parity(lay, dts):
    import torch
    cases = R.table(layouts=[lay], dtype_pairs=[dts])
    assert len(cases) >= 40
    paths = set()
    for c in cases:
        src, sc = R.generate(c), R.make_scales(c)
        ref = R.reference(src, c, sc)
        op = _make(c, sc)
        try:
            info = op.info()
            what = "%s [%s]" % (c.ident(), info.kernel_name.decode())
            paths.add(info.path)
            assert op.dst_shape == c.dst_shape and op.src_shape == c.src_shape, what
            buf, dst = _guarded(c)
            op.submit(torch.from_numpy(src).cuda(), dst)
            torch.cuda.synchronize()
            hipref.assert_bit_equal(dst.cpu().numpy(), ref, what)
            _assert_guards(buf, what)
            hipref.assert_bit_equal(op.submit_host(src), ref, what + " submit_host")
        finally:
            op.close()
    if lay[0] == lay[1]:
        assert paths == {capi.REORDER_FLAT, capi.REORDER_GENERIC}, paths
    elif lay == (R.NCHW, R.NHWC):
        assert paths == {capi.REORDER_SMALLC, capi.REORDER_TRANSPOSE}, paths
    else:
        assert paths == {capi.REORDER_TRANSPOSE}, paths


def test_query_reports_the_paths_the_design_names():
    def q(shape, sdt, ddt, sf, df, dst_c=None):
        op = dfa.Reorder(shape, sdt, ddt, src_fmt=sf, dst_fmt=df, dst_c=dst_c)
        i = op.info()
        op.close()
        return i
    i = q((128, 64, 56, 56), np.float32, np.uint8, capi.FMT_NCHW, capi.FMT_NHWC)
    assert i.path == capi.REORDER_TRANSPOSE and i.tile_pixels == 64 and i.channel_block == 64
    assert i.vec_plane == 1 and i.vec_pixel == 1 and i.block == 256 and i.lds_bytes == 64 * 65 * 4
    assert i.grid == 128 * 49 and i.algorithmic_bytes == 128 * 64 * 56 * 56 * 5
    i = q((128, 3, 224, 224), np.float32, np.uint8, capi.FMT_NCHW, capi.FMT_NHWC, 16)
    assert i.path == capi.REORDER_SMALLC and i.lds_bytes == 0
    assert i.algorithmic_bytes == 128 * 224 * 224 * (3 * 4 + 16)
    i = q((128, 256, 56, 56), np.int32, np.float32, capi.FMT_NHWC, capi.FMT_NCHW)
    assert i.path == capi.REORDER_TRANSPOSE and i.channel_block == 32 and i.tile_pixels == 64      # 128-byte pixel rows
    assert i.vec_plane == 1 and i.vec_pixel == 1 and i.lds_bytes == 32 * 65 * 4 and i.grid == 128 * 49 * 8
    i = q((2, 100, 9, 31), np.float32, np.uint8, capi.FMT_NCHW, capi.FMT_NHWC)        # 100 u8 channels: no 16-byte rows
    assert i.channel_block == 100 and i.lds_bytes == 100 * 65 * 4 and i.vec_pixel == 0 and i.vec_plane == 0
    i = q((2, 100, 8, 32), np.float32, np.uint8, capi.FMT_NCHW, capi.FMT_NHWC)        # ... but the whole span is aligned
    assert i.channel_block == 100 and i.vec_pixel == 1 and i.vec_plane == 1
    i = q((1, 1024, 7, 7), np.float32, np.uint8, capi.FMT_NCHW, capi.FMT_NHWC)      # 7x7 f32 planes: 196 bytes
    assert i.path == capi.REORDER_TRANSPOSE and i.channel_block == 64 and i.vec_plane == 0 and i.vec_pixel == 1
    i = q((3, 17, 13, 17), np.uint8, np.float32, capi.FMT_NCHW, capi.FMT_NHWC)      # 13x17 u8 planes: 221 bytes
    assert i.vec_plane == 0 and i.vec_pixel == 0
    assert q((2, 8, 4, 4), np.float32, np.float32, capi.FMT_NHWC, capi.FMT_NHWC).path == capi.REORDER_FLAT
    assert q((2, 8, 4, 4), np.float32, np.float32, capi.FMT_NHWC, capi.FMT_NHWC, 16).path == capi.REORDER_GENERIC


def _full_size_src(shape, dt, seed):
    """full-size input: seeded random values with the table's special values planted every 4099 elements"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    if dt == R.F32:
        flat = rng.uniform(-100.0, 400.0, n).astype(np.float32)
        sp = np.array([v for v in R._F32_SPECIAL], dtype=np.float32)
    else:
        flat = rng.integers(-40000, 40001, n, dtype=np.int32)
        sp = np.array(R._S32_SPECIAL, dtype=np.int64).astype(np.int32)
    pos = np.arange(0, n, 4099)
    flat[pos] = sp[np.arange(len(pos)) % len(sp)]
    flat[1::2053] = np.round(flat[1::2053]) + (0.5 if dt == R.F32 else 0)
    return flat.reshape(shape)


@pytest.mark.parametrize("which", ["res2a_entry", "image_entry", "s32_exit"])
def test_full_size_parity(which):
    import torch
    if which == "res2a_entry":      # N=128 f32 nchw 64x56x56 -> u8 nhwc, per-channel scale
        c = R.ReorderCase((128, 64, 56, 56), 64, R.NCHW, R.NHWC, R.F32, R.U8, "per")
    elif which == "image_entry":    # N=128 3x224x224 f32 nchw -> u8 nhwc padded to 16
        c = R.ReorderCase((128, 3, 224, 224), 16, R.NCHW, R.NHWC, R.F32, R.U8, "per")
    else:                           # N=128 s32 nhwc 56x56x256 -> f32 nchw
        c = R.ReorderCase((128, 256, 56, 56), 256, R.NHWC, R.NCHW, R.S32, R.F32, "per")
    src = _full_size_src(c.src_shape, c.src_dt, 11)
    sc = R.make_scales(c)
    ref = R.reference(src, c, sc)
    op = _make(c, sc)
    try:
        what = "%s [%s]" % (c.ident(), op.info().kernel_name.decode())
        buf, dst = _guarded(c)
        op.submit(torch.from_numpy(src).cuda(), dst)
        torch.cuda.synchronize()
        hipref.assert_dev_bit_equal(dst, ref, what)
        _assert_guards(buf, what)
    finally:
        op.close()


def test_one_handle_on_three_streams():
    import torch
    c = R.ReorderCase((2, 256, 14, 14), 256, R.NCHW, R.NHWC, R.F32, R.U8, "per")
    sc = R.make_scales(c)
    streams = [torch.cuda.Stream() for _ in range(3)]
    srcs, refs = [], []
    for k in range(3):
        s = R.generate(replace(c, seed=100 + k))
        srcs.append(torch.from_numpy(s).cuda())
        refs.append(R.reference(s, c, sc))
    torch.cuda.synchronize()
    op = _make(c, sc)
    try:
        outs = [[torch.full(c.dst_shape, POISON, dtype=torch.uint8, device="cuda") for _ in range(20)] for _ in range(3)]
        torch.cuda.synchronize()
        for it in range(20):
            for k, st in enumerate(streams):
                op.submit(srcs[k], outs[k][it], stream=st)
        torch.cuda.synchronize()
        for k in range(3):
            ref_dev = torch.from_numpy(refs[k]).cuda()
            for it in range(20):
                hipref.assert_dev_bit_equal(outs[k][it], refs[k], "stream %d launch %d" % (k, it), ref_dev=ref_dev)
    finally:
        op.close()


def test_misaligned_pointers_are_refused_and_nothing_is_launched():
    import torch
    c = R.ReorderCase((2, 24, 5, 100), 24, R.NCHW, R.NHWC, R.F32, R.F32)
    n = int(np.prod(c.src_shape))
    src = torch.zeros(n + 4, dtype=torch.float32, device="cuda")
    dst = torch.full((n + 4,), 7.0, dtype=torch.float32, device="cuda")
    op = _make(c, None)
    try:
        L = capi.lib()
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for so, do in ((4, 0), (0, 4), (4, 4)):      # one f32 element off
            rc = L.dfx_reorder_submit(op._h, ctypes.c_void_p(src.data_ptr() + so), ctypes.c_void_p(dst.data_ptr() + do), st)
            assert rc == 1 and b"16-byte aligned" in L.dfx_last_error(), (so, do, rc)
        with pytest.raises(dfa.DfxError):
            op.submit(src.data_ptr() + 4, dst)
        torch.cuda.synchronize()
        assert bool((dst == 7.0).all()), "a refused submit wrote to dst"
        op.submit(src, dst)                          # the aligned call goes through
        torch.cuda.synchronize()
        assert bool((dst[:n] == 0.0).all()) and bool((dst[n:] == 7.0).all())
    finally:
        op.close()


def test_chain_stays_on_the_device(oracle):
    """f32 nchw -> reorder -> u8 nhwc -> the res2a fused conv (s32 out) -> reorder (per-channel scales) -> f32 nchw,
    all on one stream, no host copy in between; equals reference o oracle conv o reference bit for bit"""
    import torch
    case = C.CONFIG3_SMALL                                           # N=2, 56x56, 64 -> 64 -> 256, s32 out
    data = C.generate(case)
    rng = np.random.default_rng(5)
    x = rng.uniform(-4.0, 28.0, (case.bs, case.ic, case.ih, case.iw)).astype(np.float32)
    x.reshape(-1)[::7] = np.round(x.reshape(-1)[::7]) + np.float32(0.5)
    rin = R.ReorderCase((case.bs, case.ic, case.ih, case.iw), case.ic, R.NCHW, R.NHWC, R.F32, R.U8, "per")
    rout = R.ReorderCase((case.bs, case.oc1x1, case.oh, case.ow), case.oc1x1, R.NHWC, R.NCHW, R.S32, R.F32, "per")
    sc_in = (np.float32(0.3) + np.arange(case.ic, dtype=np.float32) * np.float32(0.004)).astype(np.float32)
    sc_out = R.make_scales(rout)
    q_ref = R.reference(x, rin, sc_in)
    assert q_ref.max() <= 16 and q_ref.max() >= 12                   # the value range the conv cases use
    acc_ref = hipref.oracle_conv(oracle, case, dict(data, src=q_ref))
    y_ref = R.reference(acc_ref, rout, sc_out)
    r0, r1 = _make(rin, sc_in), _make(rout, sc_out)
    conv = hipref.make_conv(case, data)
    try:
        xd = torch.from_numpy(x).cuda()
        q = torch.full(rin.dst_shape, POISON, dtype=torch.uint8, device="cuda")
        acc = torch.full(conv.dst_shape, -1, dtype=torch.int32, device="cuda")
        y = torch.full(rout.dst_shape, float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r0.submit(xd, q)
        conv.submit(q, acc)
        r1.submit(acc, y)
        torch.cuda.synchronize()
        hipref.assert_dev_bit_equal(q, q_ref, "chain: quantised input")
        hipref.assert_dev_bit_equal(acc, acc_ref, "chain: conv " + conv.info().kernel_name.decode())
        hipref.assert_dev_bit_equal(y, y_ref, "chain: result")
    finally:
        r0.close()
        r1.close()
        conv.close()


def _load(d, name, dtype, shape):
    return np.fromfile(os.path.join(str(d), name), dtype=dtype).reshape(shape)


def _check_reorder_check_files(d, oracle):
    c = R.ReorderCase((3, 3, 10, 13), 16, R.NCHW, R.NHWC, R.F32, R.U8, "one")
    hipref.assert_bit_equal(_load(d, "img_dst.bin", np.uint8, c.dst_shape),
                            R.reference(_load(d, "img_src.bin", np.float32, c.src_shape), c, np.array([0.5], np.float32)), "img")
    c = R.ReorderCase((5, 24, 7, 9), 24, R.NHWC, R.NCHW, R.S32, R.F32, "per")
    hipref.assert_bit_equal(_load(d, "deq_dst.bin", np.float32, c.dst_shape),
                            R.reference(_load(d, "deq_src.bin", np.int32, c.src_shape), c, _load(d, "deq_sc.bin", np.float32, (24,))), "deq")
    c = R.ReorderCase((4, 17, 5, 6), 32, R.NHWC, R.NHWC, R.F32, R.S8, "none", R.DOWN)
    hipref.assert_bit_equal(_load(d, "pad_dst.bin", np.int8, c.dst_shape),
                            R.reference(_load(d, "pad_src.bin", np.float32, c.src_shape), c, None), "pad")
    c = R.ReorderCase((3, 40, 6, 8), 40, R.NCHW, R.NCHW, R.U8, R.F32)
    hipref.assert_bit_equal(_load(d, "flat_dst.bin", np.float32, c.dst_shape),
                            R.reference(_load(d, "flat_src.bin", np.uint8, c.src_shape), c, None), "flat")
    rin = R.ReorderCase((5, 32, 9, 11), 32, R.NCHW, R.NHWC, R.F32, R.U8, "per")
    rout = R.ReorderCase((5, 32, 9, 11), 32, R.NHWC, R.NCHW, R.S32, R.F32, "per")
    q = R.reference(_load(d, "chain_x.bin", np.float32, rin.src_shape), rin, _load(d, "chain_sc_in.bin", np.float32, (32,)))
    w0 = _load(d, "chain_w0_oihw.bin", np.int8, (32, 32, 3, 3))
    w1 = _load(d, "chain_w1_oihw.bin", np.int8, (32, 32, 1, 1))
    acc = oracle.conv(q, oracle.reorder_oihw_to_blocked(w0), w0.shape, (1, 1), (1, 1), C.S32,
                      np.array([1.0 / 256], dtype=np.float32), wei1_blk=oracle.reorder_oihw_to_blocked(w1), oc1x1=32,
                      scales1=np.array([1.0 / 8], dtype=np.float32), relu0=True, relu1=False)
    assert np.abs(acc).max() > 50                                     # the chain carries signal
    hipref.assert_bit_equal(_load(d, "chain_y.bin", np.float32, rout.dst_shape),
                            R.reference(acc, rout, _load(d, "chain_sc_out.bin", np.float32, (32,))), "chain")


def test_cpp_layer_reorder_and_chain(oracle, tmp_path):
    exe = os.path.join(TOOLS, "reorder_check")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    env = {k: v for k, v in os.environ.items() if k != "DEEPFUSION_DEVICES"}
    subprocess.check_call([exe, str(tmp_path)], env=env)
    _check_reorder_check_files(tmp_path, oracle)


@pytest.mark.parametrize("shards", ["2", "3", "all"])
def test_cpp_layer_multi_device_same_bytes(tmp_path, shards):
    """DEEPFUSION_DEVICES shards the reorder by batch like conv: every output file equals the single-device run's"""
    exe = os.path.join(TOOLS, "reorder_check")
    one, many = tmp_path / "one", tmp_path / "many"
    one.mkdir()
    many.mkdir()
    env = {k: v for k, v in os.environ.items() if k != "DEEPFUSION_DEVICES"}
    subprocess.check_call([exe, str(one)], env=env)
    subprocess.check_call([exe, str(many)], env=dict(env, DEEPFUSION_DEVICES=shards))
    names = sorted(os.listdir(str(one)))
    assert names == sorted(os.listdir(str(many))) and sum("dst" in n or n == "chain_y.bin" for n in names) == 5
    for n in names:
        assert (one / n).read_bytes() == (many / n).read_bytes(), n


def test_bench_reorder_runs():
    out = subprocess.check_output([os.path.join(TOOLS, "bench_reorder"), "-bs", "2", "-c", "3", "-dst_c", "16", "-h", "32", "-w", "32",
                                   "-burning_iter", "1", "-iter", "2", "-cold_cache"])
    assert b"DeepFusion Reorder avg time" in out and b"COLD caches" in out and b"warm caches" in out, out


@pytest.mark.parametrize("which", ["res2a_entry", "image_entry"])
def test_speed_against_the_torch_eager_chain(which):
    """What a user does today: (x * s).round_().clamp_(0, 255).to(uint8).permute(0, 2, 3, 1).contiguous() (plus F.pad
    for 3 -> 16).  Both sides timed with HIP events after warm-up, interleaved in one process, rotating over
    enough src / dst pairs to exceed 256 MiB so that the Infinity Cache serves neither.  The chain moves at
    least 31 bytes per element against the op's 5: the reorder must take at most HALF the chain's time."""
    import torch
    import torch.nn.functional as F
    if which == "res2a_entry":
        shape, dst_c = (128, 64, 56, 56), 64
    else:
        shape, dst_c = (128, 3, 224, 224), 16
    bs, c, h, w = shape
    case = R.ReorderCase(shape, dst_c, R.NCHW, R.NHWC, R.F32, R.U8, "per")
    sc = R.make_scales(case)
    pair_bytes = bs * h * w * (c * 4 + dst_c)
    npairs = (256 << 20) // pair_bytes + 2
    assert npairs * pair_bytes > (256 << 20)
    g = torch.Generator(device="cuda").manual_seed(3)
    xs = [torch.rand(shape, device="cuda", generator=g) * 300.0 - 20.0 for _ in range(npairs)]
    ds = [torch.empty(case.dst_shape, dtype=torch.uint8, device="cuda") for _ in range(npairs)]
    s = torch.from_numpy(sc).cuda()

    def eager(x):
        y = (x * s.view(1, c, 1, 1)).round_().clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        return F.pad(y, (0, dst_c - c)) if dst_c > c else y

    op = _make(case, sc)
    try:
        op.submit(xs[0], ds[0])
        torch.cuda.synchronize()
        assert torch.equal(ds[0], eager(xs[0])), "the two sides do not compute the same thing"
        for i in range(6):                              # warm-up, both sides
            op.submit(xs[i % npairs], ds[i % npairs])
            eager(xs[i % npairs])
        torch.cuda.synchronize()
        rounds, per_round = 10, 6                        # 60 launches each, interleaved round by round
        t_op, t_eager = [], []
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        k = 0
        for r in range(rounds):
            ev[0].record()
            for i in range(per_round):
                op.submit(xs[(k + i) % npairs], ds[(k + i) % npairs])
            ev[1].record()
            for i in range(per_round):
                eager(xs[(k + i) % npairs])
            ev[2].record()
            torch.cuda.synchronize()
            t_op.append(ev[0].elapsed_time(ev[1]) / per_round)
            t_eager.append(ev[1].elapsed_time(ev[2]) / per_round)
            k += per_round
        m_op, m_eager = float(np.median(t_op)), float(np.median(t_eager))
        algo = op.info().algorithmic_bytes
        print("\n%s: reorder %.4f ms (%.0f GB/s algorithmic), torch eager chain %.4f ms, ratio %.2f" % (
            which, m_op, algo / m_op / 1e6, m_eager, m_eager / m_op))
        assert rounds * per_round >= 50
        assert m_op <= 0.5 * m_eager, "reorder %.4f ms vs eager chain %.4f ms" % (m_op, m_eager)
    finally:
        op.close()
