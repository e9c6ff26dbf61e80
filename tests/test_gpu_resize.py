"""GPU: the activation resize (dfx_resize_*, deepfusion::resize / resize_add) against the numpy reference of
tests/resize_ref.py, bit for bit, on both kernel paths; band seams and the grid-stride loop; the defining properties
against dfx_deconv, dfx_pool and dfx_eltwise on the device; f32 specials; the pointer / stream / thread contract; an FPN
top-down step that stays on the device; the C++ layer on any device count; and its speed against torch's interpolate."""
import ctypes
import importlib
import os
import subprocess
import threading

import numpy as np
import pytest

import cases as C
import hipref
import resize_ref as R

pytestmark = pytest.mark.gpu
dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "deep-fusion_amd", "tools")
GUARD = 1 << 16       # guard bytes on each side of dst
POISON = 0xCD
MODES = [(a, c) for a in (R.NEAREST, R.BILINEAR) for c in (R.HALF_PIXEL, R.ALIGN_CORNERS, R.ASYMMETRIC)]


def _torch_dt(np_dtype):
    import torch
    return {np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32, np.dtype(np.int8): torch.int8,
            np.dtype(np.uint8): torch.uint8}[np.dtype(np_dtype)]


def _guarded(shape, np_dtype):
    """-> (buf, dst): dst is a view into the middle of buf; all of buf holds 0xCD"""
    import torch
    nbytes = int(np.prod(shape)) * np.dtype(np_dtype).itemsize
    buf = torch.empty(GUARD + nbytes + GUARD, dtype=torch.uint8, device="cuda")
    buf.fill_(POISON)
    return buf, buf[GUARD:GUARD + nbytes].view(_torch_dt(np_dtype)).view(shape)


def _assert_guards(buf, what):
    n = buf.numel()
    assert bool((buf[:GUARD] == POISON).all()), what + ": bytes before dst were overwritten"
    assert bool((buf[n - GUARD:] == POISON).all()), what + ": bytes behind dst were overwritten"


def _paths(c, dtype):
    """the force_path values a channel count admits, with the path each must report"""
    if R.in_band_class(c, dtype):
        return [(capi.RESIZE_BAND, R.BAND), (capi.RESIZE_GENERIC, R.GENERIC), (capi.RESIZE_AUTO, R.BAND)]
    return [(capi.RESIZE_GENERIC, R.GENERIC), (capi.RESIZE_AUTO, R.GENERIC)]


def _run(src, out_hw, algo, coord, force, want_path, ref, host=False):
    import torch
    op = dfa.Resize(src.shape, out_hw, src.dtype, algo=algo, coord=coord, force_path=force)
    try:
        info = op.info()
        what = "%s -> %s %s algo %d coord %d [%s]" % (src.shape, out_hw, src.dtype, algo, coord, info.kernel_name.decode())
        assert info.path == want_path, what
        assert info.rows_per_lane >= 1 and info.block == 256 and info.grid >= 1, what
        assert info.algorithmic_bytes == src.nbytes + ref.nbytes, what
        buf, dst = _guarded(ref.shape, src.dtype)
        op.submit(torch.from_numpy(src).cuda(), dst)
        torch.cuda.synchronize()
        hipref.assert_bit_equal(dst.cpu().numpy(), ref, what)
        _assert_guards(buf, what)
        if host:
            hipref.assert_bit_equal(op.submit_host(src), ref, what + " submit_host")
        return info.path
    finally:
        op.close()


@pytest.mark.parametrize("geom", R.GEOMS, ids=lambda g: "%dx%d-%dx%d" % g)
def test_table_parity(geom):
    ih, iw, oh, ow = geom
    seen = set()
    runs = 0
    table = list(R.CHANNELS) + [(np.int32, R.S32_CHANNELS)]
    for dtype, channels in table:
        for c in channels:
            for bs in R.BATCHES:
                src = R.random_src((bs, ih, iw, c), dtype, seed=ih * 1000 + ow * 10 + c)
                for algo, coord in MODES:
                    if dtype == np.int32 and algo == R.BILINEAR:
                        continue
                    ref = R.resize(src, (oh, ow), algo, coord)       # computed once, shared by the paths
                    for force, want in _paths(c, dtype):
                        seen.add(_run(src, (oh, ow), algo, coord, force, want, ref, host=force == capi.RESIZE_AUTO))
                        runs += 1
    assert seen == {R.BAND, R.GENERIC}, seen
    assert runs == 2 * 6 * (2 * (3 + 3 + 2 + 2) + (3 + 3 + 2)) + 2 * 3 * 3


@pytest.mark.parametrize("rows", [1, 2, 3, 8])
@pytest.mark.parametrize("geom", [(5, 7, 20, 28), (17, 3, 3, 17)], ids=lambda g: "%dx%d-%dx%d" % g)
def test_band_seams_and_the_second_grid_pass(geom, rows):
    """every band length puts the seams elsewhere; with the grid capped at one workgroup every lane of either kernel
    makes at least a second pass of its grid-stride loop"""
    import torch
    ih, iw, oh, ow = geom
    bs = 8
    try:
        capi.set_tuning("DFX_RESIZE_ROWS", rows)
        capi.set_tuning("DFX_RESIZE_MAX_GRID", 1)
        for dtype, c in ((np.uint8, 64), (np.int8, 64), (np.float32, 16)):
            src = R.random_src((bs, ih, iw, c), dtype, seed=rows)
            add = R.random_src((bs, oh, ow, c), dtype, seed=rows + 50)
            for algo, coord in MODES:
                ref = R.resize(src, (oh, ow), algo, coord)
                ref_add = R.eltwise2(ref, add, True)
                for force in (capi.RESIZE_BAND, capi.RESIZE_GENERIC):
                    op = dfa.Resize(src.shape, (oh, ow), dtype, algo=algo, coord=coord, force_path=force)
                    opa = dfa.Resize(src.shape, (oh, ow), dtype, algo=algo, coord=coord, add=True, post_relu=True, force_path=force)
                    try:
                        info = op.info()
                        what = "rows %d %s %s algo %d coord %d [%s]" % (rows, geom, dtype, algo, coord, info.kernel_name.decode())
                        assert info.grid == 1 and info.path == force, what
                        if force == capi.RESIZE_BAND:
                            assert info.rows_per_lane == rows, what
                            items = bs * -(-oh // rows) * ow * (c * np.dtype(dtype).itemsize // 16)
                        else:
                            items = ref.size
                        assert items >= 2 * 256, what                  # every lane comes round again
                        buf, dst = _guarded(ref.shape, dtype)
                        op.submit(torch.from_numpy(src).cuda(), dst)
                        torch.cuda.synchronize()
                        hipref.assert_bit_equal(dst.cpu().numpy(), ref, what)
                        _assert_guards(buf, what)
                        opa.submit(torch.from_numpy(src).cuda(), dst, add_dev=torch.from_numpy(add).cuda())
                        torch.cuda.synchronize()
                        hipref.assert_bit_equal(dst.cpu().numpy(), ref_add, what + " + add")
                        _assert_guards(buf, what + " + add")
                    finally:
                        op.close()
                        opa.close()
    finally:
        capi.set_tuning("DFX_RESIZE_ROWS", None)
        capi.set_tuning("DFX_RESIZE_MAX_GRID", None)


def _both(c, dtype):
    return [capi.RESIZE_BAND, capi.RESIZE_GENERIC] if R.in_band_class(c, dtype) else [capi.RESIZE_GENERIC]


@pytest.mark.parametrize("c", [32, 5])
@pytest.mark.parametrize("s", [2, 3])
def test_nearest_at_an_integer_factor_is_the_deconv_with_identity_weights(s, c):
    import torch
    src = R.random_src((2, 6, 5, c), np.uint8, seed=s + c)
    w = np.zeros((c, c, s, s), dtype=np.int8)
    for k in range(c):
        w[k, k] = 1
    dec = dfa.Deconv(src.shape, c, (s, s), stride=(s, s), pad=(0, 0), dst_dt=capi.DFX_U8, relu=False)
    try:
        dec.set_weights(w, np.array([1.0], dtype=np.float32))
        dinfo = dec.info()
        if s == 2:
            assert dinfo.path == (capi.DECONV_MFMA if c == 32 else capi.DECONV_GENERIC), dinfo.kernel_name
        x = torch.from_numpy(src).cuda()
        want = torch.full(dec.dst_shape, POISON, dtype=torch.uint8, device="cuda")
        dec.submit(x, want)
        torch.cuda.synchronize()
        for coord in (R.ASYMMETRIC, R.HALF_PIXEL):
            for force in _both(c, np.uint8):
                op = dfa.Resize(src.shape, (6 * s, 5 * s), np.uint8, algo=R.NEAREST, coord=coord, force_path=force)
                try:
                    got = torch.full(dec.dst_shape, POISON ^ 0xFF, dtype=torch.uint8, device="cuda")
                    op.submit(x, got)
                    torch.cuda.synchronize()
                    assert torch.equal(got, want), (s, c, coord, op.info().kernel_name, dinfo.kernel_name)
                finally:
                    op.close()
    finally:
        dec.close()


@pytest.mark.parametrize("dtype", [np.uint8, np.int8])
def test_bilinear_half_pixel_at_half_size_is_the_2x2_average_pool(dtype):
    import torch
    info = np.iinfo(dtype)
    for c in (16, 5):
        src = R.random_src((3, 10, 12, c), dtype, seed=c)
        src[0, 0:2, 0:2, :] = info.min
        src[0, 0:2, 2:4, :] = info.max
        src[0, 2:4, 0:2, 0] = [[1, 2], [3, 4]]                      # 2.5 -> 2
        src[0, 2:4, 2:4, 0] = [[1, 2], [3, 8]]                      # 3.5 -> 4
        pool = dfa.Pool(3, c, 10, 12, 5, 6, (2, 2), (2, 2), (0, 0), dtype, algo=dfa.Pool.AVG_INCLUDE_PADDING)
        try:
            x = torch.from_numpy(src).cuda()
            want = torch.zeros((3, 5, 6, c), dtype=_torch_dt(dtype), device="cuda")
            pool.submit(x, want)
            torch.cuda.synchronize()
            assert int(want[0, 1, 0, 0]) == 2 and int(want[0, 1, 1, 0]) == 4
            for force in _both(c, dtype):
                op = dfa.Resize(src.shape, (5, 6), dtype, algo=R.BILINEAR, coord=R.HALF_PIXEL, force_path=force)
                try:
                    got = torch.full((3, 5, 6, c), 77, dtype=_torch_dt(dtype), device="cuda")
                    op.submit(x, got)
                    torch.cuda.synchronize()
                    assert torch.equal(got, want), (dtype, c, op.info().kernel_name)
                finally:
                    op.close()
        finally:
            pool.close()


@pytest.mark.parametrize("dtype", [np.uint8, np.int8, np.float32, np.int32])
def test_fused_add_is_resize_then_eltwise(dtype):
    """on the device: dfx_resize with add equals dfx_resize followed by dfx_eltwise, on saturating inputs (random_src is
    full-range, so u8 / s8 / s32 sums leave the range at both ends), with and without ReLU, and in place"""
    import torch
    tdt = _torch_dt(dtype)
    c = 16 if np.dtype(dtype).itemsize == 1 else 4
    for cc in (c, 3):
        src = R.random_src((2, 5, 7, cc), dtype, seed=cc)
        add = R.random_src((2, 10, 14, cc), dtype, seed=cc + 1)
        if dtype == np.int32:
            src.flat[:8] = [2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31, 5, -5, 0, 1]
        x, a = torch.from_numpy(src).cuda(), torch.from_numpy(add).cuda()
        for algo in (R.NEAREST,) if dtype == np.int32 else (R.NEAREST, R.BILINEAR):
            for relu in (False, True):
                elt = dfa.EltwiseSum(2, add.size, dtype, post_relu=relu)
                plain = dfa.Resize(src.shape, (10, 14), dtype, algo=algo, coord=R.HALF_PIXEL, force_path=capi.RESIZE_GENERIC)
                try:
                    tmp = torch.zeros(add.shape, dtype=tdt, device="cuda")
                    want = torch.zeros(add.shape, dtype=tdt, device="cuda")
                    plain.submit(x, tmp)
                    elt.submit([tmp, a], want)
                    torch.cuda.synchronize()
                    hipref.assert_dev_bit_equal(want, R.resize_add(src, add, (10, 14), algo, R.HALF_PIXEL, relu), "the two ops")
                    saturated = dtype == np.float32 or bool((want == np.iinfo(dtype).max).any())
                    assert saturated, "the inputs do not saturate"
                    for force in _both(cc, dtype):
                        op = dfa.Resize(src.shape, (10, 14), dtype, algo=algo, coord=R.HALF_PIXEL, add=True, post_relu=relu,
                                        force_path=force)
                        try:
                            what = "%s c %d algo %d relu %d [%s]" % (dtype, cc, algo, relu, op.info().kernel_name.decode())
                            assert op.info().algorithmic_bytes == src.nbytes + 2 * add.nbytes, what
                            buf, got = _guarded(add.shape, dtype)
                            op.submit(x, got, add_dev=a)
                            torch.cuda.synchronize()
                            assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)), what
                            _assert_guards(buf, what)
                            buf, inplace = _guarded(add.shape, dtype)
                            inplace.copy_(a)
                            op.submit(x, inplace, add_dev=inplace)
                            torch.cuda.synchronize()
                            assert torch.equal(inplace.view(torch.uint8), want.view(torch.uint8)), what + " in place"
                            _assert_guards(buf, what + " in place")
                            hipref.assert_bit_equal(op.submit_host(src, add), want.cpu().numpy(), what + " submit_host")
                        finally:
                            op.close()
                finally:
                    elt.close()
                    plain.close()


def _u32(*bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def test_f32_specials():
    """NaNs of both signs, +-Inf next to a zero weight, -0, denormals, FLT_MAX: where the reference is NaN the result
    is NaN (payloads after arithmetic are not compared), everything else is bit-equal; nearest is a bit copy"""
    import torch
    specials = _u32(0x7fc12345, 0xffc00001, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x807fffff, 0x7f7fffff,
                    0xff7fffff, 0x3f800000, 0x00000000, 0x7fa00001)
    rng = np.random.default_rng(12)
    seen_nan = seen_inf = seen_plain = False
    for c in (4, 3):
        src = (rng.standard_normal((2, 6, 7, c)) * 3).astype(np.float32)
        pos = rng.permutation(src.size)[:4 * len(specials)]
        src.reshape(-1)[pos] = np.tile(specials, 4)
        for oh, ow in ((6, 7), (12, 14), (9, 5), (3, 4)):
            for algo, coord in MODES:
                ref = R.resize(src, (oh, ow), algo, coord)
                if algo == R.BILINEAR:
                    seen_nan, seen_inf, seen_plain = seen_nan | np.isnan(ref).any(), seen_inf | np.isinf(ref).any(), \
                        seen_plain | np.isfinite(ref).any()
                for force in _both(c, np.float32):
                    op = dfa.Resize(src.shape, (oh, ow), np.float32, algo=algo, coord=coord, force_path=force)
                    try:
                        got = torch.zeros(ref.shape, dtype=torch.float32, device="cuda")
                        op.submit(torch.from_numpy(src).cuda(), got)
                        torch.cuda.synchronize()
                        g = got.cpu().numpy()
                        what = "%s algo %d coord %d [%s]" % ((oh, ow), algo, coord, op.info().kernel_name.decode())
                        if algo == R.NEAREST:
                            hipref.assert_bit_equal(g, ref, what)
                        else:
                            nan = np.isnan(ref)
                            assert np.array_equal(np.isnan(g), nan), what
                            assert np.array_equal(g.view(np.uint32)[~nan], ref.view(np.uint32)[~nan]), what
                    finally:
                        op.close()
    assert seen_nan and seen_inf and seen_plain


def test_pointer_contract():
    """null, element-misaligned and 16-byte-misaligned pointers; the add pointer against the descriptor; overlap.
    gfx950 serves unaligned 16-byte accesses, so the bytes alone would not show which kernel a 16-byte-misaligned submit
    took: the library's launch counters (dfx_debug_resize_launches) do."""
    import torch
    L = capi.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    src = R.random_src((2, 5, 7, 4), np.float32, seed=1)
    add = R.random_src((2, 10, 14, 4), np.float32, seed=2)
    ref = R.resize(src, (10, 14), R.BILINEAR, R.HALF_PIXEL)
    n_src, n_dst = src.size, ref.size
    xs = torch.zeros(n_src + 8, dtype=torch.float32, device="cuda")
    ad = torch.zeros(n_dst + 8, dtype=torch.float32, device="cuda")
    ds = torch.full((n_dst + 8,), 7.0, dtype=torch.float32, device="cuda")
    op = dfa.Resize(src.shape, (10, 14), np.float32)
    opa = dfa.Resize(src.shape, (10, 14), np.float32, add=True)
    try:
        assert op.info().path == R.BAND and opa.info().path == R.BAND
        before = capi.resize_launches()
        p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)                                  # noqa: E731
        # null pointers; add given or missing against the descriptor
        for h, args in ((op, (None, None, p(ds))), (op, (p(xs), None, None)), (opa, (p(xs), None, p(ds))), (op, (p(xs), p(ad), p(ds)))):
            assert L.dfx_resize_submit(h._h, *args, st) == 1, args
        assert b"add" in L.dfx_last_error()
        # not aligned to the element
        for so, ao, do in ((2, 0, 0), (0, 0, 1), (0, 3, 0)):
            h = opa if ao else op
            assert L.dfx_resize_submit(h._h, p(xs, so), p(ad, ao) if ao else None, p(ds, do), st) == 1, (so, ao, do)
            assert b"aligned to the element" in L.dfx_last_error()
        # dst inside src
        assert L.dfx_resize_submit(op._h, p(xs), None, p(xs, 16), st) == 1 and b"overlaps" in L.dfx_last_error()
        # add overlaps dst without being dst, from either side
        for ao, do in ((16, 0), (0, 16)):
            assert L.dfx_resize_submit(opa._h, p(xs), p(ds, ao), p(ds, do), st) == 1, (ao, do)
            assert b"overlaps dst" in L.dfx_last_error()
        torch.cuda.synchronize()
        assert bool((ds == 7.0).all()), "a refused submit wrote to dst"
        assert capi.resize_launches() == before, "a refused submit launched a kernel"
        # aligned everywhere: the band kernel
        xs[:n_src] = torch.from_numpy(src.reshape(-1)).cuda()
        assert L.dfx_resize_submit(op._h, p(xs), None, p(ds), st) == 0, L.dfx_last_error()
        torch.cuda.synchronize()
        hipref.assert_bit_equal(ds[:n_dst].cpu().numpy().reshape(ref.shape), ref, "aligned")
        assert capi.resize_launches() == (before[0] + 1, before[1])
        # aligned to the element but not to 16 bytes: the generic kernel for that submit, same bytes
        for so, ao, do in ((4, 0, 0), (0, 0, 4), (4, 0, 8), (0, 4, 0), (4, 8, 12)):
            ds.fill_(7.0)
            xs[so // 4:so // 4 + n_src] = torch.from_numpy(src.reshape(-1)).cuda()
            ad[ao // 4:ao // 4 + n_dst] = torch.from_numpy(add.reshape(-1)).cuda()
            h = opa if ao else op
            band, generic = capi.resize_launches()
            assert L.dfx_resize_submit(h._h, p(xs, so), p(ad, ao) if ao else None, p(ds, do), st) == 0, L.dfx_last_error()
            assert capi.resize_launches() == (band, generic + 1), "misaligned %s did not take the generic kernel" % ((so, ao, do),)
            torch.cuda.synchronize()
            want = R.eltwise2(ref, add, False) if ao else ref
            lo = do // 4
            hipref.assert_bit_equal(ds[lo:lo + n_dst].cpu().numpy().reshape(ref.shape), want, "misaligned %s" % ((so, ao, do),))
            assert bool((ds[:lo] == 7.0).all()) and bool((ds[lo + n_dst:] == 7.0).all()), (so, ao, do)
            assert h.info().path == R.BAND                              # the handle's plan is unchanged
    finally:
        op.close()
        opa.close()


def test_one_handle_on_three_streams_and_a_non_default_stream():
    import torch
    shape, out_hw = (2, 9, 11, 32), (20, 23)
    streams = [torch.cuda.Stream() for _ in range(3)]
    srcs = [R.random_src(shape, np.uint8, seed=100 + k) for k in range(3)]
    refs = [R.resize(s, out_hw, R.BILINEAR, R.ALIGN_CORNERS) for s in srcs]
    xs = [torch.from_numpy(s).cuda() for s in srcs]
    torch.cuda.synchronize()
    op = dfa.Resize(shape, out_hw, np.uint8, algo=R.BILINEAR, coord=R.ALIGN_CORNERS)
    try:
        outs = [[torch.full(refs[0].shape, POISON, dtype=torch.uint8, device="cuda") for _ in range(10)] for _ in range(3)]
        torch.cuda.synchronize()
        for it in range(10):
            for k, st in enumerate(streams):
                op.submit(xs[k], outs[k][it], stream=st)
        torch.cuda.synchronize()
        for k in range(3):
            ref_dev = torch.from_numpy(refs[k]).cuda()
            for it in range(10):
                hipref.assert_dev_bit_equal(outs[k][it], refs[k], "stream %d launch %d" % (k, it), ref_dev=ref_dev)
        # a non-default stream through torch's stream context
        out = torch.full(refs[0].shape, POISON, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(streams[1]):
            op.submit(xs[2], out)
        streams[1].synchronize()
        hipref.assert_dev_bit_equal(out, refs[2], "non-default stream")
    finally:
        op.close()


def test_two_host_threads_share_a_handle():
    import torch
    shape, out_hw = (2, 7, 5, 16), (10, 9)
    srcs = [R.random_src(shape, np.int8, seed=k) for k in range(2)]
    refs = [R.resize(s, out_hw, R.BILINEAR, R.HALF_PIXEL) for s in srcs]
    xs = [torch.from_numpy(s).cuda() for s in srcs]
    outs = [[torch.zeros(refs[0].shape, dtype=torch.int8, device="cuda") for _ in range(20)] for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    torch.cuda.synchronize()
    op = dfa.Resize(shape, out_hw, np.int8)
    errors = []

    def work(k):
        try:
            for it in range(20):
                op.submit(xs[k], outs[k][it], stream=streams[k])
                if it % 5 == 0:
                    hipref.assert_bit_equal(op.submit_host(srcs[k]), refs[k], "thread %d submit_host" % k)
            streams[k].synchronize()
        except Exception as e:        # noqa: BLE001  (reported on the main thread)
            errors.append(e)
    try:
        threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        torch.cuda.synchronize()
        for k in range(2):
            for it in range(20):
                hipref.assert_dev_bit_equal(outs[k][it], refs[k], "thread %d launch %d" % (k, it))
    finally:
        op.close()


def test_fpn_top_down_step_stays_on_the_device(oracle):
    """a 1x1 dfx_conv lateral into dst, then resize_add (nearest x2) of the coarser level into it in place, on one
    stream with no host copy in between; equals the oracle's conv followed by the reference resize + sum"""
    import torch
    case = C.ConvCase("fpn_lateral", 2, 32, 8, 10, 32, k=(1, 1), pad=(0, 0))
    data = C.generate(case)
    coarse = R.random_src((2, 4, 5, 32), np.uint8, seed=77)
    lat_ref = hipref.oracle_conv(oracle, case, data)
    assert lat_ref.dtype == np.uint8 and lat_ref.shape == (2, 8, 10, 32) and lat_ref.max() > 0
    want = R.resize_add(coarse, lat_ref, (8, 10), R.NEAREST, R.ASYMMETRIC)
    conv = hipref.make_conv(case, data)
    op = dfa.Resize(coarse.shape, (8, 10), np.uint8, algo=R.NEAREST, coord=R.ASYMMETRIC, add=True)
    try:
        x, up = torch.from_numpy(data["src"]).cuda(), torch.from_numpy(coarse).cuda()
        buf, dst = _guarded(want.shape, np.uint8)
        torch.cuda.synchronize()
        conv.submit(x, dst)
        op.submit(up, dst, add_dev=dst)
        torch.cuda.synchronize()
        hipref.assert_dev_bit_equal(dst, want, "fpn step " + op.info().kernel_name.decode())
        _assert_guards(buf, "fpn step")
    finally:
        conv.close()
        op.close()


def _load(d, name, dtype, shape):
    return np.fromfile(os.path.join(str(d), name), dtype=dtype).reshape(shape)


def _check_dump(d):
    hipref.assert_bit_equal(_load(d, "a_dst.bin", np.uint8, (3, 10, 14, 16)),
                            R.resize(_load(d, "a_src.bin", np.uint8, (3, 5, 7, 16)), (10, 14), R.BILINEAR, R.HALF_PIXEL), "a")
    hipref.assert_bit_equal(_load(d, "b_dst.bin", np.float32, (3, 4, 11, 3)),
                            R.resize(_load(d, "b_src.bin", np.float32, (3, 9, 6, 3)), (4, 11), R.BILINEAR, R.ALIGN_CORNERS), "b")
    hipref.assert_bit_equal(_load(d, "c_dst.bin", np.int8, (4, 20, 28, 5)),
                            R.resize_add(_load(d, "c_src.bin", np.int8, (4, 5, 7, 5)), _load(d, "c_add.bin", np.int8, (4, 20, 28, 5)),
                                         (20, 28), R.NEAREST, R.ASYMMETRIC, True), "c")
    hipref.assert_bit_equal(_load(d, "d_dst.bin", np.uint8, (3, 16, 16, 32)),
                            R.resize_add(_load(d, "d_src.bin", np.uint8, (3, 8, 8, 32)), _load(d, "d_add.bin", np.uint8, (3, 16, 16, 32)),
                                         (16, 16), R.NEAREST, R.ASYMMETRIC, False), "d")


@pytest.mark.parametrize("shards", [None, "2", "3", "all"])
def test_cpp_layer_gives_the_reference_bytes_on_any_device_count(tmp_path, shards):
    exe = os.path.join(TOOLS, "resize_check")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    env = {k: v for k, v in os.environ.items() if k != "DEEPFUSION_DEVICES"}
    if shards:
        env["DEEPFUSION_DEVICES"] = shards
    subprocess.check_call([exe, "-dump", str(tmp_path)], env=env)
    _check_dump(tmp_path)


def test_resize_check_and_bench_resize_run():
    out = subprocess.check_output([os.path.join(TOOLS, "resize_check")])
    assert b"0 mismatches" in out and b"on the band kernel" in out, out
    out = subprocess.check_output([os.path.join(TOOLS, "bench_resize"), "-only", "16->32", "-burning_iter", "1", "-iter", "2",
                                   "-rounds", "1"])
    assert b"results identical" in out and b"GB/s" in out and b"resize_band<u8,nearest,add>" in out, out


def test_speed_against_torch_interpolate():
    """What a user writes without the op: F.interpolate on a channels-last f32 tensor, 64 channels, 64x64 -> 128x128,
    bilinear.  Both sides timed with HIP events after warm-up, interleaved in one process, rotating over enough src / dst
    pairs to exceed 256 MiB so that the Infinity Cache serves neither (the protocol of test_gpu_reorder.py's speed test).
    The margin is that test's too: the op must take at most HALF the eager call's time."""
    import torch
    import torch.nn.functional as F
    bs, c, ih, iw, oh, ow = 32, 64, 64, 64, 128, 128
    pair_bytes = bs * c * 4 * (ih * iw + oh * ow)
    npairs = (256 << 20) // pair_bytes + 2
    assert npairs * pair_bytes > (256 << 20)
    g = torch.Generator(device="cuda").manual_seed(3)
    # NHWC memory seen as an NCHW channels-last tensor by torch, as NHWC by the op
    xs = [(torch.rand((bs, ih, iw, c), device="cuda", generator=g) - 0.5) * 4 for _ in range(npairs)]
    ds = [torch.empty((bs, oh, ow, c), dtype=torch.float32, device="cuda") for _ in range(npairs)]

    def eager(x):
        return F.interpolate(x.permute(0, 3, 1, 2), size=(oh, ow), mode="bilinear", align_corners=False)

    op = dfa.Resize((bs, ih, iw, c), (oh, ow), np.float32, algo=R.BILINEAR, coord=R.HALF_PIXEL)
    try:
        op.submit(xs[0], ds[0])
        y = eager(xs[0])
        torch.cuda.synchronize()
        assert y.is_contiguous(memory_format=torch.channels_last)
        diff = float((y.permute(0, 2, 3, 1) - ds[0]).abs().max())
        assert diff <= R.TORCH_BILINEAR_TOL, "the two sides do not compute the same thing: %g" % diff
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
        info = op.info()
        print("\nresize %.4f ms (%.0f GB/s algorithmic, %s), torch F.interpolate %.4f ms, ratio %.2f" % (
            m_op, info.algorithmic_bytes / m_op / 1e6, info.kernel_name.decode(), m_eager, m_eager / m_op))
        assert rounds * per_round >= 50
        assert m_op <= 0.5 * m_eager, "resize %.4f ms vs torch interpolate %.4f ms" % (m_op, m_eager)
    finally:
        op.close()
