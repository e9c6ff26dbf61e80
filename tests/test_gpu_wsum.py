"""GPU: the scaled element-wise sum (dfx_wsum_*, deepfusion::scaled_sum) against the numpy reference of tests/wsum_ref.py,
bit for bit (tests/test_wsum_cpu.py pins that reference against a float64 witness), and against the ops of the library that
define it on the device: dfx_reorder (one input), dfx_eltwise (all scales 1), a table lookup.  Everything goes through the
C ABI; every dst sits between guard bands with poison fill; path, grid, LDS bytes and kernel name are asserted from info()."""
import functools
import importlib
import os
import re
import subprocess
import threading
from dataclasses import replace

import numpy as np
import pytest

import hipref
import wsum_ref as W

pytestmark = pytest.mark.gpu
dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "deep-fusion_amd", "tools")
GUARD = 1 << 16       # guard bytes on each side of dst


@functools.lru_cache(maxsize=None)
def problem(case):
    """(srcs, (scales, bias, lut), reference): computed once per case and shared; never written to"""
    srcs = W.generate(case)
    params = W.make_params(case)
    want = W.reference(case, srcs, *params)
    for a in srcs + [want]:
        a.setflags(write=False)
    return srcs, params, want


def make_op(case, params, force_path=-1):
    op = dfa.ScaledSum(case.shape, case.src_dts, case.dst_dt, case.nscales(), n_bias=case.n_bias(), post_relu=case.relu,
                       lut_in=None if case.lut_in == W.UNDEF else case.lut_in, rm=case.rm, force_path=force_path)
    op.set_params(*params)
    return op


def on_device(a, offset=0):
    """the bytes of numpy array `a` on the device, `offset` bytes off a 16-byte boundary -> uint8 tensor"""
    import torch
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf = torch.empty(raw.size + offset + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + raw.size]
    view.copy_(torch.from_numpy(raw.copy()))
    return view


def guarded(nbytes, offset=0):
    """-> (buf, dst): dst (poisoned with 0xCD, `offset` bytes off a 16-byte boundary) between two GUARD-byte bands of 0xA5"""
    import torch
    buf = torch.empty(GUARD + offset + nbytes + GUARD, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf.fill_(hipref.GUARD_BYTE)
    mid = buf[GUARD + offset:GUARD + offset + nbytes]
    mid.fill_(hipref.POISON_BYTE)
    return buf, mid


def assert_guards(buf, offset, nbytes, what):
    lo, hi = buf[:GUARD + offset], buf[GUARD + offset + nbytes:]
    assert bool((lo == hipref.GUARD_BYTE).all()) and bool((hi == hipref.GUARD_BYTE).all()), what + ": a guard band was overwritten"


def as_array(dst_dev, case):
    return dst_dev.cpu().numpy().view(W.NP_OF[case.dst_dt]).reshape(case.shape)


def run_guarded(op, case, srcs_dev, offset=0, stream=None):
    import torch
    nbytes = int(np.prod(case.shape)) * W.SIZE_OF[case.dst_dt]
    buf, dst = guarded(nbytes, offset)
    torch.cuda.synchronize()
    op.submit(srcs_dev, dst, stream=stream)
    torch.cuda.synchronize()
    assert_guards(buf, offset, nbytes, op.info().kernel_name.decode())
    return as_array(dst, case)


def want_name(case, path):
    s = "wsum_vec<" if path == W.VEC else "wsum_generic<"
    s += "n%d:%s->%s" % (case.n, ",".join(W.NAME_OF[d] for d in case.src_dts), W.NAME_OF[case.dst_dt])
    s += ",bias" if case.bias != "0" else ""
    s += ",relu" if case.relu else ""
    s += ",lut_" + W.NAME_OF[case.lut_in] if case.lut_in != W.UNDEF else ""
    s += ",down" if case.rm == W.DOWN and case.dst_dt != W.F32 else ""
    return s + ">"


def check(case, path, force_path=-1, grid_cap=0):
    """one guarded submit of `case`; the plan from info() and the bytes against the reference"""
    srcs, params, want = problem(case)
    op = make_op(case, params, force_path)
    try:
        info = op.info()
        what = "%s [%s]" % (case.ident(), info.kernel_name.decode())
        assert info.path == path, what
        assert info.kernel_name.decode() == want_name(case, path), what
        elems = int(np.prod(case.shape))
        assert info.grid == W.planned_grid(elems // 16 if path == W.VEC else elems, grid_cap), (what, info.grid)
        assert info.block == 256 and info.lds_bytes == (case.image_bytes() if path == W.VEC else 0), (what, info.lds_bytes)
        assert info.algorithmic_bytes == elems * (sum(W.SIZE_OF[d] for d in case.src_dts) + W.SIZE_OF[case.dst_dt]), what
        got = run_guarded(op, case, [on_device(s) for s in srcs])
        hipref.assert_bit_equal(got, want, what)
        return got
    finally:
        op.close()


def check_every_path(case, grid_cap=0):
    if case.vec_class:
        a = check(case, W.auto_path(case), grid_cap=grid_cap)
        b = check(case, W.VEC, force_path=W.VEC, grid_cap=grid_cap)
        c = check(case, W.GENERIC, force_path=W.GENERIC, grid_cap=grid_cap)
        assert a.tobytes() == b.tobytes() == c.tobytes()
    else:
        check(case, W.GENERIC, grid_cap=grid_cap)
        check(case, W.GENERIC, force_path=W.GENERIC, grid_cap=grid_cap)
        with pytest.raises(dfa.DfxError, match="dfx error 2"):
            make_op(case, problem(case)[1], force_path=W.VEC)


def forced_paths(case):
    """the kernels a test compares directly: both in the vec class, else the generic one"""
    return [W.VEC, W.GENERIC] if case.vec_class else [W.GENERIC]


# ---- 1. the table against the numpy reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", W.CONFIGS, ids=lambda c: c[0])
def test_table(cfg):
    """every configuration (n in 1, 2, 3, 4, 8; dtype tuples; dst u8 / s8 / f32; per-tensor and per-channel scales mixed;
    bias none / one / per channel; ReLU; both round modes; a table with u8 and with s8 index) on every shape, on both
    paths forced and on auto"""
    cases = [c for c in W.table() if c.name == cfg[0]]
    assert [c.shape for c in cases] == W.SHAPES
    for case in cases:
        check_every_path(case)


@pytest.mark.parametrize("case", W.grid_cases(), ids=lambda c: c.ident())
def test_grid_cap(tuning, case):
    """DFX_WSUM_GRID=2 on 3 x 9 x 11 x 32: 594 groups (19008 elements) over 512 lanes: several grid-stride passes and a
    ragged last one, on both kernels"""
    tuning.setenv("DFX_WSUM_GRID", 2)
    check_every_path(case, grid_cap=2)


def test_the_largest_staged_image():
    """8 per-channel inputs of 2048 channels: 64 KiB of constants in LDS, the edge of the vec class"""
    case = W.WsumCase("lds64k", (1, 1, 2, 2048), (W.U8, W.S8) * 4, W.S8, (True,) * 8, "0", True, W.NEAREST, W.UNDEF, False)
    assert case.vec_class and case.image_bytes() == 64 * 1024
    check_every_path(case)
    over = replace(case, bias="c")
    assert not over.vec_class
    check_every_path(over)


def test_auto_takes_the_vec_kernel_from_2_to_the_19_elements():
    """the AUTO RULE of include/dfx.h (DFX_WSUM_AUTO_NOTE): 64 x 64 x 128 is the first size on the vec kernel, 63 x 64 x 128
    still runs generic; outside the class auto is generic at any size"""
    cfg = [c for c in W.CONFIGS if c[0] == "u8s32"][0]
    for shape, path in (((1, 64, 64, 128), W.VEC), ((1, 63, 64, 128), W.GENERIC), ((1, 64, 64, 136), W.GENERIC)):
        case = W._case(cfg, shape)
        assert W.auto_path(case) == path
        check(case, path)


def test_the_tie_case_on_both_round_modes():
    """u8 - u8 * 1.5 -> s8: exact .5 ties whose two roundings differ, saturation on both sides"""
    for rm in (W.NEAREST, W.DOWN):
        case = replace(W.TIE_CASE, rm=rm)
        srcs = W.generate(case)
        params = W.tie_params()
        want = W.reference(case, srcs, *params)
        for path in (W.VEC, W.GENERIC):
            op = make_op(case, params, force_path=path)
            try:
                hipref.assert_bit_equal(run_guarded(op, case, [on_device(s) for s in srcs]), want, "ties rm%d path%d" % (rm, path))
            finally:
                op.close()


@pytest.mark.parametrize("path", [W.VEC, W.GENERIC], ids=["vec", "generic"])
def test_submit_needs_params_and_takes_them_again(path):
    import torch
    case = [c for c in W.table() if c.name == "u8s8" and c.shape == (2, 5, 7, 16)][0]
    srcs, params, want = problem(case)
    op = dfa.ScaledSum(case.shape, case.src_dts, case.dst_dt, case.nscales(), n_bias=case.n_bias(), post_relu=case.relu, rm=case.rm,
                       force_path=path)
    try:
        devs = [on_device(s) for s in srcs]
        buf, dst = guarded(want.nbytes)
        with pytest.raises(dfa.DfxError, match="dfx error 5"):
            op.submit(devs, dst)
        with pytest.raises(dfa.DfxError, match="dfx error 5"):
            op.submit_host(srcs)
        bad = [params[0][0].copy(), params[0][1]]
        bad[0][3] = np.inf
        with pytest.raises(dfa.DfxError, match="dfx error 1"):
            op.set_params(bad, params[1], params[2])
        with pytest.raises(dfa.DfxError, match="dfx error 1"):
            op.set_params(params[0], np.full(case.c, np.nan, np.float32), params[2])
        torch.cuda.synchronize()
        assert bool((dst == hipref.POISON_BYTE).all())
        op.set_params(*params)
        hipref.assert_bit_equal(op.submit_host(srcs), want, "submit_host")
        halved = [s * np.float32(0.5) for s in params[0]]
        op.set_params(halved, params[1], params[2])
        hipref.assert_bit_equal(run_guarded(op, case, devs), W.reference(case, srcs, halved, params[1], params[2]), "second set_params")
    finally:
        op.close()


# ---- 2. pins against the ops the library has -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 5, 7, 16), (1, 5, 3, 17)], ids=str)
@pytest.mark.parametrize("dst_dt", [W.F32, W.U8, W.S8], ids=lambda d: W.NAME_OF[d])
@pytest.mark.parametrize("src_dt", [W.F32, W.S32, W.S8, W.U8], ids=lambda d: W.NAME_OF[d])
def test_one_input_equals_the_reorder(src_dt, dst_dt, shape):
    """n = 1 without bias, ReLU and table is dfx_reorder NHWC -> NHWC with the same dtypes, scales and round mode: every
    reorder dtype pair, one scale and per-channel scales, both round modes"""
    bs, h, w, c = shape
    for per_channel in (False, True):
        for rm in (W.NEAREST, W.DOWN):
            case = W.WsumCase("pin", shape, (src_dt,), dst_dt, (per_channel,), rm=rm, seed=23)
            srcs = W.generate(case)
            scales, _, _ = W.make_params(case)
            src_dev = on_device(srcs[0])
            ro = dfa.Reorder((bs, c, h, w), src_dt, dst_dt, src_fmt=capi.FMT_NHWC, dst_fmt=capi.FMT_NHWC, scales=scales[0], round_mode=rm)
            try:
                buf, ref = guarded(int(np.prod(shape)) * W.SIZE_OF[dst_dt])
                ro.submit(src_dev, ref)
                for path in forced_paths(case):
                    op = make_op(case, (scales, None, None), force_path=path)
                    try:
                        assert op.info().path == path
                        got = run_guarded(op, case, [src_dev])
                        hipref.assert_bit_equal(got, as_array(ref, case), "%s pc%d rm%d path%d" % (case.ident(), per_channel, rm, path))
                    finally:
                        op.close()
            finally:
                ro.close()


@pytest.mark.parametrize("shape", [(2, 5, 7, 16), (1, 5, 3, 17)], ids=str)
@pytest.mark.parametrize("dt", [W.U8, W.S8, W.F32], ids=lambda d: W.NAME_OF[d])
def test_unit_scales_equal_the_eltwise_sum(dt, shape):
    """all scales 1.0f over one dtype, nearest, n = 2 .. 8, with and without ReLU, is dfx_eltwise: sums of up to 8 bytes stay
    below 2^11 and are exact in f32; f32 tensors of finite values add left to right in both ops"""
    import torch
    rng = np.random.default_rng(5)
    elems = int(np.prod(shape))
    if dt == W.F32:
        pool = [rng.uniform(-100, 100, elems).astype(np.float32).reshape(shape) for _ in range(8)]
        pool[0].reshape(-1)[:4] = [0.0, -0.0, 1e-40, -3e37]
        pool[1].reshape(-1)[:4] = [-0.0, -0.0, -1e-40, -3e37]
    else:
        lo, hi = W.RANGE[dt]
        pool = [rng.integers(lo, hi + 1, elems).astype(W.NP_OF[dt]).reshape(shape) for _ in range(8)]
    devs = [on_device(p) for p in pool]
    for n in range(2, 9):
        for relu in (False, True):
            case = W.WsumCase("pin", shape, (dt,) * n, dt, (False,) * n, relu=relu)
            el = dfa.EltwiseSum(n, elems, W.NP_OF[dt], post_relu=relu)
            try:
                buf, ref = guarded(elems * W.SIZE_OF[dt])
                el.submit(devs[:n], ref)
                torch.cuda.synchronize()
                for path in forced_paths(case):
                    op = make_op(case, ([np.ones(1, np.float32)] * n, None, None), force_path=path)
                    try:
                        assert op.info().path == path
                        got = run_guarded(op, case, devs[:n])
                        hipref.assert_bit_equal(got, as_array(ref, case), "%s n%d relu%d path%d" % (case.ident(), n, relu, path))
                    finally:
                        op.close()
            finally:
                el.close()


@pytest.mark.parametrize("shape", [(2, 5, 7, 16), (1, 5, 3, 17)], ids=str)
@pytest.mark.parametrize("lut_in", [W.U8, W.S8], ids=lambda d: W.NAME_OF[d])
def test_one_input_with_a_table_is_numpy_take(lut_in, shape):
    rng = np.random.default_rng(9)
    x = rng.integers(*(np.array(W.RANGE[lut_in]) + [0, 1]), int(np.prod(shape))).astype(W.NP_OF[lut_in]).reshape(shape)
    x.reshape(-1)[:2] = W.RANGE[lut_in]
    for lut in (rng.permutation(256).astype(np.uint8), W.hswish_table(1 / 16, 1 / 32)):
        for dst_dt in (W.U8, W.S8):
            case = W.WsumCase("take", shape, (lut_in,), dst_dt, (False,), lut_in=lut_in)
            want = np.take(lut, x.astype(np.int64) + (128 if lut_in == W.S8 else 0)).view(W.NP_OF[dst_dt])
            for path in forced_paths(case):
                op = make_op(case, ([np.ones(1, np.float32)], None, lut), force_path=path)
                try:
                    assert op.info().path == path
                    hipref.assert_bit_equal(run_guarded(op, case, [on_device(x)]), want, "%s path%d" % (case.ident(), path))
                finally:
                    op.close()


# ---- 3. in place, and the overlaps that are refused -----------------------------------------------------------------------------
IN_PLACE = [("u8x2", 0), ("u8x2", 1), ("mix4u", 1), ("n8mix", 5), ("n8s8", 7), ("mix4f", 0), ("mix4f", 3), ("n1lut_s8", 0), ("n3f", 1)]


@pytest.mark.parametrize("name, which", IN_PLACE, ids=lambda v: str(v))
@pytest.mark.parametrize("shape", [(2, 5, 7, 16), (1, 5, 3, 17), (1, 33, 17, 256)], ids=str)
def test_in_place(shape, name, which):
    """dst is input `which` (the first, the last, one in between), whose element size is dst's: every element is read from
    all inputs before its lane writes it"""
    import torch
    case = [c for c in W.table() if c.name == name and c.shape == shape][0]
    assert W.SIZE_OF[case.src_dts[which]] == W.SIZE_OF[case.dst_dt]
    srcs, params, want = problem(case)
    for path in forced_paths(case):
        op = make_op(case, params, force_path=path)
        try:
            nbytes = srcs[which].nbytes
            buf, dst = guarded(nbytes)
            dst.copy_(torch.from_numpy(srcs[which].view(np.uint8).reshape(-1).copy()))
            devs = [dst if i == which else on_device(s) for i, s in enumerate(srcs)]
            torch.cuda.synchronize()
            op.submit(devs, dst)
            torch.cuda.synchronize()
            assert_guards(buf, 0, nbytes, case.ident())
            hipref.assert_bit_equal(as_array(dst, case), want, "%s in place %d path %d" % (case.ident(), which, path))
        finally:
            op.close()


@pytest.mark.parametrize("shape", [(2, 5, 7, 16), (1, 5, 3, 17)], ids=str)
def test_one_buffer_given_twice_and_written(shape):
    """x * 1.5 + x * (-0.5) + y -> the buffer of x"""
    import torch
    case = W.WsumCase("twice", shape, (W.S8, W.S8, W.U8), W.S8, (False, True, False), exact=True)
    srcs = W.generate(case)
    srcs[1] = srcs[0]
    params = W.make_params(case)
    want = W.reference(case, srcs, *params)
    for path in forced_paths(case):
        op = make_op(case, params, force_path=path)
        try:
            buf, x = guarded(srcs[0].nbytes)
            x.copy_(torch.from_numpy(srcs[0].view(np.uint8).reshape(-1).copy()))
            y = on_device(srcs[2])
            torch.cuda.synchronize()
            op.submit([x, x, y], x)
            torch.cuda.synchronize()
            assert_guards(buf, 0, srcs[0].nbytes, case.ident())
            hipref.assert_bit_equal(as_array(x, case), want, "%s path %d" % (case.ident(), path))
        finally:
            op.close()


def test_refused_overlaps_write_nothing():
    """a 1-byte dst at the address of a 4-byte input, a 4-byte dst at a 1-byte input, and dst ranges that overlap an input
    partially: DFX_ERR_INVALID, and the poison stays intact"""
    import torch
    shape = (2, 5, 7, 16)
    elems = int(np.prod(shape))
    c1 = W.WsumCase("r", shape, (W.U8, W.S32), W.U8, (False, False))
    c2 = W.WsumCase("r", shape, (W.U8, W.S32), W.F32, (False, False))
    ones = ([np.ones(1, np.float32)] * 2, None, None)
    for case, which in ((c1, 1), (c2, 0)):
        op = make_op(case, ones)
        try:
            big = torch.full((4 * elems + 64,), hipref.POISON_BYTE, dtype=torch.uint8, device="cuda")
            other = on_device(np.zeros(shape, W.NP_OF[case.src_dts[1 - which]]))
            srcs = [big if i == which else other for i in range(2)]
            with pytest.raises(dfa.DfxError, match="dfx error 1"):
                op.submit(srcs, big)
            torch.cuda.synchronize()
            assert bool((big == hipref.POISON_BYTE).all())
        finally:
            op.close()
    case = W.WsumCase("r", shape, (W.U8, W.U8), W.U8, (False, False))
    op = make_op(case, ones)
    try:
        big = torch.full((3 * elems,), hipref.POISON_BYTE, dtype=torch.uint8, device="cuda")
        other = on_device(np.zeros(shape, np.uint8))
        for src_off, dst_off in ((0, 16), (16, 0), (0, elems - 1), (elems - 1, 0), (0, 1)):
            with pytest.raises(dfa.DfxError, match="dfx error 1"):
                op.submit([big[src_off:], other], big[dst_off:])
            with pytest.raises(dfa.DfxError, match="dfx error 1"):
                op.submit([other, big[src_off:]], big[dst_off:])
        torch.cuda.synchronize()
        assert bool((big == hipref.POISON_BYTE).all())
        op.submit([big[0:], other], big[elems:])           # adjacent ranges do not overlap
        torch.cuda.synchronize()
        assert bool((big[elems:2 * elems] == hipref.POISON_BYTE).all()) and bool((big[2 * elems:] == hipref.POISON_BYTE).all())
    finally:
        op.close()
    # a pointer that is not aligned to its 4-byte element
    case = W.WsumCase("r", shape, (W.F32,), W.U8, (False,))
    op = make_op(case, ([np.ones(1, np.float32)], None, None))
    try:
        src = on_device(np.zeros(shape, np.float32), offset=2)
        buf, dst = guarded(elems)
        with pytest.raises(dfa.DfxError, match="dfx error 1"):
            op.submit([src], dst)
        torch.cuda.synchronize()
        assert bool((dst == hipref.POISON_BYTE).all())
    finally:
        op.close()


# ---- 4. misaligned pointers take the generic kernel for that submit -----------------------------------------------------------
@pytest.mark.parametrize("name", ["u8x2", "mix4f", "mix4u", "n1lut_u8"])
def test_misaligned_submit_falls_back(name):
    """each pointer in turn 1 byte (1-byte tensors) or 4 bytes (4-byte tensors) off a 16-byte boundary: the same bytes,
    info().path unchanged, and the launch counters show which kernel ran"""
    case = [c for c in W.table() if c.name == name and c.shape == (1, 3, 3, 48)][0]
    srcs, params, want = problem(case)
    op = make_op(case, params, force_path=W.VEC)
    try:
        assert op.info().path == W.VEC
        before = capi.wsum_launches()
        hipref.assert_bit_equal(run_guarded(op, case, [on_device(s) for s in srcs]), want, "aligned")
        assert capi.wsum_launches() == (before[0] + 1, before[1])
        for k in range(case.n + 1):
            off = W.SIZE_OF[(case.src_dts + (case.dst_dt,))[k]]
            off = 1 if off == 1 else 4
            devs = [on_device(s, off if i == k else 0) for i, s in enumerate(srcs)]
            before = capi.wsum_launches()
            got = run_guarded(op, case, devs, offset=off if k == case.n else 0)
            hipref.assert_bit_equal(got, want, "%s pointer %d off by %d" % (case.ident(), k, off))
            assert capi.wsum_launches() == (before[0], before[1] + 1), k
            assert op.info().path == W.VEC
    finally:
        op.close()


# ---- 5. one handle, two streams and two host threads -------------------------------------------------------------------------
def test_two_streams_and_two_threads_share_a_handle():
    import torch
    case = [c for c in W.table() if c.name == "mix4u" and c.shape == (1, 33, 17, 256)][0]
    srcs, params, want = problem(case)
    flipped = [np.ascontiguousarray(s[:, ::-1]) for s in srcs]
    want2 = W.reference(case, flipped, *params)
    op = make_op(case, params, force_path=W.VEC)
    try:
        sets = [[on_device(s) for s in srcs], [on_device(s) for s in flipped]]
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        bufs = [guarded(want.nbytes) for _ in range(2)]
        torch.cuda.synchronize()
        errors = []

        def work(k):
            try:
                for _ in range(8):
                    op.submit(sets[k], bufs[k][1], stream=streams[k])
                streams[k].synchronize()
            except Exception as e:   # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        torch.cuda.synchronize()
        assert not errors, errors
        for k, w in enumerate((want, want2)):
            assert_guards(bufs[k][0], 0, want.nbytes, "stream %d" % k)
            hipref.assert_bit_equal(as_array(bufs[k][1], case), w, "stream %d" % k)
    finally:
        op.close()


# ---- 6. the drop-in C++ layer -----------------------------------------------------------------------------------------------
def test_wsum_check_tool():
    """scaled_sum() of the C++ API against the C ABI and the tool's scalar loop, unsharded and with the batch split over
    DEEPFUSION_DEVICES shards (2 devices where there are two, else 2 shards on one): the bytes are the same"""
    exe = os.path.join(TOOLS, "wsum_check")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    hashes = []
    for shards in ("1", "2"):
        env = dict(os.environ)
        env["DEEPFUSION_DEVICES"] = shards
        p = subprocess.run(["timeout", "-k", "10", "240", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, env=env)
        out = p.stdout.decode()
        assert p.returncode == 0 and "wsum_check: every join identical to the scalar loop" in out, out
        hashes.append(re.findall(r"hash ([0-9a-f]{16})", out))
    assert len(hashes[0]) == 8 and hashes[0] == hashes[1]
