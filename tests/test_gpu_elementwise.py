"""GPU: concat, pooling and eltwise sum (dfx_concat_*, dfx_pool_*, dfx_eltwise_*) against the CPU oracle on the inputs
of tests/elementwise_cases.py (tests/test_elementwise_cpu.py pins the oracle on the same bytes).

Everything goes through the C ABI.  Every dst is poisoned and sits between two guard bands inside one allocation;
every src is the tail of a larger allocation with a guard band behind it, so that a read past its end picks up guard
bytes, not zeros.  Comparison: bit for bit where the result is one of the inputs (max pooling, concat, ReLU of a value
passed through); NaN in the same places and bits equal everywhere else where it is computed (f32 averages and sums:
an x86 Inf - Inf gives the negative default NaN, the GPU the positive one)."""
import ctypes
import importlib
import threading

import numpy as np
import pytest

import elementwise_cases as E
import hipref
from test_oracle import POOL_CASES

pytestmark = pytest.mark.gpu
dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
BAND = 1 << 12       # guard bytes on each side of dst and behind src (a multiple of 256: keeps the alignment)
DT_IDS = [np.dtype(d).name for d in E.DTYPES]
ERR_INVALID, ERR_UNSUPPORTED = 1, 2
ALGOS = ((dfa.Pool.MAX, None), (dfa.Pool.AVG_INCLUDE_PADDING, True), (dfa.Pool.AVG_EXCLUDE_PADDING, False))
SMALL_POOL_CASES = [c for c in POOL_CASES if c[0][1] <= 16] + E.POOL_GEOM_CASES


class Dst:
    """nbytes of poison at byte `offset` behind a guard band, another band behind it, all in one allocation"""

    def __init__(self, shape, np_dt, offset=0):
        import torch
        self.shape, self.np_dt = tuple(shape), np.dtype(np_dt)
        self.nbytes = int(np.prod(shape)) * self.np_dt.itemsize
        self.start = BAND + offset
        self.buf = torch.empty(BAND + self.nbytes + BAND + 16, dtype=torch.uint8, device="cuda")
        self.buf.fill_(hipref.GUARD_BYTE)
        self.t = self.buf[self.start:self.start + self.nbytes]
        self.t.fill_(hipref.POISON_BYTE)
        assert self.buf.data_ptr() % 256 == 0
        self.ptr = self.t.data_ptr()

    def check_guards(self, what=""):
        for name, part in (("before", self.buf[:self.start]), ("behind", self.buf[self.start + self.nbytes:])):
            if not bool((part == hipref.GUARD_BYTE).all()):
                hit = (part != hipref.GUARD_BYTE).nonzero().flatten()
                raise AssertionError("%s: %d guard bytes %s dst were overwritten (offsets %d..%d of %d)" % (
                    what, hit.numel(), name, int(hit[0]), int(hit[-1]), part.numel()))

    def still_poison(self):
        return bool((self.t == hipref.POISON_BYTE).all())

    def numpy(self, what=""):
        self.check_guards(what)
        return self.t.cpu().numpy().view(self.np_dt).reshape(self.shape)


def dev_src(x, offset=0):
    """-> uint8 device view holding x's bytes: the tail of a larger allocation (a guard band in front, `offset` bytes
    past a 256-byte boundary), with a guard band behind it"""
    import torch
    raw = np.ascontiguousarray(x).reshape(-1).view(np.uint8)
    buf = torch.empty(BAND + offset + raw.size + BAND, dtype=torch.uint8, device="cuda")
    buf.fill_(hipref.GUARD_BYTE)
    t = buf[BAND + offset:BAND + offset + raw.size]
    t.copy_(torch.from_numpy(raw))
    assert (t.data_ptr() - offset) % 256 == 0
    return t


def sync():
    import torch
    torch.cuda.synchronize()


def make_pool(case, np_dt, algo):
    shape, k, s, p, o = case
    return dfa.Pool(shape[0], shape[3], shape[1], shape[2], o[0], o[1], k, s, p, np_dt, algo=algo)


def pool_reference(oracle, case, x, inc):
    shape, k, s, p, o = case
    ref = oracle.maxpool(x, k, s, p, o) if inc is None else oracle.avgpool(x, k, s, p, o, inc)
    ref.setflags(write=False)
    return ref


def assert_pool_equal(got, ref, inc, what):
    (E.assert_selected_equal if inc is None else E.assert_computed_equal)(got, ref, what)


def run_pool(case, np_dt, algo, src_t, src_off=0, dst_off=0, stream=None):
    op = make_pool(case, np_dt, algo)
    try:
        dst = Dst(op.dst_shape, np_dt, dst_off)
        sync()
        op.submit(src_t, dst.t, stream=stream)
        sync()
        return dst.numpy("pool %s %s" % (E.pool_case_id(case), np.dtype(np_dt).name))
    finally:
        op.close()


# ---- 1. special values on the small geometry cases ----
@pytest.mark.parametrize("np_dt", E.DTYPES, ids=DT_IDS)
def test_pool_special_values(oracle, np_dt):
    """max and both averages on NaN / +-0 / +-Inf / denormal / saturating inputs: windows larger than the input,
    strides larger than the window, non-square windows, padding of k - 1, one input pixel, one output pixel; the table
    holds channel counts for the 16-byte path and for the per-element path of every dtype"""
    paths = set()
    for case in SMALL_POOL_CASES:
        x = E.pool_input(case, np_dt)
        src = dev_src(x)
        paths.add(E.pool_takes_vector_path(case, np_dt))
        for algo, inc in ALGOS:
            what = "%s %s algo %d" % (E.pool_case_id(case), np.dtype(np_dt).name, algo)
            assert_pool_equal(run_pool(case, np_dt, algo, src), pool_reference(oracle, case, x, inc), inc, what)
    assert paths == {True, False}


def run_eltwise(xs, np_dt, relu, srcs=None, dst=None, stream=None):
    op = dfa.EltwiseSum(len(xs), xs[0].size, np_dt, relu)
    try:
        srcs = srcs or [dev_src(x) for x in xs]
        dst = dst or Dst(xs[0].shape, np_dt)
        sync()
        op.submit(srcs, dst.t, stream=stream)
        sync()
        return dst.numpy("eltwise %d x %d %s" % (len(xs), xs[0].size, np.dtype(np_dt).name))
    finally:
        op.close()


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("np_dt", E.DTYPES, ids=DT_IDS)
def test_eltwise_special_values(oracle, np_dt, relu):
    for elems, n in E.ELTWISE_CASES:
        xs = E.eltwise_inputs(elems, np_dt, n)
        E.assert_computed_equal(run_eltwise(xs, np_dt, relu), oracle.eltwise_sum(xs, relu),
                                "eltwise %d x %d relu %d" % (n, elems, relu))


def run_concat(srcs_np, np_dt, relu, srcs=None, stream=None):
    bs, h, w, _ = srcs_np[0].shape
    op = dfa.Concat(bs, h, w, [s.shape[3] for s in srcs_np], np_dt, relu)
    try:
        srcs = srcs or [dev_src(s) for s in srcs_np]
        dst = Dst(op.dst_shape, np_dt)
        sync()
        op.submit(srcs, dst.t, stream=stream)
        sync()
        return dst.numpy("concat %s" % np.dtype(np_dt).name)
    finally:
        op.close()


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("np_dt", E.DTYPES, ids=DT_IDS)
def test_concat_special_values(oracle, np_dt, relu):
    """a NaN keeps its bits with and without ReLU, ReLU(-0) = -0, denormals pass"""
    srcs = E.concat_inputs(E.CONCAT_PIXELS, E.CONCAT_CHANNELS[np.dtype(np_dt).itemsize], np_dt)
    E.assert_selected_equal(run_concat(srcs, np_dt, relu), oracle.concat(srcs, relu), "concat relu %d" % relu)


# ---- 2. grid-stride loops: more work items than the launch has threads ----
@pytest.mark.parametrize("algo,inc", ALGOS)
def test_pool_second_pass_vector_path(oracle, algo, inc):
    case = E.POOL_BIG_VEC
    assert E.pool_takes_vector_path(case, np.float32) and E.pool_items(case, np.float32) > 2048 * 256
    x = E.pool_input(case, np.float32)
    assert_pool_equal(run_pool(case, np.float32, algo, dev_src(x)), pool_reference(oracle, case, x, inc), inc,
                      "second pass, 16-byte path, algo %d" % algo)


def test_pool_second_pass_per_element_path(oracle):
    case = E.POOL_BIG_SCALAR
    assert not E.pool_takes_vector_path(case, np.uint8) and E.pool_items(case, np.uint8) > 2048 * 256
    x = E.pool_input(case, np.uint8)
    E.assert_selected_equal(run_pool(case, np.uint8, dfa.Pool.MAX, dev_src(x)), pool_reference(oracle, case, x, None),
                            "second pass, per-element path")


@pytest.mark.parametrize("np_dt,relu,big", [(np.float32, False, E.ELTWISE_BIG_F32), (np.float32, True, E.ELTWISE_BIG_F32),
                                            (np.uint8, False, E.ELTWISE_BIG_BYTE), (np.int8, True, E.ELTWISE_BIG_BYTE)],
                         ids=["f32", "f32-relu", "u8", "s8-relu"])
def test_eltwise_second_pass(oracle, np_dt, relu, big):
    """the last 500 vector items and the tail elements behind them are reached only by `id += stride`"""
    elems, n = big
    per = 16 // np.dtype(np_dt).itemsize
    assert elems // per > 2048 * 256 and elems % per > 0
    xs = E.eltwise_inputs(elems, np_dt, n)
    E.assert_computed_equal(run_eltwise(xs, np_dt, relu), oracle.eltwise_sum(xs, relu), "eltwise second pass")


@pytest.mark.parametrize("np_dt,channels", [(np.int8, E.CONCAT_BIG_BYTE_CHANNELS), (np.uint8, E.CONCAT_BIG_BYTE_CHANNELS),
                                            (np.float32, E.CONCAT_BIG_F32_CHANNELS)], ids=["s8", "u8", "f32"])
def test_concat_second_pass_with_relu(oracle, np_dt, channels):
    assert int(np.prod(E.CONCAT_BIG_PIXELS)) * sum(channels) * np.dtype(np_dt).itemsize // 16 > 2048 * 256
    srcs = E.concat_inputs(E.CONCAT_BIG_PIXELS, channels, np_dt)
    E.assert_selected_equal(run_concat(srcs, np_dt, True), oracle.concat(srcs, True), "concat second pass")


# ---- 3. concat limits ----
@pytest.mark.parametrize("np_dt", [np.uint8, np.int32], ids=["u8", "s32"])
def test_concat_of_64_branches(oracle, np_dt):
    blk = 16 // np.dtype(np_dt).itemsize
    srcs = E.concat_inputs(E.CONCAT_PIXELS, [blk] * 64, np_dt, seed=43)
    for relu in (False, True):
        E.assert_selected_equal(run_concat(srcs, np_dt, relu), oracle.concat(srcs, relu), "64 branches relu %d" % relu)


def test_concat_of_65_branches_is_refused():
    with pytest.raises(dfa.DfxError) as e:
        dfa.Concat(2, 3, 5, [16] * 65, np.uint8)
    assert "dfx error %d" % ERR_UNSUPPORTED in str(e.value)


# ---- 4. / 5. one handle on three streams, and from two host threads ----
def _three_ops():
    """-> [(name, make_op, inputs(seed) -> list of ndarrays, reference(oracle, inputs), dst shape, dtype, comparison)]
    at sizes of a few blocks each"""
    pool_case = ((2, 40, 37, 16), (3, 3), (2, 2), (1, 1), (20, 19))
    cat_px, cat_ch = (2, 40, 37), [32, 16, 48]
    elems = 2 * 40 * 37 * 5 + 3
    return [
        ("pool", lambda: make_pool(pool_case, np.float32, dfa.Pool.MAX),
         lambda seed: [E.special_f32(pool_case[0], seed, window=pool_case)],
         lambda orc, xs: pool_reference(orc, pool_case, xs[0], None), (2, 20, 19, 16), np.float32,
         E.assert_selected_equal),
        ("eltwise", lambda: dfa.EltwiseSum(3, elems, np.int8, True),
         lambda seed: E.eltwise_inputs(elems, np.int8, 3, seed=seed),
         lambda orc, xs: orc.eltwise_sum(xs, True), (elems,), np.int8, E.assert_computed_equal),
        ("concat", lambda: dfa.Concat(cat_px[0], cat_px[1], cat_px[2], cat_ch, np.int8, True),
         lambda seed: E.concat_inputs(cat_px, cat_ch, np.int8, seed=seed),
         lambda orc, xs: orc.concat(xs, True), cat_px + (sum(cat_ch),), np.int8, E.assert_selected_equal),
    ]


def _submit(name, op, srcs, dst, stream):
    if name == "pool":
        op.submit(srcs[0], dst.t, stream=stream)
    else:
        op.submit(srcs, dst.t, stream=stream)


@pytest.mark.parametrize("which", [0, 1, 2], ids=["pool", "eltwise", "concat"])
def test_one_handle_on_three_streams(oracle, which):
    """each stream has its own inputs and outputs; everything is submitted before the first sync"""
    import torch
    name, make_op, inputs, reference, dshape, np_dt, compare = _three_ops()[which]
    streams = [torch.cuda.Stream() for _ in range(3)]
    xs = [inputs(700 + 10 * k) for k in range(3)]
    refs = [reference(oracle, x) for x in xs]
    assert not np.array_equal(refs[0].view(np.uint8), refs[1].view(np.uint8))
    devs = [[dev_src(a) for a in x] for x in xs]
    op = make_op()
    try:
        outs = [[Dst(dshape, np_dt) for _ in range(6)] for _ in range(3)]
        sync()
        for it in range(6):
            for k, st in enumerate(streams):
                _submit(name, op, devs[k], outs[k][it], st)
        sync()
        for k in range(3):
            for it in range(6):
                what = "%s stream %d launch %d" % (name, k, it)
                compare(outs[k][it].numpy(what), refs[k], what)
    finally:
        op.close()


@pytest.mark.parametrize("which", [0, 1, 2], ids=["pool", "eltwise", "concat"])
def test_one_handle_from_two_host_threads(oracle, which):
    """each thread has its own stream and buffers and submits 30 times: a launch must never see the other thread's
    pointers (dfx_concat_submit once wrote them into the handle and launched from there)"""
    import torch
    name, make_op, inputs, reference, dshape, np_dt, compare = _three_ops()[which]
    xs = [inputs(800 + 10 * k) for k in range(2)]
    refs = [reference(oracle, x) for x in xs]
    assert not np.array_equal(refs[0].view(np.uint8), refs[1].view(np.uint8))
    devs = [[dev_src(a) for a in x] for x in xs]
    streams = [torch.cuda.Stream() for _ in range(2)]
    op = make_op()
    try:
        outs = [[Dst(dshape, np_dt) for _ in range(30)] for _ in range(2)]
        sync()
        errors = []
        gate = threading.Barrier(2)

        def worker(k):
            try:
                gate.wait()
                for it in range(30):
                    _submit(name, op, devs[k], outs[k][it], streams[k])
            except Exception as e:      # noqa: BLE001 -- reported below, on the main thread
                errors.append(e)

        ts = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        sync()
        assert not errors, errors
        for k in range(2):
            for it in range(30):
                what = "%s thread %d launch %d" % (name, k, it)
                compare(outs[k][it].numpy(what), refs[k], what)
    finally:
        op.close()


# ---- 6. pointers ----
@pytest.mark.parametrize("np_dt", E.DTYPES, ids=DT_IDS)
def test_pool_pointers_off_the_16_byte_grid(oracle, np_dt):
    """a shape of the 16-byte path with src and / or dst aligned to the element only: the per-element path must give
    the same bytes; a 4-byte type at an odd address is refused"""
    case = ((2, 13, 12, 16), (3, 3), (2, 2), (1, 1), (7, 6))
    es = np.dtype(np_dt).itemsize
    assert E.pool_takes_vector_path(case, np_dt)
    x = E.pool_input(case, np_dt)
    L = capi.lib()
    st = capi._stream_ptr(None)
    for algo, inc in ALGOS:
        ref = pool_reference(oracle, case, x, inc)
        for off in ((1, 4, 8) if es == 1 else (4, 8)):
            for so, do in ((off, 0), (0, off), (off, off)):
                got = run_pool(case, np_dt, algo, dev_src(x, so), dst_off=do)
                assert_pool_equal(got, ref, inc, "algo %d src + %d dst + %d" % (algo, so, do))
    op = make_pool(case, np_dt, dfa.Pool.MAX)
    try:
        src, dst = dev_src(x), Dst(op.dst_shape, np_dt)
        sync()
        refused = [(None, dst.ptr), (src.data_ptr(), None)]
        if es == 4:
            refused += [(src.data_ptr() + so, dst.ptr + do) for so, do in ((1, 0), (2, 0), (0, 1), (0, 2), (3, 3))]
        for sp, dp in refused:
            rc = L.dfx_pool_submit(op._h, ctypes.c_void_p(sp), ctypes.c_void_p(dp), st)
            assert rc == ERR_INVALID, (sp, dp, rc)
        if es == 4:
            assert b"aligned" in L.dfx_last_error()
        sync()
        assert dst.still_poison(), "a refused submit wrote to dst"
        op.submit(src, dst.t)                                      # the aligned call goes through
        sync()
        E.assert_selected_equal(dst.numpy("after refusals"), pool_reference(oracle, case, x, None), "after refusals")
    finally:
        op.close()


def test_concat_refuses_misaligned_and_null_pointers(oracle):
    np_dt, channels = np.uint8, [32, 16]
    srcs_np = E.concat_inputs(E.CONCAT_PIXELS, channels, np_dt)
    flat = np.concatenate([s.reshape(-1) for s in srcs_np])
    offs = [0, srcs_np[0].size]
    op = dfa.Concat(2, 3, 5, channels, np_dt, True)
    try:
        a, b = dev_src(srcs_np[0], 0), dev_src(srcs_np[1], 0)
        a8, b4 = dev_src(srcs_np[0], 8), dev_src(srcs_np[1], 4)
        g, g8 = dev_src(flat, 0), dev_src(flat, 8)
        dst, dst_odd = Dst(op.dst_shape, np_dt), Dst(op.dst_shape, np_dt, offset=1)
        sync()
        L = capi.lib()
        st = capi._stream_ptr(None)
        for pa, pb, pd in ((a8, b, dst), (a, b4, dst), (a, b, dst_odd), (a8, b4, dst_odd)):
            ptrs = (ctypes.c_void_p * 2)(pa.data_ptr(), pb.data_ptr())
            rc = L.dfx_concat_submit(op._h, ptrs, ctypes.c_void_p(pd.ptr), st)
            assert rc == ERR_INVALID and b"16-byte aligned" in L.dfx_last_error(), rc
        ptrs = (ctypes.c_void_p * 2)(a.data_ptr(), None)
        assert L.dfx_concat_submit(op._h, ptrs, ctypes.c_void_p(dst.ptr), st) == ERR_INVALID          # null branch
        ptrs = (ctypes.c_void_p * 2)(a.data_ptr(), b.data_ptr())
        assert L.dfx_concat_submit(op._h, ptrs, None, st) == ERR_INVALID                              # null dst
        assert L.dfx_concat_submit(op._h, None, ctypes.c_void_p(dst.ptr), st) == ERR_INVALID
        o64 = (ctypes.c_uint64 * 2)(*offs)
        for base, oo, pd in ((g8.data_ptr(), offs, dst), (g.data_ptr(), [0, offs[1] + 8], dst), (g.data_ptr(), offs, dst_odd),
                             (g8.data_ptr(), [8, offs[1] + 8], dst)):     # (the last: base + offset IS aligned, base is not)
            o = (ctypes.c_uint64 * 2)(*oo)
            rc = L.dfx_concat_submit_gathered(op._h, ctypes.c_void_p(base), o, ctypes.c_void_p(pd.ptr), st)
            assert rc == ERR_INVALID and b"16-byte aligned" in L.dfx_last_error(), (oo, rc)
        assert L.dfx_concat_submit_gathered(op._h, None, o64, ctypes.c_void_p(dst.ptr), st) == ERR_INVALID
        assert L.dfx_concat_submit_gathered(op._h, ctypes.c_void_p(g.data_ptr()), o64, None, st) == ERR_INVALID
        with pytest.raises(dfa.DfxError):
            op.submit([a8, b], dst.t)
        sync()
        assert dst.still_poison() and dst_odd.still_poison(), "a refused submit wrote to dst"
        dst.check_guards()
        dst_odd.check_guards()
        ref = oracle.concat(srcs_np, True)
        op.submit([a, b], dst.t)                                   # the aligned calls go through
        sync()
        E.assert_selected_equal(dst.numpy(), ref, "after refusals")
        dst2 = Dst(op.dst_shape, np_dt)
        op.submit_gathered(g, offs, dst2.t)
        sync()
        E.assert_selected_equal(dst2.numpy(), ref, "gathered after refusals")
    finally:
        op.close()


def test_eltwise_refuses_misaligned_and_null_pointers(oracle):
    np_dt, elems = np.float32, 403
    xs = E.eltwise_inputs(elems, np_dt, 2)
    op = dfa.EltwiseSum(2, elems, np_dt, True)
    try:
        a, b, a4, b8 = dev_src(xs[0]), dev_src(xs[1]), dev_src(xs[0], 4), dev_src(xs[1], 8)
        dst, dst4 = Dst((elems,), np_dt), Dst((elems,), np_dt, offset=4)
        sync()
        L = capi.lib()
        st = capi._stream_ptr(None)
        for pa, pb, pd in ((a4, b, dst), (a, b8, dst), (a, b, dst4), (a4, b8, dst4)):
            ptrs = (ctypes.c_void_p * 2)(pa.data_ptr(), pb.data_ptr())
            rc = L.dfx_eltwise_submit(op._h, ptrs, ctypes.c_void_p(pd.ptr), st)
            assert rc == ERR_INVALID and b"16-byte aligned" in L.dfx_last_error(), rc
        ptrs = (ctypes.c_void_p * 2)(None, b.data_ptr())
        assert L.dfx_eltwise_submit(op._h, ptrs, ctypes.c_void_p(dst.ptr), st) == ERR_INVALID
        ptrs = (ctypes.c_void_p * 2)(a.data_ptr(), b.data_ptr())
        assert L.dfx_eltwise_submit(op._h, ptrs, None, st) == ERR_INVALID
        assert L.dfx_eltwise_submit(op._h, None, ctypes.c_void_p(dst.ptr), st) == ERR_INVALID
        sync()
        assert dst.still_poison() and dst4.still_poison(), "a refused submit wrote to dst"
        op.submit([a, b], dst.t)                                   # the aligned call goes through
        sync()
        E.assert_computed_equal(dst.numpy(), oracle.eltwise_sum(xs, True), "after refusals")
    finally:
        op.close()


# ---- 7. aliasing ----
@pytest.mark.parametrize("np_dt", [np.float32, np.int8], ids=["f32", "s8"])
def test_eltwise_in_place_and_one_buffer_twice(oracle, np_dt):
    """the residual add as frameworks issue it: dst is the first, or the last, input; and x + x"""
    import torch
    elems, n = 2 * 9 * 7 * 20 + 3, 3
    xs = E.eltwise_inputs(elems, np_dt, n)
    ref = oracle.eltwise_sum(xs, True)
    for where in (0, n - 1):
        dst = Dst((elems,), np_dt)
        dst.t.copy_(torch.from_numpy(xs[where].view(np.uint8)))
        srcs = [dst.t if i == where else dev_src(x) for i, x in enumerate(xs)]
        E.assert_computed_equal(run_eltwise(xs, np_dt, True, srcs=srcs, dst=dst), ref, "dst is input %d" % where)
    a, c = dev_src(xs[0]), dev_src(xs[2])
    E.assert_computed_equal(run_eltwise(xs, np_dt, True, srcs=[a, c, a]), oracle.eltwise_sum([xs[0], xs[2], xs[0]], True),
                            "one buffer as two inputs")


def test_concat_one_buffer_as_two_branches(oracle):
    srcs = E.concat_inputs(E.CONCAT_PIXELS, [8, 4, 8], np.float32)
    a, b = dev_src(srcs[0]), dev_src(srcs[1])
    E.assert_selected_equal(run_concat([srcs[0], srcs[1], srcs[0]], np.float32, True, srcs=[a, b, a]),
                            oracle.concat([srcs[0], srcs[1], srcs[0]], True), "one buffer as two branches")


# ---- 8. views ----
def _views(arrays, gaps):
    """the arrays' bytes as 16-byte-aligned (and no coarser) views into ONE allocation, `gaps` bytes of 0xEE apart"""
    import torch
    raws = [np.ascontiguousarray(a).reshape(-1).view(np.uint8) for a in arrays]
    pool = torch.full((sum(r.size + 32 for r in raws) + sum(gaps) + 256,), 0xEE, dtype=torch.uint8, device="cuda")
    assert pool.data_ptr() % 32 == 0
    views, off = [], 0
    for r, g in zip(raws, gaps):
        off = (off + g + 15) // 16 * 16
        if (off // 16) % 2 == 0:
            off += 16
        v = pool[off:off + r.size]
        assert v.data_ptr() % 32 == 16
        v.copy_(torch.from_numpy(r))
        views.append(v)
        off += r.size
    return views


def test_concat_branches_are_views_of_one_allocation(oracle):
    srcs = E.concat_inputs((2, 13, 9), [32, 64, 16, 48], np.int8)
    views = _views(srcs, [16 * 3, 16 * 7, 16 * 1, 16 * 5])
    E.assert_selected_equal(run_concat(srcs, np.int8, True, srcs=views), oracle.concat(srcs, True), "views")


def test_eltwise_inputs_are_views_of_one_allocation(oracle):
    xs = E.eltwise_inputs(2 * 13 * 9 * 5 + 1, np.float32, 3)
    views = _views(xs, [16 * 3, 16 * 7, 16 * 1])
    E.assert_computed_equal(run_eltwise(xs, np.float32, False, srcs=views), oracle.eltwise_sum(xs, False), "views")
