"""GPU: the int8 layer norm / RMS norm (dfx_lnorm_*) against the numpy reference of tests/lnorm_ref.py, bit for bit
(tests/test_lnorm_cpu.py pins that reference against a pure-Python witness), and against dfx_wsum where the two ops coincide
exactly.  Everything goes through the C ABI; every dst sits between guard bands with poison fill and the WHOLE storage is
compared, so pad elements and gaps are proved unwritten; src pad channels hold 0xFF.  Path, lanes, grid, block, LDS bytes,
algorithmic bytes and kernel name are asserted from info(), the kernel that ran from lnorm_launches().  Every case runs on
both forced paths and on auto, and the results are compared with one another."""
import functools
import importlib
import threading

import numpy as np
import pytest

import hipref
import lnorm_ref as L

pytestmark = pytest.mark.gpu
dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
GUARD = 1 << 12       # guard bytes on each side of every output
Case = L.LnCase


@functools.lru_cache(maxsize=None)
def problem(case):
    """(src, params, reference): computed once per case and shared; never written to"""
    src, params = L.make_src(case), L.make_params(case)
    want = L.reference(case, src, params)
    for a in (src, want) + tuple(p for p in params if p is not None):
        a.setflags(write=False)
    return src, params, want


def make_op(case, params, force_path=-1):
    op = dfa.LayerNorm(case.rows, case.c, L.NP_OF[case.src_dt], L.NP_OF[case.dst_dt], case.eps, mode=case.mode, src_ld=case.src_ld,
                       dst_ld=case.dst_ld, force_path=force_path)
    if params is not None:
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
    """-> (buf, out): out (poisoned, `offset` bytes off a 16-byte boundary) between two GUARD-byte bands"""
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


def run_guarded(op, case, src_dev, offset=0, stream=None):
    """one submit into a guarded dst -> its whole storage {rows, dst_ld} (pad columns included) as a numpy array"""
    import torch
    what = op.info().kernel_name.decode()
    buf, out = guarded(case.rows * case.dst_ld * L.SIZE_OF[case.dst_dt], offset)
    torch.cuda.synchronize()
    op.submit(src_dev, out, stream=stream)
    torch.cuda.synchronize()
    assert_guards(buf, offset, out.numel(), what)
    return out.cpu().numpy().view(L.NP_OF[case.dst_dt]).reshape(case.rows, case.dst_ld)


def expected_storage(case, want):
    """the reference in the valid channels, poison everywhere else"""
    full = np.full((case.rows, case.dst_ld * L.SIZE_OF[case.dst_dt]), hipref.POISON_BYTE, dtype=np.uint8).view(L.NP_OF[case.dst_dt])
    full = full.reshape(case.rows, case.dst_ld).copy()
    full[:, :case.c] = want
    return full


def compare(case, got, want, what, nan_positions_only=False):
    full = expected_storage(case, want)
    if nan_positions_only:  # a generated NaN's sign and payload are the implementation's: its place must agree, all else bit for bit
        gn, wn = np.isnan(got[:, :case.c]), np.isnan(want)
        assert np.array_equal(gn, wn), what + ": NaNs in other places"
        got = got.copy()
        got[:, :case.c][gn] = 0
        full[:, :case.c][wn] = 0
    hipref.assert_bit_equal(np.ascontiguousarray(got), full, what)


def check(case, path, force_path=-1, grid_cap=0, data=None, nan_positions_only=False):
    """one guarded submit of `case`; the plan from info(), the kernel that ran and the whole storage against the reference"""
    src, params, want = data if data is not None else problem(case)
    shifted = params[2] is not None
    assert shifted == case.shift
    op = make_op(case, params, force_path)
    try:
        info = op.info()
        what = "%s [%s]" % (case.ident(), info.kernel_name.decode())
        assert info.path == path, what
        assert info.kernel_name.decode() == L.kernel_name(case, path), what
        assert info.grid == L.planned_grid(case, path, grid_cap), (what, info.grid)
        assert info.block == 256 and info.lds_bytes == L.lds_bytes(case, path), (what, info.lds_bytes)
        assert info.algorithmic_bytes == L.algorithmic_bytes(case), what
        before = dfa.lnorm_launches()
        got = run_guarded(op, case, on_device(src), case.dst_off)
        after = dfa.lnorm_launches()
        ran = path if case.dst_off % 16 == 0 else L.GENERIC
        assert [after[p] - before[p] for p in range(2)] == [int(p == ran) for p in range(2)], what
        compare(case, got, want, what, nan_positions_only)
        return got
    finally:
        op.close()


def check_every_path(case, grid_cap=0, data=None, nan_positions_only=False):
    outs = [check(case, L.auto_path(case), grid_cap=grid_cap, data=data, nan_positions_only=nan_positions_only)]
    for path in (L.ROW, L.GENERIC):
        if L.in_class(case, path):
            outs.append(check(case, path, force_path=path, grid_cap=grid_cap, data=data, nan_positions_only=nan_positions_only))
        else:
            with pytest.raises(dfa.DfxError, match="dfx error 2"):
                make_op(case, None, force_path=path)
    assert len({np.ascontiguousarray(o).tobytes() for o in outs}) == 1, case.ident()
    return outs[0]


def chunks(cases, n):
    return [tuple(cases[i::n]) for i in range(n)]


def planted(case, src_valid, gamma, beta, shift=None):
    """(src, params, want) of a case whose valid channels, gamma, beta and shifts a test gives"""
    src = np.full((case.rows, case.src_ld), 0xFF, dtype=np.uint8).view(L.NP_OF[case.src_dt])
    src[:, :case.c] = src_valid
    params = (np.asarray(gamma, dtype=np.float32), None if beta is None else np.asarray(beta, dtype=np.float32),
              None if shift is None else np.asarray(shift, dtype=np.uint8))
    with np.errstate(all="ignore"):
        want = L.reference(case, src, params)
    return src, params, want


# ---- 1. the shape grid ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", chunks(L.grid_cases(), 11), ids=lambda g: "grid%d" % len(g))
def test_shape_grid(group):
    """c in 1, 15, 16, 17, 63, 64, 65, 96, 100, 768, 1000, 1024, 1025, 4096, 4097 against rows in 1, 3, 4, 5, 63, 257 (and both
    sides of the switches of W at 128 / 256 / 512 bytes): the partial last workgroup trip at every W, the masked last group,
    the first re-read group beyond four per lane; dtypes, mode, shifts, ld > c and a dst offset rotate (tests/test_lnorm_cpu.py
    asserts the coverage)"""
    for case in group:
        check_every_path(case)


# ---- 2. extremes ------------------------------------------------------------------------------------------------------------------
def test_the_largest_statistics():
    """c = 16384 with shift 7: alternating -128 / 127 (the largest Q and u_k) and all 255 u8 (the largest |S|, D = 0: the
    output is beta); gamma / beta through global memory (8 * c bytes do not fit the LDS plan)"""
    c = 16384
    rng = np.random.RandomState(1)
    gamma, beta = (rng.standard_normal(c) * 50).astype(np.float32), (rng.standard_normal(c) * 20).astype(np.float32)
    shift = np.full(c, 7, dtype=np.uint8)
    alt = np.where(np.arange(c) % 2 == 0, -128, 127)
    for mode in (L.LAYER, L.RMS):
        case = Case("maxq", 2, c, L.S8, L.S8, mode=mode, shift=True, eps=1.0)
        assert L.lds_bytes(case, L.ROW) == 0
        check_every_path(case, data=planted(case, np.stack([alt, -1 - alt]), gamma, beta, shift))
        case = Case("maxs", 2, c, L.U8, L.F32, mode=mode, shift=True, eps=1.0)
        data = planted(case, np.full((2, c), 255), gamma, beta, shift)
        got = check_every_path(case, data=data)
        if mode == L.LAYER:
            hipref.assert_bit_equal(np.ascontiguousarray(got[:, :c]), np.stack([beta, beta]), "a constant row is beta")


def test_outlier_single_channel_and_eps_extremes():
    rng = np.random.RandomState(2)
    c = 768
    gamma, beta = (rng.standard_normal(c) * 40).astype(np.float32), (rng.standard_normal(c) * 10).astype(np.float32)
    rows = rng.randint(-3, 4, size=(5, c))
    rows[0] = 0
    rows[0, 5] = 127                                                      # one outlier in a row of zeros
    rows[1, 700] = -128
    for mode in (L.LAYER, L.RMS):
        case = Case("outlier", 5, c, L.S8, L.S8, mode=mode, eps=2.0 ** -20)
        check_every_path(case, data=planted(case, rows, gamma, beta))
    # c = 1: y = beta in LAYER mode
    case = Case("one", 5, 1, L.S8, L.F32, src_ld=16, dst_ld=4)
    got = check_every_path(case, data=planted(case, np.array([[-128], [-1], [0], [1], [127]]), [3.0], [0.25]))
    assert got[:, 0].tolist() == [0.25] * 5
    case = Case("one", 5, 1, L.U8, L.U8, mode=L.RMS, src_ld=16, dst_ld=16, eps=2.0 ** -30)
    got = check_every_path(case, data=planted(case, np.array([[64], [1], [0], [2], [128]]), [7.0], [0.5]))
    assert got[:, 0].tolist() == [8, 8, 0, 8, 8]                          # x / |x| * 7 + 0.5 = 7.5 -> 8; 0 -> 0.5 -> 0
    # eps at the smallest denormal and at 3e38
    for eps in (np.float32(1e-45), np.float32(3e38)):
        for mode in (L.LAYER, L.RMS):
            for dst_dt in (L.F32, L.S8):
                case = Case("eps", 5, 96, L.S8, dst_dt, mode=mode, eps=float(eps), src_ld=96, dst_ld=96)
                r = rng.randint(-128, 128, size=(5, 96))
                r[1] = 9                                                   # constant: v = 0, sqrt(eps) alone
                r[2] = 0
                check_every_path(case, data=planted(case, r, gamma[:96] * (1 if dst_dt == L.S8 else 1e19), beta[:96]))


# ---- 3. ties and conversion ---------------------------------------------------------------------------------------------------------
def test_tie_rows_round_to_even():
    """xhat = +-1 exactly, gamma = k + 0.5: every output on a tie; at c = 4 and as a c = 768 row (W = 64)"""
    eps = 2.0 ** -30
    for mode, pair in ((L.RMS, (2, -2)), (L.LAYER, (5, 1))):
        for c in (4, 768):
            row = np.tile(np.array(pair), c // 2)
            src = np.stack([row, row[::-1]])
            gamma = (np.arange(c) % 4 + 0.5).astype(np.float32)
            one = Case("tie", 2, c, L.S8, L.F32, mode=mode, eps=eps, src_ld=max(c, 16), dst_ld=c)
            xhat = planted(one, src, np.ones(c), None)[2]
            assert np.array_equal(np.abs(xhat), np.ones((2, c), dtype=np.float32)) and xhat[0, 0] == 1 and xhat[1, 0] == -1
            for dst_dt in (L.S8, L.U8, L.F32):
                case = Case("tie", 2, c, L.S8, dst_dt, mode=mode, eps=eps, src_ld=max(c, 16), dst_ld=max(c, 16))
                got = check_every_path(case, data=planted(case, src, gamma, None))
                if dst_dt == L.S8:
                    assert got[0, c - 4:c].tolist() == [0, -2, 2, -4] and got[1, :4].tolist() == [0, 2, -2, 4]
                elif dst_dt == L.U8:
                    assert got[0, :4].tolist() == [0, 0, 2, 0] and got[1, :4].tolist() == [0, 2, 0, 4]
                else:
                    assert got[0, :4].tolist() == [0.5, -1.5, 2.5, -3.5]


def test_nan_inf_and_saturation():
    """gamma / beta holding NaN, +-Inf and values that saturate both ways: NaN -> 0, then clamp, on both paths; an f32 dst
    takes the bits verbatim (where the arithmetic generates a NaN, its place is compared)"""
    c = 100
    rng = np.random.RandomState(4)
    rows = rng.randint(-128, 128, size=(6, c))
    rows[1] = 3                                                           # u = 0: 0 * Inf is a NaN
    gamma = (rng.standard_normal(c) * 30).astype(np.float32)
    beta = (rng.standard_normal(c) * 10).astype(np.float32)
    gamma[3], gamma[4], gamma[5], gamma[6], gamma[7] = np.nan, np.inf, -np.inf, 3e38, -3e38
    beta[10], beta[11], beta[12], beta[13], beta[14] = np.nan, np.inf, -np.inf, 1e9, -1e9
    gamma[20], beta[20] = np.inf, -np.inf                                 # Inf - Inf
    for mode in (L.LAYER, L.RMS):
        for dst_dt in (L.S8, L.U8, L.F32):
            case = Case("nan", 6, c, L.S8, dst_dt, mode=mode, src_ld=112, dst_ld=112 if dst_dt != L.F32 else 100)
            data = planted(case, rows, gamma, beta)
            want = data[2]
            if dst_dt == L.F32:
                assert np.isnan(want[:, 3]).all() and np.isnan(want[:, 10]).all() and np.isinf(want[0, 4]) and np.isinf(want[:, 11]).all()
                assert mode == L.RMS or np.isnan(want[1, 4])                  # 0 * Inf
            else:
                lo, hi = (0, 255) if dst_dt == L.U8 else (-128, 127)
                assert (want[:, 3] == 0).all() and (want[:, 10] == 0).all() and (want[:, 11] == hi).all() and (want[:, 12] == lo).all()
                assert (want[:, 13] == hi).all() and (want[:, 14] == lo).all()
            check_every_path(case, data=data, nan_positions_only=dst_dt == L.F32)


# ---- 4. alignment --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dst_dt", [L.U8, L.F32], ids=["u8", "f32"])
def test_misaligned_pointers_fall_back_to_generic_for_that_submit(dst_dt):
    """src 4 bytes off, then dst 1 byte (u8) or 4 bytes (f32) off a 16-byte boundary: the forced row handle launches the
    generic kernel for that submit (dfx_debug_lnorm_launches), info() keeps the plan, the bytes are the same"""
    case = Case("off", 9, 768, L.S8, dst_dt, shift=True)
    src, params, want = problem(case)
    op = make_op(case, params, force_path=L.ROW)
    try:
        for src_off, dst_off in ((4, 0), (0, L.SIZE_OF[dst_dt]), (0, 0)):
            before = dfa.lnorm_launches()
            got = run_guarded(op, case, on_device(src, src_off), dst_off)
            after = dfa.lnorm_launches()
            ran = L.GENERIC if src_off or dst_off else L.ROW
            assert [after[p] - before[p] for p in range(2)] == [int(p == ran) for p in range(2)], (src_off, dst_off)
            assert op.info().path == L.ROW
            compare(case, got, want, "%s offsets %d %d" % (case.ident(), src_off, dst_off))
    finally:
        op.close()


def test_odd_leading_dimensions_run_generic():
    """src_ld % 16 != 0: forced ROW is dfx error 2; auto runs the generic kernel"""
    for case in (Case("odd", 7, 100, L.S8, L.S8, src_ld=100, dst_ld=112), Case("odd", 7, 96, L.U8, L.F32, src_ld=96, dst_ld=98),
                 Case("odd", 7, 768, L.S8, L.U8, src_ld=769, dst_ld=768)):
        assert not L.in_class(case, L.ROW)
        check_every_path(case)
        assert check(case, L.GENERIC) is not None


# ---- 5. submit checks ------------------------------------------------------------------------------------------------------------------
def test_state_errors_launch_nothing():
    """submit before set_params is DFX_ERR_STATE; a null pointer, a misaligned f32 dst, a dst that overlaps src and a shift of
    8 are DFX_ERR_INVALID; nothing is launched, the poison is intact, and a valid submit works afterwards"""
    import torch
    case = Case("state", 9, 96, L.S8, L.F32)
    src, params, want = problem(case)
    dev = on_device(src)
    before = dfa.lnorm_launches()
    op = make_op(case, None, force_path=L.ROW)
    try:
        buf, dst = guarded(case.rows * case.c * 4 + 16)
        with pytest.raises(dfa.DfxError, match="dfx error 5"):
            op.submit(dev, dst)
        with pytest.raises(dfa.DfxError, match="dfx error 1"):
            op.set_params(params[0], params[1], np.full(case.c, 8, dtype=np.uint8))
        with pytest.raises(dfa.DfxError, match="dfx error 5"):
            op.submit(dev, dst)                                           # a refused set_params does not count
        op.set_params(params[0], params[1], np.full(case.c, 7, dtype=np.uint8))
        op.set_params(*params)
        with pytest.raises(dfa.DfxError, match="dfx error 1"):
            op.submit(0, dst)
        with pytest.raises(dfa.DfxError, match="dfx error 1"):
            op.submit(dev, 0)
        for off in (1, 2, 3):
            with pytest.raises(dfa.DfxError, match="dfx error 1"):
                op.submit(dev, dst[off:])                                 # an f32 dst that is not 4-byte aligned
        big = torch.zeros(case.rows * case.c * 5 + 64, dtype=torch.uint8, device="cuda")
        big[:case.rows * case.c].copy_(dev[:case.rows * case.c])
        with pytest.raises(dfa.DfxError, match="dfx error 1"):
            op.submit(big, big)                                           # in place
        with pytest.raises(dfa.DfxError, match="dfx error 1"):
            op.submit(big, big[case.rows * case.c - 4:])                  # the last src element's dword
        with pytest.raises(dfa.DfxError, match="dfx error 1"):
            op.submit(big[16:], big)                                      # src inside dst
        torch.cuda.synchronize()
        assert bool((dst == hipref.POISON_BYTE).all()) and int(big[case.rows * case.c:].sum()) == 0
        assert dfa.lnorm_launches() == before
        op.submit(big, big[case.rows * case.c:])                          # right behind src: no overlap
        torch.cuda.synchronize()
        got = big[case.rows * case.c:case.rows * case.c * 5].cpu().numpy().view(np.float32).reshape(case.rows, case.c)
        hipref.assert_bit_equal(got, want, "behind src")
        compare(case, run_guarded(op, case, dev), want, "after the refusals")
    finally:
        op.close()


# ---- 6. DFX_LNORM_GRID ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [1, 3])
def test_grid_cap(tuning, cap):
    """a dozen trips and a ragged last one under a cap of 1 and of 3 workgroups: they loop and reuse their LDS copy of gamma /
    beta (row), and their threads make several passes (generic)"""
    tuning.setenv("DFX_LNORM_GRID", cap)
    for case in (Case("cap", 4 * 12 + 1, 768, L.S8, L.S8, shift=True), Case("cap", 32 * 12 + 5, 96, L.U8, L.F32, mode=L.RMS),
                 Case("cap", 8 * 12 + 3, 400, L.S8, L.U8, src_ld=400, dst_ld=416), Case("cap", 256 * 3 + 7, 17, L.S8, L.S8, src_ld=32, dst_ld=32)):
        assert L.planned_grid(case, L.ROW) >= 12 and L.planned_grid(case, L.ROW, cap) == cap
        check_every_path(case, grid_cap=cap)


# ---- 7. threads and streams ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [L.ROW, L.GENERIC], ids=["row", "generic"])
def test_one_handle_from_two_threads_on_two_streams(path):
    """submit never writes to the handle: two host threads, each on its own stream, give the same bytes"""
    import torch
    case = Case("mt", 130, 768, L.S8, L.S8, shift=True)
    src, params, want = problem(case)
    dev = on_device(src)
    op = make_op(case, params, force_path=path)
    try:
        streams = [torch.cuda.Stream() for _ in range(2)]
        outs = [[guarded(case.rows * case.dst_ld) for _ in range(4)] for _ in range(2)]
        torch.cuda.synchronize()
        errors = []

        def work(i):
            try:
                for _, o in outs[i]:
                    op.submit(dev, o, stream=streams[i])
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        torch.cuda.synchronize()
        assert not errors, errors
        for per_stream in outs:
            for buf, o in per_stream:
                assert_guards(buf, 0, o.numel(), case.ident())
                compare(case, o.cpu().numpy().view(np.int8).reshape(case.rows, case.dst_ld), want, case.ident())
    finally:
        op.close()


# ---- 8. auto ----------------------------------------------------------------------------------------------------------------------------
def test_auto_follows_the_note():
    """the AUTO RULE of include/dfx.h (DFX_LNORM_AUTO_NOTE), mirrored by lnorm_ref.auto_path: on both sides of each bound"""
    for case in L.auto_cases():
        path = L.auto_path(case)
        assert path == L.GENERIC or L.in_class(case, L.ROW)
        check(case, path)


# ---- 9. the pin against dfx_wsum -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dst_dt", [L.S8, L.F32], ids=["s8", "f32"])
def test_equals_scaled_sum_where_the_two_coincide(dst_dt):
    """rows that are permutations of one multiset (32 x 7 and 32 x 3: S / c = 5, variance 4, eps absorbed, a * c = 2^-1) with
    dyadic gamma and beta: every product and sum is exact, so the layer norm equals scaled_sum with scale[k] = a * c *
    gamma[k] and bias[k] = beta[k] - (S / c) * scale[k], bit for bit"""
    import torch
    c, rows = 64, 37
    rng = np.random.RandomState(9)
    base = np.array([7] * 32 + [3] * 32)
    src_valid = np.stack([rng.permutation(base) for _ in range(rows)])
    gamma = (rng.randint(-40, 41, size=c) / 8.0).astype(np.float32)
    beta = (rng.randint(-40, 41, size=c) / 4.0).astype(np.float32)
    scale = (np.float32(0.5) * gamma).astype(np.float32)
    bias = (beta - np.float32(5.0) * scale).astype(np.float32)
    assert np.array_equal(scale.astype(np.float64), 0.5 * gamma.astype(np.float64))
    assert np.array_equal(bias.astype(np.float64), beta.astype(np.float64) - 5.0 * scale.astype(np.float64))
    case = Case("wsum", rows, c, L.S8, dst_dt, eps=2.0 ** -30)
    data = planted(case, src_valid, gamma, beta)
    ws = dfa.ScaledSum((1, rows, 1, c), [np.int8], L.NP_OF[dst_dt], [c], n_bias=c)
    try:
        ws.set_params([scale], bias)
        out = torch.empty(rows * c * L.SIZE_OF[dst_dt], dtype=torch.uint8, device="cuda")
        ws.submit([on_device(data[0])], out)
        torch.cuda.synchronize()
        pin = out.cpu().numpy().view(L.NP_OF[dst_dt]).reshape(rows, c)
    finally:
        ws.close()
    hipref.assert_bit_equal(pin, data[2], "dfx_wsum against the reference")
    got = check_every_path(case, data=data)
    hipref.assert_bit_equal(np.ascontiguousarray(got[:, :c]), pin, "layer norm against dfx_wsum")
