"""CPU-only: the oracle of concat, pooling and eltwise sum on the inputs of tests/elementwise_cases.py.

tests/test_gpu_elementwise.py compares the HIP kernels with oracle.maxpool / avgpool / eltwise_sum / concat on NaNs,
signed zeros, infinities, denormals and saturating integers, so the oracle must first be right about those.  It is
compared here with independent numpy formulations (refmath.maxpool_select, refmath.relu_select, refmath.avgpool,
refmath.eltwise_sum) and with values pinned by hand.

One disagreement showed when this file was written, and the independent formulation was the wrong one: for an s32
window of four INT32_MAX the quotient is exactly 2^31, and refmath.avgpool clipped it in f32, where INT32_MAX is
2^31 as well, so the cast wrapped to INT32_MIN.  The oracle gave the pinned INT32_MAX; refmath.avgpool now clips in
f64.  Everything else agreed.  (refmath.maxpool, the older formulation, propagates every NaN through np.maximum and so
cannot stand in for the vmaxps order; it is left as it is and not used here.)"""
import numpy as np
import pytest

import elementwise_cases as E
import refmath
from test_oracle import POOL_CASES

NAN_A, NAN_B = 0x7FD5A5A5, 0xFFEABCDE
ONE = 0x3F800000
SMALL_POOL_CASES = [c for c in POOL_CASES if c[0][1] <= 100] + E.POOL_GEOM_CASES
DT_IDS = [np.dtype(d).name for d in E.DTYPES]


def bits_of(a):
    return [int(v) for v in np.asarray(a, dtype=np.float32).reshape(-1).view(np.uint32)]


def window(bits):
    """a 1 x 1 x len x 1 f32 tensor holding the given bit patterns: one pooling window"""
    return E.f32_bits(*bits).reshape(1, 1, len(bits), 1)


def both_maxpools(oracle, x):
    k = (1, x.shape[2])
    return [f(x, k, k, (0, 0), (1, 1)) for f in (oracle.maxpool, refmath.maxpool_select)]


def test_hand_pinned_f32_order(oracle):
    """vmaxps(acc, x): the second operand wins ties and NaNs.  Expected values are literals."""
    for got in both_maxpools(oracle, window([NAN_A, ONE])):
        assert bits_of(got) == [0x3F800000]                    # max over [NaN, 1] is 1
    for got in both_maxpools(oracle, window([ONE, NAN_B])):
        assert bits_of(got) == [0xFFEABCDE]                    # max over [1, NaN] is that NaN, bits kept
    for got in both_maxpools(oracle, window([0x00000000, 0x80000000])):
        assert bits_of(got) == [0x80000000]                    # max over [+0, -0] is -0
    for got in both_maxpools(oracle, window([0x80000000, 0x00000000])):
        assert bits_of(got) == [0x00000000]                    # max over [-0, +0] is +0
    for got in both_maxpools(oracle, window([ONE, NAN_A, 0xBF800000])):
        assert bits_of(got) == [0xBF800000]                    # a NaN in the middle is dropped: [1, NaN, -1] is -1
    x = E.f32_bits(0x80000000, NAN_A, NAN_B, 0xBF800000, 0x00000001, 0x80000001, 0xFF800000, 0x7F800000)
    want = [0x80000000, 0x7FD5A5A5, 0xFFEABCDE, 0x00000000, 0x00000001, 0x00000000, 0x00000000, 0x7F800000]
    assert bits_of(refmath.relu_select(x)) == want             # ReLU(-0) = -0, ReLU(NaN) = NaN, denormals survive
    x4 = x.reshape(1, 1, 2, 4)
    assert bits_of(oracle.concat([x4, x4], True)) == want[:4] + want[:4] + want[4:] + want[4:]
    assert bits_of(oracle.concat([x4], False)) == bits_of(x)
    s = oracle.eltwise_sum([x, E.f32_bits(*([0x80000000] * 8))], True)       # x + -0 == x, then ReLU
    assert bits_of(s)[0] == 0x80000000 and bits_of(s)[3:] == want[3:] and np.isnan(s[1:3]).all()


def test_hand_pinned_integer_averages(oracle):
    def avg(vals, np_dt, include_padding):
        x = np.array(vals, dtype=np_dt).reshape(1, 2, 2, 1)
        outs = [f(x, (2, 2), (2, 2), (0, 0), (1, 1), include_padding) for f in (oracle.avgpool, refmath.avgpool)]
        assert outs[0].dtype == np_dt and outs[0].tolist() == outs[1].tolist()
        return int(outs[0][0, 0, 0, 0])

    for inc in (True, False):
        assert avg([2147483647] * 4, np.int32, inc) == 2147483647      # float(sum) / 4 is exactly 2^31: saturates
        assert avg([-2147483648] * 4, np.int32, inc) == -2147483648
        assert avg([2147483647, 2147483647, 2147483647, 2147483646], np.int32, inc) == 2147483647
        assert avg([0, 0, 0, 2], np.uint8, inc) == 0                   # 0.5 -> 0: ties to even
        assert avg([0, 0, 2, 4], np.uint8, inc) == 2                   # 1.5 -> 2
        assert avg([0, 0, 0, 2], np.int8, inc) == 0
        assert avg([0, 0, -2, -4], np.int8, inc) == -2                 # -1.5 -> -2
        assert avg([0, 0, 0, -2], np.int32, inc) == 0                  # -0.5 -> 0
        assert avg([255] * 4, np.uint8, inc) == 255
        assert avg([-128] * 4, np.int8, inc) == -128
        assert avg([-128, 127, -128, 127], np.int8, inc) == 0          # -0.5 -> 0


def test_hand_pinned_integer_sums(oracle):
    for np_dt, a, b, want, want_relu in ((np.uint8, 200, 100, 255, 255), (np.int8, -128, -128, -128, 0),
                                         (np.int8, 127, 127, 127, 127), (np.int8, -128, 127, -1, 0),
                                         (np.int32, 2147483647, 1, 2147483647, 2147483647),
                                         (np.int32, -2147483648, -1, -2147483648, 0)):
        xs = [np.full(3, a, np_dt), np.full(3, b, np_dt)]
        for f in (oracle.eltwise_sum, refmath.eltwise_sum):
            assert f(xs, False).tolist() == [want] * 3
            assert f(xs, True).tolist() == [want_relu] * 3


@pytest.mark.parametrize("case", E.POOL_GEOM_CASES, ids=E.pool_case_id)
def test_special_inputs_hold_the_arrangements(case):
    """special_f32 promises NaN first / last / in the middle of a window, +0 before -0, -0 before +0 and +Inf with
    -Inf in one window, as far as the windows of the case are large enough; every special value occurs"""
    x = E.pool_input(case, np.float32)
    largest = max(len(E.window_positions(case, oy, ox)) for oy in range(case[4][0]) for ox in range(case[4][1]))
    want = set()
    if largest >= 2 and x.shape[0] * x.shape[3] >= 5:
        want |= {"nan_first", "nan_last", "pz_before_nz", "nz_before_pz"}
    if largest >= 3 and x.shape[0] * x.shape[3] >= 6:
        want |= {"nan_middle", "inf_both"}
    assert want <= E.window_arrangements(x, case), (want - E.window_arrangements(x, case))
    plain = E.special_f32(case[0], 11)      # (the planted windows may overwrite the few instances of a small tensor)
    if plain.size >= len(E.F32_SPECIALS) * E.SPECIAL_SHARE:
        assert set(E.F32_SPECIALS) <= set(int(v) for v in plain.view(np.uint32).reshape(-1))
    for np_dt in (np.uint8, np.int8, np.int32):
        xi = E.pool_input(case, np_dt)
        assert xi.min() == np.iinfo(np_dt).min and xi.max() == np.iinfo(np_dt).max


def test_the_table_reaches_both_pool_paths_and_a_second_pass():
    for np_dt in E.DTYPES:
        paths = {E.pool_takes_vector_path(c, np_dt) for c in E.POOL_GEOM_CASES}
        assert paths == {True, False}, np_dt
    assert E.pool_items(E.POOL_BIG_VEC, np.float32) == 532512 > E.LAUNCH_ITEMS
    assert E.pool_takes_vector_path(E.POOL_BIG_VEC, np.float32)
    assert E.pool_items(E.POOL_BIG_SCALAR, np.uint8) == 608400 > E.LAUNCH_ITEMS
    assert not E.pool_takes_vector_path(E.POOL_BIG_SCALAR, np.uint8)
    assert E.eltwise_items(E.ELTWISE_BIG_F32[0], np.float32) == E.LAUNCH_ITEMS + 503
    assert E.eltwise_items(E.ELTWISE_BIG_BYTE[0], np.uint8) == E.LAUNCH_ITEMS + 513
    assert int(np.prod(E.CONCAT_BIG_PIXELS)) * sum(E.CONCAT_BIG_BYTE_CHANNELS) // 16 == 540800 > E.LAUNCH_ITEMS
    assert int(np.prod(E.CONCAT_BIG_PIXELS)) * sum(E.CONCAT_BIG_F32_CHANNELS) * 4 // 16 == 540800


@pytest.mark.parametrize("np_dt", E.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", SMALL_POOL_CASES, ids=E.pool_case_id)
def test_maxpool_oracle_vs_select_order(oracle, case, np_dt):
    shape, k, s, p, o = case
    x = E.pool_input(case, np_dt)
    E.assert_selected_equal(oracle.maxpool(x, k, s, p, o), refmath.maxpool_select(x, k, s, p, o), "maxpool")


@pytest.mark.parametrize("include_padding", [True, False])
@pytest.mark.parametrize("np_dt", E.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", SMALL_POOL_CASES, ids=E.pool_case_id)
def test_avgpool_oracle_vs_independent(oracle, case, np_dt, include_padding):
    shape, k, s, p, o = case
    x = E.pool_input(case, np_dt)
    with np.errstate(all="ignore"):
        ref = refmath.avgpool(x, k, s, p, o, include_padding)
    E.assert_computed_equal(oracle.avgpool(x, k, s, p, o, include_padding), ref, "avgpool")


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("np_dt", E.DTYPES, ids=DT_IDS)
def test_eltwise_sum_oracle_vs_independent(oracle, np_dt, relu):
    for elems, n in E.ELTWISE_CASES:
        xs = E.eltwise_inputs(elems, np_dt, n)
        with np.errstate(all="ignore"):
            ref = refmath.eltwise_sum(xs, relu)
        E.assert_computed_equal(oracle.eltwise_sum(xs, relu), ref, "eltwise %d x %d" % (n, elems))
        if np_dt == np.float32 and elems > 100:
            assert np.isnan(ref).any() and np.isinf(ref).any() and (ref.view(np.uint32) == E.NZ).any()
            assert ((ref != 0) & (np.abs(ref) < np.float32(1.1754944e-38))).any(), "no denormal sum"


def concat_reference(srcs, relu):
    ref = np.concatenate(srcs, axis=3)
    if not relu or ref.dtype == np.uint8:
        return ref
    return refmath.relu_select(ref) if ref.dtype == np.float32 else np.where(ref < 0, ref.dtype.type(0), ref)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("np_dt", E.DTYPES, ids=DT_IDS)
def test_concat_oracle_vs_independent(oracle, np_dt, relu):
    srcs = E.concat_inputs(E.CONCAT_PIXELS, E.CONCAT_CHANNELS[np.dtype(np_dt).itemsize], np_dt)
    E.assert_selected_equal(oracle.concat(srcs, relu), concat_reference(srcs, relu), "concat")
    blk = 16 // np.dtype(np_dt).itemsize
    srcs = E.concat_inputs(E.CONCAT_PIXELS, [blk] * 64, np_dt, seed=43)            # the most branches the op takes
    E.assert_selected_equal(oracle.concat(srcs, relu), concat_reference(srcs, relu), "concat of 64")


def test_large_shapes_once(oracle):
    """the second-pass shapes of the GPU tests, one dtype each"""
    shape, k, s, p, o = E.POOL_BIG_VEC
    x = E.pool_input(E.POOL_BIG_VEC, np.float32)
    E.assert_selected_equal(oracle.maxpool(x, k, s, p, o), refmath.maxpool_select(x, k, s, p, o), "maxpool big")
    with np.errstate(all="ignore"):
        ref = refmath.avgpool(x, k, s, p, o, False)
    E.assert_computed_equal(oracle.avgpool(x, k, s, p, o, False), ref, "avgpool big")
    shape, k, s, p, o = E.POOL_BIG_SCALAR
    x = E.pool_input(E.POOL_BIG_SCALAR, np.uint8)
    E.assert_selected_equal(oracle.maxpool(x, k, s, p, o), refmath.maxpool_select(x, k, s, p, o), "maxpool big u8")
    xs = E.eltwise_inputs(E.ELTWISE_BIG_F32[0], np.float32, E.ELTWISE_BIG_F32[1])
    with np.errstate(all="ignore"):
        ref = refmath.eltwise_sum(xs, True)
    E.assert_computed_equal(oracle.eltwise_sum(xs, True), ref, "eltwise big")
    srcs = E.concat_inputs(E.CONCAT_BIG_PIXELS, E.CONCAT_BIG_F32_CHANNELS, np.float32)
    E.assert_selected_equal(oracle.concat(srcs, True), concat_reference(srcs, True), "concat big")
