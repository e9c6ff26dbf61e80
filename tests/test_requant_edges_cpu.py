"""CPU: the adversarial input builder of requant_edges.py keeps its promises -- the accumulator bounds 255 P and
-255 N are attained exactly (checked through both oracle implementations), the tie data of every case of the GPU
table holds enough ties of every kind, and the Diophantine helper hits the limits of the proofs exactly."""
from dataclasses import replace

import numpy as np
import pytest

import cases as C
import hipref
import requant_edges as E

MAGIC1_MANT = 0x22F983           # mantissa of 1/(2 pi), the start value of the "magic" route (conv_mfma.cuh)

# K = taps of one output channel: 288 / 576 (3x3 over 32 / 64 channels), 256 / 1024 (pointwise)
STAGE0 = {288: C.ConvCase("k288", 1, 32, 3, 3, 32, 0), 576: C.ConvCase("k576", 1, 64, 3, 3, 64, 0),
          256: C.ConvCase("k256", 1, 256, 1, 1, 64, 0, k=(1, 1), pad=(0, 0)),
          1024: C.ConvCase("k1024", 1, 1024, 1, 1, 64, 0, k=(1, 1), pad=(0, 0))}
# stage 1: K = oc of a fused op whose conv0 copies the source (ic >= oc)
STAGE1 = {32: C.ConvCase("c32", 1, 32, 3, 3, 32, 32), 64: C.ConvCase("c64", 1, 64, 3, 3, 64, 128),
          128: C.ConvCase("c128", 1, 128, 3, 3, 128, 128), 256: C.ConvCase("c256k1", 1, 256, 1, 1, 256, 64, k=(1, 1), pad=(0, 0))}


def _impls(oracle):
    return ("scalar", "avx512") if oracle.have_avx512_vnni() else ("scalar", "scalar_mt")


def _channels(K):
    """three channels: all taps at the extremes, a lopsided mix, and the issue's (3, 18045)-like sliver"""
    half = K // 2
    return {1: E.weights_with_pn(K, E.W_MAX * half, -E.W_MIN * (K - half), seed=K),
            6: E.weights_with_pn(K, E.W_MAX * (K - 3), 5, seed=K + 1),
            15: E.weights_with_pn(K, 3, min(18045, -E.W_MIN * (K - 1)), seed=K + 2)}


@pytest.mark.parametrize("K", sorted(STAGE0))
def test_stage0_bounds_are_attained(oracle, K):
    case, data, slots = E.edge_op(replace(STAGE0[K], dst_dt=C.S32), 0, _channels(K))
    assert case.ic * case.k[0] * case.k[1] == K and len(slots) == 6
    ac, ad = E.attain_op(case, data, 0)
    for impl in _impls(oracle):
        E.assert_attained(hipref.oracle_conv(oracle, ac, ad, impl=impl), case, data, 0, slots)


@pytest.mark.parametrize("K", sorted(STAGE1))
def test_stage1_bounds_are_attained(oracle, K):
    case, data, slots = E.edge_op(replace(STAGE1[K], dst_dt=C.S32), 1, _channels(K))
    assert case.oc == K
    ac, ad = E.attain_op(case, data, 1)
    for impl in _impls(oracle):
        E.assert_attained(hipref.oracle_conv(oracle, ac, ad, impl=impl), case, data, 1, slots)


def test_attainment_check_has_teeth(oracle):
    """one activation off the pattern and assert_attained must notice"""
    case, data, slots = E.edge_op(replace(STAGE0[288], dst_dt=C.S32), 0, _channels(288))
    w = data["w0"][slots[0][0]]
    i, y, x = [int(v[0]) for v in np.nonzero(w > 0)]
    data["src"][0, y, x, i] -= 1
    ac, ad = E.attain_op(case, data, 0)
    with pytest.raises(AssertionError, match="the bound is"):
        E.assert_attained(hipref.oracle_conv(oracle, ac, ad, impl="scalar"), case, data, 0, slots)


@pytest.mark.parametrize("family,stage", E.tie_table(), ids=lambda v: str(v))
def test_tie_data_holds_enough_ties(family, stage):
    """tie_data itself refuses thin data; this runs it for every case the GPU table uses, without a GPU"""
    for k in E.TIE_KS:
        for dst_dt in E.TIE_DSTS:
            for rm in (0, 1):
                case = E.tie_case(family, stage, dst_dt, rm)
                data, n = E.tie_data(case, stage, k)
                assert n["total"] >= 50 and n["below"] >= 15 and n["above"] >= 15, (case.ident(), n)
                if dst_dt != C.U8 and (stage == 1 or not case.oc1x1):
                    assert n["need_negative"] and n["negative"] >= 15, (case.ident(), n)
                scales = data["scales0"] if stage == 0 else data["scales1"]
                assert (scales == np.float32(2.0 ** -k)).all()


def test_small_tie_counts_are_the_recorded_ones():
    """SMALL (2 x 9 x 7, 32 -> 32), stage 0, scale 2^-4: 125 ties inside u8 among 4032 values, split by parity"""
    data, n = E.tie_data(E.tie_case("resident_fused", 0, C.U8, 0), 0, 4)
    assert n == dict(total=125, below=64, above=61, negative=0, need_negative=False)


def test_diophantine_helper_hits_the_limits():
    lo, hi = MAGIC1_MANT, 0x7FFFFF - MAGIC1_MANT
    assert (lo, hi) == (2292099, 6096508)
    # most negative raw accumulator -(128 P + 127 N) the magic start value absorbs: the limit and one step beyond
    for target in (lo, lo + 1):
        P, N = E.solve_pn(128, 127, target, 288)
        assert 128 * P + 127 * N == target and E.taps_needed(P, N) <= 288
        assert E.pn_of(E.weights_with_pn(288, P, N)) == (P, N)
    assert E.solve_pn(128, 127, lo, 288) == (3, 18045)
    # most positive one, 127 P + 128 N: out of reach of 288 taps (at most 128 * 128 * 288 < hi), within reach of 576
    assert 128 * 128 * 288 < hi and E.solve_pn(127, 128, hi, 288) is None
    for target in (hi, hi + 1):
        P, N = E.solve_pn(127, 128, target, 576)
        assert 127 * P + 128 * N == target and E.taps_needed(P, N) <= 576
        assert E.pn_of(E.weights_with_pn(576, P, N)) == (P, N)
    # the true accumulator's bound 255 P at the binade limits 2^22 and 2^23, topped up by the bias
    for limit in (1 << 22, 1 << 23):
        P = (limit - 1) // 255
        assert 255 * P <= limit - 1 < 255 * (P + 1) and E.taps_needed(P, 0) <= 288
    # unreachable targets are refused, not approximated
    assert E.solve_pn(128, 127, 1, 288) is None and E.solve_pn(2, 4, 7, 10) is None
    with pytest.raises(AssertionError):
        E.weights_with_pn(4, 127 * 4 + 1, 0)


def test_weights_with_pn_stays_inside_int8_and_uses_both_signs():
    w = E.weights_with_pn(64, 1000, 3000, seed=3)
    assert w.dtype == np.int8 and w.min() >= -128 and w.max() <= 127 and E.pn_of(w) == (1000, 3000)
    assert (E.pattern(w, "max") == np.where(w > 0, 255, 0)).all() and (E.pattern(w, "min") == np.where(w < 0, 255, 0)).all()
