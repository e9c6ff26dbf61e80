"""CPU-only checks of the tie data of tests/op_ties.py: every (op, path, stage, k, dst type, round mode) row puts enough
values on k + 1/2 inside the unsaturated output range, the scale 1 / 6 puts enough rounded products there that an fma
would miss, and on all of that data the numpy references the GPU is held to equal the C oracle's dense conv, bit for
bit, under both round modes."""
import numpy as np
import pytest

import cases as C
import hipref
import op_ties as T
import requant_edges as E


@pytest.mark.parametrize("spec", T.TABLE, ids=T.spec_id)
def test_every_row_has_enough_ties(spec):
    """at least 50 ties, 15 with the even neighbour below, 15 above, 15 negative wherever negative results survive
    (tie_data asserts it); the counts are printed for the record"""
    base = T.base_case(spec)
    assert T.outputs(spec.op, base) >= T.MIN_OUTPUTS and spec.in_class(base)
    for k, dst_dt, rm, relu in T.rows(spec):
        case = T.tie_case(spec, dst_dt, rm, relu)
        data, n = T.tie_data(spec, case, k)
        assert n["need_negative"] == (not relu and (spec.op, spec.stage) != ("dwpw", 0)), (T.spec_id(spec), n)
        if rm == 0:
            print("TIES %s %s 2^-%d dst %s%s: total %d below %d above %d negative %d" % (
                T.spec_id(spec), base.ident().split("-u8")[0].split("-s8")[0].split("-s32")[0].split("-f32")[0], k,
                C.NAME_OF[dst_dt], "+relu" if (relu and dst_dt != C.U8) else "", n["total"], n["below"], n["above"], n["negative"]))
        # the same data with scale * 1.37 has no tie left: that run tells a tie bug from a general one
        odd = T.odd_data(spec, data)
        s = float(odd[T.scale_key(spec)][0])
        bias = data["bia" if spec.op != "dwpw" else ("bia0", "bia1")[spec.stage]].astype(np.int64)
        t = (T.accumulator(spec.op, spec.stage, case, data) + bias).astype(np.float64) * s
        assert not np.any(t - np.floor(t) == 0.5), T.spec_id(spec)


@pytest.mark.parametrize("spec", T.TABLE, ids=T.spec_id)
def test_the_sixth_scale_puts_rounded_products_on_ties(spec):
    """scale f32(1 / 6): no product is a tie as a real number, yet the separately rounded f32 chain lands on k + 1/2
    often enough (the thresholds of the 2^-k data), and an fma of the same numbers misses at least 15 of them"""
    for k, dst_dt, rm, relu in T.rows(spec):
        if k != spec.ks[0]:
            continue
        case = T.tie_case(spec, dst_dt, rm, relu)
        data = T.sixth_data(spec, T.tie_data(spec, case, k)[0])
        n = T.count_rounded(spec, case, data)
        E.assert_enough_ties(n, (T.spec_id(spec), case.ident(), "1/6"))
        bias = data["bia" if spec.op != "dwpw" else ("bia0", "bia1")[spec.stage]].astype(np.float64)
        acc = T.accumulator(spec.op, spec.stage, case, data).astype(np.float64)
        s = np.float64(T.SIXTH)
        assert not np.any(((acc + bias) * s) % 1.0 == 0.5)                                 # (exact in f64)
        two_step = ((acc + bias).astype(np.float32) * T.SIXTH).astype(np.float32)
        folded = (acc * s + (bias.astype(np.float32) * T.SIXTH).astype(np.float32).astype(np.float64)).astype(np.float32)
        tie = two_step.astype(np.float64) % 1.0 == 0.5
        assert int((tie & (folded != two_step)).sum()) >= 15, (T.spec_id(spec), int(tie.sum()), int((tie & (folded != two_step)).sum()))


def test_the_table_covers_every_op_path_and_stage():
    want = {("dwconv", "window", 0), ("dwconv", "generic", 0), ("gconv", "mfma", 0), ("gconv", "mfma_tile", 0),
            ("gconv", "generic", 0), ("fc", "mfma_sk1", 0), ("fc", "mfma_sk2", 0), ("fc", "generic", 0),
            ("imgconv", "mfma", 0), ("imgconv", "generic", 0), ("deconv", "mfma", 0), ("deconv", "generic", 0),
            ("dilconv", "mfma", 0), ("dilconv", "generic", 0), ("dwpw", "fused", 0), ("dwpw", "fused", 1),
            ("dwpw", "two_launch", 0), ("dwpw", "two_launch", 1)}
    assert {(s.op, s.path, s.stage) for s in T.TABLE} == want and len(T.TABLE) == len(want)
    assert T.KS == E.TIE_KS and T.DSTS == E.TIE_DSTS
    # split-K > 1 needs more than one k-step; the MFMA rows sit in their kernel's class
    assert T.base_case(T.find("fc", "mfma_sk2")).K // 64 >= 2 and T.base_case(T.find("fc", "mfma_sk1")).K // 64 == 1
    for s in T.TABLE:
        if s.path.startswith("mfma"):
            assert T.base_case(s).mfma_class, T.spec_id(s)


def test_count_ties_of_counts_what_it_says():
    """a hand-made list: 2^-2 ties are t = 2 (mod 4); below / above by the parity of floor(t / 4); the range clips"""
    t = np.array([2, 6, 10, -2, -6, 1, 4, 1022, 1018, -510, -514, 510], dtype=np.int64)
    n = E.count_ties_of(t, 2, C.U8, True)                  # 0.5 1.5 2.5 | 254.5 (fl 254) ; 255.5 is outside
    assert (n["total"], n["below"], n["above"], n["negative"], n["need_negative"]) == (5, 3, 2, 0, False), n
    n = E.count_ties_of(t, 2, C.S8, False)                 # -127.5 (fl -128) inside, -128.5 outside, 127.5 outside
    assert (n["total"], n["below"], n["above"], n["negative"], n["need_negative"]) == (6, 4, 2, 3, True), n
    n = E.count_ties_of(t, 2, C.S32, False)
    assert n["total"] == 10 and n["negative"] == 4 and n["need_negative"], n


@pytest.mark.parametrize("spec", T.TABLE, ids=T.spec_id)
def test_reference_equals_the_oracle_on_the_tie_data(oracle, spec):
    """wherever the case can be expressed as the dense conv the oracle computes (dwconv / gconv / dwpw block-diagonal
    twins, the dilconv and deconv stuffed twins, imgconv on 16 channels, fc as a conv whose window is the image):
    nearest-even and floor on hundreds of exact halves.  This pins the reference the GPU is then held to."""
    n = 0
    for k, dst_dt, rm, relu in T.rows(spec):
        case = T.tie_case(spec, dst_dt, rm, relu)
        data, counts = T.tie_data(spec, case, k)
        for d in (data, T.odd_data(spec, data), T.sixth_data(spec, data)):
            twin = T.dense_twin(spec, case, d)
            if twin is None:
                continue
            want = hipref.oracle_conv(oracle, *twin)
            got = T.reference(spec.op, case, d)
            if spec.op == "fc":
                want = want.reshape(got.shape)                       # {bs, 1, 1, oc} -> {bs, oc}
            hipref.assert_bit_equal(got, want,"%s %s 2^-%d %r" % (T.spec_id(spec), case.ident(), k, counts))
            n += 1
    expressible = T.base_case(spec).dense_expressible
    assert n == (3 * len(T.rows(spec)) if expressible else 0), (T.spec_id(spec), n)


def test_enough_rows_reach_the_oracle():
    """every op has at least one row that the oracle pins"""
    ops = {s.op for s in T.TABLE if T.base_case(s).dense_expressible}
    assert ops == set(T.MODULES), ops
