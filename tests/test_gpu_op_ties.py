"""GPU: rounding ties and extreme requant constants on the ops that end in accumulator -> (float(acc) + bias) * scale
-> convert: dfx_dwconv, dfx_dwpw, dfx_gconv, dfx_fc, dfx_imgconv, dfx_deconv and dfx_dilconv.

The convert is where the two routes differ: v_cvt_pk_u8_f32 (fast, u8 and s8 + ReLU), (int)rintf (fast, other outputs),
cvt_x86_rt (exact: nearest-even or floor).  The ops' own suites draw scales with which (acc + b) * s lands on
k + 1/2 for a handful of values at most, by accident (tests/op_ties.py).  Here
  test_rounding_ties      power-of-two scales put hundreds of values on k + 1/2 (tests/op_ties.py counts them): every
                          (op, path, stage) of op_ties.TABLE x two k x dst u8 / s8 / s32 x round mode 0 / 1 x DFX_NO_FAST
                          off / on, through the op module's own run() (guarded dst), bit for bit against the op's
                          reference, with the forced path, the route and the kernel-name suffix asserted; a second run
                          with scale * 1.37 (no ties) tells a tie bug from a general one, and a third with the scale
                          f32(1 / 6), whose ties exist only in the separately rounded product, catches a bias * scale
                          folded into an fma,
  test_extreme_constants  one constant at a time on ONE channel of a per-channel op on the op's proof-edge shape: s32
                          biases around 2^24 and at the ends of the type, fractional / signed-zero / huge / non-finite
                          f32 biases, zero, signed-zero, negative, denormal, huge and non-finite scales (the lists of
                          test_gpu_requant_edges.py), every dst type; the route from requant_host.h's formula computed
                          here from every channel's P, N, bias and scale; the other path as a second witness.
"""
from dataclasses import replace

import numpy as np
import pytest

import cases as C
import hipref
import op_ties as T
from test_gpu_requant_edges import F32_BIASES, S32_BIASES, SCALES

pytestmark = pytest.mark.gpu
EXACT, FAST = 0, 1
ROUTE_NAME = {0: "exact", 1: "fast", 2: "magic", 3: "fma"}       # route_name of dwpw_api.hip (two-launch: the conv's)


def _run(spec, case, data, forced=None):
    G = T.gpu_module(spec.op)
    got, info, route = G.run(case, data, force_path=spec.forced if forced is None else forced)
    return got, info, route, info.kernel_name.decode()


def _check_variant(spec, info, name):
    """the forced path and the kernel variant the spec's switches select"""
    assert info.path == spec.forced, (name, info.path)
    if spec.op == "gconv" and spec.forced == 0:
        assert name.startswith("gconv_mfma_tile<" if spec.path == "mfma_tile" else "gconv_mfma<"), name
    if spec.op == "fc" and spec.forced == 0:
        assert info.splitk == spec.switches["DFX_FC_SPLITK"], (name, info.splitk)
    if spec.op == "dwpw":
        assert name.startswith("dwpw_fused<" if spec.forced == 0 else "dwpw_two_launch<"), name


def _check_route(spec, case, switch, rm, route, name):
    """FAST exactly where the op's own want_route says so; EXACT under DFX_NO_FAST and under round mode 1"""
    G = T.gpu_module(spec.op)
    if spec.op != "dwpw":
        want = G.want_route(case, switch, spec.forced)
        assert route == want, (name, route, want)
        if switch or rm == 1:
            assert route == EXACT, (name, route)
        assert name.endswith("fast" if route == FAST else "exact"), name
        return
    want = G.want_routes(case, switch)
    assert want[spec.stage] == (EXACT if (switch or rm == 1) else FAST)
    if spec.forced == 0:
        assert tuple(route) == want, (name, route, want)
    else:
        # two launches: stage 0 is the depthwise op's window kernel, stage 1 the dense conv's proof (fast / magic / fma)
        assert route[0] == want[0] and (route[1] == EXACT) == (want[1] == EXACT), (name, route, want)
    assert name.endswith("%s/%s" % (ROUTE_NAME[route[0]], ROUTE_NAME[route[1]])), name


@pytest.mark.parametrize("spec", T.TABLE, ids=T.spec_id)
def test_rounding_ties(tuning, spec):
    """nearest-even in v_cvt_pk_u8_f32 / rintf / cvt_x86_rt and floor on negative halves (rm 1), on both routes"""
    for key, v in spec.switches.items():
        tuning.setenv(key, v)
    failures, runs = [], 0
    for k, dst_dt, rm, relu in T.rows(spec):
        case = T.tie_case(spec, dst_dt, rm, relu)
        data, n = T.tie_data(spec, case, k)
        odd, sixth = T.odd_data(spec, data), T.sixth_data(spec, data)
        ref, ref_odd, ref_sixth = (T.reference(spec.op, case, d) for d in (data, odd, sixth))
        for switch in (None, "DFX_NO_FAST"):
            if switch:
                tuning.setenv(switch, "1")
            what = "%s 2^-%d dst %s relu %d rm %d %s" % (T.spec_id(spec), k, C.NAME_OF[dst_dt], relu, rm, switch)
            # each reported on its own; scale 1 / 6: ties of the rounded product only (op_ties.sixth_data)
            for d, want, tag in ((data, ref, " " + str(n)), (odd, ref_odd, " x 1.37"), (sixth, ref_sixth, " scale 1/6")):
                try:
                    got, info, route, name = _run(spec, case, d)
                    _check_variant(spec, info, name)
                    _check_route(spec, case, switch, rm, route, name)
                    hipref.assert_bit_equal(got, want, what + tag + " [" + name + "]")
                    runs += 1
                except AssertionError as e:
                    failures.append(what + tag + ": " + str(e)[:600])
            if switch:
                tuning.setenv(switch, None)
    print("%s: %d runs, %d failures" % (T.spec_id(spec), runs, len(failures)))
    assert not failures, "%d:\n%s" % (len(failures), "\n".join(failures))


# --- extreme constants ----------------------------------------------------------------------------------------------------
CH = 5                       # the channel that carries the constant (every op's EDGE_CHANNEL)
ALL = (C.U8, C.S8, C.S32, C.F32)
EXTREME = [s for s in T.TABLE if s.forced == 0 and s.path in ("window", "mfma", "mfma_sk1", "fused")]
CONSTS = [("bias", b) for b in S32_BIASES] + [("bias", b) for b in F32_BIASES] + [("scale", s) for s in SCALES]


def extreme_case(spec, dst_dt, f32_bias):
    """the op's proof-edge shape (2 images of 3x3 -- 5x5 for the dilated op, 1x1 for fc --, its smallest channel count)
    with per-channel scales; u8 and f32 outputs behind a ReLU (f32: the sign of zero after relu_x86 is part of the
    bytes), s8 and s32 without, so that negative results reach the conversion"""
    R = T.ref_module(spec.op)
    relu, bdt = dst_dt in (C.U8, C.F32), C.F32 if f32_bias else C.S32
    if spec.op == "dwpw":
        base = R.edge0_case(R.EDGES0[0], dst_dt)[0]
        if spec.stage == 0:
            return replace(base, name="extreme0", bia0_dt=bdt, bia1_dt=C.S32, pc0=True, pc1=False, relu=relu, seed=9100)
        return replace(base, name="extreme1", bia0_dt=C.S32, bia1_dt=bdt, pc0=False, pc1=True, relu=relu, seed=9101)
    edges = R.FC_EDGES if spec.op == "fc" else R.EDGES
    base = R.edge_case(edges[0], dst_dt)[0]
    return replace(base, name="extreme", bia_dt=bdt, relu=relu, per_channel=True, seed=9000)


def _keys(spec):
    if spec.op != "dwpw":
        return "w", "bia", "scales"
    return (("w", "bia0", "scales0"), ("w1", "bia1", "scales1"))[spec.stage]


def extreme_data(spec, case, kind, value):
    """reference-range data with the constant on channel CH.  A bias constant comes with a scale that shows it: 3 on a
    4-byte dst (every count of the sum shows; the ends of s32 go past 2^31 on the exact route), one that brings the
    sum to about 100 on a 1-byte dst, 0.01 where the constant is not finite.  A scale constant comes with the bias 7,
    or 100000 -- beyond every accumulator of these shapes -- where the scale is not finite: 0 * inf would be a NaN the
    hardware GENERATES, whose sign x86 sets and the GPU does not (the ops' own NaN tests keep away from it as well)."""
    data = dict(T.ref_module(spec.op).generate(case))
    wk, bk, sk = _keys(spec)
    bias, scales = data[bk].copy(), data[sk].copy()
    if kind == "bias":
        bias[CH] = value
        if not np.isfinite(float(value)):
            scales[CH] = 0.01
        elif case.dst_dt in (C.S32, C.F32):
            scales[CH] = 3.0
        else:
            scales[CH] = 100.37 / max(abs(float(value)), 1.0)
    else:
        bias[CH] = 7 if np.isfinite(value) else 100000
        scales[CH] = value
    data[bk], data[sk] = bias, scales
    return data


def fast_must_hold(spec, data):
    """requant_host.h, fast_ok_2p30 over every channel of the stage: bias and scale finite and
    (255 * max(P, N) + |bias|) * |scale| <= 2^30, in double, with the bias as the f32 the host converts it to"""
    wk, bk, sk = _keys(spec)
    w = data[wk].astype(np.int64).reshape(data[wk].shape[0], -1)
    P, N = np.where(w > 0, w, 0).sum(axis=1), -np.where(w < 0, w, 0).sum(axis=1)
    b = data[bk].astype(np.float32).astype(np.float64)
    s = np.broadcast_to(data[sk].astype(np.float64), b.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = np.isfinite(b) & np.isfinite(s) & ((255.0 * np.maximum(P, N) + np.abs(b)) * np.abs(s) <= 2.0 ** 30)
    return bool(ok.all())


@pytest.mark.parametrize("spec", EXTREME, ids=T.spec_id)
def test_extreme_constants(spec):
    failures, runs, seen = [], 0, set()
    for kind, value in CONSTS:
        for dst_dt in ALL:
            what = "%s %s %r dst %s" % (T.spec_id(spec), kind, value, C.NAME_OF[dst_dt])
            try:
                case = extreme_case(spec, dst_dt, kind == "bias" and isinstance(value, float))
                data = extreme_data(spec, case, kind, value)
                with np.errstate(over="ignore", invalid="ignore"):       # the constants overflow on purpose
                    ref = T.reference(spec.op, case, data)
                got, info, route, name = _run(spec, case, data)
                assert info.path == spec.forced, (what, name)
                hipref.assert_bit_equal(got, ref, what + " [" + name + "] route " + str(route))
                want = FAST if fast_must_hold(spec, data) else EXACT
                seen.add(want)
                if spec.op == "dwpw":
                    assert tuple(route) == ((want, FAST) if spec.stage == 0 else (FAST, want)), (what, name, route, want)
                else:
                    assert route == want and name.endswith(ROUTE_NAME[want]), (what, name, route, want)
                wit, winfo, wroute, wname = _run(spec, case, data, forced=1)           # generic / two-launch
                assert winfo.path == 1, (what, wname)
                hipref.assert_bit_equal(wit, ref, what + " [witness " + wname + "]")
                runs += 2
            except AssertionError as e:
                failures.append(what + ": " + str(e)[:600])
    print("%s: %d runs, %d failures" % (T.spec_id(spec), runs, len(failures)))
    assert not failures, "%d:\n%s" % (len(failures), "\n".join(failures))
    assert seen == {EXACT, FAST}, seen


def test_extreme_expectations_are_not_vacuous():
    """the route expectation of every constant, from the formula alone (no launch): the non-finite ones, the huge scale,
    and the ends of s32 under the scale 3 must fail the proof; zeros, signed zeros, negative and denormal scales and
    the biases around 2^24 must pass it"""
    spec = T.find("dwconv", "window")
    want_exact = {("bias", float("inf")), ("bias", float("-inf")), ("scale", float("inf")), ("scale", 3e38),
                  ("bias", (1 << 31) - 1), ("bias", -(1 << 31)), ("bias", 1e30)}
    for kind, value in CONSTS:
        f32_bias = kind == "bias" and isinstance(value, float)
        data = extreme_data(spec, extreme_case(spec, C.S32, f32_bias), kind, value)
        nan = isinstance(value, float) and np.isnan(value)
        assert fast_must_hold(spec, data) == (not nan and (kind, value) not in want_exact), (kind, value)
