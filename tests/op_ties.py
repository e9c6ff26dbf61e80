"""Rounding-tie data for the ops that end in accumulator -> (float(acc) + bias) * scale -> convert (pure numpy, no GPU).

The ops' own generators draw scales of the kind 80 / (54 sqrt(K)) and per-channel multiples of it.  As real numbers
(acc + b) * s is then never k + 1/2; the f32 product lands on one only where sqrt(K) is rational (3x3 depthwise: s =
40/81, channel 1 of 16 has 5/18 and t = 9 gives 2.5): one to a dozen values of a tensor, by accident, on some cases.
Here the op's own generate(case) -- reference-range data, an integer (s32) bias, a single scale -- gets
  * the scale 2^-k: the exact int64 accumulators are counted (requant_edges.count_ties_of) so that enough values land on
    k + 1/2 inside the unsaturated output range; tie_data refuses data below requant_edges' thresholds,
  * that scale times 1.37 (odd_data): no ties; tells a tie bug from a general one,
  * the scale f32(1 / 6) with biases up to 200 (sixth_data): ties that exist only in the separately rounded product,
    which a bias * scale folded into an fma misses (count_rounded counts them from the f32 chain).

TABLE has one Spec per (op, path, stage): the op's *_ref module, the function that yields its exact accumulator, the
forced path with the switches that select a kernel variant, and the case.  The case is the FIRST case of the op's own
table with at least 2000 outputs that is in the path's class (for a generic path: the op's generic table first, then
its other tables, since the generic kernels take every shape); `skip` counts the cases the counter refused before it.

  op       path                case                                       outputs  ties u8 / s8 / s32 at 2^-4; 2^-3
  dwconv   window              k3s1p1-3x3 n2 c144                            2592   87 / 158 / 158;  168 / 319 / 319
  dwconv   generic             gen n2 c24 9x10 k3x3 s1x2                     2160   68 / 123 / 123;  168 / 275 / 275
  gconv    mfma, mfma_tile     s1p1-3x3 n2 c128 g32                          2304   75 / 134 / 134;  147 / 298 / 298
  gconv    generic             gen n2 24 -> 36 g3 9x10                       6480  206 / 382 / 382;  472 / 866 / 879
  fc       mfma_sk1            mfma n31 1x1x64 oc96 (one k-step)             2976   97 / 192 / 192;  172 / 354 / 367
  fc       mfma_sk2            mfma n31 1x1x192 oc96 (DFX_FC_SPLITK=2)       2976   84 / 193 / 194;  157 / 290 / 358
  fc       generic             mfma n31 1x1x64 oc96 (fc's generic table      2976   97 / 192 / 192;  172 / 354 / 367
                               has no case of 2000 outputs)
  imgconv  mfma                k7s2p3-5x5 n3 c3 oc128                        3456  115 / 216 / 216;  249 / 458 / 466
  imgconv  generic             gen n2 c1 9x10 oc16 k5x5                      2880   94 / 165 / 165;  203 / 355 / 357
  deconv   mfma                k2s2p0-3x5 n1 c160 oc64 (*)                   3840   96 / 221 / 226;  233 / 404 / 487
  deconv   generic             gen n2 c1 5x6 oc48 k3x3 s1                    2880   94 / 192 / 192;  207 / 384 / 384
  dilconv  mfma                base n1 c32 8x8 oc32                          2048   58 / 129 / 131;  131 / 216 / 266
  dilconv  generic             gen n2 c3 15x14 oc48 k5x5 s2 d3               5376  167 / 323 / 323;  371 / 680 / 682
  dwpw     fused, two_launch   s1p1-2x3 n2 c96 oc256, stage 1                3072  111 / 188 / 214;  188 / 249 / 415
  dwpw     fused, two_launch   the same, stage 0 (1152 intermediate values)         2^-3: 65 (33 / 32);  2^-2: 133 (85 / 48)

At least 55 of the s8 / s32 ties of every row are negative.  No row's first case was refused (every skip is 0).
(*) the five-K-step case; the table's n3 c64 oc96 before it also has more than 2000 outputs (17280: more run time, two
K-steps).  test_op_ties_cpu.py prints every row's counts (pytest -s).

dwpw stage 1 runs with the stage-0 scale 2^-2.  dwpw stage 0 has only 1152 intermediate values, so it uses k = 2 and 3;
its ties are visible only through stage 1, so that row runs with an s32 output, stage-1 scale 1 and no stage-1 bias:
one wrong intermediate byte changes an output by w1.
"""
import importlib
from collections import namedtuple
from dataclasses import replace

import numpy as np

import cases as C
import requant_edges as E

U8, S8, S32, UNDEF = C.U8, C.S8, C.S32, C.UNDEF
MIN_OUTPUTS = 2000
KS, KS_DWPW0 = (4, 3), (3, 2)
DSTS = (U8, S8, S32)
DWPW_SCALE0_LOG2 = -2            # the stage-0 scale of the dwpw stage-1 rows
ODD = np.float32(1.37)           # scale * ODD: the same data without ties
SIXTH = np.float32(1.0 / 6.0)    # ties that exist only after the f32 rounding of the product (sixth_data)

# op -> (*_ref module, GPU test module, reference function)
MODULES = {
    "dwconv": ("dwconv_ref", "test_gpu_dwconv", "dw_ref"),
    "gconv": ("gconv_ref", "test_gpu_gconv", "gconv_ref"),
    "fc": ("fc_ref", "test_gpu_fc", "fc_ref"),
    "imgconv": ("imgconv_ref", "test_gpu_imgconv", "imgconv_ref"),
    "deconv": ("deconv_ref", "test_gpu_deconv", "deconv_ref"),
    "dilconv": ("dilconv_ref", "test_gpu_dilconv", "dilconv_ref"),
    "dwpw": ("dwpw_ref", "test_gpu_dwpw", "ref"),
}


def ref_module(op):
    return importlib.import_module(MODULES[op][0])


def gpu_module(op):
    return importlib.import_module(MODULES[op][1])


def reference(op, case, data):
    return getattr(ref_module(op), MODULES[op][2])(case, data)


# --- the exact int64 accumulator of a stage ---------------------------------------------------------------------------
def _hw(case):
    return (case.oh, case.ow)


ACC = {
    "dwconv": lambda R, c, d: R.dw_acc(d["src"], d["w"], c.stride, c.pad, _hw(c)),
    "gconv": lambda R, c, d: R.gconv_acc(d["src"], d["w"], c.groups, c.stride, c.pad, _hw(c)),
    "fc": lambda R, c, d: R.fc_acc(d["src"], d["w"]),
    "imgconv": lambda R, c, d: R.imgconv_acc(d["src"], d["w"], c.stride, c.pad, _hw(c)),
    "deconv": lambda R, c, d: R.deconv_acc(d["src"], d["w"], c.stride, c.pad, _hw(c)),
    "dilconv": lambda R, c, d: R.dilconv_acc(d["src"], d["w"], c.stride, c.dil, c.pad, _hw(c)),
}


def accumulator(op, stage, case, data):
    R = ref_module(op)
    if op != "dwpw":
        return ACC[op](R, case, data)
    if stage == 0:
        return R.DW.dw_acc(data["src"], data["w"], case.stride, case.pad, _hw(case))
    return R.acc1_of(R.mid_ref(case, data), data["w1"])


def outputs(op, case):
    if op == "fc":
        return case.bs * case.oc
    return case.bs * case.oh * case.ow * (case.c if op == "dwconv" else case.oc)


# --- the table ------------------------------------------------------------------------------------------------------------
# op, path (a name), stage, forced path (the op's constant), switches (tuning), the k values, tables (names of the ref
# module's table functions, searched in order), in_class (a predicate on the case), skip (cases the counter refused)
Spec = namedtuple("Spec", "op path stage forced switches ks tables in_class skip")


def _any(case):
    return True


def _mfma(case):
    return case.mfma_class


TABLE = [
    Spec("dwconv", "window", 0, 0, {}, KS, ("window_table",), _any, 0),
    Spec("dwconv", "generic", 0, 1, {}, KS, ("generic_table", "window_table"), _any, 0),
    Spec("gconv", "mfma", 0, 0, {}, KS, ("mfma_table",), _mfma, 0),
    Spec("gconv", "mfma_tile", 0, 0, {"DFX_GCONV_TILE": "1"}, KS, ("mfma_table",), _mfma, 0),
    Spec("gconv", "generic", 0, 1, {}, KS, ("generic_table", "mfma_table"), _any, 0),
    Spec("fc", "mfma_sk1", 0, 0, {"DFX_FC_SPLITK": 1}, KS, ("mfma_table",), _mfma, 0),
    Spec("fc", "mfma_sk2", 0, 0, {"DFX_FC_SPLITK": 2}, KS, ("mfma_table",), lambda c: c.mfma_class and c.K >= 128, 0),
    Spec("fc", "generic", 0, 1, {}, KS, ("generic_table", "mfma_table"), _any, 0),
    Spec("imgconv", "mfma", 0, 0, {}, KS, ("mfma_table",), _mfma, 0),
    Spec("imgconv", "generic", 0, 1, {}, KS, ("generic_table", "mfma_table"), _any, 0),
    Spec("deconv", "mfma", 0, 0, {}, KS, ("mfma_table",), lambda c: c.mfma_class and c.c == 160, 0),
    Spec("deconv", "generic", 0, 1, {}, KS, ("generic_table", "mfma_table"), _any, 0),
    Spec("dilconv", "mfma", 0, 0, {}, KS, ("mfma_table",), _mfma, 0),
    Spec("dilconv", "generic", 0, 1, {}, KS, ("generic_table", "mfma_table"), _any, 0),
    Spec("dwpw", "fused", 0, 0, {}, KS_DWPW0, ("shape_table",), lambda c: c.in_class, 0),
    Spec("dwpw", "fused", 1, 0, {}, KS, ("shape_table",), lambda c: c.in_class, 0),
    Spec("dwpw", "two_launch", 0, 1, {}, KS_DWPW0, ("shape_table",), lambda c: c.in_class, 0),
    Spec("dwpw", "two_launch", 1, 1, {}, KS, ("shape_table",), lambda c: c.in_class, 0),
]


def spec_id(spec):
    return "%s-%s-%d" % (spec.op, spec.path, spec.stage)


def find(op, path, stage=0):
    return [s for s in TABLE if (s.op, s.path, s.stage) == (op, path, stage)][0]


def base_case(spec):
    """the (skip + 1)-th case of the op's own tables with at least MIN_OUTPUTS outputs in the path's class"""
    R = ref_module(spec.op)
    hits = [c for t in spec.tables for c in getattr(R, t)() if outputs(spec.op, c) >= MIN_OUTPUTS and spec.in_class(c)]
    assert len(hits) > spec.skip, spec_id(spec)
    return hits[spec.skip]


def dsts_of(spec):
    """dwpw stage 0 is visible through an s32 output only"""
    return (S32,) if (spec.op, spec.stage) == ("dwpw", 0) else DSTS


def tie_case(spec, dst_dt, rm, relu=None):
    """the spec's case with the dst type and round mode under test, an s32 bias and a single scale; signed and 4-byte
    outputs drop the ReLU so that negative halves reach the conversion (relu=True: the s8 + ReLU rows, whose fast route
    converts with v_cvt_pk_u8_f32 behind a clamp)"""
    base, relu = base_case(spec), (dst_dt == U8 if relu is None else relu)
    if spec.op != "dwpw":
        return replace(base, dst_dt=dst_dt, bia_dt=S32, relu=relu, rm=rm, per_channel=False, wide=False)
    if spec.stage == 0:
        assert dst_dt == S32
        return replace(base, dst_dt=S32, bia0_dt=S32, bia1_dt=UNDEF, relu=False, rm0=rm, rm1=0, pc0=False, pc1=False, wide=False)
    return replace(base, dst_dt=dst_dt, bia0_dt=S32, bia1_dt=S32, relu=relu, rm0=0, rm1=rm, pc0=False, pc1=False, wide=False)


def scale_key(spec):
    return "scales" if spec.op != "dwpw" else ("scales0", "scales1")[spec.stage]


def count(spec, case, data, k):
    """ties of the spec's stage: the intermediate of dwpw is u8 behind a ReLU"""
    acc = accumulator(spec.op, spec.stage, case, data)
    mid = (spec.op, spec.stage) == ("dwpw", 0)
    bias = data["bia" if spec.op != "dwpw" else ("bia0", "bia1")[spec.stage]]
    assert bias is not None and bias.dtype == np.int32, "tie data needs integer biases"
    t = acc + bias.astype(np.int64)
    return E.count_ties_of(t, k, U8 if mid else case.dst_dt, True if mid else (case.relu or case.dst_dt == U8))


def tie_data(spec, case, k):
    """the op's generate(case) with the stage's scale replaced by 2^-k -> (data, counts); refuses data without enough
    ties (requant_edges.assert_enough_ties)"""
    data = dict(ref_module(spec.op).generate(case))
    one = np.ones(1, dtype=np.float32)
    data[scale_key(spec)] = one * np.float32(2.0 ** -k)
    if spec.op == "dwpw":
        if spec.stage == 0:
            data.update(scales1=one, bia1=None)
        else:
            data["scales0"] = one * np.float32(2.0 ** DWPW_SCALE0_LOG2)
    n = count(spec, case, data, k)
    E.assert_enough_ties(n, (spec_id(spec), case.ident(), k))
    return data, n


def odd_data(spec, data):
    """the same data with the stage's scale times 1.37: no ties"""
    key = scale_key(spec)
    return dict(data, **{key: data[key] * ODD})


def sixth_data(spec, data):
    """the same data with the stage's scale f32(1 / 6) = (1 + 2^-25) / 6 and s32 biases drawn from [-200, 200]:
    t = 3 (2 j + 1) gives t * s = (j + 1/2) (1 + 2^-25), which the multiply rounds to j + 1/2 exactly.  These ties exist
    only in the separately rounded product: a route that folds bias * scale into an fma computes
    round(acc * s + round(b * s)), and the error of round(b * s) -- up to |b| / 6 * 2^-24, an ulp or two of the results
    -- moves many of them off the tie.  (With a power-of-two scale every step of either form is exact, so the 2^-k
    data cannot tell the two apart; with generate's biases of at most 10 the error is too small to.)"""
    key = scale_key(spec)
    bkey = "bia" if spec.op != "dwpw" else ("bia0", "bia1")[spec.stage]
    bias = np.random.default_rng(77).integers(-200, 201, data[bkey].shape).astype(np.int32)
    return dict(data, **{key: np.ones(1, dtype=np.float32) * SIXTH, bkey: bias})


def count_rounded(spec, case, data):
    """ties of the f32 chain itself -- float(acc) + bias, times scale, each rounded -- inside the unsaturated range"""
    from refmath import _requant
    acc = accumulator(spec.op, spec.stage, case, data)
    mid = (spec.op, spec.stage) == ("dwpw", 0)
    bias = data["bia" if spec.op != "dwpw" else ("bia0", "bia1")[spec.stage]]
    dt, relu = (U8, True) if mid else (case.dst_dt, case.relu or case.dst_dt == U8)
    f = _requant(acc, bias, data[scale_key(spec)], False).astype(np.float64)
    fl = np.floor(f)
    lo, hi = {U8: (0, 255), S8: (-128, 127)}.get(dt, (-(1 << 31), (1 << 31) - 1))
    inside = (f - fl == 0.5) & (fl >= (max(lo, 0) if relu else lo)) & (fl + 1 <= hi)
    return dict(total=int(inside.sum()), below=int((inside & (fl % 2 == 0)).sum()), above=int((inside & (fl % 2 != 0)).sum()),
                negative=int((inside & (fl < 0)).sum()), need_negative=(not relu) and dt in (S8, S32))


def rows(spec):
    """-> [(k, dst_dt, rm, relu)] of one spec: every k x dst type x round mode, and s8 behind a ReLU at every k"""
    out = [(k, dst_dt, rm, dst_dt == U8) for k in spec.ks for dst_dt in dsts_of(spec) for rm in (0, 1)]
    if S8 in dsts_of(spec):
        out += [(k, S8, 0, True) for k in spec.ks]
    return out


# --- the dense conv the C oracle computes, where the case can be expressed as one -------------------------------------
def dense_twin(spec, case, data):
    """-> (cases.ConvCase, data) of the equivalent dense conv (dwpw: the FUSED dense conv with block-diagonal conv0
    weights), or None"""
    R = ref_module(spec.op)
    if not case.dense_expressible:
        return None
    if spec.op == "dwpw":
        return R.fused_dense_case(case), R.fused_dense_data(data)
    if spec.op == "dwconv":
        return R.dense_case(case), R.dense_data(data)
    return R.dense_case(case), R.dense_data(case, data)
