"""The six single-weight-set conv ops (dwconv, gconv, imgconv, deconv, dilconv, fc) share one host-side skeleton
(csrc/weighted_op.h).  This pins what a caller sees of every refusal that needs no device: the return code and the
dfx_last_error() text, byte for byte, of every clause of each op's descriptor validation (by a descriptor that reaches
that clause and no earlier one), of one forced-path refusal per op and of a null-argument call of every entry point.
tests/golden/weighted_op_errors.json was recorded from the library as it was before the skeleton existed."""
import ctypes
import importlib
import json
import os

import pytest

capi = importlib.import_module("deep-fusion_amd.capi")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "weighted_op_errors.json")

_TAIL = dict(dst_dt=capi.DFX_U8, bia_dt=capi.DFX_UNDEF, relu=0, round_mode=capi.ROUND_NEAREST, nscales=1, force_path=-1)
_CONV = dict(bs=2, ic=32, ih=9, iw=11, oc=32, oh=9, ow=11, kh=3, kw=3, sh=1, sw=1, pad_t=1, pad_l=1, **_TAIL)
_SRC_2P31 = dict(bs=1 << 11, ih=1 << 10, iw=1 << 10, oh=1, ow=1)       # exactly 2^31 source pixels
# the clauses every op's validation ends with, in their order
_TAIL_CLAUSES = [("dst_dtype", dict(dst_dt=9)), ("bias_dtype", dict(bia_dt=7)), ("round_mode", dict(round_mode=2)),
                 ("scales", dict(nscales=4)), ("force_path", dict(force_path=2))]

# op -> (descriptor class, a valid descriptor, [(clause, what to change in it)] in the order of the op's checks, and the
# forced fast path on a shape outside its class)
OPS = {
    "dwconv": (capi.DwConvDesc,
               dict(bs=2, c=32, ih=9, iw=11, oh=9, ow=11, kh=3, kw=3, sh=1, sw=1, pad_t=1, pad_l=1, **_TAIL),
               [("dimension", dict(bs=0)), ("window_zero", dict(kh=0)), ("window_256", dict(kw=256)), ("stride", dict(sh=0)),
                ("padding", dict(pad_l=-1)), ("last_window", dict(oh=11)), ("pixels", _SRC_2P31)],
               dict(force_path=capi.DWCONV_WINDOW, kh=7, kw=7, pad_t=3, pad_l=3)),
    "gconv": (capi.GConvDesc, dict(_CONV, groups=4),
              [("dimension", dict(kh=0)), ("stride", dict(sw=0)), ("padding", dict(pad_t=-1)), ("groups", dict(groups=0)),
               ("divisible", dict(groups=3)), ("taps", dict(ic=255, oc=255, groups=1, kh=15, kw=18, pad_t=7, pad_l=8)),
               ("last_window", dict(ow=13)), ("pixels", _SRC_2P31)],
              dict(force_path=capi.GCONV_MFMA, kh=5, kw=5, pad_t=2, pad_l=2)),
    "imgconv": (capi.ImgConvDesc, dict(_CONV, ic=3),
                [("dimension", dict(oc=0)), ("channels", dict(ic=5)), ("window", dict(kh=256)), ("stride", dict(sh=-1)),
                 ("padding", dict(pad_l=-2)), ("taps", dict(ic=4, kh=128, kw=128)), ("last_window", dict(oh=11)),
                 ("pixels", _SRC_2P31)],
                dict(force_path=capi.IMGCONV_MFMA, ic=2)),
    "deconv": (capi.DeconvDesc, dict(_CONV, ih=5, iw=6, oh=10, ow=12, kh=2, kw=2, sh=2, sw=2, pad_t=0, pad_l=0),
               [("dimension", dict(iw=0)), ("window", dict(kw=256)), ("stride", dict(sh=256)), ("padding", dict(pad_t=-1)),
                ("padding_k", dict(pad_l=2)), ("taps", dict(ic=32 * 600, kh=2, kw=2)), ("output", dict(oh=11)),
                ("pixels", _SRC_2P31)],
               dict(force_path=capi.DECONV_MFMA, sh=1, sw=1, oh=6, ow=7)),
    "dilconv": (capi.DilConvDesc, dict(_CONV, iw=10, ow=10, dh=2, dw=2, pad_t=2, pad_l=2),
                [("dimension", dict(ow=0)), ("window", dict(kh=256)), ("stride", dict(sw=0)), ("dilation", dict(dh=256)),
                 ("padding", dict(pad_t=-1)), ("padding_k", dict(pad_l=5)), ("taps", dict(ic=7226)),
                 ("last_window", dict(oh=13)), ("pixels", _SRC_2P31)],
                dict(force_path=capi.DILCONV_MFMA, sh=2, sw=2, oh=5, ow=5)),
    "fc": (capi.FcDesc, dict(bs=2, ic=64, ih=1, iw=1, oc=10, **_TAIL),
           [("dimension", dict(oc=0)), ("taps_hw", dict(ih=256, iw=256, ic=1)), ("taps", dict(ic=65026)),
            ("outputs", dict(bs=1 << 16, oc=1 << 15)), ("batch", dict(bs=(1 << 31) - 31, oc=1))],
           dict(force_path=capi.FC_MFMA, ic=63)),
}


def _calls(op):
    """(id, call) of every pinned call of one op; a call returns the code"""
    L = capi.lib()
    desc_t, base, clauses, forced = OPS[op]
    fn = lambda name: getattr(L, "dfx_%s_%s" % (op, name))  # noqa: E731

    def create(**kw):
        def call():
            h = ctypes.c_void_p()
            rc = fn("create")(ctypes.byref(desc_t(**dict(base, **kw))), ctypes.byref(h))
            assert rc != 0 and not h.value, "a refusal is pinned here, not a handle"
            return rc
        return call

    out = [("%s.validate.%s" % (op, name), create(**kw)) for name, kw in clauses + _TAIL_CLAUSES]
    out.append(("%s.forced_path" % op, create(**forced)))
    out += [
        ("%s.null.create_desc" % op, lambda: fn("create")(None, ctypes.byref(ctypes.c_void_p()))),
        ("%s.null.create_out" % op, lambda: fn("create")(ctypes.byref(desc_t(**base)), None)),
        ("%s.null.set_weights" % op, lambda: fn("set_weights")(None, None, None, None)),
        ("%s.null.submit" % op, lambda: fn("submit")(None, None, None, None)),
        ("%s.null.submit_host" % op, lambda: fn("submit_host")(None, None, None)),
        ("%s.null.query" % op, lambda: fn("query")(None, None)),
        ("%s.null.requant" % op, lambda: getattr(L, "dfx_debug_%s_requant" % op)(None, None)),
        ("%s.null.destroy" % op, lambda: fn("destroy")(None)),
    ]
    return out


def observe():
    """id -> [return code, dfx_last_error() text ("" where the call succeeds: the text is the last FAILURE's)]"""
    seen = {}
    for op in OPS:
        for ident, call in _calls(op):
            assert ident not in seen, ident
            rc = call()
            seen[ident] = [rc, capi.lib().dfx_last_error().decode() if rc else ""]
    return seen


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_refusal_has_the_recorded_code_and_text(golden):
    seen = observe()
    assert len(seen) >= 6 * (5 + 5 + 1 + 8)
    for ident, got in seen.items():
        assert ident in golden, "no fixture line for %s" % ident
        assert got == golden[ident], (ident, got, golden[ident])
    assert sorted(golden) == sorted(seen), "fixture lines without a call"


def test_each_validation_clause_is_reached_by_its_own_descriptor(golden):
    """the recorded texts of one op's clauses differ pairwise and carry the op's name: no descriptor of the table stops
    at an earlier clause than the one it is there for"""
    for op, (_, _, clauses, _) in OPS.items():
        texts = [golden["%s.validate.%s" % (op, name)][1] for name, _ in clauses + _TAIL_CLAUSES]
        assert all(t.startswith(op + ": ") for t in texts), (op, texts)
        same_clause = {"window_zero": "window_256", "taps_hw": "taps"}          # two ways into one clause
        distinct = [t for (name, _), t in zip(clauses + _TAIL_CLAUSES, texts) if name not in same_clause]
        assert len(set(distinct)) == len(distinct), (op, texts)
        assert golden["%s.forced_path" % op][1].startswith("%s_create: shape outside" % op)
