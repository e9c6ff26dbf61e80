"""The twelve ops that plan a fast and a generic path (resize, wsum, head, select, nms, roialign, bmm, attn, lnorm, linear,
patchembed, window) share their host-side frame (csrc/path_op.h).  This pins what a caller sees of the refusals that frame
words: the return code and the dfx_last_error() text, byte for byte, of a null desc and a null out at create, of one
descriptor stopped by the first clause of the op's validation (the "op: why" framing), of the forced-path refusal where the
op has one, and of a null call of every other entry point, the debug hooks included.  None of these calls reaches a device
call, so the fixture is the same with and without a GPU; a successful create is not pinned.
tests/golden/path_op_errors.json was recorded from the library as it was before path_op.h existed."""
import ctypes
import importlib
import json
import os

import pytest

import attn_ref
import bmm_ref

capi = importlib.import_module("deep-fusion_amd.capi")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "path_op_errors.json")


def _fill(desc_t, **kw):
    desc = desc_t()
    for k, v in kw.items():
        if isinstance(v, (tuple, list)):
            for i, x in enumerate(v):
                getattr(desc, k)[i] = x
        else:
            setattr(desc, k, v)
    return desc


# op -> (descriptor class, the valid descriptor of the op's test_X_cpu.py, what stops it at the first clause of the op's
# validation, what forces the fast path outside its class (None: create has no such refusal), and the arguments of a null
# call of every entry point but create and destroy)
OPS = {
    "resize": (capi.ResizeDesc,
               dict(bs=2, c=16, ih=5, iw=7, oh=10, ow=14, dt=capi.DFX_U8, algo=capi.RESIZE_BILINEAR, coord=capi.COORD_HALF_PIXEL,
                    add=0, post_relu=0, force_path=capi.RESIZE_AUTO),
               dict(bs=0), dict(c=3, force_path=capi.RESIZE_BAND),
               dict(submit=(None,) * 5, submit_host=(None,) * 4, query=(None, None))),
    "wsum": (capi.WsumDesc,
             dict(bs=2, h=5, w=7, c=32, n_inputs=2, src_dt=(capi.DFX_U8, capi.DFX_S8), nscales=(1, 32), n_bias=0, dst_dt=capi.DFX_U8,
                  round_mode=capi.ROUND_NEAREST, post_relu=0, lut_in_dt=capi.DFX_UNDEF, force_path=capi.WSUM_AUTO),
             dict(bs=0), dict(c=24, nscales=(1, 24), force_path=capi.WSUM_VEC),
             dict(set_params=(None,) * 4, submit=(None,) * 4, submit_host=(None,) * 3, query=(None, None))),
    "head": (capi.HeadDesc,
             dict(rows=70, mode=capi.HEAD_TOPK, src_dt=capi.DFX_U8, dst_dt=capi.DFX_U8, c=21, src_ld=32, dst_ld=21, idx_ld=1, k=1,
                  out_scale=255.0, force_path=capi.HEAD_AUTO),
             dict(mode=7), dict(src_ld=24, force_path=capi.HEAD_ROW),
             dict(set_table=(None, None), submit=(None,) * 5, query=(None, None))),
    "select": (capi.SelectDesc,
               dict(bs=2, h=5, w=7, c=21, src_dt=capi.DFX_U8, k=100, src_ld=32, idx_ld=100, peak=capi.SELECT_ALL, min_val=0,
                    n_gather=0, force_path=capi.SELECT_AUTO),
               dict(bs=0), dict(src_ld=21, force_path=capi.SELECT_HIST),
               dict(submit=(None,) * 8, query=(None, None))),
    "nms": (capi.NmsDesc,
            dict(bs=2, n=100, max_out=50, keep_ld=50, mode=capi.NMS_DECODE, per_class=1, classes=80, anchors_per_pixel=9,
                 n_anchors=1000, row_bytes=36, idx_ld=100, iou_thr=0.5, clip_w=0.0, clip_h=0.0, force_path=capi.NMS_AUTO),
            dict(bs=0), None,
            dict(submit=(None,) * 3, query=(None, None))),
    "roialign": (capi.RoiAlignDesc,
                 dict(bs=1, n=3, mode=capi.ROI_BATCHED, levels=1, c=16, dt=capi.DFX_U8, h=(5,), w=(5,), src_ld=(16,),
                      spatial_scale=(1.0,), ph=7, pw=7, sampling_ratio=2, aligned=0, dst_ld=16, force_path=capi.ROIALIGN_AUTO),
                 dict(bs=0), None,
                 dict(submit=(None,) * 3, query=(None, None))),
    "bmm": (capi.BmmDesc, bmm_ref.desc_of(bmm_ref.BmmCase("v", 33, 37, 40, batch=(2, 3))),
            dict(m=0), None,
            dict(set_scales=(None, None), set_bias=(None,) * 3, submit=(None,) * 5, query=(None, None), debug_requant=(None, None))),
    "attn": (capi.AttnDesc, attn_ref.desc_of(attn_ref.AttnCase("v", 33, 37, 40, 35, batch=(2, 3))),
             dict(tq=0), None,
             dict(set_table=(None, None), set_scales=(None, ctypes.c_float(1.0), None), set_bias=(None,) * 3, submit=(None,) * 6,
                  query=(None, None))),
    "lnorm": (capi.LnormDesc,
              dict(rows=70, mode=capi.LNORM_LAYER, src_dt=capi.DFX_S8, dst_dt=capi.DFX_S8, c=96, src_ld=96, dst_ld=96, eps=1e-3,
                   force_path=capi.LNORM_AUTO),
              dict(mode=7), dict(src_ld=100, force_path=capi.LNORM_ROW),
              dict(set_params=(None,) * 4, submit=(None,) * 4, query=(None, None))),
    "linear": (capi.LinearDesc,
               dict(rows=70, k=96, n=40, src_dt=capi.DFX_S8, dst_dt=capi.DFX_S8, bia_dt=capi.DFX_UNDEF, relu=0, round_mode=0, nscales=1,
                    lut_in_dt=capi.DFX_UNDEF, force_path=capi.LINEAR_AUTO, src_ld=96, dst_ld=40),
               dict(rows=0), None,
               dict(set_weights=(None,) * 4, set_table=(None, None), submit=(None,) * 4, submit_host=(None,) * 3, query=(None, None),
                    debug_requant=(None, None))),
    "patchembed": (capi.PatchEmbedDesc,
                   dict(bs=2, ih=12, iw=20, ic=4, ph=4, pw=4, th=3, tw=5, oc=40, src_dt=capi.DFX_U8, dst_dt=capi.DFX_S8,
                        bia_dt=capi.DFX_UNDEF, relu=0, round_mode=0, nscales=1, table=0, tok_offset=0,
                        force_path=capi.PATCHEMBED_AUTO, img_rows=15, dst_ld=40),
                   dict(bs=0), None,
                   dict(set_weights=(None,) * 4, set_table=(None, None, 0), set_prefix=(None, None), submit=(None,) * 4,
                        submit_host=(None,) * 3, query=(None, None), debug_requant=(None, None))),
    "window": (capi.WindowDesc,
               dict(dir=capi.WINDOW_PARTITION, dt=capi.DFX_S8, bs=2, h=10, w=13, c=96, wh=7, ww=7, shift_y=3, shift_x=3,
                    order=capi.WINDOW_ROW_MAJOR, grid_ld=96, win_ld=96, pad_value=0, force_path=capi.WINDOW_AUTO),
               dict(dir=7), dict(c=20, grid_ld=20, win_ld=20, force_path=capi.WINDOW_ROW),
               dict(submit=(None,) * 4, query=(None, None))),
}


def _calls(op):
    """(id, call) of every pinned call of one op; a call returns the code"""
    L = capi.lib()
    desc_t, base, first, forced, nulls = OPS[op]
    create = getattr(L, "dfx_%s_create" % op)

    def refused(**kw):
        def call():
            h = ctypes.c_void_p()
            rc = create(ctypes.byref(_fill(desc_t, **dict(base, **kw))), ctypes.byref(h))
            assert rc != 0 and not h.value, "a refusal is pinned here, not a handle"
            return rc
        return call

    def entry(name, args):
        sym = "dfx_debug_%s_%s" % (op, name[len("debug_"):]) if name.startswith("debug_") else "dfx_%s_%s" % (op, name)
        return lambda: getattr(L, sym)(*args)

    out = [
        ("%s.null.create_desc" % op, lambda: create(None, ctypes.byref(ctypes.c_void_p()))),
        ("%s.null.create_out" % op, lambda: create(ctypes.byref(_fill(desc_t, **base)), None)),
        ("%s.validate.first" % op, refused(**first)),
    ]
    if forced is not None:
        out.append(("%s.forced_path" % op, refused(**forced)))
    out += [("%s.null.%s" % (op, name), entry(name, args)) for name, args in nulls.items()]
    out += [("%s.null.debug_launches" % op, entry("debug_launches", (None,))), ("%s.null.destroy" % op, entry("destroy", (None,)))]
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
    for ident, got in seen.items():
        assert ident in golden, "no fixture line for %s" % ident
        assert got == golden[ident], (ident, got, golden[ident])
    assert sorted(golden) == sorted(seen), "fixture lines without a call"
    for op in OPS:
        assert sum(ident.startswith(op + ".") for ident in golden) >= 6, op


def test_the_table_calls_every_entry_point_the_header_declares(golden):
    """a null call of EVERY entry point: what include/dfx.h declares for the twelve ops is what the table calls"""
    declared = set(s for s in capi.declared_symbols() for op in OPS if s.startswith("dfx_%s_" % op) or s.startswith("dfx_debug_%s_" % op))
    called = set()
    for op, (_, _, _, _, nulls) in OPS.items():
        called |= {"dfx_%s_create" % op, "dfx_%s_destroy" % op, "dfx_debug_%s_launches" % op}
        called |= {"dfx_debug_%s_%s" % (op, n[6:]) if n.startswith("debug_") else "dfx_%s_%s" % (op, n) for n in nulls}
    assert called == declared, (sorted(declared - called), sorted(called - declared))


def test_the_recorded_texts_carry_the_frame(golden):
    """the framing the shared helpers word: X_create's null argument, "X: why", the forced path's class, debug_X_launches"""
    for op, (_, _, _, forced, _) in OPS.items():
        assert golden["%s.null.create_desc" % op] == golden["%s.null.create_out" % op] == [1, "%s_create: null argument" % op]
        rc, text = golden["%s.validate.first" % op]
        assert rc == 1 and text.startswith(op + ": "), (op, text)
        if forced is not None:
            rc, text = golden["%s.forced_path" % op]
            assert rc == 2 and text.startswith("%s_create: " % op) and "class" in text, (op, text)
        assert golden["%s.null.debug_launches" % op] == [1, "debug_%s_launches: null argument" % op]
        assert golden["%s.null.query" % op] == [1, "%s_query: null argument" % op]
        assert golden["%s.null.destroy" % op] == [0, ""]
