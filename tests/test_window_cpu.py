"""CPU-only checks of the window partition / reverse op: the numpy reference the GPU tests compare against (tests/window_ref.py)
equals a torch-CPU formulation of official Swin's window_partition / window_reverse / roll and of patch merging's
cat([x0, x1, x2, x3], -1); dfa.swin_shift_mask equals the official region-label construction and dfa.swin_relative_bias the
official relative_position_index gather; the case tables cover what they claim; the op's host-side plan (csrc/window_plan.h)
is clean under the host sanitizers as a stand-alone program; the C ABI validates descriptors, in the documented order, before
it touches a device; the ctypes mirrors match the header, the symbols are exported and bound, the drop-in layer and the tools
are built."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

import window_ref as W

dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-fusion_amd")
INVALID, UNSUPPORTED, HIP, NO_DEVICE, STATE = 1, 2, 3, 4, 5


# ---- 1. the reference against torch's formulation of official Swin ---------------------------------------------------------------
def _swin_window_partition(x, ws):
    """official Swin (square window): x {B, H, W, C} -> {num_windows * B, ws, ws, C}"""
    B, H, Wd, C = x.shape
    x = x.view(B, H // ws, ws, Wd // ws, ws, C)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, ws, ws, C)


def _swin_window_reverse(windows, ws, H, Wd):
    B = int(windows.shape[0] / (H * Wd / ws / ws))
    x = windows.view(B, H // ws, Wd // ws, ws, ws, -1)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(B, H, Wd, -1)


@pytest.mark.parametrize("h,w,ws,shift", [(14, 14, 7, 0), (14, 14, 7, 3), (16, 12, 7, 3), (10, 13, 7, 3), (5, 4, 7, 0), (9, 11, 4, 2), (7, 5, 2, 0),
                                          (1, 1, 2, 1), (3, 200, 7, 6)])
def test_reference_equals_official_swin(h, w, ws, shift):
    """pad (F.pad on the bottom / right), roll(-shift), window_partition; then window_reverse, roll(+shift), crop -- the block's
    own sequence in SwinTransformerBlock.forward (the padding variant of the detection / segmentation code bases)"""
    import torch
    rng = np.random.RandomState(h * 100 + w)
    x = rng.randint(0, 256, size=(3, h, w, 6)).astype(np.uint8)
    hp, wp = W.ceil_to(h, ws), W.ceil_to(w, ws)
    t = torch.nn.functional.pad(torch.from_numpy(x.astype(np.int64)), (0, 0, 0, wp - w, 0, hp - h), value=77)
    t = torch.roll(t, shifts=(-shift, -shift), dims=(1, 2)) if shift else t
    wins = _swin_window_partition(t, ws)
    got = W.partition(x, (ws, ws), (shift, shift), W.ROW_MAJOR, 77)
    assert got.dtype == np.uint8 and np.array_equal(got, wins.reshape(-1, 6).numpy())
    back = _swin_window_reverse(wins, ws, hp, wp)
    back = torch.roll(back, shifts=(shift, shift), dims=(1, 2)) if shift else back
    back = back[:, :h, :w, :].contiguous()
    assert np.array_equal(W.reverse(got, 3, h, w, (ws, ws), (shift, shift)), back.numpy()) and np.array_equal(back.numpy(), x)


def test_rectangular_windows_and_one_axis_shifts_against_torch():
    """wh != ww and a shift on one axis only, which the square official helpers do not take: the same view / permute with two
    window sizes, torch.roll with two shifts; both token orders"""
    import torch
    rng = np.random.RandomState(5)
    for h, w, wh, ww, sy, sx in ((10, 13, 3, 5, 1, 0), (10, 13, 3, 5, 0, 2), (9, 20, 3, 5, 2, 4), (4, 4, 4, 2, 3, 1), (5, 4, 7, 7, 6, 2)):
        x = rng.randint(0, 2 ** 31, size=(2, h, w, 3)).astype(np.uint32)
        hp, wp = W.ceil_to(h, wh), W.ceil_to(w, ww)
        t = torch.nn.functional.pad(torch.from_numpy(x.astype(np.int64)), (0, 0, 0, wp - w, 0, hp - h), value=5)
        t = torch.roll(t, shifts=(-sy, -sx), dims=(1, 2)).view(2, hp // wh, wh, wp // ww, ww, 3)
        row = t.permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, 3).numpy()
        col = t.permute(0, 1, 3, 4, 2, 5).contiguous().view(-1, 3).numpy()
        for order, want in ((W.ROW_MAJOR, row), (W.COL_MAJOR, col)):
            got = W.partition(x, (wh, ww), (sy, sx), order, 5)
            assert np.array_equal(got, want), (h, w, wh, ww, order)
            assert np.array_equal(W.reverse(got, 2, h, w, (wh, ww), (sy, sx), order), x)


@pytest.mark.parametrize("h,w", [(8, 6), (7, 5), (1, 1), (2, 9)])
def test_col_major_2x2_is_patch_merging(h, w):
    """official PatchMerging: pad H and W to even, x0 = x[:, 0::2, 0::2], x1 = x[:, 1::2, 0::2], x2 = x[:, 0::2, 1::2],
    x3 = x[:, 1::2, 1::2], cat([x0, x1, x2, x3], -1): the window side of a 2 x 2 column-major partition with win_ld = c, read as
    rows of 4 c"""
    import torch
    C = 5
    x = np.random.RandomState(h * 10 + w).randint(-128, 128, size=(2, h, w, C)).astype(np.int8)
    t = torch.nn.functional.pad(torch.from_numpy(x), (0, 0, 0, w % 2, 0, h % 2))
    cat = torch.cat([t[:, 0::2, 0::2, :], t[:, 1::2, 0::2, :], t[:, 0::2, 1::2, :], t[:, 1::2, 1::2, :]], -1)
    got = W.partition(x.view(np.uint8), (2, 2), (0, 0), W.COL_MAJOR, 0)
    assert np.array_equal(got.reshape(-1, 4 * C), cat.reshape(-1, 4 * C).numpy().view(np.uint8))


def test_every_case_round_trips_and_counts_its_pads():
    assert len({c.ident() for c in W.ALL_CASES}) == len(W.ALL_CASES)
    for c in W.ALL_CASES:
        grid, win = W.grid_tokens(c), W.window_tokens(c)
        assert grid.shape == (c.grid_rows, c.c) and win.shape == (c.win_rows, c.c) and grid.dtype == win.dtype == W.RAW_OF[c.esize]
        assert np.array_equal(W.reversed_tokens(c, win), grid), c.ident()
        pads = W.pad_mask(c)
        assert pads.sum() == c.bs * (c.hp * c.wp - c.h * c.w), c.ident()
        assert (win[pads] == W.pad_scalar(c)).all(), c.ident()
        # every grid token appears exactly once among the non-pad rows (the tokens are pairwise distinct)
        assert np.array_equal(np.unique(win[~pads], axis=0), np.unique(grid, axis=0)) and (~pads).sum() == c.grid_rows, c.ident()


def test_case_tables_cover_what_the_op_can_get_wrong():
    cases = W.ALL_CASES
    assert {c.bs for c in cases} >= {1, 3}
    assert {(c.h, c.w) for c in cases} >= set(W.GRIDS) and {c.window for c in cases} >= set(W.WINDOWS)
    assert any(c.window[0] > c.h and c.window[1] > c.w for c in cases)                       # a window larger than the image
    for g in W.GRIDS:
        for win in W.WINDOWS:
            kinds = {c.shift for c in cases if (c.h, c.w) == g and c.window == win and c.name == "grid"}
            hp, wp = W.ceil_to(g[0], win[0]), W.ceil_to(g[1], win[1])
            assert {(0, 0), (win[0] // 2, win[1] // 2), (hp - 1, wp - 1)} <= kinds, (g, win)
    assert any(c.shift[0] and not c.shift[1] for c in cases) and any(c.shift[1] and not c.shift[0] for c in cases)
    padding = {(c.hp > c.h, c.wp > c.w, c.shift != (0, 0)) for c in cases}
    assert {(False, False, False), (True, False, True), (False, True, True), (True, True, True), (True, True, False)} <= padding
    assert {c.order for c in cases} == {W.ROW_MAJOR, W.COL_MAJOR} and {c.dt for c in cases} == {W.U8, W.S8, W.S32, W.F32}
    assert {c.lanes for c in cases if c.row_class} >= {1, 3, 6, 17}
    assert {c.c for c in cases if not c.row_class} >= {5, 21} and any(c.gld % 16 and c.c % 16 == 0 for c in cases if not c.row_class)
    assert any(c.gld > c.c and c.row_class for c in cases) and any(c.wld > c.c and c.row_class for c in cases)
    assert {c.pad_value for c in cases if c.hp * c.wp > c.h * c.w} >= set(W.PADS)
    assert any(c.pad_value == W.PADS[2] and c.esize == 4 and c.hp * c.wp > c.h * c.w for c in cases)
    for dt in (W.U8, W.S8, W.S32, W.F32):
        assert {c.order for c in cases if c.dt == dt and c.row_class} == {W.ROW_MAJOR, W.COL_MAJOR}, dt
    assert max(W.planned_grid(c, W.PARTITION, W.ROW) for c in cases if c.row_class) > 1      # more than one workgroup


# ---- 2. the two helpers ----------------------------------------------------------------------------------------------------------
def _official_shift_mask(Hp, Wp, ws, shift):
    """SwinTransformerBlock's attn_mask (BasicLayer.forward of the padding variant), True where it holds -100"""
    import torch
    img_mask = torch.zeros((1, Hp, Wp, 1))
    h_slices = (slice(0, -ws), slice(-ws, -shift), slice(-shift, None))
    w_slices = (slice(0, -ws), slice(-ws, -shift), slice(-shift, None))
    cnt = 0
    for hs in h_slices:
        for wsl in w_slices:
            img_mask[:, hs, wsl, :] = cnt
            cnt += 1
    mask_windows = _swin_window_partition(img_mask, ws).view(-1, ws * ws)
    attn_mask = mask_windows.unsqueeze(1) - mask_windows.unsqueeze(2)
    return (attn_mask != 0).numpy()


@pytest.mark.parametrize("h,w,ws,shift", [(14, 14, 7, 3), (16, 12, 7, 3), (10, 13, 7, 3), (56, 56, 7, 3), (8, 8, 4, 2), (5, 4, 7, 3), (9, 11, 4, 1), (7, 7, 7, 3)])
def test_shift_mask_equals_the_official_construction(h, w, ws, shift):
    hp, wp = W.ceil_to(h, ws), W.ceil_to(w, ws)
    got = dfa.swin_shift_mask(h, w, ws, shift)
    nw = (hp // ws) * (wp // ws)
    assert got.dtype == np.bool_ and got.shape == (nw, ws * ws, ws * ws)
    assert np.array_equal(got, _official_shift_mask(hp, wp, ws, shift))
    assert np.array_equal(got, dfa.swin_shift_mask(h, w, (ws, ws), (shift, shift)))
    assert not got[:, np.arange(ws * ws), np.arange(ws * ws)].any() and not got.all(axis=2).any()     # a token always sees itself


def test_shift_mask_without_a_shift_and_on_one_axis():
    for h, w, win in ((14, 14, 7), (16, 12, 7), (5, 4, 7), (10, 13, (3, 5))):
        m = dfa.swin_shift_mask(h, w, win, 0)
        assert m.dtype == np.bool_ and not m.any()
    # one axis: the labels vary along that axis only, so tokens of one window column-slice agree across the other axis
    m = dfa.swin_shift_mask(8, 8, 4, (2, 0))
    assert m.shape == (4, 16, 16) and not m[:2].any() and m[2:].any()
    lab = np.repeat(np.array([0, 0, 1, 1]), 4)                                               # the last window row: rows 4, 5 | 6, 7
    assert np.array_equal(m[2], lab[:, None] != lab[None, :]) and np.array_equal(m[2], m[3])
    for bad in ((8, 8, 4, 8), (8, 8, 0, 0), (8, 8, 4, (0, -1))):
        with pytest.raises(ValueError):
            dfa.swin_shift_mask(*bad)


def test_relative_bias_equals_the_official_index():
    import torch
    for wh, ww, heads in ((7, 7, 3), (2, 2, 1), (3, 5, 2)):
        table = np.random.RandomState(wh).standard_normal(((2 * wh - 1) * (2 * ww - 1), heads)).astype(np.float32)
        coords = torch.stack(torch.meshgrid([torch.arange(wh), torch.arange(ww)], indexing="ij"))
        flat = torch.flatten(coords, 1)
        rel = (flat[:, :, None] - flat[:, None, :]).permute(1, 2, 0).contiguous()
        rel[:, :, 0] += wh - 1
        rel[:, :, 1] += ww - 1
        rel[:, :, 0] *= 2 * ww - 1
        index = rel.sum(-1)
        want = torch.from_numpy(table)[index.view(-1)].view(wh * ww, wh * ww, -1).permute(2, 0, 1).contiguous().numpy()
        got = dfa.swin_relative_bias(table, (wh, ww))
        assert got.shape == (heads, wh * ww, wh * ww) and got.dtype == np.float32 and np.array_equal(got, want)
    assert np.array_equal(dfa.swin_relative_bias(np.arange(169 * 2).reshape(169, 2), 7), dfa.swin_relative_bias(np.arange(169 * 2).reshape(169, 2), (7, 7)))
    with pytest.raises(ValueError):
        dfa.swin_relative_bias(np.zeros((168, 2)), 7)


# ---- 3. the plan under the host sanitizers ---------------------------------------------------------------------------------------
def test_window_plan_check_is_clean_under_the_host_sanitizers(tmp_path):
    """tools/window_plan_check.cc, a stand-alone host program over csrc/window_plan.h, built with the flags of the host
    Makefile's SAN=1 rule (ASan + UBSan) into a scratch directory and run directly.  Nothing is loaded into Python."""
    src = os.path.join(PKG, "tools", "window_plan_check.cc")
    assert os.path.exists(src), "tools/window_plan_check.cc is missing"
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert "$(TOOLS)/window_plan_check: $(TOOLS)/window_plan_check.cc ../csrc/window_plan.h" in mk
    exe = tmp_path / "window_plan_check"
    flags = ["-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++"] + flags + [src, "-o", str(exe)])
    p = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()
    assert "window plans: validation order, maps, pad counts, classes, grids, extents and the 2^40 limit hold" in p.stdout.decode()


# ---- 4. descriptor and build checks ----------------------------------------------------------------------------------------------
def _desc(**kw):
    d = dict(dir=capi.WINDOW_PARTITION, dt=capi.DFX_S8, bs=2, h=10, w=13, c=96, wh=7, ww=7, shift_y=3, shift_x=3, order=capi.WINDOW_ROW_MAJOR,
             grid_ld=96, win_ld=96, pad_value=0, force_path=capi.WINDOW_AUTO)
    d.update(kw)
    desc = capi.WindowDesc()
    for k, v in d.items():
        setattr(desc, k, v)
    return desc


def _create(**kw):
    desc = _desc(**kw)
    h = ctypes.c_void_p()
    rc = capi.lib().dfx_window_create(ctypes.byref(desc), ctypes.byref(h))
    msg = capi.lib().dfx_last_error().decode()
    if rc == 0:
        assert capi.lib().dfx_window_destroy(h) == 0
    else:
        assert not h.value
    return rc, msg


def _admitted(**kw):
    rc, msg = _create(**kw)
    assert rc in (0, NO_DEVICE), (kw, rc, msg)


def test_descriptor_validation_needs_no_device():
    # every refusal, in the order of the checks: a descriptor with faults i and j > i reports i
    faults = [(dict(dir=2), "dir"), (dict(dt=0), "dtype"), (dict(bs=0), "bs must"), (dict(w=0), "h and w"), (dict(c=0), "c must"), (dict(wh=256), "wh and ww"),
              (dict(order=2), "order"), (dict(shift_y=2 ** 20), "shift_y"), (dict(shift_x=2 ** 20), "shift_x"), (dict(grid_ld=95), "grid_ld"), (dict(win_ld=95), "win_ld"),
              (dict(force_path=2), "force_path"), (dict(h=4096, w=2048), "2^22"), (dict(bs=2 ** 30), "2^40")]
    for i, (kw, word) in enumerate(faults):
        rc, msg = _create(**kw)
        assert rc == INVALID and word in msg, (kw, rc, msg)
        for kw2, _ in faults[i + 1:]:
            if set(kw) & set(kw2) or ("c" in kw and ("grid_ld" in kw2 or "win_ld" in kw2)) or ("wh" in kw and "shift_y" in kw2):
                continue
            both = dict(kw2)
            both.update(kw)
            rc, msg = _create(force_path=capi.WINDOW_ROW if "force_path" not in both else both["force_path"], **{k: v for k, v in both.items() if k != "force_path"})
            assert rc == INVALID and word in msg, (both, rc, msg)
    for kw, word in ((dict(dir=-1), "dir"), (dict(dt=5), "dtype"), (dict(bs=-2), "bs must"), (dict(h=65536), "h and w"), (dict(w=65536, ww=255), "h and w"), (dict(c=-1), "c must"),
                     (dict(ww=0), "wh and ww"), (dict(wh=-7), "wh and ww"), (dict(order=-1), "order"), (dict(shift_y=-1), "shift_y"), (dict(shift_x=-1), "shift_x"), (dict(shift_y=14), "shift_y"), (dict(shift_x=14), "shift_x"),
                     (dict(force_path=-2), "force_path")):
        rc, msg = _create(**kw)
        assert rc == INVALID and word in msg, (kw, rc, msg)
    for kw in (dict(), dict(dir=capi.WINDOW_REVERSE), dict(dt=capi.DFX_F32, c=24), dict(dt=capi.DFX_S32), dict(dt=capi.DFX_U8, pad_value=0x80),
               dict(shift_y=13, shift_x=13), dict(shift_y=0, shift_x=0), dict(h=5, w=4, shift_y=6, shift_x=6), dict(wh=255, ww=255, shift_y=254, shift_x=254),
               dict(h=65535, w=1, wh=255, ww=1, shift_y=0, shift_x=0), dict(h=2048, w=2048, wh=2, ww=2, shift_y=0, shift_x=0, c=16, grid_ld=16, win_ld=16),
               dict(order=capi.WINDOW_COL_MAJOR, wh=2, ww=2, shift_y=0, shift_x=0), dict(grid_ld=100, win_ld=2 ** 31 + 4160), dict(c=5, grid_ld=5, win_ld=7),
               dict(bs=2 ** 40 // (196 * 96)), dict(force_path=capi.WINDOW_ROW), dict(force_path=capi.WINDOW_GENERIC), dict(pad_value=0xFFFFFFFF)):
        _admitted(**kw)
    assert _create(bs=2 ** 40 // (196 * 96) + 1)[0] == INVALID
    assert _create(bs=2 ** 40 // (196 * 128) + 1, win_ld=128)[0] == INVALID and _create(bs=2 ** 40 // (196 * 128) + 1, grid_ld=128, dir=capi.WINDOW_REVERSE)[0] == INVALID
    assert _create(h=2049, w=2048, wh=2, ww=2, shift_y=0, shift_x=0)[0] == INVALID
    # a forced path outside its class: unsupported, and only after everything invalid
    for kw in (dict(force_path=capi.WINDOW_ROW, c=21, grid_ld=32, win_ld=32), dict(force_path=capi.WINDOW_ROW, grid_ld=100), dict(force_path=capi.WINDOW_ROW, win_ld=97),
               dict(force_path=capi.WINDOW_ROW, dt=capi.DFX_F32, c=5, grid_ld=8, win_ld=8), dict(force_path=capi.WINDOW_ROW, dt=capi.DFX_F32, c=4, grid_ld=6, win_ld=4)):
        rc, msg = _create(**kw)
        assert rc == UNSUPPORTED and "class" in msg, (kw, rc, msg)
        assert _create(order=7, **kw)[0] == INVALID
        kw["force_path"] = capi.WINDOW_GENERIC
        _admitted(**kw)
        kw["force_path"] = capi.WINDOW_AUTO
        _admitted(**kw)
    _admitted(force_path=capi.WINDOW_ROW, dt=capi.DFX_F32, c=4, grid_ld=8, win_ld=4)
    lib = capi.lib()
    assert lib.dfx_window_create(None, None) == INVALID
    assert lib.dfx_window_submit(None, None, None, None) == INVALID
    assert lib.dfx_window_query(None, None) == INVALID
    assert lib.dfx_debug_window_launches(None) == INVALID
    assert lib.dfx_window_destroy(None) == 0
    assert "null" in lib.dfx_last_error().decode()


def test_valid_descriptors_and_no_cpu_fallback():
    import torch
    for kw in (dict(), dict(dir=capi.WINDOW_REVERSE, dt=capi.DFX_F32, c=24), dict(force_path=capi.WINDOW_ROW)):
        rc, msg = _create(**kw)
        if torch.cuda.is_available():
            assert rc == 0, (kw, msg)
        else:
            assert rc == NO_DEVICE and "no HIP device" in msg, (kw, rc, msg)
    if not torch.cuda.is_available():
        with pytest.raises(dfa.DfxError) as e:
            dfa.WindowOp(dfa.WINDOW_PARTITION, 2, 16, 12, 64, 7, shift=3)
        assert "dfx error 4" in str(e.value) and "no HIP device" in str(e.value)
    with pytest.raises(dfa.DfxError, match="dfx error 1.*shift_y"):
        dfa.WindowOp(dfa.WINDOW_PARTITION, 2, 16, 12, 64, 7, shift=21)
    with pytest.raises(dfa.DfxError, match="dfx error 2.*class"):
        dfa.WindowOp(dfa.WINDOW_REVERSE, 2, 16, 12, 21, (7, 7), force_path=dfa.WINDOW_ROW)


def test_window_structs_match_the_header(tmp_path):
    """dfx_window_desc / dfx_window_info compiled by gcc have the sizes and field offsets of the ctypes mirrors"""
    pairs = {"dfx_window_desc": capi.WindowDesc, "dfx_window_info": capi.WindowInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dfx.h"', 'int main(void) {']
    for cname, ct in pairs.items():
        lines.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in ct._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    enums = ("DFX_WINDOW_PARTITION", "DFX_WINDOW_REVERSE", "DFX_WINDOW_ROW_MAJOR", "DFX_WINDOW_COL_MAJOR", "DFX_WINDOW_ROW", "DFX_WINDOW_GENERIC",
             "DFX_WINDOW_MAX_HW", "DFX_WINDOW_MAX_WIN", "DFX_WINDOW_MAX_PADDED", "DFX_VERSION")
    for name in enums:
        lines.append('printf("enum %s %%d\\n", %s);' % (name, name))
    lines.append('printf("dfx_lnorm_desc size %zu\\n", sizeof(dfx_lnorm_desc));')
    lines.append("return 0; }")
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = {}
    for ln in subprocess.check_output([str(exe)]).decode().splitlines():
        a, b, c = ln.split()
        seen[(a, b)] = int(c)
    for cname, ct in pairs.items():
        assert seen[(cname, "size")] == ctypes.sizeof(ct), cname
        for fname, _ in ct._fields_:
            assert seen[(cname, fname)] == getattr(ct, fname).offset, (cname, fname)
    assert [n for n, _ in capi.WindowDesc._fields_] == ["dir", "dt", "bs", "h", "w", "c", "wh", "ww", "shift_y", "shift_x", "order", "grid_ld", "win_ld", "pad_value",
                                                        "force_path"]
    assert [n for n, _ in capi.WindowInfo._fields_] == ["path", "grid", "block", "device", "algorithmic_bytes", "kernel_name"]
    assert seen[("enum", "DFX_WINDOW_PARTITION")] == capi.WINDOW_PARTITION == W.PARTITION == 0 and seen[("enum", "DFX_WINDOW_REVERSE")] == capi.WINDOW_REVERSE == W.REVERSE == 1
    assert seen[("enum", "DFX_WINDOW_ROW_MAJOR")] == capi.WINDOW_ROW_MAJOR == W.ROW_MAJOR == 0 and seen[("enum", "DFX_WINDOW_COL_MAJOR")] == capi.WINDOW_COL_MAJOR == W.COL_MAJOR == 1
    assert seen[("enum", "DFX_WINDOW_ROW")] == capi.WINDOW_ROW == W.ROW == 0 and seen[("enum", "DFX_WINDOW_GENERIC")] == capi.WINDOW_GENERIC == W.GENERIC == 1
    assert capi.WINDOW_AUTO == W.AUTO == -1 and seen[("enum", "DFX_VERSION")] == 100
    assert (seen[("enum", "DFX_WINDOW_MAX_HW")], seen[("enum", "DFX_WINDOW_MAX_WIN")], seen[("enum", "DFX_WINDOW_MAX_PADDED")]) == \
        (capi.WINDOW_MAX_HW, capi.WINDOW_MAX_WIN, capi.WINDOW_MAX_PADDED) == (65535, 255, 2 ** 22)
    assert ctypes.sizeof(capi.WindowDesc) == 72
    assert ctypes.sizeof(capi.LnormDesc) == seen[("dfx_lnorm_desc", "size")]            # the others are untouched
    assert (W.F32, W.S32, W.S8, W.U8) == (capi.DFX_F32, capi.DFX_S32, capi.DFX_S8, capi.DFX_U8)


def test_library_exports_the_window_entry_points():
    lib = capi.lib()
    for s in ("dfx_window_create", "dfx_window_submit", "dfx_window_query", "dfx_window_destroy", "dfx_debug_window_launches"):
        assert s in dfa.declared_symbols() and hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s                              # bound with a signature
    assert not [s for s in dfa.declared_symbols() if not hasattr(lib, s)]
    assert [s for s in dfa.declared_symbols() if "window" in s] == sorted(
        ["dfx_window_create", "dfx_window_submit", "dfx_window_query", "dfx_window_destroy", "dfx_debug_window_launches"])
    for name in ("WindowOp", "WindowDesc", "WindowInfo", "WINDOW_AUTO", "WINDOW_ROW", "WINDOW_GENERIC", "WINDOW_PARTITION", "WINDOW_REVERSE", "WINDOW_ROW_MAJOR",
                 "WINDOW_COL_MAJOR", "window_launches", "swin_shift_mask", "swin_relative_bias"):
        assert hasattr(dfa, name), name
    assert all(v >= 0 for v in dfa.window_launches())
    capi.set_tuning("DFX_WINDOW_GRID", "1")                                         # known to the library
    capi.set_tuning("DFX_WINDOW_GRID", None)
    with pytest.raises(dfa.DfxError):
        capi.set_tuning("DFX_WINDOW_ROWS", "1")
    header = open(os.path.join(ROOT, "include", "dfx.h")).read()
    assert "DFX_WINDOW_AUTO_NOTE" in header


def test_dropin_layer_exports_the_window_ops_and_tools_are_built():
    so = os.path.join(PKG, "libdeepfusion.so")
    assert os.path.exists(so), "run __graft_entry__.build() first"
    syms = subprocess.check_output(["nm", "-D", "-C", "--defined-only", so]).decode()
    assert "deepfusion::window_partition(" in syms and "deepfusion::window_reverse(" in syms
    for tool in ("window_check", "window_plan_check", "bench_window"):
        exe = os.path.join(PKG, "tools", tool)
        assert os.path.exists(exe) and os.access(exe, os.X_OK), tool
    p = subprocess.run([os.path.join(PKG, "tools", "window_plan_check")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0 and "the 2^40 limit hold" in p.stdout.decode(), p.stdout.decode()
    ignore = open(os.path.join(ROOT, ".gitignore")).read().split()
    for tool in ("window_check", "window_plan_check", "bench_window"):
        assert "deep-fusion_amd/tools/" + tool in ignore, tool
    # the trace stub knows the new C-ABI calls: coherence_check links against it
    stub = open(os.path.join(PKG, "tools", "dfx_trace_stub.cc")).read()
    for s in ("dfx_window_create", "dfx_window_submit", "dfx_window_destroy"):
        assert "int %s(" % s in stub, s
    # the op joins neither pipeline_net.h nor the token net: the recorded coherence traces stay as they are
    assert "window_partition" not in open(os.path.join(PKG, "tools", "pipeline_net.h")).read()
