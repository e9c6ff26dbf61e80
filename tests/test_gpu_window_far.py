"""GPU: the 64-bit offsets of the window partition / reverse op (dfx_window_*), past 2^31 and 2^32 bytes: one case per direction
and far operand in the layouts H and F of tests/far_offsets.py, on both kernels, with 1- and 4-byte elements.  The constants
and the arena helpers are those of the far-offset suite (tests/far_offsets.py, tests/test_gpu_far_offsets.py).

The shape is a 1 x 3 grid under a 1 x 3 window with shift_x = 1, so the three tokens are permuted (window row i <- grid token
(i + 1) mod 3), and the far operand's pitch carries the reach as the lnorm rows of that table do: three rows of PITCH3[layout]
bytes put row 2 into [2^31, 2^31 + 2^26) (H: a signed 32-bit offset goes wrong) or into [2^32, 2^32 + 2^26) (F: a truncated one
does, and row 1 sits in [2^31, 2^32)).  The far operand lies in the poisoned arena, the other one is small, dense and guarded.
A wrapped read sees poison and gives wrong values; a wrapped write damages poison inside the arena."""
import importlib

import numpy as np
import pytest

import far_offsets as F
import hipref
import window_ref as W
from test_gpu_far_offsets import arena, arena_holder, assert_clean, guarded, on_device, put, ran_only, segments, wipe, GUARD  # noqa: F401

pytestmark = pytest.mark.gpu
dfa = importlib.import_module("deep-fusion_amd")


def far_cases():
    out = []
    for layout in ("H", "F"):
        for dt, c in ((W.S8, 48), (W.F32, 12)):
            for direction in (W.PARTITION, W.REVERSE):
                for operand in ("src", "dst"):
                    out.append((layout, dt, c, direction, operand))
    return out


def ident(p):
    layout, dt, c, direction, operand = p
    return "%s-%s-%s-%s" % ("partition" if direction == W.PARTITION else "reverse", operand, W.NAME_OF[dt], layout)


@pytest.mark.parametrize("p", far_cases(), ids=ident)
def test_window_far(arena, p):
    import torch
    layout, dt, c, direction, operand = p
    esz = W.SIZE_OF[dt]
    pitch = F.PITCH3[layout] // esz                                            # elements
    assert F.in_window(layout, 2 * pitch * esz) and (layout == "H" or F.P31 <= pitch * esz < F.P32)
    far_is_grid = (direction == W.PARTITION) == (operand == "src")
    case = W.WinCase("far", 1, 1, 3, c, (1, 3), (0, 1), W.ROW_MAJOR, dt, grid_ld=pitch if far_is_grid else 0, win_ld=0 if far_is_grid else pitch,
                     seed=60 + esz)
    dense = W.WinCase("far", 1, 1, 3, c, (1, 3), (0, 1), W.ROW_MAJOR, dt, seed=60 + esz)
    grid, win = W.grid_tokens(dense), W.window_tokens(dense)
    assert np.array_equal(win, grid[[1, 2, 0]])                                # the permutation the shift makes
    src, want = (grid, win) if direction == W.PARTITION else (win, grid)
    far = F.Far(esz, tuple(r * pitch for r in range(3)), c)
    assert list(far.far_segments()) == ([2] if layout == "H" else [1, 2])
    for path in (W.ROW, W.GENERIC):
        op = dfa.WindowOp(direction, 1, 1, 3, c, (1, 3), shift=(0, 1), dtype=W.NP_OF[dt], grid_ld=case.gld, win_ld=case.wld, force_path=path)
        what = "%s [%s]" % (ident(p), op.info().kernel_name.decode())
        try:
            arena.fill_(hipref.POISON_BYTE)
            segs = segments(arena, far)
            before = dfa.window_launches()
            if operand == "src":
                put(segs, torch.from_numpy(np.ascontiguousarray(src).view(np.uint8).reshape(3, c * esz).copy()).cuda())
                buf, mid = guarded(3 * c * esz)
                torch.cuda.synchronize()
                op.submit(arena.data_ptr() + F.BASE, mid)
                torch.cuda.synchronize()
                assert bool((buf[:GUARD] == hipref.GUARD_BYTE).all()) and bool((buf[GUARD + mid.numel():] == hipref.GUARD_BYTE).all()), what + ": a guard band was overwritten"
                got = mid.cpu().numpy()
            else:
                dev = on_device(src)
                torch.cuda.synchronize()
                op.submit(dev, arena.data_ptr() + F.BASE)
                torch.cuda.synchronize()
                got = torch.cat(segs).cpu().numpy().reshape(-1)
            ran_only(before, dfa.window_launches(), path, what)
            wipe(segs)
            assert_clean(arena, what)                                          # first: a wrapped write names its place
            hipref.assert_bit_equal(got.view(W.RAW_OF[esz]).reshape(3, c), want, what)
        finally:
            op.close()
