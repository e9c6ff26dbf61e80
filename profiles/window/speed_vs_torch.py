"""The window partition / reverse op (dfx_window_*) against what a caller does today in eager PyTorch on the same int8 device
tensors: F.pad to a multiple of the window (where the map is none), torch.roll by the shift, view + permute + contiguous (Swin's
window_partition); for patch merging the four strided slices and torch.cat.  Both forced kernels of the op are timed, so the
table does not depend on the auto rule.  Buffers in rotation beyond the Infinity Cache, CUDA events, windows of at least 3 ms,
median of 5 rounds.  Run from the repository root on an MI355X:
    python profiles/window/speed_vs_torch.py > profiles/window/speed_vs_torch.txt"""
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
dfa = importlib.import_module("deep-fusion_amd")


def timed(fn, nsets, rounds=5, window_ms=3.0):
    def window(iters):
        for i in range(3):
            fn(i % nsets)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            fn(i % nsets)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters
    iters = int(min(5000, max(20, np.ceil(window_ms * 1.25 / max(window(10), 1e-4)))))
    return sorted(window(iters) * 1000.0 for _ in range(rounds))[rounds // 2]


def point(name, bs, h, w, c, win, shift, merge=False):
    hp, wp = -(-h // win) * win, -(-w // win) * win
    nsets = max(1, min(64, (768 << 20) // (bs * (h * w + hp * wp) * c) + 1))
    g = torch.Generator(device="cuda").manual_seed(3)
    srcs = [torch.randint(-128, 128, (bs, h, w, c), dtype=torch.int8, device="cuda", generator=g) for _ in range(nsets)]
    outs = [torch.empty(bs * hp * wp, c, dtype=torch.int8, device="cuda") for _ in range(nsets)]
    ours = {}
    for path, tag in ((dfa.WINDOW_ROW, "row"), (dfa.WINDOW_GENERIC, "generic")):
        op = dfa.WindowOp(dfa.WINDOW_PARTITION, bs, h, w, c, win, shift=shift, order=dfa.WINDOW_COL_MAJOR if merge else dfa.WINDOW_ROW_MAJOR,
                          dtype=np.int8, force_path=path)
        ours[tag] = timed(lambda i: op.submit(srcs[i], outs[i]), nsets)
        op.close()

    def eager(i):
        x = srcs[i]
        if hp > h or wp > w:
            x = torch.nn.functional.pad(x, (0, 0, 0, wp - w, 0, hp - h))
        if merge:
            return torch.cat([x[:, 0::2, 0::2, :], x[:, 1::2, 0::2, :], x[:, 0::2, 1::2, :], x[:, 1::2, 1::2, :]], -1)
        if shift:
            x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
        return x.view(bs, hp // win, win, wp // win, win, c).permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, win, win, c)
    theirs = timed(eager, nsets)
    print("%-34s row %.1f us, generic %.1f us, eager torch %.1f us, torch / row %.2f, torch / generic %.2f" %
          (name, ours["row"], ours["generic"], theirs, theirs / ours["row"], theirs / ours["generic"]))


if __name__ == "__main__":
    assert torch.cuda.is_available()
    stages = (("swin-t s1 56x56x96", 56, 96), ("swin-t s2 28x28x192", 28, 192), ("swin-t s3 14x14x384", 14, 384), ("swin-t s4 7x7x768", 7, 768))
    for bs in (1, 64):
        for name, hw, c in stages:
            for shift in (0, 3):
                point("%s bs%d shift%d" % (name, bs, shift), bs, hw, hw, c, 7, shift)
    for shift in (0, 3):
        point("det 200x304x96 bs2 shift%d" % shift, 2, 200, 304, 96, 7, shift)
    for bs in (1, 64):
        for name, hw, c in stages[:3]:
            point("merge %dx%dx%d bs%d" % (hw, hw, c, bs), bs, hw, hw, c, 2, 0, merge=True)
