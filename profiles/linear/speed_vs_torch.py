"""The int8 token linear op (dfx_linear_*) against what a caller has in eager PyTorch on the same device tensors: torch._int_mm
(s8 x s8 -> s32, no requant) and an f16 torch.matmul of pre-converted operands.  The conversions are NOT charged to torch, and
neither leg requantises: both do LESS than the op.  Both tile heights and the generic kernel of the op are timed through
force_path, so the table does not depend on the auto rule.  Buffers in rotation beyond the Infinity Cache, CUDA events, windows
of at least 3 ms, median of 5 rounds with the extremes.  Run from the repository root on an MI355X:
    python profiles/linear/speed_vs_torch.py > profiles/linear/speed_vs_torch.txt"""
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")


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
    iters = int(min(5000, max(4, np.ceil(window_ms * 1.25 / max(window(4), 1e-4)))))
    us = sorted(window(iters) * 1000.0 for _ in range(rounds))
    return us[rounds // 2], us[0], us[-1]


def point(name, rows, k, n, with_generic):
    nsets = max(1, min(64, (768 << 20) // (rows * (k + n)) + 1))
    g = torch.Generator(device="cuda").manual_seed(3)
    srcs = [torch.randint(-128, 128, (rows, k), dtype=torch.int8, device="cuda", generator=g) for _ in range(nsets)]
    outs = [torch.empty(rows, n, dtype=torch.int8, device="cuda") for _ in range(nsets)]
    w = torch.randint(-128, 128, (n, k), dtype=torch.int8, device="cuda", generator=g)
    scale = np.array([40.0 / (74.0 * 74.0 * np.sqrt(k))], dtype=np.float32)
    res = {}
    for tag, path, bm in (("tile128", dfa.LINEAR_TILE, 128), ("tile64", dfa.LINEAR_TILE, 64), ("generic", dfa.LINEAR_GENERIC, None)):
        if path == dfa.LINEAR_GENERIC and not with_generic:
            continue
        capi.set_tuning("DFX_LINEAR_BM", bm)
        op = dfa.Linear(rows, k, n, np.int8, np.int8, force_path=path)
        capi.set_tuning("DFX_LINEAR_BM", None)
        op.set_weights(w.cpu().numpy(), scale)
        res[tag] = timed(lambda i: op.submit(srcs[i], outs[i]), nsets)
        op.close()
    wt = w.t().contiguous()                                    # {k, n}: _int_mm wants the second operand column-accessible
    if rows > 16 and k % 8 == 0 and n % 8 == 0:
        res["torch._int_mm"] = timed(lambda i: torch._int_mm(srcs[i], wt), nsets)
    halves = [s.half() for s in srcs]
    wh = wt.half()
    res["torch f16 matmul"] = timed(lambda i: torch.matmul(halves[i], wh), nsets)
    ops = 2.0 * rows * k * n
    print("%-34s %s" % (name, "; ".join("%s %.1f us (%.1f .. %.1f, %.0f TOP/s)" % (t, v[0], v[1], v[2], ops / v[0] / 1e6) for t, v in res.items())))


if __name__ == "__main__":
    assert torch.cuda.is_available()
    with_generic = "-nogeneric" not in sys.argv
    for tag, rows in (("vit-b bs8", 1576), ("vit-b bs64", 12608)):
        for k, n in ((768, 2304), (768, 768), (768, 3072), (3072, 768)):
            point("%s %d %d->%d" % (tag, rows, k, n), rows, k, n, with_generic)
    for k, n in ((96, 288), (96, 384), (384, 96)):
        point("swin s1 9408 %d->%d" % (k, n), 9408, k, n, with_generic)
    for k, n in ((256, 256), (256, 2048), (2048, 256)):
        point("detr 1700 %d->%d" % (k, n), 1700, k, n, with_generic)
