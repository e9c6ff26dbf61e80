"""The image-wide top-K (dfx_select_*, histogram path forced) against eager PyTorch on the same u8 device tensors:
max_pool2d 3x3 / 1 pad 1 + compare + topk over the flattened map for the peak points, a threshold mask + topk for the others.
torch has no max_pool2d of u8: the map is converted to f16 first (exact for 0 .. 255) and the conversion IS charged to it,
since a caller who holds a u8 heat map has to pay it.  Buffers in rotation beyond the Infinity Cache, CUDA events, median of 3
rounds of 10 calls.  Run from the repository root on an MI355X:
    python profiles/select/speed_vs_torch.py > profiles/select/speed_vs_torch.txt"""
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
dfa = importlib.import_module("deep-fusion_amd")


def timed(fn, nsets, iters=10, rounds=3):
    out = []
    for _ in range(rounds):
        for i in range(2):
            fn(i % nsets)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            fn(i % nsets)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1000.0 / iters)
    return sorted(out)[len(out) // 2]


def torch_select(src, c, k, peak, min_val):
    bs = src.shape[0]
    x = src[..., :c].to(torch.float16)
    keep = x >= min_val
    if peak:
        pooled = torch.nn.functional.max_pool2d(x.permute(0, 3, 1, 2), 3, 1, 1).permute(0, 2, 3, 1)
        keep = keep & (pooled == x)
    flat = torch.where(keep, x, torch.full_like(x, -1.0)).reshape(bs, -1)
    return torch.topk(flat, min(k, flat.shape[1]), dim=1)


def point(name, bs, h, w, c, ld, k, peak, min_val):
    nsets = max(1, min(64, (768 << 20) // (bs * h * w * ld) + 1))
    g = torch.Generator(device="cuda").manual_seed(3)
    srcs = []
    for _ in range(nsets):
        a = torch.randint(0, 256, (bs, h, w, ld), dtype=torch.int32, device="cuda", generator=g)
        b = torch.randint(0, 256, (bs, h, w, ld), dtype=torch.int32, device="cuda", generator=g)
        srcs.append(((a * b) >> 8).to(torch.uint8))     # skewed: most scores low, as bench_select's
    idx = [torch.empty(bs, k, dtype=torch.int32, device="cuda") for _ in range(nsets)]
    val = [torch.empty(bs, k, dtype=torch.uint8, device="cuda") for _ in range(nsets)]
    cnt = [torch.empty(bs, dtype=torch.int32, device="cuda") for _ in range(nsets)]
    line = "%-40s" % name
    for path, pname in ((dfa.SELECT_HIST, "hist"), (dfa.SELECT_GENERIC, "generic")):
        op = dfa.SelectTopK(bs, h, w, c, np.uint8, k, src_ld=ld, peak=dfa.SELECT_PEAK3 if peak else dfa.SELECT_ALL, min_val=min_val,
                            force_path=path)
        us = timed(lambda i: op.submit(srcs[i], idx[i], cnt[i], val[i]), nsets)
        line += " %s %.1f us" % (pname, us)
        op.close()
    theirs = timed(lambda i: torch_select(srcs[i], c, k, peak, min_val), nsets)
    print(line + ", torch %.1f us   [u8 -> f16%s, mask, topk(%d) over %d values per image]" %
          (theirs, ", max_pool2d 3x3, ==" if peak else "", k, h * w * c))


if __name__ == "__main__":
    assert torch.cuda.is_available()
    for bs in (1, 8, 32):
        point("centernet %dx128x128x80 peak3 k100" % bs, bs, 128, 128, 80, 80, 100, True, 0)
    for bs in (1, 8):
        point("retinanet %dx100x136x720 min128 k1000" % bs, bs, 100, 136, 720, 720, 1000, False, 128)
    point("rpn 1x200x304x3/16 k2000", 1, 200, 304, 3, 16, 2000, False, 0)
