"""The net head (dfx_head_*) against eager PyTorch on the same device tensors: torch.argmax(dim=-1) on the u8 logits and
torch.softmax(dim=-1) on f32 logits (torch has no softmax of u8; the conversion is NOT charged to it).  Buffers in rotation
beyond the Infinity Cache, CUDA events, median of 3 rounds of 20 calls.  Run from the repository root on an MI355X:
    python profiles/head/speed_vs_torch.py > profiles/head/speed_vs_torch.txt"""
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
dfa = importlib.import_module("deep-fusion_amd")


def timed(fn, nsets, iters=20, rounds=3):
    out = []
    for _ in range(rounds):
        for i in range(3):
            fn(i % nsets)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            fn(i % nsets)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1000.0 / iters)
    return sorted(out)[len(out) // 2]


def point(name, rows, c, ld, mode):
    nsets = max(1, min(64, (768 << 20) // (rows * ld) + 1))
    g = torch.Generator(device="cuda").manual_seed(3)
    srcs = [torch.randint(0, 256, (rows, ld), dtype=torch.uint8, device="cuda", generator=g) for _ in range(nsets)]
    if mode == "argmax":
        op = dfa.TopK(rows, c, np.uint8, np.uint8, k=1, src_ld=ld)
        outs = [torch.empty(rows, dtype=torch.uint8, device="cuda") for _ in range(nsets)]
        ours = timed(lambda i: op.submit(srcs[i], outs[i]), nsets)
        theirs = timed(lambda i: torch.argmax(srcs[i][:, :c], dim=-1), nsets)
        what = "torch.argmax(u8 [:, :%d], dim=-1) -> int64" % c
    else:
        op = dfa.Softmax(rows, c, np.uint8, np.uint8, table=dfa.softmax_table(0.0625, c), src_ld=ld)
        outs = [torch.empty(rows, c, dtype=torch.uint8, device="cuda") for _ in range(nsets)]
        ours = timed(lambda i: op.submit(srcs[i], outs[i]), nsets)
        nf = max(1, min(nsets, (2 << 30) // (rows * c * 4)))
        fsrcs = [srcs[i][:, :c].float().mul_(0.0625).contiguous() for i in range(nf)]
        theirs = timed(lambda i: torch.softmax(fsrcs[i % nf], dim=-1), nf)
        what = "torch.softmax(f32 contiguous {rows, %d}, dim=-1) -> f32, conversions not charged" % c
    print("%-28s %s: head %.1f us (%s), torch %.1f us, torch / head %.2f   [%s]" %
          (name, mode, ours, op.info().kernel_name.decode(), theirs, theirs / ours, what))
    op.close()


if __name__ == "__main__":
    assert torch.cuda.is_available()
    for mode in ("argmax", "softmax"):
        point("16x129x129x21/32", 16 * 129 * 129, 21, 32, mode)
        point("4x513x513x21/32", 4 * 513 * 513, 21, 32, mode)
        point("8x512x1024x19/32", 8 * 512 * 1024, 19, 32, mode)
        point("8x128x128x150/160", 8 * 128 * 128, 150, 160, mode)
