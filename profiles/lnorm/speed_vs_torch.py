"""The int8 layer norm (dfx_lnorm_*) against what a caller does today in eager PyTorch on the same device tensors:
dequantise the s8 tokens to f32, torch.nn.functional.layer_norm, quantise back to s8 (mul, round, clamp, to int8).  The
conversions ARE charged to torch: they are the round trip the op removes.  Both forced kernels of the op are timed, so the
table does not depend on the auto rule.  Buffers in rotation beyond the Infinity Cache, CUDA events, windows of at least
3 ms, median of 5 rounds.  Run from the repository root on an MI355X:
    python profiles/lnorm/speed_vs_torch.py > profiles/lnorm/speed_vs_torch.txt"""
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


def point(name, rows, c):
    nsets = max(1, min(64, (768 << 20) // (rows * c * 2) + 1))
    g = torch.Generator(device="cuda").manual_seed(3)
    srcs = [torch.randint(-128, 128, (rows, c), dtype=torch.int8, device="cuda", generator=g) for _ in range(nsets)]
    outs = [torch.empty(rows, c, dtype=torch.int8, device="cuda") for _ in range(nsets)]
    gamma = torch.randn(c, device="cuda", generator=g)
    beta = torch.randn(c, device="cuda", generator=g)
    in_scale, out_scale, eps = 0.04, 0.03, 1e-5
    gq, bq, eps_q = dfa.lnorm_params(gamma.cpu().numpy(), beta.cpu().numpy(), in_scale, out_scale, eps)
    ours = {}
    for path, tag in ((dfa.LNORM_ROW, "row"), (dfa.LNORM_GENERIC, "generic")):
        op = dfa.LayerNorm(rows, c, np.int8, np.int8, float(eps_q), force_path=path)
        op.set_params(gq, bq)
        ours[tag] = timed(lambda i: op.submit(srcs[i], outs[i]), nsets)
        op.close()

    def eager(i):
        y = torch.nn.functional.layer_norm(srcs[i].float().mul_(in_scale), (c,), gamma, beta, eps)
        return y.mul_(1.0 / out_scale).round_().clamp_(-128, 127).to(torch.int8)
    theirs = timed(eager, nsets)
    print("%-24s row %.1f us, generic %.1f us, eager torch (dequantise + F.layer_norm + quantise) %.1f us, torch / row %.2f, torch / generic %.2f" %
          (name, ours["row"], ours["generic"], theirs, theirs / ours["row"], theirs / ours["generic"]))


if __name__ == "__main__":
    assert torch.cuda.is_available()
    point("vit-b bs8 1576x768", 8 * 197, 768)
    point("vit-b bs64 12608x768", 64 * 197, 768)
    point("swin-t s1 200704x96", 64 * 3136, 96)
    point("swin-t s2 50176x192", 64 * 784, 192)
    point("swin-t s3 12544x384", 64 * 196, 384)
    point("swin-t s4 3136x768", 64 * 49, 768)
    point("detr 1700x256", 2 * 850, 256)
    point("mobilevit 16384x144", 64 * 256, 144)
    point("4096x1280", 4096, 1280)
    point("2048x4096", 2048, 4096)
    point("512x16384", 512, 16384)
