"""The batched int8 matrix product (dfx_bmm_*, dfa.MatMul on auto) against eager PyTorch on the same operands, both products
of an attention block at the points of tools/bench_bmm:
  * torch.matmul on f16 copies of the operands ({bs, heads, T, d} views of the {bs, T, heads * d} tensors; the conversions to
    f16 are NOT charged to it, and it returns f16, not requantised bytes);
  * torch._int_mm (s8 x s8 -> s32, two-dimensional only) where the point has at most 4 matrices, one call per matrix, on
    contiguous copies made outside the timed region; "n/a" with torch's own message where it refuses the shape.
Buffers in rotation beyond the Infinity Cache, CUDA events, windows of at least 3 ms, median (min .. max) of 5 rounds.  Run
from the repository root on an MI355X:
    python profiles/bmm/speed_vs_torch.py > profiles/bmm/speed_vs_torch.txt"""
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
dfa = importlib.import_module("deep-fusion_amd")


def timed(fn, nsets, rounds=5, window_us=3000.0):
    def window(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            fn(i % nsets)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / n
    for i in range(3):
        fn(i % nsets)
    n = max(20, min(20000, int(window_us / max(window(20), 0.1)) + 1))
    out = sorted(window(n) for _ in range(rounds))
    return out[len(out) // 2], out[0], out[-1], n


def fmt(t):
    return "%9.2f us (%8.2f .. %8.2f, n %5d)" % t


def up16(v):
    return -(-v // 16) * 16


def point(name, bs, heads, t, d):
    hd, lt = heads * d, up16(t)
    set_bytes = 3 * bs * t * hd + 2 * bs * heads * t * lt
    nsets = max(1, min(64, (768 << 20) // set_bytes + 1))
    g = torch.Generator(device="cuda").manual_seed(3)
    rnd = lambda *shape: torch.randint(-128, 128, shape, dtype=torch.int8, device="cuda", generator=g)  # noqa: E731
    q, k, v = ([rnd(bs, t, hd) for _ in range(nsets)] for _ in range(3))
    logits = [torch.zeros(bs, heads, t, lt, dtype=torch.int8, device="cuda") for _ in range(nsets)]
    probs = [torch.randint(0, 256, (bs, heads, t, lt), dtype=torch.uint8, device="cuda", generator=g) for _ in range(nsets)]
    ctx = [torch.zeros(bs, t, hd, dtype=torch.int8, device="cuda") for _ in range(nsets)]
    hs = dfa.attention_strides(bs, heads, t, d)
    ls = (heads * t * lt, t * lt, lt)
    sc = lambda a_std, kk: [40.0 / (a_std * 74.0 * np.sqrt(kk))]  # noqa: E731
    qk = dfa.MatMul((bs, heads), t, t, d, a_dtype=np.int8, dst_dtype=np.int8, trans_b=True, a_strides=hs, b_strides=hs, c_strides=ls,
                    scales=sc(74.0, d))
    pv = dfa.MatMul((bs, heads), t, d, t, a_dtype=np.uint8, dst_dtype=np.int8, trans_b=False, a_strides=ls, b_strides=hs, c_strides=hs,
                    scales=sc(147.0, t))
    nf = max(1, min(nsets, (3 << 30) // (2 * set_bytes)))           # f16 copies: twice the bytes
    heads_of = lambda x: x.view(bs, t, heads, d).permute(0, 2, 1, 3)  # noqa: E731
    qf, kf, vf = ([heads_of(x[i]).half() for i in range(nf)] for x in (q, k, v))
    pf = [probs[i][..., :t].half() for i in range(nf)]
    for what, op, ours, f16 in (("Q.K^T", qk, lambda i: qk.submit(q[i], k[i], logits[i]), lambda i: torch.matmul(qf[i % nf], kf[i % nf].transpose(-1, -2))),
                                ("P.V", pv, lambda i: pv.submit(probs[i], v[i], ctx[i]), lambda i: torch.matmul(pf[i % nf], vf[i % nf]))):
        a = timed(ours, nsets)
        b = timed(f16, nf)
        line = "%-20s %-6s bmm %s [%s]   torch.matmul f16 %s   f16 / bmm %.2f" % (name, what, fmt(a), op.info().kernel_name.decode(), fmt(b), b[0] / a[0])
        if bs * heads <= 4:
            try:
                if what == "Q.K^T":
                    am = [heads_of(q[0])[b0, h].contiguous() for b0 in range(bs) for h in range(heads)]
                    bm = [heads_of(k[0])[b0, h].t().contiguous() for b0 in range(bs) for h in range(heads)]
                else:
                    am = [probs[0][b0, h, :, :t].contiguous().view(torch.int8) for b0 in range(bs) for h in range(heads)]
                    bm = [heads_of(v[0])[b0, h].contiguous() for b0 in range(bs) for h in range(heads)]
                c = timed(lambda i: [torch._int_mm(x, y) for x, y in zip(am, bm)], 1)
                line += "   torch._int_mm s32 out, %d call(s) %s   _int_mm / bmm %.2f" % (len(am), fmt(c), c[0] / a[0])
            except Exception as e:  # noqa: BLE001
                line += "   torch._int_mm n/a: %s" % str(e).splitlines()[0][:120]
        print(line, flush=True)
    qk.close()
    pv.close()


if __name__ == "__main__":
    assert torch.cuda.is_available()
    print("torch %s" % torch.__version__)
    point("ViT-B bs8", 8, 12, 197, 64)
    point("ViT-B bs64", 64, 12, 197, 64)
    point("Swin 64x3 windows", 64, 3, 49, 32)
    point("DETR bs2", 2, 8, 850, 32)
    point("non-local bs1", 1, 1, 4096, 256)
    point("non-local bs4", 4, 1, 4096, 256)
