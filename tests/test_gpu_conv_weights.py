"""dfx_conv_set_weights as the library runs it (csrc/conv_weights.h behind one upload) against tests/golden/conv_weights.json
(tests/conv_weights_golden.py), recorded on an MI355X from the commit before the packing and the proofs left dfx_api.hip:
for the golden's "gpu" cases -- one per kernel family and route combination -- the op is created with the recorded desc under
the case's switches, given the Python-generated inputs (tests/test_conv_weights_cpu.py holds them against the tool's), and
dfx_debug_conv_requant, the queried kernel name and block must be the recorded ones.  Create and set_weights launch nothing.
The two "gpu+submit" cases -- the smallest shapes of the plan golden that the role-specialised resident kernel and the
direct-weight kernel take -- are then submitted once and compared bit for bit with the oracle: the images and constants the
kernels walk are the ones the proofs were made for."""
import importlib

import numpy as np
import pytest

import cases as C
import conv_weights_golden as G
import hipref

CASES = [c for c in G.load()["cases"] if c["tag"].startswith("gpu")]


def _make(capi, c, data):
    d = dict(zip(G.DESC_FIELDS, c["desc"]))
    op = capi.Conv((d["bs"], d["ih"], d["iw"], d["ic"]), data["w0"].shape, stride=(d["sh"], d["sw"]), pad=(d["pad_t"], d["pad_l"]),
                   dst_dt=d["dst_dt"], oc1x1=d["oc1x1"], bia0_dt=d["bia0_dt"], bia1_dt=d["bia1_dt"], conv0_relu=d["conv0_relu"],
                   conv1_relu=d["conv1_relu"], rm0=d["conv0_round_mode"], rm1=d["conv1_round_mode"], nscales0=d["conv0_nscales"],
                   nscales1=d["conv1_nscales"], force_variant=d["force_variant"], fuse_pool=d["fuse_pool"])
    assert [getattr(op.desc, k) for k in G.DESC_FIELDS] == c["desc"]
    op.set_weights(G.blocked(data["w0"]), data["scales0"], bia0=data["bia0"], wei1_blk=None if data["w1"] is None else G.blocked(data["w1"]),
                   scales1=data["scales1"], bia1=data["bia1"])
    return op, d


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_set_weights_matches_the_recording(c):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    torch.cuda.set_device(0)
    capi = importlib.import_module("deep-fusion_amd.capi")
    want = G.fields(c["line"])
    data = G.generate(c["desc"], c["recipe"])
    op = None
    try:
        for k, v in c["tuning"].items():
            capi.set_tuning(k, v)
        op, d = _make(capi, c, data)
        info = op.info()
        assert (op.requant(), info.kernel_name.decode(), info.block) == (want["routes"], want["name"], want["block"])
        if c["tag"] != "gpu+submit":
            return
        from oracle import oracle as orc
        case = C.ConvCase(c["name"], d["bs"], d["ic"], d["ih"], d["iw"], d["oc"], d["oc1x1"], k=(d["kh"], d["kw"]), stride=(d["sh"], d["sw"]),
                          pad=(d["pad_t"], d["pad_l"]), dst_dt=d["dst_dt"], bia0_dt=d["bia0_dt"], bia1_dt=d["bia1_dt"], relu0=bool(d["conv0_relu"]),
                          relu1=bool(d["conv1_relu"]), rm0=d["conv0_round_mode"], rm1=d["conv1_round_mode"])
        data["src"] = np.random.default_rng(5).integers(0, 256, (d["bs"], d["ih"], d["iw"], d["ic"])).astype(np.uint8)
        ref = hipref.oracle_conv(orc, case, data)
        assert len(np.unique(ref)) > 8, "the reference output is degenerate"
        dst = torch.empty(op.dst_shape, dtype=hipref.torch_dtype(d["dst_dt"]), device="cuda")
        dst.view(torch.uint8).fill_(hipref.POISON_BYTE)                  # poison: unwritten elements must show
        op.submit(torch.from_numpy(data["src"]).cuda(), dst)
        torch.cuda.synchronize()
        hipref.assert_bit_equal(dst.cpu().numpy(), ref, "%s %s" % (c["name"], want["name"]))
    finally:
        for k in c["tuning"]:
            capi.set_tuning(k, None)
        if op is not None:
            op.close()
