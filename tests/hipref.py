"""Helpers shared by the GPU parity tests: run a ConvCase through the C ABI
(libdfx_hip.so via deep-fusion_amd.capi) and through the CPU oracle."""
import importlib

import numpy as np

import cases as C

dfa = importlib.import_module("deep-fusion_amd")


def oracle_conv(orc, case, data, impl=None):
    if impl is None:
        impl = "avx512" if orc.have_avx512_vnni() else "scalar_mt"
    wb = orc.reorder_oihw_to_blocked(data["w0"])
    w1b = orc.reorder_oihw_to_blocked(data["w1"]) if case.oc1x1 else None
    return orc.conv(data["src"], wb, data["w0"].shape, case.stride, case.pad, case.dst_dt,
                    data["scales0"], bia0=data["bia0"], wei1_blk=w1b, oc1x1=case.oc1x1,
                    scales1=data["scales1"], bia1=data["bia1"], relu0=case.relu0,
                    relu1=case.relu1, rm0=case.rm0, rm1=case.rm1, impl=impl)


def make_conv(case, data, force_variant=-1, fuse_pool=0):
    op = dfa.Conv(data["src"].shape, data["w0"].shape, stride=case.stride, pad=case.pad, fuse_pool=fuse_pool,
                  dst_dt=case.dst_dt, oc1x1=case.oc1x1, bia0_dt=case.bia0_dt,
                  bia1_dt=case.bia1_dt if case.oc1x1 else 0, conv0_relu=case.relu0,
                  conv1_relu=case.relu1, rm0=case.rm0, rm1=case.rm1,
                  nscales0=data["scales0"].size, nscales1=data["scales1"].size,
                  force_variant=force_variant)
    wb = dfa.reorder_oihw_to_blocked(data["w0"])
    w1b = dfa.reorder_oihw_to_blocked(data["w1"]) if case.oc1x1 else None
    op.set_weights(wb, data["scales0"], bia0=data["bia0"], wei1_blk=w1b,
                   scales1=data["scales1"] if case.oc1x1 else None, bia1=data["bia1"])
    return op


def hip_conv(case, data, force_variant=-1, host_path=False):
    """-> (dst ndarray, ConvInfo).  Device-resident path unless host_path."""
    import torch
    op = make_conv(case, data, force_variant)
    info = op.info()
    if host_path:
        out = op.submit_host(data["src"])
    else:
        src = torch.from_numpy(data["src"]).cuda()
        tdt = {C.F32: torch.float32, C.S32: torch.int32, C.S8: torch.int8, C.U8: torch.uint8}[case.dst_dt]
        dst = torch.empty(op.dst_shape, dtype=tdt, device="cuda")
        dst.view(torch.uint8).fill_(0xCD)      # poison: unwritten elements must show
        op.submit(src, dst)
        torch.cuda.synchronize()
        out = dst.cpu().numpy()
    op.close()
    return out, info


_SCHED_FIELDS = ("th", "tw", "linear", "uy", "ux", "total_units", "half_from", "static_rounds", "lazy_queue", "pool",
                 "teams", "roles", "ring_waits")


def check_sched(case, s):
    """Host invariant of the unit hand-out of a resident-weight op; `s` is Conv.sched() (or a dict with the same
    fields), read between set_weights and submit.  Pure Python: needs no GPU and launches nothing.

    With units = bs * uy * ux, either there are no half units (half_from >= total_units == units), or ids
    [half_from, total_units) are half units, which only conv_mfma.cuh's kernel decodes: then the role-specialised
    kernel must not run the op, there is no fused pooling, th is even, draws are lazy, and with nh half-unit PAIRS
    half_from == units - nh, total_units == units + nh, and the halves start behind everything that is handed out
    before the first queue draw can see them: nh <= units - (static_rounds + 1) * teams.
    Raises AssertionError naming the field that is off."""
    s = s._asdict() if hasattr(s, "_asdict") else dict(s)
    missing = [f for f in _SCHED_FIELDS if f not in s]
    assert not missing, "sched: fields missing: %s" % missing
    units = case.bs * s["uy"] * s["ux"]
    tag = "%s sched %r" % (case.name, s)
    assert s["th"] >= 1 and s["tw"] >= 1 and s["uy"] >= 1 and s["ux"] >= 1 and s["teams"] >= 2, "th/tw/uy/ux/teams: " + tag
    if s["half_from"] >= s["total_units"]:
        assert s["total_units"] == units, "total_units: %d ids for %d units without halves: %s" % (
            s["total_units"], units, tag)
        return
    nh = s["total_units"] - units
    assert s["roles"] == 0, ("roles: half units (ids %d..%d of %d real units) on the role-specialised kernel, which "
                             "decodes them as whole units of images >= bs: %s" % (s["half_from"], s["total_units"] - 1, units, tag))
    assert s["pool"] == 0, "pool: half units with fused pooling: " + tag
    assert s["th"] % 2 == 0, "th: half units of an odd unit height: " + tag
    assert s["lazy_queue"] == 1, "lazy_queue: half units without lazy draws: " + tag
    assert nh > 0, "total_units: %d ids for %d units, yet half_from = %d: %s" % (s["total_units"], units, s["half_from"], tag)
    assert s["half_from"] == units - nh, "half_from: %d, want units - nh = %d - %d: %s" % (s["half_from"], units, nh, tag)
    assert s["total_units"] == units + nh, "total_units: " + tag
    assert nh <= units - (s["static_rounds"] + 1) * s["teams"], (
        "half_from: nh = %d beyond the clamp units - (static_rounds + 1) * teams = %d: %s" % (
            nh, units - (s["static_rounds"] + 1) * s["teams"], tag))


def torch_dtype(dst_dt):
    import torch
    return {C.F32: torch.float32, C.S32: torch.int32, C.S8: torch.int8, C.U8: torch.uint8}[dst_dt]


GUARD_BYTE, POISON_BYTE = 0xA5, 0xCD


def guarded_dst(op, case, sched):
    """-> (buf, dst, band): `dst` (op.dst_shape, poisoned with 0xCD) is a view into the middle of ONE allocation
    `buf` with `band` bytes of 0xA5 on each side -- band = max(1 MiB, 2 x the bytes of one unit), so that a unit
    written next to the output is a test failure (assert_guards), not a fault."""
    import torch
    esz = np.dtype(C.NP_OF[case.dst_dt]).itemsize
    unit_bytes = sched.th * sched.tw * op.dst_shape[3] * esz
    band = (max(1 << 20, 2 * unit_bytes) + 255) // 256 * 256
    nbytes = int(np.prod(op.dst_shape)) * esz
    buf = torch.empty(band + nbytes + band, dtype=torch.uint8, device="cuda")
    buf.fill_(GUARD_BYTE)
    mid = buf[band:band + nbytes]
    mid.fill_(POISON_BYTE)      # poison: unwritten elements must show
    return buf, mid.view(torch_dtype(case.dst_dt)).view(op.dst_shape), band


def assert_guards(buf, band, what=""):
    for name, part in (("before", buf[:band]), ("behind", buf[buf.numel() - band:])):
        if not bool((part == GUARD_BYTE).all()):
            hit = (part != GUARD_BYTE).nonzero().flatten()
            raise AssertionError("%s: %d bytes of the guard band %s dst were overwritten (band offsets %d..%d of %d)" % (
                what, hit.numel(), name, int(hit[0]), int(hit[-1]), band))


def assert_dev_bit_equal(got_dev, ref_np, what="", ref_dev=None):
    """device-side bit comparison with an oracle result (uploaded here, or given as ref_dev when it is used for
    several runs); a difference is reported by assert_bit_equal on the host copies"""
    import torch
    if ref_dev is None:
        ref_dev = torch.from_numpy(ref_np).cuda()
    assert tuple(got_dev.shape) == tuple(ref_np.shape), (what, tuple(got_dev.shape), ref_np.shape)
    if got_dev.dtype == torch.float32:
        same = torch.equal(got_dev.view(torch.int32), ref_dev.view(torch.int32))
    else:
        same = torch.equal(got_dev, ref_dev)
    if not same:
        assert_bit_equal(got_dev.cpu().numpy(), ref_np, what)
        raise AssertionError(what + ": device and host comparison disagree")


def hip_conv_guarded(case, data, force_variant=-1, fuse_pool=0, on_device=False):
    """like hip_conv's device path, with the scheduling invariant checked before the launch (check_sched, between
    set_weights and submit) and dst inside guard bands (guarded_dst) that must come back untouched.
    -> (dst, ConvInfo, ConvSched); dst is an ndarray, or the device tensor with on_device=True."""
    import torch
    op = make_conv(case, data, force_variant, fuse_pool=fuse_pool)
    try:
        info, sched = op.info(), op.sched()
        check_sched(case, sched)
        src = torch.from_numpy(data["src"]).cuda()
        buf, dst, band = guarded_dst(op, case, sched)
        op.submit(src, dst)
        torch.cuda.synchronize()
        assert_guards(buf, band, "%s %r" % (info.kernel_name.decode(), case))
    finally:
        op.close()
    return (dst if on_device else dst.cpu().numpy()), info, sched


def assert_bit_equal(got, ref, what=""):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    g = got.view(np.uint32) if got.dtype == np.float32 else got
    r = ref.view(np.uint32) if ref.dtype == np.float32 else ref
    if not np.array_equal(g, r):
        bad = np.argwhere(g != r)
        i = tuple(bad[0])
        spread = ["axis %d: %s" % (ax, sorted(set(int(v) for v in bad[:, ax]))[:40]) for ax in range(bad.shape[1])]
        raise AssertionError("%s: %d of %d elements differ; first at %s: got %r want %r; indices hit per axis: %s" %
                             (what, len(bad), g.size, i, got[i], ref[i], "; ".join(spread)))
