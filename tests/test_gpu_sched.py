"""GPU tests of the unit hand-out of the two resident-weight kernels (conv_mfma.cuh, conv_mfma_roles.cuh): which
workgroup computes which unit, and into which bytes -- static split, device queue, lazy draws, half units at the
tail, the 16-slot queue ring.  (Their arithmetic is tests/test_gpu_parity.py's subject.)

Every output is compared with the CPU oracle bit for bit (f32 included), is written between guard bands
(hipref.hip_conv_guarded), and every handle passes the host invariant hipref.check_sched between set_weights and
submit.  What a test needs to be true of the hand-out (lazy, halves active, which kernel, queue in use) it asserts
from Conv.sched() / kernel_name: the geometry picker is free to change, the tests then say so instead of silently
testing something else."""
import ctypes
import time
from dataclasses import replace

import numpy as np
import pytest

import cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import hipref
    return hipref


def _kernel(info):
    return info.kernel_name.decode()


def _halves(s):
    """half-unit pairs of a hand-out (0: none)"""
    return s.total_units - s.half_from >> 1 if s.half_from < s.total_units else 0


def _queue_in_use(s):
    return s.static_rounds * s.teams < s.total_units


class _Oracle:
    """oracle result of a case, on the host and (uploaded once) on the device"""

    def __init__(self, hip, oracle, case, data, pooled=False):
        import torch
        self.np = hip.oracle_conv(oracle, case, data)
        if pooled:
            self.np = oracle.maxpool(self.np, (2, 2), (2, 2), (0, 0), (self.np.shape[1] // 2, self.np.shape[2] // 2))
        self.dev = torch.from_numpy(self.np).cuda()


def _run(hip, case, data, ref, what, fuse_pool=0):
    """one guarded launch, compared with the oracle on the device -> (dst on the device, info, sched)"""
    got, info, s = hip.hip_conv_guarded(case, data, fuse_pool=fuse_pool, on_device=True)
    hip.assert_dev_bit_equal(got, ref.np, "%s %s %r" % (what, _kernel(info), case), ref.dev)
    return got, info, s


# ---- 1. role-specialised kernel x lazy queue x half-unit requests ----------------------------------------------
# 32 -> 32 -> 512 with a 1-byte output: 512 output bytes per pixel = store-bound (lazy draws), and a shape of
# the role-specialised kernel, which does not decode half-unit ids
ROLES_LAZY_VARIANTS = [dict(dst_dt=C.U8), dict(dst_dt=C.S8, relu1=True), dict(dst_dt=C.S8, relu1=False),
                       dict(dst_dt=C.U8, wide=True)]


ROLES_LAZY_IDS = ["u8", "s8-relu", "s8-norelu", "u8-wide"]


@pytest.mark.parametrize("variant", ROLES_LAZY_VARIANTS, ids=ROLES_LAZY_IDS)
def test_roles_kernel_lazy_queue_default_rule(hip, oracle, tuning, variant):
    """N = 64, 112x112: more than three rounds of units, and half of a unit still has 7 tiles, so the default
    rule asks for half units with no switch set.  The role-specialised kernel must run it with lazy draws and
    WITHOUT halves (it would take ids >= 1792 for units of images 64..73); conv_mfma.cuh's kernel
    (DFX_NO_ROLES=1) runs the same op WITH halves -- a 1-byte output with half units -- to the same bytes."""
    case = C.ConvCase("rl112", 64, 32, 112, 112, 32, 512, **variant)
    data = C.generate(case)
    ref = _Oracle(hip, oracle, case, data)
    got, info, s = _run(hip, case, data, ref, "roles x lazy")
    assert _kernel(info).startswith("conv_mfma_roles_kernel") and s.roles == 1, (info.kernel_name, s)
    assert s.lazy_queue == 1 and _queue_in_use(s) and s.total_units > 3 * s.teams, s
    assert _halves(s) == 0 and s.total_units == case.bs * s.uy * s.ux, s
    tuning.setenv("DFX_NO_ROLES", "1")
    got2, info2, s2 = _run(hip, case, data, ref, "fused kernel x lazy x halves")
    assert _kernel(info2).startswith("conv_mfma_fused_kernel") and s2.roles == 0, (info2.kernel_name, s2)
    assert s2.lazy_queue == 1 and _halves(s2) > 0, s2
    import torch
    assert torch.equal(got, got2)


ROLES_LAZY_SWITCHES = [(), (("DFX_HALF_UNITS", "77"),), (("DFX_HALF_UNITS", "1000000"),), (("DFX_NO_LAZY", "1"),),
                       (("DFX_STATIC_ROUNDS", "0"),), (("DFX_STATIC_ROUNDS", "1"),), (("DFX_STATIC_ROUNDS", "99"),),
                       (("DFX_NO_LAZY", "1"), ("DFX_STATIC_ROUNDS", "1"))]


@pytest.mark.parametrize("variant", ROLES_LAZY_VARIANTS, ids=ROLES_LAZY_IDS)
def test_roles_kernel_lazy_queue_switches(hip, oracle, tuning, variant):
    """N = 128, 56x56 in 4-row units (1792): half-unit requests of every size, eager draws, and the static split
    from none to all of it, eager draws behind one static round, on the role-specialised kernel; then the same requests on conv_mfma.cuh's kernel,
    where 77 pairs of halves must be active."""
    import torch
    case = C.ConvCase("rl56", 128, 32, 56, 56, 32, 512, **variant)
    data = C.generate(case)
    ref = _Oracle(hip, oracle, case, data)
    for switches in ROLES_LAZY_SWITCHES:
        tuning.setenv("DFX_FORCE_GEOM", "4,56")
        for k, v in switches:
            tuning.setenv(k, v)
        got, info, s = _run(hip, case, data, ref, "roles %r" % (switches,))
        tuning.undo()
        assert _kernel(info).startswith("conv_mfma_roles_kernel") and s.roles == 1, (switches, info.kernel_name, s)
        assert (s.th, s.tw, s.total_units) == (4, 56, 1792) and _halves(s) == 0, (switches, s)
        if not switches or switches[0][0] == "DFX_HALF_UNITS":
            assert s.lazy_queue == 1 and _queue_in_use(s), (switches, s)
        if switches and switches[0] == ("DFX_NO_LAZY", "1"):   # (alone: four static rounds cover the op)
            assert s.lazy_queue == 0 and _queue_in_use(s) == (len(switches) == 2), (switches, s)
        if switches == (("DFX_STATIC_ROUNDS", "99"),):
            assert not _queue_in_use(s), s
        if not switches:
            roles_run = got
    for half, want in (("77", 77), ("1000000", None)):
        tuning.setenv("DFX_FORCE_GEOM", "4,56")
        tuning.setenv("DFX_NO_ROLES", "1")
        tuning.setenv("DFX_HALF_UNITS", half)
        got, info, s = _run(hip, case, data, ref, "fused kernel, DFX_HALF_UNITS=%s" % half)
        tuning.undo()
        assert _kernel(info).startswith("conv_mfma_fused_kernel") and s.roles == 0, (info.kernel_name, s)
        clamp = 1792 - (s.static_rounds + 1) * s.teams
        assert s.lazy_queue == 1 and _halves(s) == (want if want is not None else clamp) > 0, (half, s)
        assert torch.equal(got, roles_run)


# ---- 2. half units on conv_mfma.cuh -----------------------------------------------------------------------------
# store-bound s32 / f32 ops (>= 512 output bytes per pixel), more than three rounds of units for 512 loaders
HALF_CASES = [
    # column-split units on a 96-wide image, 30 rows (30 mod 4 = 2): 32- and 64-column units (the right one partial)
    (C.ConvCase("hcol32", 72, 32, 30, 96, 32, 128, dst_dt=C.S32), "4,32", None),
    (C.ConvCase("hcol64", 72, 32, 30, 96, 32, 128, dst_dt=C.F32, relu1=False), "2,64", None),
    # oh mod th = 1, 2, 3 at th = 4 (the bottom unit's second half has 0, 0, 1 rows), padding 1 and 0
    (C.ConvCase("hrem1p1", 600, 32, 9, 16, 32, 128, dst_dt=C.S32), "4,16", None),
    (C.ConvCase("hrem2p1", 600, 32, 10, 16, 32, 128, dst_dt=C.F32), "4,16", None),
    (C.ConvCase("hrem3p1", 600, 32, 11, 16, 32, 128, dst_dt=C.S32, wide=True), "4,16", None),
    (C.ConvCase("hrem1p0", 600, 32, 11, 18, 32, 128, dst_dt=C.F32, pad=(0, 0), wide=True), "4,16", None),
    (C.ConvCase("hrem2p0", 600, 32, 12, 18, 32, 128, dst_dt=C.S32, pad=(0, 0)), "4,16", None),
    (C.ConvCase("hrem3p0", 600, 32, 13, 18, 32, 128, dst_dt=C.F32, pad=(0, 0), per_channel1=True), "4,16", None),
    # an unfused op: oc = 64 in f32 is 256 bytes per pixel, store-bound only with DFX_STORE_BOUND_BYTES=256
    (C.unfused(C.ConvCase("hunf", 450, 32, 16, 16, 64, 0, dst_dt=C.F32, relu0=False)), "4,16", "256"),
]


@pytest.mark.parametrize("case,geom,store_bound", HALF_CASES, ids=[c[0].name for c in HALF_CASES])
def test_fused_kernel_half_units(hip, oracle, tuning, case, geom, store_bound):
    """half units (the tail of a lazy queue) on conv_mfma.cuh's kernel where units are split by columns, where the
    image's rows do not fill the bottom unit, with and without padding, fused and unfused: 77 pairs, and a request
    far beyond what the clamp units - (static_rounds + 1) * teams allows."""
    data = C.generate(case)
    ref = _Oracle(hip, oracle, case, data)
    th, tw = (int(v) for v in geom.split(","))
    for half in ("77", "1000000"):
        tuning.setenv("DFX_FORCE_GEOM", geom)
        tuning.setenv("DFX_HALF_UNITS", half)
        if store_bound:
            tuning.setenv("DFX_STORE_BOUND_BYTES", store_bound)
        got, info, s = _run(hip, case, data, ref, "halves %s" % half)
        tuning.undo()
        assert _kernel(info).startswith("conv_mfma_fused_kernel"), info.kernel_name
        assert (s.th, s.tw) == (th, tw) and s.linear == (tw == case.ow), s
        assert s.lazy_queue == 1 and _queue_in_use(s), s
        units = case.bs * s.uy * s.ux
        clamp = units - (s.static_rounds + 1) * s.teams
        assert clamp > 77, (units, s)
        assert _halves(s) == (77 if half == "77" else clamp), (half, units, s)


# ---- 3. several streams on one handle ---------------------------------------------------------------------------
def test_three_streams_on_one_handle(hip, oracle, tuning):
    """The queue-ring guard with a THIRD stream.  4 launches on stream A (slots 0..3, no events: one stream so
    far), 12 on B (the first B submit covers A's launches with one event), 4 on C -- whose first launch takes slot
    0, last used on A -- then one more on A, B, C.  A is held back by a gate until everything is submitted and C
    waits for the gate too, so that A's and C's launches of one slot would be in flight together if C did not wait
    for A's: two launches sharing one {next unit, finished loaders} pair skip units or do them twice.

    Deterministic part: ring_waits (stream waits the guard has issued) must grow by one across the first submit on
    C, and by one for each of C's next three (slots 1..3).  Before the slots of the single-stream phase kept their
    event the counter stayed flat there: 1 (the second stream's wait) after all 20 launches -- read from the code
    of that version, where the transition reset those slots to "never used"."""
    import torch
    tuning.setenv("DFX_STATIC_ROUNDS", "0")
    case = replace(C.CONFIG3_SMALL, name="ring3", bs=16)     # res2a, s32
    data = C.generate(case)
    op = hip.make_conv(case, data)
    tuning.undo()
    try:
        s0 = op.sched()
        hip.check_sched(case, s0)
        assert s0.static_rounds * s0.teams < s0.total_units and s0.static_rounds == 0, s0   # every unit is a queue draw
        assert s0.ring_waits == 0
        rng = np.random.default_rng(13)
        srcs_np = [rng.integers(0, 256, data["src"].shape).astype(np.uint8) for _ in range(5)]
        refs = [_Oracle(hip, oracle, case, dict(data, src=sn)) for sn in srcs_np]
        srcs = [torch.from_numpy(sn).cuda() for sn in srcs_np]
        A, B, Cs = (torch.cuda.Stream() for _ in range(3))
        order = [A] * 4 + [B] * 12 + [Cs] * 4 + [A, B, Cs]
        bufs = [hip.guarded_dst(op, case, s0) for _ in order]
        torch.cuda.synchronize()
        # the gate: a spin kernel on A, its length calibrated here.  Submitting the 23 launches took 5.4 ms when
        # measured (with the sched() queries around every submit; the test prints the figure); 4 x margin = 22 ms,
        # the gate is GATE_MS = 50 ms.
        GATE_MS, cal = 50.0, 2000000
        ms = 0.0
        for _ in range(2):   # (the first call also loads the spin kernel)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(A)
            with torch.cuda.stream(A):
                torch.cuda._sleep(cal)
            e1.record(A)
            e1.synchronize()
            ms = e0.elapsed_time(e1)
        assert ms > 0.0
        with torch.cuda.stream(A):
            torch.cuda._sleep(int(cal / ms * GATE_MS))
        gate = torch.cuda.Event()
        gate.record(A)
        Cs.wait_event(gate)
        waits = []
        t0 = time.perf_counter()
        for k, st in enumerate(order):
            before = op.sched().ring_waits
            op.submit(srcs[k % 5], bufs[k][1], stream=st)
            waits.append(op.sched().ring_waits - before)
        t_submit = time.perf_counter() - t0
        still_closed = not gate.query()
        print("three streams: %d launches submitted in %.2f ms behind a gate of %.0f ms (spin %d cycles = %.2f ms)"
              % (len(order), 1e3 * t_submit, GATE_MS, cal, ms))
        torch.cuda.synchronize()
        assert still_closed, ("gate too short: %.2f ms of submitting against a gate of %.0f ms -- the launches "
                              "were not held back together" % (1e3 * t_submit, GATE_MS))
        # A x 4: one stream, no waits.  First B: the event on A.  Rest of B: fresh slots.  C x 4: slots 0..3, last
        # used on A.  Then A on slot 4 (last B), B on slot 5 (its own), C on slot 6 (last B).
        assert waits == [0] * 4 + [1] + [0] * 11 + [1] * 4 + [1, 0, 1], waits
        for k, (buf, dst, band) in enumerate(bufs):
            what = "three streams, launch %d (stream %s)" % (k, "ABC"[[A, B, Cs].index(order[k])])
            hip.assert_guards(buf, band, what)
            hip.assert_dev_bit_equal(dst, refs[k % 5].np, what, refs[k % 5].dev)
    finally:
        op.close()


def test_second_stream_after_the_first_was_destroyed(hip, oracle):
    """two streams of the C ABI's own; the first is synchronised and DESTROYED (dfx_stream_destroy) before the
    second one submits: no event can be recorded on it any more -- handing the destroyed stream to hipEventRecord
    crashed the process, which is how this test was first met -- so the library, which keeps track of the streams
    it made, falls back to a device synchronisation and issues no wait."""
    import torch
    L = hip.dfa.lib()
    case = replace(C.CONFIG3_SMALL, name="ring2", bs=5, dst_dt=C.U8)
    data = C.generate(case)
    ref = _Oracle(hip, oracle, case, data)
    op = hip.make_conv(case, data)
    s1, s2 = ctypes.c_void_p(), ctypes.c_void_p()
    try:
        s0 = op.sched()
        hip.check_sched(case, s0)
        src = torch.from_numpy(data["src"]).cuda()
        bufs = [hip.guarded_dst(op, case, s0) for _ in range(7)]
        torch.cuda.synchronize()
        assert L.dfx_stream_create(ctypes.byref(s1)) == 0 and L.dfx_stream_create(ctypes.byref(s2)) == 0
        assert s1.value != s2.value      # (both alive at once: the second cannot reuse the first one's handle)
        for k in range(3):
            op.submit(src, bufs[k][1], stream=s1.value)
        assert L.dfx_stream_sync(s1) == 0 and L.dfx_stream_destroy(s1) == 0
        s1 = ctypes.c_void_p()
        for k in range(3, 6):
            op.submit(src, bufs[k][1], stream=s2.value)
        assert L.dfx_stream_sync(s2) == 0
        assert op.sched().ring_waits == 0
        third = torch.cuda.Stream()      # a third stream on slot 6, never used: no wait either
        op.submit(src, bufs[6][1], stream=third)
        torch.cuda.synchronize()
        assert op.sched().ring_waits == 0
        for k, (buf, dst, band) in enumerate(bufs):
            hip.assert_guards(buf, band, "launch %d" % k)
            hip.assert_dev_bit_equal(dst, ref.np, "first stream destroyed, launch %d" % k, ref.dev)
    finally:
        op.close()
        for s in (s1, s2):
            if s.value:
                L.dfx_stream_destroy(s)


# ---- 4. full-size res2a on the role-specialised kernel ----------------------------------------------------------
_RES2A = C.ConvCase("res2a", 128, 64, 56, 56, 64, 256, dst_dt=C.U8)
RES2A_CASES = [
    ("u8", _RES2A, None),
    ("s8-relu", replace(_RES2A, dst_dt=C.S8, relu1=True), None),
    ("s8-norelu", replace(_RES2A, dst_dt=C.S8, relu1=False), None),
    ("u8-wide", replace(_RES2A, wide=True), None),
    ("u8-per-channel", replace(_RES2A, per_channel0=True, per_channel1=True), None),
    ("u8-scale1.37", _RES2A, 1.37),        # a conv1 scale that is no power of two
]

def test_full_size_res2a_on_roles_kernel(hip, oracle):
    """N = 128, 56x56, 64 -> 64 -> 256 with a 1-byte output -- the op the role-specialised kernel was written for
    -- at full size: complete comparison with the oracle, and images [40, 56) alone give the same bytes.  Over the
    set, both stage-1 requant routes of the kernel ("/fma": one v_fma_f32, power-of-two scales; "/magic") occur."""
    routes = set()
    for name, case, scale1 in RES2A_CASES:
        data = C.generate(case)
        if scale1:
            data["scales1"] = data["scales1"] * np.float32(scale1)
        ref = _Oracle(hip, oracle, case, data)
        got, info, s = _run(hip, case, data, ref, "res2a " + name)
        assert _kernel(info).startswith("conv_mfma_roles_kernel") and s.roles == 1, (name, info.kernel_name, s)
        routes.add(_kernel(info).rsplit("/", 1)[1])
        sub = dict(data, src=data["src"][40:56])
        got_sub, info_sub, _ = hip.hip_conv_guarded(replace(case, bs=16), sub, on_device=True)
        assert _kernel(info_sub) == _kernel(info), (name, info_sub.kernel_name)
        hip.assert_dev_bit_equal(got_sub, ref.np[40:56], "res2a %s, batch shard" % name, got[40:56])
    assert routes == {"fma", "magic"}, routes


# ---- 5. seeded scheduling soak ----------------------------------------------------------------------------------
SOAK_SEED, SOAK_N = 7, 90
_MB = 1 << 20


def soak_cases(n=SOAK_N, seed=SOAK_SEED):
    """-> [(ConvCase, switches dict, fuse_pool)]: random shapes inside the resident kernels' domain (3x3, stride 1,
    padding 0 / 1 per axis, 32 / 64 channels, fused with oc1x1 a multiple of 32 up to 512 or unfused, every dst
    type, every option flag), three in five of them with more than two rounds of units for 512 loaders (two in five
    with more than three), each with a random draw of the scheduling switches."""
    rng = np.random.default_rng(seed)
    pick = lambda seq: seq[int(rng.integers(0, len(seq)))]  # noqa: E731
    out = []
    while len(out) < n:
        i = len(out)
        kind = ("unfused", "roles", "fused", "roles", "fused")[i % 5]
        big = int(rng.integers(0, 5)) >= 2
        ph, pw = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        ih, iw = int(rng.integers(4, 41)), int(rng.integers(4, 97))
        oh, ow = ih + 2 * ph - 2, iw + 2 * pw - 2
        ic, oc = pick((32, 64)), pick((32, 64))
        flags = dict(bia0_dt=pick((C.UNDEF, C.S8, C.U8, C.S32, C.F32)), bia1_dt=pick((C.UNDEF, C.S8, C.U8, C.S32, C.F32)),
                     relu0=bool(rng.integers(0, 2)), relu1=bool(rng.integers(0, 2)),
                     rm0=int(rng.integers(0, 2)), rm1=int(rng.integers(0, 2)),
                     per_channel0=bool(rng.integers(0, 2)), per_channel1=bool(rng.integers(0, 2)),
                     wide=bool(rng.integers(0, 2)))
        if kind == "unfused":
            oc1, dst_dt = 0, pick((C.U8, C.S8, C.S32, C.F32))
        elif kind == "roles":     # a shape of the role-specialised kernel (which takes round-to-nearest only)
            oc1, dst_dt = 128 * int(rng.integers(1, 3 if oc == 64 else 5)), pick((C.U8, C.S8))
            flags.update(rm0=0, rm1=0)
        else:
            oc1, dst_dt = 32 * int(rng.integers(1, 17)), pick((C.U8, C.S8, C.S32, C.S32, C.F32, C.F32))
        # unit geometry: (th, tw) valid for the shape -- tw the whole row or a 32-multiple below it
        th = min(oh, pick((1, 2, 2, 2, 4, 4) if big else (1, 2, 3, 4, 4)))
        tw = pick(([ow] if ow <= 72 else []) + 2 * [t for t in (32, 64) if t < ow])
        force = bool(rng.integers(0, 8 if big else 3))
        upi = -(-oh // th) * -(-ow // tw)
        units = int(rng.integers(1700, 2700)) if rng.integers(0, 4) else int(rng.integers(1100, 1500))
        bs = -(-units // upi) if big else int(rng.integers(1, 9))
        px_bytes = (oc1 if oc1 else oc) * np.dtype(C.NP_OF[dst_dt]).itemsize
        while bs > 1 and bs * oh * ow * px_bytes > 256 * _MB:
            bs = bs * 3 // 4
        sw = {}
        if force:
            sw["DFX_FORCE_GEOM"] = "%d,%d" % (th, tw)
        sw["DFX_STATIC_ROUNDS"] = pick((None, None, None, "0", "1", "2", "99"))
        sw["DFX_HALF_UNITS"] = pick((None, "0", "77", "77", "300", "300", "1000000", "1000000"))
        sw["DFX_NO_LAZY"] = pick((None,) * 9 + ("1",))
        sw["DFX_STORE_BOUND_BYTES"] = pick((None, "1", "1", "256"))   # 1 / 256: 1-byte and unfused ops are lazy too
        pool = 2 if kind == "unfused" and oh % 2 == 0 and ow % 2 == 0 and int(rng.integers(0, 6)) == 0 else 0
        case = C.ConvCase("soak%d" % i, bs, ic, ih, iw, oc, oc1, pad=(ph, pw), dst_dt=dst_dt, seed=7000 + i, **flags)
        out.append((case, {k: v for k, v in sw.items() if v is not None}, pool))
    return out


SOAK_FLOORS = dict(cases=60, fused_kernel=15, roles_kernel=15, unfused_kernel=15, lazy=20, halves=10, roles_lazy=5,
                   queue_colsplit=8)


def soak_tally(tally, info, s):
    """counts what a case exercised, from what the library says it will run"""
    name = info.kernel_name.decode()
    tally["cases"] += 1
    tally["roles_kernel"] += name.startswith("conv_mfma_roles_kernel")
    tally["unfused_kernel"] += name.startswith("conv_mfma_fused_kernel") and name.endswith(",unfused>")
    tally["fused_kernel"] += name.startswith("conv_mfma_fused_kernel") and not name.endswith(",unfused>")
    lazy = s.lazy_queue == 1 and _queue_in_use(s)
    tally["lazy"] += lazy
    tally["halves"] += _halves(s) > 0 and _queue_in_use(s)
    tally["roles_lazy"] += lazy and s.roles == 1
    tally["queue_colsplit"] += _queue_in_use(s) and s.linear == 0


def test_scheduling_soak(hip, oracle, tuning):
    """seeded soak of the unit hand-out: soak_cases(), every output against the oracle (fused pooling: oracle conv
    -> oracle 2x2 max pool).  The floors keep a later change of the geometry picker from hollowing it out."""
    tally = dict.fromkeys(SOAK_FLOORS, 0)
    for case, sw, pool in soak_cases():
        what = "soak %r switches %r fuse_pool %d" % (case, sw, pool)
        data = C.generate(case)
        ref = _Oracle(hip, oracle, case, data, pooled=bool(pool))
        for k, v in sw.items():
            tuning.setenv(k, v)
        try:
            got, info, s = _run(hip, case, data, ref, what, fuse_pool=pool)
        except hip.dfa.DfxError as e:
            raise AssertionError("%s: %s" % (what, e))
        finally:
            tuning.undo()
        assert info.variant in (hip.dfa.VARIANT_MFMA_FUSED, hip.dfa.VARIANT_MFMA_CONV), (what, info.kernel_name)
        soak_tally(tally, info, s)
    print("scheduling soak:", tally)
    low = {k: (tally[k], SOAK_FLOORS[k]) for k in SOAK_FLOORS if tally[k] < SOAK_FLOORS[k]}
    assert not low, "the soak no longer exercises (count, floor): %r of %r" % (low, tally)
