"""GPU: the 64-bit offsets that include/dfx.h promises, with one operand per case reaching more than 2^31 (layout H) and more
than 2^32 bytes (layout F) behind its base.  Layouts, case tables and the reasoning are in tests/far_offsets.py; what makes
these tests unable to fault the GPU through a 32-bit slip is asserted on the CPU by tests/test_far_offsets_cpu.py.

One arena of 2^31 + 2^32 + 2^26 bytes is allocated once and never copied to the host.  Per submit: the whole arena is filled
with poison, the far operand's bytes are placed (an input), the op runs once on the forced kernel, and then
  (a) the output's valid elements equal the dense twin's reference bit for bit (a wrapped read sees poison and shows here),
  (b) the whole arena holds poison again once the far operand's places are wiped (a wrapped write shows here),
  (c) the handle reports the forced path and the expected kernel name,
  (d) the op's launch counter shows that this kernel ran, not the per-submit fallback."""
import functools
import importlib

import numpy as np
import pytest

import attn_ref as A
import bmm_ref as B
import far_offsets as F
import head_ref as H
import hipref
import linear_ref as R
import lnorm_ref as L
import patchembed_ref as P
import wsum_ref as W

pytestmark = pytest.mark.gpu
dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
SMALL = 1 << 30                  # what the module may hold besides the arena
POISON64 = int.from_bytes(bytes([hipref.POISON_BYTE]) * 8, "little", signed=True)
IDS = lambda fc: fc.ident()  # noqa: E731


@pytest.fixture(scope="module")
def arena_holder():
    """the arena in a holder, allocated once per module; the only skip of the module: too little free memory.  At the module's
    end the holder is emptied BEFORE the cache is: pytest keeps what a fixture yielded until its teardown has run, so yielding
    the tensor itself would keep the 6 GiB in torch's caching allocator for the rest of the session."""
    import torch
    assert hipref.POISON_BYTE == F.POISON
    free = torch.cuda.mem_get_info()[0]
    if free < F.ARENA + SMALL:
        pytest.skip("the far-offset arena needs %d bytes of free device memory, %d are free" % (F.ARENA + SMALL, free))
    holder = [torch.empty(F.ARENA, dtype=torch.uint8, device="cuda")]
    assert holder[0].data_ptr() % 16 == 0
    yield holder
    holder.clear()
    torch.cuda.empty_cache()


@pytest.fixture
def arena(arena_holder):
    """the arena for one test (function scope: nothing of pytest's holds the tensor when the module's teardown runs)"""
    return arena_holder[0]


@functools.lru_cache(maxsize=None)
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def on_device(a):
    """the bytes of numpy array `a` on the device, 16 spare bytes behind them -> uint8 tensor"""
    import torch
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf = torch.empty(raw.size + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[:raw.size].copy_(torch.from_numpy(raw.copy()))
    return buf[:raw.size]


def segments(arena, far):
    """The far operand's segments as views of the arena, {rows of a group, bytes} each: consecutive segments that lie one gap
    apart and within 2^24 bytes form one group, a strided view of one plain slice (the 8 pixel rows of a patchembed image),
    so that placing, gathering and wiping them is one operation per group -> list of 2-d views, in the segments' order"""
    n = far.width * far.esz
    starts = [F.BASE + far.base + int(s) for s in far.byte_starts()]
    out, i = [], 0
    while i < len(starts):
        j, gap = i + 1, (starts[i + 1] - starts[i]) if i + 1 < len(starts) else 0
        while n <= gap and j < len(starts) and starts[j] - starts[j - 1] == gap and starts[j] + n - starts[i] <= 1 << 24:
            j += 1
        whole = arena[starts[i]:starts[j - 1] + n]
        out.append(whole.as_strided((j - i, n), (gap if j - i > 1 else n, 1)))
        i = j
    return out


def put(segs, rows):
    """rows {segments, bytes} (a device tensor) into the groups of segments()"""
    at = 0
    for view in segs:
        view.copy_(rows[at:at + view.shape[0]])
        at += view.shape[0]
    assert at == rows.shape[0]


def wipe(segs):
    for view in segs:
        view.fill_(hipref.POISON_BYTE)


def assert_clean(arena, what):
    """the whole arena holds poison: one reduction on the device"""
    import torch
    lo, hi = torch.aminmax(arena.view(torch.int64))
    if int(lo) == POISON64 and int(hi) == POISON64:
        return
    step = 1 << 28
    for at in range(0, F.ARENA, step):                               # (a failure only: where)
        bad = (arena[at:at + step] != hipref.POISON_BYTE).nonzero().flatten()
        if bad.numel():
            first = at + int(bad[0]) - F.BASE
            raise AssertionError("%s: %d bytes of poison damaged in this part of the arena, the first at base %+d (0x%x)" % (what, bad.numel(), first, first & (2 ** 64 - 1)))
    raise AssertionError(what + ": poison damaged")


def place(arena, fc):
    """the far INPUT's bytes into the (poisoned) arena -> the segments' views"""
    import torch
    segs = segments(arena, F.far_of(fc))
    put(segs, torch.from_numpy(F.input_segments(fc).copy()).cuda())
    return segs


def far_submit(arena, fc, submit, what, dst_dtype):
    """One submit of case `fc` with its far operand in the arena.  submit(far, small): `far` is the far operand's device
    pointer, `small` the poisoned dense outputs of a case whose far operand is an input (empty otherwise).  Checks (a), (b)."""
    import torch
    arena.fill_(hipref.POISON_BYTE)
    bufs = []
    if fc.is_input:
        segs = place(arena, fc)
        wants = F.dense_reference(fc)
        bufs = [guarded(w.size) for w in wants]
    else:                                                            # the far output, and val behind a far idx
        second = F.far_second(fc)
        outs = [segments(arena, F.far_of(fc))] + ([segments(arena, second)] if second is not None else [])
        segs = [view for o in outs for view in o]
        wants = [np.ascontiguousarray(F.values(fc)).view(np.uint8).reshape(-1)]
        if second is not None:
            wants.append(np.ascontiguousarray(F.second_values(fc)).view(np.uint8).reshape(-1))
    torch.cuda.synchronize()
    submit(arena.data_ptr() + F.BASE, [mid for _, mid in bufs])
    torch.cuda.synchronize()
    if fc.is_input:
        for (buf, mid), w in zip(bufs, wants):
            assert bool((buf[:GUARD] == hipref.GUARD_BYTE).all()) and bool((buf[GUARD + w.size:] == hipref.GUARD_BYTE).all()), what + ": a guard band was overwritten"
        gots = [mid.cpu().numpy() for _, mid in bufs]
    else:
        gots = [torch.cat(o).cpu().numpy().reshape(-1) for o in outs]
    wipe(segs)
    assert_clean(arena, what)                                        # (b) first: a wrapped write names its place
    for i, (got, want) in enumerate(zip(gots, wants)):               # (a)
        if not np.array_equal(got, want):
            dt = np.uint32 if np.dtype(dst_dtype).itemsize == 4 and len(wants) == 1 else np.uint8
            hipref.assert_bit_equal(got.view(dt), want.view(dt), "%s output %d" % (what, i))


GUARD = 1 << 12


def guarded(nbytes):
    """-> (buf, out): a poisoned out between two GUARD-byte bands"""
    import torch
    buf = torch.empty(GUARD + nbytes + GUARD, dtype=torch.uint8, device="cuda")
    buf.fill_(hipref.GUARD_BYTE)
    mid = buf[GUARD:GUARD + nbytes]
    mid.fill_(hipref.POISON_BYTE)
    return buf, mid


def ran_only(before, after, path, what):
    """(d): the launch counters moved by one submit of `path` and nothing else"""
    assert [after[p] - before[p] for p in range(len(before))] == [int(p == path) for p in range(len(before))], what


# ---- the ops: a generator of (what, path, launches, submit) per forced kernel ------------------------------------------------------
def linear_op(fc, path):
    c = fc.case
    op = dfa.Linear(c.rows, c.k, c.n, src_dtype=R.NP_OF[c.src_dt], dst_dtype=R.NP_OF[c.dst_dt], bia_dt=c.bia_dt, relu=c.relu, rm=c.rm,
                    nscales=c.nscales, src_ld=c.sld, dst_ld=c.dld, force_path=path)
    return op


def linear_kernels(fc):
    """tile at the case's tile heights (the route the weights prove, then the exact route), then generic, as check_case of
    tests/test_gpu_linear.py does"""
    data, c = F.data_of(fc), fc.case
    d = R.desc_of(c)
    src = on_device(data["src"]) if fc.operand != "src" else None
    for path in F.PATHS["linear"]:
        for bm in (fc.bms if path == R.TILE else (None,)):
            if bm is not None:
                capi.set_tuning("DFX_LINEAR_BM", bm)
            try:
                op = linear_op(fc, path)
            finally:
                capi.set_tuning("DFX_LINEAR_BM", None)
            try:
                for no_fast, route in (((None, int(R.fast_ok(c, data))), ("1", 0)) if path == R.TILE else ((None, 0),)):
                    if no_fast:
                        capi.set_tuning("DFX_NO_FAST", no_fast)
                    try:
                        op.set_weights(data["w"], data["scales"], data["bia"])
                    finally:
                        if no_fast:
                            capi.set_tuning("DFX_NO_FAST", None)
                    info = op.info()
                    name = info.kernel_name.decode()
                    assert info.path == path and op.requant() == route, (fc.ident(), name)
                    assert name == R.kernel_name(c, path, R.planned_bm(d, cus(), bm or 0), route), (fc.ident(), name)
                    yield name, path, dfa.linear_launches, (lambda far, small: op.submit(far, small[0])) if fc.operand == "src" else \
                        (lambda far, small: op.submit(src, far))
            finally:
                op.close()


def patchembed_kernels(fc):
    """tile at both heights (the route the weights prove, then the exact route), then generic, as check_case of
    tests/test_gpu_patchembed.py does"""
    data, c = F.data_of(fc), fc.case
    d = P.desc_of(c)
    src = on_device(data["src"]) if fc.operand != "src" else None
    for path in F.PATHS["patchembed"]:
        for bm in (fc.bms if path == P.TILE else (None,)):
            if bm is not None:
                capi.set_tuning("DFX_PATCHEMBED_BM", bm)
            try:
                op = dfa.PatchEmbed((c.bs, c.ih, c.iw, c.ic), c.oc, (c.ph, c.pw), tokens_hw=(c.th, c.tw), src_dtype=P.NP_OF[c.src_dt],
                                    dst_dtype=P.NP_OF[c.dst_dt], bia_dt=c.bia_dt, relu=c.relu, rm=c.rm, nscales=c.nscales, table=c.table,
                                    tok_offset=c.t0, img_rows=c.img_rows, dst_ld=c.dld, force_path=path)
            finally:
                capi.set_tuning("DFX_PATCHEMBED_BM", None)
            try:
                for no_fast, route in (((None, int(P.fast_ok(c, data))), ("1", 0)) if path == P.TILE else ((None, 0),)):
                    if no_fast:
                        capi.set_tuning("DFX_NO_FAST", no_fast)
                    try:
                        op.set_weights(data["w"], data["scales"], data["bia"])
                        if data["prefix"] is not None:
                            op.set_prefix(data["prefix"])
                    finally:
                        if no_fast:
                            capi.set_tuning("DFX_NO_FAST", None)
                    info = op.info()
                    name = info.kernel_name.decode()
                    assert info.path == path and op.requant() == route and info.granule == c.granule, (fc.ident(), name)
                    assert name == P.kernel_name(c, path, P.planned_bm(d, cus(), bm or 0), route), (fc.ident(), name)
                    yield name, path, dfa.patchembed_launches, (lambda far, small: op.submit(far, small[0])) if fc.operand == "src" else \
                        (lambda far, small: op.submit(src, far))
            finally:
                op.close()


def bmm_op(case, path):
    return dfa.MatMul(case.batch, case.m, case.n, case.k, a_dtype=B.NP_OF[case.a_dt], dst_dtype=B.NP_OF[case.dst_dt], trans_b=case.trans_b,
                      a_strides=case.strides("a"), b_strides=case.strides("b"), c_strides=case.strides("c"), relu=case.relu, rm=case.rm,
                      nscales=case.n if case.per_channel else 1, force_path=path)


def bmm_kernels(fc):
    """MFMA (the route the shape proves, then the exact route), then generic, as check_case of tests/test_gpu_bmm.py does"""
    data, c = F.data_of(fc), fc.case
    d = B.desc_of(c)
    dense = {w: on_device(data[w]) for w in "ab" if w != fc.operand}
    for path in F.PATHS["bmm"]:
        op = bmm_op(c, path)
        try:
            for no_fast, route in (((None, int(B.fast_ok(d, data["scales"]))), ("1", 0)) if path == B.MFMA else ((None, 0),)):
                if no_fast:
                    capi.set_tuning("DFX_NO_FAST", no_fast)
                try:
                    op.set_scales(data["scales"])
                finally:
                    if no_fast:
                        capi.set_tuning("DFX_NO_FAST", None)
                info = op.info()
                name = info.kernel_name.decode()
                assert info.path == path and op.requant() == route, (fc.ident(), name)
                assert name == B.kernel_name(c, path, route), (fc.ident(), name)

                def submit(far, small):
                    ptr = dict(dense, c=small[0] if small else None)
                    ptr[fc.operand] = far
                    op.submit(ptr["a"], ptr["b"], ptr["c"])
                yield name, path, dfa.bmm_launches, submit
        finally:
            op.close()


def attn_op(case, path, data):
    op = dfa.Attention(case.batch, case.tq, case.tk, case.d, case.dv, q_dtype=A.NP_OF[case.q_dt], dst_dtype=A.NP_OF[case.dst_dt],
                       q_strides=case.strides("q"), k_strides=case.strides("k"), v_strides=case.strides("v"), o_strides=case.strides("o"),
                       relu=case.relu, rm=case.rm, nscales=case.dv if case.per_channel else 1, prob_scale=case.prob_scale, force_path=path)
    op.set_table(data["table"])
    return op


def attn_kernels(fc):
    """fused (the routes the shape proves, then both exact), then the chain, as check_case of tests/test_gpu_attn.py does"""
    data, c = F.data_of(fc), fc.case
    d = A.desc_of(c)
    dense = {w: on_device(data[w]) for w in "qkv" if w != fc.operand}
    proved = (int(A.fast_logits(d, data["logit_scale"])), int(A.fast_context(d, data["out_scales"])))
    for path in F.PATHS["attn"]:
        op = attn_op(c, path, data)
        try:
            for no_fast, routes in (((None, proved), ("1", (0, 0))) if path == A.FUSED else ((None, proved),)):
                if no_fast:
                    capi.set_tuning("DFX_NO_FAST", no_fast)
                try:
                    op.set_scales(data["logit_scale"][0], data["out_scales"])
                finally:
                    if no_fast:
                        capi.set_tuning("DFX_NO_FAST", None)
                info = op.info()
                name = info.kernel_name.decode()
                assert info.path == path and op.requant() == routes, (fc.ident(), name)
                assert name == A.kernel_name(c, path, *routes), (fc.ident(), name)

                def submit(far, small):
                    ptr = dict(dense, o=small[0] if small else None)
                    ptr[fc.operand] = far
                    op.submit(ptr["q"], ptr["k"], ptr["v"], ptr["o"])
                yield name, path, dfa.attn_launches, submit
        finally:
            op.close()


def lnorm_op(case, path, params):
    op = dfa.LayerNorm(case.rows, case.c, L.NP_OF[case.src_dt], L.NP_OF[case.dst_dt], case.eps, mode=case.mode, src_ld=case.src_ld,
                       dst_ld=case.dst_ld, force_path=path)
    op.set_params(*params)
    return op


def lnorm_kernels(fc):
    data, c = F.data_of(fc), fc.case
    src = on_device(data["src"]) if fc.operand != "src" else None
    for path in F.PATHS["lnorm"]:
        op = lnorm_op(c, path, data["params"])
        try:
            info = op.info()
            name = info.kernel_name.decode()
            assert info.path == path and name == L.kernel_name(c, path), (fc.ident(), name)
            yield name, path, dfa.lnorm_launches, (lambda far, small: op.submit(far, small[0])) if fc.operand == "src" else \
                (lambda far, small: op.submit(src, far))
        finally:
            op.close()


def head_op(fc, path):
    c = fc.case
    if c.mode == H.TOPK:
        return dfa.TopK(c.rows, c.c, H.NP_OF[c.src_dt], H.NP_OF[c.dst_dt], k=c.k, src_ld=c.ld, idx_ld=fc.pitch or c.k, force_path=path)
    return dfa.Softmax(c.rows, c.c, H.NP_OF[c.src_dt], H.NP_OF[c.dst_dt], table=H.make_table(c), src_ld=c.ld, dst_ld=c.out_ld,
                       out_scale=c.out_scale, force_path=path)


def head_kernels(fc):
    """the row and the generic kernel; a far src of a top-k leaves idx AND val in small buffers; a far idx or val has the other
    output in the arena as well wherever far_offsets.far_second() places one (its pointer: the far base + its Far.base)"""
    c = fc.case
    src = on_device(F.data_of(fc)["src"]) if fc.operand != "src" else None
    for path in F.PATHS["head"]:
        op = head_op(fc, path)
        try:
            info = op.info()
            name = info.kernel_name.decode()
            assert info.path == path and name == H.kernel_name(c, path), (fc.ident(), name)
            if fc.operand == "src":
                submit = (lambda far, small: op.submit(far, small[0], small[1])) if c.mode == H.TOPK else (lambda far, small: op.submit(far, small[0]))
            elif fc.operand in ("idx", "val"):
                second = F.far_second(fc)
                if fc.operand == "val":
                    submit = lambda far, small: op.submit(src, far + second.base, far)  # noqa: E731
                else:
                    submit = lambda far, small: op.submit(src, far, None if second is None else far + second.base)  # noqa: E731
            else:
                submit = lambda far, small: op.submit(src, far)  # noqa: E731
            yield name, path, dfa.head_launches, submit
        finally:
            op.close()


KERNELS = {"linear": linear_kernels, "patchembed": patchembed_kernels, "bmm": bmm_kernels, "attn": attn_kernels, "lnorm": lnorm_kernels, "head": head_kernels}


def dst_dtype(fc):
    t = fc.twin
    return {"linear": R.NP_OF, "patchembed": P.NP_OF, "bmm": B.NP_OF, "attn": A.NP_OF, "lnorm": L.NP_OF, "head": H.NP_OF}[fc.op][t.dst_dt]


def check_far(arena, fc):
    seen = []
    for name, path, launches, submit in KERNELS[fc.op](fc):
        what = "%s [%s]" % (fc.ident(), name)
        before = launches()
        far_submit(arena, fc, submit, what, dst_dtype(fc))
        ran_only(before, launches(), path, what)
        seen.append(path)
    assert set(seen) == set(F.PATHS[fc.op])


@pytest.mark.parametrize("fc", F.LINEAR_CASES, ids=IDS)
def test_linear(arena, fc):
    """src through src_ld, dst (u8; f32 / s32) through dst_ld, on the tile kernel at both heights and both routes and on the
    generic kernel; rows 3, and rows BM + 2 with the far rows in the second m-tile"""
    check_far(arena, fc)


@pytest.mark.parametrize("fc", F.PATCHEMBED_CASES, ids=IDS)
def test_patchembed(arena, fc):
    """dst through dst_ld and through img_rows (with and without prefix rows; s8 and f32 / s32), src through bs with images of
    2^24 bytes at granule 16 and 4, on the tile kernel at both heights and both routes and on the generic kernel"""
    check_far(arena, fc)


@pytest.mark.parametrize("fc", F.BMM_CASES, ids=IDS)
def test_bmm(arena, fc):
    """each of A, B (both forms) and C (u8, s32) far, through each of its three strides alone, on the MFMA kernel (both
    routes) and the generic kernel"""
    check_far(arena, fc)


@pytest.mark.parametrize("fc", F.ATTN_CASES, ids=IDS)
def test_attn(arena, fc):
    """each of Q, K, V and O (s8, f32) far, through each of its three strides alone, on the fused kernel (both routes) and on the
    chain of the three ops"""
    check_far(arena, fc)


@pytest.mark.parametrize("fc", F.LNORM_CASES, ids=IDS)
def test_lnorm(arena, fc):
    """src through src_ld, dst (s8; f32) through dst_ld (int32_t pitches), on the row kernel at two lane widths and the generic
    kernel"""
    check_far(arena, fc)


@pytest.mark.parametrize("fc", F.HEAD_CASES, ids=IDS)
def test_head(arena, fc):
    """src through src_ld (1-byte, and f32 with src_ld near 2^29), idx and val through idx_ld (top-1 u8, top-5 s32 / f32), the softmax's dst
    through dst_ld (u8, f32), on the row and the generic kernel; c 21 and 1000 (int32_t pitches)"""
    check_far(arena, fc)


# ---- the overlap checks at far offsets ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fc", F.OVERLAP_CASES, ids=IDS)
def test_overlap_check_at_far_offsets(arena, fc):
    """a small dst INSIDE the far input's extent, beyond 2^32 and between two of its rows, is refused with the "overlaps" error
    and launches nothing; just BEHIND the input's last valid byte it runs and is correct (the generic kernel: dst need not be
    aligned for it; attention: the chain)"""
    import torch
    inside, behind = F.overlap_places(fc)
    want, = F.dense_reference(fc)
    path = F.PATHS[fc.op][1]
    data, c = F.data_of(fc), fc.case
    if fc.op == "linear":
        op = linear_op(fc, path)
        op.set_weights(data["w"], data["scales"], data["bia"])
        launches, submit = dfa.linear_launches, lambda src, dst: op.submit(src, dst)
    elif fc.op == "bmm":
        assert fc.operand == "a"
        op = bmm_op(c, path)
        op.set_scales(data["scales"])
        b_dev = on_device(data["b"])
        launches, submit = dfa.bmm_launches, lambda src, dst: op.submit(src, b_dev, dst)
    elif fc.op == "attn":
        assert fc.operand == "q"
        op = attn_op(c, path, data)
        op.set_scales(data["logit_scale"][0], data["out_scales"])
        k_dev, v_dev = on_device(data["k"]), on_device(data["v"])
        launches, submit = dfa.attn_launches, lambda src, dst: op.submit(src, k_dev, v_dev, dst)
    else:
        op = lnorm_op(c, path, data["params"])
        launches, submit = dfa.lnorm_launches, lambda src, dst: op.submit(src, dst)
    try:
        arena.fill_(hipref.POISON_BYTE)
        segs = place(arena, fc)
        base = arena.data_ptr() + F.BASE
        torch.cuda.synchronize()
        before = launches()
        with pytest.raises(dfa.DfxError, match="dfx error 1.*overlaps"):
            submit(base, base + inside)
        torch.cuda.synchronize()
        assert launches() == before, fc.ident()
        submit(base, base + behind)
        torch.cuda.synchronize()
        ran_only(before, launches(), path, fc.ident())
        out = arena[F.BASE + behind:F.BASE + behind + want.size]
        got = out.cpu().numpy()
        out.fill_(hipref.POISON_BYTE)
        wipe(segs)
        assert_clean(arena, fc.ident())
        assert np.array_equal(got, want), fc.ident()
    finally:
        op.close()


# ---- wsum: the dense far tensor, in place ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wc", F.WSUM_CASES, ids=lambda wc: wc.ident())
def test_wsum_in_place(arena, wc):
    """bs images of 2^24 bytes at the far base, image b = image 0 rolled by b pixels, dst = the input; the expected image b is
    the expected image 0 rolled alike, compared on the device; then the tensor is wiped and the arena must be clean"""
    import torch
    case, n = wc.case, F.WSUM_IMAGE_BYTES
    def rolled(a):
        """{bs, n / 8} words of 8 bytes: row b is np.roll(a, wsum_roll(b)), a strided view of `a` laid out twice"""
        twice = torch.from_numpy(np.concatenate([a, a])).cuda().view(torch.int64)
        return twice.as_strided((wc.bs, n // 8), (-F.wsum_roll(1) // 8, 1))

    img, exp = rolled(F.wsum_image(wc)), rolled(F.wsum_expected(wc))
    last = torch.from_numpy(np.roll(F.wsum_image(wc), F.wsum_roll(wc.bs - 1))).cuda().view(torch.int64)
    assert F.wsum_roll(1) % 8 == 0 and -F.wsum_roll(wc.bs) <= n and torch.equal(img[wc.bs - 1], last)
    arena.fill_(hipref.POISON_BYTE)
    far = arena[F.BASE:F.BASE + wc.bs * n].view(torch.int64).view(wc.bs, n // 8)
    far.copy_(img)
    op = dfa.ScaledSum(case.shape, case.src_dts, case.dst_dt, case.nscales(), n_bias=case.n_bias(), post_relu=case.relu,
                       lut_in=None if case.lut_in == W.UNDEF else case.lut_in, rm=case.rm, force_path=wc.path)
    try:
        op.set_params(*W.make_params(wc.one))
        info = op.info()
        name = info.kernel_name.decode()
        want = "%s<n1:u8->u8,bias%s>" % ("wsum_vec" if wc.path == W.VEC else "wsum_generic", ",lut_u8" if wc.lut else "")
        assert info.path == wc.path and name == want, (wc.ident(), name)
        ptr = arena.data_ptr() + F.BASE
        torch.cuda.synchronize()
        before = capi.wsum_launches()
        op.submit([ptr], ptr)
        torch.cuda.synchronize()
        ran_only(before, capi.wsum_launches(), wc.path, wc.ident())
    finally:
        op.close()
    bad = [b for b in range(wc.bs) if not torch.equal(far[b], exp[b])]     # (per image: the comparison's temporary stays small)
    far.fill_(POISON64)
    assert_clean(arena, wc.ident())
    assert not bad, "%s [%s]: images %s differ from the reference" % (wc.ident(), name, bad[:16])


# ---- the head's pixel kernel: dense far src, dense far idx ----------------------------------------------------------------------------
@pytest.mark.parametrize("pc", F.PIXEL_CASES, ids=lambda pc: pc.ident())
def test_head_pixel(arena, pc):
    """argmax over 2^32 / 160 + 1000 rows; row i is row pixel_map(i) of a random block, the expected idx is expanded by the same
    map on the device.  src far (src_ld 160, idx_ld 1; idx and val small), then idx far (src_ld 16, idx_ld 160; without val, whose
    extent would overlap idx's), on the pixel kernel and, on the same data, the generic kernel"""
    import torch
    case, rows, ld = pc.case, F.PIXEL_ROWS, F.PIXEL_LD
    block, want, want_val = F.pixel_block(pc)
    block_dev, want_dev = torch.from_numpy(block.copy()).cuda(), torch.from_numpy(want.copy()).cuda()
    i = torch.arange(rows, dtype=torch.int64, device="cuda")
    m = (i + i // F.PIXEL_R0) % F.PIXEL_R0
    assert m[-5:].tolist() == F.pixel_map(np.arange(rows - 5, rows)).tolist()
    exp, exp_val = want_dev[m], torch.from_numpy(want_val.copy()).cuda()[m]
    arena.fill_(hipref.POISON_BYTE)
    far = arena[F.BASE:F.BASE + pc.far_bytes].view(rows, ld)
    if pc.operand == "src":
        far8, block8 = far.view(torch.int64), block_dev.view(torch.int64)   # (a row is 20 words of 8 bytes)
        for r0 in range(0, rows, 1 << 21):                                # (pieces: the gather's temporary stays small)
            far8[r0:r0 + (1 << 21)] = block8[m[r0:r0 + (1 << 21)]]
        src, out, val = None, torch.empty(rows, dtype=torch.uint8, device="cuda"), torch.empty(rows, dtype=torch.uint8, device="cuda")
    else:
        src, out, val = block_dev[m].contiguous(), far[:, 0], None
    del i
    ptr = arena.data_ptr() + F.BASE
    bad = []
    for path in (H.PIXEL, H.GENERIC):
        op = dfa.TopK(rows, case.c, np.uint8, np.uint8, k=1, src_ld=case.ld, idx_ld=pc.idx_ld, force_path=path)
        try:
            info = op.info()
            name = info.kernel_name.decode()
            assert info.path == path and name == H.kernel_name(case, path), (pc.ident(), name)
            out.fill_(hipref.POISON_BYTE)
            if val is not None:
                val.fill_(hipref.POISON_BYTE)
            torch.cuda.synchronize()
            before = dfa.head_launches()
            if src is None:
                op.submit(ptr, out, val)
            else:
                op.submit(src, ptr, None)
            torch.cuda.synchronize()
            ran_only(before, dfa.head_launches(), path, pc.ident())
            for which, got, want_all in (("idx", out, exp), ("val", val, exp_val)):
                if got is not None and not torch.equal(got, want_all):
                    wrong = (got != want_all).nonzero().flatten()
                    bad.append("[%s] %s: %d rows differ, the first %s" % (name, which, wrong.numel(), wrong[:8].tolist()))
        finally:
            op.close()
    if pc.operand == "src":
        far.fill_(hipref.POISON_BYTE)
    else:
        far[:, 0] = hipref.POISON_BYTE
    assert_clean(arena, pc.ident())
    assert not bad, (pc.ident(), bad)
