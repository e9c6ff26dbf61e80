"""GPU: the int8 patch-embedding op (dfx_patchembed_*, dfa.PatchEmbed) against the numpy reference of tests/patchembed_ref.py,
bit for bit (tests/test_patchembed_cpu.py pins that reference against an element-by-element witness and against linear_ref), and
against the ops the library already has: dfx_imgconv (dfa.ImageConv with window == stride) and dfx_linear (dfa.Linear on the patch
matrix gathered on the host).  Everything goes through the C ABI.  dst's whole storage {bs * img_rows, dst_ld} sits between guard
bands and is poisoned: the comparison of the whole storage shows that the pad elements, the rows behind the tokens and, without
a prefix, the rows in front of them are not written, and that the prefix rows are stored verbatim.  The leftover pixels of src
hold 0xFF and the bytes behind it are poisoned.  The tile kernel is forced at both tile heights, on the fast and on the exact
route, then the generic kernel is forced: all against the one reference."""
import functools
import importlib
import threading

import numpy as np
import pytest

import hipref
import linear_ref as L
import lnorm_ref as LN
import patchembed_ref as R

pytestmark = pytest.mark.gpu
dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
GUARD = 1 << 12       # guard bytes on each side of dst
BEHIND = 1 << 12      # poisoned bytes behind src


@pytest.fixture(autouse=True)
def tuning():
    """no switch of one test reaches the next"""
    keys = []

    class T:
        def setenv(self, k, v):
            keys.append(k)
            capi.set_tuning(k, v)
    yield T()
    for k in keys:
        capi.set_tuning(k, None)


@functools.lru_cache(maxsize=None)
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def src_on_device(data, offset=0):
    """the image on the device, `offset` bytes off a 16-byte boundary, poison behind it -> uint8 tensor"""
    import torch
    raw = np.ascontiguousarray(data["src"]).view(np.uint8).reshape(-1)
    buf = torch.empty(offset + raw.size + BEHIND, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf.fill_(hipref.POISON_BYTE)
    view = buf[offset:offset + raw.size]
    view.copy_(torch.from_numpy(raw.copy()))
    return view


def guarded(nbytes, offset=0):
    """-> (buf, out): out (poisoned, `offset` bytes off a 16-byte boundary) between two GUARD-byte bands"""
    import torch
    buf = torch.empty(GUARD + offset + nbytes + GUARD, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf.fill_(hipref.GUARD_BYTE)
    mid = buf[GUARD + offset:GUARD + offset + nbytes]
    mid.fill_(hipref.POISON_BYTE)
    return buf, mid


def assert_guards(buf, offset, nbytes, what):
    lo, hi = buf[:GUARD + offset], buf[GUARD + offset + nbytes:]
    assert bool((lo == hipref.GUARD_BYTE).all()) and bool((hi == hipref.GUARD_BYTE).all()), what + ": a guard band was overwritten"


def make_op(case, force_path, data=None):
    op = dfa.PatchEmbed((case.bs, case.ih, case.iw, case.ic), case.oc, (case.ph, case.pw), tokens_hw=(case.th, case.tw), src_dtype=R.NP_OF[case.src_dt],
                        dst_dtype=R.NP_OF[case.dst_dt], bia_dt=case.bia_dt, relu=case.relu, rm=case.rm, nscales=case.nscales, table=case.table,
                        tok_offset=case.t0, img_rows=case.img_rows, dst_ld=case.dld, force_path=force_path)
    if data is not None:
        set_all(op, data)
    return op


def set_all(op, data):
    op.set_weights(data["w"], data["scales"], data["bia"])
    if data["table"] is not None:
        op.set_table(data["table"])
    if data["prefix"] is not None:
        op.set_prefix(data["prefix"])


def dst_bytes(case):
    return R.dst_storage(case) * R.SIZE_OF[case.dst_dt]


def run(op, case, src_dev, dst_offset=0, stream=None):
    """one submit into a guarded, poisoned dst -> dst's whole storage as bytes"""
    import torch
    n = dst_bytes(case)
    buf, dst = guarded(n, dst_offset)
    torch.cuda.synchronize()
    op.submit(src_dev, dst, stream=stream)
    torch.cuda.synchronize()
    assert_guards(buf, dst_offset, n, case.ident())
    return dst.cpu().numpy()


def same(got, want, case, what):
    """whole-storage comparison, reported per element of dst's dtype; NaNs by place and payload (the bits)"""
    if not np.array_equal(got, want):
        dt = {R.F32: np.uint32}.get(case.dst_dt, R.NP_OF[case.dst_dt])
        hipref.assert_bit_equal(got.view(dt), want.view(dt), "%s %s" % (case.ident(), what))


def check_case(case, data, paths=(R.TILE, R.GENERIC), bms=R.BMS, grid_cap=0, want=None):
    """the case on the forced tile kernel at every tile height in `bms` (the route the weights and the table prove, then the exact
    route) and on the forced generic kernel; path, route, kernel name, grid, block, LDS, granule and the algorithmic counts from
    the handle.  A case outside the tile class runs on the generic kernel only, and the forced tile path is refused."""
    want = R.reference(case, data) if want is None else want
    src_dev = src_on_device(data)
    d = R.desc_of(case)
    outs = []
    for path in paths:
        if path == R.TILE and not case.granule:
            with pytest.raises(dfa.DfxError, match="dfx error 2"):
                make_op(case, R.TILE)
            continue
        for bm in (bms if path == R.TILE else (None,)):
            if bm is not None:
                capi.set_tuning("DFX_PATCHEMBED_BM", bm)
            try:
                op = make_op(case, path)
            finally:
                capi.set_tuning("DFX_PATCHEMBED_BM", None)
            try:
                routes = ((None, int(R.fast_ok(case, data))), ("1", 0)) if path == R.TILE else ((None, 0),)
                for no_fast, route in routes:
                    if no_fast:
                        capi.set_tuning("DFX_NO_FAST", no_fast)
                    try:
                        set_all(op, data)
                    finally:
                        if no_fast:
                            capi.set_tuning("DFX_NO_FAST", None)
                    info = op.info()
                    what = "[%s]" % info.kernel_name.decode()
                    pbm = R.planned_bm(d, cus(), bm or 0)
                    assert info.path == path and op.requant() == route, (case.ident(), what, op.requant(), route)
                    assert info.kernel_name.decode() == R.kernel_name(case, path, pbm, route), (case.ident(), what)
                    assert info.grid == R.planned_grid(d, path, pbm, cus(), grid_cap) and info.block == 256, (case.ident(), what, info.grid)
                    assert info.lds_bytes == R.lds_bytes(path, pbm) and info.granule == case.granule, (case.ident(), what)
                    assert info.algorithmic_ops == R.algorithmic_ops(d), (case.ident(), what)
                    assert info.algorithmic_bytes == R.algorithmic_bytes(d, data["prefix"] is not None), (case.ident(), what)
                    before = dfa.patchembed_launches()
                    got = run(op, case, src_dev)
                    after = dfa.patchembed_launches()
                    assert [after[p] - before[p] for p in range(2)] == [int(p == path) for p in range(2)], (case.ident(), what)
                    same(got, want, case, what)
                    outs.append(got)
            finally:
                op.close()
    return outs


# ---- 1. the pairwise cover ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src_dt", [R.U8, R.S8], ids=["u8", "s8"])
@pytest.mark.parametrize("bm", R.BMS)
@pytest.mark.parametrize("part", range(4))
def test_pairwise_cover_on_the_tile_kernel(bm, src_dt, part):
    """tokens in all in 1, BM-1, BM, BM+1, 2BM+2 (bs 1, 2, 3) x oc in 1, 3, 4, 127, 128, 129, 264 x seven patch geometries as a
    pairwise cover (patchembed_ref.shape_grid), on the forced tile kernel of height BM, fast and exact route; dst dtypes, dst
    pitches, ReLU, round modes, per-channel scales, tok_offset, img_rows slack, table / bias / none and prefix rotating"""
    for case in R.shape_grid(bm, src_dt)[part::4]:
        check_case(case, R.generate(case), paths=(R.TILE,), bms=(bm,))


@pytest.mark.parametrize("src_dt", [R.U8, R.S8], ids=["u8", "s8"])
@pytest.mark.parametrize("part", range(2))
def test_pairwise_cover_on_the_generic_kernel(src_dt, part):
    """the same cover (the one of BM = 64) on the forced generic kernel"""
    for case in R.shape_grid(64, src_dt)[part::2]:
        check_case(case, R.generate(case), paths=(R.GENERIC,))


# ---- 2. compensation at depth -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [R.KMAX, 65024])
def test_compensation(k):
    """u8 tokens of all 255 and all 0 against weight rows of all -128 and all 127 at K = 65025 (255 x 255 x 1: outside the tile
    class, the generic kernel) and K = 65024 (127 x 128 x 4: the deepest K of the tile class); s32 dst and scale 1"""
    seen = 0
    for case, data in R.compensation_cases():
        if case.k != k:
            continue
        assert R.accumulate(case, data).tolist() == [[255 * -128 * k, 255 * 127 * k], [0, 0]]
        vals = R.values(case, data)
        assert abs(int(vals[0, 0, 0])) > 2 ** 30 and abs(int(vals[0, 0, 1])) > 2 ** 30
        outs = check_case(case, data)
        assert len(outs) == (1 if k == R.KMAX else 5)
        seen += 1
    assert seen == 1


# ---- 3. leftover pixels, the lane map -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.leftover_cases(), ids=lambda c: c.ident())
def test_leftover_pixels_are_never_read(case):
    """th, tw below the floor of ih / ph, iw / pw: the pixels beyond them hold 0xFF and the result is the reference's, which never
    saw them"""
    data = R.generate(case)
    assert case.ih // case.ph > case.th or case.iw // case.pw > case.tw or case.extra_h or case.extra_w
    check_case(case, data)


@pytest.mark.parametrize("bm", R.BMS)
def test_lane_map(bm):
    """s32 out, scale 1, weights and pixels with a distinct residue per (o, k): a swapped (ky, kx, i) order or a shifted run shows
    in every element.  Both granules."""
    for case, data in R.lane_map_cases(bm):
        vals = R.values(case, data)
        assert len(np.unique(vals)) > vals.size // 4
        check_case(case, data, bms=(bm,))


# ---- 4. the defining twins ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.imgconv_twin_cases(), ids=lambda c: c.ident())
def test_equals_image_conv(case):
    """no table, no prefix, t0 = 0, dst_ld = oc, u8 src, ic <= 4: dfa.ImageConv with k = s and pad 0 gives the same bytes"""
    import torch
    data = R.generate(case)
    got = check_case(case, data)[0]
    ic = dfa.ImageConv((case.bs, case.ih, case.iw, case.ic), case.oc, (case.ph, case.pw), stride=(case.ph, case.pw), pad=(0, 0), dst_dt=case.dst_dt,
                       bia_dt=case.bia_dt, relu=case.relu, rm=case.rm, nscales=case.nscales)
    try:
        assert ic.dst_shape == (case.bs, case.th, case.tw, case.oc)
        ic.set_weights(data["w"], data["scales"], data["bia"])
        buf, dst = guarded(dst_bytes(case))
        ic.submit(src_on_device(data), dst)
        torch.cuda.synchronize()
        same(dst.cpu().numpy(), got, case, "against " + ic.info().kernel_name.decode())
    finally:
        ic.close()


@pytest.mark.parametrize("case", R.linear_twin_cases(), ids=lambda c: c.ident())
def test_equals_linear_on_the_gathered_patches(case):
    """any ic and either dtype: dfa.Linear (generic path) on the patch matrix gathered on the host, with the weights in the
    op's K order, gives the same bytes into the same pitched dst"""
    import torch
    data = R.generate(case)
    got = check_case(case, data)[0]
    lin = dfa.Linear(case.rows, case.k, case.oc, src_dtype=R.NP_OF[case.src_dt], dst_dtype=R.NP_OF[case.dst_dt], bia_dt=case.bia_dt, relu=case.relu,
                     rm=case.rm, nscales=case.nscales, src_ld=case.k, dst_ld=case.dld, force_path=dfa.LINEAR_GENERIC)
    try:
        lin.set_weights(R.permute_weights(case, data["w"]), data["scales"], data["bia"])
        mat = torch.from_numpy(R.gather(case, data).view(np.uint8).reshape(-1).copy()).cuda()
        buf, dst = guarded(dst_bytes(case))
        lin.submit(mat, dst)
        torch.cuda.synchronize()
        same(dst.cpu().numpy(), got, case, "against " + lin.info().kernel_name.decode())
    finally:
        lin.close()


# ---- 5. the table -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.table_cases(), ids=lambda c: c.ident())
def test_table_of_every_dst_dtype(case):
    check_case(case, R.generate(case))


def test_one_row_repeated_equals_a_vector_bias():
    """a table whose rows all hold the same values gives the bytes of the same values as an f32 bias vector, on every path"""
    for base in R.table_cases()[:2]:
        data = dict(R.generate(base))
        row = data["table"][3].copy()
        data["table"] = np.tile(row, (base.tokens, 1))
        tabled = check_case(base, data)
        vec = R.with_case(base, table=False, bia_dt=R.F32)
        vdata = dict(data, table=None, bia=row)
        biased = check_case(vec, vdata)
        assert len(tabled) == len(biased) == 5
        for a, b in zip(tabled, biased):
            assert np.array_equal(a, b), base.ident()


@pytest.mark.parametrize("case", R.tie_cases(), ids=lambda c: c.ident())
def test_ties_at_scale_one_half(case):
    """small integers and a table of small integers: every odd sum is a tie; nearest-even and floor differ there, and both routes
    must agree with the reference"""
    data = R.generate(case)
    s = R.accumulate(case, data).reshape(case.bs, case.tokens, case.oc) + data["table"].astype(np.int64)
    assert (s % 2 != 0).mean() > 0.25
    check_case(case, data)


@pytest.mark.parametrize("case", R.nonfinite_cases(), ids=lambda c: c.ident())
def test_nonfinite_scales_take_the_exact_route(case):
    """a scale of inf or NaN is never called fast; the exact route gives the x86 0x80000000 pattern and its saturations"""
    data = R.generate(case)
    assert not R.fast_ok(case, data)
    check_case(case, data)


def test_nonfinite_table_entries_are_refused():
    case = R.ORDER_CASE
    data = R.generate(case)
    op = make_op(case, R.GENERIC)
    try:
        for bad in (np.inf, -np.inf, np.nan):
            t = data["table"].copy()
            t[case.tokens - 1, case.oc - 1] = bad
            with pytest.raises(dfa.DfxError, match="dfx error 1.*non-finite"):
                op.set_table(t)
    finally:
        op.close()


def test_set_table_before_and_after_set_weights_and_the_route_is_proved_again():
    """either order gives the same bytes and the same route; a table that breaks the fast route's bound turns the route exact,
    and the small table turns it fast again; new weights prove it again, too"""
    case = R.ORDER_CASE
    data = R.generate(case)
    want = R.reference(case, data)
    assert R.fast_ok(case, data)
    huge = dict(data, table=(data["table"] + np.float32(2.0 ** 31 / data["scales"].min())).astype(np.float32))
    assert not R.fast_ok(case, huge)
    src_dev = src_on_device(data)
    for bm in R.BMS:
        capi.set_tuning("DFX_PATCHEMBED_BM", bm)
        try:
            a, b = make_op(case, R.TILE), make_op(case, R.TILE)
        finally:
            capi.set_tuning("DFX_PATCHEMBED_BM", None)
        try:
            a.set_weights(data["w"], data["scales"])
            assert a.requant() == 1                                                       # no table yet: proved as if it were 0
            a.set_table(data["table"])
            b.set_table(data["table"])
            b.set_weights(data["w"], data["scales"])
            assert a.requant() == b.requant() == 1 and a.info().kernel_name == b.info().kernel_name
            ga, gb = run(a, case, src_dev), run(b, case, src_dev)
            same(ga, want, case, "weights first")
            same(gb, want, case, "table first")
            a.set_table(huge["table"])
            assert a.requant() == 0 and b" exact" in a.info().kernel_name
            same(run(a, case, src_dev), R.reference(case, huge), case, "huge table, exact")
            a.set_table(data["table"])
            assert a.requant() == 1
            same(run(a, case, src_dev), want, case, "small table again")
            inf = dict(data, scales=np.full_like(data["scales"], np.inf))
            a.set_weights(inf["w"], inf["scales"])
            assert a.requant() == 0
            a.set_weights(data["w"], data["scales"])
            assert a.requant() == 1
            same(run(a, case, src_dev), want, case, "weights again")
        finally:
            a.close()
            b.close()


# ---- 6. the prefix ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.prefix_cases(), ids=lambda c: c.ident())
def test_prefix_rows(case):
    """given: stored verbatim into rows 0 .. t0-1 of every image, nothing else of those rows written (the whole-storage
    comparison with poison around them); not given: the rows keep their poison"""
    data = R.generate(case)
    want = R.reference(case, data)
    rows = want.view(R.NP_OF[case.dst_dt]).reshape(case.bs, case.img_rows, case.dld)[:, :case.t0]
    if case.prefix:
        assert all(np.array_equal(rows[b, :, :case.oc].view(np.uint8), data["prefix"].view(np.uint8)) for b in range(case.bs))
        assert (rows[:, :, case.oc:].view(np.uint8) == hipref.POISON_BYTE).all()
    else:
        assert (rows.view(np.uint8) == hipref.POISON_BYTE).all()
    check_case(case, data)


def test_prefix_errors_and_a_prefix_set_later():
    import torch
    case = R.prefix_cases()[0]
    data = R.generate(case)
    op = make_op(case, R.GENERIC)
    none = make_op(R.with_case(case, t0=0, prefix=False), R.GENERIC)
    try:
        with pytest.raises(dfa.DfxError, match="dfx error 1.*tok_offset"):
            capi._check(capi.lib().dfx_patchembed_set_prefix(none._h, capi._p(data["prefix"])))
        op.set_weights(data["w"], data["scales"], data["bia"])
        if data["table"] is not None:
            op.set_table(data["table"])
        src_dev = src_on_device(data)
        same(run(op, case, src_dev), R.reference(case, dict(data, prefix=None)), case, "no prefix yet")
        op.set_prefix(data["prefix"])
        same(run(op, case, src_dev), R.reference(case, data), case, "prefix set")
        torch.cuda.synchronize()
    finally:
        op.close()
        none.close()


# ---- 7. DFX_PATCHEMBED_GRID ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [1, 3])
def test_grid_cap(cap, tuning):
    """DFX_PATCHEMBED_GRID = 1 and 3 on 12 tiles of 64 x 128: workgroups loop over several tiles, across n-blocks, and the
    prefix rows are still written once"""
    case = R.GRID_CAP_CASE
    assert R.tiles(R.desc_of(case), 64) == 12
    tuning.setenv("DFX_PATCHEMBED_GRID", cap)
    check_case(case, R.generate(case), grid_cap=cap)


# ---- 8. the per-submit fallback, state and submit errors ----------------------------------------------------------------------
def test_misaligned_src_falls_back_per_submit():
    """a src that is not aligned to the class's granule takes the generic kernel for that submit (dfx_debug_patchembed_launches);
    a G = 4 class keeps the tile kernel on a src 4 bytes off; a dst that is only element-aligned keeps the tile kernel, which
    then stores element by element; the bytes are the same"""
    for case in R.MISALIGNED_CASES:
        data = R.generate(case)
        want = R.reference(case, data)
        g = case.granule
        assert g in (4, 16)
        op = make_op(case, R.TILE, data)
        try:
            es = R.SIZE_OF[case.dst_dt]
            for src_off, dst_off in ((0, 0), (4, 0), (0, es), (1, 3 * es), (16, 0), (2, 0)):
                ran = R.TILE if src_off % g == 0 else R.GENERIC
                src_dev = src_on_device(data, src_off)
                before = dfa.patchembed_launches()
                got = run(op, case, src_dev, dst_offset=dst_off)
                after = dfa.patchembed_launches()
                assert [after[p] - before[p] for p in range(2)] == [int(p == ran) for p in range(2)], (case.ident(), src_off, dst_off)
                assert op.info().path == R.TILE
                same(got, want, case, "offsets %d, %d" % (src_off, dst_off))
        finally:
            op.close()


def test_state_and_submit_errors_launch_nothing():
    import torch
    case, tcase = R.ERROR_CASES
    data, tdata = R.generate(case), R.generate(tcase)
    src_dev = src_on_device(data)
    buf, dst = guarded(max(dst_bytes(case), dst_bytes(tcase)))
    before = dfa.patchembed_launches()
    op, top = make_op(case, R.TILE), make_op(tcase, R.TILE)
    try:
        for h in (op, top):
            with pytest.raises(dfa.DfxError, match="dfx error 5"):
                h.submit(src_dev, dst)                                    # before set_weights
            with pytest.raises(dfa.DfxError, match="dfx error 5"):
                h.requant()
        top.set_weights(tdata["w"], tdata["scales"])
        with pytest.raises(dfa.DfxError, match="dfx error 5.*set_table"):
            top.submit(src_dev, dst)                                      # a table handle before set_table
        with pytest.raises(dfa.DfxError, match="dfx error 1"):
            op.set_table(np.zeros((case.tokens, case.oc), dtype=np.float32))   # a handle created without a table
        with pytest.raises(dfa.DfxError, match="dfx error 1.*ld below"):
            capi._check(capi.lib().dfx_patchembed_set_table(top._h, capi._p(tdata["table"]), tcase.oc - 1))
        op.set_weights(data["w"], data["scales"], data["bia"])
        with pytest.raises(dfa.DfxError, match="dfx error 1.*aligned"):
            op.submit(src_dev, buf[GUARD + 2:])                           # an f32 dst off its element
        with pytest.raises(dfa.DfxError, match="dfx error 1.*overlaps"):
            op.submit(src_dev, src_dev[16:])
        with pytest.raises(dfa.DfxError, match="dfx error 1.*null"):
            op.submit(0, dst)
        torch.cuda.synchronize()
        assert dfa.patchembed_launches() == before
        assert bool((dst == hipref.POISON_BYTE).all())
    finally:
        op.close()
        top.close()


def test_submit_host():
    """dfx_patchembed_submit_host: densely packed host tensors in and out, synchronous, on both paths"""
    case = R.HOST_CASE
    data = R.generate(case)
    for path in (R.TILE, R.GENERIC):
        op = make_op(case, path, data)
        try:
            before = dfa.patchembed_launches()
            got = op.submit_host(data["src"])
            after = dfa.patchembed_launches()
            assert [after[p] - before[p] for p in range(2)] == [int(p == path) for p in range(2)]
            assert got.dtype == np.int32 and got.shape == (case.bs * case.img_rows, case.dld)
            assert np.array_equal(got.reshape(case.bs, case.tokens, case.oc), R.values(case, data)), path
        finally:
            op.close()


# ---- 9. one handle, two threads, two streams ----------------------------------------------------------------------------------
def test_one_handle_from_two_threads_on_two_streams():
    import torch
    case = R.THREADS_CASE
    data = R.generate(case)
    want = R.reference(case, data)
    for path in (R.TILE, R.GENERIC):
        op = make_op(case, path, data)
        src_dev = src_on_device(data)
        outs, errs = {}, []

        def work(i):
            try:
                st = torch.cuda.Stream()
                res = []
                for _ in range(8):
                    buf, dst = guarded(dst_bytes(case))
                    st.wait_stream(torch.cuda.current_stream())
                    op.submit(src_dev, dst, stream=st)
                    res.append((buf, dst))
                st.synchronize()
                outs[i] = res
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        try:
            torch.cuda.synchronize()
            ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
            for t in ts:
                t.start()
            for t in ts:
                t.join()
            assert not errs, errs
            for i in range(2):
                for buf, dst in outs[i]:
                    assert_guards(buf, 0, dst_bytes(case), case.ident())
                    same(dst.cpu().numpy(), want, case, "thread %d" % i)
        finally:
            op.close()


# ---- 10. auto -----------------------------------------------------------------------------------------------------------------
def test_auto_rule():
    """the AUTO RULE of include/dfx.h (DFX_PATCHEMBED_AUTO_NOTE), mirrored by patchembed_ref.auto_path: on both sides of each
    bound -- rows, oc, K, the multiply-adds and the class; the forced paths are honoured inside the class and the forced tile
    path is refused outside it.  One image of `rows` patches of 1 x 4 x ic (K = 4 ic) reaches every size."""
    want = {(12544, 12, 96): R.TILE, (12544, 12, 95): R.GENERIC,                          # oc
            (12544, 8, 96): R.GENERIC,                                                    # K 32
            (49, 768, 768): R.TILE, (48, 768, 768): R.GENERIC,                            # rows
            (3136, 12, 96): R.TILE, (3135, 12, 96): R.GENERIC,                            # 3136 * 96 * 48 multiply-adds
            (12544, 13, 768): R.TILE,                                                     # K 52: granule 4
            (1, 4, 8): R.GENERIC, (128, 3, 64): R.GENERIC}
    cases = [(R.PeCase("auto", 1, 1, rows, 1, 4, ic, oc, table=True), path) for (rows, ic, oc), path in want.items()]
    cases += [(R.PeCase("auto", 8, 14, 14, 16, 16, 3, 768, table=True), R.TILE), (R.PeCase("auto", 64, 14, 14, 16, 16, 3, 768), R.TILE),
              (R.PeCase("auto", 8, 16, 16, 14, 14, 3, 768, table=True), R.GENERIC),        # ViT /14 on RGB: outside the class
              (R.PeCase("auto", 64, 28, 28, 2, 2, 96, 192, src_dt=R.S8), R.TILE), (R.FRONT_CASE, R.GENERIC), (R.AUTO_POINT_CASE, R.TILE)]
    for case, path in cases:
        d = R.desc_of(case)
        bm = R.planned_bm(d, cus())
        op = make_op(case, -1)
        try:
            info = op.info()
            assert info.path == R.auto_path(d) == path and info.lds_bytes == R.lds_bytes(path, bm) and info.granule == case.granule, (d, info.path)
            assert info.kernel_name.decode() == R.kernel_name(case, path, bm, 0).replace(" exact", " (no weights)")
            assert info.grid == R.planned_grid(d, path, bm, cus())
        finally:
            op.close()
        if case.granule:
            op = make_op(case, R.TILE)
            try:
                assert op.info().path == R.TILE
            finally:
                op.close()
        else:
            with pytest.raises(dfa.DfxError, match="dfx error 2"):
                make_op(case, R.TILE)
        op = make_op(case, R.GENERIC)
        try:
            assert op.info().path == R.GENERIC
        finally:
            op.close()


def test_auto_takes_the_tile_kernel_at_a_measured_point_and_gives_the_reference():
    """the smallest measured point (the Swin-T stem at bs 1: 224 x 224 x 3, 4 x 4 patches, oc 96) on auto: the tile kernel runs
    and the bytes are the reference's"""
    case = R.AUTO_POINT_CASE
    data = R.generate(case)
    op = make_op(case, -1, data)
    try:
        assert op.info().path == R.TILE and op.info().granule == 4
        before = dfa.patchembed_launches()
        got = run(op, case, src_on_device(data))
        after = dfa.patchembed_launches()
        assert (after[R.TILE] - before[R.TILE], after[R.GENERIC] - before[R.GENERIC]) == (1, 0)
        same(got, R.reference(case, data), case, "auto")
    finally:
        op.close()


# ---- 11. a front end on the device --------------------------------------------------------------------------------------------
_FRONT = []


def front():
    """bs 2, 32 x 32 x 3, 4 x 4 patches, oc 64, class token: the chained numpy references of PatchEmbed -> LayerNorm -> Linear,
    computed once and shared by the three runs; left unchanged"""
    if not _FRONT:
        case = R.FRONT_CASE
        data = dict(R.generate(case))
        rng = np.random.default_rng(777)
        pos = rng.standard_normal((case.tokens + 1, case.oc)) * 0.3                      # real-valued position embedding
        step = 0.02                                                                        # the tokens' quantisation step
        data["scales"] = L.make_scales(R.lin_case(case))
        acc_step = step / float(data["scales"][0])                                         # accumulator units -> real values
        data["table"] = dfa.patch_embed_table(rng.standard_normal(case.oc) * 0.1, pos[1:], acc_step)
        data["prefix"] = dfa.patch_embed_prefix(rng.standard_normal((1, case.oc)) * 0.5, pos[:1], step, np.int8)
        tokens = R.reference(case, data).view(np.int8).reshape(case.bs * case.img_rows, case.oc)
        gamma, beta = (30.0 + 4.0 * rng.standard_normal(case.oc)).astype(np.float32), (3.0 * rng.standard_normal(case.oc)).astype(np.float32)
        normed = LN.convert(LN.reference_values(tokens, case.oc, gamma, beta, None, 0.5, LN.LAYER), LN.S8)
        n = 96
        w = rng.integers(-128, 128, (n, case.oc)).astype(np.int8)
        sd = 30.0 * 74.0 * np.sqrt(case.oc)
        lin = dict(w=w, bia=np.rint(rng.standard_normal(n) * sd / 4).astype(np.int32), scales=np.array([40.0 / sd], dtype=np.float32), lut=None)
        lcase = L.LinCase("front", tokens.shape[0], case.oc, n, src_dt=L.S8, dst_dt=L.S8, bia_dt=L.S32, src_ld=case.oc)
        out = L.values(lcase, dict(lin, src=np.ascontiguousarray(normed).reshape(-1)))
        for name, v in (("tokens", tokens), ("normed", normed), ("out", out)):             # no stage is degenerate
            v = v.astype(np.int64)
            assert v.std() > 4 and len(np.unique(v)) > 20 and ((v == -128) | (v == 127)).mean() < 0.1, name
        _FRONT.append((case, data, dict(tokens=tokens, normed=normed, out=out), (gamma, beta), lin, n))
    return _FRONT[0]


@pytest.mark.parametrize("path", [dfa.PATCHEMBED_AUTO, dfa.PATCHEMBED_TILE, dfa.PATCHEMBED_GENERIC], ids=["auto", "tile", "generic"])
def test_front_end_on_the_device(path):
    """PatchEmbed (position table, class-token prefix) -> LayerNorm -> Linear with no tensor leaving the device in between; every
    tensor against the chained numpy references"""
    import torch
    case, data, ref, (gamma, beta), lin, n = front()
    rows = case.bs * case.img_rows
    dev = {k: torch.full((rows * (n if k == "out" else case.oc),), -51, dtype=torch.int8, device="cuda") for k in ("tokens", "normed", "out")}
    pe = make_op(case, path, data)
    ln = dfa.LayerNorm(rows, case.oc, np.int8, np.int8, 0.5)
    ln.set_params(gamma, beta)
    fc = dfa.Linear(rows, case.oc, n, np.int8, np.int8, bia_dt=dfa.DFX_S32)
    fc.set_weights(lin["w"], lin["scales"], lin["bia"])
    try:
        want_path = dfa.PATCHEMBED_GENERIC if path == dfa.PATCHEMBED_AUTO else path
        assert pe.info().path == want_path
        before = dfa.patchembed_launches()
        pe.submit(src_on_device(data), dev["tokens"])
        ln.submit(dev["tokens"], dev["normed"])
        fc.submit(dev["normed"], dev["out"])
        torch.cuda.synchronize()
        after = dfa.patchembed_launches()
        assert [after[p] - before[p] for p in range(2)] == [int(p == want_path) for p in range(2)]
        for k in ("tokens", "normed", "out"):
            got = dev[k].cpu().numpy().reshape(ref[k].shape)
            assert np.array_equal(got, ref[k]), "%s differs in %d of %d elements" % (k, int((got != ref[k]).sum()), got.size)
    finally:
        pe.close()
        ln.close()
        fc.close()
