"""CPU: the tests of the far-offset tests (tests/far_offsets.py).  Every case's layout reaches where it claims, no 32-bit slip
of any touched byte offset can leave the arena (the no-fault invariant of tests/test_gpu_far_offsets.py), every descriptor
passes the Python mirror of validate in the forced kernel's class, a wrapped read changes the result in every far row, and no
case is degenerate."""
import numpy as np
import pytest

import far_offsets as F
import head_ref as H
import wsum_ref as W

IDS = lambda fc: fc.ident()  # noqa: E731


def test_the_arena_and_the_aliases():
    assert F.ARENA == 2 ** 31 + 2 ** 32 + 2 ** 26 and F.BASE == 2 ** 31 and F.ARENA % 8 == 0
    off = np.array([0, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 2 ** 26 - 1])
    true, trunc, signed = F.aliases(off)
    assert true.tolist() == off.tolist()
    assert trunc.tolist() == [0, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 0, 2 ** 26 - 1]
    assert signed.tolist() == [0, 2 ** 31 - 1, -2 ** 31, -1, 0, 2 ** 26 - 1]
    for steps in (2, 65, 129):
        for layout, lo in (("H", 2 ** 31), ("F", 2 ** 32)):
            p = F.pitch_for(layout, steps)
            assert p % 64 == 0 and (steps - 1) * p + 4096 < lo <= steps * p < lo + 2 ** 20


def test_the_tables_cover_what_the_docstring_lists():
    ids = [fc.ident() for fc in F.ALL_CASES]
    assert len(set(ids)) == len(ids)
    for op, operands in (("linear", ("src", "dst")), ("patchembed", ("src", "dst")), ("bmm", ("a", "b", "c")), ("attn", ("q", "k", "v", "o")), ("lnorm", ("src", "dst")), ("head", ("src", "idx", "dst"))):
        for operand in operands:
            for layout in "HF":
                hit = [fc for fc in F.ALL_CASES if (fc.op, fc.operand, fc.layout) == (op, operand, layout)]
                assert hit, (op, operand, layout)
                if not hit[0].is_input or op == "head":              # outputs, and the head's src: 1-byte and 4-byte elements
                    assert {F.far_of(fc).esz for fc in hit} == {1, 4}, (op, operand, layout)
    for layout in "HF":
        names = {fc.name.split("-")[0] for fc in F.LINEAR_CASES if fc.layout == layout}
        assert names == {"rows3", "tile64", "tile128"}
        for operand in "abc":
            carriers = {fc.name.split("-")[0] for fc in F.BMM_CASES if fc.layout == layout and fc.operand == operand}
            assert carriers == {"s0", "s1", "ld"}
        assert {fc.twin.trans_b for fc in F.BMM_CASES if fc.layout == layout and fc.operand == "b"} == {True, False}
        assert {fc.twin.c for fc in F.LNORM_CASES if fc.layout == layout} == {40, 300}
        pe = [fc for fc in F.PATCHEMBED_CASES if fc.layout == layout]
        assert {fc.twin.granule for fc in pe if fc.operand == "src"} == {16, 4} and {fc.twin.prefix for fc in pe if fc.operand == "dst"} == {False, True}
        assert {fc.twin.bs for fc in pe if fc.operand == "src"} == {130 if layout == "H" else 258}
        assert {(fc.twin.c, fc.twin.k) for fc in F.HEAD_CASES if fc.layout == layout and fc.operand == "idx"} == {(21, 1), (1000, 5)}
        assert {fc.twin.c for fc in F.HEAD_CASES if fc.layout == layout and fc.operand == "dst"} == {21, 1000}
        for operand in "qkvo":
            carriers = {fc.name.split("-")[0] for fc in F.ATTN_CASES if fc.layout == layout and fc.operand == operand}
            assert carriers == {"s0", "s1", "ld"}
    assert [fc.op for fc in F.OVERLAP_CASES] == ["linear", "bmm", "attn", "lnorm"]


@pytest.mark.parametrize("fc", F.ALL_CASES, ids=IDS)
def test_layout_reaches_its_window_and_no_alias_leaves_the_arena(fc):
    far = F.far_of(fc)
    starts = far.byte_starts()
    assert len(starts) >= 2 and len(set(starts.tolist())) == len(starts)
    assert F.in_window(fc.layout, int(starts.max())), (fc.ident(), int(starts.max()))
    assert int(starts.argmax()) == len(starts) - 1                  # the last row / matrix is the far one
    if fc.layout == "H":
        assert starts.max() < 2 ** 32
    off = far.byte_offsets()
    assert 0 <= off.min() < 4096 and off.max() < 2 ** 32 + 2 ** 26   # (unwritten rows in front of a patchembed image: tok_offset)
    for alias in F.aliases(off):                                     # the no-fault invariant
        at = F.BASE + alias
        assert at.min() >= 0 and at.max() < F.ARENA, fc.ident()
    if far.esz == 4:                                                 # the element index fits 32 bits: the byte offset is under test
        assert max(far.starts) + far.width < 2 ** 31
    # segments do not overlap, and a slip moves every far segment off every true one (so that it meets poison) or onto other data
    true = set(off.reshape(-1).tolist())
    assert len(true) == off.size
    for seg in far.far_segments():
        wrong = [alias for alias in F.aliases(off[seg])[1:] if not np.array_equal(alias, off[seg])]
        assert wrong, (fc.ident(), seg)                              # (H: the signed one; F: both)
        for alias in wrong:
            if not true & set(alias.tolist()):
                continue                                                 # the slip meets poison
            # patchembed's images of exactly 2^24 bytes: image 256 + i wraps onto image i.  An input only, and the bytes there differ
            assert fc.is_input and fc.op == "patchembed", (fc.ident(), seg)
            held = dict(zip(off.reshape(-1).tolist(), F.input_segments(fc).reshape(-1).tolist()))
            there = np.array([held.get(a, F.POISON) for a in alias.tolist()], dtype=np.uint8)
            assert (there != F.input_segments(fc)[seg]).any(), (fc.ident(), seg)   # (that the RESULT changes: the test below)
    assert len(far.far_segments()) >= 1


SECOND = [fc for fc in F.ALL_CASES if F.far_second(fc) is not None]


def test_val_is_far_wherever_the_arena_and_the_overlap_rule_allow():
    """idx + val both beyond 2^31 at 1 and 4 bytes (H); an f32 val beyond 2^32 (F); idx beyond 2^32 runs without val"""
    assert {(fc.operand, fc.layout, fc.twin.k, F.far_of(fc).esz, F.far_second(fc).esz) for fc in SECOND} == \
        {("idx", "H", 1, 1, 1), ("idx", "H", 5, 4, 4), ("val", "F", 5, 4, 1)}
    assert [fc for fc in F.HEAD_CASES if fc.operand == "idx" and fc.layout == "F" and F.far_second(fc) is None]


@pytest.mark.parametrize("fc", SECOND, ids=IDS)
def test_second_operand_in_the_arena(fc):
    """idx and val of a top-k in one arena: the extents do not overlap (dfx_head_submit would refuse them), each reaches what
    far_second() says, every alias of either operand, taken from that operand's own pointer, stays in the arena, and no alias
    of a far row of either meets a true byte of either"""
    first, second = F.far_of(fc), F.far_second(fc)
    assert second.starts == first.starts and second.width == first.width == fc.twin.k and second.base % 16 == 0
    ext = [(f.base, f.base + int(f.byte_starts().max()) + f.width * f.esz) for f in (first, second)]
    assert ext[0][1] <= ext[1][0] or ext[1][1] <= ext[0][0], (fc.ident(), ext)
    if fc.operand == "idx":                                              # val is far as well: its last row beyond 2^31 of ITS pointer
        assert F.in_window("H", int(second.byte_starts().max())) and second.base + second.arena_offsets().max() < 2 ** 33
    else:                                                                # idx within the arena's first 2^31 bytes: no slip can move it
        assert second.base == -F.BASE and second.byte_offsets().max() < 2 ** 31 and len(second.far_segments()) == 0
    vals = F.second_values(fc)
    assert vals.shape == (len(second.starts), second.width) and vals.dtype.itemsize == second.esz and len(np.unique(vals.view(np.uint8))) > 1
    true = set(first.arena_offsets().reshape(-1).tolist()) | set(second.arena_offsets().reshape(-1).tolist())
    assert len(true) == first.byte_offsets().size + second.byte_offsets().size
    for far in (first, second):
        off = far.byte_offsets()
        assert -F.BASE <= far.arena_offsets().min() and far.arena_offsets().max() < 2 ** 32 + 2 ** 26
        for alias in F.aliases(off):
            at = F.BASE + far.base + alias
            assert at.min() >= 0 and at.max() < F.ARENA, fc.ident()
        if far.esz == 4:
            assert max(far.starts) + far.width < 2 ** 31
        for seg in far.far_segments():
            wrong = [alias for alias in F.aliases(off[seg])[1:] if not np.array_equal(alias, off[seg])]
            assert wrong, (fc.ident(), seg)
            for alias in wrong:
                assert not true & set((far.base + alias).tolist()), (fc.ident(), seg)


@pytest.mark.parametrize("fc", F.ALL_CASES, ids=IDS)
def test_descriptor_is_valid_and_in_the_forced_kernels_class(fc):
    for path in F.PATHS[fc.op]:
        assert F.descriptor_ok(fc, path), (fc.ident(), path)
    # the twin differs from the far case in the far operand's pitch / stride alone
    far, twin = F.far_of(fc), fc.twin
    if fc.op in ("bmm", "attn"):
        assert [fc.case.strides(w) == twin.strides(w) for w in ("abc" if fc.op == "bmm" else "qkvo")].count(False) == 1
        assert sum(a != b for a, b in zip(fc.case.strides(fc.operand), twin.strides(fc.operand))) == 1
    elif fc.op == "patchembed":
        assert (fc.case.ih != twin.ih, fc.case.img_rows * fc.case.dld != twin.img_rows * twin.dld) == (fc.operand == "src", fc.operand == "dst")
        assert fc.case.granule == twin.granule
    elif fc.op == "head":
        assert (fc.case.ld != twin.ld, fc.case.out_ld != twin.out_ld, fc.pitch != 0) == (fc.operand == "src", fc.operand == "dst", fc.operand in ("idx", "val"))
    elif fc.op == "linear":
        assert (fc.case.sld != twin.sld, fc.case.dld != twin.dld) == (fc.operand == "src", fc.operand == "dst")
    else:
        assert (fc.case.src_ld != twin.src_ld, fc.case.dst_ld != twin.dst_ld) == (fc.operand == "src", fc.operand == "dst")
    assert far.width * far.esz <= 4096


@pytest.mark.parametrize("fc", [fc for fc in F.ALL_CASES if fc.is_input], ids=IDS)
def test_a_wrapped_read_changes_the_result_in_every_far_row(fc):
    vals, bad = F.values(fc), F.poisoned_values(fc)
    assert vals.shape == bad.shape
    far = F.far_of(fc)
    for seg in far.far_segments():
        assert not np.array_equal(F.affected(fc, seg, vals), F.affected(fc, seg, bad)), (fc.ident(), seg)
    near = np.setdiff1d(np.arange(len(far.starts)), far.far_segments())
    if fc.op not in ("bmm", "attn", "patchembed") or fc.operand in ("a", "q"):
        assert np.array_equal(vals[near], bad[near])


@pytest.mark.parametrize("fc", F.ALL_CASES, ids=IDS)
def test_no_case_is_degenerate(fc):
    vals = F.values(fc)
    out = F.far_of(fc) if not fc.is_input else None
    if out is not None:
        assert vals.shape == (len(out.starts), out.width), fc.ident()
    distinct = len(np.unique(np.ascontiguousarray(vals).view({1: np.uint8, 4: np.uint32, 8: np.uint64}[vals.dtype.itemsize])))
    assert distinct > (8 if vals.size >= 64 and fc.op != "head" else 1), fc.ident()      # (a top-1 of 3 rows has 3 values at most)
    assert F.saturated_fraction(fc, vals) < 0.10, (fc.ident(), F.saturated_fraction(fc, vals))
    for row in vals:                                                  # every row has something to get wrong
        assert len(np.unique(row)) > 1 or row.size == 1, fc.ident()
    if fc.is_input:
        seg = F.input_segments(fc)
        assert (seg != F.POISON).mean() > 0.9


@pytest.mark.parametrize("fc", F.OVERLAP_CASES, ids=IDS)
def test_overlap_places(fc):
    """`inside` lies in the far input's extent beyond 2^32 and touches no byte of it; `behind` starts where the extent ends;
    dst at either place, and its aliases, stay in the arena"""
    far = F.far_of(fc)
    nbytes = F.dense_reference(fc)[0].size
    inside, behind = F.overlap_places(fc)
    touched = far.byte_offsets()
    extent_end = int(far.byte_starts().max()) + F.valid_width(fc)
    assert 2 ** 32 < inside and inside + nbytes < extent_end and behind == extent_end
    for at in (inside, behind):
        span = np.arange(at, at + nbytes, dtype=np.int64)
        for alias in F.aliases(span):
            assert 0 <= F.BASE + alias.min() and F.BASE + alias.max() < F.ARENA
    span = set(range(inside, inside + nbytes))
    assert not span & set(touched.reshape(-1).tolist())


# ---- the dense far tensor of wsum ------------------------------------------------------------------------------------------------
WIDS = lambda wc: wc.ident()  # noqa: E731


def test_wsum_cases_cover_both_layouts_and_kernels():
    assert {(wc.layout, wc.path) for wc in F.WSUM_CASES} == {("H", W.VEC), ("H", W.GENERIC), ("F", W.VEC)}
    assert {wc.lut for wc in F.WSUM_CASES} == {False, True}
    assert int(np.prod(F.WSUM_IMAGE)) == F.WSUM_IMAGE_BYTES == 2 ** 24


@pytest.mark.parametrize("wc", F.WSUM_CASES, ids=WIDS)
def test_wsum_layout_descriptor_and_no_alias_leaves_the_arena(wc):
    n, case = F.WSUM_IMAGE_BYTES, wc.case
    assert F.in_window(wc.layout, (wc.bs - 1) * n) and wc.bs * n < 2 ** 32 + 2 ** 26
    # the aliases are linear between multiples of 2^31: the ends of every 2^20-byte piece of the tensor stand for all its bytes
    lo = np.arange(0, wc.bs * n, 1 << 20, dtype=np.int64)
    for off in (lo, lo + (1 << 20) - 1):
        for alias in F.aliases(off):
            assert (F.BASE + alias).min() >= 0 and (F.BASE + alias).max() < F.ARENA
    # the descriptor: one image below 2^31 elements, the tensor at most 2^40, the forced kernel's class (wsum_plan.h)
    bs, h, w, c = case.shape
    assert h * w * c < 2 ** 31 and bs * h * w * c <= 2 ** 40 and case.nscales() == [64] and case.n_bias() == 64
    assert case.vec_class and W.auto_path(case) == W.VEC


@pytest.mark.parametrize("wc", F.WSUM_CASES, ids=WIDS)
def test_wsum_rolled_images_separate_the_aliases_and_are_not_degenerate(wc):
    img, exp = F.wsum_image(wc), F.wsum_expected(wc)
    assert img.dtype == np.uint8 and img.size == exp.size == F.WSUM_IMAGE_BYTES and exp.dtype == np.uint8
    # image b against images b - 128 and b - 256 (what a signed and a truncated offset reach): a roll by 128 or 256 pixels more
    for d in (128, 256):
        assert (np.roll(img, F.wsum_roll(d)) != img).mean() > 0.99, (wc.ident(), d)
        assert (np.roll(exp, F.wsum_roll(d)) != exp).mean() > 0.9, (wc.ident(), d)      # a wrapped read changes the result
    assert (exp != img).mean() > 0.9                                    # in place: an image that was not written shows
    # the op commutes with the roll (element-wise, per-channel constants, whole pixels): checked on the last image
    b = wc.bs - 1
    assert np.array_equal(F.wsum_reference(wc, np.roll(img, F.wsum_roll(b))), np.roll(exp, F.wsum_roll(b)))
    plain = F.wsum_expected(F.WsumFar(wc.layout, wc.bs, wc.path, False))    # (saturation: of the value in front of the table)
    assert len(np.unique(exp)) > 64 and ((plain == 0) | (plain == 255)).mean() < 0.10, wc.ident()


# ---- the dense far tensors of the head's pixel kernel ---------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", F.PIXEL_CASES, ids=lambda pc: pc.ident())
def test_pixel_layout_class_and_no_alias_leaves_the_arena(pc):
    case = pc.case
    assert F.PIXEL_ROWS == 2 ** 32 // 160 + 1000 and 2 ** 32 % F.PIXEL_LD != 0
    assert F.in_window("F", (F.PIXEL_ROWS - 1) * F.PIXEL_LD) and pc.far_bytes < 2 ** 32 + 2 ** 26
    assert pc.far_bytes == F.PIXEL_ROWS * max(case.ld, pc.idx_ld)
    lo = np.arange(0, pc.far_bytes, 1 << 20, dtype=np.int64)              # (the aliases are linear between multiples of 2^31)
    for off in (lo, np.minimum(lo + (1 << 20), pc.far_bytes) - 1):
        for alias in F.aliases(off):
            assert (F.BASE + alias).min() >= 0 and (F.BASE + alias).max() < F.ARENA
    for path in (H.PIXEL, H.GENERIC):                                      # the descriptor and the forced kernels' class
        assert H.in_class(case, path)
    assert case.k == 1 and case.c <= 256 and case.ld >= case.c and F.PIXEL_ROWS * max(case.ld, pc.idx_ld) <= 2 ** 40


def test_pixel_map_separates_the_aliases():
    """for every row i that starts beyond 2^32: the rows 2^32 / 160 in front of it, rounded either way (what a truncated byte
    offset reaches), are other rows of the block; and every row of the block is used"""
    first = -(-2 ** 32 // F.PIXEL_LD)
    i = np.arange(first, F.PIXEL_ROWS, dtype=np.int64)
    assert i.size >= 999
    for d in (2 ** 32 // F.PIXEL_LD, first):
        assert (i - d).min() >= 0 and (F.pixel_map(i) != F.pixel_map(i - d)).all()
    every = F.pixel_map(np.arange(F.PIXEL_ROWS, dtype=np.int64))
    assert every.min() == 0 and every.max() == F.PIXEL_R0 - 1 and len(np.unique(every[:F.PIXEL_R0])) == F.PIXEL_R0


@pytest.mark.parametrize("pc", F.PIXEL_CASES, ids=lambda pc: pc.ident())
def test_pixel_block_is_not_degenerate(pc):
    src, idx, val = F.pixel_block(pc)
    assert src.shape == (F.PIXEL_R0, pc.case.ld) and idx.shape == val.shape == (F.PIXEL_R0,) and idx.dtype == val.dtype == np.uint8
    assert np.array_equal(val, src[:, :pc.case.c].max(axis=1)) and len(np.unique(val)) > 1
    assert len(np.unique(idx)) > pc.case.c // 2                            # the argmax lands all over the channels
    first = -(-2 ** 32 // F.PIXEL_LD)
    i = np.arange(first, F.PIXEL_ROWS, dtype=np.int64)
    # A wrapped READ (src far) must change results: one differing row among the 1000 fails the GPU test, a majority is asked
    # for here (head_ref.generate plants the maximum at channel 0 in three row kinds of eight, so some rows agree by design).
    # A wrapped WRITE (idx far) lands on poison whatever the values are; there the map's separation above is what counts.
    for d in (2 ** 32 // F.PIXEL_LD, first):
        differ = (idx[F.pixel_map(i)] != idx[F.pixel_map(i - d)]).mean()
        assert differ > (0.5 if pc.operand == "src" else 0.0), (pc.ident(), differ)
