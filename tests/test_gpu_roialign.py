"""GPU: RoIAlign (dfx_roialign_*, deepfusion::roi_align) against the numpy reference of tests/roialign_ref.py, bit for bit
(tests/test_roialign_cpu.py pins that reference against a pure-Python witness, float64 and the ops that already exist).
Everything goes through the C ABI; dst lies between guard bands with poison fill, dst_ld = c + pad with the pad elements
still poison, src_ld > c with random pad channels.  Every case runs on auto, on the generic kernel and, where in its class,
on the tile kernel; all runs are compared with the reference (for f32 the NaN positions must agree, everything else is
bitwise), and the plan and the launch counts are asserted from info() and roialign_launches()."""
import importlib
import os
import subprocess
import threading

import numpy as np
import pytest

import fc_ref
import hipref
import nms_ref
import refmath
import resize_ref
import roialign_ref as R
import select_ref as SEL

pytestmark = pytest.mark.gpu
dfa = importlib.import_module("deep-fusion_amd")
capi = importlib.import_module("deep-fusion_amd.capi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "deep-fusion_amd", "tools")
GUARD = 1 << 12
F = np.float32


def on_device(a, offset=0):
    """the bytes of numpy array `a` on the device, `offset` bytes off a 16-byte boundary -> uint8 tensor (None stays None)"""
    import torch
    if a is None:
        return None
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf = torch.empty(raw.size + offset + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + raw.size]
    view.copy_(torch.from_numpy(raw.copy()))
    return view


class Dst:
    """dst {rows, ph, pw, ld} of `dtype`, `offset` bytes off a 16-byte boundary, GUARD bytes before and behind; poisoned"""

    def __init__(self, rows, ph, pw, c, ld, dtype, offset=0):
        import torch
        self.shape, self.c, self.dtype = (rows, ph, pw, ld), c, np.dtype(dtype)
        self.start, self.n = GUARD + offset, rows * ph * pw * ld * self.dtype.itemsize
        self.template = np.full((self.start + self.n + 15) // 16 * 16 + GUARD, hipref.GUARD_BYTE, dtype=np.uint8)
        self.template[self.start:self.start + self.n] = hipref.POISON_BYTE
        self.buf = torch.from_numpy(self.template.copy()).cuda()
        assert self.buf.data_ptr() % 16 == 0

    def dev(self):
        return self.buf[self.start:self.start + self.n]

    def raw(self):
        return self.buf.cpu().numpy()

    def fetch(self, what):
        got = self.raw()
        outside = np.ones(got.size, dtype=bool)
        outside[self.start:self.start + self.n] = False
        assert (got[outside] == hipref.GUARD_BYTE).all(), what + ": a guard band was overwritten"
        full = got[self.start:self.start + self.n].copy().view(self.dtype).reshape(self.shape)
        assert (np.ascontiguousarray(full[..., self.c:]).view(np.uint8) == hipref.POISON_BYTE).all(), what + ": elements c .. dst_ld-1 were written"
        return np.ascontiguousarray(full[..., :self.c])


def assert_same(got, want, what):
    """bit for bit; for f32 the NaN positions must agree and everything else is bitwise"""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype == np.float32:
        gn, wn = np.isnan(got), np.isnan(want)
        assert np.array_equal(gn, wn), "%s: NaN positions differ at %s" % (what, np.argwhere(gn != wn)[:5].tolist())
        got, want = np.where(gn, F(0), got), np.where(wn, F(0), want)
    hipref.assert_bit_equal(np.ascontiguousarray(got), np.ascontiguousarray(want), what)


class Problem:
    """levels: padded arrays {bs, h, w, ld}; the reference sees their first c channels"""

    def __init__(self, levels, c, boxes, out_hw, scales, S, aligned, thr=(), mode=R.BATCHED, count=None, batch_idx=None, dst_pad=None):
        self.levels, self.c, self.boxes, self.out_hw, self.scales, self.S, self.aligned = levels, c, np.asarray(boxes, dtype=np.float32), out_hw, scales, S, aligned
        self.thr, self.mode, self.count, self.batch_idx = np.asarray(thr, dtype=np.float32), mode, count, batch_idx
        self.dtype = levels[0].dtype
        self.bs = levels[0].shape[0]
        self.n = self.boxes.reshape(-1, 4).shape[0] // (self.bs if mode == R.BATCHED else 1)
        self.rows = self.bs * self.n if mode == R.BATCHED else self.n
        es = self.dtype.itemsize
        self.dst_ld = c + (16 // es if dst_pad is None else dst_pad)     # a pad that keeps the tile class
        self.lds = [lv.shape[3] for lv in levels] + [self.dst_ld]
        self._want = None

    @property
    def want(self):
        if self._want is None:
            self._want = R.roi_align([lv[..., :self.c] for lv in self.levels], self.boxes, self.out_hw, self.scales, self.S, self.aligned, self.thr,
                                     self.mode, self.count, self.batch_idx)
            self._want.setflags(write=False)
        return self._want

    def in_class(self):
        return R.tile_class(self.dtype, self.c, self.lds)

    def paths(self):
        return (-1, R.GENERIC, R.TILE) if self.in_class() else (-1, R.GENERIC)

    def op(self, path=-1):
        return dfa.RoiAlign(self.bs, self.n, [lv.shape[1:3] for lv in self.levels], self.c, self.dtype, self.out_hw, self.scales, self.S,
                            self.aligned, self.mode, self.thr, src_ld=[lv.shape[3] for lv in self.levels], dst_ld=self.dst_ld, force_path=path)

    def to_device(self, offsets=None):
        o = offsets or {}
        return dict(levels_dev=[on_device(lv, o.get("src%d" % i, 0)) for i, lv in enumerate(self.levels)], boxes_dev=on_device(self.boxes, o.get("boxes", 0)),
                    count=on_device(None if self.count is None else np.asarray(self.count, dtype=np.int32)),
                    batch_idx=on_device(None if self.batch_idx is None else np.asarray(self.batch_idx, dtype=np.int32)))

    def dst(self, offset=0):
        return Dst(self.rows, self.out_hw[0], self.out_hw[1], self.c, self.dst_ld, self.dtype, offset)

    def ident(self):
        return "%s c%d ld%s %dx%d S%d a%d bs%d n%d m%d L%d" % (R.DT_NAME[self.dtype], self.c, self.lds, self.out_hw[0], self.out_hw[1], self.S, self.aligned,
                                                            self.bs, self.n, self.mode, len(self.levels))


def assert_plan(p, info, path):
    want_path = R.auto_path(p.dtype, p.c, p.lds, p.rows, p.out_hw[0], p.out_hw[1]) if path == -1 else path
    what = "%s [%s]" % (p.ident(), info.kernel_name.decode())
    ph, pw = p.out_hw
    assert info.path == want_path and info.kernel_name.decode() == R.kernel_name(want_path, p.dtype, ph, pw, p.S, len(p.levels)), what
    assert (info.grid, info.block, info.lds_bytes, info.launches) == (R.grid(want_path, p.rows, ph, pw, p.c), R.THREADS, R.lds_bytes(want_path), 1), what
    assert info.rows_per_group == (R.rows_per_group(p.rows, ph) if want_path == R.TILE else 0), what
    assert info.algorithmic_bytes == R.algorithmic_bytes(p.mode, p.bs, p.rows, ph, pw, p.c, p.S, p.dtype), what
    return want_path, what


def check_every_path(p):
    dev = p.to_device()
    for path in p.paths():
        op = p.op(path)
        try:
            ran, what = assert_plan(p, op.info(), path)
            before = dfa.roialign_launches()
            d = p.dst()
            op.submit(dst_dev=d.dev(), **dev)
            got = d.fetch(what)
            after = dfa.roialign_launches()
            assert [after[k] - before[k] for k in range(2)] == [int(k == ran) for k in range(2)], what
            assert_same(got, p.want, what)
        finally:
            op.close()
    return p.want


def maps(rng, dtype, bs, shapes, c, ld):
    """padded maps {bs, h, w, ld}: every channel random, the pad ones too"""
    if np.dtype(dtype) == np.float32:
        return [(rng.standard_normal((bs, h, w, ld)) * 40).astype(np.float32) for h, w in shapes]
    info = np.iinfo(dtype)
    return [rng.integers(info.min, info.max + 1, (bs, h, w, ld)).astype(dtype) for h, w in shapes]


def boxes_around(rng, n, w, h, spread=0.4):
    x = np.sort(rng.uniform(-spread * w - 1, (1 + spread) * w + 1, (n, 2)), axis=1)
    y = np.sort(rng.uniform(-spread * h - 1, (1 + spread) * h + 1, (n, 2)), axis=1)
    return np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], axis=1).astype(np.float32)


# (dtype, c, src_ld): the tile class (16, 32, 48 bytes; f32 c 4 and 8) and the generic kernel alone (c 20, 3; f32 c 6; an ld
# that is no whole number of 16 bytes)
CHANNELS = ((np.uint8, 16, 32), (np.int8, 32, 48), (np.uint8, 48, 64), (np.uint8, 20, 32), (np.int8, 3, 5), (np.uint8, 16, 20),
            (np.float32, 4, 8), (np.float32, 8, 12), (np.float32, 6, 8))
OUTS = ((1, 1, 1, False), (2, 3, 2, True), (7, 7, 2, False), (14, 14, 3, True), (64, 1, 4, True), (3, 5, 4, False))
MAPS = ((1, 1), (1, 5), (5, 1), (2, 2), (13, 17))


# ---- 1. shapes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", MAPS, ids=lambda s: "%dx%d" % s)
def test_maps_channels_and_bins(hw):
    rng = np.random.default_rng(hw[0] * 100 + hw[1])
    k = nonzero = 0
    for dtype, c, ld in CHANNELS:
        for ph, pw, S, aligned in OUTS:
            bs, n = 1 + k % 3, (1, 5)[k % 2]
            k += 1
            lv = maps(rng, dtype, bs, [hw], c, ld)
            boxes = boxes_around(rng, bs * n, hw[1], hw[0]).reshape(bs, n, 4)
            nonzero += bool(check_every_path(Problem(lv, c, boxes, (ph, pw), [1.0], S, aligned)).any())
    assert nonzero > k // 2
    assert Problem(maps(rng, np.uint8, 1, [hw], 16, 32), 16, np.zeros((1, 1, 4)), (1, 1), [1.0], 1, True).in_class()
    assert not Problem(maps(rng, np.uint8, 1, [hw], 16, 20), 16, np.zeros((1, 1, 4)), (1, 1), [1.0], 1, True).in_class()


@pytest.mark.parametrize("dtype,c,ld", [(np.uint8, 32, 32), (np.float32, 4, 4), (np.int8, 20, 24)], ids=["u8c32", "f32c4", "s8c20"])
def test_n_70_splits_rois_over_workgroups(dtype, c, ld):
    """bs 3 x n 70 = 210 RoIs, fewer than the plan's workgroup target: the tile plan splits the bin rows of a RoI (7 rows ->
    runs of 3, 3, 1; 14 -> 5, 5, 4); bs 8 x n 70 = 560 is not split"""
    rng = np.random.default_rng(70)
    for bs, (ph, pw), rpg in ((3, (7, 7), 3), (3, (14, 14), 5), (8, (7, 7), 7), (1, (2, 3), 1)):
        lv = maps(rng, dtype, bs, [(13, 17)], c, ld)
        boxes = boxes_around(rng, bs * 70, 17, 13).reshape(bs, 70, 4)
        p = Problem(lv, c, boxes, (ph, pw), [1.0], 2, True, count=np.array([70, 33, 0, 70, 1, 70, 70, 69][:bs]))
        assert R.rows_per_group(p.rows, ph) == rpg
        check_every_path(p)


# ---- 2. planted boxes ----------------------------------------------------------------------------------------------------------------
PLANTED = np.array([
    [-50, -50, -20, -20], [30, 2, 60, 9], [2, -40, 9, -20], [2, 30, 9, 60],        # wholly outside on each side
    [-3, 2, 4, 9], [12, 2, 25, 9], [3, -3, 9, 4], [3, 9, 9, 20],                    # straddling each border
    [-1.5, -1.5, 0.5, 0.5], [-2, -2, 0, 0], [15, 11, 19, 15], [16, 12, 18, 14],     # samples in [-1, 0), at -1, at H and W
    [2, 3, 6, 7], [0.5, 0.5, 7.5, 7.5],                                             # samples on integer coordinates
    [4, 4, 4, 4], [9, 9, 3, 2], [0, 0, 0, 0],                                       # zero-size, inverted
    [-800, -600, 900, 700],                                                         # 100 x the map
    [np.nan, 1, 5, 5], [1, np.nan, 5, np.nan], [1, 1, np.inf, 5], [-np.inf, 1, 5, 5], [-np.inf, -np.inf, np.inf, np.inf],
    [1e30, 1e30, 2e30, 2e30], [-1e30, 0, 1e30, 5], [-1e30, -1e30, 1e30, 1e30], [1e-40, 1e-40, 3e-40, 2e-40], [-1e-45, 0, 1e-45, 1e-45],
    [0, 0, 17, 13]], dtype=np.float32)


@pytest.mark.parametrize("dtype,c,ld", [(np.uint8, 16, 16), (np.int8, 3, 3), (np.float32, 4, 4)], ids=["u8", "s8", "f32"])
def test_planted_boxes(dtype, c, ld):
    rng = np.random.default_rng(21)
    lv = maps(rng, dtype, 2, [(13, 17)], c, ld)
    if np.dtype(dtype) == np.float32:   # +-Inf and NaN pixels: an Inf under a zero weight is a NaN on every kernel
        lv[0][0, 3, 4, 0], lv[0][0, 6, 8, 1], lv[0][1, 12, 16, 2], lv[0][1, 0, 0, 3] = np.inf, -np.inf, np.nan, np.inf
    boxes = np.stack([PLANTED, PLANTED[::-1]])
    seen_nan = False
    for (ph, pw), S in (((1, 1), 1), ((7, 7), 2), ((2, 3), 4), ((4, 4), 1)):
        for aligned in (False, True):
            want = check_every_path(Problem(lv, c, boxes, (ph, pw), [1.0], S, aligned))
            assert not want[:4].any() and want[len(PLANTED) - 1].any()    # outside on each side: zeros; the whole map
            seen_nan = seen_nan or bool(np.isnan(want.astype(np.float64)).any())
    assert seen_nan == (np.dtype(dtype) == np.float32)


# ---- 3. levels -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [1, 2, 4])
@pytest.mark.parametrize("dtype,c", [(np.uint8, 16), (np.float32, 6)], ids=["u8c16", "f32c6"])
def test_levels_and_thresholds(levels, dtype, c):
    rng = np.random.default_rng(levels)
    shapes = [(16, 24), (8, 12), (5, 7), (2, 3)][:levels]
    scales = [1.0, 0.5, 0.25, 0.125][:levels]
    thr = np.array([4.0, 16.0, 64.0], dtype=np.float32)[:levels - 1]
    es = np.dtype(dtype).itemsize
    lv = [maps(rng, dtype, 2, [s], c, c + (i % 2) * 16 // es)[0] for i, s in enumerate(shapes)]
    rows = []
    for t in [F(4), F(16), F(64)]:   # area exactly at, just below and above each threshold: the box is t wide and 1 high
        rows += [[0, 2, v, 3] for v in (t, np.nextafter(t, F(0)), np.nextafter(t, F(1e9)))]
    rows += [[0, 0, 1.5, 1.5], [3, 3, 20, 15], [np.nan, 0, 1, 1]]
    boxes = np.array(rows + rows[::-1], dtype=np.float32).reshape(2, len(rows), 4)
    want_levels = [R.level_of(b, thr) for b in boxes[0]]
    assert sorted(set(want_levels)) == list(range(levels))
    assert want_levels[:9:3] == [min(i + 1, levels - 1) for i in range(3)] and want_levels[1:9:3] == [min(i, levels - 1) for i in range(3)]
    check_every_path(Problem(lv, c, boxes, (3, 3), scales, 2, True, thr))
    # every RoI of the batch on one level (the last)
    big = boxes_around(rng, 10, 24, 16).reshape(2, 5, 4)
    big[..., 2:] = big[..., :2] + F(100)
    assert {R.level_of(b, thr) for b in big.reshape(-1, 4)} == {levels - 1}
    check_every_path(Problem(lv, c, big, (2, 2), scales, 1, False, thr))


# ---- 4. modes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,c,ld", [(np.uint8, 16, 16), (np.float32, 6, 6)], ids=["u8c16", "f32c6"])
def test_batched_counts_and_list_indices(dtype, c, ld):
    rng = np.random.default_rng(4)
    bs, n = 3, 5
    lv = maps(rng, dtype, bs, [(13, 17), (6, 8)], c, ld)
    boxes = boxes_around(rng, bs * n, 17, 13, spread=0.0).reshape(bs, n, 4)
    thr = [60.0]
    for count in (None, [0, n, n + 4], [-2, 3, 1], [n, n, n], [0, 0, 0]):
        p = Problem(lv, c, boxes, (2, 2), [1.0, 0.5], 2, True, thr, count=None if count is None else np.array(count))
        want = check_every_path(p).reshape(bs, n, -1)
        for r in range(bs):
            nv = n if count is None else min(max(count[r], 0), n)
            assert not want[r, nv:].any() and (nv == 0 or want[r, :nv].any())
    for idx in ([0, 1, 2, 0, 1, 2, 2], [-1, 3, 2, 0, -7, 1, 1 << 30], [2, 2, 2, 2, 2, 2, 2], [3, -1, 3, -1, 3, -1, 3]):
        flat = boxes_around(rng, len(idx), 17, 13, spread=0.0)
        want = check_every_path(Problem(lv, c, flat, (3, 2), [1.0, 0.5], 1, False, thr, mode=R.LIST, batch_idx=np.array(idx)))
        for i, b in enumerate(idx):
            assert want[i].any() == (0 <= b < bs)


# ---- 5. the pins, on the device -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.int8])
def test_pins_against_pool_resize_and_a_crop(dtype):
    import torch
    rng = np.random.default_rng(8)
    bs, h, w, c = 2, 12, 16, 16
    src = maps(rng, dtype, bs, [(h, w)], c, c)[0]
    src_d = on_device(src)
    whole = np.tile(np.array([0, 0, w, h], dtype=np.float32), (bs, 1, 1))
    # 2 x 2 / 2 average pooling == RoIAlign of the whole map to (h/2, w/2), S 2
    pool = dfa.Pool(bs, c, h, w, h // 2, w // 2, (2, 2), (2, 2), (0, 0), dtype, algo=dfa.Pool.AVG_INCLUDE_PADDING)
    pooled = torch.zeros(bs * (h // 2) * (w // 2) * c, dtype=torch.uint8, device="cuda")
    pool.submit(src_d, pooled)
    pooled = pooled.cpu().numpy().view(dtype).reshape(bs, h // 2, w // 2, c)
    pool.close()
    assert np.array_equal(pooled, refmath.avgpool(src, (2, 2), (2, 2), (0, 0), (h // 2, w // 2), True).astype(dtype))
    assert_same(check_every_path(Problem([src], c, whole, (h // 2, w // 2), [1.0], 2, True)), pooled, "pool pin")
    # bilinear x 2 (half-pixel) == RoIAlign of the whole map to (2h, 2w), S 1
    rs = dfa.Resize((bs, h, w, c), (2 * h, 2 * w), dtype)
    up = torch.zeros(bs * 4 * h * w * c, dtype=torch.uint8, device="cuda")
    rs.submit(src_d, up)
    up = up.cpu().numpy().view(dtype).reshape(bs, 2 * h, 2 * w, c)
    rs.close()
    assert np.array_equal(up, resize_ref.resize(src, (2 * h, 2 * w), resize_ref.BILINEAR, resize_ref.HALF_PIXEL))
    assert_same(check_every_path(Problem([src], c, whole, (2 * h, 2 * w), [1.0], 1, True)), up, "resize pin")
    # a crop, and the same at scale 0.5 with the box doubled
    box = np.tile(np.array([5, 3, 12, 10], dtype=np.float32), (bs, 1, 1))
    for scale, b in ((1.0, box), (0.5, box * F(2))):
        assert_same(check_every_path(Problem([src], c, b, (7, 7), [scale], 1, True)), np.ascontiguousarray(src[:, 3:10, 5:12]), "crop pin")


# ---- 6. alignment, errors --------------------------------------------------------------------------------------------------------------
def test_misaligned_pointers_fall_back_to_generic_for_that_submit():
    """a level, boxes or dst 4 bytes off a 16-byte boundary: the forced tile handle runs the generic kernel for that submit
    (dfx_debug_roialign_launches), info() keeps the plan, the bytes are the same"""
    rng = np.random.default_rng(6)
    for dtype, c in ((np.uint8, 16), (np.float32, 4)):
        lv = maps(rng, dtype, 2, [(13, 17), (6, 8)], c, c)
        p = Problem(lv, c, boxes_around(rng, 12, 17, 13).reshape(2, 6, 4), (7, 7), [1.0, 0.5], 2, True, [50.0], count=np.array([6, 4]))
        op = p.op(R.TILE)
        try:
            for in_off, out_off in (({"src0": 4}, 0), ({"src1": 4}, 0), ({"boxes": 4}, 0), ({}, 4), ({"src0": 4, "boxes": 4}, 4), ({}, 0)):
                before = dfa.roialign_launches()
                d = p.dst(out_off)
                op.submit(dst_dev=d.dev(), **p.to_device(in_off))
                got = d.fetch("offset")
                after = dfa.roialign_launches()
                ran = R.GENERIC if (in_off or out_off) else R.TILE
                assert [after[k] - before[k] for k in range(2)] == [int(k == ran) for k in range(2)], (in_off, out_off)
                assert op.info().path == R.TILE
                assert_same(got, p.want, "offset %s %s" % (in_off, out_off))
        finally:
            op.close()


def test_errors_launch_nothing():
    """invalid descriptors; null pointers, an f32 / s32 pointer off its element, a dst that overlaps an input: the error code,
    nothing is launched, dst keeps its poison"""
    import torch
    rng = np.random.default_rng(2)
    before = dfa.roialign_launches()
    for kw in (dict(sampling_ratio=0), dict(sampling_ratio=5), dict(out_hw=(0, 7)), dict(spatial_scales=[float("nan")]), dict(c=20, force_path=dfa.ROIALIGN_TILE)):
        args = dict(bs=1, n=3, level_shapes=[(5, 5)], c=16, dtype=np.uint8, out_hw=(7, 7), spatial_scales=[1.0])
        args.update(kw)
        with pytest.raises(dfa.DfxError, match="dfx error 2" if kw == dict(sampling_ratio=0) else "dfx error 1"):
            dfa.RoiAlign(**args)
    lv = maps(rng, np.float32, 2, [(13, 17), (6, 8)], 4, 4)
    boxes = boxes_around(rng, 8, 17, 13)
    pb = Problem(lv, 4, boxes.reshape(2, 4, 4), (2, 2), [1.0, 0.5], 2, True, [50.0], count=np.array([4, 2]))
    pl = Problem(lv, 4, boxes, (2, 2), [1.0, 0.5], 2, True, [50.0], mode=R.LIST, batch_idx=np.array([0, 1] * 4))
    for path in (R.TILE, R.GENERIC):
        for p in (pb, pl):
            op = p.op(path)
            try:
                d = p.dst()
                good = dict(p.to_device(), dst_dev=d.dev())
                bad = [dict(boxes_dev=None), dict(dst_dev=None), dict(levels_dev=[good["levels_dev"][0], None]),
                       dict(boxes_dev=good["boxes_dev"][2:]), dict(dst_dev=d.dev()[2:]), dict(levels_dev=[good["levels_dev"][0][2:], good["levels_dev"][1]]),
                       dict(dst_dev=good["boxes_dev"]), dict(dst_dev=good["levels_dev"][1]), dict(dst_dev=good["levels_dev"][0][64:])]
                if p.mode == R.LIST:
                    bad += [dict(batch_idx=None), dict(batch_idx=good["batch_idx"][2:]), dict(dst_dev=good["batch_idx"])]
                else:
                    bad += [dict(count=good["count"][2:]), dict(dst_dev=good["count"])]
                for b in bad:
                    with pytest.raises(dfa.DfxError, match="dfx error 1"):
                        op.submit(**dict(good, **b))
                torch.cuda.synchronize()
                assert (d.raw() == d.template).all()
            finally:
                op.close()
    assert dfa.roialign_launches() == before


def test_auto_follows_the_measured_rule():
    """DFX_ROIALIGN_AUTO_NOTE restated in roialign_ref.auto_path: the measured sizes, just below each of them, outside the
    class; and auto gives the bits of the forced kernels on both sides of the rule"""
    rng = np.random.default_rng(1)
    for dtype, c, ld, n, out_hw, want in ((np.uint8, 256, 256, 1000, (7, 7), R.TILE), (np.uint8, 256, 256, 100, (14, 14), R.TILE),
                                          (np.float32, 64, 64, 100, (7, 7), R.TILE), (np.uint8, 256, 256, 99, (7, 7), R.GENERIC),
                                          (np.uint8, 240, 240, 100, (7, 7), R.GENERIC), (np.uint8, 256, 256, 100, (6, 8), R.GENERIC),
                                          (np.uint8, 256, 260, 100, (7, 7), R.GENERIC), (np.uint8, 16, 16, 5, (7, 7), R.GENERIC)):
        lv = maps(rng, dtype, 1, [(4, 4)], c, ld)
        p = Problem(lv, c, np.zeros((1, n, 4)), out_hw, [1.0], 2, True)
        assert R.auto_path(p.dtype, p.c, p.lds, p.rows, out_hw[0], out_hw[1]) == want, p.ident()
        op = p.op(-1)
        try:
            assert op.info().path == want, p.ident()
        finally:
            op.close()
    lv = maps(rng, np.uint8, 2, [(13, 17), (6, 8)], 256, 256)
    for n in (50, 49):   # 100 RoIs: tile on auto; 98: generic
        check_every_path(Problem(lv, 256, boxes_around(rng, 2 * n, 17, 13).reshape(2, n, 4), (7, 7), [1.0, 0.5], 2, False, [60.0]))


# ---- 7. threads and streams ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [R.TILE, R.GENERIC], ids=["tile", "generic"])
def test_one_handle_from_two_threads_and_on_three_streams(path):
    """two host threads, each on its own stream, and a third stream, four submits each on alternating inputs: every output
    holds the result of ITS input"""
    import torch
    rng = np.random.default_rng(13)
    lv = maps(rng, np.uint8, 2, [(13, 17), (6, 8)], 32, 32)
    probs = [Problem(lv, 32, boxes_around(rng, 2 * 40, 17, 13).reshape(2, 40, 4), (7, 7), [1.0, 0.5], 2, True, [50.0]) for _ in range(2)]
    assert not np.array_equal(probs[0].want, probs[1].want)
    devs = [p.to_device() for p in probs]
    op = probs[0].op(path)
    try:
        streams = [torch.cuda.Stream() for _ in range(3)]
        outs = [[probs[0].dst() for _ in range(4)] for _ in range(3)]
        torch.cuda.synchronize()
        errors = []

        def work(i):
            try:
                for j, o in enumerate(outs[i]):
                    op.submit(dst_dev=o.dev(), stream=streams[i], **devs[(i + j) % 2])
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        for t in threads:
            t.start()
        work(2)
        for t in threads:
            t.join()
        torch.cuda.synchronize()
        assert not errors, errors
        for i, per_stream in enumerate(outs):
            for j, o in enumerate(per_stream):
                assert_same(o.fetch("stream %d submit %d" % (i, j)), probs[(i + j) % 2].want, "stream %d submit %d" % (i, j))
    finally:
        op.close()


# ---- 8. the chain ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [-1, R.GENERIC, R.TILE], ids=["auto", "generic", "tile"])
def test_select_nms_roialign_fc_on_the_device(path):
    """SelectTopK over a score map -> BoxNms (DECODE; boxes_out, count) -> RoiAlign over a two-level u8 feature pyramid ->
    InnerProduct over the {R, 7, 7, 16} tiles, nothing touching the host in between; every tensor against the chained numpy
    references"""
    import torch
    bs, h, w, apx, classes, k, max_out, fc_c, oc = 2, 9, 11, 3, 5, 150, 120, 16, 32
    c = apx * classes
    sel = SEL.SelectCase("chain", bs, h, w, c, 16, SEL.U8, SEL.ALL, 230, "random", 3)
    src, order = SEL.problem(sel)
    rng = np.random.default_rng(77)
    dmap = rng.integers(96, 160, (bs, h, w, 4 * apx), dtype=np.uint8)
    gather = ((4 * apx, 4 * apx),)
    sidx, _, scount, rows = SEL.reference(sel, src, k, order, [dmap], gather)
    na = h * w * apx
    cy, cx = np.divmod(np.arange(h * w), w)
    base = np.stack([cx * 16.0, cy * 16.0], axis=1).repeat(apx, axis=0)
    half = np.tile(np.array([[16.0, 16.0], [24.0, 12.0], [12.0, 24.0]]), (h * w, 1))
    anchors = np.concatenate([base - half, base + half], axis=1).astype(np.float32)
    tabs = capi.box_tables(1.0 / 32, 128, 10.0, 5.0)
    ncase = nms_ref.NmsCase("chain", bs, k, nms_ref.DECODE, 1, classes, apx, na, 4 * apx, 0.4, (float(w * 16), float(h * 16)))
    keep, kcount, kboxes = nms_ref.reference(ncase, max_out, idx=sidx, deltas=rows, anchors=anchors, tabs=tabs, count_in=scount)[:3]
    assert 1 < kcount.min() and kcount.min() < max_out            # zero rows behind a count
    feats = maps(rng, np.uint8, bs, [(h * 2, w * 2), (h, w)], fc_c, fc_c)   # strides 8 and 16 of a 176 x 144 image
    feats = [f // 16 for f in feats]                              # the fully-connected layer's reference range
    thr = np.array([1100.0], dtype=np.float32)
    p = Problem(feats, fc_c, kboxes, (7, 7), [1.0 / 8, 1.0 / 16], 2, True, thr, count=kcount, dst_pad=0)
    assert {R.level_of(b, thr) for r in range(bs) for b in kboxes[r, :kcount[r]]} == {0, 1}
    fcase = fc_ref.FcCase("chain", bs * max_out, fc_c, 7, 7, oc)
    fdata = dict(fc_ref.generate(fcase), src=p.want)
    fwant = fc_ref.fc_ref(fcase, fdata)
    select = dfa.SelectTopK(bs, h, w, c, np.uint8, k, src_ld=16, min_val=230, gather=gather)
    nms = dfa.BoxNms(bs, k, max_out, 0.4, mode=nms_ref.DECODE, per_class=True, classes=classes, anchors_per_pixel=apx, n_anchors=na,
                     row_bytes=4 * apx, idx_ld=k, clip=ncase.clip)
    roi = p.op(path)
    fc = dfa.InnerProduct((bs * max_out, 7, 7, fc_c), oc, dst_dt=fcase.dst_dt, bia_dt=fcase.bia_dt, relu=fcase.relu)
    try:
        fc.set_weights(fdata["w"], fdata["scales"], fdata["bia"])
        idx_d = torch.full((bs, k), -7, dtype=torch.int32, device="cuda")
        cnt_d = torch.full((bs,), -7, dtype=torch.int32, device="cuda")
        rows_d = torch.full((bs, k, 4 * apx), 0xCD, dtype=torch.uint8, device="cuda")
        keep_d = torch.full((bs, max_out), -7, dtype=torch.int32, device="cuda")
        kcnt_d = torch.full((bs,), -7, dtype=torch.int32, device="cuda")
        kbox_d = torch.full((bs, max_out, 4), -7.0, dtype=torch.float32, device="cuda")
        tiles = p.dst()
        out_d = torch.full((bs * max_out, oc), 0xCD, dtype=torch.uint8, device="cuda")
        select.submit(on_device(src), idx_d, cnt_d, gather_src=[on_device(dmap)], gather_dst=[rows_d])
        nms.submit(keep_d, kcnt_d, idx=idx_d, deltas=rows_d, anchors=on_device(anchors), tab_c=on_device(tabs[0]), tab_s=on_device(tabs[1]),
                   count_in=cnt_d, boxes_out=kbox_d)
        roi.submit([on_device(f) for f in feats], kbox_d, tiles.dev(), count=kcnt_d)
        fc.submit(tiles.dev(), out_d)
        hipref.assert_bit_equal(kcnt_d.cpu().numpy(), kcount, "chain count")
        hipref.assert_bit_equal(keep_d.cpu().numpy(), keep, "chain keep")
        hipref.assert_bit_equal(kbox_d.cpu().numpy(), kboxes, "chain boxes_out")
        assert_same(tiles.fetch("chain tiles"), p.want, "chain tiles")
        hipref.assert_bit_equal(out_d.cpu().numpy().view(fwant.dtype).reshape(fwant.shape), fwant, "chain fc")
        assert fwant.any() and not fwant.all()
    finally:
        for o in (select, nms, roi, fc):
            o.close()


# ---- 9. the C++ API ----------------------------------------------------------------------------------------------------------------------
def test_roialign_check_tool():
    """tools/roialign_check: roi_align() of the drop-in layer against the scalar restatement of tools/roialign_host.h"""
    p = subprocess.run([os.path.join(TOOLS, "roialign_check")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = p.stdout.decode()
    assert p.returncode == 0, text
    lines = [ln for ln in text.splitlines() if ln.startswith("roialign_check ")]
    assert len(lines) >= 6 and all(ln.endswith(": ok") for ln in lines), text
    assert text.rstrip().endswith("PASS")
