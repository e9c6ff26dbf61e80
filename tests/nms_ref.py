"""numpy f32 reference of the box decode + greedy NMS (dfx_nms_* of include/dfx.h), the case generators of the nms tests
and a Python mirror of the host plan (csrc/nms_plan.h).  Every arithmetic step is one numpy float32 operation in the order
of the definition; the selections are np.where with the definition's comparisons (np.maximum treats NaN differently)."""
import collections

import numpy as np

BOXES, DECODE = 0, 1
MASK, GENERIC = 0, 1
MAX_N, TILE = 4096, 64
GENERIC_THREADS, PREP_THREADS, MASK_THREADS, SCAN_THREADS = 1024, 256, 256, 64
MASK_AUTO_MIN_N, MASK_AUTO_MIN_OUT = 200, 100   # csrc/nms_plan.h NMS_MASK_AUTO_MIN_N, NMS_MASK_AUTO_MIN_OUT
F = np.float32

NmsCase = collections.namedtuple("NmsCase", "name bs n mode per_class classes apx n_anchors row_bytes thr clip")
NmsCase.__new__.__defaults__ = (BOXES, 0, 1, 1, None, None, 0.5, None)


def ident(case, max_out=None):
    return "%s bs%d n%d %s %s c%d A%d thr%g%s" % (case.name, case.bs, case.n, "decode" if case.mode == DECODE else "boxes",
                                                   "perclass" if case.per_class else "agnostic", case.classes, case.apx, case.thr,
                                                   "" if max_out is None else " max_out%d" % max_out)


# ---- the definition -----------------------------------------------------------------------------------------------------------
def n_valid(count_in, bs, n):
    if count_in is None:
        return [n] * bs
    return [min(max(int(c), 0), n) for c in count_in]


def clip_coord(x, hi):
    x = np.where(x < F(0), F(0), x)
    return np.where(x > F(hi), F(hi), x)


def decode(idx, deltas, anchors, tab_c, tab_s, classes, apx, clip=None):
    """idx {n} s32, deltas {n, row_bytes} u8 (raw bytes), anchors {n_anchors, 4} f32 -> boxes {n, 4} f32, ok {n} bool"""
    idx = np.asarray(idx, dtype=np.int64)
    n_entries = anchors.shape[0] * classes
    ok = (idx >= 0) & (idx < n_entries)
    e = np.where(ok, idx, 0)
    g = e // classes
    a = g % apx
    rows = np.arange(idx.size)
    q = [deltas[rows, 4 * a + i].astype(np.int64) for i in range(4)]
    A = anchors[g].astype(F)
    half = F(0.5)
    with np.errstate(all="ignore"):
        aw, ah = A[:, 2] - A[:, 0], A[:, 3] - A[:, 1]
        acx, acy = A[:, 0] + half * aw, A[:, 1] + half * ah
        cx, cy = acx + tab_c[q[0]] * aw, acy + tab_c[q[1]] * ah
        w, hh = aw * tab_s[q[2]], ah * tab_s[q[3]]
        hw, hhh = half * w, half * hh
        x1, y1, x2, y2 = cx - hw, cy - hhh, cx + hw, cy + hhh
        if clip is not None and clip[0] > 0:
            x1, x2 = clip_coord(x1, clip[0]), clip_coord(x2, clip[0])
            y1, y2 = clip_coord(y1, clip[1]), clip_coord(y2, clip[1])
    b = np.stack([x1, y1, x2, y2], axis=1).astype(F)
    b[~ok] = 0
    assert all(v.dtype == F for v in (aw, acx, cx, w, hw, x1))
    return b, ok


def area(b):
    with np.errstate(all="ignore"):
        return (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])


def suppress_row(a, others, thr):
    """does box a {4} (the LOWER position) suppress each of others {m, 4}?  Labels are the caller's."""
    with np.errstate(all="ignore"):
        xx1 = np.where(a[0] > others[:, 0], a[0], others[:, 0])
        yy1 = np.where(a[1] > others[:, 1], a[1], others[:, 1])
        xx2 = np.where(a[2] < others[:, 2], a[2], others[:, 2])
        yy2 = np.where(a[3] < others[:, 3], a[3], others[:, 3])
        w, h = xx2 - xx1, yy2 - yy1
        w = np.where(w > F(0), w, F(0))
        h = np.where(h > F(0), h, F(0))
        inter = w * h
        u = (area(a) + area(others)) - inter
        q = inter / u
        assert q.dtype == F
        return q > F(thr)


def suppress_matrix(boxes, labels, thr):
    """S[i, j]: i < j, equal labels >= 0 and box i suppresses box j"""
    n = boxes.shape[0]
    S = np.zeros((n, n), dtype=bool)
    for i in range(n - 1):
        S[i, i + 1:] = suppress_row(boxes[i], boxes[i + 1:], thr) & (labels[i + 1:] == labels[i]) & (labels[i] >= 0)
    return S


def greedy(boxes, labels, nv, thr, max_out):
    """kept positions, ascending (labels < 0: invalid)"""
    alive = labels[:nv] >= 0
    keep = []
    for j in range(nv):
        if not alive[j]:
            continue
        keep.append(j)
        if len(keep) == max_out:
            break
        if j + 1 < nv:
            alive[j + 1:] &= ~(suppress_row(boxes[j], boxes[j + 1:nv], thr) & (labels[j + 1:nv] == labels[j]))
    return keep


def labels_of(case, idx_row):
    """labels {n} (-1: invalid) of one image from its idx row (or None)"""
    if idx_row is None:
        return np.zeros(case.n, dtype=np.int64)
    e = np.asarray(idx_row, dtype=np.int64)
    ok = (e >= 0) & (e < n_anchors_of(case) * case.classes)
    lab = e % case.classes if case.per_class else np.zeros_like(e)
    return np.where(ok, lab, -1)


def n_anchors_of(case):
    return (2 ** 31 - 1) // case.classes if case.n_anchors is None else case.n_anchors


def reference(case, max_out, boxes=None, idx=None, deltas=None, anchors=None, tabs=None, count_in=None):
    """-> keep {bs, max_out} s32 (-1 behind the count), count {bs} s32, boxes_out {bs, max_out, 4} f32, decoded {bs, n, 4}"""
    keep = np.full((case.bs, max_out), -1, dtype=np.int32)
    count = np.zeros(case.bs, dtype=np.int32)
    bout = np.zeros((case.bs, max_out, 4), dtype=F)
    dec = np.zeros((case.bs, case.n, 4), dtype=F)
    reads_idx = case.mode == DECODE or case.per_class
    for r, nv in enumerate(n_valid(count_in, case.bs, case.n)):
        lab = labels_of(case, idx[r, :case.n] if reads_idx else None)
        if case.mode == DECODE:
            b, _ = decode(idx[r, :case.n], deltas[r], anchors, tabs[0], tabs[1], case.classes, case.apx, case.clip)
        else:
            b = boxes[r]
        dec[r] = b
        k = greedy(b, lab, nv, case.thr, max_out)
        keep[r, :len(k)] = k
        count[r] = len(k)
        bout[r, :len(k)] = b[k]
    return keep, count, bout, dec


# ---- generators ---------------------------------------------------------------------------------------------------------------
def clustered_boxes(rng, n, clusters=None, size=40.0, jitter=6.0, extent=512.0):
    """n boxes around a few centres: many overlaps inside a cluster, none between"""
    clusters = max(1, n // 12) if clusters is None else clusters
    centres = rng.uniform(0, extent, (clusters, 2))
    which = rng.integers(0, clusters, n)
    c = centres[which] + rng.normal(0, jitter, (n, 2))
    wh = size * rng.uniform(0.6, 1.4, (n, 2))
    return np.concatenate([c - wh / 2, c + wh / 2], axis=1).astype(F)


def grid_aligned_boxes(rng, n, extent=64):
    """coordinates multiples of 1/4 below 2^10 (here below `extent`): every f32 step before the division is exact"""
    lo = rng.integers(0, 4 * extent - 8, (n, 2))
    wh = rng.integers(0, 4 * 12, (n, 2))
    return (np.concatenate([lo, lo + wh], axis=1) / 4.0).astype(F)


def class_idx(rng, n, classes, n_anchors):
    """idx as select would emit it: e = anchor * classes + class"""
    return (rng.integers(0, n_anchors, n) * classes + rng.integers(0, classes, n)).astype(np.int32)


def decode_problem(rng, case, dtype=np.uint8):
    """idx {bs, n}, deltas {bs, n, row_bytes} u8 (raw bytes), anchors {n_anchors, 4}, (tab_c, tab_s) of a DECODE case"""
    import importlib
    capi = importlib.import_module("deep-fusion_amd.capi")
    na = n_anchors_of(case)
    cells = rng.uniform(0, 480, (na, 2))
    wh = rng.uniform(16, 96, (na, 2))
    anchors = np.concatenate([cells - wh / 2, cells + wh / 2], axis=1).astype(F)
    idx = np.stack([class_idx(rng, case.n, case.classes, na) for _ in range(case.bs)])
    deltas = rng.integers(0, 256, (case.bs, case.n, case.row_bytes), dtype=np.uint8)
    zp = 128 if np.dtype(dtype) == np.uint8 else 0
    tabs = capi.box_tables(1.0 / 32, zp, 10.0, 5.0, dtype=dtype)
    return idx, deltas, anchors, tabs


# ---- the host plan (csrc/nms_plan.h) ------------------------------------------------------------------------------------------
def blocks(n):
    return (n + TILE - 1) // TILE


def tiles(n):
    b = blocks(n)
    return b * (b + 1) // 2


def enumerate_tiles(n):
    b = blocks(n)
    return [(rb, cb) for rb in range(b) for cb in range(rb, b)]


def round16(v):
    return (v + 15) // 16 * 16


def scratch_bytes(bs, n):
    b = blocks(n)
    rows = bs * b * TILE
    return rows * 16 + round16(rows * 4) + rows * b * 8 + round16(tiles(n) * 2)


def prep_grid(bs, n):
    return (bs * blocks(n) * TILE + PREP_THREADS - 1) // PREP_THREADS


def mask_grid(bs, n):
    per = MASK_THREADS // 64
    return (bs * tiles(n) + per - 1) // per


def lds_bytes(path):
    return (MASK_THREADS // 64) * TILE * 20 if path == MASK else MAX_N * 21


def launches(path):
    return 3 if path == MASK else 1


def auto_path(case, max_out):
    """AUTO RULE of include/dfx.h (DFX_NMS_AUTO_NOTE): the mask path from n = 200 and max_out = 100 on, the smallest measured"""
    return MASK if case.n >= MASK_AUTO_MIN_N and max_out >= MASK_AUTO_MIN_OUT else GENERIC


def algorithmic_bytes(case, max_out):
    e = case.bs * case.n
    b = e * 24 if case.mode == DECODE else e * 16 + (e * 4 if case.per_class else 0)
    return b + case.bs * max_out * 4 + case.bs * 4


def kernel_name(case, path):
    return "nms_%s<%s,%s,n%d>" % ("mask" if path == MASK else "generic", "decode" if case.mode == DECODE else "boxes",
                                  "perclass" if case.per_class else "agnostic", case.n)


def block_scan(diag, cand, budget):
    """mirror of nms_block_scan: diag 64 ints, cand a 64-bit int -> kept mask"""
    live, kept, taken = cand, 0, 0
    while live and taken < budget:
        t = (live & -live).bit_length() - 1
        kept |= 1 << t
        taken += 1
        live &= ~diag[t] & ~(1 << t)
    return kept


def plan_points():
    return [(1, 1), (3, 63), (1, 64), (3, 65), (2, 128), (1, 130), (8, 1000), (1, 2000), (8, 200), (1, 4096), (8, 4096)]


# ---- the case tables of the tests ------------------------------------------------------------------------------------------------
def cut(full, max_out):
    """from reference(..., max_out = n) the result under a smaller max_out: greedy keeps a prefix of the same walk"""
    keep, count, bout, dec = full
    k = np.full((keep.shape[0], max_out), -1, dtype=np.int32)
    b = np.zeros((keep.shape[0], max_out, 4), dtype=F)
    c = np.minimum(count, max_out).astype(np.int32)
    for r in range(keep.shape[0]):
        k[r, :c[r]] = keep[r, :c[r]]
        b[r, :c[r]] = bout[r, :c[r]]
    return k, c, b, dec


def max_outs(kept, n):
    """1, kept - 1, kept, kept + 1, n"""
    return sorted({m for m in (1, kept - 1, kept, kept + 1, n) if 1 <= m <= n})


SIZES = (1, 63, 64, 65, 128, 130, 1000)


def size_problem(n, bs, seed=0):
    """clustered boxes of a BOXES / agnostic case of n candidates"""
    rng = np.random.default_rng(100 + 7 * n + bs + seed)
    return np.stack([clustered_boxes(rng, n) for _ in range(bs)])


def count_ins(n, bs):
    """the count_in vectors a size is run with: absent, and -1, 0, 1, n, n + 5 spread over the images"""
    pool = [-1, 0, 1, n, n + 5, max(1, n // 2)]
    out = [None]
    for s in range(0, len(pool), bs):
        v = pool[s:s + bs]
        out.append(np.array((v + pool)[:bs], dtype=np.int32))
    return out


def far_boxes(n):
    """n boxes 20 x 20, 30 apart: no two touch"""
    i = np.arange(n, dtype=np.float64)
    return np.stack([1000 + 30 * i, np.zeros(n), 1020 + 30 * i, np.full(n, 20.0)], axis=1).astype(F)


PLANTED = ("identical", "disjoint", "chain", "first_last", "zero_area", "inverted", "nan_inf", "at_thr", "below_thr")


def planted(name, n=130):
    """-> (boxes {1, n, 4}, thr) of a BOXES / agnostic case; what each must show is asserted in tests/test_nms_cpu.py"""
    b = far_boxes(n)
    thr = 0.5
    if name == "identical":
        b[:] = [3, 4, 13, 24]
    elif name == "chain":      # A at 0, B at 64 (suppressed by A), C at 129 overlaps only B
        thr = 0.3
        b[0], b[64], b[129] = [0, 0, 10, 10], [4, 0, 14, 10], [8, 0, 18, 10]
    elif name == "first_last":
        b[3] = b[n - 1] = [0, 0, 10, 10]
    elif name == "zero_area":  # 0 / 0: NaN, which does not suppress
        b[1] = b[2] = b[70] = [5, 5, 5, 5]
        b[4] = b[5] = [0, 0, 10, 0]
    elif name == "inverted":
        b[1] = b[2] = [10, 10, 0, 0]
        b[3], b[66] = [0, 0, 10, 10], [10, 0, 0, 10]
        b[7] = b[8] = [20, 20, 30, 10]
    elif name == "nan_inf":
        nan, inf = np.nan, np.inf
        b[1], b[2], b[3] = [nan, 0, 10, 10], [0, 0, 10, 10], [0, 0, 10, 10]
        b[5], b[6] = [0, nan, 10, 10], [nan, nan, nan, nan]
        b[10], b[11], b[12] = [-inf, -inf, inf, inf], [0, 0, inf, 10], [0, 0, inf, 10]
        b[65], b[66] = [-inf, 0, 10, 10], [-inf, 0, 10, 10]
        b[100] = [inf, inf, inf, inf]
    elif name in ("at_thr", "below_thr"):  # IoU exactly 0.5: not above 0.5, above the next float below it
        b[0], b[64] = [0, 0, 2, 2], [0, 0, 2, 1]
        thr = 0.5 if name == "at_thr" else float(np.nextafter(F(0.5), F(0)))
    elif name != "disjoint":
        raise ValueError(name)
    return b[None], thr


RANDOM = tuple((pc, classes, thr) for pc, classes in ((0, 1), (1, 1), (1, 3), (1, 80)) for thr in (0.3, 0.5, 0.7))


def random_problem(pc, classes, thr, n=200, bs=2):
    """-> (case, boxes, idx) of a clustered random BOXES case"""
    rng = np.random.default_rng(int(1000 * thr) + 10 * classes + pc)
    case = NmsCase("random", bs, n, BOXES, pc, classes, 1, 1000, None, thr)
    boxes = np.stack([clustered_boxes(rng, n, clusters=n // 20) for _ in range(bs)])
    idx = np.stack([class_idx(rng, n, classes, 1000) for _ in range(bs)])
    return case, boxes, idx


DECODES = tuple((dt, apx, classes, clip) for dt in (np.uint8, np.int8) for apx, classes in ((1, 1), (3, 80), (9, 1), (9, 80))
                for clip in (None, (400.0, 300.0)))


def decode_case(dt, apx, classes, clip, thr, n=400, bs=2):
    """-> (case, idx, deltas, anchors, tabs): every byte value in every one of the four slots, idx entries of -1 and out of
    range among the valid positions"""
    case = NmsCase("decode", bs, n, DECODE, int(classes > 1), classes, apx, 500, 4 * apx + 3, thr, clip)
    rng = np.random.default_rng(apx * 100 + classes + (7 if clip else 0) + (1 if np.dtype(dt) == np.int8 else 0))
    idx, deltas, anchors, tabs = decode_problem(rng, case, dt)
    rows = np.arange(n)
    for s in range(4 * apx):     # slot kind s % 4 of row i holds byte (7 i + 64 (s % 4)) % 256: all 256 values over 256 rows,
                                 # and rows 0 .. n - 257, the invalid ones among them, come twice
        deltas[:, :, s] = ((rows * 7 + 64 * (s % 4)) % 256).astype(np.uint8)[None, :]
    idx[:, 5] = -1
    idx[:, 70] = 500 * classes
    idx[0, 71] = 2 ** 31 - 1
    idx[bs - 1, 129] = -(2 ** 31)
    return case, idx, deltas, anchors, tabs
