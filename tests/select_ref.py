"""numpy reference of the image-wide top-K with peak filter (dfx_select_*, include/dfx.h), the Python mirror of its host
plan (csrc/select_plan.h) and the case tables of tests/test_select_cpu.py and tests/test_gpu_select.py.

The reference is the definition read literally: a candidate mask (src >= min_val; with PEAK3 also >= the maximum of the
3x3 window clipped to the image), np.lexsort by (value descending, element index ascending), the first k, fill, gather.
tests/test_select_cpu.py pins it against a pure-Python witness."""
import collections
import functools

import numpy as np

U8, S8 = 4, 3                       # DFX_U8, DFX_S8
NP_OF = {U8: np.uint8, S8: np.int8}
DT_NAME = {U8: "u8", S8: "s8"}
DT_MIN = {U8: 0, S8: -128}
DT_MAX = {U8: 255, S8: 127}
ALL, PEAK3 = 0, 1
HIST, GENERIC = 0, 1
MAX_K = 4096

# select_plan.h
THREADS, SORT_THREADS, BINS, MAX_CHUNKS = 256, 1024, 256, 1024
MIN_CHUNK_BYTES, WGS_PER_CU, MAX_GRID = 16384, 4, 1 << 20
HDR_WORDS, CHUNK_WORDS = 4, 3
HIST_AUTO_MIN_BYTES = 4096

# kind: how make_src fills the map ("random": a 12-value alphabet below the dtype's maximum, so that ties abound;
# planted kinds below).  min_val None: the dtype's minimum.
SelectCase = collections.namedtuple("SelectCase", "name bs h w c ld dt peak min_val kind seed")
SelectCase.__new__.__defaults__ = (None, "random", 0)


def ident(case, k=None):
    s = "%s-%dx%dx%dx%d/%d-%s-%s-min%s" % (case.name, case.bs, case.h, case.w, case.c, case.ld, DT_NAME[case.dt],
                                           "peak3" if case.peak else "all", case.min_val)
    return s if k is None else s + "-k%d" % k


def min_val_of(case):
    return DT_MIN[case.dt] if case.min_val is None else case.min_val


# ---- the data --------------------------------------------------------------------------------------------------------------
def alphabet(dt):
    """12 values over the dtype's range, its minimum among them and its maximum not"""
    lo, hi = DT_MIN[dt], DT_MAX[dt]
    return np.unique(np.concatenate([[lo, lo + 1, hi - 1, hi - 2], np.linspace(lo + 5, hi - 9, 8).astype(np.int64)]))


def make_src(case):
    """{bs, h, w, ld} of the case's dtype; the pad channels c .. ld-1 hold the dtype's maximum"""
    rng = np.random.default_rng(1234 + case.seed)
    shape = (case.bs, case.h, case.w, case.c)
    lo, hi = DT_MIN[case.dt], DT_MAX[case.dt]
    if case.kind == "random":
        al = alphabet(case.dt)
        # skewed: the high values are rare, as in a heat map
        p = np.linspace(3.0, 0.3, al.size)
        v = rng.choice(al, size=shape, p=p / p.sum())
    elif case.kind == "equal":
        v = np.full(shape, lo + 77, dtype=np.int64)
    elif case.kind == "two":
        # the tie bin (the lower value) spans every chunk; a few of the higher value in front, the middle and the end
        v = np.full(shape, lo + 40, dtype=np.int64)
        flat = v.reshape(case.bs, -1)
        n = flat.shape[1]
        for r in range(case.bs):
            flat[r, [1 % n, n // 2, n - 1]] = lo + 41
    elif case.kind == "plateau":
        # flat square plateaus of equal height on a low floor, some touching the border, plus lone peaks
        v = np.full(shape, lo + 3, dtype=np.int64)
        for r in range(case.bs):
            for _ in range(6):
                y, x = rng.integers(0, case.h), rng.integers(0, case.w)
                k = rng.integers(0, case.c)
                v[r, y:y + 3, x:x + 2, k] = lo + 100 + 10 * int(rng.integers(0, 3))
            for _ in range(5):
                v[r, rng.integers(0, case.h), rng.integers(0, case.w), rng.integers(0, case.c)] = hi - int(rng.integers(0, 2))
    elif case.kind == "extremes":
        v = rng.choice(np.array([lo, hi]), size=shape, p=[0.7, 0.3])
    elif case.kind.startswith("count"):
        # exactly int(kind[5:]) elements per image at the dtype's maximum, everything else at its minimum (use with ALL
        # and min_val = maximum)
        v = np.full(shape, lo, dtype=np.int64)
        flat = v.reshape(case.bs, -1)
        for r in range(case.bs):
            flat[r, rng.choice(flat.shape[1], size=int(case.kind[5:]), replace=False)] = hi
    else:
        raise ValueError(case.kind)
    src = np.full((case.bs, case.h, case.w, case.ld), hi, dtype=NP_OF[case.dt])
    src[..., :case.c] = v.astype(NP_OF[case.dt])
    return src


# ---- the reference -----------------------------------------------------------------------------------------------------------
def candidate_mask(case, src):
    """bool {bs, h, w, c}"""
    v = src[..., :case.c].astype(np.int32)
    m = v >= min_val_of(case)
    if case.peak == PEAK3:
        pad = np.full((case.bs, case.h + 2, case.w + 2, case.c), -1000, dtype=np.int32)
        pad[:, 1:-1, 1:-1, :] = v
        best = np.full_like(v, -1000)
        for dy in range(3):
            for dx in range(3):
                best = np.maximum(best, pad[:, dy:dy + case.h, dx:dx + case.w, :])
        m &= v >= best
    return m


def ranked(case, src):
    """per image: the element indices of ALL its candidates in the op's order (value descending, e ascending)"""
    m = candidate_mask(case, src).reshape(case.bs, -1)
    v = src[..., :case.c].astype(np.int32).reshape(case.bs, -1)
    out = []
    for r in range(case.bs):
        e = np.nonzero(m[r])[0]
        out.append(e[np.lexsort((e, -v[r, e]))].astype(np.int64))
    return out


def reference(case, src, k, order=None, gather_srcs=(), gather=()):
    """-> idx int32 {bs, k}, val {bs, k}, count int32 {bs}, [out_i uint8 {bs, k, row_bytes_i}].  order: ranked(case, src)
    when the caller has it.  gather_srcs: uint8 arrays {bs, h, w, pixel_stride_i}; gather: (row_bytes, stride) pairs."""
    order = ranked(case, src) if order is None else order
    flat = src[..., :case.c].reshape(case.bs, -1)
    idx = np.full((case.bs, k), -1, dtype=np.int32)
    val = np.zeros((case.bs, k), dtype=NP_OF[case.dt])
    count = np.zeros(case.bs, dtype=np.int32)
    outs = [np.zeros((case.bs, k, rb), dtype=np.uint8) for rb, _ in gather]
    for r in range(case.bs):
        e = order[r][:k]
        count[r] = e.size
        idx[r, :e.size] = e
        val[r, :e.size] = flat[r, e]
        for o, g, (rb, _) in zip(outs, gather_srcs, gather):
            o[r, :e.size] = g.reshape(case.bs, case.h * case.w, -1)[r][e // case.c, :rb]
    return (idx, val, count) + tuple(outs)


# ---- the plan (csrc/select_plan.h) ---------------------------------------------------------------------------------------------
Plan = collections.namedtuple("Plan", "chunk_px chunks items grid")


def plan(bs, px, ld, cus, forced_px=0):
    if forced_px > 0:
        cpx = forced_px
    else:
        per_image = max(1, (cus * WGS_PER_CU + bs - 1) // bs)
        cpx = max((px + per_image - 1) // per_image, (MIN_CHUNK_BYTES + ld - 1) // ld)
    cpx = min(max(cpx, (px + MAX_CHUNKS - 1) // MAX_CHUNKS), px)
    chunks = (px + cpx - 1) // cpx
    return Plan(cpx, chunks, bs * chunks, min(bs * chunks, MAX_GRID))


def round16(v):
    return (v + 15) // 16 * 16


def scratch_bytes(bs, chunks, k):
    return round16(bs * chunks * BINS * 4) + round16(bs * (HDR_WORDS + CHUNK_WORDS * chunks) * 4) + round16(bs * k * 8)


def lds_bytes(path):
    return MAX_K * 8 if path == HIST else MAX_K * 8 + BINS * 4 + 16 * 4 + 8 + 16


def launches(path):
    return 4 if path == HIST else 1


def hist_class(case):
    return case.ld % 16 == 0


def paths(case):
    return [HIST, GENERIC] if hist_class(case) else [GENERIC]


def auto_path(case):
    """AUTO RULE of include/dfx.h (DFX_SELECT_AUTO_NOTE): the histogram path in its class from images of 4096 bytes on"""
    return HIST if hist_class(case) and case.h * case.w * case.ld >= HIST_AUTO_MIN_BYTES else GENERIC


def kernel_name(case, k, path):
    return "select_%s<%s,%s,k%d>" % ("hist" if path == HIST else "generic", "peak3" if case.peak else "all", DT_NAME[case.dt], k)


def algorithmic_bytes(case, k, gather=()):
    return case.bs * case.h * case.w * case.c + case.bs * k * 4 + case.bs * 4 + sum(2 * case.bs * k * rb for rb, _ in gather)


def threshold(total, k):
    """select_threshold of select_plan.h -> (t, n_gt, quota, count)"""
    acc, lowest = 0, 0
    for b in range(BINS - 1, -1, -1):
        if total[b] == 0:
            continue
        if acc + total[b] >= k:
            return b, acc, k - acc, k
        acc += total[b]
        lowest = b
    return lowest, acc - total[lowest], total[lowest], acc


# ---- the tables ------------------------------------------------------------------------------------------------------------------
SHAPES = ((5, 7), (1, 1), (1, 9), (9, 1), (13, 16))
CLD = ((80, 80), (21, 32), (1, 16), (91, 96), (3, 3), (5, 7))   # the last two: generic only
TABLE_BS = 3
FIXED_K = (1, 7, 100, 4096)
REGIMES = ("zero", "fewer", "equal", "plus1", "more")


def min_vals(dt):
    """the dtype's minimum (all), a middle value, the dtype's maximum (above every element of a random map)"""
    return (None, DT_MIN[dt] + 120, DT_MAX[dt])


def chunk_settings(case):
    """DFX_SELECT_CHUNK values of the table: 1 pixel, two image rows minus one pixel, the default (None)"""
    return (1, max(1, 2 * case.w - 1), None)


@functools.lru_cache(maxsize=None)
def table_maps():
    """every score map of the table: the product of SHAPES, CLD, dtypes, peak modes and min_vals"""
    out = []
    for si, (h, w) in enumerate(SHAPES):
        for ci, (c, ld) in enumerate(CLD):
            for dt in (U8, S8):
                for peak in (ALL, PEAK3):
                    for mi, mv in enumerate(min_vals(dt)):
                        out.append(SelectCase("tab", TABLE_BS, h, w, c, ld, dt, peak, mv, "random", si * 100 + ci * 10 + mi))
    return tuple(out)


def regime(n, k):
    """the regime of an image with n candidates under k"""
    return "zero" if n == 0 else "fewer" if n < k else "equal" if n == k else "plus1" if n == k + 1 else "more"


def table_ks(n0):
    """the k's a map whose image 0 has n0 candidates is run with: the fixed ones, n0 and n0 +- 1"""
    return sorted({k for k in FIXED_K + (n0 - 1, n0, n0 + 1) if 1 <= k <= MAX_K})


@functools.lru_cache(maxsize=None)
def problem(case):
    """(src, order): the map and its ranked candidates, computed once per case and shared; never written to"""
    src = make_src(case)
    src.setflags(write=False)
    return src, ranked(case, src)


# the host tool (tools/select_plan_check) prints the plan of these (bs, px, ld, cus, forced) tuples; test_select_cpu.py
# compares them with plan() above
def plan_points():
    pts = []
    for h, w in SHAPES:
        for _, ld in CLD:
            if ld % 16:
                continue
            for forced in (1, max(1, 2 * w - 1), 0):
                pts.append((TABLE_BS, h * w, ld, 256, forced))
    pts += [(1, 128 * 128, 80, 256, 0), (8, 128 * 128, 80, 256, 0), (32, 128 * 128, 80, 256, 0), (1, 100 * 136, 720, 256, 0),
            (8, 100 * 136, 720, 256, 0), (1, 200 * 304, 16, 256, 0), (128, 1, 1008, 256, 0), (1, 1, 1008, 304, 0),
            (2, 3000000, 16, 256, 0), (2, 3000000, 16, 256, 5), (1000, 64, 16, 8, 0)]
    return pts
