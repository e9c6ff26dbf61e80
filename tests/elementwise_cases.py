"""Case tables and input generators shared by tests/test_elementwise_cpu.py and tests/test_gpu_elementwise.py
(concat, pooling, eltwise sum), so that the CPU pin of the oracle and the GPU comparison see the same bytes.

Inputs are built to hit what ordinary random numbers never do: NaNs of both signs with payloads, +-0, +-Inf,
+-FLT_MAX, +-FLT_MIN and denormals for f32; all-min / all-max windows, min/max pairs, exact .5 ties and averages
of exactly +-2^31 for the integer types.  The arrangements that decide an operand-order question (NaN first / last
in a window, +0 before -0, ...) are planted explicitly into chosen pooling windows, never left to the RNG;
`window_arrangements` finds them again, so a test can assert that a tensor really holds them."""
import numpy as np

DTYPES = (np.uint8, np.int8, np.int32, np.float32)


def f32_bits(*bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


PZ, NZ, PINF, NINF = 0x00000000, 0x80000000, 0x7F800000, 0xFF800000
FLT_MAX, FLT_MIN, DEN_MIN, DEN_MAX = 0x7F7FFFFF, 0x00800000, 0x00000001, 0x007FFFFF
SIGN = 0x80000000
QNANS = (0x7FC00000, 0x7FD5A5A5, 0xFFC00001, 0xFFEABCDE)      # quiet, both signs, two payloads each
F32_SPECIALS = (PZ, NZ, PINF, NINF, FLT_MAX, FLT_MAX | SIGN, FLT_MIN, FLT_MIN | SIGN, DEN_MIN, DEN_MIN | SIGN,
                DEN_MAX, DEN_MAX | SIGN) + QNANS
SPECIAL_SHARE = 8                                             # one position in 8 holds a special value


# ---- pool geometry: ((n, h, w, c), kernel, stride, pad, (oh, ow)), the format of test_oracle.POOL_CASES ----
_GEOMETRIES = [
    # name, (h, w), kernel, stride, pad, (oh, ow)
    ("window_larger_than_input", (3, 4), (5, 5), (1, 1), (2, 2), (3, 4)),
    ("stride_larger_than_window", (8, 7), (2, 2), (3, 3), (0, 0), (3, 2)),
    ("non_square", (7, 6), (1, 3), (2, 1), (0, 0), (4, 4)),
    ("padding_k_minus_1", (6, 5), (3, 3), (2, 2), (2, 2), (4, 4)),
    ("one_input_pixel", (1, 1), (1, 1), (2, 2), (0, 0), (1, 1)),
    ("one_output_pixel", (3, 3), (5, 5), (1, 1), (1, 1), (1, 1)),         # the window hangs over on all four sides
    ("overlapping_3x3", (13, 12), (3, 3), (2, 2), (1, 1), (7, 6)),         # ResNet-stem style
    ("plain_2x2", (16, 16), (2, 2), (2, 2), (0, 0), (8, 8)),
]
# c * itemsize % 16 == 0 takes the 16-byte path: 16 and 32 for every dtype, 20 and 4 for the 4-byte types only;
# 5 and 3 take the per-element path for every dtype
_CHANNELS = {"window_larger_than_input": (16, 5), "stride_larger_than_window": (32, 3), "non_square": (16, 20),
             "padding_k_minus_1": (16, 5), "one_input_pixel": (16, 4, 1), "one_output_pixel": (32, 5),
             "overlapping_3x3": (16, 20), "plain_2x2": (16, 5)}
POOL_GEOM_CASES = [((2, hw[0], hw[1], c), k, s, p, o) for name, hw, k, s, p, o in _GEOMETRIES for c in _CHANNELS[name]]


def pool_case_id(case):
    shape, k, s, p, o = case
    return "%s-k%dx%d-s%dx%d-p%dx%d" % ("x".join(map(str, shape)), k[0], k[1], s[0], s[1], p[0], p[1])


def pool_takes_vector_path(case, np_dt):
    return case[0][3] * np.dtype(np_dt).itemsize % 16 == 0


def pool_items(case, np_dt):
    """work items of one launch: one per 16 bytes of channels of an output pixel, or one per element"""
    shape, _, _, _, o = case
    es = np.dtype(np_dt).itemsize
    groups = shape[3] * es // 16 if pool_takes_vector_path(case, np_dt) else shape[3]
    return shape[0] * o[0] * o[1] * groups


# ---- second-pass shapes: pool and eltwise launch at most 2048 blocks x 256 threads = 524 288 work items and stride
#      over the rest, concat the same over 16-byte chunks ----
LAUNCH_ITEMS = 2048 * 256
# f32, c = 64 -> 16 groups of 16 bytes per pixel; (130 - 2) / 1 + 1 = 129 -> 2 * 129 * 129 * 16 = 532 512 items
POOL_BIG_VEC = ((2, 130, 130, 64), (2, 2), (1, 1), (0, 0), (129, 129))
# u8, c = 9 -> one item per element; (130 + 2 - 3) / 1 + 1 = 130 -> 4 * 130 * 130 * 9 = 608 400 items
POOL_BIG_SCALAR = ((4, 130, 130, 9), (3, 3), (1, 1), (1, 1), (130, 130))
# f32: 524 288 + 500 vector items of 4 elements, then 3 tail elements: items 524 288 .. 524 790 are a second pass
ELTWISE_BIG_F32 = (4 * LAUNCH_ITEMS + 4 * 500 + 3, 2)        # (elems, n_inputs)
# 1-byte types: 524 288 + 500 vector items of 16 elements, then 13 tail elements
ELTWISE_BIG_BYTE = (16 * LAUNCH_ITEMS + 16 * 500 + 13, 3)
# 4 * 130 * 130 = 67 600 pixels; [48, 16, 64] bytes = 8 chunks of 16 bytes per pixel -> 540 800 chunks
CONCAT_BIG_PIXELS = (4, 130, 130)
CONCAT_BIG_BYTE_CHANNELS = [48, 16, 64]
CONCAT_BIG_F32_CHANNELS = [12, 4, 16]                         # the same 8 chunks per pixel

ELTWISE_CASES = [(1683, 2), (1837, 8), (5, 2), (16 * 40, 3)]  # (elems, n_inputs): with tails of 3 / 13 / 5 / none
CONCAT_PIXELS = (2, 3, 5)
CONCAT_CHANNELS = {1: [16, 48, 32], 4: [4, 12, 8]}            # by itemsize: 1, 3 and 2 chunks of 16 bytes


def eltwise_items(elems, np_dt):
    per = 16 // np.dtype(np_dt).itemsize
    return elems // per + elems % per


# ---- windows ----
def window_positions(case, oy, ox):
    """(y, x) of the window's positions inside the input, in the order the kernels visit them (rows outer)"""
    shape, k, s, p, _ = case
    out = []
    for ky in range(k[0]):
        y = oy * s[0] - p[0] + ky
        if 0 <= y < shape[1]:
            for kx in range(k[1]):
                x = ox * s[1] - p[1] + kx
                if 0 <= x < shape[2]:
                    out.append((y, x))
    return out


def _plant_sites(case, count):
    """`count` (n, oy, ox, channel) sites whose windows do not share an input position with another site of the same
    channel; the windows with the most positions inside the input come first.  Fewer than `count` when the tensor is
    too small."""
    shape, _, _, _, o = case
    wins = [(n, oy, ox) for n in range(shape[0]) for oy in range(o[0]) for ox in range(o[1])]
    wins.sort(key=lambda w: -len(window_positions(case, w[1], w[2])))      # stable: ties stay in raster order
    used, sites = {}, []
    for ch in range(shape[3]):
        for (n, oy, ox) in wins:
            pos = set((n,) + q for q in window_positions(case, oy, ox))
            # neighbours of a taken window overlap it: keep them free too, so a planted window stays as planted
            if pos & used.setdefault(ch, set()):
                continue
            used[ch] |= pos
            sites.append((n, oy, ox, ch))
            if len(sites) == count:
                return sites
            break                                                          # next channel first: spread the sites
    for ch in range(shape[3]):                                             # second round: more windows per channel
        for (n, oy, ox) in wins:
            pos = set((n,) + q for q in window_positions(case, oy, ox))
            if pos & used[ch]:
                continue
            used[ch] |= pos
            sites.append((n, oy, ox, ch))
            if len(sites) == count:
                return sites
    return sites


def _f32_window_patterns(m):
    """[(name, bit patterns for a window of m positions in visit order)], without those that m is too small for"""
    one, two, neg = 0x3F800000, 0x40000000, 0xBF800000
    pats = {
        "nan_first": [QNANS[1]] + [one + i for i in range(m - 1)] if m >= 2 else None,
        "nan_last": [two + i for i in range(m - 1)] + [QNANS[3]] if m >= 2 else None,
        "nan_middle": [one] * (m // 2) + [QNANS[2]] + [two] * (m - m // 2 - 1) if m >= 3 else None,
        "pz_before_nz": [PZ, NZ] + [neg] * (m - 2) if m >= 2 else None,
        "nz_before_pz": [NZ, PZ] + [neg] * (m - 2) if m >= 2 else None,
        "inf_both": [PINF] + [one] * (m - 2) + [NINF] if m >= 2 else None,
        "nan_only_payload": [QNANS[1]] * m,
        "all_ninf": [NINF] * m,
        "all_nz": [NZ] * m,
        "denormals": [(DEN_MIN, DEN_MAX, FLT_MIN, DEN_MAX | SIGN)[i % 4] for i in range(m)],
        "all_flt_max": [FLT_MAX] * m,
    }
    return [(k, v) for k, v in pats.items() if v is not None]       # in this order: the decisive ones first


def special_f32(shape, seed, window=None):
    """ordinary normals; every SPECIAL_SHARE-th position (a seeded choice) holds one of F32_SPECIALS in turn; with
    `window` (a pool case of this shape) the patterns of _f32_window_patterns are written into whole windows."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape) * 100).astype(np.float32)
    flat = x.reshape(-1).view(np.uint32)
    n = flat.size
    where = rng.permutation(n)[:max(1, n // SPECIAL_SHARE)] if n >= 2 else np.arange(0)
    flat[where] = np.array([F32_SPECIALS[i % len(F32_SPECIALS)] for i in range(where.size)], dtype=np.uint32)
    if window is not None:
        assert tuple(window[0]) == tuple(shape)
        bits = x.view(np.uint32)
        sites = _plant_sites(window, 2 * 11)
        k = 0
        for (nn, oy, ox, ch) in sites:
            pos = window_positions(window, oy, ox)
            pats = _f32_window_patterns(len(pos))
            for (y, xx), b in zip(pos, pats[k % len(pats)][1]):
                bits[nn, y, xx, ch] = b
            k += 1
    return x


def _int_window_patterns(m, np_dt):
    info = np.iinfo(np_dt)
    pats = {
        "all_min": [info.min] * m,
        "all_max": [info.max] * m,
        "alternate": [(info.min, info.max)[i % 2] for i in range(m)],
    }
    if m % 2 == 0:      # sum / m lands exactly on .5 (-> 0) and on 1.5 (-> 2): nearest even
        pats["tie_half"] = [m // 2] + [0] * (m - 1)
        pats["tie_one_and_half"] = [m, m // 2] + [0] * (m - 2)
    if np_dt == np.int32 and m >= 2:
        # float(m * (2^31 - 1)) rounds up to m * 2^31 for every m <= 25, the quotient is exactly 2^31 -> INT32_MAX;
        # one value lower still rounds to the same float
        pats["near_max"] = [info.max] * (m - 1) + [info.max - 1]
        pats["near_min"] = [info.min] * (m - 1) + [info.min + 1]
    return list(pats.items())


def special_int(shape, np_dt, seed, window=None):
    """full-range random integers; the first pixel (every channel) all min, the second all max, the first half of
    the last pixel alternating min / max; with `window` whole windows of _int_window_patterns."""
    rng = np.random.default_rng(seed)
    info = np.iinfo(np_dt)
    x = rng.integers(info.min, int(info.max) + 1, shape).astype(np_dt)
    px = x.reshape(-1, shape[-1])
    if px.shape[0] >= 3:
        px[0, :] = info.min
        px[1, :] = info.max
        px[-1, ::2] = info.min
        px[-1, 1::2] = info.max
    if window is not None:
        assert tuple(window[0]) == tuple(shape)
        sites = _plant_sites(window, 2 * 7)
        k = 0
        for (nn, oy, ox, ch) in sites:
            pos = window_positions(window, oy, ox)
            pats = _int_window_patterns(len(pos), np_dt)
            for (y, xx), v in zip(pos, pats[k % len(pats)][1]):
                x[nn, y, xx, ch] = v
            k += 1
    return x


def pool_input(case, np_dt, seed=11):
    if np_dt == np.float32:
        return special_f32(case[0], seed, window=case)
    return special_int(case[0], np_dt, seed, window=case)


def window_arrangements(x, case):
    """names of the decisive arrangements that some window of `x` holds (f32 only): what special_f32 promises"""
    shape, _, _, _, o = case
    found = set()
    b = x.view(np.uint32)
    for n in range(shape[0]):
        for oy in range(o[0]):
            for ox in range(o[1]):
                pos = window_positions(case, oy, ox)
                w = np.stack([b[n, y, xx, :] for (y, xx) in pos])               # (m, c) bit patterns
                f = w.view(np.float32)
                nan = np.isnan(f)
                m = len(pos)
                if m >= 2:
                    if (nan[0] & ~nan[1:].any(axis=0)).any():
                        found.add("nan_first")
                    if (nan[-1] & ~nan[:-1].any(axis=0)).any():
                        found.add("nan_last")
                    if ((w[0] == PINF) & (w[-1] == NINF)).any():
                        found.add("inf_both")
                    rest_neg = (f[2:] < 0).all(axis=0) if m > 2 else np.ones(w.shape[1], bool)
                    if ((w[0] == PZ) & (w[1] == NZ) & rest_neg).any():
                        found.add("pz_before_nz")
                    if ((w[0] == NZ) & (w[1] == PZ) & rest_neg).any():
                        found.add("nz_before_pz")
                if m >= 3 and (nan[1:-1].any(axis=0) & ~nan[0] & ~nan[-1]).any():
                    found.add("nan_middle")
    return found


def eltwise_inputs(elems, np_dt, n, seed=31):
    """n flat tensors.  f32: special_f32, with the first positions set so that Inf - Inf, NaN + x, x + NaN, -0 + -0,
    +0 + -0, FLT_MAX + FLT_MAX and sums of denormals all occur.  Integers: special_int; even positions are scaled
    down by n so that their sums stay in range (odd positions saturate), then columns of all min, all max and
    alternating min / max."""
    if np_dt == np.float32:
        xs = [special_f32((elems,), seed + i) for i in range(n)]
        one = 0x3F800000
        cols = [[PINF, NINF], [NINF, PINF], [QNANS[1], one], [one, QNANS[3]], [NZ, NZ], [PZ, NZ], [NZ, PZ],
                [FLT_MAX, FLT_MAX], [FLT_MAX | SIGN, FLT_MAX | SIGN], [DEN_MIN, DEN_MAX], [FLT_MIN, DEN_MIN | SIGN],
                [DEN_MAX, DEN_MIN], [QNANS[0], QNANS[2]], [PINF, PINF], [NINF, one]]
        for j, col in enumerate(cols):
            # the first two inputs carry the pair; the others add -0, which changes no sum (x + -0 == x bit for bit)
            for i in range(n):
                if 2 * j + 1 < elems:
                    for pos, order in ((2 * j, col), (elems - 1 - 2 * j, col[::-1])):   # head: vector items, end: tail
                        xs[i].view(np.uint32)[pos] = order[i] if i < 2 else NZ
        return xs
    info = np.iinfo(np_dt)
    xs = [special_int((elems,), np_dt, seed + i) for i in range(n)]
    for i in range(n):
        xs[i][::2] = (xs[i][::2].astype(np.int64) // n).astype(np_dt)
        for j, v in enumerate((info.min, info.max, (info.min, info.max)[i % 2], (info.max, info.min)[i % 2])):
            for pos in (1 + 2 * j, elems - 2 - 2 * j):
                if 0 <= pos < elems:
                    xs[i][pos] = v
    return xs


def concat_inputs(pixels, channels, np_dt, seed=41):
    shapes = [tuple(pixels) + (c,) for c in channels]
    if np_dt == np.float32:
        return [special_f32(s, seed + i) for i, s in enumerate(shapes)]
    return [special_int(s, np_dt, seed + i) for i, s in enumerate(shapes)]


# ---- comparison rules ----
def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_selected_equal(got, ref, what=""):
    """bit for bit: for results that are one of the inputs (max pooling, concat, ReLU of a value passed through)"""
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    g, r = _bits(got), _bits(ref)
    if not np.array_equal(g, r):
        bad = np.argwhere(g != r)
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d elements differ; first at %s: got %r (0x%x) want %r (0x%x)" % (
            what, len(bad), g.size, i, got[i], int(g[i]), ref[i], int(r[i])))


def assert_computed_equal(got, ref, what=""):
    """for results of an addition or division: NaN exactly where the reference has NaN (an operation that produces a
    NaN gives the platform's default NaN, and which of two NaN operands survives is the platform's choice too), bits
    equal everywhere else"""
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    if got.dtype != np.float32:
        return assert_selected_equal(got, ref, what)
    gn, rn = np.isnan(got), np.isnan(ref)
    if not np.array_equal(gn, rn):
        i = tuple(np.argwhere(gn != rn)[0])
        raise AssertionError("%s: NaN in different places, %d of %d; first at %s: got %r want %r" % (
            what, int((gn != rn).sum()), got.size, i, got[i], ref[i]))
    g = np.where(rn, np.uint32(0), got.view(np.uint32))
    r = np.where(rn, np.uint32(0), ref.view(np.uint32))
    if not np.array_equal(g, r):
        bad = np.argwhere(g != r)
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d elements differ; first at %s: got %r (0x%x) want %r (0x%x)" % (
            what, len(bad), g.size, i, got[i], int(g[i]), ref[i], int(r[i])))
