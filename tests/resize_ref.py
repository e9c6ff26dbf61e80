"""Reference and case table of the activation resize tests (pure numpy, needs no GPU).

The op is defined in include/dfx.h: per axis, exact integer index arithmetic gives two source indices and, for
bilinear, one f32 division gives w1 (w0 = 1 - w1); the value is
    top = v[y0,x0]*wx0 + v[y0,x1]*wx1;  bot = v[y1,x0]*wx0 + v[y1,x1]*wx1;  out = top*wy0 + bot*wy1
with every multiply and add rounded to f32 on its own, then rint (ties to even) and a clamp for u8 / s8.  `tables` and
`resize` are the vectorised numpy formulation the GPU tests compare against bit for bit; `resize_scalar` is the same
formula as a pure-Python loop over single elements (tests/test_resize_cpu.py pins one against the other, against exact
rationals and against torch's conventions).  The library's own tables come from csrc/resize_plan.h; nothing here calls it.
"""
import numpy as np

NEAREST, BILINEAR = 0, 1                               # DFX_RESIZE_*
HALF_PIXEL, ALIGN_CORNERS, ASYMMETRIC = 0, 1, 2        # DFX_COORD_*
BAND, GENERIC = 0, 1                                   # dfx_resize_info.path
ALGOS = {"nearest": NEAREST, "bilinear": BILINEAR}
COORDS = {"half_pixel": HALF_PIXEL, "align_corners": ALIGN_CORNERS, "asymmetric": ASYMMETRIC}

# (ih, iw, oh, ow): up and down, non-integer factors, identity, one source row / column, long runs of one y0 (2 -> 33),
# y0 jumping by more than one (17 -> 3), and the two axes never the same
GEOMS = [(1, 1, 3, 5), (3, 1, 1, 5), (5, 7, 10, 14), (5, 7, 20, 28), (7, 5, 10, 9), (8, 8, 4, 4), (9, 6, 4, 11),
         (5, 7, 5, 7), (6, 14, 37, 23), (2, 2, 33, 33), (17, 3, 3, 17)]
# (numpy dtype, channel counts): 16-byte multiples (the band kernel's class) and others
CHANNELS = [(np.uint8, (16, 48, 5, 1)), (np.int8, (16, 48, 5, 1)), (np.float32, (4, 12, 3))]
S32_CHANNELS = (4,)                                    # nearest only
BATCHES = (1, 3)
# the (in, out) pairs whose tables tools/resize_plan_check must print as resize_ref.tables gives them
PLAN_PAIRS = [(1, 3), (3, 1), (5, 10), (5, 20), (7, 10), (8, 4), (9, 4), (6, 37), (14, 23), (2, 33), (17, 3), (65535, 1),
              (1, 65535)]

# The largest |resize(f32, bilinear) - torch.nn.functional.interpolate(mode='bilinear')| on N(0, 1) data over GEOMS, both
# align_corners settings, measured on the CPU (tests/test_resize_cpu.py prints it): 2.62e-06.  The two are not bit-equal
# because torch orders the operations differently; the tolerance is 4 x the measurement.  A wrong coordinate convention
# shows as 1e-1 or more.
TORCH_BILINEAR_MEASURED = 2.62e-06
TORCH_BILINEAR_TOL = 4 * TORCH_BILINEAR_MEASURED


def num_den(n, m, coord):
    """exact integer numerators (int64 array over the output index) and the denominator of the source coordinate"""
    o = np.arange(m, dtype=np.int64)
    if coord == HALF_PIXEL:
        return (2 * o + 1) * n - m, 2 * m
    if coord == ALIGN_CORNERS:
        return (o * (n - 1), m - 1) if m > 1 else (np.zeros(1, dtype=np.int64), 1)
    assert coord == ASYMMETRIC
    return o * n, m


def tables(n, m, algo, coord):
    """-> i0, i1 (int32), w0, w1 (float32) of one axis with `n` source and `m` output positions"""
    assert 1 <= n <= 65535 and 1 <= m <= 65535
    num, den = num_den(n, m, coord)
    if algo == BILINEAR:
        num = np.maximum(num, 0)
        i0 = np.minimum(num // den, n - 1)
        i1 = np.minimum(i0 + 1, n - 1)
        w1 = (num % den).astype(np.float32) / np.float32(den)
        w0 = np.float32(1.0) - w1
        return i0.astype(np.int32), i1.astype(np.int32), w0.astype(np.float32), w1.astype(np.float32)
    o = np.arange(m, dtype=np.int64)
    if coord == HALF_PIXEL:
        idx = ((2 * o + 1) * n) // (2 * m)
    elif coord == ASYMMETRIC:
        idx = (o * n) // m
    else:
        idx = (2 * num + den) // (2 * den)
    i0 = np.minimum(idx, n - 1).astype(np.int32)
    return i0, i0.copy(), np.ones(m, dtype=np.float32), np.zeros(m, dtype=np.float32)


def to_dtype(out_f32, dtype):
    """f32 -> dtype: f32 as it is; u8 / s8 rint (ties to even) and clamp"""
    if np.dtype(dtype) == np.float32:
        return out_f32.astype(np.float32)
    info = np.iinfo(dtype)
    return np.clip(np.rint(out_f32), info.min, info.max).astype(dtype)


def resize(src, out_hw, algo, coord):
    """src NHWC {bs, ih, iw, c} -> {bs, oh, ow, c} of the same dtype"""
    bs, ih, iw, c = src.shape
    oh, ow = out_hw
    y0, y1, wy0, wy1 = tables(ih, oh, algo, coord)
    x0, x1, wx0, wx1 = tables(iw, ow, algo, coord)
    if algo == NEAREST:
        return src[:, y0][:, :, x0].copy()                       # a bit copy
    assert src.dtype != np.int32, "bilinear on s32 is not part of the op"
    with np.errstate(invalid="ignore", over="ignore"):
        v = src.astype(np.float32)
        a0, a1 = wx0[None, None, :, None], wx1[None, None, :, None]
        r0, r1 = v[:, y0], v[:, y1]
        top = (r0[:, :, x0] * a0).astype(np.float32) + (r0[:, :, x1] * a1).astype(np.float32)
        bot = (r1[:, :, x0] * a0).astype(np.float32) + (r1[:, :, x1] * a1).astype(np.float32)
        b0, b1 = wy0[None, :, None, None], wy1[None, :, None, None]
        out = (top.astype(np.float32) * b0).astype(np.float32) + (bot.astype(np.float32) * b1).astype(np.float32)
    return to_dtype(out.astype(np.float32), src.dtype)


def eltwise2(a, b, post_relu):
    """dfx_eltwise on two inputs: exact integer sum saturated to the dtype, or the f32 sum a + b; then ReLU"""
    if a.dtype == np.float32:
        with np.errstate(invalid="ignore", over="ignore"):
            s = (a + b).astype(np.float32)
            return np.where(np.float32(0) > s, np.float32(0), s).astype(np.float32) if post_relu else s
    s = a.astype(np.int64) + b.astype(np.int64)
    if post_relu:
        s = np.maximum(s, 0)
    info = np.iinfo(a.dtype)
    return np.clip(s, info.min, info.max).astype(a.dtype)


def resize_add(src, add, out_hw, algo, coord, post_relu=False):
    return eltwise2(resize(src, out_hw, algo, coord), add, post_relu)


def resize_scalar(src, out_hw, algo, coord):
    """the formula of include/dfx.h one element at a time, with Python integers and np.float32 scalars"""
    bs, ih, iw, c = src.shape
    oh, ow = out_hw
    f = np.float32

    def axis(n, m, o):
        if coord == HALF_PIXEL:
            num, den = (2 * o + 1) * n - m, 2 * m
        elif coord == ALIGN_CORNERS:
            num, den = (o * (n - 1), m - 1) if m > 1 else (0, 1)
        else:
            num, den = o * n, m
        if algo == BILINEAR:
            num = max(num, 0)
            i0 = min(num // den, n - 1)
            w1 = f(f(num % den) / f(den))
            return i0, min(i0 + 1, n - 1), f(f(1.0) - w1), w1
        if coord == HALF_PIXEL:
            idx = ((2 * o + 1) * n) // (2 * m)
        elif coord == ASYMMETRIC:
            idx = (o * n) // m
        else:
            idx = (2 * num + den) // (2 * den)
        return min(idx, n - 1), min(idx, n - 1), f(1.0), f(0.0)

    ys = [axis(ih, oh, o) for o in range(oh)]
    xs = [axis(iw, ow, o) for o in range(ow)]
    dst = np.empty((bs, oh, ow, c), dtype=src.dtype)
    info = None if src.dtype in (np.float32, np.int32) else np.iinfo(src.dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for n in range(bs):
            for oy, (y0, y1, wy0, wy1) in enumerate(ys):
                for ox, (x0, x1, wx0, wx1) in enumerate(xs):
                    for k in range(c):
                        if algo == NEAREST:
                            dst[n, oy, ox, k] = src[n, y0, x0, k]
                            continue
                        top = f(f(f(src[n, y0, x0, k]) * wx0) + f(f(src[n, y0, x1, k]) * wx1))
                        bot = f(f(f(src[n, y1, x0, k]) * wx0) + f(f(src[n, y1, x1, k]) * wx1))
                        out = f(f(top * wy0) + f(bot * wy1))
                        if info is None:
                            dst[n, oy, ox, k] = out
                        else:
                            dst[n, oy, ox, k] = min(info.max, max(info.min, int(np.rint(out))))
    return dst


def random_src(shape, dtype, seed):
    """full-range integers with both ends present, N(0, 4) floats"""
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.float32:
        return (rng.standard_normal(shape) * 4).astype(np.float32)
    info = np.iinfo(dtype)
    a = rng.integers(info.min, info.max + 1, shape, dtype=np.int64).astype(dtype)
    a.flat[0], a.flat[-1] = info.min, info.max
    return a


def in_band_class(c, dtype):
    return (c * np.dtype(dtype).itemsize) % 16 == 0
