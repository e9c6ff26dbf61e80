"""numpy reference of dfx_roialign (include/dfx.h): torchvision's roi_align forward with every step one separately rounded f32
operation in the order the header writes down.

  roi_align()         the reference: a Python loop over RoIs, vectorised inside one; every operand is np.float32, so each
                      numpy operation is one f32 operation rounded to nearest
  roi_align_scalar()  the witness: one output element at a time, one np.float32 operation per line
  roi_align_f64()     the same formulas in float64 (the level is taken from the f32 rule, which is part of the definition),
                      with the smallest distance of any sample coordinate from the validity borders -1 and L
At the end: the plan of csrc/roialign_plan.h restated (class, auto rule, RoI split, grids, LDS bytes, algorithmic bytes, kernel
names), which tests/test_gpu_roialign.py asserts against info().

ERROR BOUND of the f32 result against float64, for finite maps (error_bound()).  u = 2^-24.
  coordinate: y is reached through 11 roundings (x*s, -o for both ends; rh; bh; p*bh; the sum; (i+.5)*bh; /S; the last sum),
    each relative u on an intermediate no larger than Mc = 2 * max|coordinate * scale| + 2 (the RoI's size is at most twice the
    largest scaled coordinate, plus the offset and the clamp to 1), so |dy| <= 12 u Mc (11 roundings, second-order terms in
    the twelfth).  ly = y - floor(y) is exact.  Bilinear interpolation with the clamps at 0 and L-1 is continuous and changes
    by at most |dy| * (largest difference of neighbouring pixels) <= |dy| * 2 Vmax per axis: 2 * 12 u Mc * 2 Vmax in all.
    The valid bit is a discontinuity, so the bound is claimed only where no float64 coordinate lies within 12 u Mc of -1 or
    L (roi_align_f64 returns that margin; the tests assert it of their data).
  arithmetic: hy = 1 - ly, the weight product, w * v and the three adds put at most 7 roundings on a term, and the weights sum
    to 1: a sample is within 7 u Vmax.  The S^2 - 1 accumulations add at most u * S^2 Vmax each, the division by S^2 one more
    u Vmax: (8 + S^2) u Vmax after the division.
  together: |f32 - f64| <= u * Vmax * (8 + S^2 + 48 Mc).
"""
import numpy as np

BATCHED, LIST = 0, 1
U = 2.0 ** -24


def to_dtype(out, dtype):
    """f32 -> dtype: f32 as it is; u8 / s8 rint (ties to even) and clamp (resize_ref.to_dtype)"""
    if np.dtype(dtype) == np.float32:
        return out.astype(np.float32)
    info = np.iinfo(dtype)
    return np.clip(np.rint(out), info.min, info.max).astype(dtype)


def error_bound(S, mc, vmax):
    return U * vmax * (8 + S * S + 48 * mc)


def coord_margin(mc):
    return 12 * U * mc


def rows_of(mode, bs, n, count=None, batch_idx=None):
    """per output row: the image it reads, or -1 for a row of zeros"""
    if mode == BATCHED:
        nv = np.full(bs, n) if count is None else np.clip(np.asarray(count, dtype=np.int64), 0, n)
        return [r if j < nv[r] else -1 for r in range(bs) for j in range(n)]
    return [int(b) if 0 <= int(b) < bs else -1 for b in np.asarray(batch_idx)]


def level_of(box, thr):
    """the f32 rule: area = (x2 - x1) * (y2 - y1), level = number of thresholds with area >= thr (a NaN area: 0)"""
    f = np.float32
    with np.errstate(all="ignore"):
        area = f(f(box[2]) - f(box[0])) * f(f(box[3]) - f(box[1]))
        return int(sum(1 for t in thr if area >= f(t)))


def _head(box, s, aligned, ph, pw, ft):
    x1, y1, x2, y2 = (ft(v) for v in box)
    s, o, one = ft(s), ft(0.5 if aligned else 0.0), ft(1.0)
    rsw = x1 * s - o
    rsh = y1 * s - o
    rew = x2 * s - o
    reh = y2 * s - o
    rw = rew - rsw
    rh = reh - rsh
    if not aligned:
        rw = rw if rw > one else one
        rh = rh if rh > one else one
    return rsw, rsh, rw / ft(pw), rh / ft(ph)


def _axis(start, bn, P, S, L, ft):
    """the P * S sample coordinates of one axis: lo, hi, weight of hi, weight of lo, valid, and the raw coordinate"""
    p = np.repeat(np.arange(P), S).astype(ft)
    i = np.tile(np.arange(S), P).astype(ft)
    y = (start + p * bn) + ((i + ft(0.5)) * bn) / ft(S)
    valid = (y >= ft(-1.0)) & (y <= ft(L))
    raw = y
    y = np.where(valid, y, ft(0.0))
    y = np.where(y <= 0, ft(0.0), y)
    yl = y.astype(np.int64)
    top = yl >= L - 1
    yl = np.where(top, L - 1, yl)
    yh = np.where(top, L - 1, yl + 1)
    y = np.where(top, yl.astype(ft), y)
    ly = y - yl.astype(ft)
    hy = ft(1.0) - ly
    return yl, yh, ly.astype(ft), hy.astype(ft), valid, raw


def _one(img, box, s, S, aligned, ph, pw, ft):
    """img {h, w, c} -> ({ph, pw, c} in ft, margin)"""
    H, W, c = img.shape
    rsw, rsh, bw, bh = _head(box, s, aligned, ph, pw, ft)
    yl, yh, ly, hy, yv, yraw = _axis(rsh, bh, ph, S, H, ft)
    xl, xh, lx, hx, xv, xraw = _axis(rsw, bw, pw, S, W, ft)
    v = img.astype(ft)
    w1 = (hy[:, None] * hx[None, :])[:, :, None]
    w2 = (hy[:, None] * lx[None, :])[:, :, None]
    w3 = (ly[:, None] * hx[None, :])[:, :, None]
    w4 = (ly[:, None] * lx[None, :])[:, :, None]
    smp = ((w1 * v[yl][:, xl] + w2 * v[yl][:, xh]) + w3 * v[yh][:, xl]) + w4 * v[yh][:, xh]
    smp = np.where((yv[:, None] & xv[None, :])[:, :, None], smp, ft(0.0)).reshape(ph, S, pw, S, c)
    acc = np.zeros((ph, pw, c), dtype=ft)
    for iy in range(S):
        for ix in range(S):
            acc = acc + smp[:, iy, :, ix, :]
    with np.errstate(invalid="ignore"):
        margin = min(np.nanmin(np.abs(np.concatenate([yraw + 1, yraw - H]).astype(np.float64))) if np.isfinite(yraw).any() else np.inf,
                     np.nanmin(np.abs(np.concatenate([xraw + 1, xraw - W]).astype(np.float64))) if np.isfinite(xraw).any() else np.inf)
    return acc / ft(S * S), margin


def _run(levels, boxes, out_hw, scales, S, aligned, thr, mode, count, batch_idx, ft):
    bs, c = levels[0].shape[0], levels[0].shape[3]
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    n = boxes.shape[0] // bs if mode == BATCHED else boxes.shape[0]
    rows = rows_of(mode, bs, n, count, batch_idx)
    ph, pw = out_hw
    out = np.zeros((len(rows), ph, pw, c), dtype=ft)
    margin = np.inf
    with np.errstate(all="ignore"):
        for r, img in enumerate(rows):
            if img < 0:
                continue
            lv = level_of(boxes[r], thr)
            out[r], m = _one(levels[lv][img], boxes[r], scales[lv], S, aligned, ph, pw, ft)
            margin = min(margin, m)
    return out, margin


def roi_align(levels, boxes, out_hw, scales, S, aligned, thr=(), mode=BATCHED, count=None, batch_idx=None):
    """levels: arrays {bs, h_l, w_l, c} of one dtype (valid channels only); boxes {bs, n, 4} (BATCHED) or {R, 4} (LIST).
    Returns {R, ph, pw, c} of the levels' dtype."""
    out, _ = _run(levels, boxes, out_hw, scales, S, aligned, thr, mode, count, batch_idx, np.float32)
    with np.errstate(invalid="ignore"):
        return to_dtype(out, levels[0].dtype)


def roi_align_f64(levels, boxes, out_hw, scales, S, aligned, thr=(), mode=BATCHED, count=None, batch_idx=None):
    """(float64 {R, ph, pw, c} before any conversion, smallest distance of a sample coordinate from -1 and L)"""
    return _run(levels, boxes, out_hw, scales, S, aligned, thr, mode, count, batch_idx, np.float64)


def _axis_scalar(start, bn, p, i, S, L):
    f = np.float32
    a = f(f(p) * bn)
    b = f(start + a)
    c = f(f(i) + f(0.5))
    d = f(c * bn)
    e = f(d / f(S))
    y = f(b + e)
    if not (y >= f(-1.0) and y <= f(L)):
        return 0, 0, f(0.0), f(0.0), False
    if y <= 0:
        y = f(0.0)
    yl = int(y)
    if yl >= L - 1:
        yh = yl = L - 1
        y = f(yl)
    else:
        yh = yl + 1
    ly = f(y - f(yl))
    hy = f(f(1.0) - ly)
    return yl, yh, ly, hy, True


def roi_align_scalar(levels, boxes, out_hw, scales, S, aligned, thr=(), mode=BATCHED, count=None, batch_idx=None):
    """the definition one element at a time, one np.float32 operation per line"""
    f = np.float32
    bs, c = levels[0].shape[0], levels[0].shape[3]
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    n = boxes.shape[0] // bs if mode == BATCHED else boxes.shape[0]
    rows = rows_of(mode, bs, n, count, batch_idx)
    ph, pw = out_hw
    out = np.zeros((len(rows), ph, pw, c), dtype=np.float32)
    with np.errstate(all="ignore"):
        for r, img in enumerate(rows):
            if img < 0:
                continue
            x1, y1, x2, y2 = (f(v) for v in boxes[r])
            dw = f(x2 - x1)
            dh = f(y2 - y1)
            area = f(dw * dh)
            lv = 0
            for t in thr:
                if area >= f(t):
                    lv += 1
            src = levels[lv][img]
            H, W = src.shape[:2]
            s, o = f(scales[lv]), f(0.5 if aligned else 0.0)
            rsw = f(x1 * s)
            rsw = f(rsw - o)
            rsh = f(y1 * s)
            rsh = f(rsh - o)
            rew = f(x2 * s)
            rew = f(rew - o)
            reh = f(y2 * s)
            reh = f(reh - o)
            rw = f(rew - rsw)
            rh = f(reh - rsh)
            if not aligned:
                rw = rw if rw > f(1.0) else f(1.0)
                rh = rh if rh > f(1.0) else f(1.0)
            bw = f(rw / f(pw))
            bh = f(rh / f(ph))
            for p in range(ph):
                ys = [_axis_scalar(rsh, bh, p, i, S, H) for i in range(S)]
                for q in range(pw):
                    xs = [_axis_scalar(rsw, bw, q, i, S, W) for i in range(S)]
                    for ch in range(c):
                        acc = f(0.0)
                        for yl, yh, ly, hy, yv in ys:
                            for xl, xh, lx, hx, xv in xs:
                                if not (yv and xv):
                                    acc = f(acc + f(0.0))
                                    continue
                                w1 = f(hy * hx)
                                w2 = f(hy * lx)
                                w3 = f(ly * hx)
                                w4 = f(ly * lx)
                                t1 = f(w1 * f(src[yl, xl, ch]))
                                t2 = f(w2 * f(src[yl, xh, ch]))
                                t3 = f(w3 * f(src[yh, xl, ch]))
                                t4 = f(w4 * f(src[yh, xh, ch]))
                                sm = f(t1 + t2)
                                sm = f(sm + t3)
                                sm = f(sm + t4)
                                acc = f(acc + sm)
                        out[r, p, q, ch] = f(acc / f(S * S))
        return to_dtype(out, levels[0].dtype)


def level_mapper_f64(area, k_min, k_max, canonical_scale=224, canonical_level=4, eps=1e-6):
    """torchvision's LevelMapper on an area, in float64: the level's index from k_min"""
    with np.errstate(all="ignore"):
        k = np.floor(canonical_level + np.log2(np.sqrt(np.asarray(area, dtype=np.float64)) / canonical_scale) + eps)
    return (np.clip(k, k_min, k_max) - k_min).astype(np.int64)


# ---- the plan of csrc/roialign_plan.h, restated ------------------------------------------------------------------------------
TILE, GENERIC = 0, 1
THREADS, TABLE, ENTRY_BYTES, SPLIT_TARGET, MAX_GENERIC_GRID = 256, 256, 20, 512, 1 << 20
DT_NAME = {np.dtype(np.uint8): "u8", np.dtype(np.int8): "s8", np.dtype(np.float32): "f32"}


def tile_class(dtype, c, lds):
    es = np.dtype(dtype).itemsize
    return c % (16 // es) == 0 and all(ld * es % 16 == 0 for ld in lds)


def auto_path(dtype, c, lds, rows, ph, pw):
    """DFX_ROIALIGN_AUTO_NOTE: the tile kernel in its class from 256 bytes of channels, 100 RoIs and 49 bins on, the smallest
    of each at which it was measured and won; the generic kernel elsewhere"""
    measured = c * np.dtype(dtype).itemsize >= 256 and rows >= 100 and ph * pw >= 49
    return TILE if tile_class(dtype, c, lds) and measured else GENERIC


def rows_per_group(rows, ph):
    if rows >= SPLIT_TARGET:
        return ph
    splits = min(ph, -(-SPLIT_TARGET // rows))
    return -(-ph // splits)


def grid(path, rows, ph, pw, c):
    if path == TILE:
        return rows * -(-ph // rows_per_group(rows, ph))
    return min(MAX_GENERIC_GRID, -(-rows * ph * pw * c // THREADS))


def lds_bytes(path):
    return 2 * TABLE * ENTRY_BYTES if path == TILE else 0


def algorithmic_bytes(mode, bs, rows, ph, pw, c, S, dtype):
    cb, bins = c * np.dtype(dtype).itemsize, rows * ph * pw
    return rows * 16 + (bs * 4 if mode == BATCHED else rows * 4) + bins * S * S * 4 * cb + bins * cb


def kernel_name(path, dtype, ph, pw, S, levels):
    return "roialign_%s<%s,%dx%d,s%d,l%d>" % ("tile" if path == TILE else "generic", DT_NAME[np.dtype(dtype)], ph, pw, S, levels)
