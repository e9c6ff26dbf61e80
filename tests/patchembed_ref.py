"""Reference, data, plan mirror and case tables of the int8 patch-embedding op's tests (dfx_patchembed_*, include/dfx.h; pure
numpy, needs no GPU).

The arithmetic is dfx_imgconv's / dfx_fc's: one int64 matrix product of the gathered patches with the weights in K order
(ky, kx, i), then refmath's _requant / _store, unchanged, the per-(token, channel) table taking the bias's place.
tests/test_patchembed_cpu.py pins this against an element-by-element witness that indexes the image and the oihw weights
directly, and against linear_ref on the host-gathered patch matrix; tests/test_gpu_patchembed.py compares the GPU against it, bit
for bit, over dst's whole storage.
"""
import functools
from dataclasses import dataclass, replace

import numpy as np

import linear_ref as L
from refmath import _requant, _store

UNDEF, F32, S32, S8, U8 = L.UNDEF, L.F32, L.S32, L.S8, L.U8
NP_OF, NAME_OF, SIZE_OF = L.NP_OF, L.NAME_OF, L.SIZE_OF
TILE, GENERIC = 0, 1            # DFX_PATCHEMBED_TILE / DFX_PATCHEMBED_GENERIC
INVALID, UNSUPPORTED = 1, 2
KMAX, NMAX, MAX_ELEMS, POISON = L.KMAX, L.NMAX, L.MAX_ELEMS, L.POISON
TABLE_MAX_BYTES = 1 << 30
BN, KS, BMS, THREADS = L.BN, L.KS, L.BMS, L.THREADS
up = L.up


@dataclass(frozen=True)
class PeCase:
    name: str
    bs: int
    th: int                       # tokens per axis
    tw: int
    ph: int
    pw: int
    ic: int
    oc: int
    src_dt: int = U8
    dst_dt: int = S8
    bia_dt: int = UNDEF
    relu: bool = False
    rm: int = 0
    per_channel: bool = False
    table: bool = False
    t0: int = 0                   # tok_offset
    slack: int = 0                # img_rows - (t0 + th * tw)
    prefix: bool = False          # prefix rows given (needs t0 > 0)
    dst_ld: int = None            # None: oc
    extra_h: int = 0              # leftover pixel rows below th * ph
    extra_w: int = 0              # leftover pixel columns right of tw * pw
    scale: float = None
    small: bool = False
    saturating: bool = False
    seed: int = 1

    @property
    def ih(self):
        return self.th * self.ph + self.extra_h

    @property
    def iw(self):
        return self.tw * self.pw + self.extra_w

    @property
    def run(self):
        return self.pw * self.ic

    @property
    def k(self):
        return self.ph * self.pw * self.ic

    @property
    def tokens(self):
        return self.th * self.tw

    @property
    def rows(self):
        return self.bs * self.tokens

    @property
    def img_rows(self):
        return self.t0 + self.tokens + self.slack

    @property
    def dld(self):
        return self.oc if self.dst_ld is None else self.dst_ld

    @property
    def does_relu(self):
        return self.relu or self.dst_dt == U8

    @property
    def nscales(self):
        return self.oc if self.per_channel else 1

    @property
    def granule(self):
        return granule(self.pw * self.ic, self.iw * self.ic)

    def ident(self):
        return "%s-b%d-t%dx%d-p%dx%dx%d-oc%d-%s-%s-b%s-r%d-m%d-pc%d-tab%d-t0%d+%d-pre%d-ld%d-x%d,%d" % (
            self.name, self.bs, self.th, self.tw, self.ph, self.pw, self.ic, self.oc, NAME_OF[self.src_dt], NAME_OF[self.dst_dt], NAME_OF[self.bia_dt],
            self.relu, self.rm, self.per_channel, self.table, self.t0, self.slack, self.prefix, self.dld, self.extra_h, self.extra_w)


def lin_case(case):
    """the GEMM the op is, as linear_ref's case: what make_scales, acc_sd and saturated_fraction take"""
    return L.LinCase(case.name, case.rows, case.k, case.oc, src_dt=case.src_dt, dst_dt=case.dst_dt, bia_dt=case.bia_dt, relu=case.relu, rm=case.rm,
                     per_channel=case.per_channel, src_ld=case.k, dst_ld=case.dld, scale=case.scale, small=case.small, saturating=case.saturating,
                     seed=case.seed)


def dst_storage(case):
    """elements of dst's storage: every row of every image, whole"""
    return case.bs * case.img_rows * case.dld


def permute_weights(case, w):
    """oihw {oc, ic, ph, pw} -> {oc, K} with K in the order (ky, kx, i)"""
    return np.ascontiguousarray(w.reshape(case.oc, case.ic, case.ph, case.pw).transpose(0, 2, 3, 1)).reshape(case.oc, case.k)


def gather(case, data):
    """the patch matrix {rows, K} of the src dtype, K in the order (ky, kx, i): what a host would hand dfx_linear"""
    img = data["src"].reshape(case.bs, case.ih, case.iw, case.ic)[:, :case.th * case.ph, :case.tw * case.pw]
    p = img.reshape(case.bs, case.th, case.ph, case.tw, case.pw, case.ic).transpose(0, 1, 3, 2, 4, 5)
    return np.ascontiguousarray(p).reshape(case.rows, case.k)


SAT_CAP = 0.10        # at most this share of a case's outputs on a saturation bound, except in the cases built to saturate


@functools.lru_cache(maxsize=None)
def generate(case):
    """_generate(case) at the case's seed.  The next seed is drawn where a ReLU leaves a case of a few outputs all zero and
    where a case of a few channels lands beyond the saturation cap: a u8 image against a weight row whose sum is far from 0
    shifts that whole channel by up to two of the output's standard deviations, which one channel in 1, 3 or 4 does not
    average out.  redraws(case) tells how often that happened (tests/test_patchembed_cpu.py bounds it)."""
    return _draw(case)[0]


@functools.lru_cache(maxsize=None)
def _draw(case):
    for attempt in range(16):
        out = _generate(case, case.seed + 7919 * attempt)
        if case.saturating:
            break
        v = values(case, out)
        if v.view(np.uint8).any() and saturated_fraction(case, v) <= SAT_CAP:
            break
    return out, attempt


def redraws(case):
    return _draw(case)[1]


def _generate(case, seed):
    """-> dict(src {bs, ih, iw, ic} of the src dtype, w oihw int8, bia, table, scales, prefix).  Valid pixels are uniform over
    the whole dtype (small: 0 .. 3 against -3 .. 3); the leftover pixels below th * ph and right of tw * pw hold 0xFF.  Scales
    come from linear_ref.make_scales (a 1-byte output of sd about 40); bias / table are normal with sd acc_sd / 3 (small: the
    table holds -3 .. 3)."""
    rng = np.random.default_rng(seed)
    lc = lin_case(case)
    raw = np.full((case.bs, case.ih, case.iw, case.ic), 0xFF, dtype=np.uint8)
    vh, vw = case.th * case.ph, case.tw * case.pw
    if case.small:
        raw[:, :vh, :vw] = rng.integers(0, 4, (case.bs, vh, vw, case.ic)).astype(np.uint8)
        w = rng.integers(-3, 4, (case.oc, case.k)).astype(np.int8)
    else:
        raw[:, :vh, :vw] = rng.integers(0, 256, (case.bs, vh, vw, case.ic)).astype(np.uint8)
        w = rng.integers(-128, 128, (case.oc, case.k)).astype(np.int8)
    if case.does_relu and case.src_dt == U8 and not case.small:
        # linear_ref's rule: a u8 src against a weight row of negative sum leaves little but the ReLU's zeros
        wv = w.astype(np.int16)
        flip = wv.sum(axis=1, keepdims=True) <= 0
        flip[1::2] = False
        wv = np.where(flip, np.clip(-wv, -127, 127), wv)
        wv[:, 0] = np.where(flip[:, 0] & (wv.sum(axis=1) <= 0), 1, wv[:, 0])
        w = wv.astype(np.int8)
    out = dict(src=raw.view(NP_OF[case.src_dt]), w=w.reshape(case.oc, case.ic, case.ph, case.pw), bia=None, table=None, scales=L.make_scales(lc), prefix=None)
    if case.table:
        amp = max(1.0, L.acc_sd(lc) / 3.0)
        out["table"] = (rng.integers(-3, 4, (case.tokens, case.oc)) if case.small else rng.standard_normal((case.tokens, case.oc)) * amp).astype(np.float32)
    else:
        out["bia"] = L.make_bias(lc, rng)
    if case.prefix:
        out["prefix"] = rng.integers(0, 256, case.t0 * case.oc * SIZE_OF[case.dst_dt]).astype(np.uint8).view(NP_OF[case.dst_dt]).reshape(case.t0, case.oc)
    return out


def accumulate(case, data):
    """exact int64 accumulators {rows, oc}"""
    return gather(case, data).astype(np.int64) @ permute_weights(case, data["w"]).astype(np.int64).T


def values(case, data):
    """the tokens, {bs, tokens, oc} of dst's dtype"""
    acc = accumulate(case, data).reshape(case.bs, case.tokens, case.oc)
    add = data["table"] if case.table else data["bia"]
    with np.errstate(invalid="ignore", over="ignore"):
        f = _requant(acc, add, data["scales"], case.does_relu)
        return _store(f, case.dst_dt, case.rm)


def _blank(case):
    return np.full(dst_storage(case), POISON, dtype=np.uint8).repeat(SIZE_OF[case.dst_dt]).view(NP_OF[case.dst_dt]).reshape(case.bs, case.img_rows, case.dld)


def reference(case, data):
    """dst's whole storage {bs * img_rows, dld} as bytes: POISON everywhere but the tokens and, where given, the prefix rows"""
    out = _blank(case)
    out[:, case.t0:case.t0 + case.tokens, :case.oc] = values(case, data)
    if data["prefix"] is not None:
        out[:, :case.t0, :case.oc] = data["prefix"][None]
    return out.reshape(-1).view(np.uint8)


def add_f32(case, data, t, o):
    if case.table:
        return np.float32(data["table"][t, o])
    return None if data["bia"] is None else L.bias_f32(lin_case(case), data["bia"], o)


def witness(case, data):
    """the same storage, element by element on Python ints and np.float32 scalars, indexing the image and the oihw weights"""
    src = data["src"].reshape(case.bs, case.ih, case.iw, case.ic)
    w, scales = data["w"], data["scales"]
    out = _blank(case)
    for b in range(case.bs):
        for ty in range(case.th):
            for tx in range(case.tw):
                t = ty * case.tw + tx
                patch = src[b, ty * case.ph:(ty + 1) * case.ph, tx * case.pw:(tx + 1) * case.pw].astype(np.int64)   # {ph, pw, ic}
                for o in range(case.oc):
                    acc = int((patch * w[o].astype(np.int64).transpose(1, 2, 0)).sum())
                    with np.errstate(invalid="ignore", over="ignore"):
                        f = np.float32(acc)
                        a = add_f32(case, data, t, o)
                        if a is not None:
                            f = np.float32(f + a)
                        f = np.float32(f * np.float32(scales[o if len(scales) > 1 else 0]))
                    if case.does_relu and np.float32(0) > f:
                        f = np.float32(0)
                    if case.dst_dt == F32:
                        v = f
                    else:
                        if not (f >= np.float32(-2147483648.0) and f < np.float32(2147483648.0)):
                            v = -2147483648
                        else:
                            v = int(np.floor(f)) if case.rm == 1 else int(np.rint(f))
                        if case.dst_dt == S8:
                            v = max(-128, min(127, v))
                        elif case.dst_dt == U8:
                            v = 255 if (v < 0 or v > 255) else v
                    out[b, case.t0 + t, o] = v
        if data["prefix"] is not None:
            for r in range(case.t0):
                for o in range(case.oc):
                    out[b, r, o] = data["prefix"][r, o]
    return out.reshape(-1).view(np.uint8)


def saturated_fraction(case, vals):
    return L.saturated_fraction(lin_case(case), vals)


# --- the plan of patchembed_plan.h and the image of patchembed_pack.h, mirrored ------------------------------------------------
def desc_of(case, force_path=-1):
    """the dict of dfx_patchembed_desc's fields of a case"""
    return dict(bs=case.bs, ih=case.ih, iw=case.iw, ic=case.ic, ph=case.ph, pw=case.pw, th=case.th, tw=case.tw, oc=case.oc, src_dt=case.src_dt,
                dst_dt=case.dst_dt, bia_dt=case.bia_dt, relu=int(case.relu), round_mode=case.rm, nscales=case.nscales, table=int(case.table),
                tok_offset=case.t0, force_path=force_path, img_rows=case.img_rows, dst_ld=case.dld)


def granule(run, row):
    if run % 16 == 0 and row % 16 == 0:
        return 16
    if run % 4 == 0 and row % 4 == 0:
        return 4
    return 0


def desc_granule(d):
    return granule(d["pw"] * d["ic"], d["iw"] * d["ic"])


def table_ld(oc):
    return up(oc, 4)


def validate(d):
    """0, INVALID or UNSUPPORTED for a descriptor given as a dict of dfx_patchembed_desc's fields, in the header's order"""
    if min(d["bs"], d["ih"], d["iw"], d["ic"]) < 1 or not 1 <= d["ph"] <= 255 or not 1 <= d["pw"] <= 255:
        return INVALID
    if not 1 <= d["th"] <= d["ih"] // d["ph"] or not 1 <= d["tw"] <= d["iw"] // d["pw"]:
        return INVALID
    if d["ph"] * d["pw"] * d["ic"] > KMAX or not 1 <= d["oc"] <= NMAX:
        return INVALID
    if d["src_dt"] not in (U8, S8) or d["dst_dt"] not in NP_OF or (d["bia_dt"] != UNDEF and d["bia_dt"] not in NP_OF):
        return INVALID
    if d["round_mode"] not in (0, 1) or d["nscales"] not in (1, d["oc"]) or d["table"] not in (0, 1) or (d["table"] and d["bia_dt"] != UNDEF):
        return INVALID
    if d["tok_offset"] < 0 or d["force_path"] not in (-1, TILE, GENERIC):
        return INVALID
    if d["img_rows"] < d["tok_offset"] + d["th"] * d["tw"] or d["dst_ld"] < d["oc"]:
        return INVALID
    if d["bs"] * d["ih"] * d["iw"] * d["ic"] > MAX_ELEMS or d["ph"] * d["iw"] * d["ic"] >= 2 ** 31 or d["bs"] * d["img_rows"] * d["dst_ld"] > MAX_ELEMS:
        return INVALID
    if d["table"] and d["th"] * d["tw"] * table_ld(d["oc"]) * 4 > TABLE_MAX_BYTES:
        return INVALID
    if d["force_path"] == TILE and not desc_granule(d):
        return UNSUPPORTED
    return 0


AUTO_MIN_ROWS, AUTO_MIN_OC, AUTO_MIN_K, AUTO_MIN_MACS = 49, 96, 48, 3136 * 96 * 48


def auto_path(d):
    """the AUTO RULE of include/dfx.h (DFX_PATCHEMBED_AUTO_NOTE): the tile kernel in its class from the smallest rows, oc, K and
    multiply-adds at which it was measured and beat the generic kernel and dfx_imgconv; generic everywhere else"""
    if d["force_path"] != -1:
        return d["force_path"]
    rows, k = d["bs"] * d["th"] * d["tw"], d["ph"] * d["pw"] * d["ic"]
    big = rows >= AUTO_MIN_ROWS and d["oc"] >= AUTO_MIN_OC and k >= AUTO_MIN_K and rows * d["oc"] * k >= AUTO_MIN_MACS
    return TILE if big and desc_granule(d) else GENERIC


def gemm_desc(d):
    """linear_ref's descriptor dict of the GEMM the op is (patchembed_plan.h's pe_gemm)"""
    k = d["ph"] * d["pw"] * d["ic"]
    return dict(rows=d["bs"] * d["th"] * d["tw"], k=k, n=d["oc"], src_dt=d["src_dt"], dst_dt=d["dst_dt"], bia_dt=d["bia_dt"], relu=d["relu"],
                round_mode=d["round_mode"], nscales=d["nscales"], lut_in_dt=UNDEF, force_path=d["force_path"], src_ld=k, dst_ld=d["dst_ld"])


def planned_bm(d, cus, forced=0):
    return L.planned_bm(gemm_desc(d), cus, forced)


def tiles(d, bm):
    return L.tiles(gemm_desc(d), bm)


def planned_grid(d, path, bm, cus, cap=0):
    return L.planned_grid(gemm_desc(d), path, bm, cus, cap)


def lds_bytes(path, bm):
    return L.lds_bytes(L.TILE, bm) - 256 if path == TILE else 0


def ktab(d):
    """the K offset table: per granule g of K, (g G // L) * iw * ic + (g G % L); entries at or beyond K are 0"""
    g = desc_granule(d)
    if not g:
        return np.zeros(0, dtype=np.int32)
    run, k, row = d["pw"] * d["ic"], d["ph"] * d["pw"] * d["ic"], d["iw"] * d["ic"]
    c = np.arange(L.nslabs(k) * (KS // g), dtype=np.int64) * g
    return np.where(c < k, (c // run) * row + c % run, 0).astype(np.int32)


def image_offsets(d):
    """(off_comp, off_bias, off_scale, off_ktab, off_table, off_prefix, bytes) of the device image"""
    k = d["ph"] * d["pw"] * d["ic"]
    oc_, ob, os_, ot, _ = L.image_offsets(d["oc"], k)
    off_table = ot + up(ktab(d).size * 4, 16)
    off_prefix = off_table + (d["th"] * d["tw"] * table_ld(d["oc"]) * 4 if d["table"] else 0)
    return oc_, ob, os_, ot, off_table, off_prefix, max(16, off_prefix + up(d["tok_offset"] * d["oc"] * SIZE_OF[d["dst_dt"]], 16))


def fast_ok(case, data):
    """the fast route's proof: linear_pack.h's with max_t |table[t][o]| in the place of |bias[o]|"""
    if case.rm != 0:
        return False
    w = permute_weights(case, data["w"]).astype(np.int64)
    pos, neg = np.where(w > 0, w, 0).sum(axis=1), -np.where(w < 0, w, 0).sum(axis=1)
    bound = 255.0 * np.maximum(pos, neg) if case.src_dt == U8 else 128.0 * (pos + neg)
    for o in range(case.oc):
        if case.table:
            b = float(np.abs(data["table"][:, o]).max())
        else:
            b = 0.0 if data["bia"] is None else float(L.bias_f32(lin_case(case), data["bia"], o))
        s = float(data["scales"][o if case.per_channel else 0])
        if not (np.isfinite(b) and np.isfinite(s)) or (float(bound[o]) + abs(b)) * abs(s) > 2.0 ** 30:
            return False
    return True


def kernel_name(case, path, bm, route):
    tab = " +table" if case.table else ""
    if path == TILE:
        return "patchembed_tile<%s,%s,bm%d,g%d> %s%s" % (NAME_OF[case.src_dt], NAME_OF[case.dst_dt], bm, case.granule, "fast" if route else "exact", tab)
    return "patchembed_generic<%s,%s>%s" % (NAME_OF[case.src_dt], NAME_OF[case.dst_dt], tab)


def algorithmic_ops(d):
    return 2 * d["bs"] * d["th"] * d["tw"] * d["oc"] * d["ph"] * d["pw"] * d["ic"]


def algorithmic_bytes(d, prefix):
    k, rows, esz = d["ph"] * d["pw"] * d["ic"], d["bs"] * d["th"] * d["tw"], SIZE_OF[d["dst_dt"]]
    add = 4 * d["th"] * d["tw"] * d["oc"] if d["table"] else 4 * d["oc"] if d["bia_dt"] != UNDEF else 0
    return rows * k + d["oc"] * k + rows * d["oc"] * esz + add + 4 * d["nscales"] + (d["bs"] * d["tok_offset"] * d["oc"] * esz if prefix else 0)


# --- case tables ---------------------------------------------------------------------------------------------------------------
# (ph, pw, ic): L 48 (a slab holds 1 1/3 runs); L 12, G 4, K 48 below one slab; L 16; L 64; L 80 with a K tail in the last slab;
# L 192; 255 runs of 16
GEOMETRIES = ((16, 16, 3), (4, 4, 3), (1, 4, 4), (2, 2, 32), (3, 5, 16), (2, 2, 96), (255, 1, 16))
OCS = (1, 3, 4, BN - 1, BN, BN + 1, 2 * BN + 8)


def token_counts(bm):
    return (1, bm - 1, bm, bm + 1, 2 * bm + 2)


def split_tokens(total):
    """(bs, th, tw) with bs * th * tw == total, bs the largest of 3, 2, 1 that divides it: tiles straddle image and patch-row
    boundaries wherever the count allows"""
    bs = next(b for b in (3, 2, 1) if total % b == 0)
    t = total // bs
    th = max(v for v in range(1, int(t ** 0.5) + 1) if t % v == 0)
    return bs, th, t // th


def _dst_ld(n, which):
    """0: dense; 1: a multiple of 4 above n (vector stores wherever n allows); 2: odd and above n (element stores)"""
    return (n, up(n, 4) + 4, (n + 3) | 1)[which]


@functools.lru_cache(maxsize=None)
def shape_grid(bm, src_dt):
    """A pairwise cover of tokens-in-all x oc x geometry: every pair of two axes occurs, the third rotating.  dst dtype, dst's
    pitch, ReLU, round mode, per-channel scales, tok_offset, img_rows slack, table / bias / none and prefix given / not rotate
    through the cases (tests/test_patchembed_cpu.py asserts the cover)."""
    rs = token_counts(bm)
    triples = [(i, j, (i + 2 * j) % 7) for i in range(5) for j in range(7)]
    triples += [(i, (i + g) % 7, g) for i in range(5) for g in range(7)]
    triples += [((j + g) % 5, j, g) for j in range(7) for g in range(7)]
    seen, out = set(), []
    for t in triples:
        if t in seen:
            continue
        seen.add(t)
        x = len(out)
        i, j, g = t
        bs, th, tw = split_tokens(rs[i])
        ph, pw, ic = GEOMETRIES[g]
        oc = OCS[j]
        t0 = x % 3
        add = x % 3                                     # 0 table, 1 vector bias, 2 none
        out.append(PeCase("grid", bs, th, tw, ph, pw, ic, oc, src_dt=src_dt, dst_dt=(S8, U8, S32, F32)[(i + j + g) % 4],
                          bia_dt=(S32, F32, S8, U8)[(x // 3) % 4] if add == 1 else UNDEF, relu=bool((i + g) % 2), rm=(j + g) % 2,
                          per_channel=bool((i + j) % 2), table=add == 0, t0=t0, slack=(x // 2) % 3, prefix=bool(t0) and bool((x // 3) % 2),
                          dst_ld=_dst_ld(oc, (i + 2 * j + g) % 3), seed=1000 * bm + 100 * src_dt + x))
    return tuple(out)


def compensation_cases():
    """K = 65025 (255 x 255 x 1, outside the tile class) and K = 65024 (127 x 128 x 4, the deepest K inside it): a u8 token of all
    255 and one of all 0 against a weight row of all -128 and one of all 127; s32 out, scale 1"""
    out = []
    for ph, pw, ic in ((255, 255, 1), (127, 128, 4)):
        case = PeCase("comp", 2, 1, 1, ph, pw, ic, 2, src_dt=U8, dst_dt=S32, scale=1.0, seed=20000 + ic)
        raw = np.full((2, case.ih, case.iw, case.ic), 0xFF, dtype=np.uint8)
        raw[1] = 0
        w = np.empty((2, ic, ph, pw), dtype=np.int8)
        w[0], w[1] = -128, 127
        out.append((case, dict(src=raw, w=w, bia=None, table=None, scales=np.ones(1, dtype=np.float32), prefix=None)))
    return out


def lane_map_cases(bm):
    """s32 out, scale 1, weights and pixels with a distinct residue per (o, k) and per pixel byte: a swapped (ky, kx, i) order or
    a shifted run shows in every element.  One case per granule."""
    out = []
    for ph, pw, ic in ((3, 16, 3), (4, 4, 3)):
        bs, th, tw = 2, 3, (bm + 3) // 3
        case = PeCase("lanes%d" % bm, bs, th, tw, ph, pw, ic, BN + 8, src_dt=S8, dst_dt=S32, scale=1.0, seed=21000 + bm + ic)
        n = case.bs * case.ih * case.iw * case.ic
        src = ((np.arange(n, dtype=np.int64) * 37 + (np.arange(n, dtype=np.int64) // 251) * 11) % 251 - 125).astype(np.int8).reshape(bs, case.ih, case.iw, ic)
        o, c = np.arange(case.oc).reshape(-1, 1), np.arange(case.k).reshape(1, -1)
        wk = ((o * 7 + c * 13 + (o * c) % 5) % 251 - 125).astype(np.int8)      # {oc, K} in oihw order of K: (i, ky, kx)
        out.append((case, dict(src=src, w=wk.reshape(case.oc, ic, ph, pw), bia=None, table=None, scales=np.ones(1, dtype=np.float32), prefix=None)))
    return out


def leftover_cases():
    """th, tw below the floor: the unread pixels hold 0xFF; iw * ic stays in the class (G 16 and G 4)"""
    return [PeCase("leftover", 2, 3, 5, 4, 4, 4, 40, extra_h=3, extra_w=4, table=True, seed=22000),
            PeCase("leftover", 2, 3, 5, 4, 4, 4, 40, src_dt=S8, dst_dt=U8, extra_h=9, extra_w=8, bia_dt=S32, seed=22001),
            PeCase("leftover", 3, 2, 7, 4, 4, 3, 33, dst_dt=F32, extra_h=1, extra_w=4, table=True, t0=1, prefix=True, seed=22002),
            PeCase("leftover", 1, 5, 4, 2, 2, 32, 130, src_dt=S8, extra_h=2, extra_w=3, seed=22003)]


def imgconv_twin_cases():
    """no table, no prefix, t0 = 0, dst_ld = oc, u8 src, ic <= 4: equal to dfa.ImageConv with k = s and pad 0"""
    return [PeCase("imgtwin", 2, 3, 4, ph, pw, ic, oc, dst_dt=dst, bia_dt=(UNDEF, S32)[i % 2], relu=bool(i % 2), rm=i // 2 % 2, per_channel=bool(i % 3 == 0),
                   seed=23000 + i)
            for i, (ph, pw, ic, oc, dst) in enumerate(((16, 16, 3, 40, U8), (4, 4, 3, 96, S8), (1, 4, 4, 17, S32), (4, 4, 4, 33, F32), (7, 7, 3, 20, S8)))]


def linear_twin_cases():
    """any ic and either dtype: equal to dfa.Linear (generic path) on the patch matrix gathered on the host"""
    return [PeCase("lintwin", 2, 3, 5, ph, pw, ic, oc, src_dt=(U8, S8)[i % 2], dst_dt=dst, bia_dt=(S32, UNDEF, F32)[i % 3], relu=bool(i % 2), rm=i % 2,
                   per_channel=bool(i % 2), dst_ld=_dst_ld(oc, i % 3), seed=24000 + i)
            for i, (ph, pw, ic, oc, dst) in enumerate(((2, 2, 32, 70, S8), (3, 5, 16, 133, U8), (2, 2, 96, 64, S32), (14, 14, 3, 50, F32), (4, 4, 3, 96, S8)))]


def table_cases():
    """tables with every dst dtype, both src dtypes, per-channel scales, pitched dst"""
    return [PeCase("table", 2, 4, 9, 4, 4, 4, 133, src_dt=(U8, S8)[i % 2], dst_dt=dst, table=True, per_channel=bool(i % 2), relu=bool(i // 2),
                   t0=i % 3, prefix=bool(i % 3), dst_ld=_dst_ld(133, i % 3), seed=25000 + i) for i, dst in enumerate((S8, U8, S32, F32))]


def tie_cases():
    """small integers at scale 0.5 with a table of small integers: every odd sum is a tie, in both round modes"""
    return [PeCase("ties", 2, 3, 11, 2, 2, 4, 40, src_dt=(U8, S8)[i % 2], dst_dt=(S8, U8)[i // 2], rm=rm, scale=0.5, small=True, table=True,
                   seed=26000 + i + 10 * rm) for i in range(4) for rm in (0, 1)]


def nonfinite_cases():
    """scales of inf and NaN (the exact route only: set_weights must refuse to call them fast); built to saturate"""
    return [PeCase("nonfinite", 1, 3, 11, 2, 2, 4, 34, src_dt=(U8, S8)[i % 2], dst_dt=dst, scale=scale, table=bool(i % 2), saturating=True, seed=27000 + i)
            for scale in (float("inf"), float("nan")) for i, dst in enumerate((U8, S8, S32, F32))]


def prefix_cases():
    """t0 of 1, 2 and 5 with and without the rows given, every dst dtype, slack rows behind the tokens"""
    return [PeCase("prefix", 3, 2, 5, 4, 4, 3, oc, dst_dt=dst, t0=t0, slack=i % 2, prefix=given, table=bool(i % 2), dst_ld=_dst_ld(oc, i % 3), seed=28000 + i)
            for i, (t0, oc, dst, given) in enumerate(((1, 40, S8, True), (2, 33, U8, True), (5, 129, S32, True), (1, 7, F32, True), (2, 40, S8, False),
                                                      (1, 33, F32, False)))]


GRID_CAP_CASE = PeCase("gridcap", 3, 5, 13, 4, 4, 4, 2 * BN + 8, dst_dt=S8, table=True, t0=1, prefix=True, seed=29000)   # 195 tokens: 4 x 3 tiles of 64
MISALIGNED_CASES = (PeCase("misaligned", 2, 3, 5, 4, 4, 4, 64, bia_dt=S32, seed=30000), PeCase("misaligned", 2, 3, 5, 4, 4, 3, 40, src_dt=S8, dst_dt=F32, seed=30001))
ERROR_CASES = (PeCase("errors", 2, 3, 5, 4, 4, 4, 48, dst_dt=F32, seed=31000), PeCase("errors", 2, 3, 5, 4, 4, 4, 48, table=True, t0=1, seed=31001))
THREADS_CASE = PeCase("threads", 3, 5, 10, 4, 4, 4, 140, table=True, t0=1, prefix=True, seed=32000)
ORDER_CASE = PeCase("order", 2, 3, 7, 4, 4, 4, 70, table=True, per_channel=True, seed=33000)
HOST_CASE = PeCase("host", 2, 3, 5, 4, 4, 3, 50, dst_dt=S32, bia_dt=S8, per_channel=True, seed=34000)
FRONT_CASE = PeCase("front", 2, 8, 8, 4, 4, 3, 64, dst_dt=S8, table=True, t0=1, prefix=True, seed=35000)     # bs 2, 32 x 32 x 3, 4 x 4 patches, oc 64
CXX_CASE = PeCase("cxx", 4, 4, 4, 4, 4, 3, 96, dst_dt=S8, table=True, t0=1, prefix=True, seed=36000)
AUTO_POINT_CASE = PeCase("auto-swin", 1, 56, 56, 4, 4, 3, 96, dst_dt=S8, table=True, seed=37000)     # the smallest measured point: the Swin-T stem at bs 1


def generated_cases():
    """every case whose data comes from generate(): what test_patchembed_cpu holds to the regime condition"""
    out = []
    for bm in BMS:
        for src_dt in (U8, S8):
            out += list(shape_grid(bm, src_dt))
    return out + leftover_cases() + imgconv_twin_cases() + linear_twin_cases() + table_cases() + tie_cases() + nonfinite_cases() + prefix_cases() + \
        [GRID_CAP_CASE, THREADS_CASE, ORDER_CASE, HOST_CASE, FRONT_CASE, CXX_CASE, AUTO_POINT_CASE] + list(MISALIGNED_CASES + ERROR_CASES)


def with_case(case, **kw):
    return replace(case, **kw)
