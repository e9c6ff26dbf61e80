"""Layouts and case tables of the far-offset tests (pure numpy, needs no GPU): the ops that promise 64-bit offsets in
include/dfx.h, run once with ONE operand whose rows or matrices lie more than 2^31 and more than 2^32 bytes behind its base.
tests/test_far_offsets_cpu.py checks the tables (the tests of the tests); tests/test_gpu_far_offsets.py runs them.

The arena.  One uint8 device tensor of ARENA = 2^31 + 2^32 + 2^26 bytes.  The far operand's base is arena + BASE (2^31); every
other operand of a case is small, dense and in a buffer of its own.  The far reach comes from a pitch or a stride: three rows
of 64 bytes that are 2^31 + 64 bytes apart reach past 2^32 and touch under a kilobyte.  A 32-bit slip turns a true byte offset
`off` into `off mod 2^32` (truncated) or, from 2^31 on, into `off - 2^32` (taken as a signed 32-bit value); both are what
aliases() returns.  With every true offset below 2^32 + 2^26 all of them land inside the arena, so that a slip shows as wrong
values (a wrapped read sees poison) or as damaged poison (a wrapped write), never as an access outside the allocation.

Two layouts per far operand:
  H  the last row / matrix starts in [2^31, 2^31 + 2^26): a signed 32-bit offset goes wrong, an unsigned one is still right;
  F  the last row / matrix starts in [2^32, 2^32 + 2^26): a truncated offset goes wrong.  Three rows of a pitch near 2^31 put
     the middle row into [2^31, 2^32): the arena's front 2 GiB covers its signed alias.
Both with 1-byte elements and, where the operand can be s32 / f32, with 4-byte elements: the element index then stays below
2^31 and only the byte offset overflows.

A far operand is a set of SEGMENTS of one length (Far): for an output the valid elements of a row, for an input what the
kernels may read of a row (the valid columns rounded up to 16 bytes within the pitch, as the dense suites lay their storage
out).  The data comes from the op's own generator on a DENSE TWIN of the case (the same sizes, small pitches); the reference is
the twin's, from the op's *_ref module; only the placement differs.

What is covered (op, forced kernels, far operand, layouts):

  op      kernels                                   far operand (what carries the reach)              layouts
  linear  tile bm64 + bm128 (fast, exact), generic  src (src_ld)                                      H, F  1-byte
                                                    dst (dst_ld) u8; f32 / s32                        H, F  1- and 4-byte
          shapes: rows 3, k 72, n 136; and rows BM + 2 with a pitch near 2^31 / (BM + 1) and 2^32 / (BM + 1), BM 64 and 128:
          the far rows sit in the second m-tile
  patch-  tile bm64 + bm128 (fast, exact), generic  dst (dst_ld) s8; f32 / s32: 1 image of 3 tokens           H, F  1- and 4-byte
  embed                                             dst (img_rows) s8; f32 / s32: 3 images of 4 tokens, rows
                                                    64 apart, with and without prefix rows            H, F  1- and 4-byte
                                                    src (bs 130 | 258): images of 2^24 bytes, 2048 x 2048 x 4
                                                    (granule 16) and 4096 x 4096 x 1 (granule 4); th = tw = 2,
                                                    ph = pw = 4: only each image's top-left 8 x 8 pixels
                                                    are read and placed                               H, F  1-byte
  bmm     MFMA (fast, exact), generic               A: a_s0 | a_s1 | lda                              H, F  1-byte
                                                    B: b_s0 | b_s1 | ldb, trans_b 1 and 0             H, F  1-byte
                                                    C: c_s0 | c_s1 | ldc, u8 and s32                  H, F  1- and 4-byte
          matrices 33 x 37 x 40; the dimension that counts the far operand's rows is 3 where ld carries the reach
  attn    fused (proved routes, exact), chain       Q, K, V: each of s0 | s1 | ld                     H, F  1-byte
                                                    O: o_s0 | o_s1 | ldo, s8 and f32                  H, F  1- and 4-byte
          tq 33, tk 37, d 40, dv 35, leading dimensions rounded up to 16: in the fused kernel's class; tq or tk is 3 where ld
          carries the reach
  lnorm   row (w4: c 40, w32: c 300), generic       src (src_ld)                                      H, F  1-byte
                                                    dst (dst_ld) s8; f32                              H, F  1- and 4-byte
          int32_t pitches: F takes 5 rows of a pitch near 2^30 (1-byte) or 3 rows of dst_ld near 2^29 (f32)
  head    row, generic                              src (src_ld) s8 / u8; f32                         H, F  1- and 4-byte
                                                    idx (idx_ld): top-1 u8, top-5 s32; with val far as
                                                    well (u8; f32), behind idx's extent               H     1- and 4-byte
                                                    idx (idx_ld): top-1 u8, top-5 s32, without val    F     1- and 4-byte
                                                    val (idx_ld): top-5 f32 val, its u8 idx at the
                                                    arena's start                                     F     4-byte
                                                    softmax dst (dst_ld) u8; f32                      H, F  1- and 4-byte
          c 21 and 1000, rows 3 or 5 (int32_t pitches)
  head    pixel, generic (on the same data)         argmax u8 over 2^32 / 160 + 1000 rows: src dense at src_ld 160, c 150
                                                    (src far, idx and val small); c = src_ld = 16 and idx_ld
                                                    160 (idx far, without val)                             F     1-byte
          dense: row i is row (i + i // 4096) % 4096 of a random block (PixelFar, pixel_map)
  wsum    vec (H, F), generic (H)                   one u8 tensor, in place (dst is the input), bs 130 | 258
                                                    images of 2^24 bytes; a table on two of the runs        H, F  1-byte
          dense: image b is image 0 rolled by b pixels (WsumFar), so numpy sees one image
  and the overlap checks of linear, bmm, attention and lnorm with dst inside and just behind a far src / A / Q (OVERLAP_CASES).

Left out, with the reason:
  * a 1-byte val beyond 2^32, and val next to an idx that reaches beyond 2^32 (the pixel kernel's dense idx among them):
    idx and val share idx_ld, and dfx_head_submit refuses outputs whose extents overlap, so val cannot lie between idx's rows;
    two extents of 2^32 bytes do not fit the arena.  What fits is run: idx and val both beyond 2^31 (layout H, 1- and 4-byte),
    and an f32 val beyond 2^32 next to a u8 idx of a quarter of its extent (far_second).
  * wsum's generic kernel in layout F: one thread per element over 258 images of 2^24 bytes is several times the time of any
    other case; it runs in layout H (130 images), the vec kernel in both.
  * patchembed's per-token table (the cases carry a bias) and a far table or prefix: those are small images of the handle.
  * In patchembed's far src of layout F an image is exactly 2^24 bytes, so a truncated offset of image 256 + i meets image i,
    not poison: the data of the two differ, and the CPU test shows that the result does (poisoned_values).
  * select, nms, roialign, resize, reorder, se and the conv family: their per-image limits sit below 2^31 or they have a
    4 GiB rule of their own.
  * byte offsets beyond 2^32 + 2^26 up to the documented 2^40 elements: they would need the memory itself.
"""
import functools
from dataclasses import dataclass, replace

import numpy as np

import attn_ref as A
import bmm_ref as B
import head_ref as H
import linear_ref as R
import lnorm_ref as L
import patchembed_ref as P
import wsum_ref as W

P31, P32, WIN = 1 << 31, 1 << 32, 1 << 26
BASE = P31
ARENA = P31 + P32 + WIN
POISON = 0xCD                   # hipref.POISON_BYTE


def aliases(off):
    """what a 32-bit slip makes of byte offsets `off` (int64 array): (itself, truncated, taken as signed 32-bit)"""
    off = np.asarray(off, dtype=np.int64)
    return off, off % P32, (off + P31) % P32 - P31


def in_window(layout, off):
    lo = P31 if layout == "H" else P32
    return lo <= off < lo + WIN


@dataclass(frozen=True)
class Far:
    """the far operand's geometry: segment s holds `width` elements of `esz` bytes from element starts[s] of the operand"""
    esz: int
    starts: tuple
    width: int
    base: int = 0                # bytes from the arena's far base to this operand's pointer (a second far operand: VAL_BASE)

    def byte_starts(self):
        return np.asarray(self.starts, dtype=np.int64) * self.esz

    def byte_offsets(self):
        """every byte offset of the operand that a correct kernel touches, int64 {segments, width * esz}"""
        return self.byte_starts().reshape(-1, 1) + np.arange(self.width * self.esz, dtype=np.int64).reshape(1, -1)

    def arena_offsets(self):
        """byte_offsets() counted from the arena's far base"""
        return self.base + self.byte_offsets()

    def far_segments(self):
        """the segments a signed or a truncated offset gets wrong: those from 2^31 bytes on"""
        return np.flatnonzero(self.byte_starts() >= P31)


@dataclass(frozen=True)
class FarCase:
    op: str                      # "linear" | "patchembed" | "bmm" | "attn" | "lnorm" | "head"
    name: str
    layout: str                  # "H" | "F"
    operand: str                 # linear / lnorm: "src" | "dst";  bmm: "a" | "b" | "c";  attn: "q" | "k" | "v" | "o";  head: "src" | "idx" | "val" | "dst"
    twin: object                 # the dense case of the op's *_ref module: data and reference come from it
    case: object                 # the same case with the far pitch / stride: the descriptor comes from it
    bms: tuple = R.BMS           # linear: the tile heights to force
    pitch: int = 0               # head, operand "idx": idx_ld (the case class has no field for it)

    @property
    def is_input(self):
        return self.operand in ("src", "a", "b", "q", "k", "v")

    def ident(self):
        return "%s-%s-%s-%s" % (self.op, self.name, self.operand, self.layout)


# pitches in BYTES whose second multiple lands in the window (three rows / matrices), multiples of 64
PITCH3 = {"H": (1 << 30) + 4160, "F": P31 + 4160}


def pitch_for(layout, steps):
    """the smallest multiple of 64 bytes that puts row `steps` into the layout's window"""
    lo = P31 if layout == "H" else P32
    return -(-(-(-lo // steps)) // 64) * 64


# ---- linear ---------------------------------------------------------------------------------------------------------------------
def _linear_cases():
    out = []
    seed = 41000
    for layout in ("H", "F"):
        for shape, rows, bms in (("rows3", 3, R.BMS), ("tile64", 64 + 2, (64,)), ("tile128", 128 + 2, (128,))):
            pitch = PITCH3[layout] if rows == 3 else pitch_for(layout, rows - 1)
            for operand, dst_dt in (("src", R.S8), ("dst", R.U8), ("dst", (R.F32, R.S32)[layout == "F"])):
                seed += 1
                twin = R.LinCase("far-" + shape, rows, 72, 136, src_dt=(R.U8, R.S8)[seed % 2], dst_dt=dst_dt, bia_dt=R.S32, seed=seed)
                esz = R.SIZE_OF[dst_dt]
                case = replace(twin, src_ld=pitch) if operand == "src" else replace(twin, dst_ld=pitch // esz)
                out.append(FarCase("linear", "%s-%s" % (shape, R.NAME_OF[dst_dt]), layout, operand, twin, case, bms))
    return out


def _linear_far(fc):
    c = fc.case
    if fc.operand == "src":
        return Far(1, tuple(r * c.sld for r in range(c.rows)), min(c.sld, R.up(c.k, 16)))
    return Far(R.SIZE_OF[c.dst_dt], tuple(r * c.dld for r in range(c.rows)), c.n)


# ---- patchembed -----------------------------------------------------------------------------------------------------------------
def _pe_cases():
    """dst through dst_ld (one image of 3 tokens) and through img_rows (3 images of 4 tokens, rows 64 elements apart), with and
    without prefix rows; src through bs: images of 2^24 bytes of which only the top-left 8 x 8 pixels are read (th = tw = 2,
    ph = pw = 4): 2048 x 2048 x 4 (granule 16) and 4096 x 4096 x 1 (granule 4), bs 130 (H) and 258 (F)"""
    out = []
    seed = 46000
    for layout in ("H", "F"):
        for dst_dt in (P.S8, (P.F32, P.S32)[layout == "F"]):
            esz = P.SIZE_OF[dst_dt]
            seed += 1
            twin = P.PeCase("far-ld", 1, 1, 3, 4, 4, 4, 40, src_dt=(P.U8, P.S8)[seed % 2], dst_dt=dst_dt, bia_dt=P.S32, seed=seed)
            out.append(FarCase("patchembed", "ld-" + P.NAME_OF[dst_dt], layout, "dst", twin, replace(twin, dst_ld=PITCH3[layout] // esz)))
            for prefix in (False, True):
                seed += 1
                twin = P.PeCase("far-rows", 3, 2, 2, 4, 4, 4, 40, src_dt=(P.U8, P.S8)[seed % 2], dst_dt=dst_dt, bia_dt=P.S32, t0=2, prefix=prefix,
                                dst_ld=64, seed=seed)
                slack = PITCH3[layout] // esz // 64 - (twin.t0 + twin.tokens)
                out.append(FarCase("patchembed", "rows-%s%s" % (P.NAME_OF[dst_dt], "-prefix" if prefix else ""), layout, "dst", twin,
                                   replace(twin, slack=slack)))
        for ic, side in ((4, 2048), (1, 4096)):
            seed += 1
            twin = P.PeCase("far-src", 130 if layout == "H" else 258, 2, 2, 4, 4, ic, 40, src_dt=(P.U8, P.S8)[seed % 2], dst_dt=P.S8,
                            bia_dt=P.S32, seed=seed)
            out.append(FarCase("patchembed", "bs-g%d" % twin.granule, layout, "src", twin, replace(twin, extra_h=side - 8, extra_w=side - 8)))
    return out


def _pe_out_rows(case):
    """the rows of an image that the op writes: the prefix rows where they are given, then the tokens"""
    return ([r for r in range(case.t0)] if case.prefix else []) + [case.t0 + t for t in range(case.tokens)]


def _pe_far(fc):
    c = fc.case
    if fc.operand == "src":
        img, row = c.ih * c.iw * c.ic, c.iw * c.ic
        return Far(1, tuple(b * img + y * row for b in range(c.bs) for y in range(c.th * c.ph)), c.tw * c.pw * c.ic)
    return Far(P.SIZE_OF[c.dst_dt], tuple((b * c.img_rows + r) * c.dld for b in range(c.bs) for r in _pe_out_rows(c)), c.oc)


# ---- bmm ------------------------------------------------------------------------------------------------------------------------
def _bmm_rows_cols(case, which):
    return {"a": (case.m, case.k), "b": case.b_shape, "c": (case.m, case.n)}[which]


def _bmm_cases():
    out = []
    seed = 42000
    for layout in ("H", "F"):
        for operand, trans_b, dst_dt in (("a", True, B.S8), ("b", True, B.S8), ("b", False, B.S8), ("c", True, B.U8), ("c", False, B.S32)):
            for carrier in ("s0", "s1", "ld"):
                seed += 1
                m, n, k = 33, 37, 40
                if carrier == "ld":       # the dimension that counts the far operand's rows is 3
                    if operand in ("a", "c"):
                        m = 3
                    elif trans_b:
                        n = 3
                    else:
                        k = 3
                batch = {"s0": (3, 1), "s1": (1, 3), "ld": (1, 1)}[carrier]
                twin = B.BmmCase("far-" + carrier, m, n, k, trans_b=trans_b, a_dt=(B.U8, B.S8)[seed % 2], dst_dt=dst_dt, batch=batch,
                                 c_ld=40, seed=seed)
                esz = B.SIZE_OF[dst_dt] if operand == "c" else 1
                far = PITCH3[layout] // esz
                s0, s1, ld = twin.strides(operand)
                strides = {"s0": (far, s1, ld), "s1": (s0, far, ld), "ld": (s0, s1, far)}[carrier]
                case = replace(twin, **{operand + "_strides": strides})
                out.append(FarCase("bmm", "%s-%s-%s" % (carrier, "nt" if trans_b else "nn", B.NAME_OF[dst_dt]), layout, operand, twin, case))
    return out


def _bmm_far(fc):
    c, which = fc.case, fc.operand
    s0, s1, ld = c.strides(which)
    rows, cols = _bmm_rows_cols(c, which)
    starts = tuple(b0 * s0 + b1 * s1 + r * ld for b0 in range(c.batch[0]) for b1 in range(c.batch[1]) for r in range(rows))
    return Far(B.SIZE_OF[c.dst_dt] if which == "c" else 1, starts, cols if which == "c" else min(ld, B.up16(cols)))


# ---- attention ------------------------------------------------------------------------------------------------------------------
def _attn_rows_cols(case, which):
    return {"q": (case.tq, case.d), "k": (case.tk, case.d), "v": (case.tk, case.dv), "o": (case.tq, case.dv)}[which]


def _attn_cases():
    """tq 33, tk 37, d 40, dv 35 with leading dimensions rounded up to 16: the one case is in the fused kernel's class and runs
    on the chain as well"""
    out = []
    seed = 45000
    for layout in ("H", "F"):
        for operand, dst_dt in (("q", A.S8), ("k", A.S8), ("v", A.S8), ("o", A.S8), ("o", A.F32)):
            for carrier in ("s0", "s1", "ld"):
                seed += 1
                tq, tk = 33, 37
                if carrier == "ld":       # the dimension that counts the far operand's rows is 3
                    if operand in ("q", "o"):
                        tq = 3
                    else:
                        tk = 3
                batch = {"s0": (3, 1), "s1": (1, 3), "ld": (1, 1)}[carrier]
                twin = A.AttnCase("far-" + carrier, tq, tk, 40, 35, q_dt=(A.U8, A.S8)[seed % 2], dst_dt=dst_dt, batch=batch, o_ld=40, seed=seed)
                esz = A.SIZE_OF[dst_dt] if operand == "o" else 1
                far = PITCH3[layout] // esz
                s0, s1, ld = twin.strides(operand)
                strides = {"s0": (far, s1, ld), "s1": (s0, far, ld), "ld": (s0, s1, far)}[carrier]
                case = replace(twin, **{operand + "_strides": strides})
                out.append(FarCase("attn", "%s-%s" % (carrier, A.NAME_OF[dst_dt]), layout, operand, twin, case))
    return out


def _attn_far(fc):
    c, which = fc.case, fc.operand
    s0, s1, ld = c.strides(which)
    rows, cols = _attn_rows_cols(c, which)
    starts = tuple(b0 * s0 + b1 * s1 + r * ld for b0 in range(c.batch[0]) for b1 in range(c.batch[1]) for r in range(rows))
    return Far(A.SIZE_OF[c.dst_dt] if which == "o" else 1, starts, cols if which == "o" else min(ld, A.up16(cols)))


# ---- lnorm ----------------------------------------------------------------------------------------------------------------------
def _lnorm_cases():
    out = []
    seed = 43
    for layout in ("H", "F"):
        for c in (40, 300):
            for operand, dst_dt in (("src", L.S8), ("dst", L.S8), ("dst", L.F32)):
                seed += 1
                esz = L.SIZE_OF[dst_dt] if operand == "dst" else 1
                # int32_t pitches: a 1-byte pitch near 2^30 reaches 2^31 with row 2 and 2^32 with row 4
                rows = 3 if layout == "H" or esz == 4 else 5
                pitch = PITCH3[layout] if rows == 3 else (1 << 30) + 4160
                ld = L.up16(c)
                twin = L.LnCase("far", rows, c, (L.S8, L.U8)[seed % 2], dst_dt, mode=seed % 2, src_ld=ld, dst_ld=ld, seed=seed)
                case = twin._replace(src_ld=pitch) if operand == "src" else twin._replace(dst_ld=pitch // esz)
                out.append(FarCase("lnorm", "c%d-%s" % (c, L.NAME_OF[dst_dt]), layout, operand, twin, case))
    return out


def _lnorm_far(fc):
    c = fc.case
    if fc.operand == "src":
        return Far(1, tuple(r * c.src_ld for r in range(c.rows)), min(c.src_ld, L.up16(c.c)))
    return Far(L.SIZE_OF[c.dst_dt], tuple(r * c.dst_ld for r in range(c.rows)), c.c)


# ---- head (the row and the generic kernel; the pixel kernel's class ends at src_ld 160) -------------------------------------------
HEAD_SKIP = 4                   # rows of head_ref.generate() left out in front: its row 3 is all equal, as a row of poison is


def _head_cases():
    out = []
    seed = 44
    for layout in ("H", "F"):
        for c in (21, 1000):
            k = 1 if c == 21 else 5
            idx_dt = H.U8 if c == 21 else H.S32
            specs = [("src", H.TOPK, H.S8, idx_dt, k), ("src", H.SOFTMAX, H.U8, H.F32, 1), ("idx", H.TOPK, H.U8 if c == 21 else H.F32, idx_dt, k),
                     ("dst", H.SOFTMAX, H.S8, H.U8, 1), ("dst", H.SOFTMAX, H.U8, H.F32, 1)]
            if c == 21:
                specs.append(("src", H.TOPK, H.F32, H.S32, 5))        # a 4-byte src: src_ld near 2^29 elements
                if layout == "F":
                    specs.append(("val", H.TOPK, H.F32, H.U8, 5))     # an f32 val beyond 2^32 next to a u8 idx (far_second)
            for operand, mode, src_dt, dst_dt, kk in specs:
                seed += 1
                esz = H.SIZE_OF[src_dt if operand in ("src", "val") else dst_dt]
                # int32_t pitches: a 1-byte pitch near 2^30 reaches 2^31 with row 2 and 2^32 with row 4
                rows = 3 if layout == "H" or esz == 4 else 5
                pitch = PITCH3[layout] // esz if rows == 3 else (1 << 30) + 4160
                twin = H.HeadCase("far", mode, rows, c, H._ld(c, src_dt), src_dt, dst_dt, k=kk, seed=seed)
                case = replace(twin, ld=pitch) if operand == "src" else replace(twin, dst_ld=pitch) if operand == "dst" else twin
                name = "c%d-%s-%s-%s" % (c, "softmax" if mode == H.SOFTMAX else "top%d" % kk, H.NAME_OF[src_dt], H.NAME_OF[dst_dt])
                out.append(FarCase("head", name, layout, operand, twin, case, pitch=pitch if operand in ("idx", "val") else 0))
    return out


VAL_BASE = P31 + (1 << 20)     # layout H: val's pointer behind idx's extent (the op refuses outputs whose extents overlap)


def far_second(fc):
    """The second operand in the arena of a head top-k case, or None.  idx and val share idx_ld, and dfx_head_submit refuses
    outputs whose EXTENTS overlap, so val cannot lie between idx's rows:
      operand "idx", layout H: val is far as well, its pointer VAL_BASE bytes behind idx's, behind idx's extent: two extents of
                     2^31 bytes fit the arena;
      operand "idx", layout F: None.  Two extents of 2^32 bytes do not fit: idx runs without val;
      operand "val" (layout F, f32 val, u8 idx): val's extent is four times idx's.  val is the far operand and idx lies at the
                     arena's START (base -BASE), within the first 2^31 bytes, where no 32-bit slip changes its offsets."""
    if fc.op != "head" or fc.operand not in ("idx", "val"):
        return None
    c = fc.case
    starts = tuple(r * fc.pitch for r in range(c.rows))
    if fc.operand == "val":
        return Far(H.SIZE_OF[c.dst_dt], starts, c.k, base=-BASE)
    return Far(H.SIZE_OF[c.src_dt], starts, c.k, base=VAL_BASE) if fc.layout == "H" else None


def second_values(fc):
    """the valid elements of far_second(fc), {rows, k}: val for a far idx, idx for a far val"""
    idx, val = H.reference(fc.twin, data_of(fc)["src"])
    return np.ascontiguousarray(idx if fc.operand == "val" else val)


def _head_far(fc):
    c = fc.case
    if fc.operand == "src":
        return Far(H.SIZE_OF[c.src_dt], tuple(r * c.ld for r in range(c.rows)), min(c.ld, H._ld(c.c, c.src_dt)))
    if fc.operand == "idx":
        return Far(H.SIZE_OF[c.dst_dt], tuple(r * fc.pitch for r in range(c.rows)), c.k)
    if fc.operand == "val":
        return Far(H.SIZE_OF[c.src_dt], tuple(r * fc.pitch for r in range(c.rows)), c.k)
    return Far(H.SIZE_OF[c.dst_dt], tuple(r * c.out_ld for r in range(c.rows)), c.c)


# ---- the tables and what the tests ask of a case ----------------------------------------------------------------------------------
LINEAR_CASES = tuple(_linear_cases())
PATCHEMBED_CASES = tuple(_pe_cases())
BMM_CASES = tuple(_bmm_cases())
ATTN_CASES = tuple(_attn_cases())
LNORM_CASES = tuple(_lnorm_cases())
HEAD_CASES = tuple(_head_cases())
ALL_CASES = LINEAR_CASES + PATCHEMBED_CASES + BMM_CASES + ATTN_CASES + LNORM_CASES + HEAD_CASES
# the overlap checks: the first far-src / far-A case of layout F per op (dst is placed inside and just behind the input)
OVERLAP_CASES = tuple(next(fc for fc in table if fc.layout == "F" and fc.is_input) for table in (LINEAR_CASES, BMM_CASES, ATTN_CASES, LNORM_CASES))


def far_of(fc):
    return {"linear": _linear_far, "patchembed": _pe_far, "bmm": _bmm_far, "attn": _attn_far, "lnorm": _lnorm_far, "head": _head_far}[fc.op](fc)


@functools.lru_cache(maxsize=None)
def data_of(fc):
    """the twin's data, as the op's own generator draws it; never written to"""
    if fc.op == "linear":
        return R.generate(fc.twin)
    if fc.op == "patchembed":
        return P.generate(fc.twin)
    if fc.op == "bmm":
        return B.generate(fc.twin)
    if fc.op == "attn":
        return A.generate(fc.twin)
    if fc.op == "head":
        t = fc.twin
        return dict(src=np.ascontiguousarray(H.make_src(replace(t, rows=t.rows + HEAD_SKIP))[HEAD_SKIP:]))
    return dict(src=L.make_src(fc.twin), params=L.make_params(fc.twin))


def descriptor_ok(fc, path):
    """the far case's descriptor passes the Python mirror of validate and is in the forced kernel's class"""
    if fc.op == "linear":
        d = R.desc_of(fc.case, path)
        return R.validate(d) == 0 and (path == R.GENERIC or R.tile_class(d))
    if fc.op == "patchembed":
        d = P.desc_of(fc.case, path)
        return P.validate(d) == 0 and (path == P.GENERIC or bool(P.desc_granule(d)))
    if fc.op == "bmm":
        d = B.desc_of(fc.case, path)
        return B.validate(d) == 0 and (path == B.GENERIC or B.mfma_class(d))
    if fc.op == "attn":
        d = A.desc_of(fc.case, path)
        return A.validate(d) == 0 and (path == A.CHAIN or A.fused_class(d))
    if fc.op == "head":
        c = fc.case
        lds = (c.ld, c.out_ld if c.mode == H.SOFTMAX else (fc.pitch or c.k))
        ok = c.rows >= 1 and c.ld >= c.c and lds[1] >= c.out_cols and max(lds) < P31 and c.rows * max(lds) <= 1 << 40 and \
            (c.mode == H.SOFTMAX or (1 <= c.k <= min(c.c, 8) and (c.dst_dt == H.S32 or c.c <= 256)))
        return ok and H.in_class(c, path)
    c = fc.case
    ok = c.rows >= 1 and 1 <= c.c <= L.MAX_C and c.src_ld >= c.c and c.dst_ld >= c.c and max(c.src_ld, c.dst_ld) < P31 and \
        c.rows * max(c.src_ld, c.dst_ld) <= 1 << 40
    return ok and L.in_class(c, path)


def input_segments(fc, data=None):
    """the far INPUT's segments as bytes, uint8 {segments, width * esz}: the twin's storage, row by row"""
    data = data_of(fc) if data is None else data
    far = far_of(fc)
    if fc.op == "linear":
        rows = np.asarray(data["src"]).view(np.uint8).reshape(fc.twin.rows, fc.twin.sld)
    elif fc.op == "patchembed":
        rows = np.asarray(data["src"]).view(np.uint8).reshape(-1, far.width)
    elif fc.op in ("bmm", "attn"):
        rows = np.asarray(data[fc.operand]).view(np.uint8).reshape(-1, fc.twin.strides(fc.operand)[2])
    elif fc.op == "head":
        rows = np.asarray(data["src"]).view(np.uint8).reshape(fc.twin.rows, -1)
    else:
        rows = np.asarray(data["src"]).view(np.uint8).reshape(fc.twin.rows, fc.twin.src_ld)
    assert rows.shape == (len(far.starts), far.width * far.esz), (fc.ident(), rows.shape)
    return rows


def values(fc, data=None):
    """the valid elements of the op's output from the twin's reference: {segments of the output, valid elements}"""
    data = data_of(fc) if data is None else data
    if fc.op == "linear":
        return R.values(fc.twin, data)
    if fc.op == "patchembed":
        t = fc.twin
        vals = P.values(t, data)                                       # {bs, tokens, oc}
        if t.prefix and not fc.is_input:                               # a far dst: the prefix rows of every image are written as well
            vals = np.concatenate([np.broadcast_to(data["prefix"][None], (t.bs, t.t0, t.oc)), vals], axis=1)
        return np.ascontiguousarray(vals).reshape(-1, t.oc)
    if fc.op == "bmm":
        return B.values(fc.twin, data).reshape(-1, fc.twin.n)
    if fc.op == "attn":
        return A.o_values(fc.twin, data).reshape(-1, fc.twin.dv)
    if fc.op == "head":
        want = H.reference(fc.twin, data["src"])
        if fc.twin.mode == H.SOFTMAX:
            return want
        if fc.operand == "idx":
            return want[0]
        if fc.operand == "val":
            return np.ascontiguousarray(want[1])
        bits = np.ascontiguousarray(want[1]).view({1: np.uint8, 4: np.uint32}[want[1].dtype.itemsize])
        return np.concatenate([want[0].astype(np.int64), bits.astype(np.int64)], axis=1)    # idx | val, both checked
    return L.reference(fc.twin, data["src"], data["params"])


def poisoned_values(fc):
    """values() with the far segments of the far INPUT replaced by what their first wrong alias holds: what a wrapped read would
    compute.  That is poison, except for patchembed's images of exactly 2^24 bytes, where image 256 + i wraps onto image i."""
    assert fc.is_input
    data = data_of(fc)
    far, true = far_of(fc), input_segments(fc)
    off = far.byte_offsets()
    held = dict(zip(off.reshape(-1).tolist(), true.reshape(-1).tolist()))
    seg = true.copy()
    for i in far.far_segments():
        alias = next(a for a in aliases(off[i])[1:] if not np.array_equal(a, off[i]))
        seg[i] = [held.get(a, POISON) for a in alias.tolist()]
    if fc.op == "linear":
        return values(fc, dict(data, src=seg.reshape(-1).view(R.NP_OF[fc.twin.src_dt])))
    if fc.op == "patchembed":
        t = fc.twin
        return values(fc, dict(data, src=seg.reshape(t.bs, t.ih, t.iw, t.ic).view(P.NP_OF[t.src_dt])))
    if fc.op == "bmm":
        dt = B.NP_OF[fc.twin.a_dt] if fc.operand == "a" else np.int8
        return values(fc, dict(data, **{fc.operand: seg.reshape(-1).view(dt)}))
    if fc.op == "attn":
        dt = A.NP_OF[fc.twin.q_dt] if fc.operand == "q" else np.int8
        return values(fc, dict(data, **{fc.operand: seg.reshape(-1).view(dt)}))
    if fc.op == "head":
        return values(fc, dict(data, src=seg.view(H.NP_OF[fc.twin.src_dt])))
    return values(fc, dict(data, src=seg.view(L.NP_OF[fc.twin.src_dt])))


def affected(fc, seg, vals):
    """the part of the output {segments, valid} that far input segment `seg` feeds"""
    t = fc.twin
    if fc.op == "patchembed":                                         # pixel row y of image b feeds the tokens of row y // ph
        b, y = divmod(int(seg), t.th * t.ph)
        return vals.reshape(t.bs, t.th, t.tw * t.oc)[b, y // t.ph]
    if fc.op not in ("bmm", "attn") or fc.operand in ("a", "q"):
        return vals[seg]
    if fc.op == "attn":                                               # a row of K or V feeds its whole matrix of O
        return vals.reshape(t.g, t.tq, t.dv)[int(seg) // t.tk]
    rows = t.b_shape[0]
    g, r = divmod(int(seg), rows)
    v = vals.reshape(t.g, t.m, t.n)[g]
    return v[:, r] if t.trans_b else v


def saturated_fraction(fc, vals):
    if fc.op == "linear":
        return R.saturated_fraction(fc.twin, vals)
    if fc.op == "patchembed":
        return P.saturated_fraction(fc.twin, vals)
    if fc.op == "bmm":
        return B.saturated_fraction(fc.twin, vals)
    if fc.op == "attn":
        return B.saturated_fraction(A.pv_case(fc.twin), vals)
    if fc.op == "head":                                                # (a softmax's 0 is the op's own result, as a ReLU's is)
        return float((vals == 255).mean()) if fc.twin.mode == H.SOFTMAX and fc.twin.dst_dt == H.U8 else 0.0
    if fc.twin.dst_dt == L.F32:
        return 0.0
    lo, hi = (0, 255) if fc.twin.dst_dt == L.U8 else (-128, 127)
    return float(((vals == lo) | (vals == hi)).mean())


PATHS = {"linear": (R.TILE, R.GENERIC), "patchembed": (P.TILE, P.GENERIC), "bmm": (B.MFMA, B.GENERIC), "attn": (A.FUSED, A.CHAIN), "lnorm": (L.ROW, L.GENERIC),
         "head": (H.ROW, H.GENERIC)}     # (the MFMA / tile / row kernel, generic)


def dense_reference(fc):
    """the twin's whole dense output storages as a tuple of byte arrays (poison wherever the op does not write): what a case
    with a far INPUT must leave in its small outputs (top-k: idx and val), and what the overlap checks' dst must hold"""
    data = data_of(fc)
    if fc.op == "linear":
        return (R.reference(fc.twin, data),)
    if fc.op == "patchembed":
        return (P.reference(fc.twin, data),)
    if fc.op == "bmm":
        return (B.reference(fc.twin, data),)
    if fc.op == "attn":
        return (A.reference(fc.twin, data),)
    if fc.op == "head":
        want = H.reference(fc.twin, data["src"])
        return tuple(np.ascontiguousarray(w).view(np.uint8).reshape(-1) for w in (want if isinstance(want, tuple) else (want,)))
    t = fc.twin
    full = np.full((t.rows, t.dst_ld * L.SIZE_OF[t.dst_dt]), POISON, dtype=np.uint8).view(L.NP_OF[t.dst_dt]).copy()
    full[:, :t.c] = values(fc, data)
    return (full.view(np.uint8).reshape(-1),)


def valid_width(fc):
    """the valid elements of a segment of the far operand (an input's segments are what may be READ: up to 16 more)"""
    if fc.op == "linear":
        return fc.case.k if fc.operand == "src" else fc.case.n
    if fc.op == "patchembed":
        return far_of(fc).width
    if fc.op == "bmm":
        return _bmm_rows_cols(fc.case, fc.operand)[1]
    if fc.op == "attn":
        return _attn_rows_cols(fc.case, fc.operand)[1]
    if fc.op == "head":
        return fc.case.k if fc.operand in ("idx", "val") else fc.case.c
    return fc.case.c


def overlap_places(fc):
    """byte offsets of a small dst against the far input of an F case -> (inside, behind): inside the input's extent, beyond
    2^32 and between two rows (the host's overlap check must refuse it); at the first byte behind the input's last valid
    element (it must run)"""
    far = far_of(fc)
    return P32 + 64, int(far.byte_starts().max()) + valid_width(fc)


# ---- wsum: a dense far tensor (no pitch to stretch) ---------------------------------------------------------------------------------
WSUM_IMAGE = (512, 512, 64)     # h * w * c = 2^24 bytes per image: image 128 starts at 2^31, image 256 at 2^32
WSUM_IMAGE_BYTES = 1 << 24


@dataclass(frozen=True)
class WsumFar:
    """One u8 tensor of `bs` images at the far base, IN PLACE (dst is the input: the alias rule allows it, and one far tensor
    serves both sides), per-channel scale and bias, a table on some runs.  Image b is image 0 rolled by b pixels; the op is
    element-wise with per-channel constants, so the expected image b is the expected image 0 rolled alike: numpy sees one image."""
    layout: str
    bs: int
    path: int
    lut: bool

    @property
    def one(self):
        return W.WsumCase("far", (1,) + WSUM_IMAGE, (W.U8,), W.U8, (True,), bias="c", lut_in=W.U8 if self.lut else W.UNDEF, seed=47 + self.bs)

    @property
    def case(self):
        return replace(self.one, shape=(self.bs,) + WSUM_IMAGE)

    def ident(self):
        return "wsum-%s-bs%d-%s%s" % (self.layout, self.bs, "vec" if self.path == W.VEC else "generic", "-lut" if self.lut else "")


# (the generic kernel over 258 images alone is several times the per-case time of the other tests: F runs on the vec kernel,
#  H on both)
WSUM_CASES = (WsumFar("H", 130, W.VEC, False), WsumFar("H", 130, W.GENERIC, True), WsumFar("F", 258, W.VEC, True))


def wsum_roll(b):
    """image b is np.roll(image 0, wsum_roll(b)): rolled by b pixels towards the front, so that on the device image b is the
    window from byte 64 b of image 0 laid out twice, and all images are one strided view"""
    return -WSUM_IMAGE[2] * b


@functools.lru_cache(maxsize=None)
def wsum_image(wc):
    """image 0 as flat bytes, drawn as wsum_ref.generate draws a u8 input; never written to"""
    img = W.generate(wc.one)[0].reshape(-1)
    img.setflags(write=False)
    return img


def wsum_reference(wc, img):
    """the op on one image (flat u8 -> flat u8)"""
    scales, bias, lut = W.make_params(wc.one)
    return W.reference(wc.one, [img.reshape(wc.one.shape)], scales, bias, lut).reshape(-1)


@functools.lru_cache(maxsize=None)
def wsum_expected(wc):
    out = wsum_reference(wc, wsum_image(wc))
    out.setflags(write=False)
    return out


# ---- the head's pixel kernel (class src_ld <= 160): dense far src, dense far idx ---------------------------------------------------
PIXEL_LD, PIXEL_R0 = 160, 4096
PIXEL_ROWS = P32 // PIXEL_LD + 1000          # the last 1000 rows start beyond 2^32; 2^32 is no multiple of 160, so a wrapped
#                                              address is misaligned as well


def pixel_map(i):
    """row i of the far tensor is row pixel_map(i) of a random block of PIXEL_R0 rows: the shift by i // R0 keeps row i apart
    from the rows 2^32 / 160 (rounded either way) in front of it, which a truncated offset would reach"""
    i = np.asarray(i, dtype=np.int64)
    return (i + i // PIXEL_R0) % PIXEL_R0


@dataclass(frozen=True)
class PixelFar:
    """argmax (top-1, u8 idx) over PIXEL_ROWS rows on the pixel kernel and, on the same data, the generic kernel.
    operand "src": u8 src at src_ld 160, c 150, idx_ld 1 (src far, idx small); operand "idx": a narrow src (c = src_ld = 16,
    small) and idx_ld 160 (idx far: one byte every 160; without val, whose extent would overlap idx's)"""
    operand: str

    @property
    def case(self):
        c, ld = (150, PIXEL_LD) if self.operand == "src" else (16, 16)
        return H.HeadCase("far-px", H.TOPK, PIXEL_ROWS, c, ld, H.U8, H.U8, seed=48)

    @property
    def idx_ld(self):
        return 1 if self.operand == "src" else PIXEL_LD

    @property
    def far_bytes(self):
        """the far tensor's extent: whole rows of 160 bytes"""
        return PIXEL_ROWS * PIXEL_LD

    def ident(self):
        return "head-pixel-%s" % self.operand


PIXEL_CASES = (PixelFar("src"), PixelFar("idx"))


@functools.lru_cache(maxsize=None)
def pixel_block(pc):
    """(the block {R0, src_ld} as head_ref.generate draws it, its argmax {R0} u8, its maximum {R0} u8); never written to"""
    block_case = replace(pc.case, rows=PIXEL_R0)
    src = H.generate(block_case)
    idx, val = (np.ascontiguousarray(a.reshape(-1)) for a in H.reference(block_case, src))
    for a in (src, idx, val):
        a.setflags(write=False)
    return src, idx, val
