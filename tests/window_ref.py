"""numpy reference of the window partition / reverse op (dfx_window_* of include/dfx.h) and the case tables of its tests.  Pure
numpy, needs no GPU.

The reference is written INDEPENDENTLY of the op's row map: partition is np.pad -> np.roll(-shift) -> reshape / transpose,
reverse is transpose / reshape -> np.roll(+shift) -> crop, the way official Swin does it with torch.  Everything works on
unsigned views (uint8 / uint32) of the data, so that bytes are moved and never interpreted."""
from dataclasses import dataclass

import numpy as np

F32, S32, S8, U8 = 1, 2, 3, 4                         # capi.DFX_*
PARTITION, REVERSE = 0, 1
ROW_MAJOR, COL_MAJOR = 0, 1
ROW, GENERIC, AUTO = 0, 1, -1
NP_OF = {F32: np.float32, S32: np.int32, S8: np.int8, U8: np.uint8}
SIZE_OF = {F32: 4, S32: 4, S8: 1, U8: 1}
NAME_OF = {F32: "f32", S32: "s32", S8: "s8", U8: "u8"}
RAW_OF = {1: np.uint8, 4: np.uint32}
SENTINEL = 0xCD                                        # hipref.POISON_BYTE
GUARD_ROWS = 3                                         # rows of sentinel behind the last row of every buffer


def ceil_to(n, m):
    return -(-n // m) * m


@dataclass(frozen=True)
class WinCase:
    name: str
    bs: int
    h: int
    w: int
    c: int
    window: tuple
    shift: tuple = (0, 0)
    order: int = ROW_MAJOR
    dt: int = S8
    grid_ld: int = 0                                   # 0: c
    win_ld: int = 0
    pad_value: int = 0
    seed: int = 1

    @property
    def esize(self):
        return SIZE_OF[self.dt]

    @property
    def gld(self):
        return self.grid_ld or self.c

    @property
    def wld(self):
        return self.win_ld or self.c

    @property
    def hp(self):
        return ceil_to(self.h, self.window[0])

    @property
    def wp(self):
        return ceil_to(self.w, self.window[1])

    @property
    def n_windows(self):
        return (self.hp // self.window[0]) * (self.wp // self.window[1])

    @property
    def grid_rows(self):
        return self.bs * self.h * self.w

    @property
    def win_rows(self):
        return self.bs * self.hp * self.wp

    @property
    def row_class(self):
        es = self.esize
        return (self.c * es) % 16 == 0 and (self.gld * es) % 16 == 0 and (self.wld * es) % 16 == 0

    @property
    def lanes(self):
        return self.c * self.esize // 16

    def paths(self):
        """(force_path, the kernel that must run)"""
        return ([(ROW, ROW)] if self.row_class else []) + [(GENERIC, GENERIC), (AUTO, GENERIC)]

    def ident(self):
        return "%s-bs%d-%dx%dx%d-win%dx%d-shift%d.%d-%s-%s-ld%d.%d-pad%x" % (
            self.name, self.bs, self.h, self.w, self.c, self.window[0], self.window[1], self.shift[0], self.shift[1],
            "col" if self.order else "row", NAME_OF[self.dt], self.gld, self.wld, self.pad_value)


def pad_scalar(case):
    """pad_value as one element of the raw view: its low byte for 1-byte dtypes"""
    return RAW_OF[case.esize](case.pad_value & (0xff if case.esize == 1 else 0xffffffff))


# ---- the reference --------------------------------------------------------------------------------------------------------------
def partition(x, window, shift=(0, 0), order=ROW_MAJOR, pad=0):
    """x {bs, h, w, c} -> {bs * nW * wh * ww, c}: pad to hp x wp with `pad`, roll by -shift, cut into windows"""
    bs, h, w, c = x.shape
    wh, ww = window
    hp, wp = ceil_to(h, wh), ceil_to(w, ww)
    xp = np.pad(x, ((0, 0), (0, hp - h), (0, wp - w), (0, 0)), mode="constant", constant_values=pad)
    xr = np.roll(xp, (-shift[0], -shift[1]), axis=(1, 2))
    win = xr.reshape(bs, hp // wh, wh, wp // ww, ww, c).transpose(0, 1, 3, 2, 4, 5)      # bs, wy, wx, iy, ix, c
    if order == COL_MAJOR:
        win = win.transpose(0, 1, 2, 4, 3, 5)                                            # bs, wy, wx, ix, iy, c
    return np.ascontiguousarray(win).reshape(-1, c)


def reverse(rows, bs, h, w, window, shift=(0, 0), order=ROW_MAJOR):
    """{bs * nW * wh * ww, c} -> {bs, h, w, c}: windows back to the padded map, roll by +shift, crop"""
    wh, ww = window
    hp, wp = ceil_to(h, wh), ceil_to(w, ww)
    c = rows.shape[1]
    if order == COL_MAJOR:
        win = rows.reshape(bs, hp // wh, wp // ww, ww, wh, c).transpose(0, 1, 2, 4, 3, 5)
    else:
        win = rows.reshape(bs, hp // wh, wp // ww, wh, ww, c)
    xr = win.transpose(0, 1, 3, 2, 4, 5).reshape(bs, hp, wp, c)
    xp = np.roll(xr, (shift[0], shift[1]), axis=(1, 2))
    return np.ascontiguousarray(xp[:, :h, :w, :])


def pad_mask(case):
    """boolean {win_rows}: the window-side rows that are pad tokens (by the same independent route)"""
    ones = np.ones((case.bs, case.h, case.w, 1), dtype=np.uint8)
    return partition(ones, case.window, case.shift, case.order, 0).reshape(-1) == 0


# ---- data -----------------------------------------------------------------------------------------------------------------------
def make_tokens(case, rows):
    """random raw elements {rows, c} with every row distinct, so that a misplaced token cannot compare equal"""
    raw = RAW_OF[case.esize]
    for attempt in range(8):
        rng = np.random.RandomState(case.seed * 131 + attempt)
        t = rng.randint(0, 256, size=(rows, case.c * case.esize)).astype(np.uint8)
        if np.unique(t, axis=0).shape[0] == rows:
            return np.ascontiguousarray(t).view(raw).reshape(rows, case.c)
    raise AssertionError("no seed gives distinct tokens: " + case.ident())


def storage(case, tokens, ld):
    """the tokens in a buffer of rows `ld` apart with GUARD_ROWS rows behind them, everything else SENTINEL -> raw {rows + guard, ld}"""
    rows = tokens.shape[0]
    buf = np.full((rows + GUARD_ROWS, ld * case.esize), SENTINEL, dtype=np.uint8).view(RAW_OF[case.esize]).reshape(rows + GUARD_ROWS, ld)
    buf[:rows, :case.c] = tokens
    return buf


def grid_tokens(case):
    return make_tokens(case, case.grid_rows)


def window_tokens(case):
    """what a partition of grid_tokens(case) must produce, raw {win_rows, c}"""
    x = grid_tokens(case).reshape(case.bs, case.h, case.w, case.c)
    return partition(x, case.window, case.shift, case.order, pad_scalar(case))


def reversed_tokens(case, win):
    return reverse(win, case.bs, case.h, case.w, case.window, case.shift, case.order).reshape(case.grid_rows, case.c)


# ---- the plan, restated (csrc/window_plan.h) -----------------------------------------------------------------------------------
MAX_BLOCKS, UNROLL = 2048, 4


def dst_rows(case, direction):
    return case.win_rows if direction == PARTITION else case.grid_rows


def planned_grid(case, direction, path, cap=0):
    rows = dst_rows(case, direction)
    work, per = (rows * case.lanes, 256 * UNROLL) if path == ROW else (rows * case.c, 256)
    blocks = min(-(-work // per), MAX_BLOCKS)
    if cap > 0:
        blocks = min(blocks, cap)
    return max(blocks, 1)


def kernel_name(case, direction, path):
    d = "partition" if direction == PARTITION else "reverse"
    return "window_row<%s,%s,l%d>" % (d, NAME_OF[case.dt], case.lanes) if path == ROW else "window_generic<%s,%s>" % (d, NAME_OF[case.dt])


def algorithmic_bytes(case, direction):
    token = case.c * case.esize
    if direction == PARTITION:
        return (case.grid_rows + case.win_rows) * token + 4 * case.hp * case.wp
    return 2 * case.grid_rows * token + 4 * case.h * case.w


# ---- the case tables ------------------------------------------------------------------------------------------------------------
GRIDS = ((1, 1), (7, 7), (10, 13), (3, 200), (5, 4))
WINDOWS = ((2, 2), (4, 4), (7, 7), (3, 5))
PADS = (0, 0x80, 0x3FC01234)                          # 0, a byte with the top bit set, a 4-byte f32 pattern
# (c, dtype): token bytes 16 (one lane), 48 and 96 (3 and 6 lanes), 272 (17 lanes), in all four dtypes
IN_CLASS = ((16, U8), (48, S8), (96, S8), (272, U8), (4, F32), (12, S32), (24, F32), (68, S32), (96, U8), (16, S8))


def grid_cases():
    """every grid x window x shift kind; order, batch, channels / dtype, the leading dimensions and the pad value cycle
    through their values with periods that do not divide one another"""
    out = []
    i = 0
    for h, w in GRIDS:
        for wh, ww in WINDOWS:
            hp, wp = ceil_to(h, wh), ceil_to(w, ww)
            for kind in range(4):
                shift = ((0, 0), (wh // 2, ww // 2), ((wh // 2, 0), (0, ww // 2))[(i // 4) % 2], (hp - 1, wp - 1))[kind]
                c, dt = IN_CLASS[i % len(IN_CLASS)]
                g = 16 // SIZE_OF[dt]
                ldk = (i // 2) % 4
                out.append(WinCase("grid", (1, 3)[i % 3 == 0], h, w, c, (wh, ww), shift, (i // 3) % 2, dt,
                                   grid_ld=c + g if ldk in (1, 3) else 0, win_ld=c + 2 * g if ldk in (2, 3) else 0,
                                   pad_value=PADS[i % 3], seed=100 + i))
                i += 1
    return out


def odd_cases():
    """outside the row kernel's class: c 5 and 21, c * esize no multiple of 16, a leading dimension that is none"""
    out = []
    for i, (c, dt, gld, wld) in enumerate(((5, U8, 0, 0), (21, S8, 0, 0), (21, U8, 32, 23), (5, F32, 0, 0), (5, S32, 7, 8), (16, U8, 24, 0),
                                            (16, S8, 0, 17), (4, F32, 6, 0), (3, S8, 0, 0))):
        for h, w, win, shift in ((10, 13, (7, 7), (3, 3)), (5, 4, (7, 7), (6, 2)), (3, 200, (3, 5), (0, 0))):
            out.append(WinCase("odd", (1, 3)[i % 2], h, w, c, win, shift, i % 2, dt, grid_ld=gld, win_ld=wld, pad_value=PADS[(i + 1) % 3],
                               seed=700 + 10 * i + h))
    return out


def swin_cases():
    """the shapes the op is for: a W-MSA / SW-MSA pair with padding on both axes, patch merging (2 x 2, column-major, one row of
    4 c per window), space-to-depth, and enough rows for several workgroup trips of the row kernel"""
    return [
        WinCase("wmsa", 2, 16, 12, 64, (7, 7), (0, 0), ROW_MAJOR, S8, win_ld=192, seed=901),
        WinCase("swmsa", 2, 16, 12, 64, (7, 7), (3, 3), ROW_MAJOR, S8, win_ld=192, seed=902),
        WinCase("merge", 2, 16, 12, 64, (2, 2), (0, 0), COL_MAJOR, S8, seed=903),
        WinCase("merge-odd", 1, 7, 5, 32, (2, 2), (0, 0), COL_MAJOR, U8, pad_value=0x80, seed=904),
        WinCase("reorg", 1, 8, 8, 4, (2, 2), (0, 0), ROW_MAJOR, F32, seed=905),
        WinCase("trips", 3, 56, 56, 96, (7, 7), (3, 3), ROW_MAJOR, S8, seed=906),
        WinCase("trips-pad", 2, 50, 61, 96, (7, 7), (3, 3), COL_MAJOR, U8, pad_value=0x80, seed=907),
    ]


ALL_CASES = tuple(grid_cases() + odd_cases() + swin_cases())
