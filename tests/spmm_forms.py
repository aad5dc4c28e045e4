"""The dispatch rule of mspmv_csrmm_f32 / _f64 restated on the test side, the structured matrices and the table of cases of
tests/test_spmm_forms.py (GPU) and tests/test_spmm_dispatch_rule.py (no GPU).

Written from what include/mspmv.h documents about mspmv_csrmm_* and from reading csrmm_impl; nothing of the C++ is imported or
parsed.  One call takes its k right-hand sides in groups of 16, 8, 4, 2, 1 columns, widest first.  A width runs as

  slot    spmm_lane_kernel on tiles of 256 x 11 path items: widths 8 and 16 (at least 32 bytes of right-hand sides) when
          rows + nnz >= 8 Mi and X (cols * ldx elements) spans less than 4 GB;
  pack    spmm_tile_kernel: packs of up to 16 bytes on 256 x 7 tiles always; 32-byte packs on 256 x 3 and 64-byte packs on 128 x 3
          tiles only when X is larger than 1 MiB (a width the call may not use is left to the narrower ones);
  rowwise spmm_rowwise_kernel, one launch for the whole call, when the CSR arrays are not 16-byte aligned, nnz < 4 or rows < 3.

Before the first width of a tile size its tile coordinates are computed (coords_scatter_kernel), and behind every width's kernel
runs spmm_fixup_kernel when that tile size has more than one tile.  alpha == 1 and beta == 0 is the plain form, anything else the
axpby form; a CSR stream (values, column indices, row offsets) above 200 MiB is read with non-temporal loads.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

CSRMV = "csrmv"                           # marker: k = ldx = ldy = 1 is the CsrMV call, not covered here
ELEM = {"f32": 4, "f64": 8}
TILE_NARROW, TILE_PACK32, TILE_PACK64, TILE_SLOT = 256 * 7, 256 * 3, 128 * 3, 256 * 11
TILE_ORDER = (TILE_NARROW, TILE_PACK32, TILE_PACK64, TILE_SLOT)          # the order of the coordinate regions in the temp storage
WIDE_X_BYTES = 1 << 20                    # X larger than this: 32- and 64-byte packs
SLOT_MIN_ITEMS = 8 << 20                  # rows + nnz from here on: the slot form ...
SLOT_MAX_X_BYTES = 1 << 32                # ... while X spans less than this
NT_STREAM_BYTES = 200 << 20
FIXUP_CHUNK = 512                         # carries per fix-up block (256 threads x 2)
COORD_BYTES = 8


@dataclass(frozen=True)
class Group:
    """`count` groups of `width` right-hand sides, the first at column `col0` of the call"""
    width: int
    count: int
    col0: int
    form: str                # "pack" | "slot"
    tile: int                # path items per tile
    block: int               # threads per block of the tile kernel
    vec_bytes: int           # the unit X and Y are read / written in when aligned to it (x_vec / y_vec)


def flags(prec, rows, cols, nnz, ldx):
    """(wide, slot_ok, nt) of a call"""
    eb = ELEM[prec]
    x_bytes = cols * ldx * eb
    wide = x_bytes > WIDE_X_BYTES
    slot_ok = x_bytes < SLOT_MAX_X_BYTES and rows + nnz >= SLOT_MIN_ITEMS
    nt = nnz * (eb + 4) + 4 * rows > NT_STREAM_BYTES
    return wide, slot_ok, nt


def groups_of(prec, rows, cols, nnz, k, ldx):
    """how the k columns are cut: a list of Group, widest first"""
    eb = ELEM[prec]
    wide, slot_ok, _ = flags(prec, rows, cols, nnz, ldx)
    out, col0, left = [], 0, k
    for w in (16, 8, 4, 2, 1):
        pack = w * eb
        if slot_ok and w >= 8 and pack >= 32:
            form, tile, block, vec = "slot", TILE_SLOT, 256, min(pack // 4, 16)     # four lanes per slot, at most 16 bytes per lane
        elif pack <= 16:
            form, tile, block, vec = "pack", TILE_NARROW, 256, pack
        elif wide and pack == 32:
            form, tile, block, vec = "pack", TILE_PACK32, 256, pack
        elif wide and pack == 64:
            form, tile, block, vec = "pack", TILE_PACK64, 128, pack
        else:
            continue
        count = left // w
        if count:
            out.append(Group(w, count, col0, form, tile, block, vec))
            col0 += count * w
            left -= count * w
    assert left == 0
    return out


def num_tiles(rows, nnz, tile):
    return (rows + nnz + tile - 1) // tile


def vec_flags(prec, group, ldx, ldy, x_off, y_off):
    """(x_vec, y_vec) of a group: X / Y views that start x_off / y_off elements into 256-byte aligned allocations"""
    eb = ELEM[prec]
    xv = ((x_off + group.col0) * eb) % group.vec_bytes == 0 and (ldx * eb) % group.vec_bytes == 0
    yv = ((y_off + group.col0) * eb) % group.vec_bytes == 0 and (ldy * eb) % group.vec_bytes == 0
    return xv, yv


class Launch(tuple):
    """(kernel_name, grid, block, width, groups, axpby, nt): a plain 7-tuple that also remembers the precision of its call"""
    def __new__(cls, prec, *fields):
        self = super().__new__(cls, fields)
        self.prec = prec
        return self


def expected_launches(prec, rows, cols, nnz, k, ldx, ldy, aligned=True, alpha=1.0, beta=0.0):
    """the launches of one call, in order: (kernel_name, grid, block, width, groups, axpby, nt); width 0 = not a property of that
    launch (coordinates, row-wise)"""
    out = _launches(prec, rows, cols, nnz, k, ldx, ldy, aligned, alpha, beta)
    return out if out == CSRMV else [Launch(prec, *e) for e in out]


def _launches(prec, rows, cols, nnz, k, ldx, ldy, aligned, alpha, beta):
    assert ldx >= k and ldy >= k
    if k == 1 and ldx == 1 and ldy == 1:
        return CSRMV
    if rows == 0 or k == 0:
        return []
    axpby = not (alpha == 1.0 and beta == 0.0)
    _, _, nt = flags(prec, rows, cols, nnz, ldx)
    if not aligned or nnz < 4 or rows < 3:
        return [("spmm_rowwise_kernel", (rows * k + 255) // 256, 256, 0, 1, axpby, False)]
    out, have = [], set()
    for g in groups_of(prec, rows, cols, nnz, k, ldx):
        tiles = num_tiles(rows, nnz, g.tile)
        if g.tile not in have:
            have.add(g.tile)
            out.append(("coords_scatter_kernel", ((rows + 1 + 3) // 4 + 255) // 256, 256, 0, 1, False, False))
        out.append(("spmm_lane_kernel" if g.form == "slot" else "spmm_tile_kernel", tiles, g.block, g.width, g.count, axpby, nt))
        if tiles > 1:
            out.append(("spmm_fixup_kernel", (tiles + FIXUP_CHUNK - 1) // FIXUP_CHUNK, 256, g.width, g.count, axpby, nt))
    return out


def _align256(v):
    return (v + 255) & ~255


def temp_bytes(prec, rows, cols, nnz, k, ldx, ldy=None):
    """the temp storage the size query reports: one region of tile coordinates (tiles + 1 of them) per tile size in use, in the
    order narrow / 32-byte / 64-byte / slot, then one region of carries -- per group of a width one carry per tile, a carry being
    its row (padded to an element) and `width` sums; the widths run one after the other and share it -- every region padded to
    256 bytes.  (k = ldx = ldy = 1: the CsrMV call's needs join in; not restated here.)"""
    eb = ELEM[prec]
    gs = groups_of(prec, rows, cols, nnz, k, ldx)
    carry = 256
    for g in gs:
        carry = max(carry, max(num_tiles(rows, nnz, g.tile), 1) * g.count * (eb + g.width * eb))
    off = 0
    for tile in TILE_ORDER:
        if any(g.tile == tile for g in gs):
            off = _align256(off + (num_tiles(rows, nnz, tile) + 1) * COORD_BYTES)
    return _align256(off + carry)


def form_key(entry):
    """(prec, width, form, axpby, nt) of a launch of expected_launches, None for the launches that are not a tile kernel"""
    name, _, _, width, _, axpby, nt = entry
    prec = entry.prec
    if name == "spmm_rowwise_kernel":
        return (prec, 0, "rowwise", axpby, False)
    if name == "spmm_lane_kernel":
        return (prec, width, "slot", axpby, nt)
    if name == "spmm_tile_kernel":
        return (prec, width, "pack", axpby, nt)
    return None


KERNELS = ([("f32", w, "pack") for w in (1, 2, 4, 8, 16)] + [("f32", w, "slot") for w in (8, 16)] +
           [("f64", w, "pack") for w in (1, 2, 4, 8)] + [("f64", w, "slot") for w in (8, 16)])
assert len(KERNELS) == 13


# ---------------------------------------------------------------------------------------------------------------------------
# the matrices: row lengths built so that every tile size named meets every shape its kernels distinguish.  On the merge path a
# row is its nonzeros followed by one row-end item: row r occupies len[r] + 1 consecutive path items, and tile t holds the items
# [t * T, (t + 1) * T).

SLOTS = 64                                # slots per block of the slot form: 64 (fp32, fp64 width 8) or 32 (fp64 width 16)


@dataclass
class Structure:
    name: str
    lens: np.ndarray                      # int64 [rows]
    tiles: tuple                          # the tile sizes this matrix was built for
    giant: int                            # the giant row
    marks: dict = field(default_factory=dict)          # (tile size, feature) -> first path item of the place built for it

    @property
    def rows(self):
        return int(self.lens.size)

    def nnz(self, trim=0):
        return int(self.lens.sum()) - trim

    def offsets(self, trim=0):
        off = np.zeros(self.rows + 1, np.int64)
        np.cumsum(self.lens, out=off[1:])
        off[-1] -= trim                   # (the last row is long: trimming shortens it only)
        return off


class _Builder:
    def __init__(self):
        self.parts, self.pos, self.rows, self.marks = [], 0, 0, {}

    def add(self, lens):
        a = np.asarray(lens, np.int64)
        self.parts.append(a)
        self.pos += int(a.sum()) + a.size
        self.rows += a.size

    def align(self, T, nonzeros_only=False):
        """one row that ends the current tile of size T: with its row-end item the tile's last item, or (nonzeros_only) with its
        last nonzero the tile's last item and its row-end item the first of the next tile"""
        need = (-self.pos) % T
        if nonzeros_only:
            self.add([need if need else T])
        else:
            self.add([need - 1 if need else T - 1])

    def mark(self, T, what):
        self.marks[(T, what)] = self.pos

    def section(self, T):
        self.align(T); self.mark(T, "empty_run"); self.add(np.zeros(T + 37, np.int64))       # empty rows: more than a tile of them
        self.align(T); self.mark(T, "one_tile_rows"); self.add([T - 1] * 3)                   # rows of exactly one tile's items
        self.add([T] * 2)                                                                     # ... and of one tile's worth of nonzeros
        self.align(T, nonzeros_only=True); self.mark(T, "nonzeros_end_tile")                  # (pos is one past a boundary now)
        self.align(T); self.mark(T, "row_end_ends_tile")
        # a tile of 64 equal rows: T - 64 nonzeros, every row ends where a share (T - 64) * s / 64 ends (every second one: / 32)
        self.mark(T, "share_ends"); self.add([T // SLOTS - 1] * SLOTS)
        assert self.pos % T == 0
        # rows over several shares that end inside a later one, short rows and empty rows between them
        self.mark(T, "multi_share"); self.add([T // 16 + 7, 5, T // 8 + 3, 1, 1, 0, 0, T // 5, 0, 97, T // 4 + 1, 44, 43, 42, T // 3, 2, 0, 1])
        self.align(T); self.mark(T, "sparse_tile"); self.add([2] * 5 + [0] * (T - 15))       # a tile of 10 nonzeros: fewer than slots
        assert self.pos % T == 0


def _filler(n, salt):
    """n row lengths in [0, 40], a fixed integer hash of the index"""
    i = np.arange(n, dtype=np.uint64) + np.uint64(salt)
    h = (i * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(33)
    h = (h * np.uint64(0xBF58476D)) >> np.uint64(7)
    return (h % np.uint64(41)).astype(np.int64)


def build_structure(name, tiles, giant, filler_rows):
    b = _Builder()
    b.add(_filler(filler_rows // 2, 1))
    for T in tiles:
        b.section(T)
    b.marks["giant"] = b.pos + 50
    b.add([0] * 50 + [giant] + [0] * 50)                  # a giant row between empty rows
    b.add(_filler(filler_rows - filler_rows // 2, 2))
    # the last row: 2.5 of the largest tiles long, open at the end of the last tile; (rows + 1) % 4 != 0 and nnz % 4 == 3, so that
    # trimming 0, 1, 2 nonzeros off it gives every ragged tail of the arrays
    if (b.rows + 2) % 4 == 0:
        b.add([3])
    last = 5 * max(tiles) // 2
    nnz = b.pos - b.rows
    last += (3 - (nnz + last)) % 4
    b.add([last])
    s = Structure(name, np.concatenate(b.parts), tuple(tiles), giant, b.marks)
    assert (s.rows + 1) % 4 != 0 and s.nnz() % 4 == 3
    return s


_STRUCTS = {}


def structure(name):
    """mid: below 8 Mi path items (packs only).  big: above (slot form), CSR stream below 200 MiB.  huge: stream above 200 MiB in
    both precisions (non-temporal loads).  tiny: 2 rows (row-wise kernel)"""
    if name not in _STRUCTS:
        if name == "mid":
            s = build_structure(name, (TILE_NARROW, TILE_PACK32, TILE_PACK64), 1_500_001, 40_000)
            assert s.rows + s.nnz() < SLOT_MIN_ITEMS
        elif name == "big":
            s = build_structure(name, (TILE_SLOT, TILE_NARROW, TILE_PACK32), 2_000_003, 310_000)
            assert s.rows + s.nnz(2) >= SLOT_MIN_ITEMS and s.nnz() * 12 + 4 * s.rows <= NT_STREAM_BYTES
        elif name == "huge":
            s = build_structure(name, (TILE_SLOT, TILE_NARROW, TILE_PACK32, TILE_PACK64), 2_000_003, 1_300_000)
            assert s.nnz(2) * 8 + 4 * s.rows > NT_STREAM_BYTES
        elif name == "tiny":
            s = Structure(name, np.array([2, 1], np.int64), (), 0)
        else:
            raise KeyError(name)
        _STRUCTS[name] = s
    return _STRUCTS[name]


# ---------------------------------------------------------------------------------------------------------------------------
# the cases

@dataclass(frozen=True)
class Case:
    name: str
    mat: str
    prec: str
    cols: int
    k: int
    xw: int                  # X is the view [:, x_off : x_off + k] of a [cols, xw] buffer (ldx = xw) ...
    x_off: int
    yw: int                  # ... Y likewise of a [rows, yw] buffer
    y_off: int
    alpha: int = 1
    beta: int = 0
    trim: int = 0            # nonzeros taken off the last row: nnz % 4 = 3 - trim
    pad: int = 0             # > 0: values and column indices start `pad` elements into their allocations (unaligned arrays)
    zeros: bool = False      # the zero-laden data of tests/test_spmm_forms.py (same structure, same launches)
    wide: bool = False       # the wide data: odd integers that fill the exactness budget (same structure, same launches)

    def dims(self):
        s = structure(self.mat)
        return s.rows, self.cols, s.nnz(self.trim)

    def launches(self):
        rows, cols, nnz = self.dims()
        return expected_launches(self.prec, rows, cols, nnz, self.k, self.xw, self.yw, aligned=self.pad == 0,
                                 alpha=float(self.alpha), beta=float(self.beta))

    def groups(self):
        rows, cols, nnz = self.dims()
        return groups_of(self.prec, rows, cols, nnz, self.k, self.xw)


COLS_SMALL, COLS, COLS_4GB = 1501, 70_001, (1 << 25) + 1


def _al(k, to):
    return (k + to - 1) // to * to


def _cases():
    out = []

    def add(name, mat, prec, cols, k, aligned_views, alpha, beta, trim=0, pad=0, xw=None):
        # aligned views: X and Y are the first k columns of buffers whose rows are multiples of 128 bytes -- every group's x_vec and
        # y_vec set; otherwise views one / two elements into buffers of odd width -- both clear for every width > 1
        if aligned_views:
            w = xw or _al(k + 1, 32)
            out.append(Case(name, mat, prec, cols, k, w, 0, _al(k + 1, 32), 0, alpha, beta, trim, pad))
        else:
            w = xw or (k + 3) | 1
            out.append(Case(name, mat, prec, cols, k, w, 1, (k + 5) | 1, 2, alpha, beta, trim, pad))

    for prec, kp in (("f32", 31), ("f64", 15)):
        # below 8 Mi items, X above 1 MiB: every pack width of the precision, temporal loads
        add(f"mid_packs_plain_{prec}", "mid", prec, COLS, kp, True, 1, 0, trim=0)
        add(f"mid_packs_axpby_{prec}", "mid", prec, COLS, kp, False, -2, 3, trim=1)
        # several groups of the widest pack (64 bytes), beta = 0 with alpha != 1
        add(f"mid_wide_groups_{prec}", "mid", prec, COLS, 3 * (kp + 1) // 2 + 3, False, -2, 0, trim=2)
        # X below 1 MiB: narrow packs only, several groups of them
        add(f"mid_narrow_only_{prec}", "mid", prec, COLS_SMALL, kp, True, 1, 3, trim=1)
        # unaligned CSR arrays: the row-wise kernel
        add(f"mid_rowwise_{prec}", "mid", prec, COLS, 5, False, -2, 3, trim=2, pad=1)
        add(f"tiny_rowwise_{prec}", "tiny", prec, 7, 3, True, 1, 0)
        # 8 Mi items and more: slot form for 16 and 8, packs for the rest (fp64: the 32-byte pack of 4), temporal loads
        add(f"big_slots_plain_{prec}", "big", prec, COLS, 31, True, 1, 0, trim=2)
        add(f"big_slots_axpby_{prec}", "big", prec, COLS, 31, False, -2, 3, trim=0)
        # two groups of 16 in the slot form (its loop over groups, the carries of the second group, the fix-up's second list)
        add(f"big_slot_groups_{prec}", "big", prec, COLS, 40, True, 1, 3, trim=1)
        # CSR stream above 200 MiB: non-temporal loads.  X below 4 GB: slot form (two groups of 16) and packs of 4, 2, 1 ...
        add(f"huge_slots_nt_plain_{prec}", "huge", prec, COLS, 47, True, 1, 0, trim=1)
        add(f"huge_slots_nt_axpby_{prec}", "huge", prec, COLS, 31, False, -2, 3, trim=2)
        # ... X of 4 GB and more: the 64- and 32-byte packs
        kw = 24 if prec == "f32" else 12
        add(f"huge_packs_4gb_nt_plain_{prec}", "huge", prec, COLS_4GB, kw, True, 1, 0, trim=0, xw=32 if prec == "f32" else 16)
        add(f"huge_packs_4gb_nt_axpby_{prec}", "huge", prec, COLS_4GB, kw, False, -2, 3, trim=1, xw=35 if prec == "f32" else 19)
    return out


CASES = _cases()


def _zero_cases():
    """the tiny, mid and big cases again on zero-laden data -- row-wise, every pack width, slot form, groups, fix-up --, and the slot
    form with alpha < 0 and beta == 0, which no case of CASES has.  The huge cases run the same arithmetic with non-temporal loads
    and keep their non-zero data."""
    import dataclasses
    out = [dataclasses.replace(c, name=c.name + "_zeros", zeros=True) for c in CASES if c.mat != "huge"]
    for c in CASES:
        if c.name.startswith("big_slots_axpby"):
            out.append(dataclasses.replace(c, name=f"big_slots_negative_alpha_beta_0_{c.prec}_zeros", zeros=True, beta=0))
    return out


ZERO_CASES = _zero_cases()


def _wide_cases():
    """per precision one case per form on the wide data: the row-wise kernel, every pack width (alpha = -2, beta = 3), the slot form
    of 16 and 8 with the packs behind it, two groups of 16 in the slot form; every one but the row-wise sends the giant row, the
    one-tile rows and the open last row through the carries and the fix-up"""
    import dataclasses
    heads = ("mid_rowwise", "mid_packs_axpby", "big_slots_axpby", "big_slot_groups")
    return [dataclasses.replace(c, name=c.name + "_wide", wide=True) for c in CASES if c.name.startswith(heads)]


WIDE_CASES = _wide_cases()
assert len(WIDE_CASES) == 8
# NaN / Inf containment: one pack case and one slot case per precision
CONTAINMENT = [c for c in CASES if c.name.startswith(("mid_packs_axpby", "big_slots_axpby"))]
# the same four run scaled to both ends of the exponent range and with -0.0 in Y0
SCALED = CONTAINMENT


def coverage(cases):
    """form key -> names of the cases that run it; (prec, width, form, "vec" | "novec") and (prec, width, form, "groups>=2")
    likewise"""
    cov = {}
    for c in cases:
        launches = c.launches()
        if launches == CSRMV:
            continue
        for e in launches:
            key = form_key(e)
            if key is not None:
                cov.setdefault(key, []).append(c.name)
        if launches and launches[0][0] == "spmm_rowwise_kernel":
            continue
        for g in c.groups():
            xv, yv = vec_flags(c.prec, g, c.xw, c.yw, c.x_off, c.y_off)
            if xv and yv:
                cov.setdefault((c.prec, g.width, g.form, "vec"), []).append(c.name)
            if not xv and not yv:
                cov.setdefault((c.prec, g.width, g.form, "novec"), []).append(c.name)
            if g.count >= 2:
                cov.setdefault((c.prec, g.width, g.form, "groups>=2"), []).append(c.name)
    return cov


def required_keys():
    req = []
    for prec, w, form in KERNELS:
        for axpby in (False, True):
            for nt in (False, True):
                req.append((prec, w, form, axpby, nt))
        if w > 1:
            req += [(prec, w, form, "vec"), (prec, w, form, "novec")]
    for prec in ("f32", "f64"):
        req += [(prec, 0, "rowwise", False, False), (prec, 0, "rowwise", True, False)]
        # (a call takes its groups of 16 first, so at most one group of 8 is ever left: the slot form of width 8 never loops)
        req.append((prec, 16, "slot", "groups>=2"))
    req += [("f32", 16, "pack", "groups>=2"), ("f64", 8, "pack", "groups>=2")]
    return req
