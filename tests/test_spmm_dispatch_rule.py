"""No GPU: the test-side restatement of csrmm's dispatch rule (tests/spmm_forms.py) against the library's size query, the coverage
of the compiled kernel forms by the CASES table that tests/test_spmm_forms.py runs on the device, and the shapes the structured
matrices of that file promise to every tile size."""
import ctypes

import numpy as np
import pytest

import merge_spmv_amd as M
import spmm_forms as F


def _query(prec, rows, cols, nnz, k, ldx, ldy):
    lib = M.load_library()
    fn = lib.mspmv_csrmm_f32 if prec == "f32" else lib.mspmv_csrmm_f64
    size = ctypes.c_size_t(0)
    st = fn(None, ctypes.byref(size), None, None, None, None, ldx, None, ldy, rows, cols, nnz, k, 1.0, 0.0, None, 0)
    assert st == 0, (prec, rows, cols, nnz, k, ldx, ldy, st)
    return int(size.value)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_restated_temp_layout_equals_the_size_query(prec):
    """Every k from 1 to 49, contiguous and padded X, on both sides of every threshold of the rule: X at 1 MiB and one row more,
    rows + nnz at 8 Mi - 1 and 8 Mi, X one row below 4 GB and at 4 GB."""
    eb = F.ELEM[prec]
    rows = 1000
    seen = set()
    for k in range(1, 50):
        for ldx in (k, k + 3):
            row_bytes = ldx * eb
            c1 = (1 << 20) // row_bytes                      # the most rows of X within 1 MiB
            c4 = -(-(1 << 32) // row_bytes)                  # the fewest that make 4 GB
            assert c1 * row_bytes <= (1 << 20) < (c1 + 1) * row_bytes and (c4 - 1) * row_bytes < (1 << 32) <= c4 * row_bytes
            for items in (50_000, (8 << 20) - 1, 8 << 20):
                nnz = items - rows
                for cols in (1000, c1, c1 + 1, c4 - 1, c4):
                    if k == 1 and ldx == 1:
                        assert F.expected_launches(prec, rows, cols, nnz, 1, 1, 1) == F.CSRMV
                        continue
                    want = F.temp_bytes(prec, rows, cols, nnz, k, ldx)
                    got = _query(prec, rows, cols, nnz, k, ldx, k)
                    assert got == want, f"{prec} rows={rows} cols={cols} nnz={nnz} k={k} ldx={ldx}: the library asks for {got}, the rule says {want}"
                    seen.add(F.flags(prec, rows, cols, nnz, ldx)[:2])
                    seen.update((g.form, g.tile) for g in F.groups_of(prec, rows, cols, nnz, k, ldx))
                    assert got % 256 == 0
    assert {(False, False), (True, False), (False, True), (True, True)} <= seen          # (wide, slot form allowed)
    assert {("pack", F.TILE_NARROW), ("pack", F.TILE_PACK32), ("pack", F.TILE_PACK64), ("slot", F.TILE_SLOT)} <= seen


def test_restated_rule_on_the_cases_and_on_known_calls():
    for c in F.CASES:
        rows, cols, nnz = c.dims()
        assert _query(c.prec, rows, cols, nnz, c.k, c.xw, c.yw) == F.temp_bytes(c.prec, rows, cols, nnz, c.k, c.xw), c.name
    # what tests/test_abi_exports.py and include/mspmv.h say in words
    assert [g.width for g in F.groups_of("f32", 1000, 1000, 50000, 16, 16)] == [4]                     # X of 64 KB: 16-byte packs
    assert [(g.width, g.tile) for g in F.groups_of("f32", 1000, 10_000_000, 50000, 16, 16)] == [(16, F.TILE_PACK64)]
    assert [(g.width, g.form) for g in F.groups_of("f64", 1_000_000, 1000, 9_000_000, 16, 16)] == [(16, "slot")]
    assert [(g.width, g.form, g.tile) for g in F.groups_of("f64", 1000, 10_000_000, 50000, 31, 31)] == \
        [(8, "pack", F.TILE_PACK64), (4, "pack", F.TILE_PACK32), (2, "pack", F.TILE_NARROW), (1, "pack", F.TILE_NARROW)]
    e = F.expected_launches("f32", 1000, 10_000_000, 50000, 24, 24, 24, True, 1.0, 0.0)
    assert [x[0] for x in e] == ["coords_scatter_kernel", "spmm_tile_kernel", "spmm_fixup_kernel"] * 2
    assert e[1][1:5] == (133, 128, 16, 1) and e[4][1:5] == (67, 256, 8, 1) and e[0][1:3] == (1, 256)
    assert F.expected_launches("f32", 2, 10, 50, 4, 4, 4, True, 1.0, 0.0) == [("spmm_rowwise_kernel", 1, 256, 0, 1, False, False)]
    assert F.expected_launches("f32", 100, 10, 50, 4, 4, 4, False, 2.0, 0.0)[0][5] is True
    assert F.expected_launches("f32", 0, 10, 0, 4, 4, 4) == []
    # a call takes its groups of 16 first: never two groups of 8 in the slot form
    for prec in ("f32", "f64"):
        for k in range(1, 200):
            assert all(g.count == 1 for g in F.groups_of(prec, 1000, 1000, 9_000_000, k, k) if g.form == "slot" and g.width == 8)


def test_cases_cover_every_compiled_form():
    """Every (precision, width, form) kernel the library compiles, with alpha / beta off and on and temporal / non-temporal loads;
    the row-wise kernel; aligned and unaligned X / Y for every width > 1; several groups per launch."""
    cov = F.coverage(F.CASES)
    missing = [key for key in F.required_keys() if key not in cov]
    assert not missing, "no case of CASES runs: " + ", ".join(map(str, missing))
    # nothing else is reachable: a key outside the 13 kernels means the rule (or the table) is wrong
    kernels = set(F.KERNELS)
    assert all(key[:3] in kernels or key[2] == "rowwise" for key in cov)
    # every tile size sees every ragged tail of the arrays
    tails = {}
    for c in F.CASES:
        rows, _, nnz = c.dims()
        assert (rows + 1) % 4 != 0 and nnz % 4 != 0, c.name
        if c.pad == 0 and c.mat != "tiny":
            for g in c.groups():
                assert g.tile in F.structure(c.mat).tiles, f"{c.name}: tile size {g.tile} runs on a matrix not built for it"
                tails.setdefault(g.tile, set()).add(nnz % 4)
    assert tails == {t: {1, 2, 3} for t in F.TILE_ORDER}, tails
    for c in F.CONTAINMENT:
        assert c.alpha != 1 and c.beta != 0
    assert sorted({(c.prec, c.groups()[0].form) for c in F.CONTAINMENT}) == [("f32", "pack"), ("f32", "slot"), ("f64", "pack"), ("f64", "slot")]
    # the 4 GB cases are what they claim; the X of every slot case is below
    for c in F.CASES:
        if "4gb" in c.name:
            assert c.cols * c.xw * F.ELEM[c.prec] >= 1 << 32 and all(g.form == "pack" and g.tile != F.TILE_NARROW for g in c.groups())


@pytest.mark.parametrize("drop", ["mid_wide_groups_f32", "huge_packs_4gb_nt_axpby_f64", "tiny_rowwise_f32"])
def test_coverage_names_what_a_dropped_case_covered_alone(drop):
    cov = F.coverage([c for c in F.CASES if c.name != drop])
    missing = [key for key in F.required_keys() if key not in cov]
    want = {"mid_wide_groups_f32": ("f32", 16, "pack", "groups>=2"), "huge_packs_4gb_nt_axpby_f64": ("f64", 8, "pack", True, True),
            "tiny_rowwise_f32": ("f32", 0, "rowwise", False, False)}[drop]
    assert want in missing


def _tile_coords(off, T):
    """merge-path coordinates (rows consumed, nonzeros consumed) at every tile boundary: row r is consumed at path item
    off[r + 1] + r + 1"""
    rows, nnz = off.size - 1, int(off[-1])
    ends = off[1:] + np.arange(1, rows + 1)
    d = np.minimum(np.arange(0, F.num_tiles(rows, nnz, T) + 1, dtype=np.int64) * T, rows + nnz)
    x = np.searchsorted(ends, d, side="right")
    return x, d - x


@pytest.mark.parametrize("name", ["mid", "big", "huge"])
def test_structured_matrices_hold_what_each_tile_size_needs(name):
    s = F.structure(name)
    lens, off = s.lens, s.offsets()
    rows = s.rows
    start = off[:-1] + np.arange(rows)                   # first path item of each row
    empty = lens == 0
    run = np.diff(np.flatnonzero(np.diff(np.concatenate(([0], empty.view(np.int8), [0])))))[::2]
    g = int(np.argmax(lens))
    assert lens[g] == s.giant and not lens[g - 50:g].any() and not lens[g + 1:g + 51].any()           # a giant row between empty rows
    for T in s.tiles:
        assert run.max() > T                                                                          # empty rows: more than a tile
        assert np.any((lens == T - 1) & (start % T == 0))                                             # a row that is exactly one tile
        assert np.any(lens == T)
        assert np.any((lens > 0) & ((start + lens) % T == 0))                                         # last nonzero = last item of a tile
        assert np.any((lens > 0) & ((start + lens + 1) % T == 0))                                     # row end = last item of a tile
        assert lens[g] > (F.FIXUP_CHUNK + 2) * T                                                      # carries over more than a fix-up block's chunk
        x, y = _tile_coords(off, T)
        # the last row is open at the end of the last tile: that tile starts inside it
        assert x[-2] == rows - 1 and y[-2] > off[-2] and lens[-1] > 2 * T
        # the tile of equal rows: every row ends on a share boundary of 64 slots, every second one of 32
        t = s.marks[(T, "share_ends")] // T
        assert s.marks[(T, "share_ends")] % T == 0 and x[t + 1] - x[t] == 64
        tile_nnz = int(y[t + 1] - y[t])
        rel = off[x[t] + 1:x[t + 1] + 1] - y[t]
        for ns in (64, 32):
            bounds = {tile_nnz * i // ns for i in range(1, ns + 1)}
            assert sum(int(e) in bounds for e in rel) >= ns
        # rows over several shares that end inside a later share
        t = s.marks[(T, "multi_share")] // T
        tile_nnz = int(y[t + 1] - y[t])
        rel = off[x[t]:x[t + 1] + 1] - y[t]
        share = tile_nnz / 32
        long = [(a, b) for a, b in zip(rel[:-1], rel[1:]) if b - a > 2 * share and (b * 64) % tile_nnz != 0]
        assert long, (name, T)
        # a tile with fewer nonzeros than slots
        t = s.marks[(T, "sparse_tile")] // T
        assert 0 < y[t + 1] - y[t] < 32 and x[t + 1] - x[t] > T - 32
    for trim in (0, 1, 2):
        assert s.nnz(trim) % 4 == 3 - trim and s.offsets(trim)[-1] == s.nnz(trim)
    assert (rows + 1) % 4 != 0
