"""Exact tests at the top of the accepted index range (rows + nnz = MAX_ITEMS = 2^31 - 1 - 65536, cols + nnz for the transpose)
and on arrays over 4 GB, on the formula-defined family of tests/index_range.py: integer values and x, so an fp64 y -- and an fp32
y on rows of at most 2^18 nonzeros -- must equal the exact int64 reference bit for bit whatever the association order.  A
dropped, repeated or misplaced nonzero, a wrong row or a wrong byte offset past 2^31 / 2^32 shows as an exact mismatch.

Every matrix is generated on the device (int64 throughout, chunks of 2^27 nonzeros) in a module-scoped fixture and freed before
the next; each test checks the free device memory against what it needs first.  The non-GPU tests check the helper itself
against the oracle and against Python integers.

Measured on one MI355X: the GPU tests of this file take about 50 s, and torch's allocator peaks at 138 GiB of device memory (the
stateless fp64 A^T x at cols + nnz = MAX_ITEMS asks for 114 GB of scratch, fp32 90 GB; csr_transpose's own scratch is 74 GB in fp32).
"""
import ctypes

import numpy as np
import pytest

from index_range import CHUNK, MAX_ITEMS, Family, mismatch_summary, rows_for, strict_violations

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

TDT = {"f32": torch.float32, "f64": torch.float64}
VB = {"f32": 4, "f64": 8}
FP32_EXACT_LEN = 1 << 18                    # fp32 rows up to this length have every partial sum <= 64 * 2^18 = 2^24: exact
ALPHA, BETA = 3.0, -2.0                     # axpby: y = 3 A x - 2 y0 with y0 small integers -- exact in fp32 while 3 * 64 len + 16 <= 2^24

_SHORT = rows_for(MAX_ITEMS, 7)
_SHORT_R = rows_for(MAX_ITEMS - 1, 7)
_LONG = rows_for(MAX_ITEMS, 2047)
_BAND = rows_for(MAX_ITEMS, 15)
_MM = rows_for(MAX_ITEMS, 127)
PLAN_BANDS = 16                               # the bands CsrMVPlan picks for these x (asserted below)
_PLAN = (MAX_ITEMS + 15) // (PLAN_BANDS + 15) - 1 + (MAX_ITEMS + 15) // (PLAN_BANDS + 15) % 2   # odd: bands * rows + nnz = MAX_ITEMS
_TR_COLS = 1 << 20                            # A: 2^20 - 1 rows, 2^20 columns, nnz = MAX_ITEMS - 2^20: A^T's rows + nnz = MAX_ITEMS
_TR_NNZ = MAX_ITEMS - _TR_COLS

# name: (family, precision, pad): pad = 1 -> values and column indices are views one element into their allocations
SPECS = {
    # short rows at the top: one launch of tile_kernel_snap, non-temporal streams, lean closed tiles; the ragged variant has
    # nnz = 3 mod 4 (the last tile's ragged chunk) and unaligned arrays (the dword-per-lane path)
    "short_top_f64": (Family(_SHORT, 1 << 20, MAX_ITEMS, 7, 7), "f64", 0),
    "short_top_f32": (Family(_SHORT, 1 << 20, MAX_ITEMS, 7, 7), "f32", 0),
    "short_ragged_unaligned_f64": (Family(_SHORT_R, 1 << 20, MAX_ITEMS - 1, 7, 7), "f64", 1),
    "short_ragged_unaligned_f32": (Family(_SHORT_R, 1 << 20, MAX_ITEMS - 1, 7, 7), "f32", 1),
    # one giant row between empty rows: carries over ~760 k tiles
    "giant_f64": (Family(9, 1 << 20, MAX_ITEMS, 0, 0, absorb=4), "f64", 0),
    "giant_f32": (Family(9, 1 << 20, MAX_ITEMS, 0, 0, absorb=4), "f32", 0),
    # rows all long: the classic three launches
    "long_f64": (Family(_LONG, 1 << 20, MAX_ITEMS, 2047, 1024), "f64", 0),
    "long_f32": (Family(_LONG, 1 << 20, MAX_ITEMS, 2047, 1024), "f32", 0),
    # column-band candidates at the top: the clock-scheduled bands of mspmv_tdm.hpp
    "band_f32": (Family(_BAND, 1 << 23, MAX_ITEMS, 15, 7), "f32", 0),
    "band_f64": (Family(_BAND, 1 << 22, MAX_ITEMS, 15, 7), "f64", 0),
    # ... and at the top of what the band-major CsrMVPlan accepts (its bands * rows + nnz <= MAX_ITEMS, include/mspmv.h)
    "band_plan_top_f32": (Family(_PLAN, 1 << 23, MAX_ITEMS - PLAN_BANDS * _PLAN + _PLAN, 15, 7), "f32", 0),
    "band_plan_top_f64": (Family(_PLAN, 1 << 22, MAX_ITEMS - PLAN_BANDS * _PLAN + _PLAN, 15, 7), "f64", 0),
    # x over 4 GB: gathers past byte 2^32 of x
    "wide_x_2p29_f64": (Family((1 << 24) + 1, (1 << 29) + 1, ((1 << 24) + 1) * 17, 16, 8), "f64", 0),
    "wide_x_2p31_f64": (Family((1 << 24) + 1, (1 << 31) - 1, ((1 << 24) + 1) * 17, 16, 8), "f64", 0),
    "wide_x_2p30_f32": (Family((1 << 24) + 1, (1 << 30) + 1, ((1 << 24) + 1) * 17, 16, 8), "f32", 0),
    # SpMM: rows ~2^24 at the top; X over 4 GB (k = 16, fp64)
    "mm_top_f64": (Family(_MM, 1 << 20, MAX_ITEMS, 127, 64), "f64", 0),
    "mm_top_f32": (Family(_MM, 1 << 20, MAX_ITEMS, 127, 64), "f32", 0),
    "mm_wide_x_f64": (Family((1 << 24) + 1, (1 << 25) + 1, ((1 << 24) + 1) * 17, 16, 8), "f64", 0),
    # the transpose at cols + nnz = MAX_ITEMS
    "transpose_f32": (Family(_TR_COLS - 1, _TR_COLS, _TR_COLS - 1 + _TR_NNZ, _TR_NNZ // (_TR_COLS - 2), 1024), "f32", 0),
    "transpose_f64": (Family(_TR_COLS - 1, _TR_COLS, _TR_COLS - 1 + _TR_NNZ, _TR_NNZ // (_TR_COLS - 2), 1024), "f64", 0),
}
FORWARD = [n for n in SPECS if not n.startswith(("mm_", "transpose"))]


def _bytes_needed(fam, vb, extra=0):
    """device bytes the build, the reference and one call need: the CSR arrays, x, y, y_ref / s and their boundary copies,
    the chunk temporaries and the call's own temp storage"""
    return (fam.nnz * (vb + 4) + (fam.rows + 1) * 4 + fam.cols * vb + fam.rows * (3 * vb + 6 * 8) + 12 * CHUNK * 8
            + (1 << 30) + int(extra))


def _room(need, what):
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"{what}: needs {need / 2**30:.1f} GiB of device memory, {free / 2**30:.1f} GiB free of {total / 2**30:.1f}")


class Built:
    def __init__(self, name):
        self.name = name
        self.fam, self.prec, self.pad = SPECS[name]
        self.dtype, self.vb = TDT[self.prec], VB[self.prec]


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: torch.cuda.is_available() is False")
    import merge_spmv_amd as M_
    M_.load_library()          # raises if the HIP extension is missing: no fallback
    return M_


@pytest.fixture(scope="module")
def mat(request, M):
    """one matrix of SPECS on cuda:0 with x and its exact reference; freed when the tests of the next spec begin"""
    b = Built(request.param)
    fam = b.fam
    _room(_bytes_needed(fam, b.vb), b.name)
    b.vals, b.off, b.cols = fam.build(b.dtype, "cuda", pad=b.pad)
    if not b.name.startswith(("mm_", "transpose")):
        b.x = fam.x(b.dtype, "cuda")
        b.y_ref, b.s = fam.reference(b.off)
        b.lens = (b.off[1:] - b.off[:-1]).to(torch.int64)
    torch.cuda.synchronize()
    yield b
    del b.vals, b.off, b.cols
    b.__dict__.clear()
    torch.cuda.empty_cache()


def _assert_y(b, y, y_ref=None, s=None, alpha=1.0, beta=0.0, y0=None, depth=0, what=""):
    """y exact on every row where the arithmetic is exact (fp64; fp32 rows whose partial sums stay <= 2^24), within the strict
    bound of DESIGN.md 3 (exact y_ref and s) on the others"""
    y_ref = b.y_ref if y_ref is None else y_ref
    s = b.s if s is None else s
    if alpha != 1.0 or beta != 0.0:
        y_ref = int(alpha) * y_ref + (int(beta) * y0 if y0 is not None else 0)
        s = abs(int(alpha)) * s + (abs(int(beta)) * y0.abs() if y0 is not None else 0)
    if b.vb == 8 or b.fam.max_len() * 64 * abs(alpha) + 8 * abs(beta) <= 2 ** 24:
        bad = mismatch_summary(y, y_ref, b.off)
        assert bad is None, f"{b.name} {what}: {bad[0]} rows differ from the exact reference; first: row {bad[1]} (nonzeros {bad[2]}): " \
                            f"got {bad[3]!r}, want {bad[4]!r}"
        return
    exact = b.lens * 64 * int(abs(alpha)) + 8 * int(abs(beta)) <= 2 ** 24
    bad = mismatch_summary(torch.where(exact, y.to(torch.float64), y_ref.to(torch.float64)), y_ref, b.off)
    assert bad is None, f"{b.name} {what}: {bad[0]} exact rows differ; first: row {bad[1]} (nonzeros {bad[2]}): got {bad[3]!r}, want {bad[4]!r}"
    n, worst = strict_violations(y, y_ref, s, b.off, depth)
    assert n == 0, f"{b.name} {what}: {n} rows outside the strict bound, worst ratio {worst}"


def _host_cross_check(M, b):
    """the device generator and reference against Python integers on ~100 rows where a wrap would show"""
    fam = b.fam
    info = M.launch_info(fam.rows, fam.nnz, b.vb)
    probe = fam.probe_rows(info["tile_items"], info["num_tiles"])
    rows_t = torch.tensor(probe, dtype=torch.int64, device="cuda")
    got_off = b.off[rows_t].cpu().tolist()
    got_end = b.off[rows_t + 1].cpu().tolist()
    got_y = b.y_ref[rows_t].cpu().tolist()
    got_s = b.s[rows_t].cpu().tolist()
    ks = []
    for r, o, e in zip(probe, got_off, got_end):
        assert (o, e - o) == (fam.offset(r), fam.length(r)), f"{b.name}: row {r}"
        ks.extend(range(o, min(e, o + 4)))
        ks.extend(range(max(o, e - 4), e))
        n = e - o
        if n <= 512:
            assert (got_y[probe.index(r)], got_s[probe.index(r)]) == fam.row_sum(r), f"{b.name}: reference of row {r}"
    ks = sorted(set(ks))
    kt = torch.tensor(ks, dtype=torch.int64, device="cuda")
    assert b.cols[kt].cpu().tolist() == [fam.col(k) for k in ks], f"{b.name}: column indices"
    assert b.vals[kt].cpu().tolist() == [float(fam.value(k)) for k in ks], f"{b.name}: values"
    cs = sorted({fam.col(k) for k in ks} | {0, fam.cols - 1})
    assert b.x[torch.tensor(cs, dtype=torch.int64, device="cuda")].cpu().tolist() == [float(fam.xval(c)) for c in cs]


def _y0(b):
    return b.fam.x_t(torch.arange(b.fam.rows, dtype=torch.int64, device="cuda"), j=7)


# ---------------------------------------------------------------------------------------------------------------------------
# the forward entry points on every shape

@gpu
@pytest.mark.parametrize("mat", FORWARD, indirect=True)
def test_csrmv_entry_points_are_exact_at_the_top(M, mat):
    """The stateless csrmv (plain and alpha / beta), the two-phase DeviceSpmv.CsrMV on exactly the temp size it reports, a prepared
    CsrMVWorkspace (bit for bit the stateless call), and the path each shape means to reach: one launch of row-snapped tiles for
    short rows, the classic launches for long ones, the clocked column bands (with CsrMVPlan) for the band candidates."""
    b, fam = mat, mat.fam
    rows, cols, nnz, vb = fam.rows, fam.cols, fam.nnz, mat.vb
    assert int(b.off[-1]) == nnz and b.vals.numel() == nnz
    if b.name.startswith("band_plan_top"):
        assert PLAN_BANDS * rows + int(b.off[-1]) == MAX_ITEMS
    elif b.name.startswith(("short", "giant", "long", "band")):
        assert rows + int(b.off[-1]) == (MAX_ITEMS - 1 if "ragged" in b.name else MAX_ITEMS)
    if "ragged" in b.name:
        assert nnz % 4 != 0
    if b.pad:
        assert b.vals.data_ptr() % 16 != 0 and b.cols.data_ptr() % 16 != 0
    if b.name.startswith("wide_x"):
        assert cols * vb > (1 << 32)
    _host_cross_check(M, b)
    info = M.launch_info(rows, nnz, vb, num_cols=cols)
    if b.name.startswith("short"):
        assert info["snap_head_max"] > 0, info
    if b.name.startswith(("giant", "long")):
        assert info["snap_head_max"] == 0 and info["fixup_levels"] >= 1, info
    depth = M.serial_sum_depth(rows, cols, nnz, vb)

    y = torch.full((rows,), float("nan"), dtype=b.dtype, device="cuda")
    ws = M.CsrMVWorkspace(rows, nnz, b.dtype)
    M.csrmv(b.vals, b.off, b.cols, b.x, y=y, num_cols=cols, workspace=ws)
    torch.cuda.synchronize()
    _assert_y(b, y, depth=depth, what="stateless csrmv")
    if b.name.startswith("band"):
        assert M.clocked_bands(rows, cols, nnz, vb)[0] > 0
        assert int(M.debug_band_windows(ws, rows, nnz, vb).sum()) == 64, "the windows refused the clocked bands"

    y0 = _y0(b)
    ya = y0.to(b.dtype)
    M.csrmv(b.vals, b.off, b.cols, b.x, y=ya, num_cols=cols, alpha=ALPHA, beta=BETA)
    torch.cuda.synchronize()
    _assert_y(b, ya, alpha=ALPHA, beta=BETA, y0=y0, depth=depth, what="csrmv alpha/beta")
    del ya

    # two-phase: the size the query reports is the size the call needs (no 32-bit truncation of a size_t on the way)
    st, need = M.DeviceSpmv.CsrMV(None, 0, b.vals, b.off, b.cols, b.x, y, rows, cols, nnz)
    assert st == 0 and need == info["temp_bytes"]
    tmp = torch.empty(need, dtype=torch.uint8, device="cuda")
    y2 = torch.full_like(y, float("nan"))
    st, _ = M.DeviceSpmv.CsrMV(tmp, need, b.vals, b.off, b.cols, b.x, y2, rows, cols, nnz)
    assert st == 0
    torch.cuda.synchronize()
    assert torch.equal(y, y2)
    del tmp, y2

    wsp = M.CsrMVWorkspace(rows, nnz, b.dtype).prepare(b.off)
    yp = torch.full_like(y, float("nan"))
    M.csrmv(b.vals, b.off, b.cols, b.x, y=yp, num_cols=cols, workspace=wsp)
    torch.cuda.synchronize()
    assert torch.equal(y, yp), "the prepared call differs from the stateless call"
    del yp, wsp

    if b.name.startswith("band") and not b.name.startswith("band_plan_top"):
        # the plan stacks its bands as rows: at rows + nnz = MAX_ITEMS it refuses before touching memory (include/mspmv.h)
        with pytest.raises(M.MspmvError, match="hipError 1 "):
            M.CsrMVPlan(b.vals, b.off, b.cols, cols)
    if b.name.startswith("band_plan_top"):
        plan = M.CsrMVPlan(b.vals, b.off, b.cols, cols)
        assert plan.bands == PLAN_BANDS
        yq = torch.full_like(y, float("nan"))
        plan(b.x, yq)
        torch.cuda.synchronize()
        _assert_y(b, yq, depth=M.serial_sum_depth(rows, cols, nnz, vb, extra=plan.bands), what="CsrMVPlan")
        del plan, yq


# ---------------------------------------------------------------------------------------------------------------------------
# the forced dispatch paths on the short-row and giant-row shapes

def _forced_paths():
    from test_gpu_parity import PATHS
    paths = {n: PATHS[n] for n in ("classic_three_launch", "classic_multilevel_fix", "reference_walk", "one_launch_nontemporal",
                                   "classic_nontemporal", "one_launch_general_reduction", "one_launch_general_reduction_nontemporal",
                                   "classic_interp_coords", "classic_search_kernel")}
    paths["one_launch_temporal"] = PATHS["one_launch_large_shape"] | 64          # MSPMV_TUNE_FORCE_TEMPORAL (mspmv_dev.h)
    return paths


FORCED = _forced_paths()


@gpu
@pytest.mark.parametrize("path", sorted(FORCED))
@pytest.mark.parametrize("mat", ["short_top_f64", "short_top_f32", "giant_f64", "giant_f32"], indirect=True)
def test_forced_paths_are_exact_at_the_top(M, mat, path):
    """Every dispatch path of test_gpu_parity.PATHS that serves these sizes -- the classic three launches, the multi-level fix-up,
    the reference walk, non-temporal and temporal streams, the general reduction -- exact at rows + nnz = MAX_ITEMS."""
    b, fam = mat, mat.fam
    try:
        M.set_tuning(b.vb, 0, 0, FORCED[path])
        y = torch.full((fam.rows,), float("nan"), dtype=b.dtype, device="cuda")
        M.csrmv(b.vals, b.off, b.cols, b.x, y=y, num_cols=fam.cols)
        torch.cuda.synchronize()
        _assert_y(b, y, depth=M.serial_sum_depth(fam.rows, fam.cols, fam.nnz, b.vb), what=path)
    finally:
        M.set_tuning(b.vb)


# ---------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("mat", ["wide_x_2p31_f64", "wide_x_2p30_f32"], indirect=True)
def test_hot_columns_on_x_over_4gb(M, mat):
    """CsrMVHotColumns with x in either order on an x of more than 4 GB (its order / permutation arrays span up to 2^31 - 1
    columns): exact, and bit for bit the stateless call."""
    b, fam = mat, mat.fam
    assert fam.cols * b.vb > (1 << 32)
    size = ctypes.c_size_t(0)
    assert M.load_library().mspmv_csrmv_hotcols_size(fam.rows, fam.cols, fam.nnz, b.vb, ctypes.byref(size)) == 0
    _room(int(size.value) + fam.cols * b.vb + fam.rows * b.vb * 3, f"{b.name} hot-column plan")
    y = M.csrmv(b.vals, b.off, b.cols, b.x, num_cols=fam.cols)
    plan = M.CsrMVHotColumns(b.vals, b.off, b.cols, fam.cols)
    yh = torch.full_like(y, float("nan"))
    plan(b.x, yh)
    torch.cuda.synchronize()
    _assert_y(b, yh, what="hot columns")
    assert torch.equal(y, yh)
    # the renumbering is a permutation of all cols columns (the unreferenced ones included), and permute() is x[order]
    order = plan.order().to(torch.int64)
    assert order.numel() == fam.cols
    assert int(order.min()) >= 0 and int(order.max()) < fam.cols, "order entry out of range"
    seen = torch.bincount(order, minlength=fam.cols)
    missing = int((seen == 0).sum())
    assert missing == 0, f"order is not a permutation: {missing} columns missing, {int((seen > 1).sum())} repeated; " \
                         f"first missing column {int(torch.nonzero(seen == 0)[0])}"
    del seen
    xp = plan.permute(b.x)
    for lo in range(0, fam.cols, 1 << 28):
        hi = min(lo + (1 << 28), fam.cols)
        assert torch.equal(xp[lo:hi], b.x[order[lo:hi]]), f"permute() differs from x[order] in columns [{lo}, {hi})"
    del order
    yp = torch.full_like(y, float("nan"))
    plan(xp, yp, x_is_permuted=True)
    torch.cuda.synchronize()
    assert torch.equal(y, yp), "the hot-column plan on a permuted x differs from the stateless call"
    del plan, xp, yp, yh, y


# ---------------------------------------------------------------------------------------------------------------------------
# SpMM

def _mm_reference(b, k):
    """X[:, j] = x_{j mod 4} * (1 + j // 4); the exact Y column by column from four int64 references"""
    fam = b.fam
    X = torch.empty(fam.cols, k, dtype=b.dtype, device="cuda")
    refs = []
    for j in range(min(k, 4)):
        X[:, j] = fam.x(b.dtype, "cuda", j=j)
        refs.append(fam.reference(b.off, j=j))
    for j in range(4, k):
        X[:, j] = X[:, j % 4] * (1 + j // 4)
    return X, refs


@gpu
@pytest.mark.parametrize("mat", ["mm_top_f64", "mm_top_f32", "mm_wide_x_f64"], indirect=True)
def test_csrmm_is_exact_at_the_top(M, mat):
    """csrmm with k = 1, 4, 16 at rows + nnz = MAX_ITEMS, and with an X of more than 4 GB (cols = 2^25 + 1, k = 16, fp64), which
    must take the packs rather than the slot form (mspmv_api.hip: csrmm_impl's 32-bit byte offsets into X)."""
    b, fam = mat, mat.fam
    rows, cols, nnz = fam.rows, fam.cols, fam.nnz
    if b.name.startswith("mm_top"):
        assert rows + nnz == MAX_ITEMS
    b.lens = (b.off[1:] - b.off[:-1]).to(torch.int64)
    ks = (16,) if "wide" in b.name else (1, 4, 16)
    _room(rows * 16 * (b.vb + 8 * 2) + cols * 16 * b.vb + (8 << 30), b.name)
    X, refs = _mm_reference(b, max(ks))
    for k in ks:
        x_bytes = cols * k * b.vb
        slot_form = x_bytes < (1 << 32) and rows + nnz >= (8 << 20)            # the branch condition of csrmm_impl
        if "wide" in b.name:
            assert not slot_form and rows + nnz >= (8 << 20) and x_bytes >= (1 << 32)
        Xk = X[:, :k].contiguous() if k < X.shape[1] else X
        Y = torch.full((rows, k), float("nan"), dtype=b.dtype, device="cuda")
        M.csrmm(b.vals, b.off, b.cols, Xk, Y=Y)
        torch.cuda.synchronize()
        for j in range(k):
            y_ref, s = refs[j % 4]
            _assert_y(b, Y[:, j].contiguous(), y_ref=y_ref * (1 + j // 4), s=s * (1 + j // 4),
                      depth=M.serial_sum_depth(rows, cols, nnz, b.vb), what=f"csrmm k={k} column {j}")
        del Xk, Y
    del X, refs


# ---------------------------------------------------------------------------------------------------------------------------
# the transpose

def _hash_entries(row, col, v):
    from merge_spmv_amd.generators import splitmix64
    return splitmix64(0x7A5E, row * (1 << 31) + col) ^ v


@gpu
@pytest.mark.parametrize("mat", ["transpose_f32", "transpose_f64"], indirect=True)
def test_transpose_at_the_top(M, mat):
    """csrmv(transpose=True) and csr_transpose at cols + nnz = MAX_ITEMS.  A^T x is exact against the column-wise int64 reference;
    A^T's structure is checked without a sort of 2^31 entries: row_offsets_t is the running bincount of the columns, the entries
    of each row of A^T are in A's order (non-decreasing rows, increasing permutation), the permutation maps every entry onto an
    entry of A with that row and column (so it is a permutation) and values_t = values[permutation]; an order-free fingerprint
    of (row, col, value) agrees between A and A^T.  Scratch of the stateless A^T x: 90 GB (fp32) / 114 GB (fp64); of
    csr_transpose: 74 GB / 90 GB."""
    b, fam = mat, mat.fam
    rows, cols, nnz, vb, dev = fam.rows, fam.cols, fam.nnz, mat.vb, "cuda"
    assert cols + nnz == MAX_ITEMS
    lib = M.load_library()
    ct = ctypes.c_float if vb == 4 else ctypes.c_double
    fn = lib.mspmv_csrmv_transpose_f32 if vb == 4 else lib.mspmv_csrmv_transpose_f64
    size = ctypes.c_size_t(0)
    assert fn(None, ctypes.byref(size), None, None, None, None, None, rows, cols, nnz, ct(1), ct(0), None, 0) == 0
    mv_scratch = int(size.value)
    assert mv_scratch >= nnz * (vb + 4) > (1 << 32)           # A^T's values and indices alone: not truncated to 32 bits

    # A^T x against the column-wise reference
    xr = fam.x(b.dtype, dev, j=1, n=rows)
    xr64 = fam.x_t(torch.arange(rows, dtype=torch.int64, device=dev), j=1)
    yt_ref = torch.zeros(cols, dtype=torch.int64, device=dev)
    counts = torch.zeros(cols, dtype=torch.int64, device=dev)
    fp_a = 0
    for lo, hi in fam.chunks():
        k = torch.arange(lo, hi, dtype=torch.int64, device=dev)
        r = fam.rows_t(k, b.off)
        c = b.cols[lo:hi].to(torch.int64)
        p = fam.values_t(k) * xr64[r]
        yt_ref.index_add_(0, c, p)
        counts += torch.bincount(c, minlength=cols)
        fp_a += int(_hash_entries(r, c, fam.values_t(k)).sum())
        del k, r, c, p
    off_t_ref = torch.zeros(cols + 1, dtype=torch.int64, device=dev)
    off_t_ref[1:] = torch.cumsum(counts, 0)
    assert int(counts.max()) * 64 <= 2 ** 24           # every row of A^T short enough for an exact fp32 sum
    del counts
    _room(mv_scratch + cols * vb * 2 + (2 << 30), f"{b.name} stateless A^T x")
    y = torch.full((cols,), float("nan"), dtype=b.dtype, device=dev)
    M.csrmv(b.vals, b.off, b.cols, xr, y=y, num_cols=cols, transpose=True)
    torch.cuda.synchronize()
    bad = mismatch_summary(y, yt_ref, off_t_ref)
    assert bad is None, f"{b.name} A^T x: {bad[0]} rows of A^T differ; first: column {bad[1]} (entries {bad[2]}): got {bad[3]!r}, want {bad[4]!r}"
    del y
    torch.cuda.empty_cache()
    if vb == 8:
        return                     # fp64: the structure is the same as fp32's (csr_transpose's scratch + A^T would exceed ~150 GB)

    _room(fam.nnz * (vb + 8) + 74 * (1 << 30), f"{b.name} csr_transpose")
    values_t, off_t, cols_t, perm = M.csr_transpose(b.vals, b.off, b.cols, cols)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    assert torch.equal(off_t.to(torch.int64), off_t_ref), "row_offsets_t is not the running bincount of the columns"
    fp_t = 0
    starts = torch.zeros(nnz + 1, dtype=torch.bool, device=dev)
    starts[off_t_ref] = True
    for lo, hi in fam.chunks():
        q = torch.arange(lo, hi, dtype=torch.int64, device=dev)
        c = torch.searchsorted(off_t, q.to(torch.int32), right=True).to(torch.int64) - 1         # the row of A^T = the column of A
        r = cols_t[lo:hi].to(torch.int64)
        k = perm[lo:hi].to(torch.int64)
        assert bool(((k >= 0) & (k < nnz)).all()), "permutation entry out of range"
        assert torch.equal(fam.rows_t(k, b.off), r), "permutation does not map onto an entry of A's row"
        assert torch.equal(b.cols[k].to(torch.int64), c), "permutation does not map onto an entry of A's column"
        assert torch.equal(values_t[lo:hi], b.vals[k]), "values_t != values[permutation]"
        # within a row of A^T (no row start between q and q + 1): rows non-decreasing, permutation increasing (stable)
        if hi - lo > 1:
            inner = ~starts[lo + 1:hi]
            assert bool((r[1:] >= r[:-1])[inner].all()), "rows of A decrease inside a row of A^T"
            assert bool((k[1:] > k[:-1])[inner].all()), "the permutation is not increasing inside a row of A^T"
        if lo > 0 and not bool(starts[lo]):
            assert int(perm[lo - 1]) < int(perm[lo]) and int(cols_t[lo - 1]) <= int(cols_t[lo])
        fp_t += int(_hash_entries(r, c, fam.values_t(k)).sum())
        del q, c, r, k
    assert (fp_a - fp_t) % (1 << 64) == 0, "the fingerprints of (row, col, value) of A and A^T differ"
    del values_t, off_t, cols_t, perm, starts


# ---------------------------------------------------------------------------------------------------------------------------
# the helper itself (no GPU)

def _small_families():
    return [Family(301, 97, 301 + 7 * 300 + 5, 7, 7),                    # short rows, ragged absorbing row
            Family(9, 50, 9 + 4000, 0, 0, absorb=4),                        # one long row between empty rows
            Family(61, 1000, 61 + 60 * 40 + 3, 40, 40, absorb=13),          # empty rows inside, absorbing row in the middle
            Family(rows_for(20000, 3), 5, 20000, 3, 2)]                    # duplicate columns (rows longer than cols)


@pytest.mark.parametrize("i", range(4))
def test_helper_matches_the_oracle_and_python_ints(i):
    """The family on torch CPU: row offsets from the closed formula equal the running sum of the lengths, columns stay in range and
    never decrease within a row, columns 0 and cols - 1 appear, the values are nonzero integers in [-8, 8]; the chunked reference
    (chunks far smaller than a row, so the carries matter) equals oracle.spmv_gold_acc64 exactly and Python-integer sums."""
    import index_range
    from oracle import oracle as O
    fam = _small_families()[i]
    vals, off, cols = fam.build(torch.float64, "cpu")
    x = fam.x(torch.float64, "cpu")
    assert int(off[-1]) == fam.nnz and fam.rows + fam.nnz == fam.items
    lens = [fam.length(r) for r in range(fam.rows)]
    assert off.tolist() == [0] + list(np.cumsum(lens)) and min(lens) >= 0
    assert [fam.offset(r) for r in range(fam.rows + 1)] == off.tolist()
    c = cols.numpy().astype(np.int64)
    assert c.min() == 0 and c.max() == fam.cols - 1 and 0 in c and fam.cols - 1 in c
    for r in range(fam.rows):
        seg = c[off[r]:off[r + 1]]
        assert (np.diff(seg) >= 0).all()
    v = vals.numpy()
    assert (v != 0).all() and (np.abs(v) <= 8).all() and (v == np.round(v)).all()
    assert c.tolist() == [fam.col(k) for k in range(fam.nnz)]
    assert v.tolist() == [fam.value(k) for k in range(fam.nnz)]
    old = index_range.CHUNK
    try:
        index_range.CHUNK = 37                    # chunks far shorter than a row: the carries between chunks matter
        y_ref, s = fam.reference(off)
    finally:
        index_range.CHUNK = old
    y_one, s_one = fam.reference(off)             # (one chunk)
    assert torch.equal(y_ref, y_one) and torch.equal(s, s_one)
    csr = O.Csr(fam.rows, fam.cols, off.numpy(), cols.numpy(), v)
    g, sg = O.spmv_gold_acc64(csr, x.numpy())
    assert np.array_equal(y_ref.numpy().astype(np.float64), g)
    assert np.array_equal(s.numpy().astype(np.float64), sg)
    for r in fam.probe_rows(16, (fam.items + 15) // 16, extra=8):
        assert (int(y_ref[r]), int(s[r])) == fam.row_sum(r)
    # the strict-bound helper: the exact y passes, a y one off on one row does not (fp32: 2^-24 relative is far below 1)
    assert strict_violations(y_ref.to(torch.float32), y_ref, s, off, 0)[0] == 0
    assert mismatch_summary(y_ref.to(torch.float64), y_ref, off) is None
    yb = y_ref.to(torch.float64).clone(); yb[fam.g] += 1
    assert mismatch_summary(yb, y_ref, off)[:2] == (1, fam.g)


def test_host_formulas_near_2_31():
    """Python-integer formulas at the top of the range: the offsets of a family at MAX_ITEMS are monotone across item 2^30 and
    2^31 - 2^16, end at nnz, and the probe rows cover the places a wrap would hit."""
    fam = SPECS["short_top_f64"][0]
    assert fam.rows + fam.nnz == MAX_ITEMS and 0 <= fam.absorb_len <= 2 * fam.mid + 1
    assert fam.offset(fam.rows) == fam.nnz and fam.offset(0) == 0
    for item in (1 << 30, fam.nnz - (1 << 16), fam.nnz - 1):
        r = fam.row_of(item)
        assert fam.offset(r) <= item < fam.offset(r + 1)
    for name, (f, prec, _) in SPECS.items():
        assert f.offset(f.rows) == f.nnz and f.absorb_len >= 0, name
        if prec == "f32" and not name.startswith(("giant", "transpose")):
            # fp32 rows exact except the absorbing row of a shape that says so
            assert f.mid + f.spread <= FP32_EXACT_LEN, name
    probe = fam.probe_rows(2816, (MAX_ITEMS + 2815) // 2816)
    assert 0 in probe and fam.rows - 1 in probe and len(probe) >= 60
