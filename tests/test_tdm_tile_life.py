"""What a clocked tile does outside its gather rotation (csrc/mspmv_tdm.hpp): every thread's first chunk of row ends is requested with
the nonzero stream and staged before the rotation, the other chunks behind the gathers, by tiles of more than 1024 - eshift rows only;
the band of a sorted entry comes from two band starts read per window (a walk beyond them); the products are formed from x values that
passed through the product array.  None of it may change one bit of y: the harness is tests/test_tdm.py's -- development library, the
clocked form forced by set_tdm under every clock of CLOCKS, the reference taken from the classic one-sweep kernel on the same tile
shape -- and y is compared as bit patterns (NaNs included)."""
import numpy as np
import pytest

import merge_spmv_amd as M
from oracle import oracle as O

import test_tdm as T

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

SHAPES = [("f32", 11), ("f64", 11), ("f64", 7)]
COLS = 60000            # 30 bands of 2048 columns under the narrowest clock of CLOCKS, one band under the default


def _types(prec):
    return (np.float32, torch.float32, 4) if prec == "f32" else (np.float64, torch.float64, 8)


def _csr(rng, lens, cols, dtype):
    lens = np.asarray(lens, np.int64)
    off = np.zeros(len(lens) + 1, np.int64); np.cumsum(lens, out=off[1:])
    nnz = int(off[-1])
    col = rng.integers(0, cols, nnz).astype(np.int32)
    return O.Csr(len(lens), cols, off.astype(np.int32), col, rng.uniform(-1, 1, nnz).astype(dtype))


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _rows_per_tile(csr, ipt):
    """rows that END in each merge-path tile of 256 * ipt items (row end r sits at path position r + row_end[r])"""
    pos = np.arange(csr.rows, dtype=np.int64) + csr.row_offsets[1:].astype(np.int64)
    return np.bincount(pos // (256 * ipt))


def _check(csr, x, prec, ipt, axpby=False, seed=0):
    """the clocked form under every clock of CLOCKS against the classic one-sweep kernel, bit patterns of y"""
    dtype, tdt, vb = _types(prec)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    val, off, col, dx = d(csr.values), d(csr.row_offsets), d(csr.column_indices), d(x)
    ws = M.CsrMVWorkspace(csr.rows, csr.nnz, tdt)
    y0 = np.random.default_rng(seed).uniform(-1, 1, csr.rows).astype(dtype)
    try:
        T._classic(vb, ipt)
        ref = torch.full((csr.rows,), float("nan"), dtype=tdt, device="cuda")
        M.csrmv(val, off, col, dx, y=ref, num_cols=csr.cols, workspace=ws)
        ref_ab = d(y0.copy())
        if axpby:
            M.csrmv(val, off, col, dx, y=ref_ab, num_cols=csr.cols, workspace=ws, alpha=-1.5, beta=0.5)
        torch.cuda.synchronize()
        for slot, look, shift in T.CLOCKS:
            T._clocked(vb, ipt, slot, look, shift)
            assert M.band_passes(csr.rows, csr.cols, csr.nnz, vb) == 3, "the clocked form is not what runs"
            y = torch.full((csr.rows,), float("nan"), dtype=tdt, device="cuda")
            M.csrmv(val, off, col, dx, y=y, num_cols=csr.cols, workspace=ws)
            diff = int((_bits(y) != _bits(ref)).sum())
            assert diff == 0, (prec, ipt, slot, look, shift, diff)
            if axpby:
                yab = d(y0.copy())
                M.csrmv(val, off, col, dx, y=yab, num_cols=csr.cols, workspace=ws, alpha=-1.5, beta=0.5)
                diff = int((_bits(yab) != _bits(ref_ab)).sum())
                assert diff == 0, (prec, ipt, slot, look, shift, "alpha/beta", diff)
        return ref
    finally:
        T._reset()


def _boundary_matrix(rng, dtype):
    # lengths 1, 2, 2, 2: 1.75 nonzeros per row, 2.75 path items -- a 256 x 11 tile ends 1024 rows, give or take a few
    return _csr(rng, rng.choice([1, 2, 2, 2], 40000), COLS, dtype)


@gpu
@pytest.mark.parametrize("prec,ipt", SHAPES)
def test_row_end_branch_boundary(prec, ipt):
    """tiles on both sides of the early / late row-end branch (1024 - eshift rows), with alpha and beta too"""
    dtype, _, _ = _types(prec)
    rng = np.random.default_rng(100 + ipt)
    csr = _boundary_matrix(rng, dtype)
    if ipt == 11:
        per_tile = _rows_per_tile(csr, ipt)[:-1]
        assert (per_tile <= 1020).any() and (per_tile > 1024).any(), (per_tile.min(), per_tile.max())
    _check(csr, rng.uniform(-1, 1, COLS).astype(dtype), prec, ipt, axpby=True)


@gpu
@pytest.mark.parametrize("prec,ipt", SHAPES)
def test_every_tile_takes_its_row_ends_late(prec, ipt):
    """rows of 0 and 1 nonzeros, and a stretch of empty rows long enough for tiles of nothing but row ends (every chunk of every thread)"""
    dtype, _, _ = _types(prec)
    rng = np.random.default_rng(200 + ipt)
    lens = rng.integers(0, 2, 60000)
    lens[30000:39000] = 0
    csr = _csr(rng, lens, COLS, dtype)
    per_tile = _rows_per_tile(csr, ipt)[:-1]
    assert per_tile.min() > (1024 if ipt == 11 else 0) and per_tile.max() == 256 * ipt, (per_tile.min(), per_tile.max())
    _check(csr, rng.uniform(-1, 1, COLS).astype(dtype), prec, ipt)


@gpu
@pytest.mark.parametrize("prec,ipt", SHAPES)
def test_special_values_at_the_gather(prec, ipt):
    """x with +-inf, NaN and -0.0 at a few columns of one band, values 0 and -0.0 on those columns: the products are the bits the classic
    kernel's multiply produces (0 * inf = NaN, -0.0 * x, NaN payloads), through the same reduction"""
    dtype, _, _ = _types(prec)
    rng = np.random.default_rng(300 + ipt)
    csr = _csr(rng, rng.integers(0, 41, 3000), COLS, dtype)
    x = rng.uniform(-1, 1, COLS).astype(dtype)
    special = {4100: np.inf, 4101: -np.inf, 4200: np.nan, 4300: -0.0, 5000: np.inf, 5001: np.nan, 5002: -0.0, 5003: -np.inf}     # band 2 of 2048 columns
    for c, v in special.items():
        x[c] = v
    # a good number of nonzeros on those columns, some of them with the values 0 and -0.0
    pick = rng.choice(csr.nnz, 600, replace=False)
    csr.column_indices[pick] = rng.choice(list(special), 600).astype(np.int32)
    csr.values[pick[:150]] = 0.0
    csr.values[pick[150:300]] = -0.0
    ref = _check(csr, x, prec, ipt)
    refh = ref.cpu().numpy()
    assert np.isnan(refh).any() and np.isfinite(refh).any()


def _ragged_matrix(rng, ipt, dtype):
    """nnz % 4 != 0, (rows + 1) % 4 != 0, and a last tile of about twenty path items"""
    rows, tile = 30002, 256 * ipt
    lens = rng.integers(0, 41, rows).astype(np.int64)
    lens[-5:] = 3
    rem = next(r for r in (17, 18, 19, 20) if (r - rows) % 4 != 0)           # nnz = k * tile + rem - rows, tile a multiple of 4
    lens[0] += (rem - (rows + int(lens.sum()))) % tile
    csr = _csr(rng, lens, 70001, dtype)
    assert csr.nnz % 4 != 0 and (csr.rows + 1) % 4 != 0 and (csr.rows + csr.nnz) % tile == rem < 64
    return csr


@gpu
@pytest.mark.parametrize("prec,ipt", SHAPES)
def test_ragged_tails_and_a_tiny_last_tile(prec, ipt):
    dtype, _, _ = _types(prec)
    rng = np.random.default_rng(400 + ipt)
    csr = _ragged_matrix(rng, ipt, dtype)
    _check(csr, rng.uniform(-1, 1, csr.cols).astype(dtype), prec, ipt, axpby=True)


@gpu
def test_graph_replay_of_the_forced_clocked_call():
    dtype, tdt, vb = _types("f32")
    rng = np.random.default_rng(500)
    csr = _boundary_matrix(rng, dtype)
    x = rng.uniform(-1, 1, COLS).astype(dtype)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    val, off, col, dx = d(csr.values), d(csr.row_offsets), d(csr.column_indices), d(x)
    ws = M.CsrMVWorkspace(csr.rows, csr.nnz, tdt)
    try:
        T._classic(vb, 11)
        ref = torch.full((csr.rows,), float("nan"), dtype=tdt, device="cuda")
        M.csrmv(val, off, col, dx, y=ref, num_cols=csr.cols, workspace=ws)
        T._clocked(vb, 11, 0, 0, 11)
        assert M.band_passes(csr.rows, csr.cols, csr.nnz, vb) == 3
        stream = torch.cuda.Stream()
        yg = torch.full((csr.rows,), float("nan"), dtype=tdt, device="cuda")
        with torch.cuda.stream(stream):
            M.csrmv(val, off, col, dx, y=yg, num_cols=csr.cols, workspace=ws)       # warm-up outside the capture
            stream.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                M.csrmv(val, off, col, dx, y=yg, num_cols=csr.cols, workspace=ws)
        yg.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(yg), _bits(ref))
    finally:
        T._reset()
