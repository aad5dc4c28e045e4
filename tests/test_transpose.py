"""The device CSR transpose and the transposed CsrMV (include/mspmv.h: mspmv_csr_transpose_*, mspmv_csr_transpose_values_*,
mspmv_csrmv_transpose_*; merge_spmv_amd.csr_transpose / CsrTranspose / csrmv(transpose=True)).  CPU: exports and size-query
conventions.  GPU: the conversion is bit for bit the stable transpose built on the host (numpy's stable argsort; torch's stable sort
on the device for the large matrices), deterministic across streams; A^T x is bit for bit the forward call on the host-built
transpose and within the strict bound of the fp64 oracle."""
import ctypes
import zlib

import numpy as np
import pytest

import merge_spmv_amd as M
from oracle import oracle as O

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

NEW = ["mspmv_csr_transpose_f32", "mspmv_csr_transpose_f64", "mspmv_csr_transpose_values_f32", "mspmv_csr_transpose_values_f64",
       "mspmv_csrmv_transpose_f32", "mspmv_csrmv_transpose_f64"]
MAX_ITEMS = 2 ** 31 - 1 - 65536


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_transpose_symbols_are_declared_and_exported():
    import os
    import re
    import subprocess
    from conftest import ROOT
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mspmv.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", M.library_path("product")], capture_output=True, text=True, check=True).stdout
    lib = M.load_library()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert f" T {name}\n" in out + "\n", name
        assert hasattr(lib, name)
    assert lib.mspmv_version() == 102


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_transpose_size_query_conventions(prec):
    lib = M.load_library()
    fn = getattr(lib, "mspmv_csr_transpose_" + prec)
    size = ctypes.c_size_t(0)
    call = lambda temp, sz, rows, cols, nnz, fake=None: fn(temp, ctypes.byref(sz), fake, fake, fake, rows, cols, nnz, fake, fake, fake, None,
                                                            None, 0)
    assert call(None, size, 1000, 1000, 50000) == 0 and size.value > 0
    need = size.value
    # more columns -> more digit passes -> never less storage
    big = ctypes.c_size_t(0)
    assert call(None, big, 1000, 1 << 20, 50000) == 0 and big.value >= need
    for rows, cols, nnz in ((0, 0, 0), (0, 7, 0), (7, 0, 0), (5, 5, 0), (5, 1, 9)):
        assert call(None, size, rows, cols, nnz) == 0 and size.value > 0
    # too small / misaligned temp storage; missing arrays; negative sizes; nonzeros without rows or columns
    fake = ctypes.c_void_p(4096)
    small = ctypes.c_size_t(need - 1)
    assert call(ctypes.c_void_p(256), small, 1000, 1000, 50000, fake) == 1
    enough = ctypes.c_size_t(need + 64)
    for misaligned in (4096 + 1, 4096 + 4, 4096 + 8):
        assert call(ctypes.c_void_p(misaligned), enough, 1000, 1000, 50000, fake) == 1
    assert call(ctypes.c_void_p(4096), enough, 1000, 1000, 50000, None) == 1
    for rows, cols, nnz in ((-1, 5, 5), (5, -1, 5), (5, 5, -1), (0, 5, 5), (5, 0, 5)):
        assert call(None, size, rows, cols, nnz) == 1, (rows, cols, nnz)
    assert fn(None, None, None, None, None, 5, 5, 5, None, None, None, None, None, 0) == 1
    # only one of values / values_t given
    vfn = getattr(lib, "mspmv_csr_transpose_values_" + prec)
    assert vfn(None, None, None, 0, None, 0) == 0
    assert vfn(None, fake, fake, 10, None, 0) == 1 and vfn(fake, fake, fake, -1, None, 0) == 1


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_transposed_csrmv_size_query_conventions(prec):
    lib = M.load_library()
    fn = getattr(lib, "mspmv_csrmv_transpose_" + prec)
    size = ctypes.c_size_t(0)
    call = lambda temp, sz, rows, cols, nnz, fake=None: fn(temp, ctypes.byref(sz), fake, fake, fake, fake, fake, rows, cols, nnz, 1.0, 0.0,
                                                            None, 0)
    assert call(None, size, 1000, 3000, 50000) == 0
    need = size.value
    # at least the transpose's own temp storage plus A^T's arrays and the forward call's temp storage for A^T
    tsz, fsz = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert getattr(lib, "mspmv_csr_transpose_" + prec)(None, ctypes.byref(tsz), None, None, None, 1000, 3000, 50000, None, None, None, None,
                                                        None, 0) == 0
    assert getattr(lib, "mspmv_csrmv_axpby_" + prec)(None, ctypes.byref(fsz), None, None, None, None, None, 3000, 1000, 50000, 1.0, 0.0,
                                                      None, 0) == 0
    vb = 4 if prec == "f32" else 8
    assert need >= tsz.value + fsz.value + 50000 * (4 + vb) + 3001 * 4
    fake = ctypes.c_void_p(4096)
    assert call(ctypes.c_void_p(256), ctypes.c_size_t(need - 1), 1000, 3000, 50000, fake) == 1
    for misaligned in (4096 + 1, 4096 + 4, 4096 + 8):
        assert call(ctypes.c_void_p(misaligned), ctypes.c_size_t(need + 64), 1000, 3000, 50000, fake) == 1
    for rows, cols, nnz in ((-1, 5, 5), (5, -1, 5), (5, 5, -1)):
        assert call(None, size, rows, cols, nnz) == 1
    # A^T's rows + nnz = cols + nnz must stay within the forward call's int32 path bound (rows of A do not count)
    assert call(None, size, 1000, 1000, MAX_ITEMS - 1000) == 0
    assert call(None, size, 1000, 1001, MAX_ITEMS - 1000) == 1
    assert call(None, size, 2 ** 30, 5, 2 ** 30) == 0
    assert call(None, size, 5, 2 ** 30, 2 ** 30) == 1


# ---------------------------------------------------------------------------------------------------------------- host references
def host_transpose(csr):
    """the stable transpose: entries sorted by column, ties in their order in A"""
    lens = np.diff(csr.row_offsets.astype(np.int64))
    rows_of = np.repeat(np.arange(csr.rows, dtype=np.int32), lens)
    perm = np.argsort(csr.column_indices, kind="stable").astype(np.int32)
    off_t = np.zeros(csr.cols + 1, np.int64)
    np.cumsum(np.bincount(csr.column_indices, minlength=csr.cols), out=off_t[1:])
    return O.Csr(csr.cols, csr.rows, off_t.astype(np.int32), rows_of[perm], csr.values[perm]), perm


def _csr(rng, rows, cols, lens, dtype, sort_cols=True, col_pool=None):
    off = np.zeros(rows + 1, np.int64); np.cumsum(np.asarray(lens, np.int64), out=off[1:])
    nnz = int(off[-1])
    col = (rng.integers(0, cols, nnz) if col_pool is None else rng.choice(col_pool, nnz)).astype(np.int32)
    if sort_cols:
        for r in np.nonzero(np.diff(off) > 1)[0]:
            col[off[r]:off[r + 1]].sort()
    return O.Csr(rows, cols, off.astype(np.int32), col, rng.uniform(-1, 1, nnz).astype(dtype))


SHAPES = {          # (the families of tests/test_prepared_plan.py)
    "short_rows": lambda rng: (20000, 50000, rng.integers(0, 12, 20000)),
    "power_law": lambda rng: (8000, 30000, np.minimum((rng.pareto(1.1, 8000) * 2).astype(np.int64), 20000)),
    "giant_row": lambda rng: (3000, 100000, np.where(np.arange(3000) == 1500, 300000, rng.integers(0, 3, 3000))),
    "mostly_empty": lambda rng: (40000, 7000, np.where(np.arange(40000) % 97 == 0, 50, 0)),
    "all_empty": lambda rng: (500, 500, np.zeros(500, np.int64)),
    "single_col": lambda rng: (5000, 1, rng.integers(0, 3, 5000)),
    "tiny": lambda rng: (3, 5, np.array([2, 0, 1])),
}


def _matrix(name, dtype):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if name in SHAPES:
        rows, cols, lens = SHAPES[name](rng)
        return _csr(rng, rows, cols, lens, dtype)
    if name == "unsorted_duplicates":
        csr = _csr(rng, 9000, 40000, rng.integers(0, 30, 9000), dtype, sort_cols=False)
        c = csr.column_indices
        c[1::3] = c[0:-1:3][: len(c[1::3])]              # every third entry repeats its predecessor's column
        return csr
    if name == "empty_rows_and_columns":
        return _csr(rng, 6000, 9000, np.where(rng.random(6000) < 0.4, 0, rng.integers(1, 20, 6000)), dtype,
                    col_pool=rng.choice(9000, 2500, replace=False))
    if name == "rows0":
        return O.Csr(0, 17, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, dtype))
    if name == "cols0":
        return O.Csr(17, 0, np.zeros(18, np.int32), np.zeros(0, np.int32), np.zeros(0, dtype))
    if name == "nnz0":
        return O.Csr(300, 400, np.zeros(301, np.int32), np.zeros(0, np.int32), np.zeros(0, dtype))
    if name == "cols1":
        return _csr(rng, 7000, 1, rng.integers(0, 4, 7000), dtype)
    if name == "dense_row":
        lens = rng.integers(0, 4, 64); lens[9] = 12000
        csr = _csr(rng, 64, 12000, lens, dtype)
        csr.column_indices[csr.row_offsets[9]:csr.row_offsets[10]] = np.arange(12000, dtype=np.int32)
        return csr
    if name.startswith("cols_"):                          # digit-pass boundaries: the largest column is present
        cols = int(name[5:])
        csr = _csr(rng, 3000, cols, rng.integers(0, 40, 3000), dtype)
        csr.column_indices[-1] = cols - 1
        return csr
    raise KeyError(name)


BOUNDARY = [255, 256, 257, 2047, 2049, 65536, 65537, (1 << 24) + 1]
MATRICES = sorted(SHAPES) + ["unsorted_duplicates", "empty_rows_and_columns", "rows0", "cols0", "nnz0", "cols1", "dense_row"] + \
    [f"cols_{c}" for c in BOUNDARY]


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check_equal(got, want_csr, want_perm, with_values=True):
    vt, ot, ct, perm = got
    assert np.array_equal(ot.cpu().numpy(), want_csr.row_offsets)
    assert np.array_equal(ct.cpu().numpy(), want_csr.column_indices)
    assert np.array_equal(perm.cpu().numpy(), want_perm)
    if with_values:
        assert vt.dtype == _d(want_csr.values).dtype
        assert np.array_equal(vt.cpu().numpy().view(np.uint8), want_csr.values.view(np.uint8))       # bit for bit
    else:
        assert vt is None


# ---------------------------------------------------------------------------------------------------------------- GPU: structure
@gpu
@pytest.mark.parametrize("name", MATRICES)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_transpose_is_the_stable_host_transpose(name, prec):
    dtype = np.float32 if prec == "f32" else np.float64
    csr = _matrix(name, dtype)
    want, perm = host_transpose(csr)
    got = M.csr_transpose(_d(csr.values), _d(csr.row_offsets), _d(csr.column_indices), csr.cols)
    torch.cuda.synchronize()
    _check_equal(got, want, perm)
    # structure only (either precision's entry point): the same structure and permutation, no values
    got = M.csr_transpose(None, _d(csr.row_offsets), _d(csr.column_indices), csr.cols)
    torch.cuda.synchronize()
    _check_equal(got, want, perm, with_values=False)


def _device_reference(A):
    """the stable transpose on the device (torch's stable sort) for matrices too large for numpy loops"""
    key = A.column_indices.to(torch.int64)
    perm = torch.sort(key, stable=True).indices
    lens = (A.row_offsets[1:] - A.row_offsets[:-1]).to(torch.int64)
    rows_of = torch.repeat_interleave(torch.arange(A.rows, dtype=torch.int32, device=key.device), lens)
    off_t = torch.zeros(A.cols + 1, dtype=torch.int64, device=key.device)
    off_t[1:] = torch.cumsum(torch.bincount(key, minlength=A.cols), 0)
    return A.values[perm], off_t.to(torch.int32), rows_of[perm], perm.to(torch.int32)


def _check_device(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w)


@gpu
@pytest.mark.parametrize("kind", ["rmat", "uniform"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_transpose_large_matrices(kind, prec):
    from merge_spmv_amd import generators as G
    tdt = torch.float32 if prec == "f32" else torch.float64
    A = G.rmat_csr(18, 4_000_000, dtype=tdt) if kind == "rmat" else G.uniform_csr(250_000, 1_000_000, 16, dtype=tdt)
    got = M.csr_transpose(A.values, A.row_offsets, A.column_indices, A.cols)
    _check_device(got, _device_reference(A))


# ---------------------------------------------------------------------------------------------------------------- GPU: determinism, refresh
@gpu
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_transpose_is_deterministic_across_streams(prec):
    from merge_spmv_amd import generators as G
    tdt = torch.float32 if prec == "f32" else torch.float64
    A = G.rmat_csr(16, 1_000_000, dtype=tdt)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        a = M.csr_transpose(A.values, A.row_offsets, A.column_indices, A.cols, stream=s1)
    with torch.cuda.stream(s2):
        b = M.csr_transpose(A.values, A.row_offsets, A.column_indices, A.cols, stream=s2)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@gpu
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_refresh_values_equals_a_fresh_conversion(prec):
    dtype = np.float32 if prec == "f32" else np.float64
    csr = _matrix("power_law", dtype)
    t = M.CsrTranspose(_d(csr.values), _d(csr.row_offsets), _d(csr.column_indices), csr.cols)
    new = np.random.default_rng(5).uniform(-2, 2, csr.nnz).astype(dtype)
    t.refresh_values(_d(new))
    fresh = M.csr_transpose(_d(new), _d(csr.row_offsets), _d(csr.column_indices), csr.cols)
    torch.cuda.synchronize()
    assert torch.equal(t.values_t, fresh[0]) and torch.equal(t.row_offsets_t, fresh[1]) and torch.equal(t.column_indices_t, fresh[2])
    with pytest.raises(M.MspmvError):
        t.refresh_values(_d(new[:-1]))


# ---------------------------------------------------------------------------------------------------------------- GPU: A^T x
def _forward_on_host_transpose(ct, x, alpha, beta, y0):
    y = _d(y0.copy()) if y0 is not None else None
    return M.csrmv(_d(ct.values), _d(ct.row_offsets), _d(ct.column_indices), x, y, num_cols=ct.cols, alpha=alpha, beta=beta)


@gpu
@pytest.mark.parametrize("name", ["short_rows", "power_law", "giant_row", "mostly_empty", "all_empty", "single_col", "tiny",
                                  "unsorted_duplicates", "empty_rows_and_columns", "nnz0", "cols1", "dense_row", "cols_65537"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_transposed_csrmv_bitwise_and_oracle(name, prec):
    dtype, tdt = (np.float32, torch.float32) if prec == "f32" else (np.float64, torch.float64)
    csr = _matrix(name, dtype)
    ct, _ = host_transpose(csr)
    rng = np.random.default_rng(11)
    x = _d(rng.uniform(-1, 1, csr.rows).astype(dtype))
    v, o, c = _d(csr.values), _d(csr.row_offsets), _d(csr.column_indices)
    t = M.CsrTranspose(v, o, c, csr.cols)
    # y = A^T x: the stateless call, the built transpose and the forward call on the host-built transpose, bit for bit;
    # beta == 0 never reads y (NaN prefill)
    want = _forward_on_host_transpose(ct, x, 1.0, 0.0, None)
    y_nan = torch.full((csr.cols,), float("nan"), dtype=tdt, device="cuda")
    got = M.csrmv(v, o, c, x, y_nan, num_cols=csr.cols, transpose=True)
    got_t = t(x, torch.full((csr.cols,), float("nan"), dtype=tdt, device="cuda"))
    torch.cuda.synchronize()
    assert torch.equal(got, want) and torch.equal(got_t, want)
    # within the strict bound of the fp64 oracle
    g, s = O.spmv_gold_acc64(ct, x.cpu().numpy())
    ok, worst = O.strict_check(ct, got.cpu().numpy(), g, s, items_per_thread=M.serial_sum_depth(ct.rows, ct.cols, ct.nnz, ct.values.dtype.itemsize))
    assert ok, (name, prec, worst)
    # alpha / beta
    y0 = rng.uniform(-1, 1, csr.cols).astype(dtype)
    want = _forward_on_host_transpose(ct, x, -0.5, 3.0, y0)
    got = M.csrmv(v, o, c, x, _d(y0.copy()), num_cols=csr.cols, transpose=True, alpha=-0.5, beta=3.0)
    got_t = t(x, _d(y0.copy()), alpha=-0.5, beta=3.0)
    torch.cuda.synchronize()
    assert torch.equal(got, want) and torch.equal(got_t, want)


@gpu
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_transposed_csrmv_stream_tiny_x_and_matmul(prec):
    dtype, tdt = (np.float32, torch.float32) if prec == "f32" else (np.float64, torch.float64)
    rng = np.random.default_rng(3)
    # 500 rows of A: x (A^T's x) is at most 4 KB, gathered from LDS by the forward call
    csr = _csr(rng, 500, 20000, rng.integers(0, 60, 500), dtype)
    ct, _ = host_transpose(csr)
    x = _d(rng.uniform(-1, 1, csr.rows).astype(dtype))
    v, o, c = _d(csr.values), _d(csr.row_offsets), _d(csr.column_indices)
    want = _forward_on_host_transpose(ct, x, 1.0, 0.0, None)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        got = M.csrmv(v, o, c, x, num_cols=csr.cols, transpose=True, stream=s)
    s.synchronize()
    assert torch.equal(got, want)
    # CsrTranspose.matmul is csrmm on the host-built transpose
    X = _d(rng.uniform(-1, 1, (csr.rows, 4)).astype(dtype))
    t = M.CsrTranspose(v, o, c, csr.cols)
    Y = t.matmul(X)
    Yw = M.csrmm(_d(ct.values), _d(ct.row_offsets), _d(ct.column_indices), X)
    torch.cuda.synchronize()
    assert torch.equal(Y, Yw)


@gpu
def test_transposed_csrmv_rejects_bad_tensors():
    rng = np.random.default_rng(9)
    csr = _csr(rng, 300, 700, rng.integers(0, 5, 300), np.float32)
    v, o, c = _d(csr.values), _d(csr.row_offsets), _d(csr.column_indices)
    x = _d(rng.uniform(-1, 1, 300).astype(np.float32))
    with pytest.raises(M.MspmvError):                       # x needs A's rows entries, not its cols
        M.csrmv(v, o, c, x[:299], num_cols=700, transpose=True)
    with pytest.raises(M.MspmvError):                       # y needs A's cols entries
        M.csrmv(v, o, c, x, torch.empty(300, dtype=torch.float32, device="cuda"), num_cols=700, transpose=True)
    with pytest.raises(M.MspmvError):
        M.csrmv(v, o, c, x.double(), num_cols=700, transpose=True)
    with pytest.raises(M.MspmvError):
        M.csr_transpose(v, o, c.to(torch.int64), 700)
    assert M.csrmv(v, o, c, x, num_cols=700, transpose=True).shape == (700,)


# ---------------------------------------------------------------------------------------------------------------- GPU: C2 at full size
@gpu
def test_transpose_headline_matrix_at_full_size():
    """BASELINE config 2 (3 125 000^2, 32 per row, 10^8 nonzeros, fp32): the structure is torch's stable sort, and A^T x passes the
    sampled check of the benchmark records."""
    from merge_spmv_amd import generators as G
    A = G.uniform_csr(3_125_000, 3_125_000, 32, dtype=torch.float32)
    got = M.csr_transpose(A.values, A.row_offsets, A.column_indices, A.cols)
    _check_device(got, _device_reference(A))
    x = G.uniform_pm1(G.SEED_C2 + 2, A.rows, torch.float32, "cuda")
    y = M.csrmv(A.values, A.row_offsets, A.column_indices, x, num_cols=A.cols, transpose=True)
    At = G.DeviceCsr(A.cols, A.rows, got[1], got[2], got[0])
    rec = M.sampled_check(At, x, y)
    assert rec["violations"] == 0 and rec["worst_ratio"] < 1.0, rec
    t = M.CsrTranspose(A.values, A.row_offsets, A.column_indices, A.cols)
    assert torch.equal(t(x), y)
