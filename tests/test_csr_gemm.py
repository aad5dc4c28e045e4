"""C = A * B on the device (include/mspmv.h: mspmv_csr_gemm_products, mspmv_csr_gemm_*; merge_spmv_amd.csr_gemm / CsrGemm /
csr_gemm_products).  CPU: exports, size-query conventions, the wrappers' argument checks, and the host model (tests/gemm_model.py)
pinned to hand-written cases.  GPU: every comparison is exact -- offsets, count, the first nnz_c columns and values bit for bit, the
entries past the count and the guard words around every output array untouched.  Expected values never come from the code under
test."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import merge_spmv_amd as M
from conftest import ROOT, load_golden
from gemm_model import count_products, gemm_by_rows, host_gemm

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

NEW = ["mspmv_csr_gemm_products", "mspmv_csr_gemm_f32", "mspmv_csr_gemm_f64"]
MAX_ITEMS = 2 ** 31 - 1 - 65536
TILE, SCAN_CHUNK = 2048, 4096                                    # products per expansion tile; entries per block of the scan
COUNTS = [0, 1, 2047, 2048, 2049, 4095, 4096, 4097, 3 * 2048 + 5]


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_gemm_symbols_are_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mspmv.h")).read(), flags=re.S)
    lib = M.load_library()
    for kind in ("product", "dev"):
        out = subprocess.run(["nm", "-D", "--defined-only", M.library_path(kind)], capture_output=True, text=True, check=True).stdout
        for name in NEW:
            assert f" T {name}\n" in out + "\n", (kind, name)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    for name in ("csr_gemm", "CsrGemm", "csr_gemm_products"):
        assert name in M.__all__ and callable(getattr(M, name))
    assert lib.mspmv_version() == 102


def _call(lib, prec, temp, size, rows, inner, cols, na, nb, products, cap, f=None, va="f", vb="f", vc="f"):
    fn = getattr(lib, "mspmv_csr_gemm_" + prec)
    pick = lambda v: f if v == "f" else v
    return fn(temp, ctypes.byref(size), rows, inner, cols, pick(va), f, f, na, pick(vb), f, f, nb, products, cap, pick(vc), f, f, f, None, 0)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_gemm_size_query_conventions(prec):
    lib = M.load_library()
    vbytes = 4 if prec == "f32" else 8
    fake = ctypes.c_void_p(4096)
    size = ctypes.c_size_t(0)
    ok = (1000, 900, 800, 50000, 30000, 400000, 400000)
    assert _call(lib, prec, None, size, *ok) == 0 and size.value > 0
    need = size.value
    assert need % 16 == 0
    # the layout the header states: the triples, the sort's sets, the sorted entries and the compression's words, per product
    assert 400000 * (8 + vbytes) * 2 < need < 400000 * (16 * vbytes + 64)
    assert _call(lib, prec, None, size, 1000, 900, 800, 50000, 30000, 400000, 0) == 0 and size.value == need      # (capacity has no say)
    for shape in ((0, 0, 0, 0, 0, 0, 0), (0, 7, 7, 0, 0, 0, 0), (7, 0, 7, 0, 0, 0, 0), (7, 7, 0, 0, 0, 0, 0), (5, 5, 5, 0, 0, 0, 0),
                  (5, 5, 5, 5, 0, 0, 0), (5, 5, 5, 5, 5, 0, 0), (1, 1, 1, 1, 1, 1, 1)):
        assert _call(lib, prec, None, size, *shape) == 0 and size.value > 0, shape
    # too small / misaligned temp storage; missing arrays; negative sizes
    assert _call(lib, prec, ctypes.c_void_p(256), ctypes.c_size_t(need - 1), *ok, fake) == 1
    for misaligned in (4096 + 1, 4096 + 4, 4096 + 8):
        assert _call(lib, prec, ctypes.c_void_p(misaligned), ctypes.c_size_t(need + 64), *ok, fake) == 1
    assert _call(lib, prec, ctypes.c_void_p(4096), ctypes.c_size_t(need + 64), *ok, None) == 1
    for k in range(7):
        bad = list(ok); bad[k] = -1
        assert _call(lib, prec, None, size, *bad) == 1, bad
    fn = getattr(lib, "mspmv_csr_gemm_" + prec)
    assert fn(None, None, 5, 5, 5, None, None, None, 5, None, None, None, 5, 5, 5, None, None, None, None, None, 0) == 1
    # entries together with a zero dimension
    for shape in ((0, 5, 5, 5, 0, 0, 0), (5, 0, 5, 5, 0, 0, 0), (5, 0, 5, 0, 5, 0, 0), (5, 5, 0, 0, 5, 0, 0), (5, 5, 0, 0, 0, 5, 5), (0, 5, 5, 0, 0, 5, 5),
                  (5, 0, 5, 0, 0, 5, 5), (0, 5, 5, 0, 5, 0, 0), (5, 5, 0, 5, 0, 0, 0)):
        assert _call(lib, prec, None, size, *shape) == 1, shape
    # each limit at its edge and one past it: rows + products, rows + nnz_a, inner + nnz_b
    top = MAX_ITEMS - 1000
    assert _call(lib, prec, None, size, 1000, 1000, 1000, 10, 10, top, 0) == 0
    assert _call(lib, prec, None, size, 1000, 1000, 1000, 10, 10, top + 1, 0) == 1
    assert _call(lib, prec, None, size, 1001, 1000, 1000, 10, 10, top, 0) == 1
    assert _call(lib, prec, None, size, 1000, 1000, 1000, top, 10, 10, 10) == 0
    assert _call(lib, prec, None, size, 1000, 1000, 1000, top + 1, 10, 10, 10) == 1
    assert _call(lib, prec, None, size, 1000, 1000, 1000, 10, top, 10, 10) == 0
    assert _call(lib, prec, None, size, 1000, 1000, 1000, 10, top + 1, 10, 10) == 1
    assert _call(lib, prec, None, size, 1000, 1001, 1000, 10, top, 10, 10) == 1
    assert _call(lib, prec, None, size, 1000, 1000, 1 << 30, 10, 10, 10, 10) == 0                # (columns do not count)
    assert _call(lib, prec, None, size, 10, 10, 10, 10, 10, 10, MAX_ITEMS) == 0                  # (nor does the capacity)
    # values for some matrices and not for the others (refused before anything is launched)
    big = lambda: ctypes.c_size_t(1 << 30)
    for va, vb, vc in ((None, "f", "f"), ("f", None, "f"), ("f", "f", None), (None, None, "f"), ("f", None, None), (None, "f", None)):
        assert _call(lib, prec, fake, big(), 5, 5, 5, 5, 5, 5, 5, fake, va, vb, vc) == 1, (va, vb, vc)


def test_gemm_products_size_query_conventions():
    lib = M.load_library()
    fn = lib.mspmv_csr_gemm_products
    fake = ctypes.c_void_p(4096)
    size = ctypes.c_size_t(0)
    assert fn(None, ctypes.byref(size), None, None, 1000, 900, 50000, None, 30000, None, None, 0) == 0 and size.value > 0
    need = size.value
    assert need % 16 == 0 and need < 50000                       # per block of A's entries, not per entry
    assert fn(None, ctypes.byref(size), None, None, 0, 0, 0, None, 0, None, None, 0) == 0 and size.value > 0
    assert fn(ctypes.c_void_p(256), ctypes.byref(ctypes.c_size_t(need - 1)), fake, fake, 1000, 900, 50000, fake, 30000, fake, None, 0) == 1
    for misaligned in (4096 + 1, 4096 + 4, 4096 + 8):
        assert fn(ctypes.c_void_p(misaligned), ctypes.byref(ctypes.c_size_t(need + 64)), fake, fake, 1000, 900, 50000, fake, 30000, fake, None, 0) == 1
    assert fn(fake, ctypes.byref(ctypes.c_size_t(need)), fake, fake, 1000, 900, 50000, fake, 30000, None, None, 0) == 1
    assert fn(None, None, None, None, 5, 5, 5, None, 5, None, None, 0) == 1
    for shape in ((-1, 5, 5, 5), (5, -1, 5, 5), (5, 5, -1, 5), (5, 5, 5, -1), (0, 5, 5, 5), (5, 0, 5, 0), (5, 0, 0, 5), (0, 5, 0, 5)):
        rows, inner, na, nb = shape
        assert fn(None, ctypes.byref(size), None, None, rows, inner, na, None, nb, None, None, 0) == 1, shape
    top = MAX_ITEMS - 1000
    assert fn(None, ctypes.byref(size), None, None, 1000, 1000, top, None, top, None, None, 0) == 0
    assert fn(None, ctypes.byref(size), None, None, 1000, 1000, top + 1, None, top, None, None, 0) == 1
    assert fn(None, ctypes.byref(size), None, None, 1000, 1000, top, None, top + 1, None, None, 0) == 1


def test_gemm_wrappers_reject_bad_tensors_without_a_device():
    from merge_spmv_amd.generators import DeviceCsr
    off = torch.zeros(4, dtype=torch.int32)
    col = torch.zeros(0, dtype=torch.int32)
    cpu = DeviceCsr(3, 3, off, col, None)
    for call in (M.csr_gemm, M.CsrGemm, M.csr_gemm_products):
        with pytest.raises(M.MspmvError):
            call(cpu, cpu)                                       # not on the device


def _f(x, t):
    return np.asarray(x, t)


def test_the_model_on_hand_written_cases():
    f = np.float32
    i = lambda x: np.asarray(x, np.int32)
    # 1. [[1, 2], [0, 3]] * [[4, 0, 5], [0, 6, 7]] = [[4, 12, 19], [0, 18, 21]]
    a = (i([0, 2, 3]), i([0, 1, 1]), _f([1, 2, 3], f))
    b = (i([0, 2, 4]), i([0, 2, 1, 2]), _f([4, 5, 6, 7], f))
    for off, col, val in (gemm_by_rows(2, a, b, f), host_gemm(2, 3, a, b, f)):
        assert off.tolist() == [0, 3, 5] and col.tolist() == [0, 1, 2, 1, 2] and val.tolist() == [4.0, 12.0, 19.0, 18.0, 21.0] and val.dtype == f
    assert count_products(a, b) == 6
    # 2. empty rows of A and of B anywhere, unsorted rows, a repeated column in A and in B: row 1 of A = (col 2, col 0, col 2);
    #    B row 0 = (3: 1), row 1 empty, row 2 = (3: 10, 0: 20, 3: 30) -> C[1, 3] = 2*10 + 2*30 + 5*1 + 7*10 + 7*30, in that order
    a = (i([0, 0, 3, 3, 4]), i([2, 0, 2, 1]), _f([2, 5, 7, 9], f))
    b = (i([0, 1, 1, 4]), i([3, 3, 0, 3]), _f([1, 10, 20, 30], f))
    for off, col, val in (gemm_by_rows(4, a, b, f), host_gemm(4, 4, a, b, f)):
        assert off.tolist() == [0, 0, 2, 2, 2] and col.tolist() == [0, 3] and val.tolist() == [40.0 + 140.0, 20.0 + 60.0 + 5.0 + 70.0 + 210.0]
    assert count_products(a, b) == 7
    off, col, val = gemm_by_rows(4, (a[0], a[1], None), (b[0], b[1], None))
    assert off.tolist() == [0, 0, 2, 2, 2] and col.tolist() == [0, 3] and val is None
    assert host_gemm(4, 4, (a[0], a[1], None), (b[0], b[1], None))[2] is None
    # 3. +x and -x meet: the entry stays, +0.0; a lone product of -0.0 stays -0.0
    a = (i([0, 2, 3]), i([0, 1, 0]), _f([1.5, -1.5, -0.0], f))
    b = (i([0, 1, 2]), i([4, 4]), _f([2.0, 2.0], f))
    for off, col, val in (gemm_by_rows(2, a, b, f), host_gemm(2, 5, a, b, f)):
        assert off.tolist() == [0, 1, 2] and col.tolist() == [4, 4]
        assert val.tolist() == [0.0, 0.0] and not np.signbit(val[0]) and np.signbit(val[1])
    # 4. the order of the adds: (2^24 + 1) - 2^24 = 0 in fp32 left to right, 1 in any order that cancels first
    big = 2.0 ** 24
    a = (i([0, 3]), i([0, 1, 2]), _f([big, 1.0, -big], f))
    b = (i([0, 1, 2, 3]), i([0, 0, 0]), _f([1.0, 1.0, 1.0], f))
    assert gemm_by_rows(1, a, b, f)[2].tolist() == [0.0] and host_gemm(1, 1, a, b, f)[2].tolist() == [0.0]
    a2 = (a[0], i([0, 2, 1]), _f([big, -big, 1.0], f))
    assert gemm_by_rows(1, a2, b, f)[2].tolist() == [1.0] and host_gemm(1, 1, a2, b, f)[2].tolist() == [1.0]
    # 5. every product rounded before it is added: (-1 * 1) + (3 * fl(1/3)) = -1 + 1 = 0, where a fused multiply-add would keep the
    #    rounding error of fl(1/3)
    for t in (np.float32, np.float64):
        third = t(1.0) / t(3.0)
        a = (i([0, 2]), i([0, 1]), _f([-1.0, 3.0], t))
        b = (i([0, 1, 2]), i([0, 0]), _f([1.0, third], t))
        assert gemm_by_rows(1, a, b, t)[2].tolist() == [0.0] and host_gemm(1, 1, a, b, t)[2].tolist() == [0.0]
        assert float(Fraction(3) * Fraction(float(third)) - 1) != 0.0
    # and host_gemm against the model on random matrices that are not canonical
    rng = np.random.default_rng(1)
    for dtype in (np.float32, np.float64):
        for rows, inner, cols, na, nb in ((37, 23, 53, 400, 300), (5, 1, 7, 40, 6), (1, 9, 1, 30, 20), (20, 20, 20, 0, 50), (20, 20, 20, 50, 0)):
            A, B = _random_csr(rng, rows, inner, na, dtype), _random_csr(rng, inner, cols, nb, dtype)
            got, want = host_gemm(rows, cols, A, B, dtype), gemm_by_rows(rows, A, B, dtype)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            assert got[2].dtype == want[2].dtype == dtype and got[2].tobytes() == want[2].tobytes()
            assert count_products(A, B) == sum(int(B[0][c + 1] - B[0][c]) for c in A[1])


def _fma_case(dtype, n=512):
    """A = one row (a1, a2) over B's two rows of n columns each: C[0, j] = a1 * b1[j] + a2 * b2[j]"""
    rng = np.random.default_rng(77)
    a = rng.uniform(1, 2, 2).astype(dtype)
    b = rng.uniform(1, 2, 2 * n).astype(dtype)
    A = (np.array([0, 2], np.int32), np.array([0, 1], np.int32), a)
    B = (np.array([0, n, 2 * n], np.int32), np.tile(np.arange(n, dtype=np.int32), 2), b)
    return A, B, n


def test_the_fma_case_tells_fused_from_unfused():
    for dtype in (np.float32, np.float64):
        t = np.dtype(dtype).type
        A, B, n = _fma_case(dtype)
        unfused = host_gemm(1, n, A, B, dtype)[2]
        p1 = A[2][0] * B[2][:n]
        fused = np.array([t(float(Fraction(float(A[2][1])) * Fraction(float(x)) + Fraction(float(y)))) for x, y in zip(B[2][n:], p1)], dtype)
        assert np.array_equal(unfused, p1 + A[2][1] * B[2][n:]) and (fused != unfused).sum() > 10, dtype


# ---------------------------------------------------------------------------------------------------------------- matrices
def _random_csr(rng, rows, cols, nnz, dtype, canonical=False):
    """any valid CSR: rows not sorted, columns may repeat (canonical=True: sorted rows, no repeats)"""
    if rows == 0 or cols == 0:
        nnz = 0
    r = np.sort(rng.integers(0, max(rows, 1), nnz))
    c = rng.integers(0, max(cols, 1), nnz)
    if canonical:
        keys = np.unique(r.astype(np.int64) * cols + c)
        r, c = keys // cols, keys % cols
    off = np.zeros(rows + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=rows)[:rows], out=off[1:])
    return off.astype(np.int32), c.astype(np.int32), rng.uniform(-1, 1, len(c)).astype(dtype)


def _from_rows(rows, row_of_entry, cols_of_entry, rng):
    """CSR of `rows` rows from entries given with their (non-decreasing) rows, fp64 values"""
    row_of_entry = np.asarray(row_of_entry, np.int64)
    assert np.all(np.diff(row_of_entry) >= 0)
    off = np.zeros(rows + 1, np.int64)
    np.cumsum(np.bincount(row_of_entry, minlength=rows), out=off[1:])
    return off.astype(np.int32), np.asarray(cols_of_entry, np.int32), rng.uniform(-1, 1, len(row_of_entry))


def _count_case(count, seed=0):
    """exactly `count` products from 300 rows of A over a B whose rows hold 0 .. 9 entries; an entry of A straddles every multiple of
    the tile below the count, and entries that point at empty rows of B are sprinkled in"""
    rng = np.random.default_rng(1000 + count + seed)
    rows, inner, cols = 300, 40, 61
    blen = rng.permutation(np.tile(np.arange(10), 4))
    boff = np.zeros(inner + 1, np.int64)
    np.cumsum(blen, out=boff[1:])
    B = (boff.astype(np.int32), rng.integers(0, cols, int(boff[-1])).astype(np.int32), rng.uniform(-1, 1, int(boff[-1])))
    by_len = [np.flatnonzero(blen == l) for l in range(10)]
    acols, cum = [], 0
    while cum < count:
        if rng.random() < 0.15:
            acols.append(int(rng.choice(by_len[0])))             # an empty row of B
            continue
        left, to_edge = count - cum, TILE - cum % TILE
        if to_edge <= 8 and left > to_edge:
            l = to_edge + 1                                      # straddles the edge
        elif to_edge <= 8:
            l = int(rng.integers(1, left + 1))
        else:
            l = int(rng.integers(1, min(8, left) + 1))           # (never lands on the edge)
        acols.append(int(rng.choice(by_len[l])))
        cum += l
    acols += [int(rng.choice(by_len[0]))] * 3
    A = _from_rows(rows, np.sort(rng.integers(0, rows, len(acols))), acols, rng)
    assert count_products(A, B) == count
    start = np.concatenate([[0], np.cumsum(blen[np.asarray(acols, np.int64)])])
    for edge in range(TILE, count, TILE):
        assert np.any((start[:-1] < edge) & (start[1:] > edge)), edge
    return rows, inner, cols, A, B


def _long_row_case(name):
    rng = np.random.default_rng(len(name))
    long_row = 5000
    if name == "single":                                         # one entry of A over three expansion tiles
        B = _from_rows(3, [1] * long_row, rng.integers(0, 700, long_row), rng)
        return 5, 3, 700, _from_rows(5, [2], [1], rng), B
    if name == "from_300_rows":                                  # the same row of B hit from 300 rows of A
        B = _from_rows(3, [0] + [1] * long_row + [2, 2], np.concatenate([[5], rng.integers(0, 700, long_row), [1, 699]]), rng)
        entries = [(2 * r, 1) for r in range(300)] + [(int(rng.integers(0, 600)), int(rng.choice([0, 2]))) for _ in range(40)]
        entries.sort(key=lambda t: t[0])
        return 600, 3, 700, _from_rows(600, [r for r, _ in entries], [c for _, c in entries], rng), B
    # one row of A with 300 entries whose rows of B all hold column 7: a run of 300 serial adds (and one row of B is long)
    inner = 300
    brow, bcol = [], []
    for k in range(inner):
        extra = rng.integers(0, 40, long_row if k == 150 else int(rng.integers(0, 4)))
        c = np.concatenate([extra[:len(extra) // 2], [7], extra[len(extra) // 2:]])
        brow += [k] * len(c); bcol += c.tolist()
    B = _from_rows(inner, brow, bcol, rng)
    A = _from_rows(4, [1] * inner + [3] * 5, np.concatenate([rng.permutation(inner), rng.integers(0, inner, 5)]), rng)
    return 4, inner, 40, A, B


def _empty_case(name):
    rng = np.random.default_rng(len(name) * 7)
    if name == "empty_rows_of_a":                                # at the front, at the back and in the middle
        B = _random_csr(rng, 50, 60, 400, np.float64)
        arows = np.sort(rng.choice(np.concatenate([np.arange(40, 300), np.arange(500, 900)]), 1500))
        return 1000, 50, 60, _from_rows(1000, arows, rng.integers(0, 50, 1500), rng), B
    if name == "empty_rows_of_b_3000_in_a_row":                  # a whole tile's search has to skip them (its slice of A is longer than a tile)
        blen = np.array([3, 0, 5, 0, 2])
        B = _from_rows(5, np.repeat(np.arange(5), blen), rng.integers(0, 9, 10), rng)
        acols = np.concatenate([rng.choice([0, 2, 4], 700), rng.choice([1, 3], 3000), rng.choice([0, 2, 4], 900), [1, 3, 1]])
        return 200, 5, 9, _from_rows(200, np.sort(rng.integers(0, 200, len(acols))), acols, rng), B
    if name == "one_row":
        return 1, 30, 40, _random_csr(rng, 1, 30, 25, np.float64), _random_csr(rng, 30, 40, 300, np.float64)
    if name == "inner_one":
        return 70, 1, 90, _random_csr(rng, 70, 1, 100, np.float64), _random_csr(rng, 1, 90, 60, np.float64)
    if name == "one_column":
        return 70, 30, 1, _random_csr(rng, 70, 30, 400, np.float64), _random_csr(rng, 30, 1, 50, np.float64)
    if name == "one_by_one":
        return 1, 1, 1, _random_csr(rng, 1, 1, 3, np.float64), _random_csr(rng, 1, 1, 2, np.float64)
    if name == "b_without_entries":                              # nnz_b = 0 with nnz_a > 0: no products
        return 70, 30, 40, _random_csr(rng, 70, 30, 400, np.float64), _random_csr(rng, 30, 40, 0, np.float64)
    assert name == "a_without_entries"
    return 70, 30, 40, _random_csr(rng, 70, 30, 0, np.float64), _random_csr(rng, 30, 40, 300, np.float64)


# ---------------------------------------------------------------------------------------------------------------- GPU plumbing
GUARD = 8
SENT_I, SENT_V = -0x5A5A5A5B, -12345.5


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(n, tdt, fill):
    buf = torch.full((GUARD + n + GUARD,), fill, dtype=tdt, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() > 0 else 0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def device_products(rows, inner, a, b, dev=None):
    """mspmv_csr_gemm_products on a guarded int64"""
    fn = M.load_library().mspmv_csr_gemm_products
    doa, dca, dob = dev if dev is not None else (_up(a[0]), _up(a[1]), _up(b[0]))
    buf, out = _guarded(1, torch.int64, SENT_I)
    size = ctypes.c_size_t(0)
    args = (_p(doa), _p(dca), rows, inner, len(a[1]), _p(dob), len(b[1]), _p(out))
    assert fn(None, ctypes.byref(size), *args, None, 0) == 0
    tmp = torch.full((size.value + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    assert fn(ctypes.c_void_p(tmp.data_ptr()), ctypes.byref(size), *args, _stream(), 0) == 0
    torch.cuda.synchronize()
    assert bool((tmp[size.value:] == 0x5A).all()), "temp storage overrun"
    assert bool((buf[:GUARD] == SENT_I).all()) and bool((buf[GUARD + 1:] == SENT_I).all())
    return int(out.item())


def device_gemm(rows, inner, cols, a, b, dtype, products=None, capacity=None, fill=(SENT_I, SENT_V), dev_inputs=None, temp=None, temp_fill=0x5A,
                debug=0, status=0):
    """the C call on guarded outputs; returns (row_offsets, column_indices[:count], values[:count] or None, count) as host arrays after
    checking the guard words, the entries past the count and -- when the count is -1 or above the capacity -- that no column and no
    value was written at all (for -1: C is unspecified, so only the guards are checked)"""
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    lib = M.load_library()
    fn = lib.mspmv_csr_gemm_f32 if dtype == np.float32 else lib.mspmv_csr_gemm_f64
    (oa, ca, va), (ob, cb, vb) = a, b
    structure = va is None
    if dev_inputs is None:
        dev_inputs = [None if x is None else _up(x) for x in (oa, ca, va, ob, cb, vb)]
    doa, dca, dva, dob, dcb, dvb = dev_inputs
    na, nb = len(ca), len(cb)
    products = count_products(a, b) if products is None else products
    capacity = products if capacity is None else capacity
    off_buf, off = _guarded(rows + 1, torch.int32, fill[0])
    col_buf, col = _guarded(capacity, torch.int32, fill[0])
    val_buf, val = (None, None) if structure else _guarded(capacity, tdt, fill[1])
    cnt_buf, cnt = _guarded(1, torch.int32, fill[0])
    size = ctypes.c_size_t(0)
    args = (rows, inner, cols, _p(dva), _p(doa), _p(dca), na, _p(dvb), _p(dob), _p(dcb), nb, products, capacity, _p(val), _p(off), _p(col), _p(cnt))
    q = fn(None, ctypes.byref(size), *args, None, 0)
    if status != 0:
        assert q == status
        return None
    assert q == 0
    if temp is None:
        temp = torch.full((size.value + 64,), temp_fill, dtype=torch.uint8, device="cuda")
    assert temp.numel() >= size.value + 64
    guard_from = temp.numel() - 64
    keep = temp[guard_from:].clone()
    torch.cuda.synchronize()
    st = fn(ctypes.c_void_p(temp.data_ptr()), ctypes.byref(ctypes.c_size_t(guard_from)), *args, _stream(), debug)
    assert st == 0, st
    torch.cuda.synchronize()
    assert torch.equal(temp[guard_from:], keep), "temp storage overrun"
    count = int(cnt.item())
    assert -1 <= count <= products
    written = count if 0 <= count <= capacity else (None if count == -1 else 0)
    for name, buf, view, f in (("offsets", off_buf, off, fill[0]), ("columns", col_buf, col, fill[0]), ("values", val_buf, val, fill[1]),
                               ("count", cnt_buf, cnt, fill[0])):
        if buf is None:
            continue
        assert bool((buf[:GUARD] == f).all()) and bool((buf[GUARD + view.numel():] == f).all()), f"guard words of the {name} were written"
        if name in ("columns", "values") and written is not None:
            assert bool((view[written:] == f).all()), f"{name} past the count were written"
    n = max(written or 0, 0)
    return off.cpu().numpy(), col[:n].cpu().numpy(), None if structure else val[:n].cpu().numpy(), count


def _assert_equal(got, want, what=""):
    off, col, val, count = got
    woff, wcol, wval = want
    assert count == len(wcol), (what, count, len(wcol))
    assert np.array_equal(off, woff), what
    assert np.array_equal(col, wcol), what
    if wval is None:
        assert val is None
    else:
        assert val.dtype == wval.dtype and val.tobytes() == wval.tobytes(), what          # bit for bit


def _narrow(m, dtype):
    return m[0], m[1], None if dtype is None else m[2].astype(dtype)


def _check_all_forms(rows, inner, cols, A, B, what):
    """fp32, fp64 and structure only through either entry point, and the count of products; A, B carry fp64 values"""
    products = count_products(A, B)
    assert device_products(rows, inner, A, B) == products, what
    for dtype in (np.float32, np.float64):
        a, b = _narrow(A, dtype), _narrow(B, dtype)
        _assert_equal(device_gemm(rows, inner, cols, a, b, dtype), host_gemm(rows, cols, a, b, dtype), (what, dtype.__name__))
        s = (_narrow(A, None), _narrow(B, None))
        _assert_equal(device_gemm(rows, inner, cols, *s, dtype), host_gemm(rows, cols, *s), (what, "structure", dtype.__name__))
    return products


# ---------------------------------------------------------------------------------------------------------------- GPU: shapes
@gpu
@pytest.mark.parametrize("count", COUNTS)
def test_product_counts_around_the_tile_and_scan_edges(count):
    assert _check_all_forms(*_count_case(count), count) == count


@gpu
@pytest.mark.parametrize("name", ["single", "from_300_rows", "run_of_300"])
def test_an_entry_of_a_over_a_row_of_b_with_5000_entries(name):
    rows, inner, cols, A, B = _long_row_case(name)
    assert np.diff(B[0]).max() >= 5000 and np.diff(B[0])[A[1]].max() >= 5000        # some entry of A spans three tiles
    if name == "from_300_rows":
        assert (np.diff(B[0])[A[1]] >= 5000).sum() == 300
    if name == "run_of_300":
        want = host_gemm(rows, cols, A, B, np.float64)
        assert want[1][want[0][1]:want[0][2]].tolist().count(7) == 1 and sorted(A[1][:300].tolist()) == list(range(300))
    _check_all_forms(rows, inner, cols, A, B, name)


@gpu
@pytest.mark.parametrize("name", ["empty_rows_of_a", "empty_rows_of_b_3000_in_a_row", "one_row", "inner_one", "one_column", "one_by_one",
                                  "b_without_entries", "a_without_entries"])
def test_empty_things_at_the_edges(name):
    rows, inner, cols, A, B = _empty_case(name)
    products = _check_all_forms(rows, inner, cols, A, B, name)
    if name.endswith("without_entries"):
        assert products == 0
    if name == "empty_rows_of_b_3000_in_a_row":                  # 3000 consecutive entries of A without products, inside one tile
        lens = np.diff(B[0])[A[1]]
        zero_runs = np.diff(np.flatnonzero(np.concatenate([[1], lens != 0, [1]])))
        assert zero_runs.max() - 1 >= 2500 and products > 2 * TILE


# ---------------------------------------------------------------------------------------------------------------- GPU: any valid CSR
@gpu
def test_inputs_that_are_not_canonical():
    rng = np.random.default_rng(21)
    rows, inner, cols = 150, 80, 90
    A, B = _random_csr(rng, rows, inner, 1200, np.float64, canonical=True), _random_csr(rng, inner, cols, 900, np.float64, canonical=True)
    # rows of A shuffled: the pattern of C stays, the order of the adds follows A's row
    sa = list(A)
    perm = np.concatenate([A[0][r] + rng.permutation(A[0][r + 1] - A[0][r]) for r in range(rows)]).astype(np.int64)
    sa[1], sa[2] = A[1][perm], A[2][perm]
    _check_all_forms(rows, inner, cols, tuple(sa), B, "shuffled")
    canon, shuffled = host_gemm(rows, cols, A, B, np.float32), host_gemm(rows, cols, _narrow(tuple(sa), np.float32), _narrow(B, np.float32), np.float32)
    assert np.array_equal(canon[1], shuffled[1]) and canon[2].tobytes() != shuffled[2].tobytes()        # (the case tells the orders apart)
    # repeated columns in A and in B
    Ar, Br = _random_csr(rng, rows, inner, 3000, np.float64), _random_csr(rng, inner, cols, 2500, np.float64)
    assert any(len(set(Ar[1][Ar[0][r]:Ar[0][r + 1]].tolist())) < Ar[0][r + 1] - Ar[0][r] for r in range(rows))
    assert any(len(set(Br[1][Br[0][r]:Br[0][r + 1]].tolist())) < Br[0][r + 1] - Br[0][r] for r in range(inner))
    _check_all_forms(rows, inner, cols, Ar, Br, "repeats")
    _check_all_forms(rows, rows, rows, _random_csr(rng, rows, rows, 2000, np.float64), _random_csr(rng, rows, rows, 2000, np.float64), "square")


@gpu
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_a_times_identity_is_the_sorted_and_merged_a(prec):
    """A * I against csr_sum_duplicates(coo_to_csr(A)) of the existing calls, and both against the model"""
    from merge_spmv_amd.generators import DeviceCsr
    dtype = np.float32 if prec == "f32" else np.float64
    rng = np.random.default_rng(22)
    rows, n = 200, 120
    A = _random_csr(rng, rows, n, 5000, dtype)
    eye = (np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n, dtype))
    want = host_gemm(rows, n, A, eye, dtype)
    assert len(want[1]) < len(A[1])                              # (there are duplicates to merge)
    _assert_equal(device_gemm(rows, n, n, A, eye, dtype), want)
    arow = np.repeat(np.arange(rows, dtype=np.int32), np.diff(A[0]))
    built = M.coo_to_csr(_up(A[2]), _up(arow), _up(A[1]), rows, n, sum_duplicates=True)
    assert np.array_equal(built.row_offsets.cpu().numpy(), want[0]) and np.array_equal(built.column_indices.cpu().numpy(), want[1])
    assert built.values.cpu().numpy().tobytes() == want[2].tobytes()
    c = M.csr_gemm(DeviceCsr(rows, n, _up(A[0]), _up(A[1]), _up(A[2])), DeviceCsr(n, n, _up(eye[0]), _up(eye[1]), _up(eye[2])))
    assert torch.equal(c.row_offsets, built.row_offsets) and torch.equal(c.column_indices, built.column_indices)
    assert c.values.cpu().numpy().tobytes() == built.values.cpu().numpy().tobytes()


# ---------------------------------------------------------------------------------------------------------------- GPU: values
@gpu
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_values_are_rounded_products_added_left_to_right(prec):
    dtype = np.float32 if prec == "f32" else np.float64
    i = lambda x: np.asarray(x, np.int32)
    # +x and -x meet: the entry stays, +0.0; a lone product of -0.0 stays -0.0
    a = (i([0, 2, 3]), i([0, 1, 0]), _f([1.5, -1.5, -0.0], dtype))
    b = (i([0, 1, 2]), i([4, 4]), _f([2.0, 2.0], dtype))
    got = device_gemm(2, 2, 5, a, b, dtype)
    _assert_equal(got, host_gemm(2, 5, a, b, dtype))
    assert got[3] == 2 and got[2].tolist() == [0.0, 0.0] and not np.signbit(got[2][0]) and np.signbit(got[2][1])
    # the order of the adds: (big + 1) - big = 0 left to right
    big = 2.0 ** (24 if prec == "f32" else 53)
    a = (i([0, 3]), i([0, 1, 2]), _f([big, 1.0, -big], dtype))
    b = (i([0, 1, 2, 3]), i([0, 0, 0]), _f([1.0, 1.0, 1.0], dtype))
    assert device_gemm(1, 3, 1, a, b, dtype)[2].tolist() == [0.0] == host_gemm(1, 1, a, b, dtype)[2].tolist()
    a2 = (a[0], i([0, 2, 1]), _f([big, -big, 1.0], dtype))
    assert device_gemm(1, 3, 1, a2, b, dtype)[2].tolist() == [1.0] == host_gemm(1, 1, a2, b, dtype)[2].tolist()
    # (-1 * 1) + (3 * fl(1/3)) = 0 unfused
    third = dtype(1.0) / dtype(3.0)
    a = (i([0, 2]), i([0, 1]), _f([-1.0, 3.0], dtype))
    b = (i([0, 1, 2]), i([0, 0]), _f([1.0, third], dtype))
    assert device_gemm(1, 2, 1, a, b, dtype)[2].tolist() == [0.0]
    # products that differ between fused and unfused evaluation (test_the_fma_case_tells_fused_from_unfused)
    A, B, n = _fma_case(dtype)
    got = device_gemm(1, 2, n, A, B, dtype)
    _assert_equal(got, host_gemm(1, n, A, B, dtype), "fma")
    assert np.array_equal(got[2], A[2][0] * B[2][:n] + A[2][1] * B[2][n:])


# ---------------------------------------------------------------------------------------------------------------- GPU: capacity, products
def _medium(dtype, seed=30):
    rng = np.random.default_rng(seed)
    rows, inner, cols = 400, 300, 350
    return rows, inner, cols, _random_csr(rng, rows, inner, 3000, dtype), _random_csr(rng, inner, cols, 2500, dtype)


@gpu
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_capacity(prec):
    dtype = np.float32 if prec == "f32" else np.float64
    rows, inner, cols, A, B = _medium(dtype)
    want = host_gemm(rows, cols, A, B, dtype)
    nnz_c = len(want[1])
    assert 1 < nnz_c < count_products(A, B)
    _assert_equal(device_gemm(rows, inner, cols, A, B, dtype, capacity=nnz_c), want, "exact")
    for cap in (nnz_c - 1, 0):
        for a, b in ((A, B), (_narrow(A, None), _narrow(B, None))):
            off, col, val, count = device_gemm(rows, inner, cols, a, b, dtype, capacity=cap)      # (checks that nothing was written)
            assert count == nnz_c and np.array_equal(off, want[0]) and len(col) == 0, cap


@gpu
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_products_stated_wrong(prec):
    dtype = np.float32 if prec == "f32" else np.float64
    rows, inner, cols, A, B = _medium(dtype, seed=31)
    true = count_products(A, B)
    assert true > 2 * TILE
    want = host_gemm(rows, cols, A, B, dtype)
    lib = M.load_library()
    fn = lib.mspmv_csr_gemm_f32 if dtype == np.float32 else lib.mspmv_csr_gemm_f64
    size, most = ctypes.c_size_t(0), 0
    for products in (true - 1, true + 1, true + TILE + 1, 0, true):
        assert fn(None, ctypes.byref(size), rows, inner, cols, None, None, None, len(A[1]), None, None, None, len(B[1]), products, products,
                  None, None, None, None, None, 0) == 0
        most = max(most, size.value)
    temp = torch.full((most + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    for products in (true - 1, true + 1, true + TILE + 1, 0):
        for a, b in ((A, B), (_narrow(A, None), _narrow(B, None))):
            got = device_gemm(rows, inner, cols, a, b, dtype, products=products, capacity=true + TILE + 1, temp=temp)
            assert got[3] == -1, products
            _assert_equal(device_gemm(rows, inner, cols, A, B, dtype, temp=temp), want, ("after", products))      # the same temp storage
    # products > 0 stated for factors one of which has no entry
    empty = (np.zeros(inner + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, dtype))
    assert device_gemm(rows, inner, cols, A, empty, dtype, products=5)[3] == -1


@gpu
def test_products_beyond_int32():
    """inner = 1, one row of B with 70 000 entries, 40 000 entries of A: 2.8 * 10^9 products -- the count call is exact in 64 bits,
    the product call refuses before it launches anything"""
    from merge_spmv_amd.generators import DeviceCsr
    rng = np.random.default_rng(40)
    rows, nb, na = 200, 70_000, 40_000
    A = _from_rows(rows, np.sort(rng.integers(0, rows, na)), np.zeros(na, np.int32), rng)
    B = (np.array([0, nb], np.int32), rng.integers(0, nb, nb).astype(np.int32), rng.uniform(-1, 1, nb))
    assert count_products(A, B) == 2_800_000_000 > 2 ** 31
    assert device_products(rows, 1, A, B) == 2_800_000_000
    da = DeviceCsr(rows, 1, _up(A[0]), _up(A[1]), _up(A[2]))
    db = DeviceCsr(1, nb, _up(B[0]), _up(B[1]), _up(B[2]))
    assert M.csr_gemm_products(da, db) == 2_800_000_000
    for products in (2 ** 31 - 1, MAX_ITEMS - rows + 1):
        assert device_gemm(rows, 1, nb, A, B, np.float64, products=products, capacity=0, status=1) is None
    with pytest.raises(M.MspmvError):
        M.csr_gemm(da, db)
    assert device_gemm(rows, 1, nb, A, B, np.float64, products=4096, capacity=0)[3] == -1
    # a stated count that equals the true one modulo 2^32 -- what a 32-bit sum of the lengths would come to -- is still told from it
    na, nb = 4096, 2 ** 20 + 1
    A = _from_rows(rows, np.sort(rng.integers(0, rows, na)), np.zeros(na, np.int32), rng)
    B = (np.array([0, nb], np.int32), rng.integers(0, 50, nb).astype(np.int32), rng.uniform(-1, 1, nb))
    assert count_products(A, B) == 2 ** 32 + 4096 == device_products(rows, 1, A, B)
    assert device_gemm(rows, 1, 50, A, B, np.float64, products=4096, capacity=0)[3] == -1


# ---------------------------------------------------------------------------------------------------------------- GPU: other checks
@gpu
def test_gemm_is_deterministic():
    rows, inner, cols, A, B = _medium(np.float64, seed=32)
    one = device_gemm(rows, inner, cols, A, B, np.float64, fill=(SENT_I, SENT_V), temp_fill=0x5A)
    two = device_gemm(rows, inner, cols, A, B, np.float64, fill=(0x01010101, 7.25), temp_fill=0xC3)
    assert one[3] == two[3] > 0
    for x, y in zip(one[:3], two[:3]):
        assert x.tobytes() == y.tobytes()


def _relabelled(rng, rows, inner, cols, A, B):
    """another pair of the same sizes and the same number of products: A's columns renamed, B's rows moved with them, B's columns
    reversed (which unsorts its rows), new values"""
    pi = rng.permutation(inner)
    a = (A[0], pi[A[1]].astype(np.int32), rng.uniform(-1, 1, len(A[1])).astype(A[2].dtype))
    lens = np.diff(B[0])
    src = np.argsort(pi)                                         # row k of the new B is row src[k] of the old one
    boff = np.zeros(inner + 1, np.int64)
    np.cumsum(lens[src], out=boff[1:])
    take = np.concatenate([np.arange(B[0][s], B[0][s + 1]) for s in src]).astype(np.int64) if len(B[1]) else np.zeros(0, np.int64)
    b = (boff.astype(np.int32), (cols - 1 - B[1][take]).astype(np.int32), rng.uniform(-1, 1, len(take)).astype(B[2].dtype))
    assert count_products(a, b) == count_products(A, B)
    return a, b


@gpu
def test_launches_depend_on_the_sizes_alone(capfd):
    rng = np.random.default_rng(33)
    rows, inner, cols, A, B = _medium(np.float32, seed=33)
    A2, B2 = _relabelled(rng, rows, inner, cols, A, B)
    capfd.readouterr()
    _assert_equal(device_gemm(rows, inner, cols, A, B, np.float32, debug=1), host_gemm(rows, cols, A, B, np.float32))
    one = [l for l in capfd.readouterr().out.splitlines() if l.startswith("mspmv:")]
    want2 = host_gemm(rows, cols, A2, B2, np.float32)
    _assert_equal(device_gemm(rows, inner, cols, A2, B2, np.float32, debug=1), want2)
    two = [l for l in capfd.readouterr().out.splitlines() if l.startswith("mspmv:")]
    assert one == two and len(one) > 10 and any("gemm_expand_kernel" in l for l in one) and any("tr_downsweep_kernel" in l for l in one)
    assert want2[1].tobytes() != host_gemm(rows, cols, A, B, np.float32)[1].tobytes()            # (the matrices do differ)


@gpu
def test_gemm_replays_in_a_graph_on_new_patterns():
    """CsrGemm reads nothing back on the host: captured on a side stream, replayed after the factors' values AND patterns (same sizes,
    same number of products) were overwritten in place, it gives the new product every time"""
    from merge_spmv_amd.generators import DeviceCsr
    rng = np.random.default_rng(34)
    rows, inner, cols, A, B = _medium(np.float32, seed=34)
    products = count_products(A, B)
    a = DeviceCsr(rows, inner, _up(A[0]), _up(A[1]), _up(A[2]))
    b = DeviceCsr(inner, cols, _up(B[0]), _up(B[1]), _up(B[2]))
    op = M.CsrGemm(a, b, products=products)                      # (allocates the outputs and the temp storage once)
    got = op.trimmed()
    want = host_gemm(rows, cols, A, B, np.float32)
    assert np.array_equal(got.column_indices.cpu().numpy(), want[1]) and got.values.cpu().numpy().tobytes() == want[2].tobytes()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        op(stream=side)                                          # warm-up outside the capture
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            op(stream=side)
    torch.cuda.synchronize()
    for _ in range(3):
        A, B = _relabelled(rng, rows, inner, cols, A, B)
        for t, h in zip((a.row_offsets, a.column_indices, a.values, b.row_offsets, b.column_indices, b.values), A + B):
            t.copy_(_up(h))
        op.column_indices.fill_(-7)
        op.count.fill_(-7)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want = host_gemm(rows, cols, A, B, np.float32)
        n = int(op.count.item())
        assert n == len(want[1]) and np.array_equal(op.row_offsets.cpu().numpy(), want[0])
        assert np.array_equal(op.column_indices[:n].cpu().numpy(), want[1]) and op.values[:n].cpu().numpy().tobytes() == want[2].tobytes()
        assert bool((op.column_indices[n:] == -7).all())


@gpu
def test_the_wrappers():
    from merge_spmv_amd.generators import DeviceCsr
    rows, inner, cols, A, B = _medium(np.float64, seed=35)
    want = host_gemm(rows, cols, A, B, np.float64)
    a = DeviceCsr(rows, inner, _up(A[0]), _up(A[1]), _up(A[2]))
    b = DeviceCsr(inner, cols, _up(B[0]), _up(B[1]), _up(B[2]))
    products = M.csr_gemm_products(a, b)
    assert products == count_products(A, B)
    c = M.csr_gemm(a, b)
    assert (c.rows, c.cols) == (rows, cols) and c.column_indices.numel() == len(want[1]) == c.values.numel()
    assert np.array_equal(c.row_offsets.cpu().numpy(), want[0]) and np.array_equal(c.column_indices.cpu().numpy(), want[1])
    assert c.values.cpu().numpy().tobytes() == want[2].tobytes()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    full = M.csr_gemm(a, b, stream=side, trim=False)
    side.synchronize()
    assert full.column_indices.numel() == products and int(full.row_offsets[-1].item()) == len(want[1])
    s = M.csr_gemm(DeviceCsr(rows, inner, a.row_offsets, a.column_indices, None), DeviceCsr(inner, cols, b.row_offsets, b.column_indices, None))
    assert s.values is None and np.array_equal(s.column_indices.cpu().numpy(), want[1])
    sym = M.CsrGemm(a, b, products=products, capacity=0)        # the symbolic phase
    assert int(sym.count.item()) == len(want[1]) and np.array_equal(sym.row_offsets.cpu().numpy(), want[0])
    with pytest.raises(M.MspmvError):
        sym.trimmed()                                            # no room for C's entries
    with pytest.raises(M.MspmvError):
        M.CsrGemm(a, b, products=products + 1).trimmed()         # not the factors' count
    with pytest.raises(M.MspmvError):
        M.csr_gemm(a, a)                                         # inner dimensions differ
    with pytest.raises(M.MspmvError):
        M.csr_gemm(a, DeviceCsr(inner, cols, b.row_offsets, b.column_indices, None))             # values for one only
    with pytest.raises(M.MspmvError):
        M.csr_gemm(a, DeviceCsr(inner, cols, b.row_offsets, b.column_indices, b.values.float()))


@gpu
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_csrmv_on_the_product_of_a_golden_matrix(prec):
    """C = A * A for a golden matrix: csrmv(C, x) against csrmv(A, csrmv(A, x)).  Both approximate A A x.  With eps the unit
    round-off, c(M) = 2 (ceil(log2(longest row + 1)) + depth + 8) the constant of the library's CsrMV bound |y - M x| <= c eps |M| |x|
    (oracle.strict_check) and L the longest row of A (an entry of C is the sum of at most L rounded products: relative error below
    (L + 1) eps of |A| |A|), to first order
        |csrmv(C, x) - A A x| <= (c(C) + L + 1) eps S      and      |csrmv(A, csrmv(A, x)) - A A x| <= 2 c(A) eps S,
    S = |A| (|A| |x|); the test allows their sum with a factor 2 for the higher-order terms."""
    from merge_spmv_amd.generators import DeviceCsr
    dtype, tdt, vb, eps = (np.float32, torch.float32, 4, 2.0 ** -24) if prec == "f32" else (np.float64, torch.float64, 8, 2.0 ** -53)
    case = next(c for c in load_golden("matrices.json")["cases"] if c["label"] == "grid3d_4")
    n = case["rows"]
    rng = np.random.default_rng(50)
    A = (np.asarray(case["row_offsets"], np.int32), np.asarray(case["column_indices"], np.int32), rng.uniform(-1, 1, case["nnz"]).astype(dtype))
    want = host_gemm(n, n, A, A, dtype)
    da = DeviceCsr(n, n, _up(A[0]), _up(A[1]), _up(A[2]))
    c = M.csr_gemm(da, da)                                       # (A and B the same arrays)
    assert np.array_equal(c.row_offsets.cpu().numpy(), want[0]) and np.array_equal(c.column_indices.cpu().numpy(), want[1])
    assert c.values.cpu().numpy().tobytes() == want[2].tobytes()
    x = rng.uniform(-1, 1, n).astype(dtype)
    dx = _up(x)
    y = M.csrmv(c.values, c.row_offsets, c.column_indices, dx, num_cols=n)
    z = M.csrmv(da.values, da.row_offsets, da.column_indices, M.csrmv(da.values, da.row_offsets, da.column_indices, dx, num_cols=n), num_cols=n)
    torch.cuda.synchronize()
    dense = np.zeros((n, n))
    dense[np.repeat(np.arange(n), np.diff(A[0])), A[1]] = A[2].astype(np.float64)                 # (the golden grid has no repeated column)
    S = np.abs(dense) @ (np.abs(dense) @ np.abs(x.astype(np.float64)))
    L = int(np.diff(A[0]).max())
    const = lambda lens, nnz: 2.0 * (np.ceil(np.log2(lens.max() + 1.0)) + M.serial_sum_depth(n, n, nnz, vb) + 8)
    bound = 2.0 * (const(np.diff(want[0]), len(want[1])) + L + 1 + 2 * const(np.diff(A[0]), case["nnz"])) * eps * S
    err = np.abs(y.cpu().numpy().astype(np.float64) - z.cpu().numpy().astype(np.float64))
    assert np.all(err <= bound), float((err / bound).max())
    exact = dense @ (dense @ x.astype(np.float64))
    assert np.all(np.abs(y.cpu().numpy() - exact) <= bound)
