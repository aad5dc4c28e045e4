"""C = alpha*A + beta*B on the device (include/mspmv.h: mspmv_csr_add_*; merge_spmv_amd.csr_add / CsrAdd / csr_symmetrize).
CPU: exports, size-query conventions, the wrappers' argument checks, and the host restatement the GPU tests compare against pinned
to hand-written cases.  GPU: every comparison is exact -- offsets, the first `count` columns and values bit for bit, the entries
past `count` and the guard words around every output array untouched.  Expected values never come from the code under test."""
import ctypes
import os
import subprocess
import sys
import zlib
from fractions import Fraction

import numpy as np
import pytest

import merge_spmv_amd as M
from conftest import ROOT, load_golden
from oracle import oracle as O

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

NEW = ["mspmv_csr_add_f32", "mspmv_csr_add_f64"]
MAX_ITEMS = 2 ** 31 - 1 - 65536
TILE = 1792                                                     # merged entries per tile (include/mspmv.h says so)
ALPHA_BETA = [(1.0, 1.0), (1.0, -1.0), (0.5, -3.0), (0.0, 1.0)]


# ---------------------------------------------------------------------------------------------------------------- the host restatement
def host_add(rows, cols, a, b, alpha=1.0, beta=1.0, dtype=None):
    """a, b = (row_offsets, column_indices, values or None) with sorted rows and no repeated column.  Per row the sorted union of the
    two column lists; values alpha * a, beta * b, (alpha * a) + (beta * b) in the value dtype: two products, then one sum."""
    (oa, ca, va), (ob, cb, vb) = a, b
    ra = np.repeat(np.arange(rows, dtype=np.int64), np.diff(np.asarray(oa, np.int64)))
    rb = np.repeat(np.arange(rows, dtype=np.int64), np.diff(np.asarray(ob, np.int64)))
    ka, kb = ra * cols + np.asarray(ca, np.int64), rb * cols + np.asarray(cb, np.int64)
    keys = np.union1d(ka, kb)                                    # sorted by (row, column), every key once
    off = np.zeros(rows + 1, np.int64)
    np.cumsum(np.bincount(keys // cols, minlength=rows), out=off[1:])
    col = (keys % cols).astype(np.int32)
    if va is None:
        return off.astype(np.int32), col, None
    t = np.dtype(dtype).type
    pa, pb = t(alpha) * np.asarray(va, dtype), t(beta) * np.asarray(vb, dtype)          # each product rounded on its own
    ia, ib = np.searchsorted(keys, ka), np.searchsorted(keys, kb)
    val = np.zeros(len(keys), dtype)
    val[ia] = pa
    both_b = np.isin(kb, ka, assume_unique=True)
    only_b = ~both_b
    val[ib[only_b]] = pb[only_b]
    val[ib[both_b]] = val[ib[both_b]] + pb[both_b]               # (alpha * a) + (beta * b)
    return off.astype(np.int32), col, val


def host_add_by_rows(rows, cols, a, b, alpha, beta, dtype):
    """the same, row by row with python sets: what host_add is pinned against"""
    (oa, ca, va), (ob, cb, vb) = a, b
    t = np.dtype(dtype).type
    off, col, val = [0], [], []
    for r in range(rows):
        da = {int(ca[j]): va[j] for j in range(oa[r], oa[r + 1])}
        db = {int(cb[j]): vb[j] for j in range(ob[r], ob[r + 1])}
        for c in sorted(set(da) | set(db)):
            col.append(c)
            if c in da and c in db:
                val.append(t(t(alpha) * t(da[c])) + t(t(beta) * t(db[c])))
            elif c in da:
                val.append(t(alpha) * t(da[c]))
            else:
                val.append(t(beta) * t(db[c]))
        off.append(len(col))
    return np.asarray(off, np.int32), np.asarray(col, np.int32).reshape(-1), np.asarray(val, dtype).reshape(-1)


def _csr_from_keys(rows, cols, keys, rng, dtype):
    keys = np.asarray(keys, np.int64)
    off = np.zeros(rows + 1, np.int64)
    np.cumsum(np.bincount(keys // cols, minlength=rows), out=off[1:])
    return off.astype(np.int32), (keys % cols).astype(np.int32), rng.uniform(-1, 1, len(keys)).astype(dtype)


def _random_pair(rng, rows, cols, na, nb, overlap, dtype):
    """two canonical matrices whose patterns share `overlap` (0, 0.5 or 1) of B's entries with A"""
    cells = rows * cols
    if overlap == 1.0:
        ka = np.unique(rng.integers(0, cells, na)); kb = ka
    elif overlap == 0.0:                                         # A on even cells, B on odd ones
        ka = np.unique(rng.integers(0, (cells + 1) // 2, na)) * 2
        kb = np.unique(rng.integers(0, cells // 2, nb)) * 2 + 1 if cells > 1 else np.zeros(0, np.int64)
    else:
        ka = np.unique(rng.integers(0, cells, na))
        fresh = np.unique(rng.integers(0, cells, nb // 2))
        kb = np.union1d(rng.choice(ka, min(nb // 2, len(ka)), replace=False), fresh)
    return _csr_from_keys(rows, cols, ka, rng, dtype), _csr_from_keys(rows, cols, kb, rng, dtype)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_add_symbols_are_declared_and_exported():
    import re
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mspmv.h")).read(), flags=re.S)
    lib = M.load_library()
    for kind in ("product", "dev"):
        out = subprocess.run(["nm", "-D", "--defined-only", M.library_path(kind)], capture_output=True, text=True, check=True).stdout
        for name in NEW:
            assert f" T {name}\n" in out + "\n", (kind, name)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    for name in ("csr_add", "CsrAdd", "csr_symmetrize"):
        assert name in M.__all__ and callable(getattr(M, name))
    assert lib.mspmv_version() == 102


def _call(lib, prec, temp, size, rows, cols, na, nb, f=None, va="f", vb="f", vc="f"):
    fn = getattr(lib, "mspmv_csr_add_" + prec)
    pick = lambda v: f if v == "f" else v
    return fn(temp, ctypes.byref(size), rows, cols, 1.0, pick(va), f, f, na, 1.0, pick(vb), f, f, nb, pick(vc), f, f, f, None, 0)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_add_size_query_conventions(prec):
    lib = M.load_library()
    fake = ctypes.c_void_p(4096)
    size = ctypes.c_size_t(0)
    assert _call(lib, prec, None, size, 1000, 1000, 50000, 30000) == 0 and size.value > 0
    need = size.value
    for rows, cols, na, nb in ((0, 0, 0, 0), (0, 7, 0, 0), (7, 0, 0, 0), (5, 5, 0, 0), (5, 1, 5, 0), (1, 5, 0, 5)):
        assert _call(lib, prec, None, size, rows, cols, na, nb) == 0 and size.value > 0, (rows, cols, na, nb)
    # too small / misaligned temp storage; missing arrays; negative sizes; entries without rows or columns
    assert _call(lib, prec, ctypes.c_void_p(256), ctypes.c_size_t(need - 1), 1000, 1000, 50000, 30000, fake) == 1
    for misaligned in (4096 + 1, 4096 + 4, 4096 + 8):
        assert _call(lib, prec, ctypes.c_void_p(misaligned), ctypes.c_size_t(need + 64), 1000, 1000, 50000, 30000, fake) == 1
    assert _call(lib, prec, ctypes.c_void_p(4096), ctypes.c_size_t(need + 64), 1000, 1000, 50000, 30000, None) == 1
    for rows, cols, na, nb in ((-1, 5, 5, 5), (5, -1, 5, 5), (5, 5, -1, 5), (5, 5, 5, -1), (0, 5, 5, 0), (5, 0, 0, 5)):
        assert _call(lib, prec, None, size, rows, cols, na, nb) == 1, (rows, cols, na, nb)
    # rows + nnz_a + nnz_b: exactly at the limit is accepted, one above is refused (whichever of the three grows)
    half = (MAX_ITEMS - 1000) // 2
    assert _call(lib, prec, None, size, 1000, 1000, half, MAX_ITEMS - 1000 - half) == 0
    assert _call(lib, prec, None, size, 1001, 1000, half, MAX_ITEMS - 1000 - half) == 1
    assert _call(lib, prec, None, size, 1000, 1000, half + 1, MAX_ITEMS - 1000 - half) == 1
    assert _call(lib, prec, None, size, 1000, 1000, half, MAX_ITEMS - 1000 - half + 1) == 1
    assert _call(lib, prec, None, size, 1000, 1 << 30, half, MAX_ITEMS - 1000 - half) == 0       # (columns do not count)
    assert _call(lib, prec, None, size, 1000, 1000, MAX_ITEMS - 1000, 0) == 0
    fn = getattr(lib, "mspmv_csr_add_" + prec)
    assert fn(None, None, 5, 5, 1.0, None, None, None, 5, 1.0, None, None, None, 5, None, None, None, None, None, 0) == 1
    # values for some matrices and not for the others (refused before anything is launched)
    big = lambda: ctypes.c_size_t(1 << 30)
    for va, vb, vc in ((None, "f", "f"), ("f", None, "f"), ("f", "f", None), (None, None, "f"), ("f", None, None), (None, "f", None)):
        assert _call(lib, prec, fake, big(), 5, 5, 5, 5, fake, va, vb, vc) == 1, (va, vb, vc)
    # per tile, not per entry: 10^8 + 10^8 entries need less than 1/100 of the input's bytes
    vb_ = 4 if prec == "f32" else 8
    assert _call(lib, prec, None, size, 3_000_000, 3_000_000, 100_000_000, 100_000_000) == 0
    assert size.value * 100 < 200_000_000 * (4 + vb_) + 2 * 3_000_001 * 4
    assert size.value * 100 < 200_000_000 * 4                   # (and of the column indices alone)


def test_host_restatement_on_hand_written_cases():
    f = np.float32
    # 1. one row, overlapping in the middle: columns {0, 2, 5} + {2, 3} -> {0, 2, 3, 5}
    a = (np.array([0, 3]), np.array([0, 2, 5]), np.array([1.0, 2.0, 3.0], f))
    b = (np.array([0, 2]), np.array([2, 3]), np.array([10.0, 20.0], f))
    off, col, val = host_add(1, 6, a, b, 1.0, 1.0, f)
    assert off.tolist() == [0, 4] and col.tolist() == [0, 2, 3, 5] and val.tolist() == [1.0, 12.0, 20.0, 3.0] and val.dtype == f
    # 2. empty rows anywhere, alpha / beta, an entry that cancels to 0 and stays
    a = (np.array([0, 0, 2, 2, 3]), np.array([1, 3, 0]), np.array([4.0, -6.0, 1.0], f))
    b = (np.array([0, 1, 2, 2, 2]), np.array([2, 3]), np.array([7.0, -1.0], f))
    off, col, val = host_add(4, 4, a, b, 0.5, -3.0, f)
    assert off.tolist() == [0, 1, 3, 3, 4] and col.tolist() == [2, 1, 3, 0] and val.tolist() == [-21.0, 2.0, 0.0, 0.5]
    # 3. alpha == 0 keeps A's pattern; structure only
    off, col, val = host_add(4, 4, a, b, 0.0, 1.0, f)
    assert col.tolist() == [2, 1, 3, 0] and val.tolist() == [7.0, 0.0, -1.0, 0.0]
    off, col, val = host_add(4, 4, (a[0], a[1], None), (b[0], b[1], None))
    assert off.tolist() == [0, 1, 3, 3, 4] and col.tolist() == [2, 1, 3, 0] and val is None
    # 4. the products are rounded before the sum: 3 * (1/3) in fp32 is exactly 1, so 3 * fl(1/3) + (-1) * 1 = 0, where a fused
    #    multiply-add would keep the rounding error of fl(1/3)
    third = f(1.0) / f(3.0)
    a = (np.array([0, 1]), np.array([0]), np.array([third], f)); b = (np.array([0, 1]), np.array([0]), np.array([1.0], f))
    assert host_add(1, 1, a, b, 3.0, -1.0, f)[2].tolist() == [0.0]
    assert float(Fraction(3) * Fraction(float(third)) - 1) != 0.0
    # and against the row-by-row statement on random matrices
    rng = np.random.default_rng(1)
    for dtype in (np.float32, np.float64):
        for overlap in (0.0, 0.5, 1.0):
            A, B = _random_pair(rng, 37, 53, 400, 300, overlap, dtype)
            for alpha, beta in ALPHA_BETA:
                got, want = host_add(37, 53, A, B, alpha, beta, dtype), host_add_by_rows(37, 53, A, B, alpha, beta, dtype)
                assert all(np.array_equal(g, w) for g, w in zip(got, want)) and got[2].dtype == dtype


def _fma_pair(dtype, n=512):
    """values and factors for which a fused (alpha * a) + beta * b differs from the unfused one in some entry"""
    rng = np.random.default_rng(77)
    a, b = rng.uniform(1, 2, n).astype(dtype), rng.uniform(1, 2, n).astype(dtype)
    return a, b, 1.0 / 3.0, -0.3


def test_the_fma_case_tells_fused_from_unfused():
    for dtype in (np.float32, np.float64):
        t = np.dtype(dtype).type
        a, b, alpha, beta = _fma_pair(dtype)
        unfused = t(alpha) * a + t(beta) * b
        pb, pa = t(beta) * b, t(alpha) * a
        fused_a = np.array([t(float(Fraction(float(t(alpha))) * Fraction(float(x)) + Fraction(float(y)))) for x, y in zip(a, pb)], dtype)
        fused_b = np.array([t(float(Fraction(float(t(beta))) * Fraction(float(x)) + Fraction(float(y)))) for x, y in zip(b, pa)], dtype)
        assert (fused_a != unfused).sum() > 10 and (fused_b != unfused).sum() > 10, dtype


def test_add_wrappers_reject_bad_tensors_without_a_device():
    from merge_spmv_amd.generators import DeviceCsr
    off = torch.zeros(4, dtype=torch.int32)
    col = torch.zeros(0, dtype=torch.int32)
    cpu = DeviceCsr(3, 3, off, col, None)
    with pytest.raises(M.MspmvError):
        M.csr_add(cpu, cpu)                                      # not on the device
    with pytest.raises(M.MspmvError):
        M.CsrAdd(cpu, cpu)
    with pytest.raises(M.MspmvError):
        M.csr_symmetrize(DeviceCsr(3, 4, off, col, None))        # not square


# ---------------------------------------------------------------------------------------------------------------- GPU plumbing
GUARD = 8
SENT_I, SENT_V = -0x5A5A5A5B, -12345.5


def _up(a, shift=0):
    """a host array on the device; shift > 0: as a slice starting `shift` elements into a larger tensor (not 16-byte aligned).  The
    library stages with dword loads whatever the alignment, so the shifted runs pin the contract (any element-aligned array is
    accepted and gives the same bits), not a second code path."""
    a = np.ascontiguousarray(a)
    if shift == 0:
        return torch.from_numpy(a).cuda()
    big = torch.zeros(a.size + shift + 3, dtype=torch.from_numpy(a).dtype, device="cuda")
    big[shift:shift + a.size] = torch.from_numpy(a).cuda()
    v = big[shift:shift + a.size]
    assert v.data_ptr() % 16 != 0 or a.size == 0
    return v


def _guarded(n, tdt, fill, shift=0):
    buf = torch.full((GUARD + shift + n + GUARD,), fill, dtype=tdt, device="cuda")
    return buf, buf[GUARD + shift:GUARD + shift + n]


def device_add(rows, cols, a, b, alpha, beta, dtype, shift=0, fill=(SENT_I, SENT_V), dev_inputs=None):
    """the C call on guarded outputs; returns (row_offsets, column_indices, values or None, count) as host arrays, after checking
    that the guard words and the entries past the count still hold what they were filled with"""
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    lib = M.load_library()
    fn = lib.mspmv_csr_add_f32 if dtype == np.float32 else lib.mspmv_csr_add_f64
    (oa, ca, va), (ob, cb, vb) = a, b
    structure = va is None
    if dev_inputs is None:
        dev_inputs = [None if x is None else _up(x, shift) for x in (oa, ca, va, ob, cb, vb)]
    doa, dca, dva, dob, dcb, dvb = dev_inputs
    na, nb = len(ca), len(cb)
    n = na + nb
    p = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() > 0 else 0)
    off_buf, off = _guarded(rows + 1, torch.int32, fill[0], shift)
    col_buf, col = _guarded(n, torch.int32, fill[0], shift)
    val_buf, val = (None, None) if structure else _guarded(n, tdt, fill[1], shift)
    cnt_buf, cnt = _guarded(1, torch.int32, fill[0])
    size = ctypes.c_size_t(0)
    args = lambda: (rows, cols, alpha, p(dva), p(doa), p(dca), na, beta, p(dvb), p(dob), p(dcb), nb, p(val), p(off), p(col), p(cnt))
    assert fn(None, ctypes.byref(size), *args(), None, 0) == 0
    tmp_buf = torch.full((size.value + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    status = fn(ctypes.c_void_p(tmp_buf.data_ptr()), ctypes.byref(size), *args(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), 0)
    assert status == 0, status
    torch.cuda.synchronize()
    assert bool((tmp_buf[size.value:] == 0x5A).all()), "temp storage overrun"
    count = int(cnt.item())
    assert 0 <= count <= n
    for name, buf, view, f in (("offsets", off_buf, off, fill[0]), ("columns", col_buf, col, fill[0]), ("values", val_buf, val, fill[1]),
                               ("count", cnt_buf, cnt, fill[0])):
        if buf is None:
            continue
        lead = GUARD + (shift if name != "count" else 0)
        assert bool((buf[:lead] == f).all()) and bool((buf[lead + view.numel():] == f).all()), f"guard words of the {name} were written"
        if name in ("columns", "values"):
            assert bool((view[count:] == f).all()), f"{name} past the count were written"
    return off.cpu().numpy(), col[:count].cpu().numpy(), None if structure else val[:count].cpu().numpy(), count


def _assert_equal(got, want, what=""):
    off, col, val, count = got
    woff, wcol, wval = want
    assert count == len(wcol), (what, count, len(wcol))
    assert np.array_equal(off, woff), what
    assert np.array_equal(col, wcol), what
    if wval is None:
        assert val is None
    else:
        assert val.dtype == wval.dtype and np.array_equal(val.view(np.uint8), wval.view(np.uint8)), what          # bit for bit


def _check_all_forms(rows, cols, A, B, what, alpha_beta=((1.0, 1.0), (0.5, -3.0)), shifts=(0,)):
    """fp32, fp64 and structure only; A, B carry fp64 values that are narrowed for fp32"""
    for shift in shifts:
        for dtype in (np.float32, np.float64):
            a, b = (A[0], A[1], A[2].astype(dtype)), (B[0], B[1], B[2].astype(dtype))
            for alpha, beta in alpha_beta:
                _assert_equal(device_add(rows, cols, a, b, alpha, beta, dtype, shift=shift), host_add(rows, cols, a, b, alpha, beta, dtype),
                              (what, dtype.__name__, alpha, beta, shift))
        s = ((A[0], A[1], None), (B[0], B[1], None))
        _assert_equal(device_add(rows, cols, *s, 1.0, 1.0, np.float32, shift=shift), host_add(rows, cols, *s), (what, "structure", shift))
        _assert_equal(device_add(rows, cols, *s, 1.0, 1.0, np.float64, shift=shift), host_add(rows, cols, *s), (what, "structure64", shift))


def _grid5(k, dtype=np.float64):
    """the 5-point stencil on a k x k grid (rows sorted by column)"""
    idx = np.arange(k * k).reshape(k, k)
    r, c = [idx.ravel()], [idx.ravel()]
    for sl_a, sl_b in ((np.s_[1:, :], np.s_[:-1, :]), (np.s_[:-1, :], np.s_[1:, :]), (np.s_[:, 1:], np.s_[:, :-1]), (np.s_[:, :-1], np.s_[:, 1:])):
        r.append(idx[sl_a].ravel()); c.append(idx[sl_b].ravel())
    r, c = np.concatenate(r).astype(np.int64), np.concatenate(c).astype(np.int64)
    rng = np.random.default_rng(4)
    return _csr_from_keys(k * k, k * k, np.sort(r * (k * k) + c), rng, dtype)


SHAPES = ["identical", "disjoint", "b_empty", "a_empty", "both_empty", "one_row", "mostly_empty_rows", "one_column", "diag_vs_grid",
          "one_tile_0", "one_tile_50", "one_tile_100", "few_tiles_0", "few_tiles_50", "few_tiles_100", "exact_tile", "one_entry_each"]


def _shape(name):
    """(rows, cols, A, B) with fp64 values"""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    d = np.float64
    empty = lambda rows: (np.zeros(rows + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, d))
    if name == "identical":
        A, _ = _random_pair(rng, 300, 400, 9000, 0, 1.0, d)
        return 300, 400, A, (A[0], A[1], rng.uniform(-1, 1, len(A[1])))
    if name == "disjoint":                                       # even / odd columns
        rows, cols = 200, 500
        ka = np.unique(rng.integers(0, rows * cols // 2, 8000)) * 2
        kb = np.unique(rng.integers(0, rows * cols // 2, 8000)) * 2 + 1
        return rows, cols, _csr_from_keys(rows, cols, ka, rng, d), _csr_from_keys(rows, cols, kb, rng, d)
    if name in ("b_empty", "a_empty", "both_empty"):
        A, _ = _random_pair(rng, 300, 400, 9000, 0, 1.0, d)
        return 300, 400, (empty(300) if name != "b_empty" else A), (empty(300) if name != "a_empty" else A)
    if name == "one_row":                                        # one row holds everything: 10^6 + 10^6 entries
        cols = 3_000_000
        ka, kb = np.unique(rng.integers(0, cols, 1_230_000))[:1_000_000], np.unique(rng.integers(0, cols, 1_230_000))[:1_000_000]
        assert len(ka) == len(kb) == 1_000_000
        return 1, cols, _csr_from_keys(1, cols, ka, rng, d), _csr_from_keys(1, cols, kb, rng, d)
    if name == "mostly_empty_rows":                              # 10^6 rows, 99 % of them empty in both
        rows, cols = 1_000_000, 1000
        live = np.sort(rng.choice(rows, 10_000, replace=False)).astype(np.int64)
        ka = np.unique(rng.choice(live, 60_000) * cols + rng.integers(0, cols, 60_000))
        kb = np.unique(rng.choice(live, 60_000) * cols + rng.integers(0, cols, 60_000))
        return rows, cols, _csr_from_keys(rows, cols, ka, rng, d), _csr_from_keys(rows, cols, kb, rng, d)
    if name == "one_column":
        rows = 50_000
        ka, kb = np.unique(rng.integers(0, rows, 20_000)), np.unique(rng.integers(0, rows, 20_000))
        return rows, 1, _csr_from_keys(rows, 1, ka, rng, d), _csr_from_keys(rows, 1, kb, rng, d)
    if name == "diag_vs_grid":                                   # A - sigma I: the grid against a diagonal
        k = 70
        G = _grid5(k)
        n = k * k
        return n, n, G, (np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n))
    if name == "exact_tile":                                     # nnz_a + nnz_b a multiple of the tile, rows ending on tile boundaries
        rows, cols = 4, TILE
        full = np.arange(rows * cols, dtype=np.int64)
        return rows, cols, _csr_from_keys(rows, cols, full, rng, d), _csr_from_keys(rows, cols, full, rng, d)
    if name == "one_entry_each":
        return 3, 3, (np.array([0, 0, 1, 1], np.int32), np.array([2], np.int32), np.array([1.5])), \
            (np.array([0, 0, 1, 1], np.int32), np.array([2], np.int32), np.array([-1.5]))
    size, overlap = name.rsplit("_", 1)
    n = {"one_tile": 600, "few_tiles": 5 * TILE}[size]
    A, B = _random_pair(rng, 97, 211, n, n, int(overlap) / 100.0, d)
    return 97, 211, A, B


# ---------------------------------------------------------------------------------------------------------------- GPU: shapes
@gpu
@pytest.mark.parametrize("name", SHAPES)
def test_add_is_the_host_union(name):
    rows, cols, A, B = _shape(name)
    big = name in ("one_row", "mostly_empty_rows")
    _check_all_forms(rows, cols, A, B, name, shifts=(0,) if big else (0, 1, 3))


@gpu
@pytest.mark.parametrize("overlap", [0, 50, 100])
def test_add_over_ten_thousand_tiles(overlap):
    rng = np.random.default_rng(overlap)
    rows, cols, n = 300_000, 250_000, 10_500 * TILE // 2
    A, B = _random_pair(rng, rows, cols, n, n, overlap / 100.0, np.float32)
    assert (len(A[1]) + len(B[1])) >= 10_000 * TILE
    _assert_equal(device_add(rows, cols, A, B, 0.5, -3.0, np.float32), host_add(rows, cols, A, B, 0.5, -3.0, np.float32), overlap)
    if overlap == 50:
        a, b = (A[0], A[1], A[2].astype(np.float64)), (B[0], B[1], B[2].astype(np.float64))
        _assert_equal(device_add(rows, cols, a, b, 1.0, -1.0, np.float64, shift=1), host_add(rows, cols, a, b, 1.0, -1.0, np.float64), overlap)


# ---------------------------------------------------------------------------------------------------------------- GPU: values
@gpu
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_add_values_are_two_products_and_one_sum(prec):
    dtype = np.float32 if prec == "f32" else np.float64
    rng = np.random.default_rng(6)
    A, B = _random_pair(rng, 500, 700, 30_000, 30_000, 0.5, dtype)
    for alpha, beta in ALPHA_BETA:
        _assert_equal(device_add(500, 700, A, B, alpha, beta, dtype), host_add(500, 700, A, B, alpha, beta, dtype), (alpha, beta))
    # a + b cancels to 0 in every shared entry: the entries stay
    Bm = (A[0], A[1], -A[2])
    off, col, val, count = got = device_add(500, 700, A, Bm, 1.0, 1.0, dtype)
    _assert_equal(got, host_add(500, 700, A, Bm, 1.0, 1.0, dtype))
    assert count == len(A[1]) and not val.any()
    # products that differ between fused and unfused evaluation (test_the_fma_case_tells_fused_from_unfused), 100 % overlap
    a, b, alpha, beta = _fma_pair(dtype)
    n = len(a)
    offs, colsi = np.array([0, n], np.int32), np.arange(n, dtype=np.int32) * 3
    got = device_add(1, 3 * n, (offs, colsi, a), (offs, colsi, b), alpha, beta, dtype)
    _assert_equal(got, host_add(1, 3 * n, (offs, colsi, a), (offs, colsi, b), alpha, beta, dtype), "fma")
    t = np.dtype(dtype).type
    assert np.array_equal(got[2], t(alpha) * a + t(beta) * b)


@gpu
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_a_plus_a_on_the_same_tensors(prec):
    dtype = np.float32 if prec == "f32" else np.float64
    rng = np.random.default_rng(8)
    A, _ = _random_pair(rng, 700, 900, 40_000, 0, 1.0, dtype)
    dev = [_up(x) for x in A]
    got = device_add(700, 900, A, A, 1.0, 1.0, dtype, dev_inputs=dev + dev)
    assert got[3] == len(A[1]) and np.array_equal(got[0], A[0]) and np.array_equal(got[1], A[1])
    assert np.array_equal(got[2], dtype(2) * A[2])
    for x, d in zip(A, dev):
        assert np.array_equal(d.cpu().numpy(), x)                # the inputs are as they were


@gpu
def test_add_is_deterministic():
    rng = np.random.default_rng(10)
    A, B = _random_pair(rng, 5000, 7000, 400_000, 400_000, 0.5, np.float64)
    one = device_add(5000, 7000, A, B, 0.5, -3.0, np.float64, fill=(SENT_I, SENT_V))
    two = device_add(5000, 7000, A, B, 0.5, -3.0, np.float64, fill=(0x01010101, 7.25))
    assert one[3] == two[3]
    for x, y in zip(one[:3], two[:3]):
        assert x.tobytes() == y.tobytes()


# ---------------------------------------------------------------------------------------------------------------- GPU: the wrappers
def _dcsr(rows, cols, m):
    from merge_spmv_amd.generators import DeviceCsr
    return DeviceCsr(rows, cols, _up(m[0]), _up(m[1]), None if m[2] is None else _up(m[2]))


@gpu
def test_csr_add_wrapper_and_trim():
    rng = np.random.default_rng(12)
    A, B = _random_pair(rng, 300, 400, 9000, 9000, 0.5, np.float32)
    want = host_add(300, 400, A, B, 2.0, 0.25, np.float32)
    c, count = M.csr_add(_dcsr(300, 400, A), _dcsr(300, 400, B), alpha=2.0, beta=0.25)
    n = int(count.item())
    assert n == len(want[1]) and c.column_indices.numel() == len(A[1]) + len(B[1])
    assert np.array_equal(c.row_offsets.cpu().numpy(), want[0]) and np.array_equal(c.column_indices[:n].cpu().numpy(), want[1])
    assert np.array_equal(c.values[:n].cpu().numpy(), want[2])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    c, count = M.csr_add(_dcsr(300, 400, A), _dcsr(300, 400, B), alpha=2.0, beta=0.25, stream=side, trim=True)
    assert c.column_indices.numel() == n == c.values.numel() and np.array_equal(c.values.cpu().numpy(), want[2])
    s, _ = M.csr_add(_dcsr(300, 400, (A[0], A[1], None)), _dcsr(300, 400, (B[0], B[1], None)), trim=True)
    assert s.values is None and np.array_equal(s.column_indices.cpu().numpy(), want[1])


@gpu
def test_add_wrappers_reject_bad_tensors():
    from merge_spmv_amd.generators import DeviceCsr
    rng = np.random.default_rng(13)
    A, B = _random_pair(rng, 30, 40, 200, 200, 0.5, np.float32)
    a, b = _dcsr(30, 40, A), _dcsr(30, 40, B)
    with pytest.raises(M.MspmvError):
        M.csr_add(a, DeviceCsr(31, 40, torch.cat([b.row_offsets, b.row_offsets[-1:]]), b.column_indices, b.values))       # rows differ
    with pytest.raises(M.MspmvError):
        M.csr_add(a, DeviceCsr(30, 40, b.row_offsets, b.column_indices, None))                    # values for one only
    with pytest.raises(M.MspmvError):
        M.csr_add(a, DeviceCsr(30, 40, b.row_offsets, b.column_indices, b.values.double()))       # dtypes differ
    with pytest.raises(M.MspmvError):
        M.csr_add(a, DeviceCsr(30, 40, b.row_offsets.long(), b.column_indices, b.values))
    with pytest.raises(M.MspmvError):
        M.csr_add(a, DeviceCsr(30, 40, b.row_offsets, b.column_indices[::2], b.values[::2]))      # not contiguous
    with pytest.raises(M.MspmvError):
        M.csr_add(a, DeviceCsr(30, 40, b.row_offsets, b.column_indices, b.values[:-1]))
    with pytest.raises(M.MspmvError):
        M.csr_add(a, DeviceCsr(30, 40, b.row_offsets.cpu(), b.column_indices, b.values))
    with pytest.raises(TypeError):
        M.csr_add(DeviceCsr(30, 40, a.row_offsets, a.column_indices, a.values.half()), b)


@gpu
@pytest.mark.parametrize("label", ["mtx_general_dups", None])
def test_symmetrize_a_golden_matrix(label):
    """A + A^T through csr_symmetrize against the host union of A and its host transpose (duplicates merged on the host first)"""
    cases = load_golden("matrices.json")["cases"]
    case = next(c for c in cases if c["label"] == label) if label else next(c for c in cases if c["rows"] == c["cols"] and c["nnz"] > 50)
    n = max(case["rows"], case["cols"])                         # (made square by padding with empty rows / columns)
    off = np.asarray(case["row_offsets"], np.int64)
    r = np.repeat(np.arange(case["rows"]), np.diff(off)).astype(np.int64)
    c = np.asarray(case["column_indices"], np.int64)
    v = np.asarray(case["f64"]["values"], np.float64)
    keys, first = np.unique(r * n + c, return_index=True)        # canonical: one entry per (row, column), the first value of each
    A = _csr_from_keys(n, n, keys, np.random.default_rng(0), np.float64)
    A = (A[0], A[1], v[first])
    tk = (keys % n) * n + keys // n
    o = np.argsort(tk, kind="stable")
    At = _csr_from_keys(n, n, tk[o], np.random.default_rng(0), np.float64)
    At = (At[0], At[1], A[2][o])
    want = host_add(n, n, A, At, 1.0, 1.0, np.float64)
    got = M.csr_symmetrize(_dcsr(n, n, A))
    assert np.array_equal(got.row_offsets.cpu().numpy(), want[0]) and np.array_equal(got.column_indices.cpu().numpy(), want[1])
    assert np.array_equal(got.values.cpu().numpy(), want[2])
    # symmetric: its own transpose has the same pattern
    vt, ot, ct, _ = M.csr_transpose(got.values, got.row_offsets, got.column_indices, n)
    assert torch.equal(ot, got.row_offsets) and torch.equal(ct, got.column_indices) and torch.equal(vt, got.values)


# ---------------------------------------------------------------------------------------------------------------- GPU: composition
@gpu
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_csrmv_on_the_sum(prec):
    dtype, tdt, vb = (np.float32, torch.float32, 4) if prec == "f32" else (np.float64, torch.float64, 8)
    rng = np.random.default_rng(14)
    rows, cols = 20_000, 15_000
    A, B = _random_pair(rng, rows, cols, 300_000, 300_000, 0.5, dtype)
    want = host_add(rows, cols, A, B, 1.0, 1.0, dtype)
    c, _ = M.csr_add(_dcsr(rows, cols, A), _dcsr(rows, cols, B), trim=True)
    x = rng.uniform(-1, 1, cols).astype(dtype)
    dx = _up(x)
    y = M.csrmv(c.values, c.row_offsets, c.column_indices, dx, num_cols=cols)
    yw = M.csrmv(_up(want[2]), _up(want[0]), _up(want[1]), dx, num_cols=cols)
    torch.cuda.synchronize()
    assert torch.equal(y, yw)
    # within the oracle's bound of A x + B x: the union's entries are a + b rounded once, so compare against the product of the
    # host union (the exact sum of A x and B x up to that one rounding per shared entry, which the bound's |a||x| terms cover)
    csr = O.Csr(rows, cols, want[0], want[1], want[2])
    gold, s = O.spmv_gold_acc64(csr, x)
    ok, worst = O.strict_check(csr, y.cpu().numpy(), gold, s, items_per_thread=M.serial_sum_depth(rows, cols, len(want[1]), vb))
    assert ok, worst
    # ... and of A x + B x: an entry of the union is a + b rounded once, an error of at most eps (|a| + |b|) |x| per shared entry on
    # top of the product's own c eps s(union), s(union) <= (1 + eps) (s(A) + s(B)): together below (c + 2) eps (s(A) + s(B)), which
    # is the oracle's bound with one more item of depth
    ga, sa = O.spmv_gold_acc64(O.Csr(rows, cols, *A), x)
    gb, sb = O.spmv_gold_acc64(O.Csr(rows, cols, *B), x)
    ok, worst = O.strict_check(csr, y.cpu().numpy(), ga + gb, sa + sb, items_per_thread=M.serial_sum_depth(rows, cols, len(want[1]), vb) + 1)
    assert ok, worst


# ---------------------------------------------------------------------------------------------------------------- GPU: graph capture
@gpu
def test_add_and_multiply_replay_in_a_graph_on_new_patterns():
    """CsrAdd reads nothing back on the host: captured once with csrmv on a side stream (one linear chain), replayed after the
    addends' values AND patterns (same counts) were overwritten in place, it gives the new sum every time"""
    from merge_spmv_amd.generators import DeviceCsr
    rows, cols, na, nb = 8000, 6000, 150_000, 120_000
    rng = np.random.default_rng(15)

    def pair():                                                  # half of B's entries are A's, half lie outside A: the union has k
        ka = np.sort(rng.choice(rows * cols, na, replace=False))
        fresh = np.setdiff1d(rng.choice(rows * cols, nb, replace=False), ka)[:nb // 2]
        kb = np.union1d(rng.choice(ka, nb // 2, replace=False), fresh)
        assert len(kb) == nb
        return _csr_from_keys(rows, cols, ka, rng, np.float32), _csr_from_keys(rows, cols, kb, rng, np.float32)

    A, B = pair()
    a, b = _dcsr(rows, cols, A), _dcsr(rows, cols, B)
    x = _up(rng.uniform(-1, 1, cols).astype(np.float32))
    y = torch.zeros(rows, dtype=torch.float32, device="cuda")
    op = M.CsrAdd(a, b, alpha=0.5, beta=-3.0)                   # (allocates the outputs and the temp storage once)
    k = na + nb // 2                                             # the union's count, the same for every pair: csrmv needs it on the host
    assert int(op.count.item()) == k
    cv, cc = op.values[:k], op.column_indices[:k]
    ws = M.CsrMVWorkspace(rows, k, torch.float32)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        op.add(stream=side)                                      # warm-up outside the capture
        M.csrmv(cv, op.row_offsets, cc, x, y, num_cols=cols, workspace=ws, stream=side)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            op.add(stream=side)
            M.csrmv(cv, op.row_offsets, cc, x, y, num_cols=cols, workspace=ws, stream=side)
    torch.cuda.synchronize()
    for _ in range(3):
        A, B = pair()
        for t, h in zip((a.row_offsets, a.column_indices, a.values, b.row_offsets, b.column_indices, b.values), A + B):
            t.copy_(_up(h))
        y.fill_(float("nan"))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want = host_add(rows, cols, A, B, 0.5, -3.0, np.float32)
        assert int(op.count.item()) == k == len(want[1]) and np.array_equal(op.row_offsets.cpu().numpy(), want[0])
        assert np.array_equal(cc.cpu().numpy(), want[1]) and np.array_equal(cv.cpu().numpy(), want[2])
        yw = M.csrmv(_up(want[2]), _up(want[0]), _up(want[1]), x, num_cols=cols)
        torch.cuda.synchronize()
        assert torch.equal(y, yw)


# ---------------------------------------------------------------------------------------------------------------- GPU: the limit
@gpu
def test_add_at_the_item_limit():
    """rows + nnz_a + nnz_b = MAX_ITEMS, structure only: closed-formula inputs made on the device, exact integer reference
    (tests/csr_add_limit_worker.py, run once in a process of its own under a time limit; exit status 77 = not enough free device
    memory)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "csr_add_limit_worker.py")], capture_output=True, text=True, timeout=900)
    if r.returncode == 77:
        pytest.skip(r.stdout.strip().splitlines()[-1])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "add limit OK" in r.stdout
