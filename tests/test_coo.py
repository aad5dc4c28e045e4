"""CSR from unsorted COO on the device, duplicate summing and the stateless COO SpMV (include/mspmv.h: mspmv_coo_to_csr_*,
mspmv_coo_to_csr_values_*, mspmv_csr_sum_duplicates_*, mspmv_coomv_*; merge_spmv_amd.coo_to_csr / CooToCsr / csr_sum_duplicates /
coomv).  CPU: exports, size-query conventions, and the expected-result builders of the GPU tests pinned to the reference's own
CsrMatrix(coo) through tests/golden.  GPU: the build is bit for bit the stable sort by (row, column) -- numpy's lexsort on the
host, two stable torch sorts on the device for the large inputs -- deterministic, writes nothing outside its arrays, can be captured
in a graph; the COO SpMV is bit for bit the forward call on the builder's CSR and within the strict bound of the fp64 oracle.
Expected values never come from the code under test."""
import ctypes
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import merge_spmv_amd as M
from conftest import ROOT, load_golden
from oracle import oracle as O

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

NEW = ["mspmv_coo_to_csr_f32", "mspmv_coo_to_csr_f64", "mspmv_coo_to_csr_values_f32", "mspmv_coo_to_csr_values_f64",
       "mspmv_csr_sum_duplicates_f32", "mspmv_csr_sum_duplicates_f64", "mspmv_coomv_f32", "mspmv_coomv_f64"]
MAX_ITEMS = 2 ** 31 - 1 - 65536


# ---------------------------------------------------------------------------------------------------------------- expected results
def host_build(rows, r, c, v=None):
    """the reference's CsrMatrix(coo): the triples sorted stably by (row, column), duplicates kept"""
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    perm = np.lexsort((c, r))                                    # (stable; the last key is the primary one)
    off = np.zeros(rows + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=rows), out=off[1:])
    return off.astype(np.int32), c[perm].astype(np.int32), None if v is None else np.asarray(v)[perm], perm.astype(np.int32)


def host_sum_duplicates(rows, off, col, val=None):
    """every run of equal (row, column) of a sorted CSR merged, the run's values added left to right in the value type"""
    out_off, out_col, out_val = [0], [], []
    for r in range(rows):
        for j in range(off[r], off[r + 1]):
            if j > off[r] and col[j] == col[j - 1]:
                if val is not None:
                    out_val[-1] = val.dtype.type(out_val[-1] + val[j])
            else:
                out_col.append(col[j])
                if val is not None:
                    out_val.append(val[j])
        out_off.append(len(out_col))
    return (np.asarray(out_off, np.int32), np.asarray(out_col, np.int32).reshape(-1),
            None if val is None else np.asarray(out_val, val.dtype).reshape(-1))


def _mtx_triples(path):
    lines = [l for l in open(path).read().splitlines() if l.strip() and not l.startswith("%")]
    rows, cols, nnz = (int(t) for t in lines[0].split())
    t = [l.split() for l in lines[1:1 + nnz]]
    return rows, cols, np.array([int(a[0]) - 1 for a in t]), np.array([int(a[1]) - 1 for a in t]), np.array([float(a[2]) for a in t])


def _golden_cases():
    return load_golden("matrices.json")["cases"]


def _golden_triples(case, dtype):
    off = np.asarray(case["row_offsets"], np.int64)
    r = np.repeat(np.arange(case["rows"]), np.diff(off))
    return r, np.asarray(case["column_indices"], np.int64), np.asarray(case["f32" if dtype == np.float32 else "f64"]["values"], dtype)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_coo_symbols_are_declared_and_exported():
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
    assert lib.mspmv_version() == 102


def _callers(lib, prec):
    """(name, call(temp, size, rows, cols, nnz, fake)) of the three families with temp storage"""
    build, dups, mv = (getattr(lib, s + prec) for s in ("mspmv_coo_to_csr_", "mspmv_csr_sum_duplicates_", "mspmv_coomv_"))
    return [
        ("coo_to_csr", lambda t, sz, r, c, n, f=None: build(t, ctypes.byref(sz), f, f, f, r, c, n, f, f, f, None, None, 0)),
        ("sum_duplicates", lambda t, sz, r, c, n, f=None: dups(t, ctypes.byref(sz), f, f, f, r, c, n, f, f, f, f, None, 0)),
        ("coomv", lambda t, sz, r, c, n, f=None: mv(t, ctypes.byref(sz), f, f, f, f, f, r, c, n, 1.0, 0.0, None, 0)),
    ]


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_coo_size_query_conventions(prec):
    lib = M.load_library()
    fake = ctypes.c_void_p(4096)
    for name, call in _callers(lib, prec):
        size = ctypes.c_size_t(0)
        assert call(None, size, 1000, 1000, 50000) == 0 and size.value > 0, name
        need = size.value
        # more index bits -> more digit passes -> never less storage
        for rows, cols in ((1000, 1 << 20), (1 << 20, 1000), (1 << 20, 1 << 20)):
            big = ctypes.c_size_t(0)
            assert call(None, big, rows, cols, 50000) == 0 and big.value >= need, (name, rows, cols)
        for rows, cols, nnz in ((0, 0, 0), (0, 7, 0), (7, 0, 0), (5, 5, 0), (5, 1, 9), (1, 5, 9)):
            assert call(None, size, rows, cols, nnz) == 0 and size.value > 0, (name, rows, cols, nnz)
        # too small / misaligned temp storage; missing arrays; negative sizes; nonzeros without rows or columns
        assert call(ctypes.c_void_p(256), ctypes.c_size_t(need - 1), 1000, 1000, 50000, fake) == 1, name
        for misaligned in (4096 + 1, 4096 + 4, 4096 + 8):
            assert call(ctypes.c_void_p(misaligned), ctypes.c_size_t(need + 64), 1000, 1000, 50000, fake) == 1, name
        assert call(ctypes.c_void_p(4096), ctypes.c_size_t(need + 64), 1000, 1000, 50000, None) == 1, name
        for rows, cols, nnz in ((-1, 5, 5), (5, -1, 5), (5, 5, -1), (0, 5, 5), (5, 0, 5)):
            assert call(None, size, rows, cols, nnz) == 1, (name, rows, cols, nnz)
        # what is built can be multiplied: rows + nnz within the forward call's bound
        assert call(None, size, 1000, 1000, MAX_ITEMS - 1000) == 0, name
        assert call(None, size, 1001, 1000, MAX_ITEMS - 1000) == 1, name
        assert call(None, size, 1000, 1 << 30, MAX_ITEMS - 1000) == 0, name          # (columns do not count)
    assert lib.mspmv_coo_to_csr_f32(None, None, None, None, None, 5, 5, 5, None, None, None, None, None, 0) == 1
    # only one of values / values_csr given
    size = ctypes.c_size_t(1 << 30)
    build = getattr(lib, "mspmv_coo_to_csr_" + prec)
    assert build(fake, ctypes.byref(size), fake, fake, fake, 5, 5, 5, fake, fake, None, None, None, 0) == 1
    assert build(fake, ctypes.byref(size), None, fake, fake, 5, 5, 5, fake, fake, fake, None, None, 0) == 1
    dups = getattr(lib, "mspmv_csr_sum_duplicates_" + prec)
    assert dups(fake, ctypes.byref(size), fake, fake, fake, 5, 5, 5, fake, fake, fake, None, None, 0) == 1       # no place for the count
    vfn = getattr(lib, "mspmv_coo_to_csr_values_" + prec)
    assert vfn(None, None, None, 0, None, 0) == 0
    assert vfn(None, fake, fake, 10, None, 0) == 1 and vfn(fake, fake, fake, -1, None, 0) == 1


def test_coomv_size_query_covers_the_build_the_matrix_and_the_forward_call():
    lib = M.load_library()
    for prec, vb in (("f32", 4), ("f64", 8)):
        rows, cols, nnz = 3000, 1000, 50000
        total, b, f = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert getattr(lib, "mspmv_coomv_" + prec)(None, ctypes.byref(total), None, None, None, None, None, rows, cols, nnz, 1.0, 0.0, None, 0) == 0
        assert getattr(lib, "mspmv_coo_to_csr_" + prec)(None, ctypes.byref(b), None, None, None, rows, cols, nnz, None, None, None, None, None, 0) == 0
        assert getattr(lib, "mspmv_csrmv_axpby_" + prec)(None, ctypes.byref(f), None, None, None, None, None, rows, cols, nnz, 1.0, 0.0, None, 0) == 0
        assert total.value >= b.value + f.value + nnz * (4 + vb) + (rows + 1) * 4


def test_host_builder_reproduces_the_reference_on_general_dups():
    """the builder the GPU tests compare against IS the reference's CsrMatrix(coo): golden mtx_general_dups came from the reference's
    own code reading this file (unsorted, a duplicated entry, empty rows)"""
    case = next(c for c in _golden_cases() if c["label"] == "mtx_general_dups")
    rows, cols, r, c, v = _mtx_triples(os.path.join(ROOT, "tests/golden/mtx/general_dups.mtx"))
    assert (rows, cols, len(r)) == (case["rows"], case["cols"], case["nnz"])
    for dtype, key in ((np.float32, "f32"), (np.float64, "f64")):
        off, col, val, perm = host_build(rows, r, c, v.astype(dtype))
        assert off.tolist() == case["row_offsets"] and col.tolist() == case["column_indices"]
        assert np.array_equal(val, np.asarray(case[key]["values"], dtype))
        assert np.array_equal(val, v.astype(dtype)[perm])
        # the duplicate sum by hand: (2,3) -> -4.0 + 0.5 = -3.5, 8 entries left
        o2, c2, v2 = host_sum_duplicates(rows, off, col, val)
        assert o2.tolist() == [0, 3, 4, 6, 6, 8, 8] and c2.tolist() == [0, 1, 4, 2, 0, 4, 1, 3]
        assert v2.dtype == dtype and v2[3] == dtype(-3.5) and len(v2) == 8
        assert np.array_equal(np.delete(v2, 3), np.delete(val, [3, 4]))


def test_host_builder_gives_every_golden_csr_back_from_a_shuffle():
    cases = _golden_cases()
    assert len(cases) == 21
    for case in cases:
        for dtype in (np.float32, np.float64):
            r, c, v = _golden_triples(case, dtype)
            sh = np.random.default_rng(zlib.crc32(case["label"].encode())).permutation(len(r))
            # (a shuffle reorders duplicates: shuffle the positions, then restore input order among equal (row, col) by sorting the
            # shuffled positions inside each group -- only mtx_general_dups has any)
            key = r[sh] * case["cols"] + c[sh]
            for k in np.unique(key):
                g = np.nonzero(key == k)[0]
                sh[g] = np.sort(sh[g])
            off, col, val, perm = host_build(case["rows"], r[sh], c[sh], v[sh])
            assert off.tolist() == case["row_offsets"] and col.tolist() == case["column_indices"], case["label"]
            assert np.array_equal(val, v), case["label"]
            assert np.array_equal(sh[perm], np.arange(len(r))), case["label"]


def test_host_sum_duplicates_adds_left_to_right():
    # 1e8 + 1 - 1e8 in fp32: left to right gives 0 (1e8 + 1 rounds to 1e8); any other order gives 1
    off, col = np.array([0, 3], np.int32), np.array([2, 2, 2], np.int32)
    _, c2, v2 = host_sum_duplicates(1, off, col, np.array([1e8, 1.0, -1e8], np.float32))
    assert c2.tolist() == [2] and v2.tolist() == [0.0]


# ---------------------------------------------------------------------------------------------------------------- GPU inputs
def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _random_triples(rng, rows, cols, nnz, top=True):
    r, c = rng.integers(0, rows, nnz), rng.integers(0, cols, nnz)
    if top and nnz > 0:                                          # the largest indices are present: every digit pass has work
        r[rng.integers(0, nnz)] = rows - 1; c[rng.integers(0, nnz)] = cols - 1
    return r, c


DIMS = [1, 255, 256, 257, 65536, 65537, (1 << 24) + 1]
NNZS = [1, 63, 64, 65, 2047, 2048, 2049]
SMALL = (["general_dups_file_order", "sorted", "reverse_sorted", "one_row", "one_column", "row_vector", "column_vector", "empty",
          "empty_leading_rows", "empty_trailing_rows", "every_other_row_empty", "one_by_one", "many_tiles"] +
         [f"golden_{i}" for i in range(21)] + [f"nnz_{n}" for n in NNZS] + [f"dims_{d}_{d}" for d in DIMS] +
         ["dims_1_16777217", "dims_16777217_1", "dims_257_65537", "dims_65537_255", "dims_256_16777217", "dims_16777217_65536"])


def _case(name, dtype):
    """(rows, cols, row indices, column indices, values) of a named input, on the host"""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    vals = lambda n: rng.uniform(-1, 1, n).astype(dtype)
    if name == "general_dups_file_order":
        rows, cols, r, c, v = _mtx_triples(os.path.join(ROOT, "tests/golden/mtx/general_dups.mtx"))
        return rows, cols, r, c, v.astype(dtype)
    if name.startswith("golden_"):
        case = _golden_cases()[int(name[7:])]
        r, c, v = _golden_triples(case, dtype)
        sh = rng.permutation(len(r))
        return case["rows"], case["cols"], r[sh], c[sh], v[sh]
    if name in ("sorted", "reverse_sorted"):
        r, c = _random_triples(rng, 3000, 5000, 40000)
        o = np.lexsort((c, r))
        o = o if name == "sorted" else o[::-1]
        return 3000, 5000, r[o], c[o], vals(40000)
    if name == "one_row":
        return 700, 9000, np.full(30000, 413), rng.integers(0, 9000, 30000), vals(30000)
    if name == "one_column":
        return 9000, 700, rng.integers(0, 9000, 30000), np.full(30000, 77), vals(30000)
    if name == "row_vector":
        return 1, 50000, np.zeros(20000, np.int64), rng.integers(0, 50000, 20000), vals(20000)
    if name == "column_vector":
        return 50000, 1, rng.integers(0, 50000, 20000), np.zeros(20000, np.int64), vals(20000)
    if name == "empty":
        return 300, 400, np.zeros(0, np.int64), np.zeros(0, np.int64), vals(0)
    if name == "one_by_one":
        return 1, 1, np.zeros(5000, np.int64), np.zeros(5000, np.int64), vals(5000)
    if name == "empty_leading_rows":
        return 5000, 300, rng.integers(4000, 5000, 9000), rng.integers(0, 300, 9000), vals(9000)
    if name == "empty_trailing_rows":
        return 5000, 300, rng.integers(0, 700, 9000), rng.integers(0, 300, 9000), vals(9000)
    if name == "every_other_row_empty":
        return 5000, 300, rng.integers(0, 2500, 9000) * 2 + 1, rng.integers(0, 300, 9000), vals(9000)
    if name == "many_tiles":                                    # 3000 tiles and a ragged last one
        n = 3000 * 2048 + 777
        r, c = _random_triples(rng, 100000, 70000, n)
        return 100000, 70000, r, c, vals(n)
    if name.startswith("nnz_"):
        n = int(name[4:])
        r, c = _random_triples(rng, 300, 70000, n, top=n > 1)
        return 300, 70000, r, c, vals(n)
    if name.startswith("dims_"):
        rows, cols = (int(t) for t in name[5:].split("_"))
        r, c = _random_triples(rng, rows, cols, 30000)
        return rows, cols, r, c, vals(30000)
    raise KeyError(name)


def _check_build(got, perm, want, with_values=True):
    off, col, val, wperm = want
    assert np.array_equal(got.row_offsets.cpu().numpy(), off)
    assert np.array_equal(got.column_indices.cpu().numpy(), col)
    if perm is not None:
        assert np.array_equal(perm.cpu().numpy(), wperm)
    if with_values:
        assert got.values.dtype == _d(val).dtype
        assert np.array_equal(got.values.cpu().numpy().view(np.uint8), val.view(np.uint8))          # bit for bit
    else:
        assert got.values is None


# ---------------------------------------------------------------------------------------------------------------- GPU: the build
@gpu
@pytest.mark.parametrize("name", SMALL)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_coo_to_csr_is_the_stable_host_sort(name, prec):
    dtype = np.float32 if prec == "f32" else np.float64
    rows, cols, r, c, v = _case(name, dtype)
    want = host_build(rows, r, c, v)
    dr, dc, dv = _d(r.astype(np.int32)), _d(c.astype(np.int32)), _d(v)
    got, perm = M.coo_to_csr(dv, dr, dc, rows, cols, return_permutation=True)
    torch.cuda.synchronize()
    assert (got.rows, got.cols, got.nnz) == (rows, cols, len(r))
    _check_build(got, perm, want)
    got = M.coo_to_csr(dv, dr, dc, rows, cols)                   # no permutation asked for
    torch.cuda.synchronize()
    _check_build(got, None, want)
    got, perm = M.coo_to_csr(None, dr, dc, rows, cols, return_permutation=True)         # structure only
    torch.cuda.synchronize()
    _check_build(got, perm, want, with_values=False)
    # the inputs are as they were
    assert np.array_equal(dr.cpu().numpy(), r) and np.array_equal(dc.cpu().numpy(), c) and np.array_equal(dv.cpu().numpy(), v)


def _device_build(rows, r, c, v=None):
    """the stable sort by (row, column) on the device with torch alone: a stable sort by column, then a stable sort by row"""
    p1 = torch.sort(c.to(torch.int64), stable=True).indices
    p2 = torch.sort(r.to(torch.int64)[p1], stable=True).indices
    perm = p1[p2]
    off = torch.zeros(rows + 1, dtype=torch.int64, device=r.device)
    off[1:] = torch.cumsum(torch.bincount(r.to(torch.int64), minlength=rows), 0)
    return off.to(torch.int32), c[perm].to(torch.int32), None if v is None else v[perm], perm.to(torch.int32)


def _large(kind, tdt):
    from merge_spmv_amd import generators as G
    g = torch.Generator(device="cuda"); g.manual_seed(7)
    if kind == "heavy_duplicates":                               # 10^6 entries over 16 x 16: stability is the whole test
        rows = cols = 16
        r = torch.randint(0, 16, (1_000_000,), device="cuda", generator=g, dtype=torch.int32)
        c = torch.randint(0, 16, (1_000_000,), device="cuda", generator=g, dtype=torch.int32)
    elif kind == "rmat":                                         # R-MAT edges at scale 20: duplicates occur
        rows = cols = 1 << 20
        r, c = G.rmat_edges(20, 0, 3_100_000, "cuda", G.SEED_C5)
        assert int(torch.unique(r * cols + c).numel()) < r.numel()
        sh = torch.randperm(r.numel(), device="cuda", generator=g)
        r, c = r[sh].to(torch.int32), c[sh].to(torch.int32)
    else:
        raise KeyError(kind)
    # small integers: sums of duplicates are exact in either precision whatever the order
    v = torch.randint(-4, 5, (r.numel(),), device="cuda", generator=g).to(tdt)
    return rows, cols, r.contiguous(), c.contiguous(), v


@gpu
@pytest.mark.parametrize("kind", ["heavy_duplicates", "rmat"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_coo_to_csr_large_inputs(kind, prec):
    tdt = torch.float32 if prec == "f32" else torch.float64
    rows, cols, r, c, v = _large(kind, tdt)
    got, perm = M.coo_to_csr(v, r, c, rows, cols, return_permutation=True)
    off, col, val, wperm = _device_build(rows, r, c, v)
    assert torch.equal(got.row_offsets, off) and torch.equal(got.column_indices, col) and torch.equal(perm, wperm)
    assert got.values.dtype == tdt and torch.equal(got.values, val)
    # duplicates merged: structure, count and (integer-valued, so exact) values against torch's unique / index_add
    merged = M.coo_to_csr(v, r, c, rows, cols, sum_duplicates=True)
    key = r.to(torch.int64) * cols + c.to(torch.int64)
    uniq, inv = torch.unique(key, return_inverse=True)
    sums = torch.zeros(uniq.numel(), dtype=torch.float64, device="cuda").index_add_(0, inv, v.to(torch.float64))
    woff = torch.zeros(rows + 1, dtype=torch.int64, device="cuda")
    woff[1:] = torch.cumsum(torch.bincount(uniq // cols, minlength=rows), 0)
    assert merged.nnz == uniq.numel() and merged.column_indices.numel() == uniq.numel()
    assert torch.equal(merged.row_offsets, woff.to(torch.int32))
    assert torch.equal(merged.column_indices, (uniq % cols).to(torch.int32))
    assert torch.equal(merged.values, sums.to(tdt))
    # idempotent on its own output
    v2, o2, c2, n2 = M.csr_sum_duplicates(merged.values, merged.row_offsets, merged.column_indices, cols)
    assert int(n2.item()) == merged.nnz
    assert torch.equal(o2, merged.row_offsets) and torch.equal(c2, merged.column_indices) and torch.equal(v2, merged.values)


# ---------------------------------------------------------------------------------------------------------------- GPU: determinism, guards
@gpu
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_coo_to_csr_is_deterministic_and_stays_inside_its_arrays(prec):
    tdt = torch.float32 if prec == "f32" else torch.float64
    rows, cols, r, c, v = _large("rmat", tdt)
    nnz = r.numel()
    keep = (r.clone(), c.clone(), v.clone())
    lib = M.load_library()
    fn = getattr(lib, "mspmv_coo_to_csr_" + prec)
    size = ctypes.c_size_t(0)
    assert fn(None, ctypes.byref(size), None, None, None, rows, cols, nnz, None, None, None, None, None, 0) == 0
    GUARD, PAT = 64, 0x5A

    def run(stream):
        # every output array and the temp storage carry GUARD bytes of a pattern behind their last byte
        bufs = {"off": (rows + 1) * 4, "col": nnz * 4, "val": nnz * v.element_size(), "perm": nnz * 4, "temp": size.value}
        t = {k: torch.full((n + GUARD,), PAT, dtype=torch.uint8, device="cuda") for k, n in bufs.items()}
        assert all(x.data_ptr() % 16 == 0 for x in t.values())
        torch.cuda.synchronize()
        sz = ctypes.c_size_t(size.value)
        p = lambda x: ctypes.c_void_p(x.data_ptr())
        assert fn(p(t["temp"]), ctypes.byref(sz), p(v), p(r), p(c), rows, cols, nnz, p(t["off"]), p(t["col"]), p(t["val"]), p(t["perm"]),
                  ctypes.c_void_p(stream.cuda_stream), 0) == 0
        stream.synchronize()
        for k, n in bufs.items():
            assert bool((t[k][n:] == PAT).all()), k
        return {k: t[k][:n].clone() for k, n in bufs.items() if k != "temp"}

    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a, b, a2 = run(s1), run(s2), run(s1)
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], a2[k]), k
    off, col, val, perm = _device_build(rows, r, c, v)
    assert torch.equal(a["off"].view(torch.int32), off) and torch.equal(a["col"].view(torch.int32), col)
    assert torch.equal(a["perm"].view(torch.int32), perm) and torch.equal(a["val"].view(tdt), val)
    for x, y in zip(keep, (r, c, v)):
        assert torch.equal(x, y)                                 # the inputs are as they were


@gpu
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_refreshed_values_equal_a_fresh_build(prec):
    dtype = np.float32 if prec == "f32" else np.float64
    rows, cols, r, c, v = _case("many_tiles", dtype)
    dr, dc = _d(r.astype(np.int32)), _d(c.astype(np.int32))
    b = M.CooToCsr(_d(v), dr, dc, rows, cols)
    new = np.random.default_rng(5).uniform(-2, 2, len(r)).astype(dtype)
    b.refresh_values(_d(new))
    fresh = M.coo_to_csr(_d(new), dr, dc, rows, cols)
    torch.cuda.synchronize()
    want = host_build(rows, r, c, new)
    _check_build(fresh, None, want)
    assert torch.equal(b.values, fresh.values) and torch.equal(b.row_offsets, fresh.row_offsets) and torch.equal(b.column_indices, fresh.column_indices)
    with pytest.raises(M.MspmvError):
        b.refresh_values(_d(new[:-1]))


# ---------------------------------------------------------------------------------------------------------------- GPU: duplicates
@gpu
@pytest.mark.parametrize("name", ["general_dups_file_order", "one_by_one", "one_row", "one_column", "empty", "golden_4", "nnz_2049",
                                  "every_other_row_empty", "cancelling"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_sum_duplicates_adds_each_run_left_to_right(name, prec):
    dtype = np.float32 if prec == "f32" else np.float64
    if name == "cancelling":            # runs whose value depends on the order of the adds: 1e8 + 1 - 1e8 and friends, 40 x 7 cells
        rng = np.random.default_rng(3)
        rows, cols = 40, 7
        r, c = rng.integers(0, rows, 6000), rng.integers(0, cols, 6000)
        v = (rng.choice([1e8, -1e8, 1.0, 3.0, 1e-3], 6000) * rng.choice([1, -1], 6000)).astype(dtype)
    else:
        rows, cols, r, c, v = _case(name, dtype)
    off, col, val, _ = host_build(rows, r, c, v)
    woff, wcol, wval = host_sum_duplicates(rows, off, col, val)
    got = M.coo_to_csr(_d(v), _d(r.astype(np.int32)), _d(c.astype(np.int32)), rows, cols, sum_duplicates=True)
    assert got.nnz == len(wcol) and np.array_equal(got.row_offsets.cpu().numpy(), woff)
    assert np.array_equal(got.column_indices.cpu().numpy(), wcol)
    assert np.array_equal(got.values.cpu().numpy().view(np.uint8), wval.view(np.uint8))
    # the C call itself: entries past the count are left untouched; structure-only mode
    dv, do, dc = _d(val), _d(off), _d(col)
    v2, o2, c2, n2 = M.csr_sum_duplicates(None, do, dc, cols)
    assert v2 is None and int(n2.item()) == len(wcol) and np.array_equal(o2.cpu().numpy(), woff)
    assert np.array_equal(c2.cpu().numpy()[:len(wcol)], wcol)
    # idempotent
    v3, o3, c3, n3 = M.csr_sum_duplicates(got.values, got.row_offsets, got.column_indices, cols)
    assert int(n3.item()) == got.nnz and torch.equal(o3, got.row_offsets)
    assert torch.equal(c3[:got.nnz], got.column_indices) and torch.equal(v3[:got.nnz], got.values)
    del dv


# ---------------------------------------------------------------------------------------------------------------- GPU: COO SpMV
def _spmv_case(name, tdt):
    """(rows, cols, r, c, v) on the device, and what the forward call must run for the built matrix"""
    g = torch.Generator(device="cuda"); g.manual_seed(11)
    ri = lambda hi, n: torch.randint(0, hi, (n,), device="cuda", generator=g, dtype=torch.int32)
    if name == "one_launch":
        rows, cols, n = 200_000, 150_000, 2_000_000
        r, c = ri(rows, n), ri(cols, n)
    elif name == "band_candidate":                               # x of 12 MiB (fp32) over 24 M nonzeros
        rows, cols, n = 1_000_000, 3_145_728, 24_000_000
        r, c = ri(rows, n), ri(cols, n)
    elif name == "giant_row":                                    # one row of 8.1 M entries among 1000: the long-rows form
        rows, cols, n = 1000, 500_000, 8_100_000 + 2000
        r = torch.cat([torch.full((8_100_000,), 500, dtype=torch.int32, device="cuda"), ri(rows, 2000)])
        c = ri(cols, n)
        sh = torch.randperm(n, device="cuda", generator=g)
        r, c = r[sh].contiguous(), c[sh].contiguous()
    else:
        raise KeyError(name)
    v = (torch.rand(n, device="cuda", generator=g, dtype=torch.float64) * 2 - 1).to(tdt)
    return rows, cols, r, c, v


@gpu
@pytest.mark.parametrize("name", ["one_launch", "band_candidate", "giant_row"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_coomv_bitwise_the_forward_call_and_within_the_oracle_bound(name, prec):
    tdt, vb = (torch.float32, 4) if prec == "f32" else (torch.float64, 8)
    rows, cols, r, c, v = _spmv_case(name, tdt)
    nnz = r.numel()
    info = M.launch_info(rows, nnz, vb, num_cols=cols)
    if name == "one_launch":
        assert info["snap_head_max"] > 0 and M.band_passes(rows, cols, nnz, vb) == 0, info
    elif name == "band_candidate":
        assert M.band_passes(rows, cols, nnz, vb) > 0, info
    else:
        assert info["snap_head_max"] == 0 and info["fixup_levels"] >= 1, info
    off, col, val, _ = _device_build(rows, r, c, v)
    g = torch.Generator(device="cuda"); g.manual_seed(2)
    x = (torch.rand(cols, device="cuda", generator=g, dtype=torch.float64) * 2 - 1).to(tdt)
    y0 = (torch.rand(rows, device="cuda", generator=g, dtype=torch.float64) * 2 - 1).to(tdt)
    # beta == 0 never reads y (NaN prefill)
    want = M.csrmv(val, off, col, x, num_cols=cols)
    got = M.coomv(v, r, c, x, torch.full((rows,), float("nan"), dtype=tdt, device="cuda"), num_cols=cols)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    csr = O.Csr(rows, cols, off.cpu().numpy(), col.cpu().numpy(), val.cpu().numpy())
    gold, s = O.spmv_gold_acc64(csr, x.cpu().numpy())
    ok, worst = O.strict_check(csr, got.cpu().numpy(), gold, s, items_per_thread=M.serial_sum_depth(rows, cols, nnz, vb))
    assert ok, (name, prec, worst)
    # alpha / beta general
    want = M.csrmv(val, off, col, x, y0.clone(), num_cols=cols, alpha=-0.5, beta=3.0)
    got = M.coomv(v, r, c, x, y0.clone(), num_cols=cols, alpha=-0.5, beta=3.0)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


@gpu
@pytest.mark.parametrize("name", ["general_dups_file_order", "empty", "one_by_one", "column_vector", "golden_12", "dims_65537_255"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_coomv_small_inputs(name, prec):
    dtype = np.float32 if prec == "f32" else np.float64
    rows, cols, r, c, v = _case(name, dtype)
    off, col, val, _ = host_build(rows, r, c, v)
    rng = np.random.default_rng(1)
    x, y0 = rng.uniform(-1, 1, cols).astype(dtype), rng.uniform(-1, 1, rows).astype(dtype)
    want = M.csrmv(_d(val), _d(off), _d(col), _d(x), _d(y0.copy()), num_cols=cols, alpha=1.5, beta=-2.0)
    got = M.coomv(_d(v), _d(r.astype(np.int32)), _d(c.astype(np.int32)), _d(x), _d(y0.copy()), num_cols=cols, alpha=1.5, beta=-2.0)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    csr = O.Csr(rows, cols, off, col, val)
    gold, s = O.spmv_gold_acc64(csr, x)
    got = M.coomv(_d(v), _d(r.astype(np.int32)), _d(c.astype(np.int32)), _d(x), num_rows=rows, num_cols=cols)
    ok, worst = O.strict_check(csr, got.cpu().numpy(), gold, s, items_per_thread=M.serial_sum_depth(rows, cols, len(r), v.itemsize))
    assert ok, (name, prec, worst)


@gpu
def test_coo_wrappers_reject_bad_tensors():
    r = torch.zeros(4, dtype=torch.int32, device="cuda")
    v = torch.zeros(4, dtype=torch.float32, device="cuda")
    with pytest.raises(M.MspmvError):
        M.coo_to_csr(v, r.to(torch.int64), r, 3, 3)
    with pytest.raises(M.MspmvError):
        M.coo_to_csr(v, r, r[:3], 3, 3)
    with pytest.raises(M.MspmvError):
        M.coo_to_csr(v.cpu(), r, r, 3, 3)
    with pytest.raises(TypeError):
        M.coo_to_csr(v.to(torch.float16), r, r, 3, 3)
    with pytest.raises(M.MspmvError):
        M.coomv(v, r, r, torch.zeros(2, dtype=torch.float32, device="cuda"), num_rows=3, num_cols=3)
    with pytest.raises(M.MspmvError):
        M.coo_to_csr(v, r, r, 0, 3)                              # nonzeros without rows: refused by the library


# ---------------------------------------------------------------------------------------------------------------- GPU: graph capture
@gpu
def test_build_and_multiply_replay_in_a_graph_on_new_triples():
    """the build reads nothing back on the host: captured once with csrmv, replayed after the triples were overwritten in place, it
    gives the new matrix's result every time"""
    rows, cols, nnz = 40_000, 30_000, 600_000
    rng = np.random.default_rng(9)

    def triples():
        r, c = _random_triples(rng, rows, cols, nnz)
        return r.astype(np.int32), c.astype(np.int32), rng.uniform(-1, 1, nnz).astype(np.float32)

    r0, c0, v0 = triples()
    dr, dc, dv = _d(r0), _d(c0), _d(v0)
    x = _d(rng.uniform(-1, 1, cols).astype(np.float32))
    y = torch.zeros(rows, dtype=torch.float32, device="cuda")
    b = M.CooToCsr(dv, dr, dc, rows, cols)                       # (allocates the outputs and the temp storage once)
    ws = M.CsrMVWorkspace(rows, nnz, torch.float32)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        b.rebuild(dv, dr, dc, stream=side)                       # warm-up outside the capture
        M.csrmv(b.values, b.row_offsets, b.column_indices, x, y, num_cols=cols, workspace=ws, stream=side)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            b.rebuild(dv, dr, dc, stream=side)
            M.csrmv(b.values, b.row_offsets, b.column_indices, x, y, num_cols=cols, workspace=ws, stream=side)
    torch.cuda.synchronize()
    for _ in range(3):
        r1, c1, v1 = triples()
        dr.copy_(_d(r1)); dc.copy_(_d(c1)); dv.copy_(_d(v1))
        y.fill_(float("nan"))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        off, col, val, _ = host_build(rows, r1, c1, v1)
        assert np.array_equal(b.row_offsets.cpu().numpy(), off) and np.array_equal(b.column_indices.cpu().numpy(), col)
        assert np.array_equal(b.values.cpu().numpy(), val)
        want = M.csrmv(_d(val), _d(off), _d(col), x, num_cols=cols)
        torch.cuda.synchronize()
        assert torch.equal(y, want)


# ---------------------------------------------------------------------------------------------------------------- GPU: the limit
@gpu
def test_coo_to_csr_at_the_item_limit():
    """rows + nnz = MAX_ITEMS, structure and permutation: closed-formula triples made on the device, exact integer reference
    (tests/coo_limit_worker.py, run once in a process of its own under a time limit; exit status 77 = not enough free device memory)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "coo_limit_worker.py")], capture_output=True, text=True, timeout=900)
    if r.returncode == 77:
        pytest.skip(r.stdout.strip().splitlines()[-1])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "coo limit OK" in r.stdout
