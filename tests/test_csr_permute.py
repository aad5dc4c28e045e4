"""B = A[row_perm, :] with the columns renumbered, canonical (include/mspmv.h: mspmv_csr_permute_*; merge_spmv_amd.csr_permute).
CPU: exports, the two-phase size query, refusals (nothing launched, no device), and the numpy model (tests/color_model.py: permute)
pinned to a hand-written 4 x 5 example.  GPU: B's three arrays and the permutation on the BIT PATTERNS against the model in fp32 and
fp64 (values hold -0.0, subnormals and NaNs with payloads: they are moved, never recomputed); the guard words around the outputs stay
untouched, the inputs stay unchanged.  Expected values never come from the library."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import merge_spmv_amd as M
from conftest import ROOT
import color_model as model

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

NEW = ["mspmv_csr_permute_f32", "mspmv_csr_permute_f64"]
MAX_ITEMS = 2 ** 31 - 1 - 65536
NP = {"f32": np.float32, "f64": np.float64}
BITS = {"f32": np.uint32, "f64": np.uint64}
PRECS = ["f32", "f64"]


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_csr_permute_symbols_are_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mspmv.h")).read(), flags=re.S)
    lib = M.load_library()
    for kind in ("product", "dev"):
        out = subprocess.run(["nm", "-D", "--defined-only", M.library_path(kind)], capture_output=True, text=True, check=True).stdout
        assert sorted(re.findall(r" T (mspmv_csr_permute_\w+)", out)) == sorted(NEW), kind
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    assert "csr_permute" in M.__all__ and lib.mspmv_version() == 102


def _raw_call(prec, temp, size, rows, cols, nnz, val=4096, off=4096, col=4096, row_perm=None, col_map=None, val_b=4096, off_b=4096,
              col_b=4096, perm=None):
    fn = getattr(M.load_library(), "mspmv_csr_permute_" + prec)
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    return fn(p(temp), size, p(val), p(off), p(col), rows, cols, nnz, p(row_perm), p(col_map), p(val_b), p(off_b), p(col_b), p(perm), None, 0)


@pytest.mark.parametrize("prec", PRECS)
def test_csr_permute_size_query_and_refusals(prec):
    """every refusal comes before anything is launched: this runs without a device"""
    size = ctypes.c_size_t(0)
    q = lambda rows, cols, nnz: _raw_call(prec, None, ctypes.byref(size), rows, cols, nnz)
    assert q(300, 300, 2000) == 0 and size.value > 0 and size.value % 16 == 0
    small = size.value
    assert q(300, 300, 200000) == 0 and size.value > small           # grows with the entries
    need = size.value
    assert q(0, 0, 0) == 0 and size.value > 0 and q(5, 0, 0) == 0 and q(0, 5, 0) == 0
    assert _raw_call(prec, None, None, 300, 300, 2000) == 1        # nowhere to put the size
    assert q(-1, 5, 0) == 1 and q(5, -1, 0) == 1 and q(5, 5, -1) == 1
    assert q(0, 5, 7) == 1 and q(5, 0, 7) == 1                     # entries without rows or columns
    assert q(MAX_ITEMS + 1, 5, 0) == 1 and q(1000, 5, MAX_ITEMS - 1000 + 1) == 1 and q(1000, 5, MAX_ITEMS - 1000) == 0
    # the second phase: too little temp, a misaligned temp, missing arrays, values on one side only
    size = ctypes.c_size_t(need)
    ok = dict(rows=300, cols=300, nnz=200000)
    assert _raw_call(prec, 4096, ctypes.byref(ctypes.c_size_t(need - 1)), **ok) == 1
    assert _raw_call(prec, 4096 + 8, ctypes.byref(size), **ok) == 1
    for missing in ("off", "col", "off_b", "col_b"):
        assert _raw_call(prec, 4096, ctypes.byref(size), **ok, **{missing: None}) == 1, missing
    assert _raw_call(prec, 4096, ctypes.byref(size), **ok, val=None) == 1 and _raw_call(prec, 4096, ctypes.byref(size), **ok, val_b=None) == 1
    assert _raw_call(prec, 4096, ctypes.byref(size), 5, 5, 0, off_b=None) == 1


def test_csr_permute_wrapper_rejects_bad_tensors_without_a_device():
    off, col, val = torch.zeros(4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), torch.zeros(2)
    for bad in (lambda: M.csr_permute(val, off, col, 3), lambda: M.csr_permute(None, None, col, 3), lambda: M.csr_permute(None, off, col.long(), 3),
                lambda: M.csr_permute(val, off, col, 3, row_perm=torch.zeros(3, dtype=torch.int32))):
        with pytest.raises(M.MspmvError):
            bad()


def test_the_model_on_a_hand_written_example():
    """4 x 5: row_perm = [2, 0, 3, 1] (B's row 0 is A's row 2, ...), columns 0 1 2 3 4 -> 4 0 0 2 1"""
    off = np.array([0, 2, 2, 5, 6], np.int32)
    col = np.array([3, 0, 4, 1, 4, 2], np.int32)
    val = np.array([10, 11, 12, 13, 14, 15], np.float32)
    off_b, col_b, val_b, perm = model.permute(off, col, val, 5, [2, 0, 3, 1], [4, 0, 0, 2, 1])
    # A's row 2 = (4, 12) (1, 13) (4, 14) -> (1, 12) (0, 13) (1, 14) -> sorted stably: (0, 13) (1, 12) (1, 14); row 0 -> (2, 10) (4, 11)
    assert off_b.tolist() == [0, 3, 5, 6, 6] and col_b.tolist() == [0, 1, 1, 2, 4, 0]
    assert val_b.tolist() == [13, 12, 14, 10, 11, 15] and perm.tolist() == [3, 2, 4, 0, 1, 5]
    # both NULL: every row sorted stably by column
    off_b, col_b, val_b, perm = model.permute(off, col, val, 5)
    assert off_b.tolist() == off.tolist() and col_b.tolist() == [0, 3, 1, 4, 4, 2] and perm.tolist() == [1, 0, 3, 2, 4, 5]
    # structure only; no entries
    assert model.permute(off, col, None, 5, [2, 0, 3, 1])[2] is None
    assert model.permute(np.zeros(4, np.int32), np.zeros(0, np.int32), None, 5, [2, 0, 1])[0].tolist() == [0, 0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------- GPU
GUARD = 8
SENTINEL = -77


def _device(a):
    return torch.from_numpy(np.array(a)).cuda()


def _guarded(n, tdt, shift_elems):
    """n entries between guard words; the first entry sits shift_elems elements behind a 16-byte boundary + the guard"""
    buf = torch.full((GUARD + shift_elems + n + GUARD,), SENTINEL, dtype=tdt, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf[GUARD + shift_elems: GUARD + shift_elems + n]


def _guards_intact(buf, view):
    lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    return bool((buf[:lo] == SENTINEL).all()) and bool((buf[lo + view.numel():] == SENTINEL).all())


def _special(val, rng, prec):
    """-0.0, subnormals, and NaNs with payloads among the values"""
    bits = val.view(BITS[prec]).copy()
    n = len(bits)
    if n >= 8:
        where = rng.choice(n, 8, replace=False)
        top = 31 if prec == "f32" else 63
        quiet = (0x7fc00000 if prec == "f32" else 0x7ff8000000000000)
        signalling = (0x7f800000 if prec == "f32" else 0x7ff0000000000000)
        bits[where[0]] = 1 << top                                  # -0.0
        bits[where[1]] = 1                                         # the smallest subnormal
        bits[where[2]] = (1 << top) | 0x1234                       # a negative subnormal
        bits[where[3]] = quiet | 0x2a                              # a quiet NaN with a payload
        bits[where[4]] = (1 << top) | quiet | 0x155
        bits[where[5]] = signalling | 0x77                         # a signalling NaN: it must come out as it went in
        bits[where[6]] = 0
        bits[where[7]] = signalling                                # inf
    return bits.view(NP[prec])


class Run:
    """one call through the C ABI on guarded, possibly misaligned outputs: B and the permutation against the model on the bits, the
    guards intact, the inputs unchanged"""

    def __init__(self, prec, off, col, val, cols, row_perm=None, col_map=None, shift=0, want_perm=True, structure_only=False):
        self.prec, self.rows, self.cols, self.nnz = prec, len(off) - 1, cols, len(col)
        tdt = torch.float32 if prec == "f32" else torch.float64
        self.host = (off, col, val, row_perm, col_map)
        self.d_off, self.d_col = _device(off), _device(col)
        self.d_val = None if structure_only else _device(val)
        self.d_rp = None if row_perm is None else _device(np.asarray(row_perm, np.int32))
        self.d_cm = None if col_map is None else _device(np.asarray(col_map, np.int32))
        k = shift // 4
        self.obuf, self.off_b = _guarded(self.rows + 1, torch.int32, k)
        self.cbuf, self.col_b = _guarded(self.nnz, torch.int32, k)
        self.pbuf, self.perm = _guarded(self.nnz, torch.int32, k) if want_perm else (None, None)
        self.vbuf, self.val_b = (None, None) if structure_only else _guarded(self.nnz, tdt, max(k * 4 // self.d_val.element_size(), 1 if shift else 0))
        if shift:
            assert self.off_b.data_ptr() % 16 == shift and (self.nnz == 0 or self.col_b.data_ptr() % 16 == shift)
        self.fn = getattr(M.load_library(), "mspmv_csr_permute_" + prec)
        self.args = (M._ptr(self.d_val), M._ptr(self.d_off), M._ptr(self.d_col), self.rows, self.cols, self.nnz, M._ptr(self.d_rp), M._ptr(self.d_cm),
                     M._ptr(self.val_b), ctypes.c_void_p(self.off_b.data_ptr()), M._ptr(self.col_b), M._ptr(self.perm))
        size = ctypes.c_size_t(0)
        assert self.fn(None, ctypes.byref(size), *self.args, None, 0) == 0
        self.size = size.value
        self.temp = torch.empty(self.size, dtype=torch.uint8, device="cuda")
        assert self.temp.data_ptr() % 16 == 0
        self.want = model.permute(off, col, None if structure_only else val, cols, row_perm, col_map)

    def call(self, debug=0):
        size = ctypes.c_size_t(self.size)
        assert self.fn(ctypes.c_void_p(self.temp.data_ptr()), ctypes.byref(size), *self.args, M._stream_handle(None), debug) == 0
        return self

    def check(self):
        torch.cuda.synchronize()
        off_b, col_b, val_b, perm = self.want
        assert torch.equal(self.off_b.cpu(), torch.from_numpy(off_b)) and torch.equal(self.col_b.cpu(), torch.from_numpy(col_b))
        assert _guards_intact(self.obuf, self.off_b) and _guards_intact(self.cbuf, self.col_b)
        if self.perm is not None:
            assert torch.equal(self.perm.cpu(), torch.from_numpy(perm)) and _guards_intact(self.pbuf, self.perm)
        if self.val_b is not None:
            bits = BITS[self.prec]
            assert np.array_equal(self.val_b.cpu().numpy().view(bits), val_b.view(bits)) and _guards_intact(self.vbuf, self.val_b)
        off, col, val, row_perm, col_map = self.host
        assert np.array_equal(self.d_off.cpu().numpy(), off) and np.array_equal(self.d_col.cpu().numpy(), col)
        if self.d_val is not None:
            assert np.array_equal(self.d_val.cpu().numpy().view(BITS[self.prec]), val.view(BITS[self.prec]))
        if self.d_rp is not None:
            assert np.array_equal(self.d_rp.cpu().numpy(), row_perm)
        if self.d_cm is not None:
            assert np.array_equal(self.d_cm.cpu().numpy(), col_map)
        return self


def _random_csr(rows, cols, rng, prec, canonical=False, max_len=12):
    """unsorted rows with duplicates and empty rows (canonical: sorted, no duplicates)"""
    rowlists = []
    for r in range(rows):
        n = 0 if rng.random() < 0.15 else int(rng.integers(1, max_len + 1))
        cs = [int(c) for c in rng.integers(0, cols, n)]
        if canonical:
            cs = sorted(set(cs))
        elif n > 2:
            cs += cs[:2]
        rowlists.append(cs)
    off = np.zeros(rows + 1, np.int32)
    np.cumsum([len(r) for r in rowlists], out=off[1:])
    col = np.asarray([c for r in rowlists for c in r], np.int32)
    val = _special(rng.uniform(-1, 1, len(col)).astype(NP[prec]), rng, prec)
    return off, col, val


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_random_permutations_of_a_messy_square_matrix(prec):
    rng = np.random.default_rng(31)
    off, col, val = _random_csr(300, 300, rng, prec)
    order = rng.permutation(300).astype(np.int32)
    inverse = np.empty(300, np.int32); inverse[order] = np.arange(300, dtype=np.int32)
    Run(prec, off, col, val, 300, order, inverse).call().check()                     # P A P^T
    Run(prec, off, col, val, 300, order, rng.permutation(300).astype(np.int32)).call().check()
    r = Run(prec, off, col, val, 300, order, inverse, shift=4).call().check()        # outputs off the 16-byte boundary
    assert r.off_b.data_ptr() % 16 == 4
    Run(prec, off, col, val, 300, order, inverse, want_perm=False).call().check()    # no permutation asked for


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_rectangular_and_the_identities(prec):
    rng = np.random.default_rng(37)
    off, col, val = _random_csr(200, 333, rng, prec, canonical=True)
    Run(prec, off, col, val, 333, None, rng.permutation(333).astype(np.int32)).call().check()
    Run(prec, off, col, val, 333, rng.permutation(200).astype(np.int32), None).call().check()
    r = Run(prec, off, col, val, 333).call().check()
    # a canonical input comes out as it went in, the permutation is the identity
    assert np.array_equal(r.off_b.cpu().numpy(), off) and np.array_equal(r.col_b.cpu().numpy(), col)
    assert np.array_equal(r.val_b.cpu().numpy().view(BITS[prec]), val.view(BITS[prec])) and np.array_equal(r.perm.cpu().numpy(), np.arange(len(col)))


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_columns_sent_to_one_column_keep_their_stored_order(prec):
    rng = np.random.default_rng(41)
    off, col, val = _random_csr(120, 50, rng, prec, max_len=30)
    col_map = (np.arange(50) // 7).astype(np.int32)                                 # seven columns to one, again and again
    r = Run(prec, off, col, val, 50, rng.permutation(120).astype(np.int32), col_map).call().check()
    # independently of the model: inside a run of equal new columns the positions in A ascend
    off_b, col_b, perm = (t.cpu().numpy() for t in (r.off_b, r.col_b, r.perm))
    for i in range(120):
        seg = slice(off_b[i], off_b[i + 1])
        assert np.all(np.diff(col_b[seg]) >= 0) and np.all(np.diff(perm[seg])[np.diff(col_b[seg]) == 0] > 0)


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_one_long_row_among_empty_rows(prec):
    rng = np.random.default_rng(43)
    rows, cols = 2001, 7000
    off = np.zeros(rows + 1, np.int32); off[1235:] = 5000                             # row 1234 holds everything
    col = rng.integers(0, cols, 5000).astype(np.int32)
    val = _special(rng.uniform(-1, 1, 5000).astype(NP[prec]), rng, prec)
    Run(prec, off, col, val, cols, rng.permutation(rows).astype(np.int32), rng.permutation(cols).astype(np.int32)).call().check()


@gpu
def test_structure_only_and_no_entries():
    rng = np.random.default_rng(47)
    off, col, val = _random_csr(300, 300, rng, "f32")
    order = rng.permutation(300).astype(np.int32)
    for prec in PRECS:
        Run(prec, off, col, None, 300, order, order, structure_only=True).call().check()
        for rows, cols in ((5, 7), (0, 0), (1, 1)):
            r = Run(prec, np.zeros(rows + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, NP[prec]), cols,
                    rng.permutation(rows).astype(np.int32), None).call().check()
            assert r.off_b.cpu().tolist() == [0] * (rows + 1)


@gpu
def test_a_captured_call_replays_to_the_eager_result():
    rng = np.random.default_rng(53)
    off, col, val = _random_csr(300, 300, rng, "f64")
    order = rng.permutation(300).astype(np.int32)
    r = Run("f64", off, col, val, 300, order, order).call().check()                  # (warm-up outside the capture, and the eager result)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r.call()
    for _ in range(2):
        for t in (r.off_b, r.col_b, r.perm):
            t.fill_(-5)
        r.val_b.fill_(float("nan"))
        graph.replay()
        r.check()


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_new_values_through_the_returned_permutation_and_the_wrapper(prec):
    rng = np.random.default_rng(59)
    off, col, val = _random_csr(300, 300, rng, prec)
    order = rng.permutation(300).astype(np.int32)
    d_off, d_col, d_val, d_order = _device(off), _device(col), _device(val), _device(order)
    csr, perm = M.csr_permute(d_val, d_off, d_col, 300, row_perm=d_order, col_map=d_order, return_permutation=True)
    want = model.permute(off, col, val, 300, order, order)
    assert torch.equal(csr.row_offsets.cpu(), torch.from_numpy(want[0])) and torch.equal(csr.column_indices.cpu(), torch.from_numpy(want[1]))
    assert np.array_equal(csr.values.cpu().numpy().view(BITS[prec]), want[2].view(BITS[prec])) and torch.equal(perm.cpu(), torch.from_numpy(want[3]))
    assert (csr.rows, csr.cols) == (300, 300)
    new = _special(rng.uniform(-1, 1, len(col)).astype(NP[prec]), rng, prec)
    d_new, out = _device(new), torch.empty_like(d_val)
    fn = getattr(M.load_library(), "mspmv_coo_to_csr_values_" + prec)
    assert fn(M._ptr(d_new), M._ptr(perm), M._ptr(out), len(col), M._stream_handle(None), 0) == 0
    fresh = M.csr_permute(d_new, d_off, d_col, 300, row_perm=d_order, col_map=d_order)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(BITS[prec]), fresh.values.cpu().numpy().view(BITS[prec]))
    assert np.array_equal(out.cpu().numpy().view(BITS[prec]), new[want[3]].view(BITS[prec]))
    structure = M.csr_permute(None, d_off, d_col, 300, row_perm=d_order)
    assert structure.values is None and torch.equal(structure.row_offsets.cpu(), torch.from_numpy(model.permute(off, col, None, 300, order)[0]))
