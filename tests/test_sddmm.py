"""SDDMM on the device (include/mspmv.h: mspmv_sddmm_f32 / _f64 / _bf16_f32; merge_spmv_amd.sddmm): for every stored entry of a CSR
pattern C[e] = alpha * (U[r, :] . V[c, :]) + beta * C[e], the dot product added left to right, every operation rounded on its own.
CPU: exports, argument conventions (no kernel launched), and the numpy model (tests/sddmm_model.py) pinned to exact rational
arithmetic rounded per operation.  GPU: every comparison is torch.equal on the BIT PATTERNS against the model; the guard words
around C stay untouched and U, V and the pattern stay unchanged.  Expected values never come from the library."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import merge_spmv_amd as M
from conftest import ROOT
from sddmm_model import entry_rows, narrow_bf16, sddmm_model, widen_bf16

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

NEW = ["mspmv_sddmm_f32", "mspmv_sddmm_f64", "mspmv_sddmm_bf16_f32"]
MAX_ITEMS = 2 ** 31 - 1 - 65536
T = 512                                                          # entries per tile of sddmm_kernel (SDDMM_TILE)
CHUNK = {"f32": 32, "f64": 16, "bf16": 64}                       # elements of k per 128-byte chunk of the 16-byte path
KS = sorted({0, 1, 2, 3, 4, 5, 8, 15, 16, 17, 33, 64, 129} | {c + d for c in CHUNK.values() for d in (-1, 0, 1)})
NP = {"f32": np.float32, "f64": np.float64, "bf16": np.uint16}


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_sddmm_symbols_are_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mspmv.h")).read(), flags=re.S)
    lib = M.load_library()
    for kind in ("product", "dev"):
        out = subprocess.run(["nm", "-D", "--defined-only", M.library_path(kind)], capture_output=True, text=True, check=True).stdout
        for name in NEW:
            assert f" T {name}\n" in out + "\n", (kind, name)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None and getattr(lib, name).restype is ctypes.c_int, name
    assert "sddmm" in M.__all__ and callable(M.sddmm)
    assert lib.mspmv_version() == 102


@pytest.mark.parametrize("prec", ["f32", "f64", "bf16_f32"])
def test_sddmm_argument_conventions(prec):
    """every refusal comes before anything is launched: this runs without a device"""
    fn = getattr(M.load_library(), "mspmv_sddmm_" + prec)
    f = ctypes.c_void_p(4096)

    def call(rows, cols, nnz, k, ldu=None, ldv=None, off=f, col=f, u=f, v=f, c=f):
        return fn(off, col, u, k if ldu is None else ldu, v, k if ldv is None else ldv, c, rows, cols, nnz, k, 1.0, 0.0, None, 0)

    # a negative size in each position
    assert call(-1, 5, 0, 4) == 1 and call(5, -1, 0, 4) == 1 and call(5, 5, -1, 4) == 1 and call(5, 5, 0, -1) == 1
    assert call(5, 5, 0, 4, ldu=-1) == 1 and call(5, 5, 0, 4, ldv=-1) == 1
    # ld < k, for either operand, with and without entries
    for nnz in (0, 7):
        assert call(5, 5, nnz, 4, ldu=3) == 1 and call(5, 5, nnz, 4, ldv=3) == 1
    # rows + nnz: 0 at the limit (no entries: nothing is launched), 1 one past it, however the sum is split
    assert call(MAX_ITEMS, 5, 0, 4) == 0
    assert call(MAX_ITEMS + 1, 5, 0, 4) == 1
    assert call(1000, 5, MAX_ITEMS - 1000 + 1, 4) == 1
    assert call(1, 5, MAX_ITEMS, 4) == 1
    assert call(2 ** 31 - 1, 5, 2 ** 31 - 1, 4) == 1
    assert call(0, 2 ** 31 - 1, 0, 2 ** 31 - 1) == 0             # (columns and k do not count)
    # entries together with a zero dimension
    assert call(0, 5, 7, 4) == 1 and call(5, 0, 7, 4) == 1 and call(0, 0, 7, 4) == 1
    # NULL arrays with nnz > 0, each in turn
    for name in ("off", "col", "u", "v", "c"):
        assert call(5, 5, 7, 4, **{name: None}) == 1, name
    for name in ("off", "col", "c"):
        assert call(5, 5, 7, 0, **{name: None}) == 1, name       # (k == 0: U and V have no entries and no say, the others do)
    # nnz == 0 succeeds with NULL arrays and launches nothing
    none = dict(off=None, col=None, u=None, v=None, c=None)
    assert call(5, 5, 0, 4, **none) == 0 and call(0, 0, 0, 0, **none) == 0 and call(0, 5, 0, 4, **none) == 0 and call(5, 0, 0, 4, ldu=9, **none) == 0


def test_sddmm_wrapper_rejects_bad_tensors_without_a_device():
    off, col = torch.zeros(4, dtype=torch.int32), torch.zeros(0, dtype=torch.int32)
    U = torch.zeros(3, 4)
    with pytest.raises(M.MspmvError):
        M.sddmm(off, col, U, U)                                  # not on the device
    with pytest.raises(M.MspmvError):
        M.sddmm(off, col, None, U)


# ---- exact rational arithmetic, rounded per operation to the nearest, ties to even (subnormals included)
def _round(fr, dtype):
    p, emin = (24, -126) if dtype == np.float32 else (53, -1022)
    a = abs(fr)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1)
    quantum = Fraction(2) ** (max(e, emin) - (p - 1))
    n = round(a / quantum)                                       # (Fraction.__round__: ties to even)
    v = float(n * quantum)                                       # (exact: at most 53 bits)
    return dtype(-v if fr < 0 else v)


def _mul(a, b, dtype):
    fr = Fraction(float(a)) * Fraction(float(b))
    if fr == 0:
        return dtype(-0.0) if bool(np.signbit(a)) != bool(np.signbit(b)) else dtype(0.0)
    return _round(fr, dtype)


def _add(a, b, dtype):
    fr = Fraction(float(a)) + Fraction(float(b))
    if fr == 0:
        return dtype(-0.0) if (np.signbit(a) and np.signbit(b)) else dtype(0.0)
    return _round(fr, dtype)


def _exact(off, col, U, V, alpha, beta, C, dtype):
    rows = entry_rows(off, len(col))
    out = np.empty(len(col), dtype)
    for e, (r, c) in enumerate(zip(rows, col)):
        s = dtype(0.0)
        for t in range(U.shape[1]):
            s = _add(s, _mul(U[r, t], V[c, t], dtype), dtype)
        b = dtype(0.0) if dtype(beta) == 0 else _mul(dtype(beta), C[e], dtype)
        out[e] = _add(_mul(dtype(alpha), s, dtype), b, dtype)
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_model_on_hand_written_cases(dtype):
    i = lambda x: np.asarray(x, np.int32)
    f = lambda x: np.asarray(x, dtype)
    nan = float("nan")
    # 1. [[1, 2], [3, 4]] sampled against V = [[5, 6], [7, 8], [9, 10]] at (0,0) (0,2) (1,1): 17, 29, 53
    off, col = i([0, 2, 3]), i([0, 2, 1])
    U, V = f([[1, 2], [3, 4]]), f([[5, 6], [7, 8], [9, 10]])
    assert sddmm_model(off, col, U, V).tolist() == [17.0, 29.0, 53.0]
    assert sddmm_model(off, col, U, V, 2.0, -1.0, f([1, 2, 3])).tolist() == [33.0, 56.0, 103.0]
    # 2. beta == 0 never reads C: a NaN there does not come through; beta != 0 does read it
    assert sddmm_model(off, col, U, V, 1.0, 0.0, f([nan, nan, nan])).tolist() == [17.0, 29.0, 53.0]
    assert np.isnan(sddmm_model(off, col, U, V, 1.0, 1.0, f([nan, 0, 0]))[0])
    # 3. a row whose products are all -0.0: s stays +0.0; with a negative alpha alpha * s is -0.0 and the + (+0.0) makes it +0.0;
    #    with beta != 0 and an old C of -0.0 the sum of two -0.0 is -0.0
    U, V = f([[-1.0, -2.0, -0.0]]), f([[0.0, 0.0, 3.0]])
    off, col = i([0, 1]), i([0])
    for alpha in (1.0, -2.0):
        got = sddmm_model(off, col, U, V, alpha, 0.0, f([nan]))
        assert got.tolist() == [0.0] and not np.signbit(got[0])
    got = sddmm_model(off, col, U, V, -2.0, 1.0, f([-0.0]))
    assert got.tolist() == [0.0] and np.signbit(got[0])
    # 4. k == 0: alpha * (+0.0) + the beta term; an empty row in front, a repeated column
    off, col = i([0, 0, 2]), i([1, 1])
    U, V = np.zeros((2, 0), dtype), np.zeros((3, 0), dtype)
    got = sddmm_model(off, col, U, V, -3.0, 0.0, f([nan, nan]))
    assert got.tolist() == [0.0, 0.0] and not np.signbit(got).any()
    assert sddmm_model(off, col, U, V, -3.0, 0.5, f([4.0, -6.0])).tolist() == [2.0, -3.0]
    # 5. the order of the adds: (big + 1) - big = 0 left to right
    big = 2.0 ** (24 if dtype == np.float32 else 53)
    off, col = i([0, 1]), i([0])
    assert sddmm_model(off, col, f([[big, 1.0, -big]]), f([[1.0, 1.0, 1.0]])).tolist() == [0.0]
    assert sddmm_model(off, col, f([[big, -big, 1.0]]), f([[1.0, 1.0, 1.0]])).tolist() == [1.0]
    # 6. every product rounded before it is added: (-1 * 1) + (3 * fl(1/3)) = 0, where a fused multiply-add keeps fl(1/3)'s error
    third = dtype(1.0) / dtype(3.0)
    assert sddmm_model(off, col, f([[-1.0, 3.0]]), f([[1.0, third]])).tolist() == [0.0]
    assert float(Fraction(3) * Fraction(float(third)) - 1) != 0.0
    # 7. against exact rational arithmetic rounded per operation: random values, subnormal products, zeros of both signs
    rng = np.random.default_rng(5)
    tiny = float(np.finfo(dtype).tiny)
    for scale in (1.0, tiny ** 0.5 / 4):
        rows, cols, k = 5, 4, 7
        lens = [0, 3, 0, 4, 2]
        off = np.zeros(rows + 1, np.int32); np.cumsum(lens, out=off[1:])
        col = rng.integers(0, cols, int(off[-1])).astype(np.int32)
        U = (rng.uniform(-1, 1, (rows, k)) * scale).astype(dtype)
        V = (rng.uniform(-1, 1, (cols, k)) * scale).astype(dtype)
        U[1, 2], U[3, 0], V[1, 4], V[2] = 0.0, -0.0, -0.0, 0.0
        C = rng.uniform(-1, 1, col.size).astype(dtype) * dtype(scale * scale)
        for alpha, beta in ((1.0, 0.0), (-2.0, 0.0), (0.5, -1.5), (0.0, 1.0), (-1.0, 1.0)):
            got, want = sddmm_model(off, col, U, V, alpha, beta, C), _exact(off, col, U, V, alpha, beta, C, dtype)
            assert np.array_equal(_bits(got), _bits(want)), (scale, alpha, beta)
        if scale != 1.0:
            s = np.abs(sddmm_model(off, col, U, V))
            assert ((s > 0) & (s < tiny)).any()                  # (the draw does reach the subnormals)


def test_the_model_widens_bf16_exactly():
    h = np.array([0x3F80, 0xBF80, 0x0000, 0x8000, 0x0001, 0x7F7F, 0x4049], np.uint16)
    w = widen_bf16(h)
    assert w.dtype == np.float32 and w[:4].tolist() == [1.0, -1.0, 0.0, 0.0] and np.signbit(w[3]) and w[4] == np.float32(2.0 ** -133)
    assert np.array_equal(narrow_bf16(w), h)
    off, col = np.array([0, 2], np.int32), np.array([1, 0], np.int32)
    U, V = h[[0, 6]].reshape(1, 2), h[[1, 0, 6, 6]].reshape(2, 2)
    got = sddmm_model(off, col, U, V)
    assert got.dtype == np.float32 and np.array_equal(got, sddmm_model(off, col, widen_bf16(U).reshape(1, 2), widen_bf16(V).reshape(2, 2)))


# ---------------------------------------------------------------------------------------------------------------- GPU
GUARD = 8
TORCH = {"f32": (torch.float32, torch.float32), "f64": (torch.float64, torch.float64), "bf16": (torch.bfloat16, torch.float32)}


def _pattern(lens, cols, rng, col=None):
    off = np.zeros(len(lens) + 1, np.int32); np.cumsum(lens, out=off[1:])
    if col is None:
        col = rng.integers(0, cols, int(off[-1]))
    return off, np.asarray(col, np.int32)


def _short_rows(nnz, rng):
    """rows of 0-3 entries holding nnz entries in all"""
    lens = []
    while sum(lens) < nnz:
        lens.append(int(rng.integers(0, 4)))
    lens[-1] -= sum(lens) - nnz
    return lens


def _draw(rng, shape, prec, scale=1.0):
    a = (rng.uniform(-1, 1, shape) * scale).astype(np.float32 if prec == "bf16" else NP[prec])
    return narrow_bf16(a).reshape(shape) if prec == "bf16" else a


def _strided(a, ld, shift, tdt):
    """a host matrix as a device tensor with leading dimension ld whose first element sits `shift` elements behind a 16-byte
    boundary; the gaps between the rows hold NaN (bf16: 0x7FC0)"""
    rows, k = a.shape
    n = shift + max(rows - 1, 0) * ld + k
    host = np.full(n, 0x7FC0 if a.dtype == np.uint16 else np.nan, a.dtype)
    for r in range(rows):
        host[shift + r * ld: shift + r * ld + k] = a[r]
    buf = torch.from_numpy(host.view(np.int16) if a.dtype == np.uint16 else host).cuda()
    if a.dtype == np.uint16:
        buf = buf.view(torch.bfloat16)
    assert buf.data_ptr() % 16 == 0
    return buf, torch.as_strided(buf, (rows, k), (ld, 1), shift)


def _aligned_ld(k, prec):
    epw = 16 // np.dtype(NP[prec]).itemsize
    return max(-(-k // epw) * epw, epw)


def _raw(t):
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def run(prec, off, col, U, V, alpha=1.0, beta=0.0, C=None, ldu=None, ldv=None, shift_u=0, shift_v=0, shift_c=0, shift_col=0, same=False,
        path=None):
    """One call of M.sddmm on guarded, possibly misaligned arrays, compared bit for bit with the model.  path: "wide" (16-byte
    aligned bases, leading dimensions rounded up to whole words) or "element" (bases one element off); None: as the arguments say."""
    in_dt, out_dt = TORCH[prec]
    out_np = np.float32 if prec == "bf16" else NP[prec]
    k = U.shape[1]
    if path == "wide":
        ldu, ldv = _aligned_ld(k, prec), _aligned_ld(k, prec)
    elif path == "element":
        ldu, ldv, shift_u, shift_v = k + 1, k + 3, 1, 1
    ldu, ldv = k if ldu is None else ldu, k if ldv is None else ldv
    nnz = col.size
    old = np.full(nnz, np.nan, out_np) if C is None else np.asarray(C, out_np)
    want = sddmm_model(off, col, U, V, alpha, beta, old)
    ubuf, dU = _strided(U, ldu, shift_u, in_dt)
    vbuf, dV = (ubuf, dU) if same else _strided(V, ldv, shift_v, in_dt)
    d_off = torch.from_numpy(off).cuda()
    colbuf = torch.zeros(shift_col + nnz, dtype=torch.int32, device="cuda")
    d_col = colbuf[shift_col:]
    d_col.copy_(torch.from_numpy(col))
    sentinel = 12345.0
    cbuf = torch.full((GUARD + shift_c + nnz + GUARD,), sentinel, dtype=out_dt, device="cuda")
    d_c = cbuf[GUARD + shift_c: GUARD + shift_c + nnz]
    d_c.copy_(torch.from_numpy(old))
    assert d_col.data_ptr() % 16 == 4 * (shift_col % 4) and (k == 0 or dU.data_ptr() % 16 == (shift_u * dU.element_size()) % 16)
    keep = [_raw(t).clone() for t in (ubuf, vbuf, d_off, colbuf)]
    got = M.sddmm(d_off, d_col, dU, dV, out=d_c, alpha=alpha, beta=beta)
    torch.cuda.synchronize()
    assert got is d_c
    assert torch.equal(_raw(d_c).cpu(), torch.from_numpy(_bits(want))), (prec, k, alpha, beta)
    assert bool((cbuf[:GUARD + shift_c] == sentinel).all()) and bool((cbuf[GUARD + shift_c + nnz:] == sentinel).all()), "guard words written"
    for t, was in zip((ubuf, vbuf, d_off, colbuf), keep):
        assert torch.equal(_raw(t), was), "an input was modified"
    return d_c


def _structure_cases():
    rng = np.random.default_rng(11)
    cases = {}
    for nnz in (1, T - 1, T, T + 1, 2 * T + 5):
        cases[f"short_rows_{nnz}"] = (_short_rows(nnz, rng), 37)
    cases["one_long_row"] = ([0, 0, 3 * T + 7, 0, 0, 0], 37)
    cases["boundary_at_row_start"] = ([T - 3, 3, 5, T - 5, 7], 37)                      # tiles 1 and 2 start with a row's first entry
    cases["boundary_at_row_end"] = ([T - 4, 5, T - 3, 3, 4], 37)                        # ... with a row's last entry
    cases["empty_rows_inside_a_tile"] = ([0, 0, 0, 2] + [0] * (T + 1) + [3, 0, 0, 0, 0], 37)      # the search in global memory
    cases["slice_of_T_rows"] = ([1] + [0] * (T - 2) + [1], 37)                         # the longest slice that is staged
    cases["slice_of_T_plus_1_rows"] = ([1] + [0] * (T - 1) + [1, 0], 37)               # the shortest that is not
    cases["empty_rows_across_tiles"] = ([T - 1] + [0] * (2 * T) + [T + 2] + [0] * 3, 37)
    cases["one_row"] = ([T + 9], 37)
    cases["one_column"] = (_short_rows(T + 40, rng), 1)
    cases["unsorted_repeated_columns"] = ([int(x) for x in rng.integers(0, 10, 150)], 5)
    return cases


STRUCTURE = _structure_cases()


@gpu
@pytest.mark.parametrize("path", ["wide", "element"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("case", sorted(STRUCTURE))
def test_structure(case, prec, path):
    lens, cols = STRUCTURE[case]
    rng = np.random.default_rng(len(lens))
    off, col = _pattern(lens, cols, rng)
    k = CHUNK[prec] + 5                                          # one whole chunk, one whole word behind it and a ragged one
    U, V = _draw(rng, (len(lens), k), prec), _draw(rng, (cols, k), prec)
    C = rng.uniform(-1, 1, col.size)
    run(prec, off, col, U, V, 0.5, -1.5, C, path=path)


@gpu
@pytest.mark.parametrize("path", ["wide", "element"])
@pytest.mark.parametrize("prec", ["f32", "f64", "bf16"])
@pytest.mark.parametrize("k", KS)
def test_every_k(k, prec, path):
    rng = np.random.default_rng(1000 + k)
    lens = _short_rows(T + 70, rng)
    off, col = _pattern(lens, 29, rng)
    U, V = _draw(rng, (len(lens), k), prec), _draw(rng, (29, k), prec)
    run(prec, off, col, U, V, -2.0, 0.0, path=path)              # (beta == 0 over a NaN-filled C)
    run(prec, off, col, U, V, 0.5, -1.5, rng.uniform(-1, 1, col.size), path=path)


@gpu
@pytest.mark.parametrize("prec", ["f32", "f64", "bf16"])
def test_layout(prec):
    rng = np.random.default_rng(3)
    lens = _short_rows(T + 70, rng)
    rows, cols = len(lens), 41
    off, col = _pattern(lens, cols, rng)
    for k in (8, CHUNK[prec] + 1):
        U, V = _draw(rng, (rows, k), prec), _draw(rng, (cols, k), prec)
        C = rng.uniform(-1, 1, col.size)
        for ld in (k, k + 1, k + 4):
            run(prec, off, col, U, V, 0.5, -1.5, C, ldu=ld, ldv=ld)
            run(prec, off, col, U, V, 0.5, -1.5, C, ldu=ld, ldv=_aligned_ld(k, prec))
        ld = _aligned_ld(k, prec)
        for shift in ("shift_u", "shift_v", "shift_c", "shift_col"):                   # each one element off a 16-byte boundary
            run(prec, off, col, U, V, 0.5, -1.5, C, ldu=ld, ldv=ld, **{shift: 1})
        run(prec, off, col, U, V, 0.5, -1.5, C, ldu=ld, ldv=ld, shift_u=1, shift_v=1, shift_c=1, shift_col=1)
    # U and V the same tensor (edge scores: a square pattern)
    n, k = 57, CHUNK[prec] + 3
    off, col = _pattern([int(x) for x in rng.integers(0, 30, n)], n, rng)
    H = _draw(rng, (n, k), prec)
    for path in ("wide", "element"):
        run(prec, off, col, H, H, 1.0, 0.0, same=True, path=path)


@gpu
@pytest.mark.parametrize("prec", ["f32", "f64", "bf16"])
@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (-2.0, 0.0), (0.5, -1.5), (0.0, 1.0), (-1.0, 1.0)])
def test_scalars(alpha, beta, prec):
    rng = np.random.default_rng(17)
    out_np = np.float32 if prec == "bf16" else NP[prec]
    lens = _short_rows(T + 70, rng)
    rows, cols, k = len(lens), 23, CHUNK[prec] + 6
    off, col = _pattern(lens, cols, rng)
    # plain draw; beta == 0 runs over a NaN-filled C (run's default), otherwise over a drawn one
    U, V = _draw(rng, (rows, k), prec), _draw(rng, (cols, k), prec)
    C = None if beta == 0 else rng.uniform(-1, 1, col.size)
    for path in ("wide", "element"):
        run(prec, off, col, U, V, alpha, beta, C, path=path)
    # zero-laden: zeros of both signs in U, V and the old C, and rows of U that are all -0.0 or all negative against all-zero
    # rows of V, so that every product of such an entry is -0.0
    neg_zero = narrow_bf16(np.float32(-0.0)) if prec == "bf16" else NP[prec](-0.0)
    Uz, Vz = U.copy(), V.copy()
    Uz[rng.random(Uz.shape) < 0.3] = 0
    Uz[rng.random(Uz.shape) < 0.2] = neg_zero
    Vz[rng.random(Vz.shape) < 0.3] = 0
    Vz[rng.random(Vz.shape) < 0.2] = neg_zero
    Uz[::5] = neg_zero
    if prec == "bf16":
        Uz[1::5] = U[1::5] | np.uint16(0x8000)
    else:
        Uz[1::5] = -np.abs(U[1::5]) - 1
    Vz[::2] = 0
    Cz = rng.uniform(-1, 1, col.size).astype(out_np)
    Cz[::3], Cz[1::3] = 0.0, -0.0
    want = sddmm_model(off, col, Uz, Vz, alpha, beta, Cz)
    assert (want == 0).sum() > col.size // 4
    for path in ("wide", "element"):
        run(prec, off, col, Uz, Vz, alpha, beta, None if beta == 0 else Cz, path=path)
    # products and sums in the subnormals: nothing is flushed
    tiny = float(np.finfo(np.float32 if prec == "bf16" else NP[prec]).tiny)
    scale = tiny ** 0.5 / 4
    Us, Vs = _draw(rng, (rows, k), prec, scale), _draw(rng, (cols, k), prec, scale)
    Cs = (rng.uniform(-1, 1, col.size) * tiny * 8).astype(out_np)
    s = np.abs(sddmm_model(off, col, Us, Vs))
    assert ((s > 0) & (s < tiny)).sum() > col.size // 20
    for path in ("wide", "element"):
        run(prec, off, col, Us, Vs, alpha, beta, None if beta == 0 else Cs, path=path)


@gpu
def test_bf16_equals_f32_on_the_widened_tensors():
    rng = np.random.default_rng(23)
    lens = _short_rows(2 * T + 5, rng)
    rows, cols = len(lens), 31
    off, col = _pattern(lens, cols, rng)
    for k in (5, 64, 129):
        U, V = _draw(rng, (rows, k), "bf16"), _draw(rng, (cols, k), "bf16")
        C = rng.uniform(-1, 1, col.size)
        for path in ("wide", "element"):
            narrow = run("bf16", off, col, U, V, 0.5, -1.5, C, path=path).clone()
            wide = run("f32", off, col, widen_bf16(U).reshape(U.shape), widen_bf16(V).reshape(V.shape), 0.5, -1.5, C, path=path)
            assert torch.equal(_raw(narrow), _raw(wide))


@gpu
@pytest.mark.parametrize("prec", ["f32", "f64", "bf16"])
def test_identities_on_integer_valued_inputs(prec):
    """every intermediate is an integer below 2^24 (bf16: inputs below 2^8): exact, so the association cannot matter"""
    rng = np.random.default_rng(29)
    out_np = np.float32 if prec == "bf16" else NP[prec]
    rows, cols, k = 83, 61, 33
    lens = [int(x) for x in rng.integers(0, 20, rows)]
    off, col = _pattern(lens, cols, rng)
    Ui, Vi = rng.integers(-8, 9, (rows, k)), rng.integers(-8, 9, (cols, k))
    conv = (lambda a: narrow_bf16(a.astype(np.float32)).reshape(a.shape)) if prec == "bf16" else (lambda a: a.astype(NP[prec]))
    r = entry_rows(off, col.size)
    # 1. the gather of the int64 dense product
    dense = Ui.astype(np.int64) @ Vi.astype(np.int64).T
    want = dense[r, col]
    for path in ("wide", "element"):
        got = run(prec, off, col, conv(Ui), conv(Vi), path=path)
        assert np.array_equal(got.cpu().numpy().astype(np.int64), want) and np.array_equal(got.cpu().numpy(), want.astype(out_np))
    # 2. the gradient of sum(dY * (A X)) with respect to A's values, by autograd on the host in float64 (exact on integers)
    vals = torch.from_numpy(rng.integers(-4, 5, col.size).astype(np.float64)).requires_grad_(True)
    dY, X = torch.from_numpy(Ui.astype(np.float64)), torch.from_numpy(Vi.astype(np.float64))
    A = torch.zeros(rows, cols, dtype=torch.float64).index_put((torch.from_numpy(r), torch.from_numpy(col.astype(np.int64))), vals, accumulate=True)
    (dY * (A @ X)).sum().backward()
    got = run(prec, off, col, conv(Ui), conv(Vi), path="wide")
    assert torch.equal(got.cpu().double(), vals.grad)
    if prec != "bf16":
        # ... and the forward product this is the gradient of runs on the same arrays: Y = A X through csrmm, U = dY, V = X
        tdt = TORCH[prec][0]
        d_vals = vals.detach().to(tdt).cuda()
        d_off, d_col, d_X = torch.from_numpy(off).cuda(), torch.from_numpy(col).cuda(), torch.from_numpy(Vi.astype(NP[prec])).cuda()
        Y = M.csrmm(d_vals, d_off, d_col, d_X)
        torch.cuda.synchronize()
        assert torch.equal(Y.cpu().double(), (A @ X).detach())


@gpu
@pytest.mark.parametrize("ld", [2 ** 30, 2 ** 30 + 1], ids=["wide", "element"])
@pytest.mark.parametrize("wide_operand", ["V", "U"])
def test_row_bases_beyond_4_gib(wide_operand, ld):
    """fp32, three rows with a leading dimension of 2^30 elements: the row bases are 0, 4 and 8 GiB (one element more: the
    element-wise kernel).  Only the three rows are ever touched (torch.empty commits nothing)."""
    rng = np.random.default_rng(31)
    k = 37
    big = torch.empty(2 * ld + k, dtype=torch.float32, device="cuda")
    Wide = torch.as_strided(big, (3, k), (ld, 1))
    wide_np = rng.uniform(-1, 1, (3, k)).astype(np.float32)
    Wide.copy_(torch.from_numpy(wide_np))
    if wide_operand == "V":
        rows, cols = 40, 3
        off, col = _pattern([int(x) for x in rng.integers(0, 7, rows)], cols, rng)
        other_np = rng.uniform(-1, 1, (rows, k)).astype(np.float32)
        other = torch.zeros(rows, 40, dtype=torch.float32, device="cuda")[:, :k]
        other.copy_(torch.from_numpy(other_np))
        U, V, U_np, V_np = other, Wide, other_np, wide_np
    else:
        rows, cols = 3, 40
        off, col = _pattern([30, 5, 45], cols, rng)
        other_np = rng.uniform(-1, 1, (cols, k)).astype(np.float32)
        other = torch.zeros(cols, 40, dtype=torch.float32, device="cuda")[:, :k]
        other.copy_(torch.from_numpy(other_np))
        U, V, U_np, V_np = Wide, other, wide_np, other_np
    assert {0, 1, 2} <= set((col if wide_operand == "V" else entry_rows(off, col.size)).tolist())
    want = sddmm_model(off, col, U_np, V_np, -2.0, 0.0)
    cbuf = torch.full((GUARD + col.size + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    out = cbuf[GUARD:GUARD + col.size]
    M.sddmm(torch.from_numpy(off).cuda(), torch.from_numpy(col).cuda(), U, V, out=out, alpha=-2.0)
    torch.cuda.synchronize()
    assert torch.equal(_raw(out).cpu(), torch.from_numpy(_bits(want)))
    assert bool(cbuf[:GUARD].isnan().all()) and bool(cbuf[GUARD + col.size:].isnan().all())
    assert torch.equal(Wide.cpu(), torch.from_numpy(wide_np))


@gpu
def test_graph_capture_and_replay():
    """one call is one kernel: captured, replayed after U was overwritten in place, equal to a fresh call and to the model"""
    rng = np.random.default_rng(37)
    lens = _short_rows(2 * T + 5, rng)
    rows, cols, k = len(lens), 19, 40
    off, col = _pattern(lens, cols, rng)
    U0, U1, V = _draw(rng, (rows, k), "f32"), _draw(rng, (rows, k), "f32"), _draw(rng, (cols, k), "f32")
    d_off, d_col = torch.from_numpy(off).cuda(), torch.from_numpy(col).cuda()
    dU, dV = torch.from_numpy(U0).cuda(), torch.from_numpy(V).cuda()
    out = torch.full((col.size,), float("nan"), dtype=torch.float32, device="cuda")
    M.sddmm(d_off, d_col, dU, dV, out=out, alpha=-2.0)          # (loads the code object outside the capture)
    torch.cuda.synchronize()
    assert torch.equal(_raw(out).cpu(), torch.from_numpy(_bits(sddmm_model(off, col, U0, V, -2.0))))
    out.fill_(float("nan"))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        M.sddmm(d_off, d_col, dU, dV, out=out, alpha=-2.0)
    dU.copy_(torch.from_numpy(U1))
    graph.replay()
    torch.cuda.synchronize()
    fresh = M.sddmm(d_off, d_col, dU, dV, alpha=-2.0)
    torch.cuda.synchronize()
    assert torch.equal(_raw(out), _raw(fresh))
    assert torch.equal(_raw(out).cpu(), torch.from_numpy(_bits(sddmm_model(off, col, U1, V, -2.0))))
