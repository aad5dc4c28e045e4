"""mspmv_csr_fill_* (merge_spmv_amd.CsrFill / csr_fill; include/mspmv_fill.h, libmspmv_fill.so): the level-of-fill pattern F_p, its
levels and its sources, compared EXACTLY with tests/fill_model.py -- the classical row-by-row symbolic ILU(p), where the device runs
one levelled product per level -- and the scatter of values into the filled pattern, on the bits.  There is no tolerance anywhere.
The CPU part: the boundary (header, exports, prototypes, refusals before any device is touched, no rows), the model against the
product form restated as a fixed point, and the counts the device tests assert through the model."""
import ctypes
import functools
import importlib
import os
import subprocess
import time

import numpy as np
import pytest

import merge_spmv_amd as M
from conftest import ROOT
import fill_model as model
from test_abi_prototypes import declared, mismatches, prototyped
from test_code_object import READELF, kernel_resources

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu
F = importlib.import_module("merge_spmv_amd.fill")

NEW = ["mspmv_csr_fill_column_indices", "mspmv_csr_fill_create", "mspmv_csr_fill_destroy", "mspmv_csr_fill_info", "mspmv_csr_fill_levels",
       "mspmv_csr_fill_row_offsets", "mspmv_csr_fill_source", "mspmv_csr_fill_values_f32", "mspmv_csr_fill_values_f64"]
LIMIT = 2 ** 31 - 65537                          # rows + entries + pairs of a round, at most


# ------------------------------------------------------------------------------------------------------------ the boundary
def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(l.split()[-1] for l in out.splitlines() if " T mspmv_" in l)


def test_the_header_is_plain_c(tmp_path):
    src = tmp_path / "hdr.c"
    src.write_text('#include "include/mspmv_fill.h"\n'
                   "int use(void) { mspmv_csr_fill_t *f = 0; mspmv_csr_fill_info_t info;\n"
                   "  int e = mspmv_csr_fill_create(&f, 0, 0, 0, 0, MSPMV_CSR_FILL_MAX_LEVEL, 0, 0);\n"
                   "  e |= mspmv_csr_fill_info(f, &info); e |= mspmv_csr_fill_values_f64(f, 0, 0, 0, 0);\n"
                   "  return e | mspmv_csr_fill_destroy(f) | (mspmv_csr_fill_source(f) != 0) | info.max_level; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-c", str(src), "-o", str(tmp_path / "hdr.o"), "-I", ROOT],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_library_exports_what_the_header_declares_and_nothing_else():
    functions = declared("mspmv_fill.h")
    assert sorted(functions) == NEW
    assert _exported(F.fill_library_path()) == NEW
    assert not set(_exported(M.library_path("product"))) & set(NEW) and not set(declared("mspmv.h")) & set(NEW)
    undefined = subprocess.run(["nm", "-D", "--undefined-only", F.fill_library_path()], capture_output=True, text=True, check=True).stdout
    assert not [l for l in undefined.splitlines() if " mspmv_" in l]              # it calls nothing of libmspmv.so
    assert "getenv" not in undefined


def test_the_prototypes_match_the_header():
    lib = F.load_fill_library()
    functions = declared("mspmv_fill.h")
    assert mismatches(lib, functions) == []
    assert sorted(prototyped(lib)) == sorted(functions)
    assert functions["mspmv_csr_fill_create"] == ("i32", ["pointer"] * 3 + ["i32"] * 3 + ["pointer", "i32"])
    assert functions["mspmv_csr_fill_levels"] == ("pointer", ["pointer"])
    product = M.load_library()
    assert lib is not product and not [n for n in prototyped(product) if "csr_fill" in n]
    # the info block as ctypes lays it out is the header's: six int32, one uint64
    assert ctypes.sizeof(F._CsrFillInfo) == 32 and F._CsrFillInfo.max_level.offset == 16 and F._CsrFillInfo.device_bytes.offset == 24


def test_the_surface():
    assert M.CsrFill is F.CsrFill and M.csr_fill is F.csr_fill and "CsrFill" not in M.__all__
    assert issubclass(M.Iluk, M.Ilu0) and issubclass(M.Ick, M.Ic0)
    assert M.load_library().mspmv_version() == 102
    for fn in (M.pcg, M.bicgstab, M.gmres):
        import inspect
        assert inspect.signature(fn).parameters["fill_level"].default == 0


@pytest.mark.skipif(not os.path.exists(READELF), reason="needs ROCm's llvm-readelf")
def test_no_kernel_of_the_library_spills_or_uses_scratch():
    rows = kernel_resources(F.fill_library_path())
    assert len([n for n in rows if "fill_" in n]) >= 10 and any("tr_downsweep_kernel" in n for n in rows)
    bad = {n: r for n, r in rows.items() if r["vgpr_spill_count"] or r["sgpr_spill_count"] or r["private_segment_fixed_size"]}
    assert not bad, bad


def _create(rows, nnz, level=1, off=4096, col=4096, out=True):
    """mspmv_csr_fill_create on fake device pointers (refusals come before anything is touched; rows == 0 touches nothing at all)"""
    lib = F.load_fill_library()
    handle = ctypes.c_void_p(0x55)
    st = lib.mspmv_csr_fill_create(ctypes.byref(handle) if out else None, ctypes.c_void_p(off) if off else None,
                                   ctypes.c_void_p(col) if col else None, rows, nnz, level, None, 0)
    return st, handle.value


def test_create_refuses_before_any_launch():
    for bad in (dict(rows=-1, nnz=0), dict(rows=5, nnz=-1), dict(rows=2 ** 30 + 1, nnz=0), dict(rows=2 ** 30, nnz=2 ** 30),
                dict(rows=1000, nnz=LIMIT - 1000 + 1), dict(rows=0, nnz=5), dict(rows=5, nnz=5, level=-1), dict(rows=5, nnz=5, level=33),
                dict(rows=5, nnz=5, off=0), dict(rows=5, nnz=5, col=0), dict(rows=5, nnz=0, off=0)):
        assert _create(**bad) == (1, None), bad                                   # hipErrorInvalidValue, *fill NULL
    assert _create(0, 0, out=False)[0] == 1
    lib = F.load_fill_library()
    assert lib.mspmv_csr_fill_destroy(None) == 1 and lib.mspmv_csr_fill_info(None, None) == 1
    assert lib.mspmv_csr_fill_values_f32(None, None, None, None, 0) == 1 and lib.mspmv_csr_fill_values_f64(None, None, None, None, 0) == 1
    assert lib.mspmv_csr_fill_levels(None) is None


@pytest.mark.parametrize("level", [0, 1, 32])
def test_no_rows_touch_no_device(level):
    lib = F.load_fill_library()
    st, handle = _create(0, 0, level=level, off=0, col=0)
    assert st == 0 and handle
    handle = ctypes.c_void_p(handle)
    info = F._CsrFillInfo()
    assert lib.mspmv_csr_fill_info(handle, ctypes.byref(info)) == 0 and lib.mspmv_csr_fill_info(handle, None) == 1
    assert (info.rows, info.nnz, info.level, info.nnz_filled, info.max_level, info.device_bytes) == (0, 0, level, 0, 0, 0)
    for getter in ("row_offsets", "column_indices", "levels", "source"):
        assert getattr(lib, "mspmv_csr_fill_" + getter)(handle) is None
    assert lib.mspmv_csr_fill_values_f32(handle, None, None, None, 0) == 0 and lib.mspmv_csr_fill_values_f64(handle, None, None, None, 0) == 0
    assert lib.mspmv_csr_fill_destroy(handle) == 0


# ------------------------------------------------------------------------------------------------------------ the model
LEVELS = (0, 1, 2, 3, 5)


def _random_cases(count, seed):
    rng = np.random.default_rng(seed)
    return [model.random_pattern(rng, int(rng.integers(1, 41)), rng.uniform(0.02, 0.3), symmetric=t % 3 == 0) for t in range(count)]


def _well_formed(pat, p, got):
    off, col = pat
    foff, fcol, lev, src = got
    rows = len(off) - 1
    assert foff.dtype == fcol.dtype == lev.dtype == src.dtype == np.int32 and foff[0] == 0 and len(foff) == rows + 1
    assert foff[-1] == len(fcol) == len(lev) == len(src)
    for i in range(rows):
        assert (np.diff(fcol[foff[i]:foff[i + 1]]) > 0).all()                     # canonical
    assert lev.min(initial=0) >= 0 and lev.max(initial=0) <= p
    kept = src >= 0
    assert np.array_equal(src[kept], np.arange(len(col))) and (lev[kept] == 0).all() and (lev[~kept] > 0).all()
    assert np.array_equal(fcol[kept], col)


def test_the_model_is_the_fixed_point_of_the_levelled_product():
    """statement (1), the classical algorithm, against statement (2) restated on its own, on random patterns with 15 % of the
    diagonals missing; a third of them structurally symmetric, whose fill and levels are then symmetric too"""
    for t, pat in enumerate(_random_cases(120, 7)):
        for p in LEVELS:
            got = model.fill(*pat, p)
            _well_formed(pat, p, got)
            d = model.as_dict(got[0], got[1], got[2])
            assert d == model.fill_product(*pat, p), (t, p)
            if t % 3 == 0:
                assert all(d.get((j, i)) == l for (i, j), l in d.items())
        zero = model.fill(*pat, 0)
        assert np.array_equal(zero[0], pat[0]) and np.array_equal(zero[1], pat[1]) and not zero[2].any()


def _count(pat, p):
    return len(model.fill(*pat, p)[1])


def test_the_counts_of_the_model():
    assert [_count(model.grid2d(12), p) for p in range(4)] == [672, 914, 1134, 1552]
    assert [_count(model.grid2d(12, order=model.red_black(12)), p) for p in (0, 1, 2)] == [672, 1154, 1154]
    assert [_count(model.grid3d(6), p) for p in range(3)] == [1296, 2196, 3416]
    for p in (0, 1, 2, 5, 9, 10, 32):
        off, col, lev, _ = model.fill(*model.cycle(12), p)
        assert len(col) == 36 + 2 * min(p, 9) and lev.max() == min(p, 9)
        assert sorted(np.bincount(lev)[1:]) == [2] * min(p, 9)                    # each level exists only through the one below it
    assert [_count(model.arrow(70), p) for p in (0, 1, 2)] == [208, 4900, 4900]
    assert [_count(model.arrow(70, first=False), p) for p in (0, 1, 5)] == [208, 208, 208]
    assert [_count(model.grid2d(70), p) for p in (1, 2)] == [33742, 43126]
    assert _count(model.diagonal(9), 3) == 9 and _count(model.empty(5), 3) == 0 and _count(model.from_pairs(1, [(0, 0)]), 3) == 1


def _full_arrow(n):
    """F_p, p >= 1, of the arrow with a dense first row and column in closed form: every position, level 1 off the arrow"""
    i, j = np.divmod(np.arange(n * n), n)
    lev = ((i != j) & (i != 0) & (j != 0)).astype(np.int32)
    src = np.full(n * n, -1, np.int32)
    src[lev == 0] = np.arange(3 * n - 2)
    return np.arange(0, n * n + 1, n, dtype=np.int32), j.astype(np.int32), lev, src


def test_the_closed_form_of_the_full_arrow_is_the_models():
    for p in (1, 2):
        for got, want in zip(_full_arrow(70), model.fill(*model.arrow(70), p)):
            assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------------------ the device
PATTERNS = {
    "one": lambda: model.from_pairs(1, [(0, 0)]),
    "empty5": lambda: model.empty(5),
    "diagonal": lambda: model.diagonal(9),
    "grid12": lambda: model.grid2d(12),
    "grid12-red-black": lambda: model.grid2d(12, order=model.red_black(12)),
    "grid3d-6": lambda: model.grid3d(6),
    "cycle12": lambda: model.cycle(12),
    "arrow70": lambda: model.arrow(70),
    "arrow70-last": lambda: model.arrow(70, first=False),
    "grid70": lambda: model.grid2d(70),
}
CASES = [("one", 0), ("one", 3), ("empty5", 0), ("empty5", 2), ("diagonal", 0), ("diagonal", 3)] + [("grid12", p) for p in range(4)] + [("grid12-red-black", p) for p in (0, 1, 2)] \
    + [("grid3d-6", p) for p in range(3)] + [("cycle12", p) for p in (0, 1, 2, 5, 9, 10, 32)] + [("arrow70", p) for p in (0, 1, 2)] \
    + [("arrow70-last", p) for p in (0, 1, 4)] + [("grid70", p) for p in (0, 1, 2)]


@functools.lru_cache(maxsize=None)
def _pattern(name):
    return PATTERNS[name]()


@functools.lru_cache(maxsize=None)
def _reference(name, p):
    """the model's run, computed once and shared"""
    return model.fill(*_pattern(name), p)


def _device_fill(pat, p, **kw):
    """((off, col, levels, source) as numpy, info) of the device, with the input arrays checked to be bitwise unchanged"""
    d_off, d_col = (torch.from_numpy(a).cuda() for a in pat)
    fill = M.CsrFill(d_off, d_col, p, **kw)
    try:
        got = tuple(t.cpu().numpy() for t in (fill.row_offsets, fill.column_indices, fill.levels, fill.source))
        info = dict(fill.info)
        assert fill.nnz_filled == info["nnz_filled"] and (info["rows"], info["nnz"], info["level"]) == (len(pat[0]) - 1, len(pat[1]), p)
    finally:
        fill.close()
    assert np.array_equal(d_off.cpu().numpy(), pat[0]) and np.array_equal(d_col.cpu().numpy(), pat[1])
    return got, info


def _assert_fill(got, info, want):
    for name, g, w in zip(("row_offsets", "column_indices", "levels", "source"), got, want):
        assert g.dtype == np.int32 and np.array_equal(g, w), name
    assert info["nnz_filled"] == len(want[1]) and info["max_level"] == int(want[2].max(initial=0))
    assert info["device_bytes"] == 4 * (len(want[0]) + 3 * len(want[1]))


def _assert_level_zero(got, info, pat):
    """F_0 is A: its offsets and columns, levels all 0, source the identity"""
    assert np.array_equal(got[0], pat[0]) and np.array_equal(got[1], pat[1]) and not got[2].any()
    assert np.array_equal(got[3], np.arange(len(pat[1]))) and (info["nnz_filled"], info["max_level"]) == (len(pat[1]), 0)


@gpu
@pytest.mark.parametrize("name,p", CASES, ids=[f"{n}-p{p}" for n, p in CASES])
def test_the_filled_pattern_is_the_models(name, p):
    pat, want = _pattern(name), _reference(name, p)
    got, info = _device_fill(pat, p)
    print(f"fill {name} p = {p}: {len(pat[1])} -> {info['nnz_filled']} entries, max level {info['max_level']}")
    _assert_fill(got, info, want)
    if p == 0:
        _assert_level_zero(got, info, pat)


@gpu
def test_the_cycle_climbs_one_level_at_a_time():
    for p in (0, 1, 2, 5, 9, 10, 32):
        got, info = _device_fill(_pattern("cycle12"), p)
        assert (info["nnz_filled"], info["max_level"]) == (36 + 2 * min(p, 9), min(p, 9))


@gpu
def test_one_row_longer_than_a_workgroup():
    """the arrow of 300: row 0 holds 300 entries, every other row's pairs are 299 of one entry, and F_1 is full (90 000 entries)"""
    got, info = _device_fill(model.arrow(300), 0)
    _assert_level_zero(got, info, model.arrow(300))
    for p in (1, 2):
        got, info = _device_fill(model.arrow(300), p)
        _assert_fill(got, info, _full_arrow(300))
    got, info = _device_fill(model.arrow(300, first=False), 3)
    assert info["nnz_filled"] == 898 and info["max_level"] == 0


@gpu
def test_random_patterns_with_missing_diagonals():
    for t, pat in enumerate(_random_cases(30, 11)):
        for p in (0, 1, 2, 3, 5):
            want = model.fill(*pat, p)
            got, info = _device_fill(pat, p)
            _assert_fill(got, info, want)
            if p == 0:
                _assert_level_zero(got, info, pat)
            if t % 3 == 0:                                                        # structurally symmetric: so are F_p and its levels
                d = model.as_dict(got[0], got[1], got[2])
                assert all(d.get((j, i)) == l for (i, j), l in d.items())


@gpu
def test_a_fill_beyond_the_count_limit_is_refused_from_the_counts():
    """the arrow of 46 400 rows at p = 1: 46 399 entries below the diagonal with 46 399 pairs each, (n - 1)^2 > 2^31"""
    n = 46400
    assert (n - 1) ** 2 > 2 ** 31
    here = torch.arange(n, dtype=torch.int32, device="cuda")
    off = torch.cat([torch.zeros(1, dtype=torch.int32, device="cuda"), n + 2 * here]).contiguous()
    off[-1] = 3 * n - 2
    col = torch.cat([here, torch.stack([torch.zeros(n - 1, dtype=torch.int32, device="cuda"), here[1:]], dim=1).reshape(-1)]).contiguous()
    assert col.numel() == 3 * n - 2 and int(off[1]) == n and int(off[2]) == n + 2
    torch.cuda.synchronize()
    lib = F.load_fill_library()
    handle = ctypes.c_void_p(0x55)
    before = torch.cuda.mem_get_info()[0]
    t0 = time.perf_counter()
    st = lib.mspmv_csr_fill_create(ctypes.byref(handle), ctypes.c_void_p(off.data_ptr()), ctypes.c_void_p(col.data_ptr()), n, col.numel(), 1,
                                   None, 0)
    seconds = time.perf_counter() - t0
    print(f"fill beyond the limit: refused after {seconds * 1e3:.2f} ms")
    assert st == 1 and handle.value is None
    assert seconds < 1.0                                                          # from the counts: nothing of 2^31 entries was made
    assert torch.cuda.mem_get_info()[0] >= before - (1 << 20)                     # nothing leaked
    with pytest.raises(M.MspmvError):
        M.CsrFill(off, col, 1)
    fill = M.CsrFill(off, col, 0)                                                 # the same pattern at level 0 is fine
    assert fill.nnz_filled == 3 * n - 2
    fill.close()
    got, info = _device_fill(_pattern("grid12"), 1)                               # and a small one afterwards
    _assert_fill(got, info, _reference("grid12", 1))


@gpu
def test_launch_lines(capfd):
    capfd.readouterr()
    _device_fill(_pattern("grid12"), 2, debug_synchronous=True)
    lines = [l for l in capfd.readouterr().out.splitlines() if l.startswith("mspmv: ")]
    for kernel in ("fill_init_kernel", "fill_upper_kernel", "fill_lengths_kernel", "fill_total_kernel", "fill_keep_kernel", "fill_expand_kernel",
                   "fill_compact_kernel", "fill_unpack_kernel"):
        assert sum(l.startswith(f"mspmv: {kernel}<<<") for l in lines) == (1 if kernel in ("fill_init_kernel", "fill_unpack_kernel") else 2), kernel


# ------------------------------------------------------------------------------------------------------------ the values
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def _special_values(n, dtype, seed=4):
    v = np.random.default_rng(seed).uniform(-1, 1, n).astype(dtype)
    v[::7] = -0.0
    v[3] = np.nan; v[5] = np.inf; v[8] = -np.inf; v[11] = np.finfo(dtype).tiny / 4       # a NaN, infinities, a subnormal
    return v


@gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_values_are_moved_on_the_bits(dtype):
    """fill entries +0.0 whatever A stores elsewhere; NaN, Inf, -0.0 and subnormals arrive untouched; guard words either side of an
    output that starts one element behind a 16-byte boundary; on a side stream; in a replayed graph"""
    pat = _pattern("grid12")
    off, col, lev, src = _reference("grid12", 2)
    val = _special_values(len(pat[1]), dtype)
    want = model.scatter(val, src)
    assert (_bits(want[src < 0]) == 0).all() and np.signbit(want[src >= 0][::7]).all()
    d_off, d_col, d_val = (torch.from_numpy(a).cuda() for a in (pat[0], pat[1], val))
    fill = M.CsrFill(d_off, d_col, 2)
    nf = fill.nnz_filled
    out = fill.values(d_val)
    assert out.dtype == d_val.dtype and np.array_equal(_bits(out.cpu().numpy()), _bits(want))
    guard = dtype(-7.25)
    buf = torch.full((nf + 6,), float(guard), dtype=d_val.dtype, device="cuda")
    start = 1 + (-(buf.data_ptr() // buf.element_size()) % (16 // buf.element_size()))      # one element behind a 16-byte boundary
    view = buf[start:start + nf]
    assert view.data_ptr() % 16 == buf.element_size()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    assert fill.values(d_val, out=view, stream=side) is view
    side.synchronize()
    host = buf.cpu().numpy()
    assert np.array_equal(_bits(host[start:start + nf]), _bits(want))
    assert (host[:start] == guard).all() and (host[start + nf:] == guard).all()
    assert np.array_equal(_bits(d_val.cpu().numpy()), _bits(val))                 # the input is only read
    # captured once, replayed on new values
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fill.values(d_val, out=view)
    for seed in (5, 6):
        again = _special_values(len(val), dtype, seed)
        d_val.copy_(torch.from_numpy(again))
        view.fill_(3)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(view.cpu().numpy()), _bits(model.scatter(again, src)))
    both = torch.zeros(len(val) + nf, dtype=d_val.dtype, device="cuda")
    other = torch.float64 if dtype == np.float32 else torch.float32
    for bad in (dict(values=d_val[:-1]), dict(values=d_val, out=buf[:nf - 1]), dict(values=d_val, out=torch.empty(nf, dtype=other, device="cuda")),
                dict(values=d_val.cpu()), dict(values=both[:len(val)], out=both[len(val) - 1:len(val) - 1 + nf])):      # (the last: they overlap)
        with pytest.raises(M.MspmvError):
            fill.values(bad["values"], out=bad.get("out"))
    assert np.array_equal(fill.source.cpu().numpy(), src)
    fill.close()
    with pytest.raises(M.MspmvError, match="closed"):
        fill.values(d_val)
    assert np.array_equal(fill.source.cpu().numpy(), src)                         # (a closed handle still shows what it was asked for before)
    with pytest.raises(M.MspmvError, match="closed"):
        fill.levels


@gpu
def test_the_one_shot_call():
    pat = _pattern("grid3d-6")
    off, col, lev, src = _reference("grid3d-6", 1)
    val = np.random.default_rng(2).uniform(-1, 1, len(pat[1]))
    d_off, d_col, d_val = (torch.from_numpy(a).cuda() for a in (pat[0], pat[1], val))
    csr = M.csr_fill(d_val, d_off, d_col, 1)
    assert (csr.rows, csr.cols, csr.nnz) == (216, 216, 2196)
    for got, want in ((csr.row_offsets, off), (csr.column_indices, col), (csr.levels, lev)):
        assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(_bits(csr.values.cpu().numpy()), _bits(model.scatter(val, src)))
    assert M.csr_fill(None, d_off, d_col, 1).values is None
    with pytest.raises(M.MspmvError):
        M.CsrFill(d_off, d_col, 33)
    with pytest.raises(M.MspmvError):
        M.CsrFill(d_off, d_col, -1)
