"""The deterministic multicolouring (include/mspmv.h: mspmv_csr_color_*; merge_spmv_amd.CsrColoring / csr_color / multicolor_reorder).
CPU: exports, argument conventions (nothing launched, no device), wrapper refusals, and the numpy model (tests/color_model.py) pinned
to an example coloured by hand.  GPU: colours, order, inverse, offsets and the figures by torch.equal against the model; independently
of the model, no stored off-diagonal entry joins two vertices of one colour; the LOWER and UPPER level schedules of P A P^T have at
most as many levels as there are colours and solve bit for bit what the model solves; IC(0)-preconditioned CG end to end in the
multicolour order.  Expected values never come from the library."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import merge_spmv_amd as M
from conftest import ROOT
import color_model as model
import csrsv_model as sv_model

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

NEW = ["mspmv_csr_color_create", "mspmv_csr_color_info", "mspmv_csr_color_colors", "mspmv_csr_color_order", "mspmv_csr_color_inverse",
       "mspmv_csr_color_offsets", "mspmv_csr_color_destroy"]
MAX_ITEMS = 2 ** 31 - 1 - 65536


# ---------------------------------------------------------------------------------------------------------------- patterns
def _csr(rowlists):
    off = np.zeros(len(rowlists) + 1, np.int32)
    np.cumsum([len(r) for r in rowlists], out=off[1:])
    return off, np.asarray([c for r in rowlists for c in r], np.int32)


def _sym(n, pairs):
    """the canonical pattern of the graph's adjacency + I: rows sorted, no column twice"""
    rows = [{r} for r in range(n)]
    for u, v in pairs:
        rows[u].add(v); rows[v].add(u)
    return [sorted(s) for s in rows]


def _grid5(n):
    at = lambda i, j: i * n + j
    return _sym(n * n, [(at(i, j), at(i, j + 1)) for i in range(n) for j in range(n - 1)] + [(at(i, j), at(i + 1, j)) for i in range(n - 1) for j in range(n)])


def _grid7(n):
    at = lambda i, j, k: (i * n + j) * n + k
    pairs = []
    for i in range(n):
        for j in range(n):
            for k in range(n):
                pairs += [(at(i, j, k), at(i + d[0], j + d[1], k + d[2])) for d in ((1, 0, 0), (0, 1, 0), (0, 0, 1))
                          if i + d[0] < n and j + d[1] < n and k + d[2] < n]
    return _sym(n ** 3, pairs)


def _clique_star(k=70, leaves=300):
    """a clique of k vertices (more than 64 colours: the mask window moves) and a star on vertex 0 (a hub: the whole wave scans it)"""
    return _sym(k + leaves, [(u, v) for u in range(k) for v in range(u)] + [(0, k + i) for i in range(leaves)])


def _rmat(scale=10, factor=8, seed=3):
    rng = np.random.default_rng(seed)
    n, m = 1 << scale, factor << scale
    u = np.zeros(m, np.int64); v = np.zeros(m, np.int64)
    for _ in range(scale):
        q = rng.choice(4, m, p=[0.57, 0.19, 0.19, 0.05])
        u = u * 2 + (q >> 1); v = v * 2 + (q & 1)
    return _sym(n, [(int(a), int(b)) for a, b in zip(u, v) if a != b])


def _one_sided(n=200, seed=5):
    """strictly lower, nothing mirrored, no diagonal: two vertices are joined by A[v,u] alone"""
    rng = np.random.default_rng(seed)
    return [sorted({int(c) for c in rng.integers(0, r, int(rng.integers(0, 5)))}) if r else [] for r in range(n)]


def _messy(n=150, seed=9):
    """unsorted rows, repeated columns, stored diagonals (some twice), empty rows at the front, in the middle and at the end"""
    rng = np.random.default_rng(seed)
    rowlists = []
    for r in range(n):
        if r < 3 or 70 <= r < 75 or r >= n - 4:
            rowlists.append([])
            continue
        cs = [int(c) for c in rng.integers(0, n, int(rng.integers(1, 9)))]
        cs += cs[:2] + [r] * int(rng.integers(0, 3))
        rng.shuffle(cs)
        rowlists.append(cs)
    return rowlists


def _path(n):
    return [[c for c in (r - 1, r + 1) if 0 <= c < n] for r in range(n)]


@functools.lru_cache(maxsize=None)
def _case(name):
    """name -> (off, col, priorities, the model's coloring): computed once, shared, left unchanged"""
    prio = None
    if name == "grid24":
        rowlists = _grid5(24)
    elif name == "grid80":
        rowlists = _grid5(80)                                      # 6400 vertices: above the cap of 4096, wide rounds and the finish
    elif name == "grid7":
        rowlists = _grid7(12)
    elif name == "clique_star":
        rowlists = _clique_star()
    elif name == "one_sided":
        rowlists = _one_sided()
    elif name == "messy":
        rowlists = _messy()
    elif name == "no_entries":
        rowlists = [[] for _ in range(5)]
    elif name == "path":
        rowlists, prio = _path(5000), np.full(5000, 7, np.int32)
    elif name == "ties":
        rowlists, prio = _grid5(24), np.random.default_rng(11).integers(0, 4, 576).astype(np.int32)
    elif name == "red_black":
        rowlists, prio = _grid5(24), (-np.arange(576)).astype(np.int32)
    elif name == "rmat":
        rowlists = _rmat()
    off, col = _csr(rowlists)
    for a in (off, col):
        a.setflags(write=False)
    return off, col, prio, model.coloring(off, col, prio)


CASES = ["grid24", "grid80", "grid7", "clique_star", "one_sided", "messy", "no_entries", "path", "ties", "red_black", "rmat"]
PROPERTY = ["grid24", "grid80", "grid7", "clique_star", "rmat"]


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_csr_color_symbols_are_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mspmv.h")).read(), flags=re.S)
    lib = M.load_library()
    for kind in ("product", "dev"):
        out = subprocess.run(["nm", "-D", "--defined-only", M.library_path(kind)], capture_output=True, text=True, check=True).stdout
        assert sorted(re.findall(r" T (mspmv_csr_color_\w+)", out)) == sorted(NEW), kind
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    for name in ("CsrColoring", "csr_color", "csr_permute", "multicolor_reorder"):
        assert name in M.__all__ and callable(getattr(M, name)), name
    assert lib.mspmv_version() == 102


def _create(rows, nnz, off=ctypes.c_void_p(4096), col=ctypes.c_void_p(4096), prio=None, handle=True):
    lib = M.load_library()
    h = ctypes.c_void_p(0)
    return lib.mspmv_csr_color_create(ctypes.byref(h) if handle else None, off, col, rows, nnz, prio, None, 0), h


def test_csr_color_argument_conventions():
    """every refusal comes before anything is launched or allocated: this runs without a device"""
    lib = M.load_library()
    assert _create(-1, 0)[0] == 1 and _create(5, -1)[0] == 1
    assert _create(MAX_ITEMS + 1, 0)[0] == 1 and _create(1000, MAX_ITEMS - 1000 + 1)[0] == 1 and _create(2 ** 31 - 1, 2 ** 31 - 1)[0] == 1
    assert _create(0, 7)[0] == 1                                  # entries without rows
    assert _create(5, 7, off=None)[0] == 1 and _create(5, 7, col=None)[0] == 1
    assert _create(0, 0, handle=False)[0] == 1                    # nowhere to put the handle
    info = M._CsrColorInfo()
    assert lib.mspmv_csr_color_info(None, ctypes.byref(info)) == 1 and lib.mspmv_csr_color_destroy(None) == 1
    for name in NEW[2:6]:
        assert getattr(lib, name)(None) is None, name
    # rows == 0: a valid handle with 0 colours; no device is touched
    for prio in (None, ctypes.c_void_p(4096)):
        status, h = _create(0, 0, off=None, col=None, prio=prio)
        assert status == 0 and h.value
        assert lib.mspmv_csr_color_info(h, None) == 1 and lib.mspmv_csr_color_info(h, ctypes.byref(info)) == 0
        assert (info.rows, info.nnz, info.colors, info.max_color_rows, info.rounds, info.edges, info.device_bytes) == (0, 0, 0, 0, 0, 0, 0)
        for name in NEW[2:6]:
            assert getattr(lib, name)(h) is None, name
        assert lib.mspmv_csr_color_destroy(h) == 0


def test_csr_color_wrappers_reject_bad_tensors_without_a_device():
    off, col = torch.zeros(4, dtype=torch.int32), torch.zeros(0, dtype=torch.int32)
    for bad in (lambda: M.CsrColoring(off, col), lambda: M.CsrColoring(None, col), lambda: M.csr_color(off, col),
                lambda: M.csr_color(off.to(torch.int64), col), lambda: M.csr_color(off, col, priorities=torch.zeros(3, dtype=torch.int32)),
                lambda: M.multicolor_reorder(torch.zeros(0), off, col), lambda: M.multicolor_reorder(None, off.tolist(), col)):
        with pytest.raises(M.MspmvError):
            bad()


def _fmix32(h):
    """the finaliser once more, in Python integers"""
    h ^= h >> 16; h = h * 0x85ebca6b & 0xffffffff; h ^= h >> 13; h = h * 0xc2b2ae35 & 0xffffffff; h ^= h >> 16
    return h


SIX = [[1, 2], [0, 1], [5], [1, 4], [3, 5, 5], []]                 # (1, 1) is a self loop; A[2,5] and A[3,1] have no mirror entry
SIX_PRIO = [5, 3, 9, 3, 1, 7]                                     # descending key: 2, 5, 0, 3, 1, 4 (3 before 1: the larger index)


def test_the_model_on_an_example_coloured_by_hand():
    assert _fmix32(0) == 0 and _fmix32(1) == 0x514e28b7
    sample = [0, 1, 2, 3, 255, 65536, 123456789, 2 ** 31, 2 ** 32 - 1]
    assert model.fmix32(np.array(sample)).tolist() == [_fmix32(v) for v in sample]
    assert model.keys(3).tolist() == [_fmix32(v) << 32 | v for v in range(3)]
    assert model.keys(3, np.array([-1, 0, 5], np.int32)).tolist() == [0xffffffff << 32, 1, 5 << 32 | 2]
    off, col = _csr(SIX)
    # 2 -> 0; 5 sees 2 (through A[2,5] alone) -> 1; 0 sees 2 -> 1; 3 sees no larger key -> 0; 1 sees 0 and 3 -> 2; 4 sees 3 and 5 -> 2
    got = model.coloring(off, col, np.array(SIX_PRIO, np.int32))
    assert got["colors"].tolist() == [1, 2, 0, 0, 2, 1]
    assert got["order"].tolist() == [2, 3, 0, 5, 1, 4] and got["inverse"].tolist() == [2, 4, 0, 1, 5, 3]
    assert got["offsets"].tolist() == [0, 2, 4, 6]
    assert (got["num_colors"], got["max_color_rows"], got["edges"]) == (3, 2, 9)
    # without the mirror of A[2,5], vertex 5 (an empty row) would have taken colour 0, vertex 2's
    assert model.neighbours(off, col)[5] == {2, 4} and model.neighbours(off, col)[1] == {0, 3}
    # all priorities equal: the key falls to the index, the path is coloured from its top
    off, col = _csr(_path(7))
    assert model.colors(off, col, np.zeros(7, np.int32)).tolist() == [0, 1, 0, 1, 0, 1, 0]
    assert model.coloring(*_csr([[] for _ in range(3)]))["offsets"].tolist() == [0, 3]
    assert model.coloring(*_csr([]))["offsets"].tolist() == [0] and model.coloring(*_csr([]))["num_colors"] == 0


# ---------------------------------------------------------------------------------------------------------------- GPU
def _device(a):
    return torch.from_numpy(np.array(a)).cuda()                   # (a copy: the shared cases are read-only)


def _color(name, debug=False):
    off, col, prio, want = _case(name)
    d_off, d_col = _device(off), _device(col)
    d_prio = None if prio is None else _device(prio)
    coloring = M.CsrColoring(d_off, d_col, d_prio, debug_synchronous=debug)
    torch.cuda.synchronize()
    assert torch.equal(d_off.cpu(), torch.from_numpy(off.copy())) and torch.equal(d_col.cpu(), torch.from_numpy(col.copy()))
    return coloring, want, (d_off, d_col)


@gpu
@pytest.mark.parametrize("name", CASES)
def test_coloring_equals_the_model(name):
    off, col, prio, _ = _case(name)
    coloring, want, _ = _color(name)
    rows = len(off) - 1
    colors = coloring.colors.cpu()
    for key in ("colors", "order", "inverse", "offsets"):
        got = getattr(coloring, key).cpu()
        assert got.dtype == torch.int32 and torch.equal(got, torch.from_numpy(want[key])), key
    info = coloring.info
    assert (info["rows"], info["nnz"], info["colors"], info["max_color_rows"], info["edges"]) == \
        (rows, len(col), want["num_colors"], want["max_color_rows"], want["edges"])
    assert coloring.num_colors == want["num_colors"] and info["device_bytes"] == 4 * (3 * rows + want["num_colors"] + 1) and info["rounds"] >= 0
    # independently of the model: a proper colouring, and order is a permutation
    r_of = np.repeat(np.arange(rows), np.diff(off))
    c = colors.numpy()
    assert (c >= 0).all() and not ((c[r_of] == c[col]) & (r_of != col)).any()
    assert np.array_equal(np.sort(coloring.order.cpu().numpy()), np.arange(rows))
    if name == "no_entries":
        assert c.tolist() == [0] * 5 and info["rounds"] == 0
        none = M.CsrColoring(torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"))
        assert none.num_colors == 0 and none.offsets.tolist() == [0] and none.colors.numel() == none.order.numel() == none.inverse.numel() == 0
        none.close()
    if name == "path":
        assert c.tolist() == [(rows - 1 - v) % 2 for v in range(rows)]
    if name == "red_black":
        assert coloring.num_colors == 2 and c.tolist() == [1 - (v // 24 + v % 24) % 2 for v in range(rows)]
    if name == "clique_star":
        assert coloring.num_colors == 70
    coloring.close()
    if name in ("no_entries", "ties"):                             # the one-shot wrapper; a closed handle has nothing to show
        again = _color(name)[0]
        again.close()
        with pytest.raises(M.MspmvError):
            again.order
        d_off, d_col = _device(off), _device(col)
        got, n = M.csr_color(d_off, d_col, None if prio is None else _device(prio))
        assert n == want["num_colors"] and torch.equal(got.cpu(), torch.from_numpy(want["colors"]))


@gpu
def test_wide_rounds_and_the_one_workgroup_finish_both_run(capfd):
    capfd.readouterr()
    coloring, want, _ = _color("grid80", debug=True)
    lines = [l for l in capfd.readouterr().out.splitlines() if l.startswith("mspmv: ")]
    wide = [l for l in lines if l.startswith("mspmv: color_wide_kernel<<<")]
    narrow = [l for l in lines if l.startswith("mspmv: color_narrow_kernel<<<1, 1024>>>")]
    assert len(wide) >= 1 and len(narrow) == 1 and coloring.info["rounds"] == len(wide) + 1, lines
    assert lines.index(narrow[0]) > lines.index(wide[-1])
    assert torch.equal(coloring.colors.cpu(), torch.from_numpy(want["colors"]))
    # at or below the cap the one workgroup does it all
    capfd.readouterr()
    coloring, want, _ = _color("grid24", debug=True)
    lines = [l for l in capfd.readouterr().out.splitlines() if l.startswith("mspmv: ")]
    assert not [l for l in lines if "color_wide_kernel" in l] and len([l for l in lines if "color_narrow_kernel" in l]) == 1
    assert coloring.info["rounds"] == 1


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def _values(off, col, rng):
    """diagonal in [1, 2], everything else in [-1, 1] divided by the row length"""
    r_of = np.repeat(np.arange(len(off) - 1), np.diff(off))
    n = np.diff(off)[r_of]
    return np.where(col == r_of, rng.uniform(1, 2, len(col)), rng.uniform(-1, 1, len(col)) / n)


@gpu
@pytest.mark.parametrize("name", PROPERTY)
def test_the_permuted_matrix_has_at_most_as_many_levels_as_colours(name):
    off, col, _, want = _case(name)
    rows = len(off) - 1
    rng = np.random.default_rng(17)
    val, b = _values(off, col, rng), rng.uniform(-1, 1, rows)
    off_p, col_p, val_p, _ = model.permute(off, col, val, rows, want["order"], want["inverse"])
    d_off, d_col, d_val, d_b = _device(off), _device(col), _device(val), _device(b)
    coloring, csr = M.multicolor_reorder(d_val, d_off, d_col)
    assert torch.equal(coloring.order.cpu(), torch.from_numpy(want["order"]))
    assert torch.equal(csr.row_offsets.cpu(), torch.from_numpy(off_p)) and torch.equal(csr.column_indices.cpu(), torch.from_numpy(col_p))
    assert torch.equal(csr.values.cpu().view(torch.int64), torch.from_numpy(_bits(val_p)))
    b_p = coloring.permute_vector(d_b)
    assert torch.equal(b_p.cpu(), torch.from_numpy(b[want["order"]]))
    assert torch.equal(coloring.permute_vector(b_p, back=True).cpu(), torch.from_numpy(b))
    for lower in (True, False):
        plan = M.CsrSv(csr.row_offsets, csr.column_indices, lower=lower)
        levels = sv_model.levels(off_p, col_p, lower)
        order, lo = sv_model.schedule(levels)
        assert plan.info["levels"] <= coloring.num_colors, (lower, plan.info["levels"], coloring.num_colors)
        assert plan.info["levels"] == len(lo) - 1
        assert torch.equal(plan.order.cpu(), torch.from_numpy(order)) and torch.equal(plan.level_offsets.cpu(), torch.from_numpy(lo))
        x = plan.solve(csr.values, b_p)
        want_x = sv_model.solve(off_p, col_p, val_p, b[want["order"]], 1.0, lower, False)
        assert torch.equal(x.cpu().view(torch.int64), torch.from_numpy(_bits(want_x))), lower
        torch.cuda.synchronize()
        plan.close()
    coloring.close()


# ---- end to end: IC(0)-preconditioned conjugate gradients in natural and in multicolour order (the loop of tests/test_csric0.py)
def _pcg(d_val, d_off, d_col, b, precondition, limit=400):
    """conjugate gradients on the device: A p by csrmv, dots and updates in torch; stops when the recurrence residual reaches
    1e-10 |b|.  (x, iterations)"""
    n = b.numel()
    x = torch.zeros_like(b)
    r = b.clone()
    z = precondition(r).clone()
    p = z.clone()
    rz = torch.dot(r, z)
    stop = 1e-10 * float(torch.linalg.norm(b))
    for it in range(1, limit + 1):
        q = M.csrmv(d_val, d_off, d_col, p, num_cols=n)
        alpha = rz / torch.dot(p, q)
        x += alpha * p
        r -= alpha * q
        if float(torch.linalg.norm(r)) <= stop:
            return x, it
        z = precondition(r)
        rz_new = torch.dot(r, z)
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, limit + 1


@gpu
def test_preconditioned_conjugate_gradients_in_multicolour_order():
    """the 5-point Laplacian of a 24 x 24 grid, fp64, the right-hand side and the stopping rule of tests/test_csric0.py: IC(0) in
    natural order, IC(0) on P A P^T with b[order] and the result mapped back through inverse, and no preconditioner.  All three
    converge, the true residual recomputed on the host in the ORIGINAL numbering is <= 1e-8 |b|, the reordered run takes fewer
    iterations than the plain one (the numpy model of this loop: 48 against 88, 32 in natural order: the weaker factor is the known
    price of the ordering), and the reordered factor's lower plan has at most as many levels as there are colours."""
    off, col, _, _ = _case("grid24")
    n = len(off) - 1
    r_of = np.repeat(np.arange(n), np.diff(off))
    val = np.where(col == r_of, 4.0, -1.0)
    b = np.random.default_rng(22).uniform(-1, 1, n)
    d_off, d_col, d_val, d_b = _device(off), _device(col), _device(val), _device(b)
    ic = M.Ic0(d_off, d_col)
    assert int(ic.factor(d_val).item()) == -1
    x_ic, it_ic = _pcg(d_val, d_off, d_col, d_b, ic.solve)
    x_cg, it_cg = _pcg(d_val, d_off, d_col, d_b, lambda r: r)
    coloring, p = M.multicolor_reorder(d_val, d_off, d_col)
    ic_mc = M.Ic0(p.row_offsets, p.column_indices)
    assert int(ic_mc.factor(p.values).item()) == -1
    x_p, it_mc = _pcg(p.values, p.row_offsets, p.column_indices, coloring.permute_vector(d_b), ic_mc.solve)
    x_mc = coloring.permute_vector(x_p, back=True)
    torch.cuda.synchronize()
    print(f"pcg: {it_ic} iterations with IC(0) in natural order, {it_mc} in multicolour order, {it_cg} without")
    print(f"pcg: lower plan: {ic.lower.info['levels']} levels, {ic.lower.info['launches']} launches in natural order; "
          f"{ic_mc.lower.info['levels']} levels, {ic_mc.lower.info['launches']} launches in multicolour order ({coloring.num_colors} colours)")
    assert it_ic <= 400 and it_mc <= 400 and it_cg <= 400
    for x in (x_ic, x_mc, x_cg):
        ax = np.zeros(n)
        np.add.at(ax, r_of, val * x.cpu().numpy()[col])
        res = float(np.linalg.norm(b - ax))
        print(f"pcg: true residual {res:.3e}, |b| {np.linalg.norm(b):.3e}")
        assert res <= 1e-8 * float(np.linalg.norm(b))
    assert it_mc < it_cg, (it_mc, it_cg)
    assert ic_mc.lower.info["levels"] <= coloring.num_colors
    for h in (ic, ic_mc, coloring):
        h.close()
