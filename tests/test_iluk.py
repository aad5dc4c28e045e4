"""Iluk / Ick (merge_spmv_amd.solve) and the fill_level of the one-shot solvers: ILU(k) / IC(k) as CsrFill's pattern, the scatter of A's
values into it and the unchanged numeric kernels.  Everything is compared ON THE BITS with the models run on the MODEL's filled
arrays (tests/fill_model.py): the factor with csrilu0_model / csric0_model, the sweeps with csrsv_model, and the solvers with
bicgstab_model / gmres_model / pcg_model whose M^-1 is those sweep models on the model's factor.  A p of the solver models is
M.csrmv on the device, as in the solvers' own tests (the library has no host model of csrmv's bits for general values); the CPU part
uses the host product.  There is no tolerance anywhere."""
import functools

import numpy as np
import pytest

import merge_spmv_amd as M
import bicgstab_common as C
import bicgstab_model
import csric0_model
import csrilu0_model
import csrsv_model
import fill_model
import gmres_model
import pcg_model
from pcg_common import LIMIT, NP, PRECS, RTOL, TORCH, _bits, _host_product

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu


def poisson(w, h, dtype):
    """the 5-point Laplacian of a w x h grid, -1 off the diagonal, with the row-varying diagonal of C.convection_diffusion: symmetric
    positive definite, and no two rows alike"""
    off, col, val = C.convection_diffusion(w, h, np.float64)
    val = np.where(col == C.rows_of(off), val, -1.0)
    return off, col, val.astype(dtype)


def permuted(matrix, order):
    """P A P^T for order: new index -> old vertex"""
    off, col, val = matrix
    new = np.argsort(np.asarray(order))
    return C._csr(len(off) - 1, new[C.rows_of(off)], new[col], val, val.dtype)


@functools.lru_cache(maxsize=None)
def _matrix(kind, w, h, prec, red_black=False):
    m = (C.convection_diffusion if kind == "ilu" else poisson)(w, h, NP[prec])
    return permuted(m, fill_model.red_black(w, h)) if red_black else m


@functools.lru_cache(maxsize=None)
def _host_factor(kind, w, h, prec, red_black, p):
    """the model's filled pattern, A's values scattered into it, and the model's factor of them: (off, col, factor, pivot)"""
    off, col, val = _matrix(kind, w, h, prec, red_black)
    foff, fcol, lev, src = fill_model.fill(off, col, p)
    filled = fill_model.scatter(val, src)
    if kind == "ilu":
        factor, pivot = csrilu0_model.ilu0(foff, fcol, filled)
    else:
        factor, pivot = csric0_model.ic0(foff, fcol, filled, mirror=True)
    return foff, fcol, factor, pivot


def _host_precond(kind, w, h, prec, red_black, p):
    """M^-1 r as the two sweep models on the model's factor"""
    foff, fcol, factor, pivot = _host_factor(kind, w, h, prec, red_black, p)
    assert pivot == -1

    def apply(r):
        mid = csrsv_model.solve(foff, fcol, factor, r, lower=True, unit=kind == "ilu")
        return csrsv_model.solve(foff, fcol, factor, mid, lower=False, unit=False)
    return apply


def _rhs(n, prec):
    return C.rhs(n, NP[prec])


# ------------------------------------------------------------------------------------------------------------ CPU
def test_red_black_order_fills_the_black_block():
    off, col, _ = _matrix("ic", 12, 12, "f64", True)
    assert np.array_equal(off, fill_model.grid2d(12, order=fill_model.red_black(12))[0])
    assert [len(fill_model.fill(off, col, p)[1]) for p in (0, 1, 2)] == [672, 1154, 1154]
    dense = np.zeros((144, 144))
    dense[C.rows_of(off), col] = _matrix("ic", 12, 12, "f64", True)[2]
    assert np.array_equal(dense, dense.T) and np.unique(np.diag(dense)).size == 144


def test_level_one_needs_fewer_iterations_on_the_host():
    """from the models alone (the host product, the sweep models on the model's factor), fp64, 24 x 24, natural order"""
    off, col, val = _matrix("ilu", 24, 24, "f64")
    b = _rhs(576, "f64")
    its = [bicgstab_model.bicgstab(_host_product(off, col, val), _host_precond("ilu", 24, 24, "f64", False, p), b, None, RTOL["f64"], 0.0, LIMIT)[1:3]
           for p in (0, 1)]
    print("bicgstab, ILU(0) / ILU(1):", its)
    assert its[0][0] == its[1][0] == bicgstab_model.CONVERGED and its[1][1] < its[0][1]
    off, col, val = _matrix("ic", 24, 24, "f64")
    its = [pcg_model.pcg(_host_product(off, col, val), _host_precond("ic", 24, 24, "f64", False, p), b, None, RTOL["f64"], 0.0, LIMIT)[1:3]
           for p in (0, 1)]
    print("pcg, IC(0) / IC(1):", its)
    assert its[0][0] == its[1][0] == pcg_model.CONVERGED and its[1][1] < its[0][1]


# ------------------------------------------------------------------------------------------------------------ GPU: the factor
def _device(matrix):
    return tuple(torch.from_numpy(a).cuda() for a in matrix)


def _make(kind, d_off, d_col, p):
    return (M.Iluk if kind == "ilu" else M.Ick)(d_off, d_col, p)


@gpu
@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("red_black", [False, True], ids=["natural", "red-black"])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind", ["ilu", "ic"])
def test_the_factor_on_the_filled_pattern_on_the_bits(kind, prec, red_black, p):
    d_off, d_col, d_val = _device(_matrix(kind, 12, 12, prec, red_black))
    foff, fcol, want, pivot = _host_factor(kind, 12, 12, prec, red_black, p)
    f = _make(kind, d_off, d_col, p)
    try:
        assert int(f.factor(d_val).item()) == pivot == -1
        assert np.array_equal(f.row_offsets.cpu().numpy(), foff) and np.array_equal(f.column_indices.cpu().numpy(), fcol)
        assert (f.level, f.source_nnz, f.nnz, f.fill.nnz_filled) == (p, 672, len(fcol), len(fcol))
        got = (f.lu_values if kind == "ilu" else f.l_values).cpu().numpy()
        assert got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want))
        # again on other values of the same pattern: the kept filled array is reused
        other = (d_val * 1.5).contiguous()
        assert int(f.factor(other).item()) == -1
        off, col, val = _matrix(kind, 12, 12, prec, red_black)
        filled = fill_model.scatter(other.cpu().numpy(), fill_model.fill(off, col, p)[3])
        again = csrilu0_model.ilu0(foff, fcol, filled)[0] if kind == "ilu" else csric0_model.ic0(foff, fcol, filled, mirror=True)[0]
        assert np.array_equal(_bits((f.lu_values if kind == "ilu" else f.l_values).cpu().numpy()), _bits(again))
        for bad in (d_val[:-1], f._filled, d_val.cpu()):                           # A's values are asked for, not the filled ones
            with pytest.raises(M.MspmvError):
                f.factor(bad)
    finally:
        f.close()
    with pytest.raises(M.MspmvError, match="closed"):
        f.factor(d_val)


@gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind", ["ilu", "ic"])
def test_level_zero_is_the_factor_on_the_own_pattern(kind, prec):
    d_off, d_col, d_val = _device(_matrix(kind, 12, 12, prec))
    f, f0 = _make(kind, d_off, d_col, 0), (M.Ilu0 if kind == "ilu" else M.Ic0)(d_off, d_col)
    try:
        assert torch.equal(f.factor(d_val), f0.factor(d_val))
        assert torch.equal(f.row_offsets, d_off) and torch.equal(f.column_indices, d_col)
        assert torch.equal(f._factor.view(torch.int32 if prec == "f32" else torch.int64), f0._factor.view(torch.int32 if prec == "f32" else torch.int64))
        r = torch.from_numpy(_rhs(144, prec)).cuda()
        assert torch.equal(f.solve(r), f0.solve(r))
    finally:
        f.close(); f0.close()


@gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind", ["ilu", "ic"])
def test_the_sweeps_on_the_filled_factor(kind, prec):
    d_off, d_col, d_val = _device(_matrix(kind, 12, 12, prec, True))
    apply = _host_precond(kind, 12, 12, prec, True, 1)
    R = np.random.default_rng(9).uniform(-1, 1, (144, 3)).astype(NP[prec])
    f = _make(kind, d_off, d_col, 1)
    try:
        f.factor(d_val)
        X = f.solve_many(torch.from_numpy(R).cuda()).cpu().numpy()
        for j in range(3):
            want = apply(R[:, j].copy())
            got = f.solve(torch.from_numpy(R[:, j].copy()).cuda()).cpu().numpy()
            assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(X[:, j].copy()), _bits(want))
    finally:
        f.close()


# ------------------------------------------------------------------------------------------------------------ GPU: the solvers
def _same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and bool(np.all((_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))))


@gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("solver", ["bicgstab", "gmres", "pcg"])
def test_the_solvers_take_the_filled_factor(solver, prec):
    kind = "ic" if solver == "pcg" else "ilu"
    off, col, val = _matrix(kind, 24, 24, prec)
    b = _rhs(576, prec)
    d_off, d_col, d_val = _device((off, col, val))
    d_b = torch.from_numpy(b).cuda()
    apply_A = lambda v: M.csrmv(d_val, d_off, d_col, torch.from_numpy(v).cuda(), num_cols=576).cpu().numpy()
    apply_M = _host_precond(kind, 24, 24, prec, False, 1)
    f = _make(kind, d_off, d_col, 1)
    assert int(f.factor(d_val).item()) == -1 and f.nnz > len(col)
    if solver == "bicgstab":
        want = bicgstab_model.bicgstab(apply_A, apply_M, b, None, RTOL[prec], 0.0, LIMIT)
        s = M.Bicgstab(d_off, d_col, TORCH[prec], preconditioner=f)
    elif solver == "gmres":
        want = gmres_model.gmres(apply_A, apply_M, b, None, RTOL[prec], 0.0, 30, LIMIT)
        s = M.Gmres(d_off, d_col, TORCH[prec], preconditioner=f, restart=30)
    else:
        want = pcg_model.pcg(apply_A, apply_M, b, None, RTOL[prec], 0.0, LIMIT) + (None,)
        s = M.Pcg(d_off, d_col, TORCH[prec], preconditioner=f)
    try:
        x = s.solve(d_val, d_b, rtol=RTOL[prec], max_iterations=LIMIT, history=True)
        state = s.state
        print(f"{solver} {prec} with level 1: {state['iterations']} iterations, {state['status']}")
        assert want[1] == "CONVERGED" and 0 < want[2] < LIMIT
        assert (state["status"], state["iterations"], state.get("exit")) == (want[1], want[2], want[4])
        assert _same(s.history.cpu().numpy()[:want[2] + 1], want[3])
        assert _same(x.cpu().numpy(), want[0])
    finally:
        s.close(); f.close()


def _by_hand(solver, d_val, d_off, d_col, d_b, prec, reorder, p):
    """the one-shot call spelt out: multicolor_reorder, Ick / Iluk (Ic0 / Ilu0 at level 0), the solver class"""
    coloring = None
    val, off, col, rhs = d_val, d_off, d_col, d_b
    if reorder:
        coloring, a = M.multicolor_reorder(d_val, d_off, d_col)
        val, off, col, rhs = a.values, a.row_offsets, a.column_indices, coloring.permute_vector(d_b)
    if solver == "pcg":
        f = M.Ick(off, col, p) if p else M.Ic0(off, col)
    else:
        f = M.Iluk(off, col, p) if p else M.Ilu0(off, col)
    f.factor(val)
    s = {"pcg": M.Pcg, "bicgstab": M.Bicgstab, "gmres": M.Gmres}[solver](off, col, TORCH[prec], preconditioner=f)
    x = s.solve(val, rhs, rtol=RTOL[prec], max_iterations=LIMIT)
    if coloring is not None:
        x = coloring.permute_vector(x, back=True)
    state = s.state
    for held in (s, f, coloring):
        if held is not None:
            held.close()
    return x, state


@gpu
@pytest.mark.parametrize("reorder", [False, True], ids=["natural", "multicolour"])
@pytest.mark.parametrize("solver", ["pcg", "bicgstab", "gmres"])
def test_the_one_shot_calls_with_a_fill_level(solver, reorder):
    prec = "f64"
    d_off, d_col, d_val = _device(_matrix("ic" if solver == "pcg" else "ilu", 24, 24, prec))
    d_b = torch.from_numpy(_rhs(576, prec)).cuda()
    call = getattr(M, solver)
    iterations = {}
    for p in (0, 1):
        x, state = call(d_val, d_off, d_col, d_b, reorder=reorder, rtol=RTOL[prec], max_iterations=LIMIT, return_state=True, fill_level=p)
        want, want_state = _by_hand(solver, d_val, d_off, d_col, d_b, prec, reorder, p)
        assert state["status"] == "CONVERGED" and (state["status"], state["iterations"]) == (want_state["status"], want_state["iterations"])
        assert torch.equal(x.view(torch.int64), want.view(torch.int64))
        iterations[p] = state["iterations"]
    print(f"{solver} one-shot, {'multicolour' if reorder else 'natural'} order: {iterations[0]} iterations at level 0, {iterations[1]} at level 1")
    today = call(d_val, d_off, d_col, d_b, reorder=reorder, rtol=RTOL[prec], max_iterations=LIMIT)      # the default is level 0
    assert torch.equal(today.view(torch.int64), call(d_val, d_off, d_col, d_b, reorder=reorder, rtol=RTOL[prec], max_iterations=LIMIT,
                                                     fill_level=0).view(torch.int64))
    with pytest.raises(M.MspmvError):
        call(d_val, d_off, d_col, d_b, fill_level=-1)
    with pytest.raises(M.MspmvError):
        call(d_val, d_off, d_col, d_b, fill_level=33)
