"""The one allocation of Pcg, Bicgstab and Gmres: state["device_bytes"] against the closed form of each solver's carve (the solvers'
own arrays in csrc/mspmv_pcg.hip, mspmv_bicgstab.hip, mspmv_gmres.hip; the operator's in csrc/mspmv_krylov_op.hpp) -- the 256-byte
state block, the vectors of the kind (each rounded up to 256 bytes), the positions of the diagonal, the partials, for GMRES the basis,
the rows of partials and the small block, and the prepared product.  The form was written from the carve of the commit before the
operator layer was shared and held on a build of it."""
import pytest

torch = pytest.importorskip("torch")

import merge_spmv_amd as M
import bicgstab_common as C
from pcg_common import NP, PRECS, TORCH

gpu = pytest.mark.gpu

SYSTEMS = {"grid-24x24": lambda dtype: C.convection_diffusion(24, 24, dtype),
           "band-1025": lambda dtype: C.banded(1025, dtype)}                     # 1025 rows: one row past a single chunk of partials
RESTARTS = (1, 3)


def _align256(v):
    return (v + 255) // 256 * 256


def _expected(solver, kind, rows, nnz, vb, restart=None):
    vec, m = _align256(rows * vb), max(1, (rows + 1023) // 1024)
    hat = vec if kind != "none" else 0                                          # z (Pcg) or the hat vector: none of its own without M
    precond = {"none": 0, "jacobi": vec + _align256(rows * 4), "factor": vec}[kind]              # d and dpos, or mid
    product = _align256(M.launch_info(rows, nnz, vb)["temp_bytes"])
    part = _align256(m * vb)
    if solver == "pcg":                                                         # q, p, r; three rows of partials
        return 256 + 3 * vec + hat + precond + 3 * part + product
    if solver == "bicgstab":                                                    # p, v, r, rh, t; two rows of partials
        return 256 + 5 * vec + hat + precond + 2 * part + product
    pstride = (m * vb + 15) // 16 * 16 // vb                                    # rows of partials are 16-byte aligned
    return (256 + (restart + 1) * vec + vec + hat + precond + _align256((restart + 1) * pstride * vb)
            + _align256((restart * restart + 7 * restart + 1) * vb) + product)


@gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", sorted(SYSTEMS))
def test_device_bytes_is_the_closed_form_of_the_carve(name, prec):
    off, col, val = SYSTEMS[name](NP[prec])
    rows, nnz, vb = len(off) - 1, len(col), val.dtype.itemsize
    d_off, d_col, d_val = (torch.from_numpy(a).cuda() for a in (off, col, val))
    ilu = M.Ilu0(d_off, d_col)
    ilu.factor(d_val)
    seen = 0
    for kind, precond in (("none", None), ("jacobi", "jacobi"), ("factor", ilu)):
        makers = [("pcg", None, lambda: M.Pcg(d_off, d_col, TORCH[prec], preconditioner=precond)),
                  ("bicgstab", None, lambda: M.Bicgstab(d_off, d_col, TORCH[prec], preconditioner=precond))]
        makers += [("gmres", r, lambda r=r: M.Gmres(d_off, d_col, TORCH[prec], preconditioner=precond, restart=r)) for r in RESTARTS]
        for solver, restart, make in makers:
            s = make()
            got, want = s.state["device_bytes"], _expected(solver, kind, rows, nnz, vb, restart)
            s.close()
            print(f"{name} {prec} {solver} {kind} restart {restart}: device_bytes {got}, closed form {want}")
            assert got == want, (solver, kind, restart)
            seen += 1
    ilu.close()
    assert seen == 3 * (2 + len(RESTARTS))
