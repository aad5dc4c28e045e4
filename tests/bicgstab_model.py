"""The right-preconditioned BiCGStab of include/mspmv_krylov.h (mspmv_bicgstab_*), restated in numpy.  Calls nothing of the library: the
operators A and M^-1 are passed in.  Every dot is pcg_model.dot, the deterministic reduction R; every other operation is one numpy
operation on arrays or scalars of the value type, so every result is rounded on its own."""
import numpy as np

from pcg_model import BREAKDOWN, CONVERGED, RUNNING, dot

EXITS = (None, "start", "half", "rr", "rv", "tt", "rr-nan", "omega", "rho")        # mspmv_bicgstab_state_t.exit_test 0 .. 8


def bicgstab(apply_A, apply_M, b, x0, rtol, atol, max_iterations, info=None):
    """(x, status, iterations, history, exit): history[0 .. iterations] as an array of b's dtype; exit is one of EXITS, the test that
    ended the solve (None: max_iterations).  apply_A(p) -> A p, apply_M(r) -> M^-1 r, both on arrays of b's dtype; x0 None: x = +0,
    r = b.  info: a dict that receives the scalars as the solve leaves them (rr, bb, stop2, rho, alpha, omega, of b's dtype)."""
    t = b.dtype.type
    with np.errstate(all="ignore"):
        if x0 is None:
            x, r = np.zeros_like(b), b.copy()
        else:
            x = x0.copy()
            r = b - apply_A(x)
        bb = dot(b, b)
        rt, at = t(rtol), t(atol)
        s0, a2 = t(rt * rt) * bb, at * at
        stop2 = s0 if s0 > a2 else a2
        rr = dot(r, r)
        history = [rr]
        status, iterations, left = RUNNING, 0, None
        rho, alpha, omega = rr, t(0), t(0)
        if rr <= stop2 and rr < np.inf:                              # (an infinite residual never counts as converged)
            status, left = CONVERGED, "start"
        rh, p = r.copy(), r.copy()
        for k in range(1, max_iterations + 1 if status == RUNNING else 0):
            ph = apply_M(p)
            v = apply_A(ph)
            rv = dot(rh, v)
            if not abs(rv) > 0:
                status, left = BREAKDOWN, "rv"
                break
            alpha = rho / rv
            x = x + alpha * ph
            s = r - alpha * v
            ss = dot(s, s)
            if ss <= stop2 and ss < np.inf:
                rr, iterations, status, left = ss, k, CONVERGED, "half"
                history.append(ss)
                break
            sh = apply_M(s)
            tv = apply_A(sh)
            ts, tt = dot(tv, s), dot(tv, tv)
            if not tt > 0:
                rr, iterations, status, left = ss, k, BREAKDOWN, "tt"          # (x keeps the half step: s is its true residual)
                history.append(ss)
                break
            omega = ts / tt
            x = x + omega * sh
            r = s - omega * tv
            rr, rho2 = dot(r, r), dot(rh, r)
            history.append(rr)
            iterations = k
            if rr <= stop2 and rr < np.inf:
                status, left = CONVERGED, "rr"
            elif rr != rr:
                status, left = BREAKDOWN, "rr-nan"
            elif not abs(omega) > 0:
                status, left = BREAKDOWN, "omega"
            elif not abs(rho2) > 0:
                status, left = BREAKDOWN, "rho"
            if status != RUNNING:
                break
            beta = t(rho2 / rho) * t(alpha / omega)
            rho = rho2
            p = r + beta * (p - omega * v)
        if info is not None:
            info.update(bb=bb, stop2=stop2, rr=rr, rho=rho, alpha=alpha, omega=omega, exit=left)
        return x, status, iterations, np.array(history, dtype=b.dtype), left
