"""The right-preconditioned restarted GMRES(m) of include/mspmv_gmres.h (mspmv_gmres_*), restated in numpy, line for line.  Calls
nothing of the library: the operators A and M^-1 are passed in.  Every dot is pcg_model.dot, the deterministic reduction R; every
other operation is one numpy operation on arrays or scalars of the value type, so every result is rounded on its own; every root is
np.sqrt (correctly rounded)."""
import numpy as np

from pcg_model import BREAKDOWN, CONVERGED, RUNNING, dot, reduce_loop

EXITS = (None, "start", "rr", "beta", "d")        # mspmv_gmres_state_t.exit_test 0 .. 4


def gmres(apply_A, apply_M, b, x0, rtol, atol, restart, max_iterations, info=None):
    """(x, status, iterations, history, exit): history[0 .. iterations] as an array of b's dtype (true residuals where a cycle closed,
    the rotations' estimates between); exit is one of EXITS, the test that ended the solve (None: the slots of max_iterations are used
    up).  apply_A(p) -> A p, apply_M(r) -> M^-1 r, both on arrays of b's dtype; x0 None: x = +0, r = b.  info: a dict that receives
    rr, bb, stop2, beta (of b's dtype), slots, cycles, exit and `missed`: the number of cycles that the estimate closed and whose
    true residual did not converge."""
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
        status, iterations, slots, cycles, missed, left, beta = RUNNING, 0, 0, 0, 0, None, t(0)
        if rr <= stop2 and rr < np.inf:                              # (an infinite residual never counts as converged)
            status, left = CONVERGED, "start"
        while status == RUNNING and slots < max_iterations:
            beta = np.sqrt(rr)
            if not (beta > 0 and beta < np.inf):
                status, left = BREAKDOWN, "beta"
                break
            V = [r / beta]
            g = [beta]
            width = min(restart, max_iterations - slots)
            slots += width
            cycles += 1
            cols, pending, by_estimate = 0, False, False
            c, s, R = [], [], []                                     # R[j]: column j of the triangle, j + 1 entries
            for j in range(width):
                k = iterations + 1
                w = apply_A(apply_M(V[j]))
                h1 = [dot(V[i], w) for i in range(j + 1)]
                for i in range(j + 1):
                    w = w - h1[i] * V[i]
                h2 = [dot(V[i], w) for i in range(j + 1)]
                for i in range(j + 1):
                    w = w - h2[i] * V[i]
                h = [h1[i] + h2[i] for i in range(j + 1)]
                hn = np.sqrt(dot(w, w))
                for i in range(j):
                    tt = t(c[i] * h[i]) + t(s[i] * h[i + 1])
                    h[i + 1] = t(c[i] * h[i + 1]) - t(s[i] * h[i])
                    h[i] = tt
                d = np.sqrt(t(h[j] * h[j]) + t(hn * hn))
                if not (d > 0 and d < np.inf):
                    pending = True                                   # the column is dropped
                    break
                c.append(h[j] / d)
                s.append(hn / d)
                R.append(h[:j] + [d])
                g.append(t(-s[j]) * g[j])
                g[j] = c[j] * g[j]
                gg = g[j + 1] * g[j + 1]
                history.append(gg)
                iterations, cols = k, j + 1
                if gg <= stop2 or gg != gg or not hn > 0 or j == width - 1:
                    by_estimate = bool(gg <= stop2)
                    break
                V.append(w / hn)
            if cols > 0:
                y = [None] * cols
                for i in range(cols - 1, -1, -1):
                    acc = g[i]
                    for l in range(i + 1, cols):
                        acc = acc - t(R[l][i] * y[l])
                    y[i] = acc / R[i][i]
                u = y[0] * V[0]
                for i in range(1, cols):
                    u = u + y[i] * V[i]
                x = x + apply_M(u)
                r = b - apply_A(x)
                rr = dot(r, r)
                history[iterations] = rr                             # the TRUE residual
            if pending:
                status, left = BREAKDOWN, "d"
            elif rr <= stop2 and rr < np.inf:
                status, left = CONVERGED, "rr"
            elif by_estimate:
                missed += 1
        if info is not None:
            info.update(bb=bb, stop2=stop2, rr=rr, beta=beta, slots=slots, cycles=cycles, missed=missed, exit=left)
        return x, status, iterations, np.array(history, dtype=b.dtype), left


def gmres_loop(a, b, rtol, atol, restart, max_iterations):
    """The same arithmetic as plain Python loops over scalars of b's dtype, for a dense matrix a and no preconditioner (slow; the
    model's own check): (x, status, iterations, history, exit, slots, cycles)."""
    t = b.dtype.type
    n = len(b)
    a = [[t(v) for v in row] for row in np.asarray(a)]
    b = [t(v) for v in b]

    def product(p):
        out = []
        for row in a:
            acc = t(0)
            for e in range(n):
                acc = acc + row[e] * p[e]
            out.append(acc)
        return out

    def rdot(p, q):
        return reduce_loop([p[e] * q[e] for e in range(n)])

    with np.errstate(all="ignore"):
        x, r = [t(0)] * n, list(b)
        bb = rdot(b, b)
        rt, at = t(rtol), t(atol)
        s0, a2 = t(rt * rt) * bb, at * at
        stop2 = s0 if s0 > a2 else a2
        rr = rdot(r, r)
        history = [rr]
        status, iterations, slots, cycles, left = RUNNING, 0, 0, 0, None
        if rr <= stop2 and rr < np.inf:
            status, left = CONVERGED, "start"
        while status == RUNNING and slots < max_iterations:
            beta = np.sqrt(rr)
            if not (beta > 0 and beta < np.inf):
                status, left = BREAKDOWN, "beta"
                break
            V, g = [[r[e] / beta for e in range(n)]], [beta]
            width = min(restart, max_iterations - slots)
            slots, cycles = slots + width, cycles + 1
            cols, pending = 0, False
            c, s, R = [], [], {}
            for j in range(width):
                w = product(V[j])
                h = [t(0)] * (j + 1)
                for _ in range(2):
                    hp = [rdot(V[i], w) for i in range(j + 1)]
                    for i in range(j + 1):
                        for e in range(n):
                            w[e] = w[e] - hp[i] * V[i][e]
                    h = hp if _ == 0 else [h[i] + hp[i] for i in range(j + 1)]
                hn = np.sqrt(rdot(w, w))
                for i in range(j):
                    tt = c[i] * h[i] + s[i] * h[i + 1]
                    h[i + 1] = c[i] * h[i + 1] - s[i] * h[i]
                    h[i] = tt
                d = np.sqrt(h[j] * h[j] + hn * hn)
                if not (d > 0 and d < np.inf):
                    pending = True
                    break
                c.append(h[j] / d); s.append(hn / d)
                for i in range(j):
                    R[i, j] = h[i]
                R[j, j] = d
                g.append(-s[j] * g[j])
                g[j] = c[j] * g[j]
                gg = g[j + 1] * g[j + 1]
                history.append(gg)
                iterations, cols = iterations + 1, j + 1
                if gg <= stop2 or gg != gg or not hn > 0 or j == width - 1:
                    break
                V.append([w[e] / hn for e in range(n)])
            if cols > 0:
                y = [None] * cols
                for i in range(cols - 1, -1, -1):
                    acc = g[i]
                    for l in range(i + 1, cols):
                        acc = acc - R[i, l] * y[l]
                    y[i] = acc / R[i, i]
                for e in range(n):
                    u = y[0] * V[0][e]
                    for i in range(1, cols):
                        u = u + y[i] * V[i][e]
                    x[e] = x[e] + u
                q = product(x)
                r = [b[e] - q[e] for e in range(n)]
                rr = rdot(r, r)
                history[iterations] = rr
            if pending:
                status, left = BREAKDOWN, "d"
            elif rr <= stop2 and rr < np.inf:
                status, left = CONVERGED, "rr"
        return np.array(x, dtype=t), status, iterations, np.array(history, dtype=t), left, slots, cycles
