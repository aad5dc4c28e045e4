"""The deterministic reduction R and the conjugate gradients of include/mspmv.h (mspmv_vec_dot_*, mspmv_pcg_*), restated in numpy.
Calls nothing of the library: the operators A and M^-1 are passed in.  Every operation is one numpy operation on arrays or scalars of
the value type, so every result is rounded on its own."""
import numpy as np

CHUNK = 1024
RUNNING, CONVERGED, BREAKDOWN = "RUNNING", "CONVERGED", "BREAKDOWN"


def _chunks(c):
    """chunk(.) of every row of the padded level c (a multiple of 1024 long): four consecutive summands left to right, then pairwise,
    neighbours first"""
    q = c.reshape(-1, 256, 4)
    q = ((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3]
    while q.shape[1] > 1:
        q = q[:, 0::2] + q[:, 1::2]
    return q[:, 0]


def _level(v):
    """v cut into chunks of 1024, the last one filled up with +0.0 (an empty v: one chunk of zeros); the chunk sums"""
    m = max(1, -(-v.size // CHUNK))
    c = np.zeros(m * CHUNK, dtype=v.dtype)
    c[:v.size] = v
    return _chunks(c)


def reduce(v):
    """R(v), a scalar of v's dtype"""
    v = np.ascontiguousarray(v)
    with np.errstate(all="ignore"):
        p = _level(v)
        if p.size > CHUNK:
            p = _level(p)
        return _level(p)[0]


def dot(a, b):
    """R(a o b): the products rounded on their own"""
    with np.errstate(all="ignore"):
        return reduce(a * b)


def reduce_loop(v):
    """R(v) as a plain Python loop over the stated tree (slow; the model's own check)"""
    t = type(v[0]) if len(v) else np.float64
    zero = t(0)

    def chunk(c):
        q = [((c[4 * i] + c[4 * i + 1]) + c[4 * i + 2]) + c[4 * i + 3] for i in range(256)]
        while len(q) > 1:
            q = [q[2 * i] + q[2 * i + 1] for i in range(len(q) // 2)]
        return q[0]

    def level(s):
        s = list(s)
        m = max(1, -(-len(s) // CHUNK))
        s += [zero] * (m * CHUNK - len(s))
        return [chunk(s[CHUNK * j:CHUNK * (j + 1)]) for j in range(m)]

    with np.errstate(all="ignore"):
        p = level(v)
        if len(p) > CHUNK:
            p = level(p)
        return level(p)[0]


def pcg(apply_A, apply_M, b, x0, rtol, atol, max_iterations, info=None):
    """(x, status, iterations, history): history[0 .. iterations] as an array of b's dtype.  apply_A(p) -> A p, apply_M(r) -> M^-1 r, both
    on arrays of b's dtype; x0 None: x = +0, r = b.  info: a dict that receives the scalars as the solve leaves them (bb, stop2, rr, rz
    and the last pq, of b's dtype; rz None if the solve ended before z was made, pq None before the first iteration) and
    `exit`, the test that ended it: "start" or "rr" (CONVERGED),
    "pq", "rr-nan" or "rz" (BREAKDOWN), None (max_iterations)."""
    t = b.dtype.type
    with np.errstate(all="ignore"):
        if x0 is None:
            x, r = np.zeros_like(b), b.copy()
        else:
            x = x0.copy()
            r = b - apply_A(x)
        bb = dot(b, b)
        rt, at = t(rtol), t(atol)
        s, a2 = t(rt * rt) * bb, at * at
        stop2 = s if s > a2 else a2
        rr = dot(r, r)
        history = [rr]
        status, iterations, rz, pq, left = RUNNING, 0, None, None, None
        if rr <= stop2 and rr < np.inf:                              # (an infinite residual never counts as converged)
            status, left = CONVERGED, "start"
        else:
            z = apply_M(r)
            rz = dot(r, z)
            p = z.copy()
        for k in range(1, max_iterations + 1 if status == RUNNING else 0):
            q = apply_A(p)
            pq = dot(p, q)
            if not pq > 0:
                status, left = BREAKDOWN, "pq"
                break
            alpha = rz / pq
            x = x + alpha * p
            r = r - alpha * q
            rr = dot(r, r)
            history.append(rr)
            iterations = k
            if rr <= stop2 and rr < np.inf:
                status, left = CONVERGED, "rr"
                break
            if rr != rr:
                status, left = BREAKDOWN, "rr-nan"
                break
            z = apply_M(r)
            rz2 = dot(r, z)
            if not rz2 > 0:
                status, left = BREAKDOWN, "rz"
                break
            beta = rz2 / rz
            rz = rz2
            p = z + beta * p
        if info is not None:
            info.update(bb=bb, stop2=stop2, rr=rr, rz=rz, pq=pq, exit=left)
        return x, status, iterations, np.array(history, dtype=b.dtype)
