"""What the conjugate gradient tests share (tests/test_pcg.py, tests/test_pcg_shapes.py): the precisions, the tolerances and the host
helpers.  Nothing here calls the library."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

NP = {"f32": np.float32, "f64": np.float64}
TORCH = {"f32": torch.float32, "f64": torch.float64}
PRECS = ["f32", "f64"]
RTOL = {"f32": 1e-5, "f64": 1e-10}
RESIDUAL = {"f32": 1e-4, "f64": 1e-8}          # the true residual |b - A x| <= this |b|
LIMIT = 400


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def _true_residual(off, col, val, x, b):
    """|b - A x| / |b| in fp64 on the host"""
    r_of = np.repeat(np.arange(len(off) - 1), np.diff(off))
    ax = np.zeros(len(off) - 1)
    np.add.at(ax, r_of, val.astype(np.float64) * x.astype(np.float64)[col])
    return float(np.linalg.norm(b.astype(np.float64) - ax)) / float(np.linalg.norm(b.astype(np.float64)))


def _host_product(off, col, val):
    """A p on the host, every product and every add rounded in the value type"""
    r_of = np.repeat(np.arange(len(off) - 1), np.diff(off))

    def apply(p):
        y = np.zeros(len(off) - 1, val.dtype)
        np.add.at(y, r_of, val * p[col])
        return y
    return apply
