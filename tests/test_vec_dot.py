"""mspmv_vec_dot_* (merge_spmv_amd.vec_dot): the deterministic dot product, compared ON THE BITS with tests/pcg_model.py, the numpy
restatement of the tree that include/mspmv.h defines.  The CPU part checks the model against a plain loop over the stated tree and
against math.fsum, and the refusals that need no device."""
import ctypes
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import merge_spmv_amd as M
from conftest import ROOT
import pcg_model as model

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

NEW = ["mspmv_vec_dot_f32", "mspmv_vec_dot_f64"]
NP = {"f32": np.float32, "f64": np.float64}
PRECS = ["f32", "f64"]
# every boundary of the tree: the four summands of a lane, the wave (64 lanes = 256 summands), the chunk (1024), the one-level fold
# (1024 partials = 2^20 summands) and several chunks of partials in the two-level fold
SIZES = [0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2049, 256 * 1024 - 1, 256 * 1024 + 1, 2 ** 20 - 1, 2 ** 20,
         2 ** 20 + 1, 3 * 2 ** 20 + 5]
FEW = [0, 1, 1025, 2 ** 20, 2 ** 20 + 1, 3 * 2 ** 20 + 5]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def _same(got, want):
    """equal bits; a NaN equals any NaN (its sign and payload are not defined)"""
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and bool(np.all((_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))))


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_vec_dot_symbols_are_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mspmv.h")).read(), flags=re.S)
    for kind in ("product", "dev"):
        out = subprocess.run(["nm", "-D", "--defined-only", M.library_path(kind)], capture_output=True, text=True, check=True).stdout
        for name in NEW:
            assert re.search(r"\b%s\s*\(" % name, text) and f" T {name}\n" in out, (kind, name)


@pytest.mark.parametrize("prec", PRECS)
def test_the_model_is_the_stated_tree(prec):
    rng = np.random.default_rng(1)
    for n in (0, 1, 3, 4, 5, 255, 257, 1023, 1024, 1025, 2049, 3000):
        v = rng.standard_normal(n).astype(NP[prec])
        got, want = model.reduce(v), model.reduce_loop(v)
        assert type(got) is NP[prec] and _same(got, NP[prec](want)), n
    # the sign of a zero: the fill is +0.0 and the last step is always made
    assert _bits(model.reduce(np.full(1024, -0.0, NP[prec])))[()] == 0
    assert _bits(model.reduce(np.zeros(0, NP[prec])))[()] == 0
    assert _bits(model.reduce(np.full(2 ** 20, -0.0, NP[prec])))[()] != 0           # every level full: -0.0


@pytest.mark.parametrize("prec", PRECS)
def test_the_model_against_fsum(prec):
    rng = np.random.default_rng(2)
    eps = float(np.finfo(NP[prec]).eps)
    for n in (1, 7, 1000, 1025, 5000, 70000):
        v = rng.standard_normal(n).astype(NP[prec])
        exact = math.fsum(float(e) for e in v)
        assert abs(float(model.reduce(v)) - exact) <= n * eps * math.fsum(abs(float(e)) for e in v), n


def test_refusals_and_the_size_query_need_no_device():
    lib = M.load_library()
    size = ctypes.c_size_t(0)
    for fn, vb in ((lib.mspmv_vec_dot_f32, 4), (lib.mspmv_vec_dot_f64, 8)):
        assert fn(None, None, None, None, 10, None, None, 0) == 1                   # NULL size pointer
        assert fn(None, ctypes.byref(size), None, None, -1, None, None, 0) == 1     # n < 0
        assert fn(None, ctypes.byref(size), None, None, 2 ** 30 + 1, None, None, 0) == 1
        for n, partials in ((0, 1), (1, 1), (1024, 1), (1025, 2), (2 ** 20 + 1, 1025), (2 ** 30, 2 ** 20)):
            assert fn(None, ctypes.byref(size), None, None, n, None, None, 0) == 0
            assert size.value == (partials * vb + 15) // 16 * 16, n
        small = ctypes.c_size_t(15)
        assert fn(ctypes.c_void_p(4096), ctypes.byref(small), None, None, 10, None, None, 0) == 1        # too small
        big = ctypes.c_size_t(4096)
        assert fn(ctypes.c_void_p(4096 + 8), ctypes.byref(big), None, None, 10, None, None, 0) == 1      # misaligned temp
        assert fn(ctypes.c_void_p(4096), ctypes.byref(big), None, None, 10, None, None, 0) == 1          # NULL result and inputs


# ---------------------------------------------------------------------------------------------------------------- GPU
def _temp_bytes(n, prec):
    size = ctypes.c_size_t(0)
    fn = M.load_library().mspmv_vec_dot_f32 if prec == "f32" else M.load_library().mspmv_vec_dot_f64
    assert fn(None, ctypes.byref(size), None, None, n, None, None, 0) == 0
    return int(size.value)


def _dot(a, b, prec, fill=0xA5, extra=0, stream=None):
    """the call with guard words round the result and guard bytes round the temp storage (filled with `fill`, `extra` bytes larger than
    asked); the result as a numpy scalar"""
    need = _temp_bytes(a.numel(), prec) + extra
    buf = torch.full((64 + need + 64,), fill, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    res = torch.full((3,), 12345.0, dtype=a.dtype, device="cuda")
    out = M.vec_dot(a, b, out=res[1:2], temp=buf[64:64 + need], stream=stream)
    assert out.data_ptr() == res.data_ptr() + a.element_size()
    torch.cuda.synchronize()
    h = res.cpu().numpy()
    assert h[0] == 12345.0 and h[2] == 12345.0
    g = buf.cpu().numpy()
    assert (g[:64] == fill).all() and (g[64 + need:] == fill).all()
    return h[1]


@functools.lru_cache(maxsize=None)
def _draws(prec, n, kind):
    rng = np.random.default_rng(1000 + n % 9973 + len(kind))
    dt = NP[prec]
    a, b = rng.standard_normal(n).astype(dt), rng.standard_normal(n).astype(dt)
    if kind == "subnormal":                     # products of 2^-140 (fp32) / 2^-1060 (fp64): inside the subnormal range
        s = dt(2.0 ** (-70 if prec == "f32" else -530))
        a, b = a * s, b * s
    elif kind == "huge":                        # products of 2^120 / 2^1010: sums reach the top binades (and may overflow, like the model)
        s = dt(2.0 ** (60 if prec == "f32" else 505))
        a, b = a * s, b * s
    elif kind == "negzero":                     # every product is -0.0
        a, b = np.zeros(n, dt), -np.abs(b) - dt(1)
    elif kind == "inf":
        a[n // 3] = np.inf
    elif kind == "nan":
        a[n // 3] = np.inf
        b[(2 * n) // 3] = np.nan
    return a, b


def _check(prec, n, kind):
    a, b = _draws(prec, n, kind)
    want = model.dot(a, b)
    got = _dot(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), prec)
    assert _same(got, want), (prec, n, kind, got, want)
    return got


@gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("prec", PRECS)
def test_normal_draws_on_the_bits(prec, n):
    _check(prec, n, "normal")


@gpu
@pytest.mark.parametrize("kind", ["subnormal", "huge", "negzero", "inf", "nan"])
@pytest.mark.parametrize("prec", PRECS)
def test_the_ends_of_the_number_line(prec, kind):
    for n in FEW[1:] + [1024, 2049]:
        got = _check(prec, n, kind)
        if kind == "subnormal":
            a, b = _draws(prec, n, kind)
            assert 0 < np.abs(a * b).max() < np.finfo(NP[prec]).tiny            # (the products are subnormal, none flushed)
            assert n < 64 or got != 0
        if kind == "negzero":
            assert got == 0 and bool(np.signbit(got)) == (n == 2 ** 20)         # -0.0 only where no step of the tree met a fill
        if kind == "nan":
            assert np.isnan(got)


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_alignment_aliasing_and_stale_temp_do_not_matter(prec):
    for n in FEW[1:] + [1023, 2047]:
        a, b = _draws(prec, n, "normal")
        want = model.dot(a, b)
        # one element behind a 16-byte boundary: a alone, b alone, both
        da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        ua, ub = torch.zeros(n + 1, dtype=da.dtype, device="cuda"), torch.zeros(n + 1, dtype=da.dtype, device="cuda")
        ua[1:].copy_(da); ub[1:].copy_(db)
        assert ua[1:].data_ptr() % 16 == da.element_size()
        for x, y in ((ua[1:], db), (da, ub[1:]), (ua[1:], ub[1:])):
            assert _same(_dot(x, y, prec), want), n
        # the squared norm: the same array twice
        assert _same(_dot(da, da, prec), model.dot(a, a)) and _same(_dot(ua[1:], ua[1:], prec), model.dot(a, a)), n
        # two garbage fills of a temp storage of two sizes
        assert _same(_dot(da, db, prec, fill=0xFF), want) and _same(_dot(da, db, prec, fill=0x7F, extra=4096), want), n


@gpu
@pytest.mark.parametrize("prec", PRECS)
def test_side_stream_and_graph_replay(prec):
    n = 3 * 2 ** 20 + 5
    a, b = _draws(prec, n, "normal")
    c, _ = _draws(prec, n, "huge")
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        assert _same(_dot(da, db, prec, stream=side), model.dot(a, b))
    temp = torch.empty(_temp_bytes(n, prec), dtype=torch.uint8, device="cuda")
    out = torch.zeros(1, dtype=da.dtype, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        M.vec_dot(da, db, out=out, temp=temp)
    for vec, want in ((a, model.dot(a, b)), (c, model.dot(c, b))):
        da.copy_(torch.from_numpy(vec))
        out.fill_(7)
        temp.fill_(0x33)
        graph.replay()
        torch.cuda.synchronize()
        assert _same(out.cpu().numpy()[0], want)
