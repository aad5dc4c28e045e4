"""Mixed-precision CsrMV (mspmv_csrmv_mixed_*, merge_spmv_amd.csrmv_mixed): the matrix values stored narrow -- fp32 values in an
fp64 product, bf16 values in an fp32 one --, x, y, alpha, beta and every sum in the compute type.

Widening is exact (every fp32 is an fp64, every bf16 an fp32), so the oracle is exact too: a mixed call returns, BIT FOR BIT,
what the wide call of the compute type returns for the widened values (include/mspmv.h says when: same alignment of the arrays,
the wide call neither a column-band candidate nor on its small-shape layout).  No tolerance of its own anywhere: where a bound
is checked it is the strict bound of tests/test_gpu_parity.py against the oracle on the widened matrix.

test_values_that_fill_the_stored_significand_equal_the_int64_model compares with the int64 model of tests/axpby_model.py on values
that use every bit of the stored type (odd integers up to 2^24 - 1 as fp32, up to 255 as bf16) and x, y0 as wide as the exactness
budget allows: an error the mixed and the wide call share, or a conversion through float behind the widening, shows there.

CPU tests: exports, the size query, what the Python face refuses.  GPU tests (-m gpu): everything else.  Measured on one MI355X:
the 474 GPU tests of this file take 10.4 s, the 459 before the wide cases 10.1 s."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import merge_spmv_amd as Mod
from oracle import oracle as O

torch = pytest.importorskip("torch")
import test_gpu_parity as T          # noqa: E402 - helpers of the wide suite: SHAPES, PATHS, CASES, random_csr, check_strict

SYMBOLS = ["mspmv_csrmv_mixed_f32_f64", "mspmv_csrmv_mixed_bf16_f32", "mspmv_csrmv_mixed_prepared_f32_f64", "mspmv_csrmv_mixed_prepared_bf16_f32"]
# pair -> (stored torch dtype, compute torch dtype, compute numpy dtype, compute bytes, stored bytes)
PAIRS = {"f32_f64": (torch.float32, torch.float64, np.float64, 8, 4), "bf16_f32": (torch.bfloat16, torch.float32, np.float32, 4, 2)}


def narrow(pair, a):
    """numpy array of the compute type -> the same numbers rounded to the stored type, as (stored tensor, widened numpy array)"""
    sdt, cdt, npdt, _, _ = PAIRS[pair]
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=npdt)).to(sdt)
    return t, t.to(cdt).numpy()


def narrow_exact(pair, a):
    """narrow() for values the stored type holds exactly, made from the bit patterns on the host (no conversion routine that might
    round or flush a subnormal, and -0.0 keeps its sign: bf16 -0.0 is 0x8000)"""
    sdt, cdt, npdt, _, _ = PAIRS[pair]
    a = np.ascontiguousarray(a, dtype=npdt)
    if pair == "bf16_f32":
        u = a.view(np.uint32)
        assert not (u & 0xFFFF).any(), "not a bf16"
        t = torch.from_numpy((u >> 16).astype(np.uint16).view(np.int16)).view(torch.bfloat16)
    else:
        n = a.astype(np.float32)
        assert np.array_equal(n.astype(np.float64).view(np.int64), a.view(np.int64)), "not an fp32"
        t = torch.from_numpy(n)
    return t, a


# ------------------------------------------------------------------------------------------------------------------ CPU

def test_narrow_exact_keeps_signed_zeros_and_subnormals():
    t, w = narrow_exact("bf16_f32", np.array([-0.0, 0.0, 2.0 ** -133, -2.0 ** -132, 1.0], np.float32))
    assert t.view(torch.int16).tolist() == [-0x8000, 0, 1, -0x8000 + 2, 0x3F80] and t.dtype == torch.bfloat16
    t, w = narrow_exact("f32_f64", np.array([-0.0, 0.0, 2.0 ** -149, -2.0 ** -148], np.float64))
    assert t.view(torch.int32).tolist() == [-2 ** 31, 0, 1, -2 ** 31 + 2]
    with pytest.raises(AssertionError):
        narrow_exact("bf16_f32", np.array([1.0 + 2.0 ** -10], np.float32))
    with pytest.raises(AssertionError):
        narrow_exact("f32_f64", np.array([2.0 ** -150], np.float64))


@pytest.mark.parametrize("kind", ["product", "dev"])
def test_the_four_entry_points_are_exported_and_declared(kind):
    lib = ctypes.CDLL(Mod.library_path(kind))
    header = open(os.path.join(ROOT, "include", "mspmv.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s), f"{s} missing from {Mod.library_path(kind)}"
        assert re.search(r"\bint\s+" + s + r"\s*\(", header), f"{s} not declared in mspmv.h"
    assert lib.mspmv_version() == 102           # no bump: found by symbol


@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("prepared", [False, True])
def test_size_query_two_phase_convention(pair, prepared):
    """the cases of tests/test_abi_exports.py::test_size_query_two_phase_convention"""
    lib = Mod.load_library()
    vb = PAIRS[pair][3]
    ct = ctypes.c_double if vb == 8 else ctypes.c_float
    fn = getattr(lib, ("mspmv_csrmv_mixed_prepared_" if prepared else "mspmv_csrmv_mixed_") + pair)
    call = lambda temp, size, ptr, rows, cols, nnz: fn(temp, ctypes.byref(size), ptr, ptr, ptr, ptr, ptr, rows, cols, nnz, ct(1.0), ct(0.0), None, 0)
    size = ctypes.c_size_t(0)
    if prepared:
        assert call(None, size, None, 1000, 1000, 50000) == 1          # a prepared call needs its temp storage
        size = ctypes.c_size_t(Mod.launch_info(1000, 50000, vb)["temp_bytes"])
    else:
        for rows, nnz in ((1000, 50000), (3_000_000, 12_000_000), (0, 0), (7, 0)):
            size = ctypes.c_size_t(0)
            assert call(None, size, None, rows, 1000, nnz) == 0
            assert size.value == Mod.launch_info(rows, nnz, vb)["temp_bytes"] > 0        # the COMPUTE type's layout, whatever the stored type
        assert call(None, size, None, 1000, 1000, 50000) == 0
    small = ctypes.c_size_t(size.value - 1)
    assert call(ctypes.c_void_p(256), small, None, 1000, 1000, 50000) == 1
    big = ctypes.c_size_t(size.value + 64)
    fake = ctypes.c_void_p(4096)
    for misaligned in (4096 + 1, 4096 + 4, 4096 + 8):
        assert call(ctypes.c_void_p(misaligned), big, fake, 1000, 1000, 50000) == 1
    if not prepared:
        assert call(None, size, None, -1, 5, 5) == 1
        assert call(None, size, None, 5, -1, 5) == 1
        assert call(None, size, None, 5, 5, -1) == 1
        assert call(None, size, None, 2**30, 5, 2**30 + 5) == 1
        assert call(None, size, None, 1000, 5, 2**31 - 1 - 65536 - 1000 + 1) == 1
        assert call(None, size, None, 1000, 5, 2**31 - 1 - 65536 - 1000) == 0
    assert fn(None, None, None, None, None, None, None, 10, 10, 10, ct(1.0), ct(0.0), None, 0) == 1


def test_python_face_refuses_before_anything_reaches_the_library():
    ro = torch.tensor([0, 1, 2], dtype=torch.int32); ci = torch.tensor([0, 1], dtype=torch.int32)
    bad_pairs = [(torch.float32, torch.float32), (torch.float64, torch.float64), (torch.float64, torch.float32), (torch.bfloat16, torch.float64),
                 (torch.float16, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.int32, torch.float32)]
    for vdt, xdt in bad_pairs:
        with pytest.raises(Mod.MspmvError, match="csrmv_mixed"):
            Mod.csrmv_mixed(torch.ones(2).to(vdt), ro, ci, torch.ones(2).to(xdt))
    # supported pairs, CPU tensors
    for pair in PAIRS:
        sdt, cdt = PAIRS[pair][:2]
        with pytest.raises(Mod.MspmvError, match="CUDA"):
            Mod.csrmv_mixed(torch.ones(2, dtype=sdt), ro, ci, torch.ones(2, dtype=cdt))
    with pytest.raises(Mod.MspmvError):
        Mod.csrmv_mixed(np.ones(2, np.float32), ro, ci, torch.ones(2, dtype=torch.float64))
    # csrmv itself keeps refusing mismatched dtypes
    with pytest.raises((Mod.MspmvError, TypeError)):
        Mod.csrmv(torch.ones(2, dtype=torch.float32), ro, ci, torch.ones(2, dtype=torch.float64))
    assert "csrmv_mixed" in Mod.__all__


# ------------------------------------------------------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: torch.cuda.is_available() is False")
    Mod.load_library()
    Mod.set_tuning(4); Mod.set_tuning(8)
    return Mod


def off_by_one(t):
    """the same data at an address one element past a 256-byte boundary: not 16-byte aligned, so the dword-per-lane tile_kernel runs"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    buf[1:].copy_(t)
    return buf[1:]


class Problem:
    """a CSR matrix whose values were drawn in the stored type (the widened matrix IS the matrix), on the device in both forms"""

    def __init__(self, pair, rows, cols, offsets, col, val, x, shift=False, exact=False):
        sdt, cdt, npdt, vb, _ = PAIRS[pair]
        self.pair, self.vb, self.cdt, self.rows, self.cols, self.nnz = pair, vb, cdt, int(rows), int(cols), int(len(col))
        v_narrow, v_wide = (narrow_exact if exact else narrow)(pair, val)
        self.csr = O.Csr(self.rows, self.cols, np.asarray(offsets, np.int32), np.asarray(col, np.int32), v_wide)
        self.x = np.asarray(x, npdt)
        place = off_by_one if shift else (lambda t: t)
        self.d_narrow, self.d_wide = place(v_narrow.cuda()), place(torch.from_numpy(v_wide).cuda())
        self.d_ro, self.d_ci = place(torch.from_numpy(self.csr.row_offsets).cuda()), place(torch.from_numpy(self.csr.column_indices).cuda())
        self.d_x = torch.from_numpy(self.x).cuda()

    def workspace(self, prepare=False):
        ws = Mod.CsrMVWorkspace(self.rows, self.nnz, self.cdt)      # exactly launch_info(rows, nnz, sizeof(compute)).temp_bytes
        assert ws.bytes == Mod.launch_info(self.rows, self.nnz, self.vb)["temp_bytes"]
        return ws.prepare(self.d_ro) if prepare else ws

    def y0(self, seed=5):
        return torch.from_numpy(np.random.default_rng(seed).uniform(-1, 1, self.rows).astype(PAIRS[self.pair][2])).cuda()

    def wide(self, ws, y=None, **kw):
        y = torch.full((self.rows,), float("nan"), dtype=self.cdt, device="cuda") if y is None else y.clone()
        if "alpha" not in kw:
            kw = dict(kw, alpha=1.0, beta=0.0)             # (the axpby entry point: what the mixed call is specified against)
        Mod.csrmv(self.d_wide, self.d_ro, self.d_ci, self.d_x, y=y, num_cols=self.cols, workspace=ws, **kw)
        return y

    def mixed(self, ws, y=None, **kw):
        y = torch.full((self.rows,), float("nan"), dtype=self.cdt, device="cuda") if y is None else y.clone()
        Mod.csrmv_mixed(self.d_narrow, self.d_ro, self.d_ci, self.d_x, y=y, num_cols=self.cols, workspace=ws, **kw)
        return y


def shape_problem(pair, shape, shift=False):
    rng = np.random.default_rng(sum(map(ord, shape)))
    rows, cols, lens = T.SHAPES[shape](rng)
    csr = T.random_csr(rng, rows, cols, np.asarray(lens, np.int64), PAIRS[pair][2])
    x = rng.uniform(-1, 1, size=cols)
    return Problem(pair, rows, cols, csr.row_offsets, csr.column_indices, csr.values, x, shift=shift)


def same_bits(a, b):
    # (torch.equal on the bit patterns: NaN-safe, and -0.0 is not +0.0)
    it = torch.int64 if a.dtype == torch.float64 else torch.int32
    return a.dtype == b.dtype and torch.equal(a.view(it), b.view(it))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(T.SHAPES))
@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("path", sorted(T.PATHS))
def test_bitwise_equal_to_the_wide_call_on_the_widened_values(G, shape, pair, path):
    """every shape x pair x dispatch path (forced through the development library's set_tuning(sizeof(compute), ...)): plain and
    alpha / beta, stateless and prepared, first call and call on hints, aligned arrays and arrays one element off"""
    vb = PAIRS[pair][3]
    atomic = path == "classic_atomic_fix"          # (the one path the existing suite exempts from bitwise reproducibility: the strict bound instead)
    try:
        Mod.set_tuning(vb, 0, 0, T.PATHS[path])
        for shift in (False, True):
            P = shape_problem(pair, shape, shift=shift)
            assert Mod.band_passes(P.rows, P.cols, P.nnz, vb) <= 1         # none of these sizes is a column-band candidate
            y0 = P.y0()
            for prepared in (False, True):
                ws_w, ws_m = P.workspace(prepared), P.workspace(prepared)
                for kw in ({}, {"alpha": -1.75, "beta": 0.375}):
                    for call in ("first", "on hints"):
                        yin = y0 if kw else None
                        yw, ym = P.wide(ws_w, yin, **kw), P.mixed(ws_m, yin, **kw)
                        torch.cuda.synchronize()
                        where = (shape, pair, path, shift, prepared, kw, call)
                        assert not torch.isnan(ym).any(), where
                        if atomic:
                            if not kw:
                                T.check_strict(Mod, P.csr, P.x, ym.cpu().numpy())
                        else:
                            assert same_bits(yw, ym), where
            if not shift:
                T.check_strict(Mod, P.csr, P.x, P.mixed(P.workspace()).cpu().numpy())
    finally:
        Mod.set_tuning(vb)


def mixed_e_values(pair, which, total):
    """e_values of axpby_model.scale_exponents for a mixed pair, from the STORED type's own range: "bottom_stored" puts one unit of
    the values at the stored type's smallest subnormal (2^-133 for bf16, 2^-149 for fp32); "bottom" and "top" split the total evenly
    between values and x, moved just far enough that the values (1 and 2 units) stay normal and finite in the stored type"""
    fi = torch.finfo(PAIRS[pair][0])
    emin = int(np.log2(fi.tiny))                                   # the smallest normal: 2^emin
    mant = int(round(-np.log2(fi.eps)))
    emax = int(np.floor(np.log2(fi.max)))
    if which == "bottom_stored":
        return emin - mant
    return min(max(total // 2, emin), emax - 2)


def test_mixed_e_values_follow_the_stored_type():
    assert [mixed_e_values("bf16_f32", w, t) for w, t in (("bottom", -148), ("bottom_stored", -148), ("top", 104))] == [-74, -133, 52]
    assert [mixed_e_values("f32_f64", w, t) for w, t in (("bottom", -1073), ("bottom_stored", -1073), ("top", 971))] == [-126, -149, 125]


@pytest.mark.gpu
@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("path", sorted(T.PATHS))
def test_zero_laden_and_scaled_values_equal_the_wide_call_and_the_model(G, pair, path):
    """A zero-laden problem (tests/axpby_model.zero_problem: stored zeros of both signs -- widening keeps the sign --, zeros in x and
    y0, rows whose products are all -0.0) through the loop of test_bitwise_equal_to_the_wide_call_on_the_widened_values -- every
    dispatch path, stateless and prepared, aligned arrays and arrays one element off, first call and call on hints --, and the same
    problem scaled to both ends of the exponent range (subnormal bf16 / fp32 stored values through the widening included): the
    mixed call equals the wide call AND the int64 model on the bits -- the model directly, because an error the two calls share
    passes the first comparison.  The atomic fix-up too: on exact data it is order-independent."""
    import axpby_model as AM
    sdt, cdt, npdt, vb, _ = PAIRS[pair]
    rng = np.random.default_rng(99)
    rows, cols, lens = T.SHAPES["power_law"](rng)
    base = AM.zero_problem(rng, rows, cols, np.asarray(lens, np.int64), npdt)
    try:
        Mod.set_tuning(vb, 0, 0, T.PATHS[path])
        for which in ("plain", "bottom", "bottom_stored", "top"):
            pairs = AM.PAIRS + [(-0.5, 0)] if which == "plain" else AM.SCALE_PAIRS
            ev, ex = 0, 0
            if which != "plain":
                total = sum(AM.scale_exponents(npdt, which))
                ev, ex = AM.scale_exponents(npdt, which, e_values=mixed_e_values(pair, which, total))
            csr, x, y0 = AM.scaled(base, ev, ex)
            mag = np.abs(csr.values[csr.values != 0]).astype(np.float64)          # (on the host: nothing here can flush)
            tiny = float(torch.finfo(sdt).tiny)
            if which == "bottom_stored":
                assert 0 < mag.min() and mag.max() < tiny
            elif which != "plain":
                assert tiny <= mag.min() and mag.max() <= float(torch.finfo(sdt).max)
            want = {(a, b): torch.from_numpy(AM.model(*base, a, b, scale=ev + ex)) for a, b in pairs + [(1, 0)]}
            for shift in (False, True):
                P = Problem(pair, rows, cols, csr.row_offsets, csr.column_indices, csr.values, x, shift=shift, exact=True)
                stored = P.d_narrow.cpu()
                assert np.array_equal(stored.view(torch.int16 if pair == "bf16_f32" else torch.int32).numpy(), narrow_exact(pair, csr.values)[0].view(
                    torch.int16 if pair == "bf16_f32" else torch.int32).numpy()), "the stored values on the device are not the host's bit patterns"
                assert Mod.band_passes(P.rows, P.cols, P.nnz, vb) <= 1
                yin = torch.from_numpy(y0).cuda()
                for prepared in (False, True):
                    for alpha, beta in pairs:
                        ws_w, ws_m = P.workspace(prepared), P.workspace(prepared)
                        for call in ("first", "on hints"):
                            kw = {"alpha": float(alpha), "beta": float(beta)}
                            yw, ym = P.wide(ws_w, yin, **kw), P.mixed(ws_m, yin, **kw)
                            torch.cuda.synchronize()
                            where = (pair, path, which, shift, prepared, alpha, beta, call)
                            assert same_bits(ym.cpu(), want[(alpha, beta)]), (where, "mixed call against the model")
                            assert same_bits(yw, ym), (where, "wide call against the mixed call")
                    assert same_bits(P.mixed(P.workspace(prepared)).cpu(), want[(1, 0)]), (pair, path, which, shift, prepared, "plain mixed call")
    finally:
        Mod.set_tuning(vb)


WIDE_STORED_MAX = {"f32_f64": (1 << 24) - 1, "bf16_f32": 255}        # the largest odd integers the stored types hold exactly
WIDE_PATHS = ["one_launch_small_shape", "one_launch_large_shape", "classic_three_launch"]


def _long_among_short(rng):
    """rows of 8 .. 40 entries and three rows longer than a tile: short enough (6000) that x keeps a few bits in fp32"""
    lens = rng.integers(8, 41, 4000); lens[1000] = lens[1001] = 3000; lens[2500] = 6000
    return 4000, 3000, lens


WIDE_SHAPES = dict(T.COMPACT_SHAPES, long_among_short=_long_among_short)
# bf16 values have 8 bits and a long row leaves x few: a result has bits in the low half of a float only where a row sums several
# products, so the bf16 shapes hold no rows of one or two entries beside a long row (the shares are asserted below)
WIDE_CASES = [("f32_f64", "power_law"), ("f32_f64", "giant_plus_sprinkle"), ("f32_f64", "long_among_short"),
              ("bf16_f32", "five_point"), ("bf16_f32", "long_among_short")]


@pytest.mark.gpu
@pytest.mark.parametrize("pair,shape", WIDE_CASES)
@pytest.mark.parametrize("path", WIDE_PATHS)
def test_values_that_fill_the_stored_significand_equal_the_int64_model(G, shape, pair, path):
    """tests/axpby_model.wide_problem with the values capped at what the stored type holds: odd integers up to 2^24 - 1 stored as
    fp32 in an fp64 product -- every bit of the stored significand set somewhere, and a product of 44 bits: a conversion through
    float anywhere behind the widening changes y --, up to 255 stored as bf16 in an fp32 product; x and y0 odd integers as wide as
    the exactness budget allows.  The mixed call against the INT64 MODEL on the bits (not only against the wide call, which would
    share such an error): the one-launch kernel on both tile shapes and the classic launches, stateless and prepared, first call
    and call on hints, plain and alpha / beta."""
    import axpby_model as AM
    sdt, cdt, npdt, vb, _ = PAIRS[pair]
    rng = np.random.default_rng(101)
    rows, cols, lens = WIDE_SHAPES[shape](rng)
    csr, x, y0 = AM.wide_problem(rng, rows, cols, np.asarray(lens, np.int64), npdt, vcap=WIDE_STORED_MAX[pair])
    assert WIDE_STORED_MAX[pair] * 15 // 16 <= np.abs(csr.values).max() <= WIDE_STORED_MAX[pair]
    pairs = [(1, 0), (-1.5, 0.5), (-0.5, 0)]
    want = {p: AM.model(csr, x, y0, *p) for p in pairs}
    assert all(AM.low_half_share(csr, w) >= 0.95 for w in want.values())
    if pair == "f32_f64":
        assert all(share >= 0.9 for _, _, share in AM.carry_low_half_shares(csr, x))
    want = {p: torch.from_numpy(w) for p, w in want.items()}
    try:
        Mod.set_tuning(vb, 0, 0, T.PATHS[path])
        assert Mod.launch_info(rows, csr.nnz, vb)["flags"] == T.PATHS[path]
        P = Problem(pair, rows, cols, csr.row_offsets, csr.column_indices, csr.values, x, exact=True)
        assert Mod.band_passes(P.rows, P.cols, P.nnz, vb) <= 1
        yin = torch.from_numpy(y0).cuda()
        for prepared in (False, True):
            for alpha, beta in pairs:
                ws_w, ws_m = P.workspace(prepared), P.workspace(prepared)
                for call in ("first", "on hints"):
                    kw = {"alpha": float(alpha), "beta": float(beta)}
                    yw, ym = P.wide(ws_w, yin, **kw), P.mixed(ws_m, yin, **kw)
                    torch.cuda.synchronize()
                    where = (shape, pair, path, prepared, alpha, beta, call)
                    assert same_bits(ym.cpu(), want[(alpha, beta)]), (where, "mixed call against the model")
                    assert same_bits(yw, ym), (where, "wide call against the mixed call")
            assert same_bits(P.mixed(P.workspace(prepared)).cpu(), want[(1, 0)]), (shape, pair, path, prepared, "plain mixed call")
    finally:
        Mod.set_tuning(vb)


@pytest.mark.gpu
@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_golden_matrices_within_the_strict_bound_of_the_oracle_on_the_widened_csr(G, pair):
    npdt = PAIRS[pair][2]
    for case in T.CASES:
        args = [os.path.join(ROOT, case["args"][0])] if case["kind"] == "mtx" else case["args"]
        csr = O.make(case["kind"], *args, dtype=npdt)
        rng = np.random.default_rng(len(case["label"]))
        val = csr.values if case["kind"] == "mtx" else rng.uniform(-1, 1, csr.nnz)
        for x in (np.ones(csr.cols), np.arange(1, csr.cols + 1) * 0.5):
            P = Problem(pair, csr.rows, csr.cols, csr.row_offsets, csr.column_indices, val, x)
            ym = P.mixed(P.workspace())
            T.check_strict(Mod, P.csr, P.x, ym.cpu().numpy())          # same bound, same serial_sum_depth term: no new constant
            assert same_bits(P.wide(P.workspace()), ym), case["label"]


@pytest.mark.gpu
@pytest.mark.parametrize("pair,nnz_m", [("f32_f64", 25), ("bf16_f32", 40)])
def test_nontemporal_threshold_follows_the_true_bytes(G, pair, nnz_m, capfd):
    """full size, stream-bound: the wide stream is above 256 MB (non-temporal loads), the mixed one below (ordinary loads) -- the
    tile shape, and with it every sum, is the wide call's all the same"""
    _, _, npdt, vb, sb = PAIRS[pair]
    rows = nnz_m * 1_000_000 // 32
    nnz = rows * 32
    assert nnz * (vb + 4) + 4 * rows > 256 << 20 > nnz * (sb + 4) + 4 * rows          # crosses the threshold on one side only
    rng = np.random.default_rng(nnz_m)
    cols = 1 << 16
    col = np.sort(rng.integers(0, cols, size=(rows, 32), dtype=np.int32), axis=1).reshape(-1)
    P = Problem(pair, rows, cols, np.arange(rows + 1, dtype=np.int64) * 32, col, rng.uniform(-1, 1, nnz).astype(np.float32), rng.uniform(-1, 1, cols))
    assert Mod.band_passes(rows, cols, nnz, vb) <= 1
    ws_w, ws_m = P.workspace(), P.workspace()
    for _ in range(2):                       # first call, call on hints
        yw, ym = P.wide(ws_w), P.mixed(ws_m)
        torch.cuda.synchronize()
        assert same_bits(yw, ym)
    T.check_strict(Mod, P.csr, P.x, ym.cpu().numpy())


@pytest.mark.gpu
def test_a_column_band_candidate_equals_the_wide_calls_one_launch_form(G):
    """BASELINE config 2's shape, f32 -> f64: the wide call of these sizes is a candidate for the column bands (classic launches);
    the mixed call never is, and equals the wide call with the bands switched off (mspmv.h: the hot-column plan's rule)"""
    pair, vb = "f32_f64", 8
    rows = cols = 3_125_000
    per = 32
    nnz = rows * per
    assert Mod.band_passes(rows, cols, nnz, vb) > 1
    rng = np.random.default_rng(2)
    col = np.sort(rng.integers(0, cols, size=(rows, per), dtype=np.int32), axis=1).reshape(-1)
    P = Problem(pair, rows, cols, np.arange(rows + 1, dtype=np.int64) * per, col, rng.uniform(-1, 1, nnz).astype(np.float32), rng.uniform(-1, 1, cols))
    ym = P.mixed(P.workspace())
    try:
        Mod.set_band_passes(vb, -1)
        yw = P.wide(P.workspace())
        torch.cuda.synchronize()
    finally:
        Mod.set_band_passes(vb, 0)
    assert same_bits(yw, ym)
    T.check_strict(Mod, P.csr, P.x, ym.cpu().numpy())


def _guarded(t, fill, guard=64):
    """t's data between two guard bands of `guard` elements (what tests/test_gpu_parity.py::_guarded does), guard sized in elements of t's own type"""
    buf = torch.full((t.numel() + 2 * guard,), fill, dtype=t.dtype, device="cuda")
    buf[guard:guard + t.numel()] = t
    return buf, buf[guard:guard + t.numel()]


@pytest.mark.gpu
@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("flags", [0, 16, 4, 0xF000010])
def test_nothing_outside_the_arrays_is_used_or_written(G, pair, flags):
    """the cases of tests/test_gpu_parity.py::test_nothing_outside_the_arrays_is_used_or_written, the value guard sized for the
    stored type: NaN around values and x (a product with anything read from there would poison y), a pattern around y and the
    temp storage that must survive; nnz made ODD -- a bf16 array of odd length ends in the middle of a dword"""
    sdt, cdt, npdt, vb, _ = PAIRS[pair]
    rng = np.random.default_rng(flags + vb)
    try:
        Mod.set_tuning(vb, 0, 0, flags)
        for rows, cols, hi in ((1001, 333, 9), (40003, 1777, 40), (7, 5, 3)):
            lens = rng.integers(0, hi, rows)
            if (int(lens.sum()) & 1) == 0:
                lens[rows // 2] += 1                                     # odd nnz
            csr = T.random_csr(rng, rows, cols, lens, npdt)
            P = Problem(pair, rows, cols, csr.row_offsets, csr.column_indices, csr.values, rng.uniform(-1, 1, cols))
            assert P.nnz % 2 == 1
            gv, v = _guarded(P.d_narrow, float("nan"))
            gw, w = _guarded(P.d_wide, float("nan"))
            gro, ro = _guarded(P.d_ro, 0)
            gci, ci = _guarded(P.d_ci, 0)
            gx, x = _guarded(P.d_x, float("nan"))
            gy, y = _guarded(torch.zeros(rows, dtype=cdt, device="cuda"), 123.0)
            gy2, y2 = _guarded(torch.zeros(rows, dtype=cdt, device="cuda"), 123.0)
            before = [g.clone() for g in (gv, gro, gci, gx)]
            ws = P.workspace()
            tbuf = torch.full((ws.bytes + 512,), 0xAB, dtype=torch.uint8, device="cuda")
            ws.buffer = tbuf[256:256 + ws.bytes]
            Mod.csrmv_mixed(v, ro, ci, x, y=y, num_cols=cols, workspace=ws)
            Mod.csrmv(w, ro, ci, x, y=y2, num_cols=cols, workspace=P.workspace(), alpha=1.0, beta=0.0)
            torch.cuda.synchronize()
            for g, b in zip((gv, gro, gci, gx), before):
                assert torch.equal(g.view(torch.uint8), b.view(torch.uint8))         # inputs and their guards untouched
            assert torch.all(gy[:64] == 123.0) and torch.all(gy[64 + rows:] == 123.0)
            assert bool((tbuf[:256] == 0xAB).all()) and bool((tbuf[-256:] == 0xAB).all())
            assert not torch.isnan(y).any()
            assert same_bits(y, y2)
            T.check_strict(Mod, P.csr, P.x, y.cpu().numpy())
    finally:
        Mod.set_tuning(vb)


@pytest.mark.gpu
@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_degenerate_inputs(G, pair):
    sdt, cdt, npdt, vb, _ = PAIRS[pair]
    rng = np.random.default_rng(11)
    # rows == 0 and nnz == 0
    e32 = torch.zeros(0, dtype=torch.int32, device="cuda")
    y = Mod.csrmv_mixed(torch.zeros(0, dtype=sdt, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"), e32, torch.zeros(4, dtype=cdt, device="cuda"), num_cols=4)
    assert y.numel() == 0
    y = torch.full((5,), float("nan"), dtype=cdt, device="cuda")
    Mod.csrmv_mixed(torch.zeros(0, dtype=sdt, device="cuda"), torch.zeros(6, dtype=torch.int32, device="cuda"), e32, torch.ones(4, dtype=cdt, device="cuda"), y=y, num_cols=4)
    assert torch.equal(y, torch.zeros(5, dtype=cdt, device="cuda"))
    # beta == 0 never reads y (NaN in y does not survive); rows without entries get exactly 0, also under alpha / beta
    for rows, cols, lens in ((5000, 300, np.concatenate([np.zeros(2000, np.int64), rng.integers(1, 9, 1000), np.zeros(2000, np.int64)])),
                             (3000, 1, rng.integers(0, 3, 3000)),                           # one column
                             (1, 500, np.array([300001])),                                  # one giant row (odd length)
                             (4000, 512 if vb == 8 else 1024, rng.integers(0, 12, 4000))):  # x small enough for the LDS copy
        csr = T.random_csr(rng, rows, cols, np.asarray(lens, np.int64), npdt)
        P = Problem(pair, rows, cols, csr.row_offsets, csr.column_indices, csr.values, rng.uniform(-1, 1, cols))
        ws_w, ws_m = P.workspace(), P.workspace()
        nan_y = torch.full((rows,), float("nan"), dtype=cdt, device="cuda")
        ym = P.mixed(ws_m, nan_y, alpha=2.0, beta=0.0)
        assert not torch.isnan(ym).any()
        assert same_bits(ym, P.wide(ws_w, nan_y, alpha=2.0, beta=0.0))
        empty = torch.from_numpy(np.asarray(lens) == 0).cuda()
        assert torch.all(ym[empty] == 0)
        T.check_strict(Mod, P.csr, P.x, P.mixed(ws_m).cpu().numpy())
    # NaN / Inf stay in their rows
    rows, cols = 3000, 3000
    csr = T.random_csr(rng, rows, cols, rng.integers(1, 20, rows), npdt)
    val = csr.values.copy()
    bad_rows = np.array([0, 1234, rows - 1])
    for r, b in zip(bad_rows, (np.nan, np.inf, -np.inf)):
        val[csr.row_offsets[r]] = b
    P = Problem(pair, rows, cols, csr.row_offsets, csr.column_indices, val, rng.uniform(0.5, 1, cols))
    ym = P.mixed(P.workspace()).cpu().numpy()
    finite = np.ones(rows, bool); finite[bad_rows] = False
    assert np.isfinite(ym[finite]).all() and not np.isfinite(ym[bad_rows]).any()
    assert same_bits(P.wide(P.workspace()), torch.from_numpy(ym).cuda())


@pytest.mark.gpu
@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_capturable_into_a_hip_graph_and_correct_on_a_side_stream(G, pair, capfd):
    P = shape_problem(pair, "power_law")
    want = P.wide(P.workspace())
    ws = P.workspace()
    side = torch.cuda.Stream()
    y = torch.full((P.rows,), float("nan"), dtype=P.cdt, device="cuda")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        Mod.csrmv_mixed(P.d_narrow, P.d_ro, P.d_ci, P.d_x, y=y, num_cols=P.cols, workspace=ws, stream=side, debug_synchronous=True)
    side.synchronize()
    assert same_bits(y, want)
    assert "tile_kernel_snap<<<" in capfd.readouterr().out                 # debug_sync prints the launch lines
    # captured, replayed after x changed
    g = torch.cuda.CUDAGraph()
    y.fill_(float("nan"))
    with torch.cuda.graph(g):
        Mod.csrmv_mixed(P.d_narrow, P.d_ro, P.d_ci, P.d_x, y=y, num_cols=P.cols, workspace=ws, stream=torch.cuda.current_stream())
    g.replay(); torch.cuda.synchronize()
    assert same_bits(y, want)
    P.d_x.mul_(2.0)
    g.replay(); torch.cuda.synchronize()
    assert same_bits(y, P.wide(P.workspace()))
