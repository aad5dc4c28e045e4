"""The partitioned (multi-GPU) CsrMV operator, mspmv_mg_plan_* / mspmv_mg_csrmv / mspmv_mg_allgather_rows, on the bits.
No tolerance anywhere; bit patterns are compared (axpby_model.bits: -0.0 is not +0.0).  All parts on device 0, peer exchange.

Two layers, because each sees what the other cannot:
  (a) ROUTING on integer data (axpby_model: every product and every sum in any association is exact): the assembled y must be the
      int64 model of the whole matrix, every part's open-row entry the exact sum of its share.  A carry dropped, taken twice or
      taken by the wrong part shows; the ORDER of the adds cannot.
  (b) COMPOSITION on rounding data: y of a plan = the prepared single-GPU call (mspmv_csrmv_prepared_*) on each part's own device
      arrays + the fold of the open-row entries in ascending part order (tests/mg_model.py: fold), open rows included.  This pins
      the order of the fold and the decisions of the plan's inner call.  On uniform data a wrong order shows only where the
      roundings happen to differ; one probe, built so that they must, pins the order by construction.
  (c) both with every part's arrays one element past a 256-byte boundary: the dword-per-lane classic form on coordinates found
      while the value and column pointers were still unknown.
  (d) K rounds of csrmv(); allgather_rows() enqueued WITHOUT a host synchronisation, against the same chain driven from the host.
  (e) the routing of (a) on mg_model.wide_problem (odd integers that fill the exactness budget) at 2, 7 and 64 parts, with and
      without the parts' hot-column plans, on unaligned part arrays, and through the RCCL one-rank backend: every part's sums, the
      open-row entries of a boundary row shared by several parts and the folded carries then hold bits in the low word of a double.
tests/test_mg_model.py guards the model and the inputs on the CPU; the hipIpc backend needs a process per part: its exact and its
wide case are tests/test_mg_plan.py::test_ipc_backend_two_processes_sharing_the_device's (tests/mg_ipc_worker.py).  Measured on one MI355X: the 338 tests of this file take 51.8 s, the 288
before the wide draw 35.1 s (a plan of 64 parts is built and closed per test: about 0.3 s each)."""
import functools

import numpy as np
import pytest

import axpby_model as AM
import mg_model as MM
import merge_spmv_amd as M
from merge_spmv_amd import multi_gpu as MG

torch = pytest.importorskip("torch")
from test_mixed_precision import off_by_one   # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = sorted(MM.PROBLEMS)
NONSQUARE = MM.NONSQUARE_COLS
PRECS = {"f32": (np.float32, torch.float32, 4), "f64": (np.float64, torch.float64, 8)}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: torch.cuda.is_available() is False")
    M.load_library()


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _integer(name, prec):
    """(csr, x, the int64 model of A*x): computed once per problem and precision, read-only"""
    csr, x = MM.integer_problem(name, PRECS[prec][0])
    want = AM.model(csr, x, None, 1, 0)
    _frozen(csr.row_offsets, csr.column_indices, csr.values, x, want)
    return csr, x, want


@functools.lru_cache(maxsize=None)
def _wide(name, prec):
    """_integer on mg_model.wide_problem: odd integers that fill the exactness budget (both halves of every fp64 sum, open-row entry
    and folded carry hold bits; tests/test_mg_model.py asserts it)"""
    csr, x = MM.wide_problem(name, PRECS[prec][0])
    want = AM.model(csr, x, None, 1, 0)
    _frozen(csr.row_offsets, csr.column_indices, csr.values, x, want)
    return csr, x, want


@functools.lru_cache(maxsize=None)
def _rounding(name, prec, scale=1.0):
    csr, x = MM.float_problem(name, PRECS[prec][0], scale)
    _frozen(csr.row_offsets, csr.column_indices, csr.values, x)
    return csr, x


class Built:
    """a plan with all parts on device 0 (tests/test_mg_plan.py::_plan_on_one_device) that keeps the parts' device tensors"""

    def __init__(self, csr, parts, prec, exchange=MG.EXCHANGE_PEER, place=None, id128=None):
        self.dtype, self.tdt, self.vb = PRECS[prec]
        self.csr, self.parts = csr, parts
        place = place or (lambda t: t)
        off = csr.row_offsets.astype(np.int64)
        self.row_split, self.nz_split = MG.partition(off, parts)
        self.plan = MG.MgPlan(self.row_split, self.nz_split, csr.cols, self.tdt, list(range(parts)), [0] * parts, exchange=exchange, id128=id128)
        self.tensors, self.ws = [], {}
        try:
            for g in range(parts):
                lo = MG.local_offsets(off, self.row_split[g], self.row_split[g + 1], self.nz_split[g], self.nz_split[g + 1])
                a, b = int(self.nz_split[g]), int(self.nz_split[g + 1])
                t = (place(torch.from_numpy(csr.values[a:b].copy()).cuda()), place(torch.from_numpy(lo).cuda()),
                     place(torch.from_numpy(csr.column_indices[a:b].copy()).cuda()))
                self.tensors.append(t)
                self.plan.set_part(g, *t)
        except BaseException:
            self.plan.close()
            raise

    def set_x(self, x):
        self.plan.x(0).copy_(torch.from_numpy(np.array(x)).cuda())
        torch.cuda.synchronize()

    def snapshot(self):
        """(assembled y, every part's open-row entry) as the plan holds them now"""
        locals_ = [self.plan.y(g, with_open_row=True).cpu().numpy() for g in range(self.parts)]
        assert all(l.size == self.row_split[g + 1] - self.row_split[g] + 1 for g, l in enumerate(locals_))
        return np.concatenate([l[:-1] for l in locals_]), np.array([l[-1] for l in locals_], self.dtype)

    def single_gpu_locals(self, x_dev, debug=False):
        """the prepared single-GPU call on the SAME device tensors of every part: its y (owned rows + the open row), as host arrays"""
        ys = []
        for g, (vals, lo, ci) in enumerate(self.tensors):
            lr, ln = lo.numel() - 1, vals.numel()
            if g not in self.ws:
                self.ws[g] = M.CsrMVWorkspace(lr, ln, self.tdt).prepare(lo)
            y = torch.full((lr,), float("nan"), dtype=self.tdt, device="cuda")
            M.csrmv(vals, lo, ci, x_dev, y=y, num_cols=self.csr.cols, workspace=self.ws[g], debug_synchronous=debug)
            ys.append(y)
        torch.cuda.synchronize()
        return [y.cpu().numpy() for y in ys]

    def assert_default_form(self):
        """no part is a column-band candidate, none would take the small tile shape for short rows over a tiny x: the two forms in
        which a prepared call may differ from the plan's inner call (include/mspmv.h at mspmv_mg_csrmv)"""
        for vals, lo, _ in self.tensors:
            lr, ln = lo.numel() - 1, vals.numel()
            assert M.band_passes(lr, self.csr.cols, ln, self.vb) <= 1
            assert M.launch_info(lr, ln, self.vb, num_cols=self.csr.cols)["items_per_thread"] == M.launch_info(lr, ln, self.vb)["items_per_thread"]

    def close(self):
        self.plan.close()


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    diff = np.flatnonzero(AM.bits(got) != AM.bits(want))
    assert diff.size == 0, (what, f"{diff.size} entries differ, first at {diff[0]}: got {got[diff[0]]!r}, want {want[diff[0]]!r}")


def _exact_open_rows(csr, x, row_split, nz_split, dtype):
    """every part's exact share of its open row (int64); the empty share is +0.0"""
    parts = len(row_split) - 1
    return np.array([AM.row_sums(MM.local_csr(csr, row_split, nz_split, g), x)[0][-1] for g in range(parts)], np.int64).astype(dtype)


# --------------------------------------------------------------------------------------------------------------- (a) routing

def _check_routing(name, parts, prec, place=None, data=_integer):
    csr, x, want = data(name, prec)
    B = Built(csr, parts, prec, place=place)
    plan = B.plan
    try:
        opens = _exact_open_rows(csr, x, B.row_split, B.nz_split, B.dtype)
        B.set_x(x)
        plan.csrmv(); plan.synchronize()
        y, o = B.snapshot()
        _same(y, want, (name, parts, prec, "y"))
        _same(o, opens, (name, parts, prec, "open rows"))
        # three more steps back to back: a take applied twice, or a y not rewritten, shows here
        for _ in range(3):
            plan.csrmv()
        plan.synchronize()
        y, o = B.snapshot()
        _same(y, want, (name, parts, prec, "y after 3 unsynchronised steps"))
        _same(o, opens, (name, parts, prec, "open rows after 3 unsynchronised steps"))
        assert plan.info()["steps"] == 4
        plan.hot_columns(True)
        assert plan.info()["hot_parts"] == parts
        plan.csrmv(); plan.synchronize()
        y, o = B.snapshot()
        _same(y, want, (name, parts, prec, "y, hot columns"))
        _same(o, opens, (name, parts, prec, "open rows, hot columns"))
        plan.hot_columns(False)
        assert plan.info()["hot_parts"] == 0
        plan.csrmv(); plan.synchronize()
        y, o = B.snapshot()
        _same(y, want, (name, parts, prec, "y, hot columns off again"))
        _same(o, opens, (name, parts, prec, "open rows, hot columns off again"))
    finally:
        B.close()


@pytest.mark.parametrize("prec", sorted(PRECS))
@pytest.mark.parametrize("parts", MM.PARTS)
@pytest.mark.parametrize("name", NAMES)
def test_routing_is_exact_on_integer_data(name, parts, prec):
    _check_routing(name, parts, prec)


@pytest.mark.parametrize("prec", sorted(PRECS))
@pytest.mark.parametrize("parts", MM.WIDE_PARTS)
@pytest.mark.parametrize("name", MM.WIDE_NAMES)
def test_routing_is_exact_on_numbers_that_fill_the_significand(name, parts, prec):
    """the routing test on mg_model.wide_problem at 2, 7 and 64 parts, the peer exchange with and without the parts' hot-column
    plans: the open-row entries and the folded carries of a boundary row shared by several parts now have bits in the low word
    of a double, so a carry that travels as a float, or as two words of which one is lost or taken from another part, shows"""
    _check_routing(name, parts, prec, data=_wide)


@pytest.mark.parametrize("parts", [7])
@pytest.mark.parametrize("name", ["giant_middle", "short"])
def test_unaligned_part_arrays_on_numbers_that_fill_the_significand(name, parts):
    _check_routing(name, parts, "f64", place=off_by_one, data=_wide)


@pytest.mark.parametrize("with_id", [False, True])
@pytest.mark.parametrize("prec", sorted(PRECS))
@pytest.mark.parametrize("name", NAMES)
def test_one_part_through_the_rccl_backend_is_exact(name, prec, with_id):
    """parts == 1 through the RCCL one-rank backend: the single-process form (ncclCommInitAll) and the multi-process form with a
    shipped id (ncclCommInitRank); its all-gather of the one carry is issued every step.  The shapes of mg_model.WIDE_NAMES on the
    wide draw as well."""
    for data in ([_integer, _wide] if name in MM.WIDE_NAMES else [_integer]):
        _one_part_through_rccl(name, prec, with_id, data)


def _one_part_through_rccl(name, prec, with_id, data):
    csr, x, want = data(name, prec)
    B = Built(csr, 1, prec, exchange=MG.EXCHANGE_RCCL, id128=MG.unique_id() if with_id else None)
    try:
        assert B.plan.info()["exchange"] == MG.EXCHANGE_RCCL
        B.set_x(x)
        B.plan.csrmv(); B.plan.synchronize()
        y, o = B.snapshot()
        _same(y, want, (name, prec, with_id, "y"))
        assert o[0] == 0 and not np.signbit(o[0])
        for _ in range(3):
            B.plan.csrmv()
        B.plan.synchronize()
        _same(B.snapshot()[0], want, (name, prec, with_id, "y after 3 unsynchronised steps"))
    finally:
        B.close()


# ----------------------------------------------------------------------------------------------------------- (b) composition

def _check_composition(name, parts, prec, place=None, capfd=None):
    csr, x = _rounding(name, prec)
    B = Built(csr, parts, prec, place=place)
    try:
        B.assert_default_form()
        B.set_x(x)
        B.plan.csrmv(); B.plan.synchronize()
        y, o = B.snapshot()
        if capfd is not None:
            capfd.readouterr()
        locals_ = B.single_gpu_locals(B.plan.x(0), debug=capfd is not None)
        log = capfd.readouterr().out if capfd is not None else None
        assert not any(np.isnan(l).any() for l in locals_)
        want_y, want_o = MM.fold(locals_, B.row_split, B.dtype)
        _same(o, want_o, (name, parts, prec, "open rows"))
        _same(y, want_y, (name, parts, prec, "y"))
        # a second step leaves the same bits (y is rewritten, not accumulated into)
        B.plan.csrmv(); B.plan.synchronize()
        _same(B.snapshot()[0], want_y, (name, parts, prec, "y, second step"))
        return log
    finally:
        B.close()


@pytest.mark.parametrize("prec", sorted(PRECS))
@pytest.mark.parametrize("parts", [p for p in MM.PARTS if p > 1])
@pytest.mark.parametrize("name", NAMES)
def test_plan_is_the_prepared_call_per_part_plus_the_fold_in_part_order(name, parts, prec):
    _check_composition(name, parts, prec)


@pytest.mark.parametrize("prec", sorted(PRECS))
@pytest.mark.parametrize("parts", [3, 8, 64])
@pytest.mark.parametrize("big", ["first", "last"])
def test_the_order_of_the_fold_shows_in_the_result_by_construction(big, parts, prec):
    """On uniform data two orders of the fold often round to the same bits (a case above sees a reversed fold only by chance).
    Here the order shows by construction: ONE row of 1919 nonzeros cut into `parts` shares, every share a single nonzero value
    among zeros (so each part's sum is exact whatever its association), x = 1.  The last part owns the row; its own share is 1,
    one source's share is B = 2^24 (2^53: the first integer whose successor the type cannot hold), every other source's is 1.
    Adding 1 to B rounds back to B (ties to even), so
        big = first:  ((1 + B) + 1) + 1 ... = B              any order that adds another source before it gives B + 2 or more
        big = last:   ((1 + 1) + 1 ...) + B = B + parts - 1 rounded to even      any order that adds it earlier gives less."""
    dtype, _, vb = PRECS[prec]
    nnz = 1919                                              # rows + nnz = 1920 = 3 * 640 = 8 * 240 = 64 * 30: equal swaths
    B_ = dtype(2.0 ** (24 if vb == 4 else 53))
    off = np.array([0, nnz], np.int64)
    row_split, nz_split = MM.partition(off, parts)
    assert np.all(row_split[:-1] == 0) and row_split[-1] == 1 and np.all(np.diff(nz_split) >= 1)
    assert MM.sources(row_split)[-1] == list(range(parts - 1))
    val = np.zeros(nnz, dtype)
    val[nz_split[:-1]] = 1                                  # the first nonzero of every share
    val[nz_split[0 if big == "first" else parts - 2]] = B_
    rng = np.random.default_rng(parts)
    csr = AM.Csr(1, NONSQUARE, off.astype(np.int32), np.sort(rng.integers(0, NONSQUARE, nnz)).astype(np.int32), val)
    shares = val[nz_split[:-1]]
    y_locals = [np.array([s], dtype) for s in shares[:-1]] + [np.array([shares[-1], 0], dtype)]
    want, want_open = MM.fold(y_locals, row_split, dtype)
    backwards = shares[-1]
    for s in shares[-2::-1]:
        backwards = dtype(backwards + s)
    assert want[0] == (B_ if big == "first" else dtype(int(B_) + parts - 1)) and backwards != want[0]      # (one rounding of the exact integer) the probe can see the order
    built = Built(csr, parts, prec)
    try:
        built.set_x(np.ones(NONSQUARE, dtype))
        built.plan.csrmv(); built.plan.synchronize()
        y, o = built.snapshot()
        _same(o, want_open, (big, parts, prec, "open rows"))
        _same(y, want, (big, parts, prec, "y"))
    finally:
        built.close()


# ------------------------------------------------------------------------------------------------- (c) unaligned part arrays

@pytest.mark.parametrize("prec", sorted(PRECS))
@pytest.mark.parametrize("parts", [3, 8])
@pytest.mark.parametrize("name", ["giant_middle", "short"])
def test_unaligned_part_arrays(name, parts, prec, capfd):
    """every part's values, local offsets and column indices one element past a 256-byte boundary: not 16-byte aligned"""
    _check_routing(name, parts, prec, place=off_by_one)
    log = _check_composition(name, parts, prec, place=off_by_one, capfd=capfd)
    # the composed call ran the classic three launches with the dword-per-lane tile kernel, on prepared coordinates
    assert log.count("mspmv: tile_kernel<<<") == parts, log
    assert "tile_kernel_snap" not in log and "tile_kernel_vec" not in log and "search_kernel" not in log and "coords_" not in log, log


def test_aligned_part_arrays_take_the_16_byte_forms(capfd):
    """the counterpart of the log assertion above: the same parts on aligned arrays do NOT run the dword-per-lane kernel"""
    log = _check_composition("short", 3, "f64", capfd=capfd)
    assert "mspmv: tile_kernel<<<" not in log and ("tile_kernel_snap" in log or "tile_kernel_vec" in log), log


# ----------------------------------------------------------------------------------------------------- (d) pipelined iteration

ROUNDS = 6


@pytest.mark.parametrize("twice", [False, True])
@pytest.mark.parametrize("prec", sorted(PRECS))
@pytest.mark.parametrize("parts", [2, 8, 64])
@pytest.mark.parametrize("name", ["short", "giant_middle"])
def test_pipelined_iteration_equals_the_host_driven_chain(name, parts, prec, twice):
    """x_{k+1} = A x_k, 6 rounds of csrmv(); allgather_rows() (twice: two csrmv() per round) enqueued back to back -- only the plan's
    own done / applied / pushed event edges order them -- then ONE synchronize.  Expected: x_{k+1} = fold(single-GPU calls on x_k),
    driven from the host round by round."""
    csr, x0 = _rounding(name, prec, 0.05)                   # (values scaled so that the iterates stay bounded)
    assert csr.rows == csr.cols
    B = Built(csr, parts, prec)
    try:
        B.set_x(x0)
        for _ in range(ROUNDS):
            B.plan.csrmv()
            if twice:
                B.plan.csrmv()
            B.plan.allgather_rows()
        B.plan.synchronize()
        got_x = B.plan.x(0).cpu().numpy()
        got_y, _ = B.snapshot()
        assert B.plan.info()["steps"] == ROUNDS * (2 if twice else 1)
        x = x0
        xd = torch.empty(csr.cols, dtype=B.tdt, device="cuda")
        for _ in range(ROUNDS):
            xd.copy_(torch.from_numpy(np.array(x)).cuda())
            x, _ = MM.fold(B.single_gpu_locals(xd), B.row_split, B.dtype)
        assert np.isfinite(x).all() and np.count_nonzero(x) > x.size // 4          # the chain neither blew up nor died out
        _same(got_x, x, (name, parts, prec, twice, "x replica"))
        _same(got_y, x, (name, parts, prec, twice, "y"))
    finally:
        B.close()


def test_allgather_rows_needs_a_square_operator():
    csr, x, _ = _integer("giant_first", "f64")
    assert csr.rows != csr.cols
    B = Built(csr, 2, "f64")
    try:
        B.set_x(x)
        B.plan.csrmv()
        with pytest.raises(M.MspmvError):
            B.plan.allgather_rows()
        B.plan.synchronize()
    finally:
        B.close()
