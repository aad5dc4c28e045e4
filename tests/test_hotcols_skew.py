"""mspmv_csrmv_hotcols_skew against its definition (tests/plan_model.py: skew): the figure the multi-GPU operator decides on by
itself whether a part gets the hot-column plan.  wide_windows must be equal; the permille must be equal, or one off where the
model's own quotient lies within 1e-6 of a half-integer (the host's exp against numpy's) -- at most once in this file."""
import ctypes

import numpy as np
import pytest

import merge_spmv_amd as M
import plan_model as PM

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

HALF_INTEGER_CASES = []                   # the cases that needed the rounding allowance


def upload(col):
    d = torch.from_numpy(np.ascontiguousarray(col, dtype=np.int32)).cuda() if col.size else torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()              # (the probe may run on another stream than the copy)
    return d


def probe(d, cols, nnz, vb, stream=None, want_wide=True):
    permille, wide = ctypes.c_int32(-7), ctypes.c_int32(-7)
    handle = ctypes.c_void_p(stream.cuda_stream) if stream is not None else None
    st = M.load_library().mspmv_csrmv_hotcols_skew(ctypes.c_void_p(d.data_ptr()), cols, nnz, vb, handle, ctypes.byref(permille),
                                                   ctypes.byref(wide) if want_wide else None)
    assert st == 0
    return permille.value, wide.value


def pareto_columns(rng, cols, nnz):
    """the scale-free draw of tests/test_hot_columns.py"""
    hot = rng.permutation(cols)
    return hot[np.minimum((rng.pareto(0.9, nnz) * 3).astype(np.int64), cols - 1)].astype(np.int32)


def band_columns(rng, rows, per_row, half_width):
    col = np.repeat(np.arange(rows, dtype=np.int64), per_row) + rng.integers(-half_width, half_width + 1, rows * per_row)
    return np.clip(col, 0, rows - 1).astype(np.int32)


def wide_by_construction(rng, cols, wide):
    """512 disjoint windows (starts 4096 apart); `wide` of them hold columns 0 and cols - 1, everything else stays inside the
    first quarter of the columns"""
    nnz = PM.SKEW_WINDOW + (PM.SKEW_WINDOWS - 1) * 4096
    col = rng.integers(0, cols // 4, nnz).astype(np.int32)
    for w in rng.choice(PM.SKEW_WINDOWS, wide, replace=False):
        col[w * 4096 + 100], col[w * 4096 + 1900] = 0, cols - 1
    return col


CASES = {
    "uniform": lambda rng: (rng.integers(0, 200_000, 1_200_000).astype(np.int32), 200_000),
    "band50": lambda rng: (band_columns(rng, 150_000, 8, 50), 150_000),
    "pareto": lambda rng: (pareto_columns(rng, 200_000, 1_200_000), 200_000),
    "nnz2048": lambda rng: (rng.integers(0, 50_000, 2048).astype(np.int32), 50_000),
    "nnz2049": lambda rng: (np.r_[np.full(2048, 7), 49_999].astype(np.int32), 50_000),       # only the last window sees the far column
    "nnz2047": lambda rng: (rng.integers(0, 50_000, 2047).astype(np.int32), 50_000),
    "no_columns": lambda rng: (np.zeros(4096, np.int32), 0),
    "wide300": lambda rng: (wide_by_construction(rng, 100_000, 300), 100_000),
    "cols33": lambda rng: ((np.arange(4096) % 33).astype(np.int32), 33),
    "cols17": lambda rng: ((np.arange(4096) % 17).astype(np.int32), 17),
}
# what the construction itself says, besides the model: (vb or None = both, field, value)
BY_CONSTRUCTION = {"nnz2047": (None, "permille", -1), "no_columns": (None, "permille", -1), "wide300": (None, "wide", 300), "uniform": (None, "wide", 512),
                   "band50": (None, "wide", 0), "nnz2049": (None, "wide", 1), "cols33": (4, "distinct", 2), "cols17": (8, "distinct", 2)}


@gpu
@pytest.mark.parametrize("vb", [4, 8])
@pytest.mark.parametrize("name", sorted(CASES))
def test_skew_probe_equals_its_definition(name, vb):
    col, cols = CASES[name](np.random.default_rng(sum(map(ord, name))))
    distinct, wide, samples, permille, ratio = PM.skew(col, cols, vb)
    only_vb, field, value = BY_CONSTRUCTION.get(name, (None, None, None))
    if field and only_vb in (None, vb):
        assert {"permille": permille, "wide": wide, "distinct": distinct}[field] == value
    d = upload(col)
    got_permille, got_wide = probe(d, cols, col.size, vb)
    print(f"{name} vb={vb}: device {got_permille} / {got_wide}, model {permille} / {wide} (distinct {distinct}, samples {samples}, quotient {ratio})")
    assert got_wide == wide
    if got_permille != permille:
        near_half = permille >= 0 and abs((ratio + 0.5) - round(ratio + 0.5)) <= 1e-6
        assert near_half and abs(got_permille - permille) == 1, (got_permille, permille, ratio)
        HALF_INTEGER_CASES.append((name, vb))
    assert len(HALF_INTEGER_CASES) <= 1, HALF_INTEGER_CASES
    # on a side stream, and without the wide-window count
    assert probe(d, cols, col.size, vb, stream=torch.cuda.Stream()) == (got_permille, got_wide)
    assert probe(d, cols, col.size, vb, want_wide=False) == (got_permille, -7)
