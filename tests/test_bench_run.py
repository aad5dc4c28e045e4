"""bench.py end to end on one GPU: the plain run the driver times (headline only, `--steps` timed steps, `ms_per_step` on the line)
and what --dump-outputs writes -- y of the last timed step, checked here against the same seeded inputs regenerated in this
process; beyond DUMP_BYTES a fixed, seeded sample of rows."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

gpu = pytest.mark.gpu


def _bench(*args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert lines and lines[-1].startswith("{") and len(lines[-1].encode()) < 4096, lines[-3:]
    return json.loads(lines[-1])


@gpu
def test_plain_run_is_the_headline_alone_and_dumps_its_y(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR`: the contract's keys with K timed steps, nothing that takes a run
    of its own (roofline pass, cpu_baseline, configs) and no detail file; DIR/y.npy is the headline's y in its own precision."""
    import torch
    import merge_spmv_amd as M
    from merge_spmv_amd import generators as G
    import bench
    out = _bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert out["metric"] == "CsrMV GFLOP/s" and out["unit"] == "GFLOP/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1 and out["ms_per_step"] > 0
    nnz = bench.C2_ROWS_PER_GPU * bench.C2_NPR
    assert abs(out["value"] - 2.0 * nnz / (out["ms_per_step"] * 1e-3) / 1e9) <= 1e-3 * out["value"]
    for k in ("roofline", "cpu_baseline", "configs", "sampled_worst_ratio", "detail"):
        assert k not in out, k
    assert sorted(os.listdir(tmp_path)) == ["y.npy"]
    y = np.load(tmp_path / "y.npy")
    assert y.dtype == np.float32 and y.shape == (bench.C2_ROWS_PER_GPU,) and np.isfinite(y).all()
    # the same seeded inputs, rebuilt here: the dumped y is A x within the witness's bound
    dev = torch.device("cuda", 0)
    A = G.uniform_csr(bench.C2_ROWS_PER_GPU, bench.C2_ROWS_PER_GPU, bench.C2_NPR, dtype=torch.float32, device=dev)
    x = G.uniform_pm1(G.SEED_C2 + 2, A.cols, torch.float32, dev)
    chk = M.sampled_check(A, x, torch.from_numpy(y).to(dev))
    assert chk["violations"] == 0 and chk["worst_ratio"] < 1, chk


@gpu
def test_dump_of_a_large_y_is_a_seeded_sample(tmp_path):
    """A y beyond DUMP_BYTES (R-MAT scale 23 in fp64: 64 MiB) is written as a fixed sample of rows, the row numbers beside it; both runs
    of the same command write the same rows, and the values are those of the same call made here."""
    import torch
    import merge_spmv_amd as M
    from merge_spmv_amd import generators as G
    import bench
    scale, edges = 23, 20_000_000
    args = ("--gpus", "1", "--steps", "2", "--warmup", "1", "--workload", "c5", "--c5-scale", str(scale), "--c5-edges", str(edges))
    out = _bench(*args, "--dump-outputs", str(tmp_path / "a"))
    assert out["dtype"] == "f64" and out["steps"] == 2
    _bench(*args, "--dump-outputs", str(tmp_path / "b"))
    files = {f: os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sorted(files) == ["y.npy", "y_rows.npy"] and sum(files.values()) <= bench.DUMP_BYTES + 512
    rows, y = np.load(tmp_path / "a" / "y_rows.npy"), np.load(tmp_path / "a" / "y.npy")
    assert rows.dtype == np.float64 and y.dtype == np.float64 and rows.shape == y.shape
    assert np.array_equal(rows, np.load(tmp_path / "b" / "y_rows.npy"))
    r = rows.astype(np.int64)
    assert np.array_equal(r, rows) and (np.diff(r) > 0).all() and r[0] >= 0 and r[-1] < (1 << scale)
    dev = torch.device("cuda", 0)
    A = G.rmat_csr(scale, edges, dtype=torch.float64, device=dev, seed=G.SEED_C5)
    x = G.uniform_pm1(G.SEED_C5 + 2, A.cols, torch.float64, dev)
    yd = M.csrmv(A.values, A.row_offsets, A.column_indices, x, num_cols=A.cols)
    np.testing.assert_allclose(y, yd[torch.from_numpy(r).to(dev)].cpu().numpy(), rtol=1e-10, atol=1e-9)
