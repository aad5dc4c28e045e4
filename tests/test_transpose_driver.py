"""gpu_spmv --transpose: the device-built A^T is checked entry for entry against the stable host transpose, and the three method lines
(the forward call on the built A^T, the stateless transposed call, rocSPARSE's transposed CsrMV) verify against the host gold of A^T x."""
import os
import subprocess

import pytest

from conftest import ROOT

gpu = pytest.mark.gpu


def _gpu_spmv(*args, timeout=300):
    exe = os.path.join(ROOT, "merge_spmv_amd", "gpu_spmv")
    if not os.path.exists(exe):                  # normally built by __graft_entry__.build()
        subprocess.run(["make", "-C", os.path.join(ROOT, "merge_spmv_amd"), "gpu_spmv"], check=True, capture_output=True, timeout=600)
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _transpose_block(out):
    i = out.index("Merge-based CsrMV (transpose: A^T built once on the device)")
    j = out.index("rocSPARSE CsrMV, ", i) if "rocSPARSE CsrMV, " in out[i:] else len(out)
    return out[i:j]


@gpu
def test_driver_transpose_lines_on_a_grid():
    out = _gpu_spmv("--grid2d=300", "--i=5", "--transpose", "--no-hyb")
    block = _transpose_block(out)
    assert "transpose built on the device: PASS" in block
    for method in ("Merge-based CsrMV (transpose: A^T built once on the device), ", "Merge-based CsrMV (transpose: stateless",
                   "rocSPARSE CsrMV (transpose), "):
        assert method in block
    assert block.count("\tPASS") == 3 and "FAIL" not in out
    assert block.count("strict check: PASS") == 3


@gpu
def test_driver_transpose_lines_on_matrix_market_input_fp32_alpha_beta():
    mtx = os.path.join(ROOT, "tests/golden/mtx/giant_row.mtx")
    out = _gpu_spmv("--mtx=" + mtx, "--i=3", "--transpose", "--fp32", "--alpha=2.5", "--beta=-0.5", "--no-hyb")
    block = _transpose_block(out)
    assert "transpose built on the device: PASS" in block and "rocSPARSE CsrMV (transpose), " in block
    assert block.count("\tPASS") == 3 and "FAIL" not in out
