"""gpu_spmv --coo: the CSR built on the device from the matrix's shuffled triples is checked entry for entry against a stable sort on
the host, the forward call on it and the stateless COO call verify against the host gold, and rocSPARSE's coosort + coo2csr is timed."""
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


def _coo_block(out):
    i = out.index("Merge-based CsrMV (COO: CSR built once on the device)")
    j = out.index("rocSPARSE CsrMV, ", i) if "rocSPARSE CsrMV, " in out[i:] else len(out)
    return out[i:j]


@gpu
def test_driver_coo_lines_on_a_grid():
    out = _gpu_spmv("--grid2d=300", "--i=5", "--coo", "--no-hyb")
    block = _coo_block(out)
    assert "CSR built on the device from shuffled COO: PASS" in block
    assert "Merge-based CooMV (stateless, CSR built inside every call), " in block
    assert "rocSPARSE coosort_by_row + coo2csr + gthr: " in block and "row offsets agree" in block
    assert block.count("\tPASS") == 2 and "FAIL" not in out
    assert block.count("strict check: PASS") == 2


@gpu
def test_driver_coo_lines_on_matrix_market_input_with_duplicates_fp32_alpha_beta():
    mtx = os.path.join(ROOT, "tests/golden/mtx/general_dups.mtx")
    out = _gpu_spmv("--mtx=" + mtx, "--i=3", "--coo", "--fp32", "--alpha=2.5", "--beta=-0.5", "--no-hyb")
    block = _coo_block(out)
    assert "CSR built on the device from shuffled COO: PASS" in block
    assert block.count("\tPASS") == 2 and "FAIL" not in out
