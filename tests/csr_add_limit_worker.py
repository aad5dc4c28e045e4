"""Worker of tests/test_csr_add.py::test_add_at_the_item_limit: one structure-only C = A + B with rows + nnz_a + nnz_b = MAX_ITEMS.

The first R rows of A hold the columns = 0 mod 2 of C = 6 K columns, those of B the columns = 0 mod 3; E trailing rows are empty in
both.  The union of a row is the columns = 0, 2, 3, 4 mod 6 -- 4 K entries, a third of B's entries being partners of A's --, so the
offsets, the columns and the count are known in closed form and compared exactly, in chunks, with int64 arithmetic on the device.
Exit status 77: not enough free device memory (the last line printed says how much is needed)."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import merge_spmv_amd as M

MAX_ITEMS = 2 ** 31 - 1 - 65536
K = 100
C = 6 * K
R = MAX_ITEMS // (5 * K + 1)        # rows with entries: 3 K of A and 2 K of B each
E = MAX_ITEMS - R * (5 * K + 1)     # empty rows behind them
ROWS, NA, NB = R + E, 3 * K * R, 2 * K * R
CHUNK = 1 << 26


def _fill(col, per_row, step):
    for i0 in range(0, col.numel(), CHUNK):
        i = torch.arange(i0, min(i0 + CHUNK, col.numel()), dtype=torch.int64, device=col.device)
        col[i0:i0 + i.numel()] = ((i % per_row) * step).to(torch.int32)


def main():
    lib = M.load_library()
    assert ROWS + NA + NB == MAX_ITEMS and E >= 0
    size = ctypes.c_size_t(0)
    q = lambda *a: lib.mspmv_csr_add_f32(None, ctypes.byref(size), ROWS, C, 1.0, None, None, None, a[0], 1.0, None, None, None, a[1], None, None,
                                         None, None, None, 0)
    assert q(NA, NB) == 0 and q(NA + 1, NB) == 1
    need = size.value + 4 * 2 * (NA + NB) + 3 * 4 * (ROWS + 1) + (8 << 30)      # inputs, the output, offsets, room for the checks
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        print(f"skipped: the addition at the item limit needs {need / 2**30:.1f} GiB of free device memory, {free / 2**30:.1f} GiB are free")
        return 77
    dev = "cuda"
    r = torch.arange(ROWS + 1, dtype=torch.int64, device=dev).clamp_(max=R)
    off_a, off_b = (r * (3 * K)).to(torch.int32), (r * (2 * K)).to(torch.int32)
    col_a = torch.empty(NA, dtype=torch.int32, device=dev)
    col_b = torch.empty(NB, dtype=torch.int32, device=dev)
    _fill(col_a, 3 * K, 2)
    _fill(col_b, 2 * K, 3)
    off_c = torch.full((ROWS + 1,), -1, dtype=torch.int32, device=dev)
    col_c = torch.full((NA + NB,), -1, dtype=torch.int32, device=dev)
    count = torch.full((1,), -1, dtype=torch.int32, device=dev)
    temp = torch.empty(size.value, dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    status = lib.mspmv_csr_add_f32(p(temp), ctypes.byref(size), ROWS, C, 1.0, None, p(off_a), p(col_a), NA, 1.0, None, p(off_b), p(col_b), NB,
                                   None, p(off_c), p(col_c), p(count), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), 0)
    assert status == 0, status
    torch.cuda.synchronize()
    del temp, col_a, col_b
    n = 4 * K * R
    assert int(count.item()) == n, (int(count.item()), n)
    assert torch.equal(off_c.to(torch.int64), r * (4 * K)), "row offsets differ"
    residues = torch.tensor([0, 2, 3, 4], dtype=torch.int64, device=dev)
    for j0 in range(0, n, CHUNK):
        j = torch.arange(j0, min(j0 + CHUNK, n), dtype=torch.int64, device=dev)
        m = j % (4 * K)
        assert torch.equal(col_c[j0:j0 + j.numel()].to(torch.int64), 6 * (m // 4) + residues[m % 4]), f"columns differ in entries {j0}.."
    for j0 in range(n, NA + NB, CHUNK):
        assert bool((col_c[j0:min(j0 + CHUNK, NA + NB)] == -1).all()), "entries past the count were written"
    print(f"add limit OK: rows {ROWS} + nnz_a {NA} + nnz_b {NB} = {ROWS + NA + NB}, {n} entries in the union, "
          f"{size.value / 2**20:.1f} MiB of temp storage")
    return 0


if __name__ == "__main__":
    sys.exit(main())
