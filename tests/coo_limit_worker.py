"""Worker of tests/test_coo.py::test_coo_to_csr_at_the_item_limit: one structure-only COO -> CSR build with rows + nnz = MAX_ITEMS.

Entry i of the input is (row, col) = (R - 1 - i % R, C - 1 - (i // R) % C): rows arrive descending and, inside a row, columns
descending, so the build reverses everything.  With fewer entries per row than C the columns of a row are distinct and the output is
known in closed form: row r holds the entries i = (R - 1 - r) + R k, k = K_r - 1 .. 0, K_r = q + 1 for the last rem + 1 rows and q
for the others (q, rem = divmod(N - 1, R)).  Offsets, columns and the permutation are compared exactly, in chunks, with int64
arithmetic on the device.  Exit status 77: not enough free device memory (the last line printed says how much is needed)."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import merge_spmv_amd as M

MAX_ITEMS = 2 ** 31 - 1 - 65536
R, C = (1 << 20) + 3, 4096          # 3 row passes, 2 column passes
N = MAX_ITEMS - R
CHUNK = 1 << 26


def main():
    lib = M.load_library()
    q, rem = divmod(N - 1, R)
    assert q + 1 < C and R + N == MAX_ITEMS
    size = ctypes.c_size_t(0)
    assert lib.mspmv_coo_to_csr_f32(None, ctypes.byref(size), None, None, None, R, C, N, None, None, None, None, None, 0) == 0
    need = size.value + 4 * 4 * N + 4 * (R + 1) + (8 << 30)      # temp, two inputs, two outputs, offsets, room for the checks
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        print(f"skipped: the build at the item limit needs {need / 2**30:.1f} GiB of free device memory, {free / 2**30:.1f} GiB are free")
        return 77
    dev = "cuda"
    row = torch.empty(N, dtype=torch.int32, device=dev)
    col = torch.empty(N, dtype=torch.int32, device=dev)
    for i0 in range(0, N, CHUNK):
        i = torch.arange(i0, min(i0 + CHUNK, N), dtype=torch.int64, device=dev)
        row[i0:i0 + i.numel()] = (R - 1 - i % R).to(torch.int32)
        col[i0:i0 + i.numel()] = (C - 1 - (i // R) % C).to(torch.int32)
    del i
    off = torch.empty(R + 1, dtype=torch.int32, device=dev)
    col_csr = torch.empty(N, dtype=torch.int32, device=dev)
    perm = torch.empty(N, dtype=torch.int32, device=dev)
    temp = torch.empty(size.value, dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    status = lib.mspmv_coo_to_csr_f32(p(temp), ctypes.byref(size), None, p(row), p(col), R, C, N, p(off), p(col_csr), None, p(perm),
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), 0)
    assert status == 0, status
    torch.cuda.synchronize()
    del temp
    t = R - 1 - rem                                             # rows below t hold q entries, the others q + 1
    r = torch.arange(R + 1, dtype=torch.int64, device=dev)
    want_off = r * q + torch.clamp(r - t, min=0)
    assert int(want_off[-1]) == N
    assert torch.equal(off.to(torch.int64), want_off), "row offsets differ"
    for j0 in range(0, N, CHUNK):
        j = torch.arange(j0, min(j0 + CHUNK, N), dtype=torch.int64, device=dev)
        low = j < t * q
        jj = j - t * q
        rr = torch.where(low, j // q, t + jj // (q + 1))
        kdesc = torch.where(low, j % q, jj % (q + 1))
        k = torch.where(low, q - 1 - kdesc, q - kdesc)
        want_i = (R - 1 - rr) + R * k
        assert torch.equal(perm[j0:j0 + j.numel()].to(torch.int64), want_i), f"permutation differs in entries {j0}.."
        assert torch.equal(col_csr[j0:j0 + j.numel()].to(torch.int64), C - 1 - k), f"columns differ in entries {j0}.."
    print(f"coo limit OK: rows {R} + nnz {N} = {R + N}, {size.value / 2**30:.1f} GiB of temp storage")
    return 0


if __name__ == "__main__":
    sys.exit(main())
