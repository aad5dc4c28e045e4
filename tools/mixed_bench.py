"""tools/mixed_bench.py -- mixed-precision CsrMV against the wide call on the widened values (profiles/mixed_bench.txt).

Per matrix and pair (f32 -> f64, bf16 -> f32): the wide call of the compute type on the widened values (mspmv_csrmv_axpby_*), the
mixed call (mspmv_csrmv_mixed_*) and, with --parent-lib, the wide call of ANOTHER build of the library (the parent commit's) on the
same arrays -- the versions ALTERNATED call by call inside one run, every call timed on its own between two events on the stream
after warm-up; the table gives the median and the spread (min .. max) of `--reps` calls.  Beside the time ratio stands the ratio of
algorithmic stream bytes, (nnz (4 + sizeof stored) + 4 rows) / (nnz (4 + sizeof compute) + 4 rows), and whether y was bitwise equal.
All calls go through the C ABI with the same ctypes overhead.  Development / reporting aid.

    python tools/mixed_bench.py [--only dense32,c2] [--pairs f32_f64,bf16_f32] [--reps 15] [--parent-lib path/to/libmspmv.so]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import merge_spmv_amd as M                                  # noqa: E402
from merge_spmv_amd import generators as G                  # noqa: E402

vp = ctypes.c_void_p
PAIRS = {"f32_f64": (torch.float32, torch.float64, "f64", ctypes.c_double), "bf16_f32": (torch.bfloat16, torch.float32, "f32", ctypes.c_float)}


def parent_axpby(path, sfx, ct):
    lib = ctypes.CDLL(path)
    fn = getattr(lib, "mspmv_csrmv_axpby_" + sfx)
    fn.restype = ctypes.c_int
    fn.argtypes = [vp, ctypes.POINTER(ctypes.c_size_t), vp, vp, vp, vp, vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ct, ct, vp, ctypes.c_int]
    return fn


def alternated(calls, reps, warm=3):
    """{name: [median, min, max] ms}: the calls take turns, each between its own pair of events; the order rotates from round to
    round, so that no version always runs on what one particular other version left in the caches"""
    times = {k: [] for k in calls}
    names = list(calls)
    for it in range(warm + reps):
        for k in names[it % len(names):] + names[:it % len(names)]:
            fn = calls[k]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            if it >= warm:
                times[k].append(e0.elapsed_time(e1))
    return {k: [round(statistics.median(t), 5), round(min(t), 5), round(max(t), 5)] for k, t in times.items()}


def run(label, A, pair, reps, parent):
    sdt, cdt, sfx, ct = PAIRS[pair]
    lib = M.load_library()
    narrow = A.values.to(sdt)                # the values are DRAWN in the stored type: the widened matrix is the matrix
    wide = narrow.to(cdt)
    x = G.uniform_pm1(12345, A.cols, cdt, "cuda")
    vb, sb = wide.element_size(), narrow.element_size()
    info = M.launch_info(A.rows, A.nnz, vb)
    stream = vp(torch.cuda.current_stream().cuda_stream)
    out = {"matrix": label, "pair": pair, "rows": A.rows, "cols": A.cols, "nnz": A.nnz,
           "stream_bytes_wide": A.nnz * (4 + vb) + 4 * A.rows, "stream_bytes_mixed": A.nnz * (4 + sb) + 4 * A.rows,
           "wide_is_band_candidate": M.band_passes(A.rows, A.cols, A.nnz, vb) > 1}
    out["byte_ratio"] = round(out["stream_bytes_mixed"] / out["stream_bytes_wide"], 4)

    def caller(fn, values):
        temp = torch.empty(int(info["temp_bytes"]), dtype=torch.uint8, device="cuda")      # the same size for every version
        y = torch.full((A.rows,), float("nan"), dtype=cdt, device="cuda")
        size = ctypes.c_size_t(temp.numel())
        args = (vp(temp.data_ptr()), ctypes.byref(size), vp(values.data_ptr()), vp(A.row_offsets.data_ptr()), vp(A.column_indices.data_ptr()),
                vp(x.data_ptr()), vp(y.data_ptr()), A.rows, A.cols, A.nnz, ct(1.0), ct(0.0), stream, 0)

        def call():
            st = fn(*args)
            assert st == 0, st
        return call, y
    calls, ys = {}, {}
    calls["wide"], ys["wide"] = caller(getattr(lib, "mspmv_csrmv_axpby_" + sfx), wide)
    calls["mixed"], ys["mixed"] = caller(getattr(lib, "mspmv_csrmv_mixed_" + pair), narrow)
    if parent:
        calls["parent_wide"], ys["parent_wide"] = caller(parent_axpby(parent, sfx, ct), wide)
    t = alternated(calls, reps)
    for k, v in t.items():
        out[k + "_ms"] = v
    out["mixed_over_wide"] = round(t["mixed"][0] / t["wide"][0], 4)
    out["wide_spread"] = round((t["wide"][2] - t["wide"][1]) / t["wide"][0], 4)
    out["wide_tbs"] = round(out["stream_bytes_wide"] / t["wide"][0] / 1e9, 3)
    out["mixed_tbs"] = round(out["stream_bytes_mixed"] / t["mixed"][0] / 1e9, 3)
    it = torch.int64 if cdt == torch.float64 else torch.int32
    out["bitwise_equal"] = bool(torch.equal(ys["wide"].view(it), ys["mixed"].view(it)))
    if parent:
        out["mixed_over_parent_wide"] = round(t["mixed"][0] / t["parent_wide"][0], 4)
        out["wide_over_parent_wide"] = round(t["wide"][0] / t["parent_wide"][0], 4)
        out["wide_equals_parent_wide"] = bool(torch.equal(ys["wide"].view(it), ys["parent_wide"].view(it)))
    return out


MATRICES = {
    "dense32": lambda: ("--dense=32, 2^20 rows (33.5 M nonzeros)", G.dense_csr(1 << 20, 32, dtype=torch.float32, ones=False)),
    "c4": lambda: ("C4 degenerate_csr (2^24 rows, a 2^26-entry row)", G.degenerate_csr(dtype=torch.float32, ones=False)),
    "rows512": lambda: ("rows of 512 over a tiny x, 100 M nonzeros", G.dense_csr(195312, 512, dtype=torch.float32, ones=False)),
    "rows2048": lambda: ("rows of 2048, 50 M nonzeros", G.dense_csr(24414, 2048, dtype=torch.float32, ones=False)),
    "rows4096": lambda: ("rows of 4096, 30 M nonzeros", G.dense_csr(7324, 4096, dtype=torch.float32, ones=False)),
    "grid2d": lambda: ("grid2d 2000 (4 M rows, 5-point)", G.grid2d_csr(2000, dtype=torch.float32)),
    "c2": lambda: ("C2 uniform 3125000^2, 32/row (gather-bound)", G.uniform_csr(3_125_000, 3_125_000, 32, dtype=torch.float32)),
    "small": lambda: ("uniform 3125^2, 32/row, 10^5 nonzeros (launch-bound)", G.uniform_csr(3125, 3125, 32, dtype=torch.float32)),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=",".join(MATRICES))
    ap.add_argument("--pairs", default=",".join(PAIRS))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--parent-lib", default=None, help="another build of libmspmv.so (the parent commit's): its wide call joins the alternation")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    for key in a.only.split(","):
        label, A = MATRICES[key]()
        for pair in a.pairs.split(","):
            print(json.dumps(run(label, A, pair, a.reps, a.parent_lib)), flush=True)
        del A
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
