#!/usr/bin/env python3
"""tools/trace_tiles.py [workload ...] -- development: per-phase cycle stamps inside tile_kernel_vec
(the ABLATE=6 build of the kernel writes clock64() at phase boundaries for the first 16 tiles of each block).
tools/trace_tiles.py clocked [c2 | c2d] -- the same for the clock-scheduled column bands (csrc/mspmv_tdm.hpp): eight wall-clock
stamps per block (thread 0), median and p90 of every interval of a tile's life on the automatic C2 call.
Needs the development library: make -C merge_spmv_amd exp && MSPMV_LIB=merge_spmv_amd/libmspmv_exp.so python tools/trace_tiles.py"""
import ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch, numpy as np
import merge_spmv_amd as M
import sweep
lib = M.load_library()
lib.mspmv_dev_set_trace.argtypes = [ctypes.c_void_p]


CLOCKED_POINTS = ["coordinates there", "stream there", "sorted words back in registers", "first gather issued", "last gather back",
                  "row ends there", "products done", "reduction done"]


def clocked(names):
    """One block per tile: stamp i of block b at word 8 b + i, in ticks of the 100 MHz wall clock (thread 0; wave 0's gathers).
    Where the kernel has the row ends before its rotation, "last gather back -> row ends there" is what is left of them behind it."""
    for label, A, x in sweep.workloads(names):
        vb = A.values.element_size()
        info = M.launch_info(A.rows, A.nnz, vb)
        assert M.band_passes(A.rows, A.cols, A.nnz, vb) >= 2, "not a call the clocked bands are offered"
        nblk = info["num_tiles"]
        # (room for the smallest tile shape any build has, 128 x 5 path items: the kernel stamps every block it launches)
        buf = torch.zeros(max(nblk, (A.rows + A.nnz) // 640 + 64) * 8, dtype=torch.int64, device="cuda")
        ws = M.CsrMVWorkspace(A.rows, A.nnz, A.values.dtype)
        y = torch.empty(A.rows, dtype=A.values.dtype, device="cuda")
        try:
            for _ in range(3):                       # (untraced: the verdicts, the caches)
                M.csrmv(A.values, A.row_offsets, A.column_indices, x, y=y, num_cols=A.cols, workspace=ws)
            torch.cuda.synchronize()
            assert lib.mspmv_dev_set_trace(ctypes.c_void_p(buf.data_ptr())) == 0
            M.csrmv(A.values, A.row_offsets, A.column_indices, x, y=y, num_cols=A.cols, workspace=ws)
            torch.cuda.synchronize()
        finally:
            assert lib.mspmv_dev_set_trace(ctypes.c_void_p(0)) == 0
        t = buf.cpu().numpy()[:nblk * 8].reshape(nblk, 8).astype(np.float64)
        ok = (t > 0).all(axis=1)
        # steady state: not the first blocks of the launch (every CU fills at once) nor the drain
        order = np.argsort(t[:, 0]); lo, hi = int(0.15 * nblk), int(0.85 * nblk)
        steady = np.zeros(nblk, bool); steady[order[lo:hi]] = True
        sel = t[ok & steady] / 100.0                 # microseconds
        print(f"== {label}: tile {info['block_threads']}x{info['items_per_thread']}, {nblk} tiles, {int(ok.sum())} fully stamped, {len(sel)} in the steady "
              f"state; kernel {(t[ok][:, 7].max() - t[ok][:, 0].min()) / 100.0:.1f} us from first to last stamp")
        print(f"  {'interval (us)':58s} {'median':>8s} {'p90':>8s}")
        for i in range(1, 8):
            d = sel[:, i] - sel[:, i - 1]
            print(f"  {CLOCKED_POINTS[i - 1] + ' -> ' + CLOCKED_POINTS[i]:58s} {np.median(d):8.2f} {np.percentile(d, 90):8.2f}")
        life = sel[:, 7] - sel[:, 0]
        rot = sel[:, 4] - sel[:, 3]
        print(f"  {'whole life':58s} {np.median(life):8.2f} {np.percentile(life, 90):8.2f}")
        print(f"  {'life outside the rotation (whole - first..last gather)':58s} {np.median(life - rot):8.2f} {np.percentile(life - rot, 90):8.2f}")


def sweep_body(names):
    for label, A, x in sweep.workloads(names):
        vb = A.values.element_size()
        info = M.launch_info(A.rows, A.nnz, vb)
        M.set_tuning(vb, info["block_threads"], info["items_per_thread"], 0x60000 | 0x400)    # stamps build, resident grid of 4 blocks per CU
        nblk = 4 * 256 + 64
        buf = torch.zeros(nblk * 16 * 8, dtype=torch.int64, device="cuda")
        assert lib.mspmv_dev_set_trace(ctypes.c_void_p(buf.data_ptr())) == 0
        ws = M.CsrMVWorkspace(A.rows, A.nnz, A.values.dtype)
        y = torch.empty(A.rows, dtype=A.values.dtype, device="cuda")
        for _ in range(3):
            buf.zero_()
            M.csrmv(A.values, A.row_offsets, A.column_indices, x, y=y, num_cols=A.cols, workspace=ws)
        torch.cuda.synchronize()
        assert lib.mspmv_dev_set_trace(ctypes.c_void_p(0)) == 0
        t = buf.cpu().numpy().reshape(nblk, 16, 8).astype(np.float64)
        print("  stamps recorded per slot:", [(int((t[:, :, i] > 0).sum())) for i in range(8)])
        ok = (t[:, :, 5] > 0) & (t[:, :, 0] > 0)
        ok[:, :2] = False            # steady state only
        ok[:, 12:] = False
        sel = t[ok]
        print(f"== {label}: tile {info['block_threads']}x{info['items_per_thread']}, {ok.sum()} traced tiles (cycles of the 100 MHz*? shader clock; averages)")
        def d(a, b): return float(np.mean(sel[:, b] - sel[:, a]))
        print(f"  wait for the tile's stream loads (issued one iteration ago) : {d(0,1):8.0f}")
        print(f"  staging: row offsets + x gathers + products/flags to LDS + barrier: {d(1,2):8.0f}")
        print(f"  issue next tile's loads                                     : {d(2,3):8.0f}")
        print(f"  nonzero phase up to the block scan                          : {d(3,6):8.0f}")
        print(f"  block scan + carry + S write + barrier                      : {d(6,7):8.0f}")
        print(f"  row phase (y stores) + carry-out                            : {d(7,4):8.0f}")
        print(f"  end-of-tile barrier                                         : {d(4,5):8.0f}")
        # iteration period: stamp 0 of consecutive tiles
        per = t[:, 3:12, 0] - t[:, 2:11, 0]
        okp = (t[:, 3:12, 0] > 0) & (t[:, 2:11, 0] > 0) & (t[:, 3:12, 5] > 0)
        print(f"  whole iteration                                             : {float(np.mean(per[okp])):8.0f}")
        M.set_tuning(vb)


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "clocked":
        clocked(args[1:] or ["c2"])
    else:
        sweep_body(args or ["dense32d"])
