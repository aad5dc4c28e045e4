"""What the library says about itself and the aids for measuring and testing it: the launch layout of a call, the column-band
queries, the setters of the development library (include/mspmv_dev.h), the profiling pair, the debug readers and the sampled
correctness witness of bench.py."""
from __future__ import annotations

import ctypes
from typing import Optional

from ._lib import _LaunchInfo, _check, _setter, load_library
from ._args import _stream_handle


def launch_info(num_rows: int, num_nonzeros: int, value_bytes: int, num_cols: Optional[int] = None) -> dict:
    """mspmv_get_launch_info; with `num_cols` mspmv_get_launch_info_cols: exactly the layout a stateless call of these sizes runs (one
    family of calls -- large fp64 matrices of short rows over a tiny x -- picks its tile shape by the column count too)."""
    info = _LaunchInfo()
    if num_cols is None:
        _check(load_library().mspmv_get_launch_info(int(num_rows), int(num_nonzeros), int(value_bytes),
                                                    ctypes.byref(info)), "mspmv_get_launch_info")
    else:
        _check(load_library().mspmv_get_launch_info_cols(int(num_rows), int(num_cols), int(num_nonzeros), int(value_bytes),
                                                         ctypes.byref(info)), "mspmv_get_launch_info_cols")
    return {name: getattr(info, name) for name, _ in _LaunchInfo._fields_}


def serial_sum_depth(num_rows: int, num_cols: int, num_nonzeros: int, value_bytes: int, extra: int = 0) -> int:
    """How many products one thread of the tile kernel adds up serially before the scan tree takes over, for a call of these
    sizes -- the compiled tile's items per thread rounded up to whole 4-element chunks -- plus one re-association per
    column-band pass the call may run, plus `extra` (parts of a multi-GPU split, bands of a prepared plan).  It is the
    `items_per_thread` term of the stated error bound |y - g| <= 2 (ceil(log2(len + 1)) + items_per_thread + 8) eps s
    (DESIGN.md 3): derived from the compiled shape, so the bound follows the library when a shape changes."""
    ipt = launch_info(num_rows, num_nonzeros, value_bytes)["items_per_thread"]
    return 4 * (ipt // 4 + 1) + max(band_passes(num_rows, num_cols, num_nonzeros, value_bytes), 0) + int(extra)


def set_tuning(value_bytes: int, block_threads: int = 0, items_per_thread: int = 0, flags: int = 0) -> None:
    """mspmv_set_tuning (development library: a non-default value switches to it, see _setter)."""
    _setter("mspmv_set_tuning", block_threads == 0 and items_per_thread == 0 and flags == 0,
            int(value_bytes), int(block_threads), int(items_per_thread), int(flags))


def profile_begin(max_calls: int) -> None:
    """Record hipEvents around the three kernels of the next `max_calls` CsrMV calls."""
    _check(load_library().mspmv_profile_begin(int(max_calls)), "mspmv_profile_begin")


def profile_end() -> dict:
    """Average per-call milliseconds of each pass since profile_begin()."""
    calls = ctypes.c_int32()
    ms = [ctypes.c_float() for _ in range(3)]
    _check(load_library().mspmv_profile_end(ctypes.byref(calls), *[ctypes.byref(m) for m in ms]), "mspmv_profile_end")
    return {"calls": calls.value, "search_ms": ms[0].value, "tile_ms": ms[1].value, "fixup_ms": ms[2].value}


def set_band_passes(value_bytes: int, passes: int = 0) -> None:
    """Column-band passes (mspmv_set_band_passes): 0 automatic, < 0 never, >= 2 always that many."""
    _setter("mspmv_set_band_passes", passes == 0, int(value_bytes), int(passes))


def set_tdm(value_bytes: int, policy: int = 0, slot_permille: int = 0, lookahead_plus_1: int = 0, band_shift: int = 0) -> None:
    """Clock-scheduled column bands (mspmv_set_tdm): policy 0 the library's rule, < 0 never (the passes), > 0 always where the passes are offered."""
    _setter("mspmv_set_tdm", policy == 0 and slot_permille == 0 and lookahead_plus_1 == 0 and band_shift == 0,
            int(value_bytes), int(policy), int(slot_permille), int(lookahead_plus_1), int(band_shift))


def device_caches() -> dict:
    """What the column-band policy is derived from (mspmv_get_device_caches): one XCD's L2 bytes, XCD count, CU count."""
    l2 = ctypes.c_int64(0); x = ctypes.c_int32(0); c = ctypes.c_int32(0)
    _check(load_library().mspmv_get_device_caches(ctypes.byref(l2), ctypes.byref(x), ctypes.byref(c)), "mspmv_get_device_caches")
    return {"l2_bytes_per_xcd": l2.value, "xcds": x.value, "cus": c.value}


def set_record_polls(polls: int = 0) -> None:
    """Testing aid (mspmv_set_record_polls): 0 = library default, 1 = one look, -1 = never look: tiles in which a long row ends
    compute the pieces held by other workgroups themselves instead of taking the published records."""
    _setter("mspmv_set_record_polls", polls == 0, int(polls))


def cache_stream_rate(nbytes: int, reps: int = 20) -> float:
    """GB/s of a bare 16-byte-per-lane read stream (mspmv_probe_read_stream, ordinary loads) over a buffer of `nbytes` that has been
    read before -- for nbytes within the 256 MB Infinity Cache this is the rate out of that cache (and the L2s), the bound a
    cache-resident SpMV's algorithmic bytes are to be read against (bench.py)."""
    import time
    import torch
    lib = load_library()
    n = max(int(nbytes) // 16 * 16, 16)
    buf = torch.zeros(n, dtype=torch.uint8, device="cuda")
    st = _stream_handle(None)
    for _ in range(3):
        _check(lib.mspmv_probe_read_stream(ctypes.c_void_p(buf.data_ptr()), n, 0, st), "mspmv_probe_read_stream")
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        lib.mspmv_probe_read_stream(ctypes.c_void_p(buf.data_ptr()), n, 0, st)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    del buf
    return n / dt / 1e9


def set_compact_tiles(max_tiles: int = 0) -> None:
    """Testing / tuning aid (mspmv_set_compact_tiles): up to how many tiles a call of the small tile shape runs the one-launch kernel
    behind its compact front end (0 = library default, > 0 = that many, < 0 = never).  y is bit for bit the same either way."""
    _setter("mspmv_set_compact_tiles", max_tiles == 0, int(max_tiles))


def clocked_bands(rows: int, cols: int, nnz: int, value_bytes: int):
    """(bands, columns per band) of the clock-scheduled form for a call of these sizes (mspmv_get_clocked_bands); (0, 0): not a candidate."""
    b = ctypes.c_int32(0); c = ctypes.c_int32(0)
    _check(load_library().mspmv_get_clocked_bands(int(rows), int(cols), int(nnz), int(value_bytes), ctypes.byref(b), ctypes.byref(c)), "mspmv_get_clocked_bands")
    return b.value, c.value


def band_passes(rows: int, cols: int, nnz: int, value_bytes: int) -> int:
    """Passes a call of these sizes is offered (0: none); automatic setting: subject to the device-side verdicts."""
    n = ctypes.c_int32(0)
    _check(load_library().mspmv_get_band_passes(int(rows), int(cols), int(nnz), int(value_bytes), ctypes.byref(n)), "mspmv_get_band_passes")
    return n.value


def debug_band_windows(workspace, rows: int, nnz: int, value_bytes: int):
    """The 64 window verdicts the last automatic large-problem call left in the workspace (numpy int32[64])."""
    import numpy as np
    out = np.zeros(64, np.int32)
    tmp = workspace.buffer if hasattr(workspace, "buffer") else workspace
    _check(load_library().mspmv_debug_band_windows(ctypes.c_void_p(tmp.data_ptr()), int(rows), int(nnz), int(value_bytes),
                                                   out.ctypes.data_as(ctypes.c_void_p), None), "mspmv_debug_band_windows")
    return out


def debug_read_tiles(workspace_buffer, num_rows: int, num_nonzeros: int, value_bytes: int, stream=None):
    """(coords[num_tiles+1, 2], carry_keys[num_tiles], carry_values[num_tiles])
    left in temp storage by the last CsrMV call, as numpy arrays."""
    import numpy as np
    info = launch_info(num_rows, num_nonzeros, value_bytes)
    nt = info["num_tiles"]
    coords = np.zeros((nt + 1, 2), dtype=np.int32)
    keys = np.zeros(max(nt, 1), dtype=np.int32)
    vals = np.zeros(max(nt, 1), dtype=np.float32 if value_bytes == 4 else np.float64)
    _check(load_library().mspmv_debug_read_tiles(
        ctypes.c_void_p(workspace_buffer.data_ptr()), int(num_rows), int(num_nonzeros), int(value_bytes),
        coords.ctypes.data_as(ctypes.c_void_p), keys.ctypes.data_as(ctypes.c_void_p),
        vals.ctypes.data_as(ctypes.c_void_p), _stream_handle(stream)), "mspmv_debug_read_tiles")
    return coords, keys[:nt], vals[:nt]


def sampled_check(A, x, y, samples: int = 1 << 16, seed: int = 0x5A3D, depth: Optional[int] = None) -> dict:
    """An untimed correctness witness for a benchmark record (NOT the parity tests: those are tests/ -m gpu against the oracle):
    `samples` seeded rows -- plus the first, the last and the longest row -- recomputed on the device in fp64 with torch gathers
    (val.double() * x.double()[col], rows up to 4096 nonzeros by index_add_, longer ones by torch.sum's tree) and compared with
    y under the stated bound of SURVEY 8d / DESIGN 3: |y - g| <= 2 (ceil(log2(len + 1)) + depth + 8) eps s, s = sum |val x|,
    eps = 2^-24 / 2^-53, empty rows exactly zero.  depth = serial_sum_depth of the call's shape unless given.
    Returns {"rows_checked", "worst_ratio" (max |y - g| / bound; < 1 passes), "violations", "longest_row"}."""
    import torch
    rows, nnz = int(A.rows), int(A.nnz)
    dev = A.values.device
    if rows == 0:
        return {"rows_checked": 0, "worst_ratio": 0.0, "violations": 0, "longest_row": 0}
    vb = A.values.element_size()
    if depth is None:
        depth = serial_sum_depth(rows, A.cols, nnz, vb)
    eps = 2.0 ** -24 if vb == 4 else 2.0 ** -53
    off = A.row_offsets.to(torch.int64)
    lens_all = off[1:] - off[:-1]
    g = torch.Generator(device="cpu"); g.manual_seed(int(seed))
    pick = torch.randint(0, rows, (min(int(samples), rows),), generator=g, dtype=torch.int64).to(dev)
    longest = int(torch.argmax(lens_all).item())
    pick = torch.unique(torch.cat([pick, torch.tensor([0, rows - 1, longest], dtype=torch.int64, device=dev)]))
    lens = lens_all[pick]
    start = off[pick]
    gold = torch.zeros(pick.numel(), dtype=torch.float64, device=dev)
    mag = torch.zeros_like(gold)
    xd = x.double()
    short = lens <= 4096
    if bool(short.any()):
        sl = lens[short]; st = start[short]
        total = int(sl.sum().item())
        if total > 0:
            seg = torch.repeat_interleave(torch.arange(sl.numel(), device=dev), sl)
            first = torch.cumsum(sl, 0) - sl
            j = st[seg] + (torch.arange(total, device=dev) - first[seg])
            p = A.values[j].double() * xd[A.column_indices[j].to(torch.int64)]
            gs = torch.zeros(sl.numel(), dtype=torch.float64, device=dev); ms = torch.zeros_like(gs)
            gs.index_add_(0, seg, p); ms.index_add_(0, seg, p.abs())
            gold[short] = gs; mag[short] = ms
    for k in torch.nonzero(~short).flatten().tolist():          # a handful of long rows: tree sums
        a, b = int(start[k].item()), int(start[k].item() + lens[k].item())
        gk, mk = 0.0, 0.0
        for c0 in range(a, b, 1 << 26):
            c1 = min(b, c0 + (1 << 26))
            p = A.values[c0:c1].double() * xd[A.column_indices[c0:c1].to(torch.int64)]
            gk += float(p.sum().item()); mk += float(p.abs().sum().item())
        gold[k] = gk; mag[k] = mk
    yy = y[pick].double()
    c = 2.0 * (torch.ceil(torch.log2(lens.double() + 1.0)) + float(depth) + 8.0)
    bound = c * eps * mag
    err = (yy - gold).abs()
    bad_empty = (lens == 0) & (y[pick] != 0)
    ratio = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    ratio = torch.where(torch.isfinite(yy), ratio, torch.full_like(ratio, float("inf")))
    ratio = torch.where(bad_empty, torch.full_like(ratio, float("inf")), ratio)
    worst = float(ratio.max().item())
    return {"rows_checked": int(pick.numel()), "worst_ratio": round(worst, 4) if worst != float("inf") else "inf",
            "violations": int((ratio > 1.0).sum().item()), "longest_row": int(lens_all[longest].item()), "depth_term": int(depth)}
