"""An exact, formula-defined CSR family for tests at the top of the accepted index range (rows + nnz up to MAX_ITEMS) and for
arrays over 4 GB (tests/test_index_range.py).

Every quantity is a closed formula of its index, evaluated with int64 arithmetic in chunks on the tensors' device (torch) or with
Python integers on the host, so the test's own generator cannot wrap at 2^31 and nothing of size nnz has to reach the host:

  row lengths   all rows but one ("the absorbing row", by default the last) come in pairs (2i, 2i+1) of lengths mid + d_i and
                mid - d_i, d_i = hash(i) in [-spread, spread]; the absorbing row takes the remainder, so rows + nnz is exactly
                the target.  The start of row r is then a closed formula too (a pair sums to 2 mid).
  columns       stratified within a row: col(k) = floor((j * cols + u_k) / len), j = k's place in its row, u_k = hash(k) mod cols,
                so the columns of a row never decrease and span [0, cols); nonzero 0 sits in column 0 and the last nonzero in
                column cols - 1.
  values, x     v(k), x(c) = hashes mapped onto the nonzero integers in [-8, 8].

Every product is then an integer of magnitude <= 64, every partial sum of a row of length L one of magnitude <= 64 L: an fp64 y
is exact whatever the association order (64 * 2^31 < 2^53), and so is an fp32 y on rows of at most 2^18 nonzeros (<= 2^24).
The reference y_ref[r] = P[off[r+1]] - P[off[r]], P the running int64 prefix sum of v(k) x(col(k)), is exact as well and uses
no atomics and nothing of the library; s[r] = sum |v x| comes the same way.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

from merge_spmv_amd.generators import splitmix64

MAX_ITEMS = 0x7FFFFFFF - 65536            # include/mspmv.h / mspmv_internal.hpp: the largest rows + nnz one call accepts
CHUNK = 1 << 27
SEED_LEN, SEED_COL, SEED_VAL, SEED_X = 0x1D0001, 0x1D0002, 0x1D0003, 0x1D0004
_M64 = (1 << 64) - 1
_M63 = (1 << 63) - 1


# ---------------------------------------------------------------------------------------------------------------------------
# the hashes, on int64 tensors and on Python ints (bit for bit the same)

def _hash_t(seed: int, idx: torch.Tensor) -> torch.Tensor:
    """non-negative int64 hash of int64 counters"""
    return splitmix64(seed, idx) & _M63


def _hash_i(seed: int, i: int) -> int:
    z = (i * 0x9E3779B97F4A7C15 + seed + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return (z ^ (z >> 31)) & _M63


def _small_t(seed: int, idx: torch.Tensor) -> torch.Tensor:
    t = _hash_t(seed, idx) & 15
    return t - 8 + (t >= 8).to(torch.int64)            # {-8..-1, 1..8}


def _small_i(seed: int, i: int) -> int:
    t = _hash_i(seed, i) & 15
    return t - 8 + (1 if t >= 8 else 0)


def x_seed(j: int = 0) -> int:
    """seed of the j-th x vector of a family (csrmm uses several)"""
    return SEED_X + 0x100 * j


# ---------------------------------------------------------------------------------------------------------------------------

def rows_for(items: int, mid: int) -> int:
    """the largest odd row count whose regular rows (mean length mid) leave the absorbing row 0..2 mid + 1 nonzeros for
    rows + nnz = items"""
    rows = (items + mid) // (mid + 1)
    return rows if rows % 2 == 1 else rows - 1


@dataclass(frozen=True)
class Family:
    rows: int
    cols: int
    items: int                 # rows + nnz
    mid: int
    spread: int
    absorb: int = -1           # the row that takes the remainder (-1: the last)
    seed: int = 0

    def __post_init__(self):
        assert self.rows >= 1 and self.cols >= 1 and 0 <= self.spread <= self.mid
        assert (self.rows - 1) % 2 == 0, "the regular rows come in pairs: rows must be odd"
        assert self.items <= MAX_ITEMS + 1
        assert self.absorb_len >= 0, f"target {self.items} below the regular rows' {self.rows - 1 + self.mid * (self.rows - 1)}"

    @property
    def g(self) -> int:
        return self.rows - 1 if self.absorb < 0 else self.absorb

    @property
    def nnz(self) -> int:
        return self.items - self.rows

    @property
    def absorb_len(self) -> int:
        return self.nnz - self.mid * (self.rows - 1)

    def max_len(self) -> int:
        return max(self.absorb_len, self.mid + self.spread)

    # ---- host: Python ints ----
    def _d(self, i: int) -> int:
        return _hash_i(SEED_LEN + self.seed, i) % (2 * self.spread + 1) - self.spread

    def length(self, r: int) -> int:
        if r == self.g:
            return self.absorb_len
        q = r if r < self.g else r - 1
        d = self._d(q // 2)
        return self.mid + d if q % 2 == 0 else self.mid - d

    def offset(self, r: int) -> int:
        """row_offsets[r], 0 <= r <= rows"""
        q = r if r <= self.g else r - 1
        o = q * self.mid + (self._d(q // 2) if q % 2 == 1 else 0)
        return o + (self.absorb_len if r > self.g else 0)

    def row_of(self, k: int) -> int:
        """the row holding nonzero k"""
        lo, hi = 0, self.rows - 1                  # the largest r with offset(r) <= k
        while lo < hi:
            m = (lo + hi + 1) // 2
            if self.offset(m) <= k:
                lo = m
            else:
                hi = m - 1
        return lo

    def row_at_item(self, d: int) -> int:
        """the row the merge path is in at diagonal d (rows + nonzeros consumed = d): smallest r with r + offset(r+1) >= d"""
        lo, hi = 0, self.rows - 1
        while lo < hi:
            m = (lo + hi) // 2
            if m + self.offset(m + 1) >= d:
                hi = m
            else:
                lo = m + 1
        return lo

    def col(self, k: int) -> int:
        if k == 0:
            return 0
        if k == self.nnz - 1:
            return self.cols - 1
        r = self.row_of(k)
        o, n = self.offset(r), self.length(r)
        return ((k - o) * self.cols + _hash_i(SEED_COL + self.seed, k) % self.cols) // n

    def value(self, k: int) -> int:
        return _small_i(SEED_VAL + self.seed, k)

    def xval(self, c: int, j: int = 0) -> int:
        return _small_i(x_seed(j) + self.seed, c)

    def row_sum(self, r: int, j: int = 0):
        """(y_ref[r], s[r]) with Python ints"""
        y = s = 0
        for k in range(self.offset(r), self.offset(r + 1)):
            p = self.value(k) * self.xval(self.col(k), j)
            y += p; s += abs(p)
        return y, s

    # ---- device: int64 tensors, chunk by chunk ----
    def offsets_t(self, lo: int, hi: int, device) -> torch.Tensor:
        """row_offsets[lo:hi] as int64"""
        r = torch.arange(lo, hi, dtype=torch.int64, device=device)
        q = torch.where(r <= self.g, r, r - 1)
        d = _hash_t(SEED_LEN + self.seed, q // 2) % (2 * self.spread + 1) - self.spread
        o = q * self.mid + torch.where(q % 2 == 1, d, torch.zeros_like(d))
        return o + torch.where(r > self.g, torch.full_like(o, self.absorb_len), torch.zeros_like(o))

    def row_offsets(self, device) -> torch.Tensor:
        out = torch.empty(self.rows + 1, dtype=torch.int32, device=device)
        for lo in range(0, self.rows + 1, CHUNK):
            hi = min(lo + CHUNK, self.rows + 1)
            out[lo:hi] = self.offsets_t(lo, hi, device).to(torch.int32)
        return out

    def rows_t(self, k: torch.Tensor, off32: torch.Tensor) -> torch.Tensor:
        """row of each nonzero k (int64) given the device row offsets (a sorted int32 tensor)"""
        return torch.searchsorted(off32, k.to(torch.int32), right=True).to(torch.int64) - 1

    def cols_t(self, k: torch.Tensor, off32: torch.Tensor) -> torch.Tensor:
        r = self.rows_t(k, off32)
        o = off32[r].to(torch.int64)
        n = off32[r + 1].to(torch.int64) - o
        c = ((k - o) * self.cols + _hash_t(SEED_COL + self.seed, k) % self.cols) // n
        c = torch.where(k == 0, torch.zeros_like(c), c)
        return torch.where(k == self.nnz - 1, torch.full_like(c, self.cols - 1), c)

    def values_t(self, k: torch.Tensor) -> torch.Tensor:
        return _small_t(SEED_VAL + self.seed, k)

    def x_t(self, c: torch.Tensor, j: int = 0) -> torch.Tensor:
        return _small_t(x_seed(j) + self.seed, c)

    def chunks(self, n: int = None, chunk: int = None):
        n = self.nnz if n is None else n
        chunk = CHUNK if chunk is None else chunk
        for lo in range(0, n, chunk):
            yield lo, min(lo + chunk, n)

    def build(self, dtype, device, pad: int = 0):
        """(values, row_offsets, column_indices) on `device`; pad > 0: values and column_indices are views that start `pad`
        elements into their allocations (unaligned arrays)"""
        off = self.row_offsets(device)
        vals = torch.empty(self.nnz + pad, dtype=dtype, device=device)[pad:]
        cols = torch.empty(self.nnz + pad, dtype=torch.int32, device=device)[pad:]
        for lo, hi in self.chunks():
            k = torch.arange(lo, hi, dtype=torch.int64, device=device)
            cols[lo:hi] = self.cols_t(k, off).to(torch.int32)
            vals[lo:hi] = self.values_t(k).to(dtype)
        return vals, off, cols

    def x(self, dtype, device, j: int = 0, n: int = None) -> torch.Tensor:
        n = self.cols if n is None else n
        out = torch.empty(n, dtype=dtype, device=device)
        for lo, hi in self.chunks(n):
            out[lo:hi] = self.x_t(torch.arange(lo, hi, dtype=torch.int64, device=device), j).to(dtype)
        return out

    def reference(self, off32: torch.Tensor, j: int = 0):
        """(y_ref, s) int64 [rows]: exact, from the running int64 prefix sum of v(k) x(col(k)) carried from chunk to chunk"""
        dev = off32.device
        p_at = torch.zeros(self.rows + 1, dtype=torch.int64, device=dev)     # P[off[r]]
        s_at = torch.zeros(self.rows + 1, dtype=torch.int64, device=dev)
        carry_p = carry_s = 0
        for lo, hi in self.chunks():
            k = torch.arange(lo, hi, dtype=torch.int64, device=dev)
            p = self.values_t(k) * self.x_t(self.cols_t(k, off32), j)
            cp = torch.cumsum(p, 0) + carry_p
            cs = torch.cumsum(p.abs(), 0) + carry_s
            # the row starts in (lo, hi]: P[off] is the prefix through nonzero off - 1
            a = int(torch.searchsorted(off32, torch.tensor([lo], dtype=torch.int32, device=dev), right=True))
            b = int(torch.searchsorted(off32, torch.tensor([hi], dtype=torch.int32, device=dev), right=True))
            if b > a:
                at = off32[a:b].to(torch.int64) - 1 - lo
                p_at[a:b] = cp[at]
                s_at[a:b] = cs[at]
            carry_p, carry_s = int(cp[-1]), int(cs[-1])
            del k, p, cp, cs
        return p_at[1:] - p_at[:-1], s_at[1:] - s_at[:-1]

    def check_rows(self, rows_to_check):
        """host-side values of the formulas at the given rows: {r: (offset, length, y_ref or None, s or None)}; the sums only for
        rows short enough to add up with Python ints"""
        out = {}
        for r in rows_to_check:
            n = self.length(r)
            ys = self.row_sum(r) if n <= 4096 else (None, None)
            out[r] = (self.offset(r), n) + ys
        return out

    def probe_rows(self, tile_items: int = 0, num_tiles: int = 0, extra: int = 64):
        """~100 rows where an index wrap would show: the first and last rows, the rows around nonzero / merge-path item 2^30 and
        2^31 - 2^16, the rows at the last three tile boundaries, the absorbing row and its neighbours, and `extra` hashed rows"""
        picks = {0, 1, self.rows - 2, self.rows - 1, self.g, max(self.g - 1, 0), min(self.g + 1, self.rows - 1)}
        for item in (1 << 30, (1 << 31) - (1 << 16), self.nnz - 1, self.items - 1):
            if item < self.nnz:
                picks.add(self.row_of(item))
            if item < self.items:
                picks.add(self.row_at_item(item))
        for t in range(max(num_tiles - 3, 0), num_tiles + 1):
            d = min(t * tile_items, self.items)
            r = self.row_at_item(d)
            picks.update((max(r - 1, 0), r, min(r + 1, self.rows - 1)))
        for i in range(extra):
            picks.add(_hash_i(0x51DE, i) % self.rows)
        return sorted(p for p in picks if 0 <= p < self.rows)


# ---------------------------------------------------------------------------------------------------------------------------
# comparisons on the device; only a summary comes back

def mismatch_summary(y: torch.Tensor, y_ref: torch.Tensor, off32: torch.Tensor):
    """None when y equals y_ref exactly (both read as fp64; y_ref < 2^53), else (count, first bad row, its nonzero range,
    got, want)"""
    yd, rd = y.to(torch.float64), y_ref.to(torch.float64)
    if torch.equal(yd, rd):
        return None
    bad = (yd != rd) | torch.isnan(yd)
    n = int(bad.sum())
    r = int(torch.nonzero(bad)[0])
    return n, r, (int(off32[r]), int(off32[r + 1])), float(yd[r]), float(rd[r])


def strict_violations(y: torch.Tensor, y_ref: torch.Tensor, s: torch.Tensor, off32: torch.Tensor, depth: int):
    """|y - y_ref| <= 2 (ceil(log2(len + 1)) + depth + 8) eps s, y_ref and s exact; returns (violations,
    worst ratio)"""
    eps = 2.0 ** -24 if y.dtype == torch.float32 else 2.0 ** -53
    lens = (off32[1:] - off32[:-1]).to(torch.float64)
    bound = 2.0 * (torch.ceil(torch.log2(lens + 1.0)) + depth + 8) * eps * s.to(torch.float64)
    err = (y.to(torch.float64) - y_ref.to(torch.float64)).abs()
    ratio = torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones_like(bound)),
                        torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    ratio = torch.nan_to_num(ratio, nan=math.inf)             # (a NaN in y)
    return int((ratio > 1).sum()), float(ratio.max())
