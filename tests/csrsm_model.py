"""numpy model of the level-scheduled triangular solve for k right-hand sides (include/mspmv.h: mspmv_csrsm_*): the solve is
csrsv_model.solve applied to each column (that model is pinned to exact rational arithmetic by tests/test_csrsv.py); the lanes per
row, the passes and the segments (launches) given the lane budget follow the header's rules.  Nothing here calls the library."""
import numpy as np

import csrsv_model

MAX_LANES = 64


def solve(off, col, val, B, alpha=1.0, lower=True, unit=False):
    """column j of the result = csrsv_model.solve on column j of B"""
    B = np.asarray(B)
    X = np.zeros(B.shape, B.dtype)
    for j in range(B.shape[1]):
        X[:, j] = csrsv_model.solve(off, col, val, np.ascontiguousarray(B[:, j]), alpha, lower, unit)
    return X


def lanes_per_row(k):
    """P: the smallest power of two >= min(k, 64)"""
    p = 1
    while p < min(k, MAX_LANES):
        p *= 2
    return p


def passes(k):
    """ceil(k / 64): the right-hand sides one lane takes, one after the other"""
    return -(-k // MAX_LANES)


def segments(level_offsets, narrow_lanes, P):
    """[(first level, one past the last, narrow)]: a level of n rows is narrow when n * P <= narrow_lanes; a maximal run of narrow
    levels is one launch, every other level its own"""
    sizes = np.diff(np.asarray(level_offsets, np.int64))
    out, l = [], 0
    while l < len(sizes):
        if sizes[l] * P <= narrow_lanes:
            m = l
            while m < len(sizes) and sizes[m] * P <= narrow_lanes:
                m += 1
            out.append((l, m, True))
            l = m
        else:
            out.append((l, l + 1, False))
            l += 1
    return out


def launches(level_offsets, narrow_lanes, k):
    return len(segments(level_offsets, narrow_lanes, lanes_per_row(k)))
