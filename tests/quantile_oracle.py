"""Sort oracle and shared inputs for the quantile-leaf tests (CPU and GPU).

The oracle is independent of the radix select under test: a numpy stable
sort of the residuals plus a cumulative sum of the integer weights.
"""

import math

import numpy as np

CHUNK = 2048  # rows one workgroup chunk of leaf_quantile_hist covers


def fold(r):
    """fp32 with -0.0 folded into +0.0 (the documented residual form)."""
    return (np.asarray(r, np.float32) + np.float32(0.0)).astype(np.float32)


def threshold(alpha, w_total):
    return min(max(int(math.ceil(float(alpha) * float(w_total))), 1),
               int(w_total))


def oracle_quantile(resid, W, alpha):
    """Smallest residual v present with sum(W[resid <= v]) >= T, or None
    for a segment without weight."""
    r = fold(resid)
    W = np.asarray(W, np.int64)
    if r.size == 0 or int(W.sum()) == 0:
        return None
    order = np.argsort(r, kind="stable")
    cw = np.cumsum(W[order])
    T = threshold(alpha, cw[-1])
    return fold(r[order][int(np.searchsorted(cw, T, side="left"))])


def key_of(v):
    """Order-preserving uint32 key of one fp32 value (as a python int)."""
    u = int(fold(v).reshape(1).view(np.uint32)[0])
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def make_case(weighted, big=False, seed=0):
    """Residuals by row id, integer weights (or None), and 7 contiguous
    leaf segments of a shuffled row-index array (9 with ``big``: one
    segment longer than two chunks and one of chunk+1 rows)."""
    rng = np.random.RandomState(seed)
    parts = []
    a = rng.randn(1000).astype(np.float32)
    a[::50] = 0.0
    a[25::50] = -0.0
    parts.append(a)                                            # mixed signs
    parts.append(np.zeros(0, np.float32))                      # empty
    parts.append(np.array([-3.25], np.float32))                # single row
    parts.append(np.full(300, 0.7, np.float32))                # all equal
    j = rng.permutation(256).astype(np.float32)
    parts.append((np.float32(1.0) + j * np.float32(2.0 ** -23))
                 .astype(np.float32))                          # last byte only
    parts.append(rng.randint(-3, 4, 700).astype(np.float32))   # heavy ties
    parts.append((rng.randn(740) * np.exp(rng.randn(740) * 4))
                 .astype(np.float32))                          # wide exponents
    if big:
        parts.append(rng.randn(2 * CHUNK + 777).astype(np.float32))
        parts.append((rng.randn(CHUNK + 1) * 1e-3).astype(np.float32))
    counts = np.array([p.size for p in parts], np.int64)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    n = int(counts.sum())
    ridx = rng.permutation(n).astype(np.int32)
    resid = np.zeros(n, np.float32)
    resid[ridx] = np.concatenate(parts)
    W = None
    if weighted:
        W = rng.randint(0, 2 ** 30 + 1, n).astype(np.int64)
        W[rng.rand(n) < 0.1] = 0
        W[ridx[starts[5]]] = 2 ** 30
    return resid, W, ridx, starts, counts


def segment_oracle(resid, W, ridx, starts, counts, alpha):
    """Per-segment oracle quantile (None where the segment has no weight)."""
    out = []
    for s, c in zip(starts.tolist(), counts.tolist()):
        rows = ridx[s:s + c]
        w = np.ones(c, np.int64) if W is None else W[rows]
        out.append(oracle_quantile(resid[rows], w, alpha))
    return out
