"""Inputs and oracle results for the multiclass AUC kernels, built once.

The device ``exp`` may differ from numpy's by a few ulps, so a row whose
``p_k * n_bins`` lay next to an inner bin edge could land on either side.
Every case asserts, on the reference alone, that none does. The guard, in
ulps of ``p_k * n_bins``: one ``exp`` per value (each side within 2 ulps of
the true value: 4 apart), K - 1 adds into s (the terms are positive, so s
inherits the 4 and gains at most 1 per add), one divide (the errors of e_k
and s, and 1) and one multiply (1): 4 + 4 + (K - 1) + 2 = K + 9, taken as
K + 16 with the binary cases' allowance (``aux_cases.AUC_EDGE_ULPS``).
A row of all-equal margins is exact on both sides (exp(0) = 1, s = K) and is
left out, as the binary cases leave margin 0 out."""

import functools

import numpy as np
import torch

from xgboost_ray_amd import ops
from xgboost_ray_amd.ops.cpu import _softmax_rows

# (K, n, n_bins, weighted): K and n paired as a Latin square
CASES = [
    (2, 1, 16384, True), (3, 257, 2, False), (16, 16385, 1000, True),
    (17, 70001, 16384, False), (33, 257, 16384, True), (2, 70001, 1000, False),
    (3, 16385, 16384, False), (17, 1, 2, False), (33, 16385, 2, False),
    (16, 257, 16384, False),
]


def edge_guard_ulps(K):
    return K + 16


def edge_distance_ulps(x, y, B):
    """Smallest distance, in ulps of p * B, of a value from an inner bin edge
    (edges 1 .. B-1), over the rows whose margins are not all equal."""
    d, e, s, _ = _softmax_rows(torch.from_numpy(x), torch.from_numpy(y))
    with np.errstate(invalid="ignore"):
        t = (e / s[:, None]) * float(B)
        k = np.rint(t)
        inner = (k >= 1) & (k <= B - 1) & (d != 0).any(1, keepdims=True)
    if not inner.any():
        return np.inf
    return float((np.abs(t - k)[inner] / np.spacing(t[inner])).min())


@functools.lru_cache(maxsize=None)
def case(K, n, B, weighted):
    """([margin, label, weight] CPU tensors, oracle int64 [K, 2, B])."""
    rng = np.random.RandomState(1000 * K + n % 997 + B)
    x = (rng.randn(n, K) * 3).astype(np.float32)
    y = rng.randint(0, K, n).astype(np.float32)
    if n >= 257:
        y[:3] = [-1.0, K, 2.7]          # no class, no class, class 2 (or none)
        x[70, K - 1] = np.nan           # a NaN row: bin 0 of every class
        x[130, 0] = np.inf              # inf - inf: NaN as well
        x[200] = 0.75                   # all equal: p = 1 / K exactly
    w = None
    if weighted:
        w = rng.uniform(0.25, 4, n).astype(np.float32)
        w[5::7] = 0.0
        w[3::11] = 2.0 ** -22           # under 2^-21: rounds to W = 0
    dist = edge_distance_ulps(x, y, B)
    assert dist > edge_guard_ulps(K), (K, n, B, dist)
    t = [torch.from_numpy(x), torch.from_numpy(y),
         None if w is None else torch.from_numpy(w)]
    ref = ops.cpu.eval_auc_multiclass(*t, n_bins=B)
    mass = n if w is None else int(
        np.rint(w.astype(np.float64) * 2.0 ** 20).sum())
    assert (ref.sum((1, 2)) == mass).all()
    return t, ref, mass
