"""ops.cpu.weighted_cuts (the sort-based oracle) against the definition
itself, and the radix-select route of ops.weighted_cuts against the oracle
on CPU tensors."""

import numpy as np
import pytest
import torch

from tests.sketch_cases import col_max, hessian_like, matrix
from xgboost_ray_amd import ops


def _brute(col, w, nb):
    """Expand each row w times, sort, index: v_j = sorted[T_j - 1]."""
    ok = ~np.isnan(col)
    rep = np.sort(np.repeat(col[ok] + np.float32(0.0), np.maximum(w[ok], 0)))
    if not ok.any():
        return []
    vals = {float(rep[-(-j * len(rep) // nb) - 1])
            for j in range(1, nb) if len(rep)}
    above = float(np.nextafter(np.float32(np.nanmax(col)), np.float32(np.inf)))
    return sorted(vals | {above})


@pytest.mark.parametrize("max_bin", [2, 3, 7, 256])
@pytest.mark.parametrize("seed", [0, 1])
def test_oracle_is_the_definition(max_bin, seed):
    rng = np.random.RandomState(seed)
    n = 41
    X = np.stack([
        rng.randn(n), rng.randint(-2, 3, n).astype(np.float64),
        np.full(n, np.nan), np.where(rng.rand(n) < 0.3, np.nan, rng.rand(n)),
        np.zeros(n)], 1).astype(np.float32)
    X[0, 1], X[1, 1] = -0.0, 0.0
    W = rng.randint(-1, 4, n).astype(np.int64)
    cuts = ops.cpu.weighted_cuts(
        torch.from_numpy(X), torch.from_numpy(W), max_bin, col_max(X))
    ptr = cuts.cut_ptr.numpy()
    for f in range(X.shape[1]):
        got = cuts.cuts_flat.numpy()[ptr[f]:ptr[f + 1]].tolist()
        assert got == _brute(X[:, f], W, min(max_bin, 255)), f
    assert cuts.max_bins == max(1, int(np.diff(ptr).max()))


def test_unit_weights_by_hand():
    """Ten distinct values, nb = 5: T_j = 2j, so v_j = sorted[2j - 1]."""
    col = np.array([7, 3, 9, 1, 5, 0, 8, 2, 6, 4], np.float32)[:, None]
    cuts = ops.cpu.weighted_cuts(
        torch.from_numpy(col), torch.ones(10, dtype=torch.int32), 5,
        col_max(col))
    want = [1.0, 3.0, 5.0, 7.0, float(np.nextafter(np.float32(9), np.float32(10)))]
    assert cuts.cuts_flat.tolist() == want
    assert cuts.cut_ptr.tolist() == [0, 5] and cuts.max_bins == 5


@pytest.mark.parametrize("n,F,max_bin", [(1, 1, 2), (65, 3, 3), (1000, 9, 256)])
def test_radix_route_equals_oracle_on_cpu(n, F, max_bin):
    X, W, h = torch.from_numpy(matrix(n, F)), hessian_like(n), n // 3
    ref = ops.cpu.weighted_cuts(X, W, max_bin, col_max(X))
    got = ops.weighted_cuts([X[:h], X[h:]], [W[:h], W[h:]], max_bin,
                            col_max(X))
    assert torch.equal(got.cuts_flat, ref.cuts_flat)
    assert torch.equal(got.cut_ptr, ref.cut_ptr)
    assert got.max_bins == ref.max_bins
