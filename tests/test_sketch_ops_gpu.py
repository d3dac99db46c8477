"""The HIP sketch kernels: ``ops.weighted_cuts`` equals the sort-based CPU
oracle byte for byte on any sharding; the re-bin equals ``bin_matrix``."""

import numpy as np
import pytest
import torch

from tests.sketch_cases import col_max, hessian_like, matrix
from xgboost_ray_amd import ops

pytestmark = pytest.mark.gpu

NS = (1, 63, 64, 65, 1000, 70001)
FS = (1, 3, 28, 70)  # 70: three pass-0 feature tiles, tables outside LDS
BINS = (2, 3, 16, 256)


def _same_cuts(got, ref):
    assert got.cuts_flat.is_cuda
    assert np.array_equal(got.cuts_flat.cpu().numpy().view(np.uint32),
                          ref.cuts_flat.numpy().view(np.uint32))
    assert np.array_equal(got.cut_ptr.cpu().numpy(), ref.cut_ptr.numpy())
    assert got.max_bins == ref.max_bins


# every n and every F meets every max_bin (a Latin square of the three sets)
@pytest.mark.parametrize("n,F,max_bin", [
    (n, F, BINS[(i + k) % 4]) for i, n in enumerate(NS)
    for k, F in enumerate(FS)])
def test_cuts_equal_oracle(n, F, max_bin):
    X, W = matrix(n, F), hessian_like(n)
    Xt, cm = torch.from_numpy(X), col_max(X)
    ref = ops.cpu.weighted_cuts(Xt, W, max_bin, cm)
    _same_cuts(ops.weighted_cuts(Xt.cuda(), W.cuda(), max_bin, cm), ref)


WEIGHTS = {
    "half_zero": lambda n, r: hessian_like(n) * torch.from_numpy(
        r.randint(0, 2, n)).int(),
    "all_zero": lambda n, r: torch.zeros(n, dtype=torch.int32),
    "negative": lambda n, r: hessian_like(n) - (1 << 28),
    # sums pass 2^53
    "int64_big": lambda n, r: torch.from_numpy(
        r.randint(0, 1 << 40, n, dtype=np.int64)),
    # the hessian column of an [n, 2] pair tensor, read in place
    "strided": lambda n, r: torch.stack([hessian_like(n)] * 2, 1),
}


@pytest.mark.parametrize("kind,n,F,max_bin,off", [
    ("half_zero", 1000, 28, 16, 0), ("all_zero", 1000, 28, 16, 0),
    ("negative", 1000, 28, 16, 0), ("int64_big", 20000, 28, 256, 0),
    ("strided", 1000, 3, 256, 0), ("half_zero", 1000, 3, 16, 1),
    ("strided", 1000, 70, 16, 1)])
def test_weight_cases(kind, n, F, max_bin, off):
    """``off`` rows are cut off the front as a view: X[1:] starts F * 4 bytes
    past a 16-byte boundary and takes scalar loads, not a copy."""
    X, W = matrix(n + off, F), WEIGHTS[kind](n + off, np.random.RandomState(7))
    Xd, Wd, X, W = torch.from_numpy(X).cuda()[off:], W.cuda()[off:], X[off:], W[off:]
    assert (Xd.data_ptr() % 16 != 0) == bool(off)
    if kind == "strided":
        W, Wd = W[:, 1], Wd[:, 1]
    ref = ops.cpu.weighted_cuts(torch.from_numpy(X), W, max_bin, col_max(X))
    _same_cuts(ops.weighted_cuts(Xd, Wd, max_bin, col_max(X)), ref)


@pytest.mark.parametrize("n,F,max_bin", [(1000, 28, 256), (70001, 3, 16)])
def test_shards_and_repeats(n, F, max_bin):
    """Two and three row shards accumulated into one histogram, and a second
    launch, give the bytes of the single call."""
    X, W = matrix(n, F), hessian_like(n)
    Xd, Wd, cm = torch.from_numpy(X).cuda(), W.cuda(), col_max(X)
    one = ops.weighted_cuts(Xd, Wd, max_bin, cm)
    for parts in (1, 2, 3):
        edges = [n * i // parts for i in range(parts + 1)]
        Xs = [Xd[a:b] for a, b in zip(edges, edges[1:])]
        Ws = [Wd[a:b] for a, b in zip(edges, edges[1:])]
        got = ops.weighted_cuts(Xs, Ws, max_bin, cm)
        assert torch.equal(got.cuts_flat.view(torch.int32),
                           one.cuts_flat.view(torch.int32))
        assert torch.equal(got.cut_ptr, one.cut_ptr)


@pytest.mark.parametrize("n,F,off", [(1, 1, 0), (65, 28, 0), (4099, 70, 1)])
def test_rebin_into_padded_storage(n, F, off):
    """``bin_matrix(out=)`` writes the rule's bins into the resident matrix
    (16-byte padded rows) and leaves the padding alone; ``off`` rows are cut
    off the front as an unaligned view."""
    X = matrix(n + off, F)[off:]
    Xd = torch.from_numpy(matrix(n + off, F)).cuda()[off:]
    cuts = ops.weighted_cuts(Xd, hessian_like(n).cuda(), 256, col_max(X))
    fresh = ops.bin_matrix(Xd, cuts.cuts_flat, cuts.cut_ptr)
    full = torch.full((n, (F + 15) // 16 * 16), 255, dtype=torch.uint8,
                      device="cuda")
    ops.bin_matrix(Xd, cuts.cuts_flat, cuts.cut_ptr, out=full[:, :F])
    assert torch.equal(full[:, :F], fresh)
    assert bool((full[:, F:] == 255).all())
