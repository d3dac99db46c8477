"""Inputs shared by the weighted-sketch tests."""

import numpy as np
import torch

_SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, 1e-40, -1e-40, 3e-45, 1.0],
                    np.float32)
KINDS = [
    lambda n, r: r.randn(n),                                  # normal data
    lambda n, r: r.randn(n) * 10.0 ** r.randint(-6, 7, n),    # across the sign
    lambda n, r: _SPECIAL[r.randint(0, 8, n)],       # +-0, +-inf, denormals
    lambda n, r: np.full(n, 2.5),                             # constant
    lambda n, r: np.array([-1.0, 0.5, 7.0])[r.randint(0, 3, n)],
    lambda n, r: np.full(n, np.nan),                          # all missing
    lambda n, r: np.where(r.rand(n) < 1 / 3, np.nan, r.rand(n)),
    lambda n, r: np.where(r.rand(n) < 0.7, 1.0, np.round(r.randn(n) * 3)),  # ties
    lambda n, r: r.rand(n) * 1e-3 + 1.0,             # 16 key bits shared
]


def matrix(n, F, seed=0):
    """f32 [n, F]: column f is of kind f % len(KINDS)."""
    rng = np.random.RandomState(seed + 1000 * F + n)
    return np.stack([KINDS[f % len(KINDS)](n, rng) for f in range(F)],
                    1).astype(np.float32)


def col_max(X):
    """f32 [F] tensor: the largest non-NaN value per column, NaN if none."""
    Xt = torch.as_tensor(X)
    nan = torch.isnan(Xt)
    mx = torch.where(nan, torch.full_like(Xt, float("-inf")), Xt).amax(0)
    return torch.where((~nan).any(0), mx, torch.full_like(mx, float("nan")))


def hessian_like(n, seed=0):
    """int32 weights in [0, 2^30], as the quantized hessian column."""
    w = np.random.RandomState(seed).rand(n) ** 2 * (1 << 30)
    return torch.from_numpy(np.round(w).astype(np.int32))
