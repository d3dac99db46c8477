"""Inputs shared by the pointwise regression tests: one seeded draw."""

import numpy as np
import torch

from xgboost_ray_amd.engine import objectives as O

# gradient kind -> (objective, param of ops.pointwise_grad)
GRADS = {
    "absoluteerror": (O.AbsoluteError(), 0.0),
    "poisson": (O.Poisson(), 0.0),
    "gamma": (O.Gamma(), 0.0),
    "tweedie": (O.Tweedie(1.2), 1.2),
    "squaredlogerror": (O.SquaredLogError(), 0.0),
    "pseudohuber": (O.PseudoHuber(1.5), 1.5),
    "hinge": (O.Hinge(), 0.0),
}
ALPHAS = [0.05, 0.1, 0.2, 0.25, 0.3, 0.4, 0.45, 0.5, 0.55, 0.6, 0.7, 0.75,
          0.8, 0.9, 0.95, 0.99]
# metric name -> (kind, objective that sets the transform, param)
METRICS = {
    "rmse": ("se", O.SquaredError(), 0.0),
    "rmse/sigmoid": ("se", O.Logistic(), 0.0),
    "mae": ("ae", O.Poisson(), 0.0),
    "mape": ("ape", O.Gamma(), 0.0),
    "rmsle": ("sle", O.SquaredLogError(), 0.0),
    "mphe": ("mphe", O.PseudoHuber(), 0.0),
    "poisson-nloglik": ("poisson", O.Poisson(), 0.0),
    "gamma-nloglik": ("gamma", O.Gamma(), 0.0),
    "tweedie-nloglik@1.2": ("tweedie", O.Tweedie(1.2), 1.2),
}


def draw(n, kind, weighted, K=0):
    """(margin, label, weight or None) float32 CPU tensors; margin [n, K]
    for K > 0. Labels suit the kind: counts, positives, {0, 1}, or reals."""
    rng = np.random.RandomState(1000 * n + 7 * len(kind) + K)
    m = rng.uniform(-1.5, 2.0, (n, K) if K else n)
    y = rng.uniform(0.2, 3.0, n)
    if kind == "poisson":
        y = np.floor(2.0 * y)
    elif kind == "tweedie":
        y[rng.rand(n) < 0.3] = 0.0
    elif kind == "hinge":
        y = (y > 1.5).astype(np.float64)
    elif kind in ("absoluteerror", "pseudohuber", "quantile", "pinball",
                  "se", "ae", "mphe"):
        y = y - 1.5
    w = rng.uniform(0.25, 4.0, n) if weighted else None
    f32 = lambda a: torch.from_numpy(a.astype(np.float32))  # noqa: E731
    return f32(m), f32(y), None if w is None else f32(w)


def grad_bound(ref, scale, weight):
    """2^-22 |ref| + 2^-22 max |term|: a few float32 roundings of the chain
    against float64 (``ops.cpu.pointwise_terms`` names the terms)."""
    w = 1.0 if weight is None else weight.numpy().astype(np.float64)
    w = np.reshape(w, np.shape(w) + (1,) * (scale.ndim - np.ndim(w)))
    return 2.0 ** -22 * (np.abs(ref) + w * scale)
