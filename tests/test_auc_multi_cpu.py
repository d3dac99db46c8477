"""Multiclass auc / aucpr on the CPU: the numpy oracle of the HIP kernels
against a per-row loop of the contract, and the metric against an exact
pairwise one-vs-rest AUC."""

import math

import numpy as np
import pytest
import torch

from xgboost_ray_amd import ops
from xgboost_ray_amd.engine.metrics import get_metric

# the envelope tests/test_engine_cpu.py (TestBinnedAUCTolerance) states for
# the 16384-bin AUC at a realistic score spread
BINNED_AUC_TOL = 5e-3


def _brute_hist(x, y, w, B):
    """The contract, one row and one class at a time."""
    n, K = x.shape
    hist = np.zeros((K, 2, B), np.int64)
    for i in range(n):
        m = -math.inf
        for v in x[i]:
            if v > m:
                m = float(v)
        with np.errstate(invalid="ignore"):
            e = [np.exp(np.float64(v) - np.float64(m)) for v in x[i]]
            s = np.float64(0.0)
            for v in e:
                s = s + v
            p = [v / s for v in e]
        yi = int(y[i]) if -1 < y[i] < K else -1  # int() truncates toward 0
        W = 1 if w is None else int(np.rint(np.float64(w[i]) * 2.0 ** 20))
        for k in range(K):
            t = p[k] * B
            b = min(int(t), B - 1) if t >= 1 else 0
            hist[k, int(k == yi), b] += W
    return hist


@pytest.mark.parametrize("n,K,B,weighted", [
    (1, 2, 2, False), (37, 3, 16384, True), (50, 17, 1000, False),
    (23, 5, 7, True),
])
def test_cpu_form_equals_a_per_row_loop_of_the_contract(n, K, B, weighted):
    rng = np.random.RandomState(n + K)
    x = (rng.randn(n, K) * 3).astype(np.float32)
    y = rng.randint(0, K, n).astype(np.float32)
    if n > 20:
        x[3, 1], x[5, 0], x[7] = np.nan, np.inf, 0.25
        y[:3] = [-1.0, K, 1.7]
    w = None
    if weighted:
        w = rng.uniform(0, 4, n).astype(np.float32)
        w[:2] = [0.0, 2.0 ** -22]  # the second rounds to W = 0
    got = ops.cpu.eval_auc_multiclass(
        torch.from_numpy(x), torch.from_numpy(y),
        None if w is None else torch.from_numpy(w), B)
    assert got.dtype == torch.int64 and tuple(got.shape) == (K, 2, B)
    np.testing.assert_array_equal(got.numpy(), _brute_hist(x, y, w, B))


def test_gpu_cases_keep_every_value_off_the_bin_edges():
    import auc_multi_cases as amc

    for c in amc.CASES:
        amc.case(*c)  # asserts the guard and the mass on the reference


def _value(name, x, y, w=None):
    m = get_metric(name)
    return m.finalize(m.local_stats(
        torch.from_numpy(x), torch.from_numpy(y),
        None if w is None else torch.from_numpy(w), None, None))


def _exact_ovr_auc(x, y):
    """Pairwise one-vs-rest AUC by the rank formula, ties counted 1/2,
    weighted by each class's number of positives."""
    d = x.astype(np.float64) - x.max(1, keepdims=True)
    p = np.exp(d) / np.exp(d).sum(1, keepdims=True)
    total = mass = 0.0
    for k in range(x.shape[1]):
        pos, neg = p[y == k, k], p[y != k, k]
        if len(pos) == 0 or len(neg) == 0:
            continue
        allv = np.sort(np.concatenate([pos, neg]))
        # mid-ranks: ties share the mean of their positions
        rank = (np.searchsorted(allv, pos, "left")
                + np.searchsorted(allv, pos, "right") + 1) / 2.0
        u = rank.sum() - len(pos) * (len(pos) + 1) / 2.0
        total += len(pos) * u / (len(pos) * len(neg))
        mass += len(pos)
    return total / mass


def test_multiclass_auc_is_the_prevalence_weighted_one_vs_rest_auc():
    rng = np.random.RandomState(0)
    n, K = 3000, 4
    y = rng.choice(K, n, p=[0.5, 0.3, 0.15, 0.05]).astype(np.float32)
    x = (rng.randn(n, K) + 1.5 * np.eye(K)[y.astype(int)]).astype(np.float32)
    exact = _exact_ovr_auc(x, y)
    got = _value("auc", x, y)
    print(f"binned {got:.6f} exact {exact:.6f}")
    assert 0.6 < exact < 0.99 and abs(got - exact) < BINNED_AUC_TOL
    # a class that no row has is skipped: the same rows with a fifth,
    # never-predicted class keep their value within the envelope
    x5 = np.concatenate([x, np.full((n, 1), -30.0, np.float32)], 1)
    assert abs(_value("auc", x5, y) - _exact_ovr_auc(x5, y)) < BINNED_AUC_TOL
    assert 0.0 < _value("aucpr", x, y) <= 1.0
    # unit weights change nothing: AUC is invariant to the 2^20 scale
    assert _value("auc", x, y, np.ones(n, np.float32)) == got


def test_no_class_with_both_kinds_of_mass_gives_the_neutral_values():
    x = np.random.RandomState(1).randn(20, 3).astype(np.float32)
    for y in (np.full(20, 1.0, np.float32), np.full(20, -1.0, np.float32)):
        assert _value("auc", x, y) == 0.5
        assert _value("aucpr", x, y) == 0.0


def test_train_logs_multiclass_auc_and_aucpr():
    from xgboost_ray_amd.engine.quantile import BinnedMatrix
    from xgboost_ray_amd.engine.trainer import EvalPack, run_training

    rng = np.random.RandomState(5)
    X = rng.randn(600, 5).astype(np.float32)
    y = np.digitize(X[:, 0] + 0.3 * rng.randn(600), [-0.5, 0.5])
    dm = BinnedMatrix.build(torch.from_numpy(X),
                            label=torch.from_numpy(y.astype(np.float32)),
                            max_bin=32)
    res = {}
    run_training({"objective": "multi:softprob", "num_class": 3,
                  "max_depth": 3, "eval_metric": ["auc", "aucpr"]},
                 dm, 3, evals=[EvalPack(name="train", X=None)],
                 evals_result=res)
    for name in ("auc", "aucpr"):
        vals = res["train"][name]
        assert len(vals) == 3 and all(0.0 < v <= 1.0 for v in vals)
    assert res["train"]["auc"][-1] > 0.8
