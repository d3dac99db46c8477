"""The float64 survival forms of ``ops.cpu`` against the objective and metric
classes users train with today, on CPU float64 tensors."""

import numpy as np
import pytest
import torch

from xgboost_ray_amd import ops
from xgboost_ray_amd.engine.metrics import AFTNLogLik, CoxNLogLik
from xgboost_ray_amd.engine.objectives import AFT, Cox


def _close(got, ref):
    """The float32 bits, or one ulp where the transcendentals differ."""
    got, ref = got.double().numpy(), ref.double().numpy()
    assert (np.abs(got - ref) <= 2.0 ** -23 * np.abs(ref)).all()


def _aft_data(n=403):
    """All four censoring kinds, about a quarter each."""
    rng = np.random.RandomState(11)
    lo = np.exp(rng.uniform(-2, 2, n)).astype(np.float32)
    hi = (lo * np.exp(rng.uniform(0.3, 2, n))).astype(np.float32)
    kind = rng.randint(0, 4, n)
    hi[kind == 0] = lo[kind == 0]
    hi[kind == 1] = np.inf
    lo[kind == 2] = 0.0
    margin = rng.uniform(-2, 2, n).astype(np.float32)
    w = rng.uniform(0.25, 4, n).astype(np.float32)
    return (torch.from_numpy(margin), torch.from_numpy(np.stack([lo, hi], 1)),
            torch.from_numpy(w))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("sigma", [0.7, 1.0, 2.5])
@pytest.mark.parametrize("dist", ops.cpu.AFT_DISTS)
def test_aft_forms_match_the_objective(dist, sigma, weighted):
    margin, label, w = _aft_data()
    w = w if weighted else None
    obj = AFT(dist, sigma)
    ref = obj.gradients(margin.double(), label.double(),
                        None if w is None else w)
    gp, mx = ops.aft_grad(margin, label, w, dist, sigma)
    assert gp.dtype == torch.float32 and torch.equal(mx, gp.abs().amax(0))
    _close(gp, ref)
    nll = obj.nll(margin.double(), label[:, 0].double(), label[:, 1].double())
    nll = nll.numpy()
    # a censored row is -log D with D = 1 - F or F_u - F_l: an error of a few
    # 2^-53 in F (ndtr against erfc) is divided by D = exp(-nll)
    tol = 2.0 ** -50 * (np.exp(np.maximum(nll, 0.0)) + np.abs(nll))
    got = ops.cpu.aft_nll_rows(margin, label, dist, sigma).numpy()
    assert (np.abs(got - nll) <= tol).all()
    ref_stats = AFTNLogLik().local_stats(margin, label, w, None, obj).numpy()
    stats = ops.eval_aft(margin, label, w, dist, sigma).numpy()
    wmax = 4.0 if weighted else 1.0
    assert abs(stats[0] - ref_stats[0]) <= wmax * tol.sum()
    assert abs(stats[1] - ref_stats[1]) <= 1e-12 * ref_stats[1]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("ties", [False, True])
def test_cox_forms_match_the_objective(ties, weighted):
    rng = np.random.RandomState(5)
    n = 517
    t = (rng.randint(1, 60, n) if ties
         else rng.permutation(n) + 1).astype(np.float32)
    label = torch.from_numpy(t * np.where(rng.rand(n) < 0.6, 1, -1)
                             .astype(np.float32))
    margin = torch.from_numpy(rng.uniform(-8, 8, n).astype(np.float32))
    w = torch.from_numpy(rng.uniform(0.25, 4, n).astype(np.float32))
    w = w if weighted else None
    lay = ops.cox_layout(label)
    assert ops.cox_layout(label) is lay  # cached on the label tensor
    gp, mx = ops.cox_grad(margin, lay, w)
    assert torch.equal(mx, gp.abs().amax(0))
    _close(gp, Cox().gradients(margin.double(), label.double(), w))
    np.testing.assert_allclose(
        ops.eval_cox(margin, lay).numpy(),
        CoxNLogLik().local_stats(margin, label, None, None, None).numpy(),
        rtol=1e-13)
