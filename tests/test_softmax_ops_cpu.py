"""ops.cpu.softmax_grad / eval_multiclass against a per-row math.fsum
reference, and the unchanged torch route of SoftmaxBase.gradients on CPU."""

import math

import numpy as np
import pytest
import torch

from xgboost_ray_amd import ops
from xgboost_ray_amd.engine.objectives import SoftProb


def _case(n, K, weighted, seed=3):
    rng = np.random.RandomState(seed)
    x = rng.uniform(-8, 8, (n, K)).astype(np.float32)
    x[0] = 1.5                          # all classes equal
    x[1], x[1, K // 2] = -80.0, 80.0    # hessian clamp
    x[2, 0] = x[2, K - 1] = 9.0         # tie: class 0 is the prediction
    y = rng.randint(0, K, n).astype(np.float32)
    y[1], y[2] = K // 2, K - 1
    w = rng.uniform(0.25, 4, n).astype(np.float32) if weighted else None
    return x, y, w


def _reference(x, y, w):
    """Per row: exp, fsum, divide, all in float64 python arithmetic."""
    n, K = x.shape
    gp = np.zeros((n, K, 2), np.float32)
    stats = [[], [], []]
    for i in range(n):
        row = [float(v) for v in x[i]]
        m = max(row)
        e = [math.exp(v - m) for v in row]
        s = math.fsum(e)
        wi = np.float32(1.0 if w is None else w[i])
        for k in range(K):
            p = e[k] / s
            gp[i, k, 0] = np.float32(p - (k == int(y[i]))) * wi
            gp[i, k, 1] = np.float32(max(2.0 * p * (1.0 - p), 1e-16)) * wi
        stats[0].append(float(wi) * (math.log(s) - (row[int(y[i])] - m)))
        stats[1].append(float(wi) * (row.index(m) != int(y[i])))
        stats[2].append(float(wi))
    return gp, np.array([math.fsum(v) for v in stats])


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("K", [2, 5, 40])
def test_cpu_forms_match_fsum_reference(K, weighted):
    x, y, w = _case(37, K, weighted)
    ref_gp, ref_stats = _reference(x, y, w)
    tw = None if w is None else torch.from_numpy(w)
    gp, mx = ops.softmax_grad(torch.from_numpy(x), torch.from_numpy(y), tw)
    assert gp.shape == (37, K, 2) and gp.dtype == torch.float32
    assert all(gp[:, c, :].is_contiguous() for c in range(K))
    wmax = np.ones(37) if w is None else np.maximum(1.0, w)
    # the ascending sum against fsum: K roundings of 2^-53 on s, far inside
    # the float32 rounding the bound allows
    bound = 2.0 ** -23 * np.abs(ref_gp) + 2.0 ** -40 * wmax[:, None, None]
    assert (np.abs(gp.numpy().astype(np.float64) - ref_gp) <= bound).all()
    np.testing.assert_array_equal(mx.numpy(), gp.abs().amax(0).numpy())
    assert gp[1, (K // 2 + 1) % K, 1] == np.float32(1e-16) * (
        1 if w is None else w[1])
    stats = ops.eval_multiclass(torch.from_numpy(x), torch.from_numpy(y), tw)
    # per term (2K + 16) roundings, plus at most n for numpy's own sum
    np.testing.assert_allclose(stats.numpy(), ref_stats,
                               rtol=(2 * K + 16 + 37) * 2.0 ** -53)


def test_cpu_bad_labels_and_nan():
    x, y, _ = _case(8, 4, False)
    y[3], y[4] = 4.0, -1.0
    x[5, 2] = np.nan
    gp, mx = ops.softmax_grad(torch.from_numpy(x), torch.from_numpy(y))
    p = torch.softmax(torch.from_numpy(x).double(), 1).float()
    for i in (3, 4):  # no class: g is p itself
        torch.testing.assert_close(gp[i, :, 0], p[i], rtol=2.0 ** -22, atol=0)
    assert torch.isnan(gp[5]).all() and torch.isnan(mx).all()
    assert not torch.isnan(gp[[0, 1, 2, 3, 4, 6, 7]]).any()
    assert torch.isnan(
        ops.eval_multiclass(torch.from_numpy(x), torch.from_numpy(y))[0])


@pytest.mark.parametrize("weighted", [False, True])
def test_softmax_objective_cpu_keeps_torch_bytes(weighted):
    x, y, w = _case(100, 5, weighted)
    m, lab = torch.from_numpy(x), torch.from_numpy(y)
    tw = None if w is None else torch.from_numpy(w)
    obj = SoftProb(5)
    got = obj.gradients(m, lab, tw)
    assert obj.last_route == "torch"
    p = torch.softmax(m, dim=1)
    g = p - torch.nn.functional.one_hot(lab.long(), 5).to(p.dtype)
    h = torch.clamp(2.0 * p * (1.0 - p), min=1e-16)
    if weighted:
        g, h = g * tw.unsqueeze(1), h * tw.unsqueeze(1)
    assert torch.equal(got, torch.stack([g, h], dim=-1))
    assert not hasattr(got, "_rxgb_absmax_cls")
