"""The HIP multiclass kernels against their numpy float64 forms, and the
routes that reach them from the trainer."""

import functools

import numpy as np
import pytest
import torch

from xgboost_ray_amd import ops
from xgboost_ray_amd.engine.objectives import SoftProb

pytestmark = pytest.mark.gpu

NS = [1, 63, 64, 65, 257, 1000]
KC = ops.SOFTMAX_CHUNK_CLASSES  # asserted equal to the module's on load
KS = sorted({2, 3, 7, 33, KC, KC + 1, 2 * KC + 5})


@functools.lru_cache(maxsize=None)
def _case(n, K, weighted):
    """Inputs (total n rows: uniform margins, then the fixed rows) and the
    CPU forms' results, computed once."""
    if n * K > 300_000:
        n = 257
    rng = np.random.RandomState(n * 131 + K)
    fixed = np.zeros((4, K), np.float32)
    fixed[0] = 0.75                           # all classes equal
    fixed[1], fixed[1, K // 2] = -80.0, 80.0  # hessian clamp at 1e-16
    fixed[2] = rng.uniform(-8, 8, K)
    fixed[2, K - 1] = 8.5                     # maximum in the last class
    fixed[3] = rng.uniform(-8, 8, K)
    fixed[3, 0] = fixed[3, K - 1] = 9.0       # tie: class 0 is predicted
    nf = min(4, n)
    x = np.concatenate([rng.uniform(-8, 8, (n - nf, K)).astype(np.float32),
                        fixed[4 - nf:]])
    y = rng.randint(0, K, n).astype(np.float32)
    y[n - nf:] = np.array([1, K // 2, K - 1, K - 1], np.float32)[4 - nf:]
    w = rng.uniform(0.25, 4, n).astype(np.float32) if weighted else None
    t = [torch.from_numpy(x), torch.from_numpy(y),
         None if w is None else torch.from_numpy(w)]
    return t, ops.cpu.softmax_grad(*t), ops.cpu.eval_multiclass(*t)


def _cuda(t):
    return [None if a is None else a.cuda() for a in t]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n", NS)
def test_softmax_grad_and_eval_match_cpu_forms(n, K, weighted):
    t, (ref_gp, _), ref_stats = _case(n, K, weighted)
    n = len(t[1])
    dev = _cuda(t)
    gp, mx = ops.softmax_grad(*dev)
    assert gp.shape == (n, K, 2) and gp.dtype == torch.float32
    assert all(gp[:, c, :].is_contiguous() for c in range(K))
    gp2, mx2 = ops.softmax_grad(*dev)
    assert torch.equal(gp, gp2) and torch.equal(mx, mx2)
    np.testing.assert_array_equal(mx.cpu().numpy(),
                                  gp.abs().amax(0).cpu().numpy())
    ref = ref_gp.numpy().astype(np.float64)
    wmax = 1.0 if t[2] is None else np.maximum(1.0, t[2].numpy())
    bound = 2.0 ** -23 * np.abs(ref) + 2.0 ** -40 * np.reshape(wmax, (-1, 1, 1))
    frac = np.abs(gp.cpu().numpy().astype(np.float64) - ref) / bound
    print(f"softmax_grad n={n} K={K} w={weighted}: {frac.max():.3f} of bound")
    assert frac.max() <= 1.0

    stats = ops.eval_multiclass(*dev).cpu().numpy()
    ref_s = ref_stats.numpy()
    # every w * nll term is >= 0, so the summed per-term bound is the sum's
    tol = [(2 * K + 16) * 2.0 ** -53 * ref_s[0], n * 2.0 ** -53 * ref_s[1],
           n * 2.0 ** -53 * ref_s[2]]
    print(f"eval_multiclass: {np.abs(stats - ref_s)} of {tol}")
    assert (np.abs(stats - ref_s) <= tol).all()
    if n >= 4:
        assert ref_s[1] >= (1.0 if t[2] is None else 0.25)  # the tied row


@pytest.mark.parametrize("K", [3, KC + 1])
def test_nan_rows_and_labels_outside_the_classes(K):
    (x, y, _), _, _ = _case(65, K, False)
    x, y = x.clone(), y.clone()
    x[7, K - 1] = float("nan")
    y[3], y[4] = float(K), -1.0
    gp, mx = ops.softmax_grad(x.cuda(), y.cuda())
    gp = gp.cpu()
    bad = torch.zeros(65, dtype=torch.bool)
    bad[7] = True
    assert torch.isnan(gp[bad]).all() and not torch.isnan(gp[~bad]).any()
    assert torch.isnan(mx).all()
    p = torch.softmax(x.double(), dim=1)
    for i in (3, 4):
        assert torch.isfinite(gp[i]).all()
        torch.testing.assert_close(gp[i, :, 0].double(), p[i],
                                   rtol=2.0 ** -23, atol=2.0 ** -40)
    assert torch.isnan(ops.eval_multiclass(x.cuda(), y.cuda())[0])


def _train(rounds=5):
    from xgboost_ray_amd.engine.quantile import BinnedMatrix
    from xgboost_ray_amd.engine.trainer import BoostingEngine, EvalPack

    rng = np.random.RandomState(5)
    X = rng.randn(2000, 6).astype(np.float32)
    y = np.digitize(X[:, 0] + 0.5 * X[:, 1] + 0.3 * rng.randn(2000),
                    [-0.5, 0.5]).astype(np.float32)
    dm = BinnedMatrix.build(torch.from_numpy(X).cuda(),
                            label=torch.from_numpy(y).cuda(), max_bin=64)
    eng = BoostingEngine({"objective": "multi:softprob", "num_class": 3,
                          "max_depth": 3, "tree_method": "gpu_hist",
                          "eval_metric": ["mlogloss"]}, dm)
    losses = []
    for _ in range(rounds):
        eng.update()
        losses.append(
            eng.eval_sets([EvalPack(name="train", X=None)])["train"]["mlogloss"])
    return eng, y, losses


def test_engine_trains_on_the_hip_route():
    eng, y, losses = _train()
    assert eng.obj.last_route == "hip"
    gp = eng.obj.gradients(eng.margin, eng._train_label, eng.dtrain.weight)
    for c in range(3):
        assert gp[:, c, :].is_contiguous()
        assert torch.equal(gp._rxgb_absmax_cls[c], gp[:, c, :].abs().amax(0))
    assert all(b < a for a, b in zip(losses, losses[1:]))
    m = eng.margin.cpu().numpy().astype(np.float64)
    d = m - m.max(1, keepdims=True)
    nll = np.log(np.exp(d).sum(1)) - d[np.arange(len(y)), y.astype(int)]
    assert abs(losses[-1] - nll.mean()) <= 1e-12 * nll.mean()


def test_fused_grad_switch_keeps_the_torch_bytes(monkeypatch):
    monkeypatch.setenv("RXGB_FUSED_GRAD", "0")
    (x, y, w), _, _ = _case(257, 7, True)
    m, lab, tw = x.cuda(), y.cuda(), w.cuda()
    obj = SoftProb(7)
    got = obj.gradients(m, lab, tw)
    assert obj.last_route == "torch"
    p = torch.softmax(m, dim=1)
    g = (p - torch.nn.functional.one_hot(lab.long(), 7).to(p.dtype))
    h = torch.clamp(2.0 * p * (1.0 - p), min=1e-16)
    want = torch.stack([g * tw.unsqueeze(1), h * tw.unsqueeze(1)], dim=-1)
    assert torch.equal(got, want)
