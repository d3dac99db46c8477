"""The HIP pointwise regression kernels: bitwise against the objectives' torch
compositions on the same GPU tensors, within bounds of the float64 forms in
``ops.cpu``, and the routes that reach them from the trainer."""

import numpy as np
import pytest
import torch

from tests.pointwise_cases import ALPHAS, GRADS, METRICS, draw, grad_bound
from xgboost_ray_amd import ops
from xgboost_ray_amd.engine import objectives as O

pytestmark = pytest.mark.gpu

# (n, max_blocks, offset): the four-row tail, a partial wave, a second
# workgroup; several grid-stride turns; a view off the 16-byte boundary
SHAPES = [(n, 0, 0) for n in (1, 3, 4, 5, 63, 65, 255, 257, 1027)]
SHAPES += [(4099, 2, 0), (1027, 0, 1)]


def _same(a, b):
    """``torch.equal`` that also holds NaN to NaN. A NaN's sign bit is not
    compared: it follows the compiler's choice between a negation and a
    source modifier, in torch's kernels as in these."""
    nan = torch.isnan(a)
    return (a.shape == b.shape and torch.equal(nan, torch.isnan(b))
            and torch.equal(a.masked_fill(nan, 0), b.masked_fill(nan, 0)))


def _dev(n, kind, weighted, K=0, offset=0):
    """The draw on the GPU; ``offset`` rows are cut off the front as a view."""
    cpu = draw(n + offset, kind, weighted, K)
    dev = [None if t is None else t.cuda()[offset:] for t in cpu]
    return [None if t is None else t[offset:] for t in cpu], dev


def _torch_route(monkeypatch, obj, *args):
    monkeypatch.setenv("RXGB_FUSED_GRAD", "0")
    want = obj.gradients(*args)
    assert obj.last_route == "torch"
    monkeypatch.delenv("RXGB_FUSED_GRAD")
    return want


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kind", list(GRADS))
def test_pointwise_grad(kind, weighted, monkeypatch):
    obj, param = GRADS[kind]
    for n, max_blocks, offset in SHAPES:
        cpu, dev = _dev(n, kind, weighted, offset=offset)
        gp, mx = ops.pointwise_grad(*dev, kind, param, max_blocks=max_blocks)
        want = _torch_route(monkeypatch, obj, *dev)
        assert _same(gp, want) and _same(mx, want.abs().amax(0)), (kind, n)
        gp2, mx2 = ops.pointwise_grad(*dev, kind, param,
                                      max_blocks=max_blocks)
        assert _same(gp, gp2) and _same(mx, mx2)
        routed = obj.gradients(*dev)
        assert obj.last_route == "hip" and _same(routed, gp)
        assert _same(routed._rxgb_absmax, mx)
        ref = ops.cpu.pointwise_grad(*cpu, kind, param)[0].numpy()
        *_, sg, sh = ops.cpu.pointwise_terms(cpu[0], cpu[1], kind, param)
        bound = grad_bound(ref, np.stack([sg, sh], -1), cpu[2])
        assert (np.abs(gp.cpu().numpy() - ref) <= bound).all(), (kind, n)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("K", [0, 1, 2, 3, 16])
def test_quantile_grad(K, weighted, monkeypatch):
    alphas = ALPHAS[:max(K, 1)]
    obj = O.QuantileError(alphas)
    shapes = SHAPES if K == 0 else [(5, 0, 0), (257, 0, 0), (1027, 2, 0)]
    for n, max_blocks, offset in shapes:
        cpu, dev = _dev(n, "quantile", weighted, K, offset)
        for t in (cpu, dev):
            t[0][n // 2] = t[1][n // 2]  # residual exactly 0
            t[0][0] = float("nan")
        gp, mx = ops.quantile_grad(*dev, alphas, max_blocks=max_blocks)
        want = _torch_route(monkeypatch, obj, *dev)
        assert _same(gp, want) and _same(mx, want.abs().amax(0)), (K, n)
        gp2, mx2 = ops.quantile_grad(*dev, alphas, max_blocks=max_blocks)
        assert _same(gp, gp2) and _same(mx, mx2)
        routed = obj.gradients(*dev)
        assert obj.last_route == "hip" and _same(routed, gp)
        if K:
            assert gp.permute(1, 0, 2).is_contiguous()
            assert _same(routed._rxgb_absmax_cls, mx)
        ref = ops.cpu.quantile_grad(*cpu, alphas)[0].numpy()
        bound = grad_bound(ref, np.ones(ref.shape), cpu[2])
        assert (np.abs(gp.cpu().numpy() - ref) <= bound).all(), (K, n)


# (margin, label): NaN; exp overflowing and underflowing as torch's does;
# residual 0; margin * y == 1 for hinge; margin <= -1 for squared log;
# label 0 for poisson and tweedie
EDGES = [(float("nan"), 1.0), (float("inf"), 1.0), (float("-inf"), 1.0),
         (88.0, 1.0), (-88.0, 1.0), (89.0, 2.0), (-104.0, 2.0), (0.75, 0.75),
         (1.0, 1.0), (-1.0, 0.5), (-2.0, 0.5), (0.5, 0.0)]


@pytest.mark.parametrize("kind", list(GRADS) + ["quantile"])
def test_edge_values_follow_torch(kind, monkeypatch):
    e = torch.tensor(EDGES, dtype=torch.float32).cuda()
    m, y = e[:, 0].contiguous(), e[:, 1].contiguous()
    w = torch.linspace(0.5, 2.0, len(EDGES)).cuda()
    for weight in (None, w):
        if kind == "quantile":
            obj = O.QuantileError([0.3])
            gp, mx = ops.quantile_grad(m, y, weight, [0.3])
        else:
            obj, param = GRADS[kind]
            gp, mx = ops.pointwise_grad(m, y, weight, kind, param)
        want = _torch_route(monkeypatch, obj, m, y, weight)
        assert _same(gp, want), (kind, gp, want)
        assert _same(mx, want.abs().amax(0))
    if kind == "hinge":  # the comparison is false for NaN
        assert gp[0].tolist() == [0.0, float(np.float32(1e-16)) * 0.5]
    elif kind not in ("absoluteerror", "quantile"):
        assert torch.isnan(gp[0]).all() and torch.isnan(mx).all()


def _eval_case(kind, transform, param, weighted, n, max_blocks, offset, K=0):
    cpu, dev = _dev(n, kind, weighted, K, offset)
    got = ops.eval_pointwise(*dev, kind, transform, param,
                             max_blocks=max_blocks)
    assert got.dtype == torch.float64 and got.shape == (2,)
    assert _same(got, ops.eval_pointwise(*dev, kind, transform, param,
                                         max_blocks=max_blocks))
    ref = ops.cpu.eval_pointwise(*cpu, kind, transform, param).numpy()
    rows = ops.cpu.pointwise_loss_rows(cpu[0], cpu[1], kind, transform, param)
    w = 1.0 if cpu[2] is None else cpu[2].numpy().astype(np.float64)
    tol = (n + 64) * 2.0 ** -53 * np.array([np.sum(w * np.abs(rows)), ref[1]])
    err = np.abs(got.cpu().numpy() - ref)
    return float((err / tol).max())


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", list(METRICS))
def test_eval_pointwise(name, weighted):
    kind, obj, param = METRICS[name]
    worst = max(_eval_case(kind, obj.eval_transform, param, weighted, *s)
                for s in SHAPES)
    print(f"eval {name} w={weighted}: {worst:.3f} of bound")
    assert worst <= 1.0


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("K", [0, 1, 2, 3, 16])
def test_eval_pinball(K, weighted):
    alphas = ALPHAS[:max(K, 1)]
    worst = max(_eval_case("pinball", "identity", alphas, weighted, *s, K=K)
                for s in [(5, 0, 0), (257, 0, 0), (1027, 2, 1)])
    print(f"pinball K={K} w={weighted}: {worst:.3f} of bound")
    assert worst <= 1.0


TRAIN = {
    "reg:absoluteerror": {}, "count:poisson": {}, "reg:gamma": {},
    "reg:tweedie": {"tweedie_variance_power": 1.2},
    "reg:squaredlogerror": {}, "reg:pseudohubererror": {},
    "binary:hinge": {},
    "reg:quantileerror": {"quantile_alpha": [0.1, 0.5, 0.9]},
}


def _train(objective, extra, rounds=20):
    from xgboost_ray_amd.engine.quantile import BinnedMatrix
    from xgboost_ray_amd.engine.trainer import BoostingEngine, EvalPack

    rng = np.random.RandomState(11)
    X = rng.randn(2000, 5).astype(np.float32)
    y = np.exp(0.5 * X[:, 0] + 0.2 * rng.randn(2000))
    if objective == "count:poisson":
        y = np.floor(2.0 * y)
    elif objective == "binary:hinge":
        y = (y > 1.0).astype(np.float64)
    dm = BinnedMatrix.build(torch.from_numpy(X).cuda(),
                            label=torch.from_numpy(y.astype(np.float32)).cuda(),
                            max_bin=64)
    eng = BoostingEngine({"objective": objective, "max_depth": 3,
                          "tree_method": "gpu_hist", **extra}, dm)
    for _ in range(rounds):
        eng.update()
    logged = eng.eval_sets([EvalPack(name="train", X=None)])["train"]
    return eng.obj.last_route, eng.margin.cpu().numpy(), logged


@pytest.mark.parametrize("objective", list(TRAIN))
def test_routes_train_the_same_model(objective, monkeypatch):
    route, margin, logged = _train(objective, TRAIN[objective])
    assert route == "hip"
    monkeypatch.setenv("RXGB_FUSED_GRAD", "0")
    monkeypatch.setenv("RXGB_FUSED_EVAL", "0")
    route0, margin0, logged0 = _train(objective, TRAIN[objective])
    assert route0 == "torch"
    assert np.array_equal(margin, margin0)
    assert logged.keys() == logged0.keys() and logged
    for k in logged:
        assert abs(logged[k] - logged0[k]) <= 1e-12 * abs(logged0[k]), k
