"""The HIP survival kernels against their float64 forms in ``ops.cpu``, and
the routes that reach them from the trainer."""

import functools

import numpy as np
import pytest
import torch

from xgboost_ray_amd import ops
from xgboost_ray_amd.engine.objectives import AFT, Cox

pytestmark = pytest.mark.gpu

T = ops.COX_TILE_ROWS  # asserted equal to the module's on load
# 65 T + 1: more tiles than a wave has lanes, so the tile scan crosses a wave
NS = [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3, 65 * T + 1]
PATTERNS = ["distinct", "equal", "runs", "no_events", "events_at_max"]


def _frac(out, ref, bound):
    return float((np.abs(out.cpu().numpy().astype(np.float64) - ref)
                  / bound).max())


@functools.lru_cache(maxsize=None)
def _cox_case(n, pattern, weighted):
    rng = np.random.RandomState(n % 9973 + len(pattern))
    if pattern == "equal":
        t = np.full(n, 3.0)
    elif pattern == "runs":  # runs of 1-5 equal times
        t = np.repeat(np.arange(n), rng.randint(1, 6, n))[:n] + 1.0
        if n > T + 2:  # descending order puts this run across a tile edge
            t[n - T - 3:n - T + 2] = t[n - T - 3]
        t = t[rng.permutation(n)]
    else:
        t = rng.permutation(n) + 1.0
    ev = rng.rand(n) < 0.6
    if pattern == "no_events":
        ev[:] = False
    elif pattern == "events_at_max":
        ev = t == t.max()
    m = rng.uniform(-8, 8, n).astype(np.float32)
    if n >= 3:  # one row far above the rest, one whose eta underflows to 0
        m[n // 2] = 80.0
        m[n // 3] = 80.0 - 700.0
    t = [torch.from_numpy(m),
         torch.from_numpy((t * np.where(ev, 1, -1)).astype(np.float32)),
         torch.from_numpy(rng.uniform(0.25, 4, n).astype(np.float32))
         if weighted else None]
    lay = ops.cpu.cox_layout(t[1])
    m_s, eta, C, A, B, _ = ops.cpu.cox_terms(t[0], lay)
    scale = torch.empty(n, 2, dtype=torch.float64)  # in row order
    scale[lay.order.long()] = torch.stack(
        [1.0 + eta * A, eta * A + eta * eta * B], dim=1)
    e = lay.event > 0  # the metric's terms: m - shift and log C per event
    abs_terms = float(m_s[e].abs().sum() + C[e].log().abs().sum())
    return (t, ops.cpu.cox_grad(t[0], lay, t[2])[0], scale.numpy(),
            ops.cpu.eval_cox(t[0], lay).numpy(), abs_terms)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", NS)
def test_cox_grad_and_eval_match_cpu_forms(n, pattern, weighted):
    (m, label, w), ref_gp, scale, ref_stats, abs_terms = _cox_case(
        n, pattern, weighted)
    m, label = m.cuda(), label.cuda()
    w = None if w is None else w.cuda()
    lay = ops.cox_layout(label)
    assert ops.cox_layout(label) is lay and lay.order.dtype == torch.int32
    gp, mx = ops.cox_grad(m, lay, w)
    assert gp.shape == (n, 2) and gp.dtype == torch.float32
    gp2, mx2 = ops.cox_grad(m, lay, w)
    assert torch.equal(gp, gp2) and torch.equal(mx, mx2)
    assert torch.equal(mx, gp.abs().amax(0))
    ref = ref_gp.numpy().astype(np.float64)
    wmax = 1.0 if w is None else np.maximum(1.0, w.cpu().numpy())[:, None]
    bound = 2.0 ** -23 * np.abs(ref) + 2.0 ** -40 * wmax * scale
    frac = _frac(gp, ref, bound)
    print(f"cox_grad n={n} {pattern} w={weighted}: {frac:.3f} of bound")
    assert frac <= 1.0

    stats = ops.eval_cox(m, lay)
    assert torch.equal(stats, ops.eval_cox(m, lay))
    # per-term bound: the terms are m - shift and log C of every event row
    tol = n * 2.0 ** -53 * abs_terms
    err = abs(float(stats[0]) - ref_stats[0])
    print(f"eval_cox: {err:.3e} of {tol:.3e}")
    assert err <= tol and float(stats[1]) == ref_stats[1]


AFT_NS = [1, 63, 64, 65, 1023, 1024, 1025, 4 * 1024 * 3 + 5]


@functools.lru_cache(maxsize=None)
def _aft_case(n, weighted):
    """n random rows of all four kinds, then the fixed rows."""
    rng = np.random.RandomState(n + 17)
    lo = np.exp(rng.uniform(-2, 2, n)).astype(np.float32)
    hi = (lo * np.exp(rng.uniform(0.3, 2, n))).astype(np.float32)
    kind = np.arange(n) % 4
    hi[kind == 0] = lo[kind == 0]
    hi[kind == 1] = np.inf
    lo[kind == 2] = 0.0
    m = rng.uniform(-2, 2, n).astype(np.float32)
    inf = np.inf
    fixed = np.array([  # (margin, lower, upper)
        [-60.0, 2.0, 2.0], [60.0, 2.0, 2.0],    # uncensored, z at +-15
        [-60.0, 2.0, inf], [60.0, 2.0, inf],    # right, z at +-15
        [-60.0, 0.0, 2.0], [60.0, 0.0, 2.0],    # left (yl = 0), z at +-15
        [0.5, 1e-9, 2.0], [0.5, 1.0, 1e9],      # interval, one z clamped
        [0.5, 0.0, inf], [0.5, 3.0, 3.0]], np.float32)
    m = np.concatenate([m, fixed[:, 0]])
    label = np.concatenate([np.stack([lo, hi], 1), fixed[:, 1:]])
    w = rng.uniform(0.25, 4, len(m)).astype(np.float32) if weighted else None
    return (torch.from_numpy(m), torch.from_numpy(label),
            None if w is None else torch.from_numpy(w))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dist", ops.cpu.AFT_DISTS)
@pytest.mark.parametrize("n", AFT_NS)
def test_aft_grad_and_eval_match_cpu_forms(n, dist, weighted):
    m, label, w = _aft_case(n, weighted)
    sigma = 1.3
    ref_gp, _ = ops.cpu.aft_grad(m, label, w, dist, sigma)
    dev = [m.cuda(), label.cuda(), None if w is None else w.cuda()]
    gp, mx = ops.aft_grad(*dev, dist, sigma)
    assert gp.shape == (len(m), 2) and gp.dtype == torch.float32
    gp2, mx2 = ops.aft_grad(*dev, dist, sigma)
    assert torch.equal(gp, gp2) and torch.equal(mx, mx2)
    assert torch.equal(mx, gp.abs().amax(0))
    ref = ref_gp.numpy().astype(np.float64)
    wmax = 1.0 if w is None else np.maximum(1.0, w.numpy())[:, None]
    frac = _frac(gp, ref, 2.0 ** -23 * np.abs(ref) + 2.0 ** -40 * wmax)
    print(f"aft_grad n={n} {dist} w={weighted}: {frac:.3f} of bound")
    assert frac <= 1.0

    stats = ops.eval_aft(*dev, dist, sigma)
    assert torch.equal(stats, ops.eval_aft(*dev, dist, sigma))
    nll = ops.cpu.aft_nll_rows(m, label, dist, sigma)
    wd = torch.ones_like(nll) if w is None else w.double()
    ref_s = ops.cpu.eval_aft(m, label, w, dist, sigma).numpy()
    tol = len(m) * 2.0 ** -53 * np.array([float((wd * nll).abs().sum()),
                                         ref_s[1]])
    err = np.abs(stats.cpu().numpy() - ref_s)
    print(f"eval_aft: {err} of {tol}")
    assert (err <= tol).all()


def test_nan_margins():
    m, label, _ = _aft_case(65, False)
    m = m.clone()
    m[7] = float("nan")
    gp, mx = ops.aft_grad(m.cuda(), label.cuda(), None, "normal", 1.0)
    bad = torch.zeros(len(m), dtype=torch.bool)
    bad[7] = True
    gp = gp.cpu()
    assert torch.isnan(gp[bad]).all() and not torch.isnan(gp[~bad]).any()
    assert torch.isnan(mx).all()
    (m, label, _), *_ = _cox_case(T + 1, "runs", False)
    m = m.clone()
    m[T] = float("nan")
    gp, mx = ops.cox_grad(m.cuda(), ops.cox_layout(label.cuda()))
    assert torch.isnan(gp).all() and torch.isnan(mx).all()


def _train(objective, label, metric, rounds=5):
    from xgboost_ray_amd.engine.quantile import BinnedMatrix
    from xgboost_ray_amd.engine.trainer import BoostingEngine, EvalPack

    X = np.random.RandomState(5).randn(2000, 6).astype(np.float32)
    dm = BinnedMatrix.build(torch.from_numpy(X).cuda(), max_bin=64)
    for k, v in label(X).items():
        setattr(dm, k, torch.from_numpy(v).cuda())
    eng = BoostingEngine({"objective": objective, "max_depth": 3,
                          "tree_method": "gpu_hist"}, dm)
    losses = []
    for _ in range(rounds):
        eng.update()
        losses.append(
            eng.eval_sets([EvalPack(name="train", X=None)])["train"][metric])
    assert eng.obj.last_route == "hip"
    gp = eng.obj.gradients(eng.margin, eng._train_label, eng.dtrain.weight)
    assert torch.equal(gp._rxgb_absmax, gp.abs().amax(0))
    assert all(b < a for a, b in zip(losses, losses[1:]))
    return eng, losses


def _time(X):
    rng = np.random.RandomState(6)
    return np.exp(0.7 * X[:, 0] + 0.3 * rng.randn(len(X))), rng


def test_engine_trains_aft_on_the_hip_route():
    def label(X):
        t, rng = _time(X)
        lo, hi = t.astype(np.float32), t.astype(np.float32)
        hi[rng.rand(len(X)) < 0.3] = np.inf
        return {"label_lower_bound": lo, "label_upper_bound": hi}

    eng, losses = _train("survival:aft", label, "aft-nloglik")
    m, lab = eng.margin.cpu(), eng._train_label.cpu()
    nll = ops.cpu.aft_nll_rows(m, lab, "normal", 1.0)
    assert (abs(losses[-1] - float(nll.mean()))
            <= len(m) * 2.0 ** -53 * float(nll.abs().mean()))


def test_engine_trains_cox_on_the_hip_route():
    def label(X):
        t, rng = _time(X)
        return {"label": (t * np.where(rng.rand(len(X)) < 0.7, 1, -1))
                .astype(np.float32)}

    eng, losses = _train("survival:cox", label, "cox-nloglik")
    lab = eng._train_label.cpu()
    lay = ops.cpu.cox_layout(lab)
    ref = ops.cpu.eval_cox(eng.margin.cpu(), lay)
    m_s, _, C, *_ = ops.cpu.cox_terms(eng.margin.cpu(), lay)
    e = lay.event > 0
    terms = float(m_s[e].abs().sum() + C[e].log().abs().sum())
    assert (abs(losses[-1] - float(ref[0] / ref[1]))
            <= len(lab) * 2.0 ** -53 * terms / float(ref[1]))


def test_fused_grad_switch_keeps_the_torch_bytes(monkeypatch):
    monkeypatch.setenv("RXGB_FUSED_GRAD", "0")
    m, label, w = (a.cuda() for a in _aft_case(257, True))
    obj = AFT("normal", 1.0)
    got = obj.gradients(m, label, w)
    assert obj.last_route == "torch"
    # in line: every kind of row through torch float64, as before the kernels
    yl, yu, md = label[:, 0].double(), label[:, 1].double(), m.double()
    zl = ((torch.log(yl.clamp(min=1e-16)) - md) / 1.0).clamp(-15, 15)
    zu = ((torch.log(yu.clamp(min=1e-16)) - md) / 1.0).clamp(-15, 15)
    pdf = lambda z: torch.exp(-0.5 * z * z) / np.sqrt(2 * np.pi)  # noqa: E731
    S = lambda z: torch.special.ndtr(-z)  # noqa: E731
    hz = pdf(zl) / S(zl).clamp(min=1e-300)
    rh = pdf(zu) / torch.special.ndtr(zu).clamp(min=1e-300)
    D = (S(zl) - S(zu)).clamp(min=1e-300)
    df = pdf(zu) - pdf(zl)
    pick = lambda u, r, l, i: torch.where(  # noqa: E731
        yl == yu, u, torch.where(torch.isinf(yu), r,
                                 torch.where(yl <= 0, l, i)))
    g = pick(-zl, -hz, rh, df / D).float()
    h = pick(torch.ones_like(zl), hz * (hz - zl), -(rh * (-zu - rh)),
             df ** 2 / (D * D) - (pdf(zu) * -zu - pdf(zl) * -zl) / D)
    want = torch.stack([g * w, h.clamp(min=1e-6).float() * w], dim=-1)
    assert torch.equal(got, want)
    (m, label, w), *_ = _cox_case(T + 1, "runs", True)
    obj = Cox()
    obj.gradients(m.cuda(), label.cuda(), w.cuda())
    assert obj.last_route == "torch"
