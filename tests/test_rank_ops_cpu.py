"""Ranking ops: float64 references, the shared cases, and the numpy twins.

The references are written from the contract in docs/parity.md, "Ranking on
the device", and import nothing from ``ops`` or the objective and metric
classes; ``rank`` and the full ``idcg`` come from ``aux_cases.ref_rank_prep``.
``tests/test_rank_ops_gpu.py`` runs the HIP kernels against the same
references; this file checks ``ops.cpu`` against them, and so the references
against a second implementation.
"""

import functools
import math

import numpy as np
import pytest
import torch

from tests import aux_cases as ac

F32 = np.float32
KS = (0, 1, 10, 5000)
EDGE_SIZES = (127, 128, 129, 2047, 2048, 6, 9)


def _groups(c):
    gp = c["group_ptr"]
    return [(int(gp[g]), int(gp[g + 1])) for g in range(len(gp) - 1)]


def ref_stats(c, k):
    """-> (stats [G, 4] = [dcg@k, idcg@k, idcg, ap], terms [G, 4]): every
    sum by math.fsum; ``terms`` is the number of terms of each sum."""
    rank, _ = c["prep"]
    out, terms = [], []
    for s, e in _groups(c):
        L = e - s
        kk = L if k <= 0 or k > L else k
        order = np.argsort(rank[s:e])
        y = c["label"][s:e].astype(np.float64)
        gain = np.exp2(y) - 1.0
        disc = 1.0 / np.log2(np.arange(L, dtype=np.float64) + 2.0)
        ideal = np.sort(gain)[::-1] * disc
        rel = y[order] > 0
        hits = np.cumsum(rel)[rel] / (np.flatnonzero(rel) + 1.0)
        out.append([math.fsum((gain[order] * disc)[:kk]),
                    math.fsum(ideal[:kk]), math.fsum(ideal),
                    math.fsum(hits) / rel.sum() if rel.any() else 0.0])
        terms.append([kk, kk, L, L])
    return np.array(out), np.array(terms, np.float64)


def stats_bound(ref, terms):
    """One rounding per multiply and per add, 2 ulp in a gain, one division;
    all terms are non-negative, so the bound is relative."""
    return (2.0 * terms + 16.0) * 2.0 ** -53 * np.abs(ref)


def ref_scores(ref, name):
    """Per-group metric from the reference sums: ndcg = dcg@k / idcg@k (1
    without gain), map = ap (1 without a relevant row)."""
    if name == "map":
        return np.where(ref[:, 3] > 0, ref[:, 3], 1.0)
    with np.errstate(invalid="ignore"):
        return np.where(ref[:, 1] > 0, ref[:, 0] / ref[:, 1], 1.0)


def ref_lambdamap(c):
    """rank:map gradient pairs in float64 -> (gpair [n, 2], S [n, 2]), S the
    per-row sums of absolute pair terms (as ``aux_cases.ref_lambdarank``)."""
    rank, _ = c["prep"]
    out = np.zeros((c["n"], 2))
    S = np.zeros((c["n"], 2))
    for s, e in _groups(c):
        L = e - s
        m, y, r = c["margin"][s:e], c["label"][s:e], rank[s:e].astype(int)
        rel = (y[np.argsort(r)] > 0).astype(np.float64)
        win = y[:, None] > y[None, :]
        if L < 2 or not rel.any() or not win.any():
            continue
        pos = np.arange(1, L + 1, dtype=np.float64)
        t, Ssum = np.cumsum(rel) / pos, np.cumsum(rel / pos)
        lo = np.minimum(r[:, None], r[None, :])
        hi = np.maximum(r[:, None], r[None, :])
        delta = np.abs(t[hi] - t[lo] - (Ssum[np.maximum(hi - 1, 0)]
                                        - Ssum[lo])) / rel.sum()
        d = (m[:, None] - m[None, :]).astype(np.float64)  # float32 subtract
        with np.errstate(over="ignore"):
            rho = 1.0 / (1.0 + np.exp(d))
        lam = np.where(win, rho * delta, 0.0)
        hess = np.where(win, np.maximum(rho * (1.0 - rho), ac.EPS) * delta,
                        0.0)
        out[s:e, 0] = -lam.sum(1) + lam.sum(0)
        S[s:e, 0] = lam.sum(1) + lam.sum(0)
        out[s:e, 1] = S[s:e, 1] = hess.sum(1) + hess.sum(0)
    return out, S


def _finish(c):
    c["prep"] = ac.ref_rank_prep(c["margin"], c["label"], c["group_ptr"])
    c["map"] = ref_lambdamap(c)
    for k in KS:
        c["stats", k] = ref_stats(c, k)
    return c


def _layout(name, sizes, seed):
    rng = np.random.RandomState(seed)
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(gp[-1])
    return {"id": name, "n": n, "group_ptr": gp,
            "margin": rng.randn(n).astype(F32),
            "label": rng.randint(0, 5, n).astype(F32),
            "qid": np.repeat(np.arange(len(sizes)), sizes).astype(np.int64),
            "weight": (rng.rand(n) * 2.0).astype(F32)}


@functools.lru_cache(maxsize=None)
def cases():
    """aux_cases' ranking layouts plus the edges of the new kernels: the
    power-of-two pads around 128 and 2048, +0.0 / -0.0 margins in one group
    (of 6 rows) and a group (of 9 rows) whose labels are all 0."""
    e = _layout("edges", EDGE_SIZES, 4201)
    z = int(e["group_ptr"][5])
    e["margin"][z:z + 6] = np.array([0.0, -0.0, 1.0, -0.0, 0.0, -1.0], F32)
    e["label"][z:z + 6] = np.array([0, 2, 1, 3, 1, 4], F32)
    e["label"][z + 6:z + 15] = 0.0
    e["ref", True] = ac.ref_lambdarank(e["margin"], e["label"],
                                       e["group_ptr"], True)
    return tuple(_finish(dict(c)) for c in
                 ac.rank_cases() + (ac.rank_round0_case(), e))


@functools.lru_cache(maxsize=None)
def long_group_case():
    """One group of 2049 rows: longer than RANK_LDS_MAX_GROUP."""
    c = _layout("g2049", (2049,), 4202)
    c["ref", True] = ac.ref_lambdarank(c["margin"], c["label"],
                                       c["group_ptr"], True)
    return _finish(c)


def ids(cs):
    return [c["id"] for c in cs]


def rank_bound(ref, S):
    """The project's ranking bound (tests/test_aux_ops_gpu.py)."""
    return 2.0 ** -23 * np.abs(ref) + 1e-12 * S


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("c", cases(), ids=ids(cases()))
def test_cpu_rank_group_stats(c, k):
    from xgboost_ray_amd import ops

    rank, stats = ops.rank_group_stats(
        _t(c["margin"]), _t(c["label"]), _t(c["group_ptr"]),
        ops.rank_disc_table("cpu"), k)
    assert np.array_equal(rank.numpy(), c["prep"][0])
    ref, terms = c["stats", k]
    assert (np.abs(stats.numpy() - ref) <= stats_bound(ref, terms)).all()
    assert np.allclose(ref[:, 2], c["prep"][1], rtol=1e-13, atol=0)


@pytest.mark.parametrize("c", cases(), ids=ids(cases()))
def test_cpu_lambdamap_grad(c):
    from xgboost_ray_amd import ops

    got = ops.lambdamap_grad(_t(c["margin"]), _t(c["label"]),
                             _t(c["group_ptr"])).numpy().astype(np.float64)
    ref, S = c["map"]
    assert got.shape == ref.shape and (c["n"] == 1 or np.abs(ref).max() > 0)
    assert (np.abs(got - ref) <= rank_bound(ref, S)).all()


def test_cpu_objective_and_metrics_keep_the_torch_route():
    from xgboost_ray_amd.engine.metrics import get_metric
    from xgboost_ray_amd.engine.objectives import RankMAP

    c = cases()[0]
    m, y, q = _t(c["margin"]), _t(c["label"]), _t(c["qid"])
    obj = RankMAP()
    got = obj.gradients(m, y, None, q).numpy().astype(np.float64)
    ref, S = c["map"]
    # the CPU loop accumulates a row's pair terms in float32
    assert (np.abs(got - ref) <= 2.0 ** -23 * (np.abs(ref) + 700 * S)).all()
    for name in ("ndcg@10", "map"):
        met = get_metric(name)
        st = met.local_stats(m, y, None, q, None)
        assert met.last_route == "torch" and st[1] == len(c["sizes"])
        score = ref_scores(c["stats", 10][0], name)
        assert abs(float(st[0]) - math.fsum(score)) <= 1e-12 * len(score)
