"""The HIP ranking kernels and their public routes against the float64
references and cases of ``tests/test_rank_ops_cpu.py`` (bounds: docs/parity.md,
"Ranking on the device")."""

import math

import numpy as np
import pytest
import torch

from tests import test_rank_ops_cpu as rc

pytestmark = pytest.mark.gpu

CASES = rc.cases()
ALL = CASES + (rc.long_group_case(),)   # the last one takes the torch route


def _d(a):
    return None if a is None else torch.from_numpy(
        np.ascontiguousarray(a)).cuda()


def _route(c):
    return "torch" if c["id"] == "g2049" else "hip"


@pytest.mark.parametrize("k", rc.KS)
@pytest.mark.parametrize("c", CASES, ids=rc.ids(CASES))
def test_rank_group_stats(c, k):
    from xgboost_ray_amd import ops

    args = (_d(c["margin"]), _d(c["label"]), _d(c["group_ptr"]),
            ops.rank_disc_table("cuda"), k)
    rank, stats = ops.rank_group_stats(*args)
    rank2, stats2 = ops.rank_group_stats(*args)
    assert np.array_equal(rank.cpu().numpy(), c["prep"][0])
    assert torch.equal(rank, rank2) and torch.equal(stats, stats2)
    ref, terms = c["stats", k]
    err = np.abs(stats.cpu().numpy() - ref)
    bound = rc.stats_bound(ref, terms)
    print(c["id"], k, "largest error / bound:",
          (err / np.where(bound > 0, bound, 1.0)).max())
    assert (err <= bound).all()


@pytest.mark.parametrize("c", CASES, ids=rc.ids(CASES))
def test_lambdamap_grad(c):
    from xgboost_ray_amd import ops

    args = (_d(c["margin"]), _d(c["label"]), _d(c["group_ptr"]))
    got = ops.lambdamap_grad(*args)
    assert torch.equal(got, ops.lambdamap_grad(*args))
    ref, S = c["map"]
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
    assert got.shape == ref.shape and (err <= rc.rank_bound(ref, S)).all()


@pytest.mark.parametrize("weighted", [False, True], ids=["nw", "w"])
@pytest.mark.parametrize("name", ["rank:map", "rank:ndcg"])
@pytest.mark.parametrize("c", ALL, ids=rc.ids(ALL))
def test_objective_route(c, name, weighted):
    from xgboost_ray_amd.engine.objectives import get_objective

    obj = get_objective(name)
    w = c["weight"] if weighted else None
    got = obj.gradients(_d(c["margin"]), _d(c["label"]), _d(w),
                        _d(c["qid"])).cpu().numpy().astype(np.float64)
    assert obj.last_route == _route(c)
    ref, S = c["map"] if name == "rank:map" else c["ref", True]
    bound = rc.rank_bound(ref, S)
    if weighted:    # one more float32 multiply, by an exact float32 weight
        w64 = w.astype(np.float64)[:, None]
        ref = ref * w64
        bound = bound * w64 + 2.0 ** -23 * np.abs(ref)
    err = np.abs(got - ref)
    print(c["id"], name, obj.last_route, "largest error / bound:",
          (err / np.where(bound > 0, bound, 1.0)).max(),
          "errors where the bound is 0:", err[bound == 0].max(initial=0.0))
    assert (err <= bound).all()


@pytest.mark.parametrize("name", ["ndcg@10", "ndcg", "map"])
@pytest.mark.parametrize("c", ALL, ids=rc.ids(ALL))
def test_metric_route(c, name):
    from xgboost_ray_amd.engine.metrics import get_metric

    met = get_metric(name)
    st = met.local_stats(_d(c["margin"]), _d(c["label"]), None, _d(c["qid"]),
                         None).cpu().numpy()
    assert met.last_route == _route(c)
    ref, terms = c["stats", 10 if name == "ndcg@10" else 0]
    score = rc.ref_scores(ref, name)
    m = terms[:, 3 if name == "map" else 0]
    # a score is a ratio of two bounded sums (or one sum): 2 (2 m + 16) + 1
    # roundings each; adding the G non-negative scores takes G - 1 more
    G = len(score)
    bound = (((4.0 * m + 33.0) * score).sum()
             + (G - 1) * score.sum()) * 2.0 ** -53
    assert st[1] == G and abs(st[0] - math.fsum(score)) <= bound
