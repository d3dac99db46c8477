"""LambdaRank with top-k pair truncation: the float64 reference, the shared
cases and the CPU routes; ``test_rank_topk_gpu.py`` runs the HIP kernels
against the same reference, which imports nothing from the package."""

import functools

import numpy as np
import pytest
import torch

from tests import aux_cases as ac
from tests.utils import create_labeled_sorted_rank_data

KS = (1, 2, 63, 64, 65, 300, 4096)
PM, PK = "lambdarank_pair_method", "lambdarank_num_pair_per_sample"


def ref_lambdarank_topk(margin, label, group_ptr, ndcg, k):
    """``aux_cases.ref_lambdarank`` over the pairs (i, j), label_i > label_j,
    with min(rank_i, rank_j) < k -> (gpair [n, 2], S [n, 2]); rank and the
    untruncated idcg from ``aux_cases.ref_rank_prep``."""
    m32, y32 = np.asarray(margin, np.float32), np.asarray(label, np.float32)
    out, S = np.zeros((len(m32), 2)), np.zeros((len(m32), 2))
    rank, idcg = ac.ref_rank_prep(m32, y32, group_ptr)
    for gi in range(len(group_ptr) - 1):
        s, e = int(group_ptr[gi]), int(group_ptr[gi + 1])
        if e - s < 2 or (ndcg and not idcg[gi] > 0.0):
            continue
        m, y, r = m32[s:e], y32[s:e], rank[s:e]
        win = (y[:, None] > y[None, :]) \
            & (np.minimum(r[:, None], r[None, :]) < k)
        d = (m[:, None] - m[None, :]).astype(np.float64)   # float32 subtract
        with np.errstate(over="ignore"):
            rho = 1.0 / (1.0 + np.exp(d))
        hess = np.maximum(rho * (1.0 - rho), ac.EPS)
        if ndcg:
            gain = np.exp2(y.astype(np.float64)) - 1.0
            disc = 1.0 / np.log2(r.astype(np.float64) + 2.0)
            w = np.abs((gain[:, None] - gain[None, :])
                       * (disc[:, None] - disc[None, :])) / idcg[gi]
            rho, hess = rho * w, hess * w
        rho, hess = np.where(win, rho, 0.0), np.where(win, hess, 0.0)
        out[s:e, 0] = -rho.sum(1) + rho.sum(0)
        S[s:e, 0] = rho.sum(1) + rho.sum(0)
        out[s:e, 1] = S[s:e, 1] = hess.sum(1) + hess.sum(0)
    return out, S


@functools.lru_cache(maxsize=None)
def cases():
    """sizes-a; round 0 (every margin tied); the LDS maximum next to a group
    just past a power of two; random margins in groups of at most a wave."""
    return (ac.rank_cases()[0], ac.rank_round0_case(),
            ac._rank_case("g2048", (2048, 1025, 5), 4301),
            ac._rank_case("g64", (64, 63, 40, 33, 2), 4302))


@functools.lru_cache(maxsize=None)
def ref(ci, ndcg, k):
    c = cases()[ci]
    return ref_lambdarank_topk(c["margin"], c["label"], c["group_ptr"],
                               ndcg, k)


def rank_bound(r, S):     # the project's ranking bound (docs/parity.md)
    return 2.0 ** -23 * np.abs(r) + 1e-12 * S


def weighted(r, bound, w):  # one more float32 multiply, by an exact weight
    w64 = w.astype(np.float64)[:, None]
    return r * w64, bound * w64 + 2.0 ** -23 * np.abs(r * w64)


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def topk_objective(ndcg, k):
    from xgboost_ray_amd.engine.objectives import RankNDCG, RankPairwise

    obj = RankNDCG() if ndcg else RankPairwise()
    obj.pair_method, obj.topk = "topk", k
    return obj


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("ndcg", [False, True])
@pytest.mark.parametrize("ci", range(4))
def test_cpu_op_matches_reference(ci, ndcg, k):
    from xgboost_ray_amd import ops

    c = cases()[ci]
    r, S = ref(ci, ndcg, k)
    # the reference's own check: all pairs once k covers every group (the
    # last rank has no partner below it, so L - 1 already does)
    full = all(np.array_equal(a, b) for a, b in zip((r, S), c["ref", ndcg]))
    assert full == (k >= max(c["sizes"]) - 1)
    got = ops.lambdarank_topk_grad(
        _t(c["margin"]), _t(c["label"]), _t(c["group_ptr"]),
        ops.rank_disc_table("cpu"), k, ndcg).numpy()
    assert got.shape == r.shape
    assert (np.abs(got - r) <= rank_bound(r, S)).all()


@pytest.mark.parametrize("wt", [False, True])
@pytest.mark.parametrize("k", [2, 65])
@pytest.mark.parametrize("ndcg", [False, True])
def test_cpu_objective_matches_reference(ndcg, k, wt):
    c = cases()[0]
    obj = topk_objective(ndcg, k)
    w = c["weight"] if wt else None
    got = obj.gradients(_t(c["margin"]), _t(c["label"]), _t(w),
                        _t(c["qid"])).numpy()
    assert obj.last_route == "torch"
    r, S = ref(0, ndcg, k)
    # float32 terms summed in float32: L * 2^-24 * S_i (docs/parity.md)
    L = np.repeat(np.asarray(c["sizes"]), c["sizes"])[:, None]
    bound = L * ac.U24 * S
    if wt:
        r, bound = weighted(r, bound, w)
    assert (np.abs(got - r) <= bound).all()


@pytest.mark.parametrize("params", [
    {PM: "mean"}, {PM: "topk", PK: 0}, {PM: "all", PK: 8},
    {PM: "topk", "objective": "rank:map"}])
def test_bad_parameters_raise(params):
    from xgboost_ray_amd.engine.trainer import TrainParams

    with pytest.raises(ValueError, match="lambdarank|rank:map"):
        TrainParams.from_dict({"objective": "rank:ndcg", **params})
    p = TrainParams.from_dict({PM: "topk"})
    assert p.lambdarank_num_pair_per_sample == 32
    assert TrainParams.from_dict(
        {PM: "topk", PK: "8"}).lambdarank_num_pair_per_sample == 8


def test_all_is_unchanged_and_topk_reaches_the_objective():
    from xgboost_ray_amd import RayParams, RayXGBRanker
    from xgboost_ray_amd.engine.quantile import BinnedMatrix
    from xgboost_ray_amd.engine.trainer import run_training

    X, y, qid = create_labeled_sorted_rank_data(n_groups=8, group_size=20)
    dm = BinnedMatrix.build(_t(X), label=_t(y), qid=_t(qid), max_bin=32)

    def model(**extra):
        return run_training({"objective": "rank:ndcg", "max_depth": 3,
                             **extra}, dm, 3).save_raw()

    def margins(**kw):      # sklearn kwargs -> params -> an actor
        rk = RayXGBRanker(n_estimators=3, max_depth=3, **kw)
        rk.fit(X, y, qid=qid, ray_params=RayParams(num_actors=1))
        return rk.predict(X, output_margin=True)

    assert model(**{PM: "all"}) == model()
    assert model(**{PM: "topk", PK: 1}) != model()
    assert not np.array_equal(margins(**{PM: "topk", PK: 1}), margins())
