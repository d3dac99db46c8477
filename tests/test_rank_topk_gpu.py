"""``lambdarank_topk_grad`` on the GPU and its routes against the float64
reference and cases of ``tests/test_rank_topk_cpu.py`` (bound:
docs/parity.md, "Ranking on the device")."""

import numpy as np
import pytest
import torch

from tests import test_rank_topk_cpu as tc

pytestmark = pytest.mark.gpu
TOPK8 = {"objective": "rank:ndcg", "tree_method": "gpu_hist", "max_depth": 4,
         "eval_metric": ["ndcg@8"], tc.PM: "topk", tc.PK: 8}


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check(ci, ndcg, k, **kw):
    from xgboost_ray_amd import ops

    c = tc.cases()[ci]
    args = (_d(c["margin"]), _d(c["label"]), _d(c["group_ptr"]),
            ops.rank_disc_table("cuda"), k, ndcg)
    got = ops.lambdarank_topk_grad(*args, **kw)
    assert torch.equal(got, ops.lambdarank_topk_grad(*args, **kw))
    r, S = tc.ref(ci, ndcg, k)
    got = got.cpu().numpy()
    # a group longer than max_len is left untouched
    live = np.repeat(np.asarray(c["sizes"]) <= kw.get("max_len", 2048),
                     c["sizes"])
    assert not got[~live].any() and (live.all() or r[~live].any())
    err, bound = np.abs(got - r)[live], tc.rank_bound(r, S)[live]
    print("largest error / bound:",
          (err / np.where(bound > 0, bound, 1)).max())
    assert got.shape == r.shape and (err <= bound).all()
    # rows without a counted pair (k = 1: every row that shares the top
    # row's label) and groups of one row: exact zeros
    none = S[:, 1] == 0
    single = np.repeat(np.asarray(c["sizes"]) == 1, c["sizes"])
    assert none[single].all() and (k > 1 or none.sum() > single.sum())
    assert not got[none].any()


@pytest.mark.parametrize("k", tc.KS)
@pytest.mark.parametrize("ndcg", [False, True])
@pytest.mark.parametrize("ci", range(4))
def test_topk_grad(ci, ndcg, k):
    _check(ci, ndcg, k)


@pytest.mark.parametrize("k", [1, 2, 32])
@pytest.mark.parametrize("ndcg", [False, True])
@pytest.mark.parametrize("variant", [1, 2])
def test_both_variants_on_shuffled_short_groups(variant, ndcg, k):
    _check(3, ndcg, k, variant=variant)     # 1: a wave per group, k < L


def test_group_longer_than_max_len_is_rejected_or_untouched():
    with pytest.raises(RuntimeError, match="RANK_LDS_MAX_GROUP"):
        _check(0, True, 2, max_len=2049)
    _check(0, True, 2, max_len=256)         # sizes-a holds 257 and 700


@pytest.mark.parametrize("gpu_rank", ["1", "0"])
@pytest.mark.parametrize("ci,ndcg,k", [(0, False, 2), (0, True, 65),
                                       (1, True, 2), (2, True, 64),
                                       (3, True, 32)])
def test_objective_route(ci, ndcg, k, gpu_rank, monkeypatch):
    monkeypatch.setenv("RXGB_RANK_GPU", gpu_rank)
    c = tc.cases()[ci]
    obj = tc.topk_objective(ndcg, k)
    got = obj.gradients(_d(c["margin"]), _d(c["label"]), _d(c["weight"]),
                        _d(c["qid"])).cpu().numpy()
    assert obj.last_route == ("hip" if gpu_rank == "1" else "torch")
    r, S = tc.ref(ci, ndcg, k)
    r, bound = tc.weighted(r, tc.rank_bound(r, S), c["weight"])
    assert (np.abs(got - r) <= bound).all()


def test_train_on_the_gpu(monkeypatch):
    """``train()`` through a GPU actor must improve ndcg@8; the loop it runs
    there, run in this process, shows the objective's route."""
    from xgboost_ray_amd import RayDMatrix, RayParams, train
    from xgboost_ray_amd.engine.objectives import RankNDCG
    from xgboost_ray_amd.engine.quantile import BinnedMatrix
    from xgboost_ray_amd.engine.trainer import run_training

    rng = np.random.RandomState(4400)
    sizes = rng.randint(5, 81, 60)
    X = rng.randn(int(sizes.sum()), 8).astype(np.float32)
    y = np.digitize(X[:, 0] + 0.5 * rng.randn(len(X)), [0.0, 1.0]).astype(
        np.float32)
    qid = np.repeat(np.arange(60), sizes)
    res = {}
    train(TOPK8, RayDMatrix(X, y, qid=qid), 5, evals_result=res,
          evals=[(RayDMatrix(X, y, qid=qid), "train")],
          ray_params=RayParams(num_actors=1, gpus_per_actor=1))
    assert res["train"]["ndcg@8"][-1] > res["train"]["ndcg@8"][0]
    routes, inner = [], RankNDCG.gradients

    def spy(self, *a, **kw):
        out = inner(self, *a, **kw)
        routes.append((self.pair_method, self.topk, self.last_route))
        return out

    monkeypatch.setattr(RankNDCG, "gradients", spy)
    dm = BinnedMatrix.build(_d(X), label=_d(y), qid=_d(qid), max_bin=64)
    run_training(TOPK8, dm, 5)
    assert routes == [("topk", 8, "hip")] * 5
