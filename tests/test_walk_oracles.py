"""The CPU oracles of the leaf-index and Saabas walks against the
independent references of ``walk_cases``, against the Booster's own numpy
walks, and the sklearn ``apply()`` built on them. Every comparison is
exact."""

import numpy as np
import pytest
import torch

import shap_cases as sc
import walk_cases as wc
from xgboost_ray_amd import (RayParams, RayXGBClassifier, RayXGBRegressor,
                             ops)
from xgboost_ray_amd.booster import _fill_node_means
from xgboost_ray_amd.ops import cpu, gpu

F_LDS = gpu.saabas_lds_max_features()
# a narrower block (34), the last width with LDS sums, the first without
WIDE = wc.wide_cases((34, F_LDS, F_LDS + 1))
ALL = list(wc.walk_cases()) + list(WIDE)
_id = lambda c: c["id"]  # noqa: E731


def test_wide_cases_straddle_the_lds_budget():
    assert [c["F"] for c in WIDE] == [34, F_LDS, F_LDS + 1]
    room = gpu.SAABAS_LDS_BYTES - 24 * gpu.SAABAS_TILE_NODES
    assert gpu.saabas_block_threads(33) == gpu.SAABAS_THREADS
    assert 64 <= gpu.saabas_block_threads(34) < gpu.SAABAS_THREADS
    for F in (1, 28, 33, 34, F_LDS):
        t = gpu.saabas_block_threads(F)
        assert t % 64 == 0 and 8 * t * (F + 1) <= room
    assert gpu.saabas_block_threads(F_LDS) == 64
    assert 8 * 64 * (F_LDS + 2) > room
    assert gpu.saabas_block_threads(F_LDS + 1) == 0


@pytest.mark.parametrize("case", ALL, ids=_id)
def test_predict_leaf_oracle(case):
    f = wc.torch_forest(case["forest"])
    out = torch.full((case["n"], case["T"]), -7, dtype=torch.int32)
    got = ops.predict_leaf(torch.from_numpy(case["X"]), f["feat"], f["thr"],
                           f["left"], f["default_left"], f["tree_ptr"], out)
    assert got is out
    assert np.array_equal(out.numpy(), case["ref_leaves"])


@pytest.mark.parametrize("case", ALL, ids=_id)
def test_saabas_oracle(case):
    f = wc.torch_forest(case["forest"])
    out = torch.from_numpy(case["out0"].copy())
    ops.saabas_contribs(torch.from_numpy(case["X"]), f["feat"], f["thr"],
                        f["left"], f["default_left"],
                        torch.from_numpy(case["node_mean"]), f["tree_ptr"],
                        out)
    assert np.array_equal(out.numpy(), case["ref_saabas"])


def test_saabas_oracle_into_a_strided_group_slice():
    case = wc.walk_cases()[1]
    f = wc.torch_forest(case["forest"])
    n, F = case["n"], case["F"]
    full = torch.full((n, 3, F + 1), 0.125, dtype=torch.float64)
    full[:, 1, :] = torch.from_numpy(case["out0"])
    cpu.saabas_contribs(torch.from_numpy(case["X"]), f["feat"], f["thr"],
                        f["left"], f["default_left"],
                        torch.from_numpy(case["node_mean"]), f["tree_ptr"],
                        full[:, 1, :])
    assert np.array_equal(full[:, 1, :].numpy(), case["ref_saabas"])
    assert (full[:, 0, :] == 0.125).all() and (full[:, 2, :] == 0.125).all()


def test_walk_rejects_a_forest_that_leaves_its_arrays():
    case = wc.walk_cases()[1]
    f = wc.torch_forest(case["forest"])
    X = torch.from_numpy(case["X"])
    out = torch.zeros((case["n"], case["T"]), dtype=torch.int32)
    args = lambda **kw: [  # noqa: E731
        {**f, **kw}[k] for k in ("feat", "thr", "left", "default_left",
                                 "tree_ptr")]
    with pytest.raises(ValueError, match="splits on feature"):
        ops.predict_leaf(X[:, :-1].contiguous(), *args(), out)
    split = int(np.nonzero(case["forest"]["feat"] >= 0)[0][-1])
    for bad in (0, 10 ** 6):
        left = f["left"].clone()
        left[split] = bad
        with pytest.raises(ValueError, match="children"):
            ops.predict_leaf(X, *args(left=left), out)


# -- against the Booster's numpy walks ----------------------------------------

def _case_forest(case, idx):
    """Flat arrays (and node means) of the case's trees ``idx``."""
    trees = [case.trees[i] for i in idx]
    means = []
    for t in trees:
        m = np.zeros(t.num_nodes, np.float64)
        _fill_node_means(t, m, t.cover.astype(np.float64))
        means.append(m)
    cat = lambda name, dt: torch.from_numpy(  # noqa: E731
        np.concatenate([getattr(t, name) for t in trees]).astype(dt))
    return (cat("feat", np.int32), cat("thr", np.float32),
            cat("left", np.int32), cat("default_left", np.uint8),
            torch.from_numpy(np.concatenate(means)),
            torch.from_numpy(np.cumsum(
                [0] + [t.num_nodes for t in trees]).astype(np.int32)))


@pytest.mark.parametrize("case", sc.CASES + [sc.WIDE], ids=repr)
def test_ops_equal_the_booster_walks(case):
    assert {c.n_groups for c in sc.CASES} >= {1, 3}
    assert any(c.scale == 0.5 for c in sc.CASES)  # num_parallel_tree = 2
    bst = sc.case_booster(case)
    X = torch.from_numpy(case.X)
    n, F, G = len(case.X), case.F, case.n_groups

    feat, thr, left, dl, _, ptr = _case_forest(case, range(len(case.trees)))
    leaves = torch.zeros((n, len(case.trees)), dtype=torch.int32)
    ops.predict_leaf(X, feat, thr, left, dl, ptr, leaves)
    want = bst.predict(case.X, pred_leaf=True)
    assert want.dtype == np.int32
    assert np.array_equal(leaves.numpy(), want)

    want = bst.predict(case.X, pred_contribs=True, approx_contribs=True)
    base = float(bst._obj().prob_to_margin(bst.base_score))
    out = torch.zeros((n, G, F + 1), dtype=torch.float64)
    out[:, :, F] += base
    for g in range(G):
        idx = [i for i, gi in enumerate(case.groups) if gi == g]
        feat, thr, left, dl, mean, ptr = _case_forest(case, idx)
        ops.saabas_contribs(X, feat, thr, left, dl, mean, ptr, out[:, g, :])
    assert np.array_equal(out.numpy().reshape(want.shape), want)


# -- sklearn apply() ----------------------------------------------------------

RP = RayParams(num_actors=2)


def _data(n_classes=None):
    rng = np.random.RandomState(5)
    X = rng.randn(300, 6).astype(np.float32)
    X[rng.rand(300, 6) < 0.1] = np.nan
    s = np.nan_to_num(X[:, 0]) + 0.5 * np.nan_to_num(X[:, 1])
    if n_classes is None:
        return X, s.astype(np.float32)
    return X, np.digitize(s, np.quantile(s, [1 / 3, 2 / 3])[:n_classes - 1])


@pytest.mark.parametrize("kind", ["regressor", "classifier3"])
def test_sklearn_apply(kind):
    if kind == "regressor":
        X, y = _data()
        est = RayXGBRegressor(n_estimators=4, max_depth=3)
        per_round = 1
    else:
        X, y = _data(3)
        est = RayXGBClassifier(n_estimators=4, max_depth=3)
        per_round = 3
    est.fit(X, y, ray_params=RP)
    bst = est.get_booster()
    leaves = est.apply(X, ray_params=RP)
    assert leaves.dtype == np.int32
    assert leaves.shape == (300, 4 * per_round)
    assert np.array_equal(leaves, bst.predict(X, pred_leaf=True))
    assert leaves.max() > 0
    part = est.apply(X, iteration_range=(1, 3), ray_params=RP)
    assert part.shape == (300, 2 * per_round)
    assert np.array_equal(
        part, bst.predict(X, pred_leaf=True, iteration_range=(1, 3)))
    assert np.array_equal(part, leaves[:, per_round:3 * per_round])
