"""Path-form TreeSHAP on the CPU: ``ops.cpu.shap_paths`` /
``tree_shap`` / ``tree_shap_interactions`` against brute-force Shapley
values and against the ``booster._tree_shap`` recursion."""

import warnings

import numpy as np
import pytest
import torch

import shap_cases as sc
from xgboost_ray_amd import booster as booster_mod
from xgboost_ray_amd import ops
from xgboost_ray_amd.ops import cpu

N_BRUTE = 10


def _contribs(case, X):
    out = np.zeros((len(X), case.n_groups, case.F + 1), np.float64)
    cpu.tree_shap(X, sc.case_paths(case), case.n_groups, out)
    return out


def _recursion(case, X):
    with warnings.catch_warnings():  # 0/0 on cover-0 nodes
        warnings.simplefilter("ignore")
        return sc.recursion_contribs(case, X)


@pytest.fixture(scope="module")
def op_and_recursion():
    """(op, recursion) contributions of every case, computed once."""
    return {c.name: (_contribs(c, c.X), _recursion(c, c.X))
            for c in sc.CASES}


@pytest.mark.parametrize("case", sc.BRUTE_CASES, ids=repr)
def test_tree_shap_vs_brute_force(case, op_and_recursion):
    got = op_and_recursion[case.name][0][:N_BRUTE]
    want = sc.brute_force_contribs(case, case.X[:N_BRUTE])
    assert np.isfinite(got).all()
    assert np.abs(got[:, :, :case.F] - want).max() < sc.BRUTE_TOL
    assert (got[:, :, case.F] == 0).all()  # the bias column is the caller's


def test_tree_shap_vs_recursion(op_and_recursion):
    """Measures d over the whole case set; it must not exceed the
    recorded constant. Rows on which the recursion divides 0 by 0 (they
    miss a cover-0 node) are compared with brute force above instead."""
    d = 0.0
    for case in sc.CASES:
        got, ref = op_and_recursion[case.name]
        assert np.isfinite(got).all()
        finite = np.isfinite(ref).all(axis=(1, 2))
        if case.name == "zero_cover":
            assert not finite.any()
            continue
        if case.name == "zero_leaf":
            assert 0 < finite.sum() < len(finite)
        else:
            assert finite.all()
        diff = np.abs(got[..., :case.F] - ref[..., :case.F])[finite].max()
        print(f"{case.name}: d = {diff!r}")
        d = max(d, diff)
        # the recursion's bias column is what shap_paths reports
        bias = sc.case_paths(case)["bias"]
        assert np.abs(ref[finite][:, :, case.F] - bias[None]).max() <= sc.SHAP_D
    print(f"case set: d = {d!r}")
    assert d <= sc.SHAP_D


@pytest.mark.parametrize("case", sc.CASES, ids=repr)
def test_additivity(case, op_and_recursion):
    got = op_and_recursion[case.name][0]
    bias = sc.case_paths(case)["bias"]
    total = got.sum(-1) + bias[None, :]
    assert np.abs(total - sc.margins(case, case.X)).max() < sc.ADDITIVITY_TOL


@pytest.mark.parametrize(
    "case", [c for c in sc.CASES if c.n_groups == 1], ids=repr)
def test_interactions_vs_booster(case):
    X = case.X[:16]
    F = case.F
    bst = sc.case_booster(case)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = bst.predict_interactions(X)
    paths = sc.case_paths(case)
    M = np.zeros((len(X), F + 1, F + 1), np.float64)
    cpu.tree_shap_interactions(X, paths, M)
    assert (np.diagonal(M, axis1=1, axis2=2) == 0).all()
    assert (M[:, F, :] == 0).all() and (M[:, :, F] == 0).all()
    # host post-processing, as Booster.predict_interactions does it
    contribs = _contribs(case, X)[:, 0]
    contribs[:, F] += paths["bias"][0] + bst._obj().prob_to_margin(
        bst.base_score)
    M[:, :F, :F] = (M[:, :F, :F] + np.transpose(M[:, :F, :F],
                                                (0, 2, 1))) / 2.0
    for i in range(F):
        M[:, i, i] = contribs[:, i] - M[:, i, :F].sum(axis=1)
    M[:, F, F] = contribs[:, F]
    finite = np.isfinite(want).all(axis=(1, 2))
    if case.name == "zero_cover":
        assert not finite.any()
    else:
        assert finite.any()
        assert np.abs(M - want)[finite].max() <= sc.inter_cpu_tol(F)
    # every row, finite in the recursion or not: the matrix sums to the
    # margin
    margin = sc.margins(case, X)[:, 0] + bst._obj().prob_to_margin(
        bst.base_score)
    assert np.abs(M.sum(axis=(1, 2)) - margin).max() < sc.ADDITIVITY_TOL


def test_shap_paths_invariants():
    for case in sc.CASES + [sc.WIDE]:
        p = sc.case_paths(case)
        ptr = p["path_ptr"]
        assert ptr[0] == 0 and ptr[-1] == len(p["feature"])
        assert (p["lo"] < p["hi"]).all()  # no empty interval
        assert p["n_groups"] == case.n_groups
        assert len(p["value"]) == sum(
            int((t.feat < 0).sum()) for t in case.trees)
        prod = np.ones(len(ptr) - 1)
        for i in range(len(ptr) - 1):
            feats = p["feature"][ptr[i]:ptr[i + 1]]
            assert len(set(feats.tolist())) == len(feats)  # merged
            prod[i] = np.prod(p["zero_fraction"][ptr[i]:ptr[i + 1]])
        per_tree = np.bincount(p["tree"], weights=prod,
                               minlength=len(case.trees))
        assert np.abs(per_tree - 1.0).max() < 1e-12


def test_shap_paths_merge_and_root_only():
    p = cpu.shap_paths([sc.build_tree(sc.REPEAT),
                        sc.build_tree(sc.ROOT_ONLY)], [1.0, 0.5])
    ptr = p["path_ptr"]
    # REPEAT, second leaf: root left (thr .5, default left), then right
    # (thr .2, default right), then left (thr .4, default left, NOT
    # followed) - three splits on feature 0, one element
    assert ptr[1] + 1 == ptr[2]
    e = ptr[1]
    assert p["feature"][e] == 0
    assert p["lo"][e] == np.float32(0.2) and p["hi"][e] == np.float32(0.4)
    assert p["miss_ok"][e] == 1
    assert p["zero_fraction"][e] == pytest.approx(10 / 18 * 7 / 10 * 2 / 7)
    # the third leaf takes the third split to the right, against its
    # default, and then splits on feature 1
    assert ptr[2] + 2 == ptr[3] and p["feature"][ptr[2] + 1] == 1
    e = ptr[2]
    assert p["feature"][e] == 0 and p["miss_ok"][e] == 0
    assert p["lo"][e] == np.float32(0.4) and p["hi"][e] == np.float32(0.5)
    # the root-only tree: one path without elements, bias only
    assert ptr[-1] == ptr[-2]
    assert p["value"][-1] == 0.75 * 0.5
    t0 = sc.build_tree(sc.REPEAT)
    mean = np.zeros(t0.num_nodes)
    booster_mod._fill_node_means(t0, mean, t0.cover.astype(np.float64))
    assert p["bias"][0] == mean[0] + 0.75 * 0.5


def test_path_length_cap_falls_back(monkeypatch):
    cap = ops.SHAP_MAX_PATH_LEN
    long_tree, ok_tree = sc.chain_tree(cap + 1), sc.chain_tree(cap)
    assert cpu.shap_paths([ok_tree])["max_len"] == cap
    paths = cpu.shap_paths([long_tree])
    assert paths["max_len"] == cap + 1
    X = sc.rows(cap + 1, n=6, seed=5)
    with pytest.raises(ValueError):
        cpu.tree_shap(X, paths, 1, np.zeros((6, 1, cap + 2)))
    with pytest.raises(ValueError):
        ops.tree_shap(torch.from_numpy(X), paths, 1,
                      torch.zeros((6, 1, cap + 2), dtype=torch.float64))
    # the Booster route: the batch qualifies for the device, the forest
    # does not, so the recursion runs and the op is never reached
    bst = booster_mod.Booster(
        {"objective": "reg:squarederror", "num_feature": cap + 1},
        [long_tree], [0])
    want = bst.predict(X, pred_contribs=True)

    def boom(*a, **k):
        raise AssertionError("device op reached")

    monkeypatch.setattr(booster_mod, "SHAP_GPU_MIN_ROWS", 4)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(ops, "tree_shap", boom)
    assert bst._shap_device_paths(6, cap + 1, 0, 1) is None
    got = bst.predict(X, pred_contribs=True)
    assert np.array_equal(got, want, equal_nan=True)


def test_small_batches_never_build_paths(monkeypatch):
    case = sc.CASES[0]
    bst = sc.case_booster(case)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    assert bst._shap_device_paths(booster_mod.SHAP_GPU_MIN_ROWS - 1,
                                  case.F, 0, 1) is None
    assert bst._shap_cache is None
    monkeypatch.setenv("RXGB_SHAP_GPU", "0")
    assert bst._shap_device_paths(booster_mod.SHAP_GPU_MIN_ROWS,
                                  case.F, 0, 1) is None
