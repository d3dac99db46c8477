"""The HIP path-form TreeSHAP kernels against their float64 numpy oracle
(``ops.cpu.tree_shap`` / ``tree_shap_interactions``), and the Booster's
routing of large pred_contribs / pred_interactions batches to them."""

import numpy as np
import pytest
import torch

import shap_cases as sc
from xgboost_ray_amd import booster as booster_mod
from xgboost_ray_amd import ops
from xgboost_ray_amd.ops import cpu

pytestmark = pytest.mark.gpu

SINGLE = [c for c in sc.CASES if c.n_groups == 1]


def _cpu_contribs(case, paths=None, X=None):
    X = case.X if X is None else X
    out = np.zeros((len(X), case.n_groups, case.F + 1), np.float64)
    cpu.tree_shap(X, paths or sc.case_paths(case), case.n_groups, out)
    return out


def _gpu_contribs(case, paths=None, X=None, device_out=False, **kw):
    X = case.X if X is None else X
    out = torch.zeros((len(X), case.n_groups, case.F + 1),
                      dtype=torch.float64,
                      device="cuda" if device_out else "cpu")
    ops.tree_shap(torch.from_numpy(X).cuda(), paths or sc.case_paths(case),
                  case.n_groups, out, **kw)
    return out.cpu()


def _cpu_inter(case, X=None):
    X = case.X if X is None else X
    out = np.zeros((len(X), case.F + 1, case.F + 1), np.float64)
    cpu.tree_shap_interactions(X, sc.case_paths(case), out)
    return out


def _gpu_inter(case, X=None, **kw):
    X = case.X if X is None else X
    out = torch.zeros((len(X), case.F + 1, case.F + 1), dtype=torch.float64)
    ops.tree_shap_interactions(torch.from_numpy(X).cuda(),
                               sc.case_paths(case), out, **kw)
    return out


def _check(got, want):
    got = got.numpy()
    assert np.isfinite(got).all()
    diff = np.abs(got - want).max()
    print(f"max |gpu - cpu| = {diff!r} (bound {sc.SHAP_GPU_TOL!r})")
    assert diff <= sc.SHAP_GPU_TOL


@pytest.mark.parametrize("case", sc.CASES + [sc.WIDE], ids=repr)
def test_kernel_vs_cpu(case):
    assert len(case.X) == 300
    got = _gpu_contribs(case)
    _check(got, _cpu_contribs(case))
    # bitwise repeatable, and the same with the output kept on the device
    assert torch.equal(got, _gpu_contribs(case))
    assert torch.equal(got, _gpu_contribs(case, device_out=True))


def test_kernel_accumulates_into_out():
    case = sc.CASES[0]
    out = torch.full((300, 1, case.F + 1), 1.5, dtype=torch.float64)
    ops.tree_shap(torch.from_numpy(case.X).cuda(), sc.case_paths(case), 1,
                  out)
    _check(out - 1.5, _cpu_contribs(case))
    assert (out[:, :, case.F] == 1.5).all()  # bias column untouched


def test_forest_spanning_several_lds_tiles():
    tile = ops.gpu.shap_tile_elems()
    trees, n_elems, seed = [], 0, 100
    while n_elems <= 2 * tile:  # at least three tiles
        trees += sc.random_forest(seed, 9, 6, 4, p_leaf=0.1)
        seed += 1
        n_elems = len(cpu.shap_paths(trees)["feature"])
    case = sc.Case("tiles", trees, 9, groups=[i % 3 for i in range(len(trees))],
                   brute=False)
    paths = sc.case_paths(case)
    assert len(paths["feature"]) > 2 * tile
    got = _gpu_contribs(case, paths)
    _check(got, _cpu_contribs(case, paths))
    assert torch.equal(got, _gpu_contribs(case, paths))


@pytest.mark.parametrize("case", [sc.CASES[0], sc.CASES[5]], ids=repr)
def test_chunked_copy_out_with_one_row_tail(case):
    # 300 rows = 13 chunks of 23 + a tail of one row
    row_bytes = 8 * case.n_groups * (case.F + 1)
    got = _gpu_contribs(case, max_out_bytes=23 * row_bytes)
    assert torch.equal(got, _gpu_contribs(case))
    _check(got, _cpu_contribs(case))


@pytest.mark.parametrize("case", SINGLE, ids=repr)
def test_interactions_kernel_vs_cpu(case):
    got = _gpu_inter(case)
    _check(got, _cpu_inter(case))
    assert torch.equal(got, _gpu_inter(case))
    row_bytes = 8 * (case.F + 1) ** 2
    assert torch.equal(got, _gpu_inter(case, max_out_bytes=23 * row_bytes))


def test_interactions_wide_forest():
    _check(_gpu_inter(sc.WIDE), _cpu_inter(sc.WIDE))


# -- Booster routing ----------------------------------------------------------

def _boom(*a, **k):
    raise AssertionError("must not be reached")


def _big_rows(F, n=booster_mod.SHAP_GPU_MIN_ROWS):
    return np.ascontiguousarray(
        np.resize(sc.rows(F, n=997, seed=3), (n, F)))


def _small_model(n_groups=1):
    """Two depth-2 trees per group on F = 3."""
    trees = sc.random_forest(31, 3, 2, 2 * n_groups, p_leaf=0.0)
    groups = [i % n_groups for i in range(len(trees))]
    case = sc.Case("route", trees, 3, groups=groups)
    return case, sc.case_booster(case)


def test_small_batches_stay_on_the_cpu(monkeypatch):
    case, bst = _small_model()
    X = case.X
    before = bst.predict(X[:8], pred_contribs=True)
    before_i = bst.predict(X[:8], pred_interactions=True)
    monkeypatch.setattr(ops, "tree_shap", _boom)
    monkeypatch.setattr(ops, "tree_shap_interactions", _boom)
    assert np.array_equal(bst.predict(X[:8], pred_contribs=True), before)
    assert np.array_equal(bst.predict(X[:8], pred_interactions=True),
                          before_i)


@pytest.mark.parametrize("n_groups", [1, 3])
def test_large_batches_run_the_kernel(monkeypatch, n_groups):
    case, bst = _small_model(n_groups)
    F = case.F
    X = _big_rows(F)
    assert len(X) == 16384
    margin = bst.predict(X, output_margin=True)
    monkeypatch.setattr(booster_mod, "_tree_shap", _boom)
    got = bst.predict(X, pred_contribs=True)
    assert got.dtype == np.float64
    assert got.shape == ((len(X), F + 1) if n_groups == 1
                         else (len(X), n_groups, F + 1))
    # the margin is float32 kernel output: a few float32 ulp of |m| <= 8
    assert np.abs(got.sum(-1) - margin).max() < 1e-5
    want = _cpu_contribs(case, X=X)
    assert np.abs(got.reshape(want.shape)[..., :F]
                  - want[..., :F]).max() <= sc.SHAP_GPU_TOL
    # the first rows agree with the recursion the small-batch path runs
    monkeypatch.undo()
    ref = bst.predict(X[:8], pred_contribs=True)
    assert np.abs(got[:8] - ref).max() <= sc.SHAP_GPU_TOL + sc.SHAP_D
    # cached path form is dropped with the rest of the derived state
    assert bst._shap_cache is not None
    assert bst.__getstate__()["_shap_cache"] is None
    monkeypatch.setattr(booster_mod, "_tree_shap", _boom)
    monkeypatch.setenv("RXGB_SHAP_GPU", "0")
    with pytest.raises(AssertionError):
        bst.predict(X, pred_contribs=True)


def test_large_batch_interactions_run_the_kernel(monkeypatch):
    case, bst = _small_model()
    F = case.F
    X = _big_rows(F)
    margin = bst.predict(X, output_margin=True)
    ref = bst.predict(X[:8], pred_interactions=True)
    monkeypatch.setattr(booster_mod, "_tree_shap", _boom)
    got = bst.predict(X, pred_interactions=True)
    assert got.dtype == np.float64 and got.shape == (len(X), F + 1, F + 1)
    assert np.abs(got.sum(axis=(1, 2)) - margin).max() < 1e-5
    assert np.abs(got - np.transpose(got, (0, 2, 1))).max() == 0
    # vs the recursion: the CPU bound plus the kernel's own
    assert np.abs(got[:8] - ref).max() <= (
        sc.inter_cpu_tol(F) + (F + 1) * sc.SHAP_GPU_TOL)
    monkeypatch.setenv("RXGB_SHAP_GPU", "0")
    with pytest.raises(AssertionError):
        bst.predict(X, pred_interactions=True)


def test_multiclass_interactions_still_unsupported():
    _, bst = _small_model(3)
    with pytest.raises(NotImplementedError):
        bst.predict(_big_rows(3), pred_interactions=True)


def test_iteration_range_and_parallel_trees_route(monkeypatch):
    """num_parallel_tree = 2 (scale 1/2) and a round slice, on the
    device, against the oracle built from the same slice."""
    trees = sc.random_forest(41, 3, 2, 4, p_leaf=0.0)
    case = sc.Case("npt", trees, 3, scale=0.5)
    bst = sc.case_booster(case)
    assert bst.num_boosted_rounds() == 2
    X = _big_rows(3)
    monkeypatch.setattr(booster_mod, "_tree_shap", _boom)
    got = bst.predict(X, pred_contribs=True, iteration_range=(1, 2))
    half = sc.Case("npt_half", trees[2:], 3, scale=0.5)
    want = _cpu_contribs(half, X=X)[:, 0]
    assert np.abs(got[:, :3] - want[:, :3]).max() <= sc.SHAP_GPU_TOL
    # and, bias column included, what the recursion gives for the slice
    # (it applies the 1/num_parallel_tree scale the same way)
    monkeypatch.undo()
    ref = bst.predict(X[:8], pred_contribs=True, iteration_range=(1, 2))
    assert np.abs(got[:8] - ref).max() <= sc.SHAP_GPU_TOL + sc.SHAP_D
    monkeypatch.setattr(booster_mod, "_tree_shap", _boom)
    # a different slice rebuilds the cached paths
    full = bst.predict(X, pred_contribs=True)
    want = _cpu_contribs(case, X=X)[:, 0]
    assert np.abs(full[:, :3] - want[:, :3]).max() <= sc.SHAP_GPU_TOL


def test_over_long_path_gives_the_cpu_result(monkeypatch):
    """A path of more than SHAP_MAX_PATH_LEN unique features is not the
    kernel's: the batch qualifies (threshold lowered here, so the
    recursion does not have to walk 16384 rows) and still takes the CPU
    code."""
    F = ops.SHAP_MAX_PATH_LEN + 1
    bst = booster_mod.Booster(
        {"objective": "reg:squarederror", "num_feature": F},
        [sc.chain_tree(F)], [0])
    X = sc.rows(F, n=24, seed=7)
    want = bst.predict(X, pred_contribs=True)
    monkeypatch.setattr(booster_mod, "SHAP_GPU_MIN_ROWS", 24)
    monkeypatch.setattr(ops, "tree_shap", _boom)
    assert np.array_equal(bst.predict(X, pred_contribs=True), want)
    # one feature fewer fits, and then the kernel is what runs
    monkeypatch.undo()
    monkeypatch.setattr(booster_mod, "SHAP_GPU_MIN_ROWS", 24)
    monkeypatch.setattr(booster_mod, "_tree_shap", _boom)
    case = sc.Case("chain32", [sc.chain_tree(F - 1)], F - 1, brute=False)
    Xc = sc.rows(F - 1, n=24, seed=7)
    got = sc.case_booster(case).predict(Xc, pred_contribs=True)
    want = _cpu_contribs(case, X=Xc)[:, 0]
    assert np.abs(got[:, :F - 1] - want[:, :F - 1]).max() <= sc.SHAP_GPU_TOL
