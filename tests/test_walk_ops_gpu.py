"""The HIP leaf-index and Saabas walk kernels against the references of
``walk_cases`` (exact, bitwise), and the Booster's routing of large
pred_leaf / approx_contribs batches to them."""

import numpy as np
import pytest
import torch

import shap_cases as sc
import walk_cases as wc
from xgboost_ray_amd import booster as booster_mod
from xgboost_ray_amd import ops
from xgboost_ray_amd.ops import gpu

pytestmark = pytest.mark.gpu

F_LDS = gpu.saabas_lds_max_features()
# a narrower block (34), the last width with LDS sums, the first without
WIDE = wc.wide_cases((34, F_LDS, F_LDS + 1))
ALL = list(wc.walk_cases()) + list(WIDE)
_id = lambda c: c["id"]  # noqa: E731


def _leaf(case, out=None, **kw):
    f = wc.torch_forest(case["forest"])
    if out is None:
        out = torch.full((case["n"], case["T"]), -7, dtype=torch.int32,
                         device="cuda")
    ops.predict_leaf(torch.from_numpy(case["X"]).cuda(), f["feat"], f["thr"],
                     f["left"], f["default_left"], f["tree_ptr"], out, **kw)
    return out


def _saabas(case, out=None, **kw):
    f = wc.torch_forest(case["forest"])
    if out is None:
        out = torch.from_numpy(case["out0"]).cuda()
    ops.saabas_contribs(torch.from_numpy(case["X"]).cuda(), f["feat"],
                        f["thr"], f["left"], f["default_left"],
                        torch.from_numpy(case["node_mean"]), f["tree_ptr"],
                        out, **kw)
    return out


@pytest.fixture(params=["lds", "plain"])
def variant(request, monkeypatch):
    """Node tiles in LDS (the default) or the plain global-node kernels.
    An over-tile forest takes the plain ones either way - the host decides
    from the same tiling ``aux_cases.lds_tiles`` reproduces."""
    if request.param == "plain":
        monkeypatch.setenv("RXGB_PREDICT_LDS", "0")
    else:
        monkeypatch.delenv("RXGB_PREDICT_LDS", raising=False)
    return request.param


@pytest.mark.parametrize("case", ALL, ids=_id)
def test_predict_leaf_kernel(case, variant):
    assert (case["tiles"] is None) == (case["forest_name"] == "overtile")
    got = _leaf(case)
    assert np.array_equal(got.cpu().numpy(), case["ref_leaves"])
    assert torch.equal(got, _leaf(case))  # two launches, equal bytes
    # a strided device out: the [n, T] view of a tree-major buffer
    scratch = torch.full((case["T"], case["n"]), -7, dtype=torch.int32,
                         device="cuda")
    _leaf(case, out=scratch.t())
    assert torch.equal(got, scratch.t())


@pytest.mark.parametrize("case", ALL, ids=_id)
def test_saabas_kernel_both_accumulator_routes(case, variant):
    want = case["ref_saabas"]
    fits = case["F"] <= F_LDS
    if variant == "lds" and case["tiles"] is not None and not fits:
        # beyond the LDS budget: global accumulation is what runs
        with pytest.raises(RuntimeError, match="do not fit"):
            _saabas(case, lds_accumulators=True)
    elif fits:
        got = _saabas(case, lds_accumulators=True)
        assert np.array_equal(got.cpu().numpy(), want)
    auto = _saabas(case)
    assert np.array_equal(auto.cpu().numpy(), want)
    assert torch.equal(auto, _saabas(case))  # two launches, equal bytes
    glob = _saabas(case, lds_accumulators=False)
    assert np.array_equal(glob.cpu().numpy(), want)


def test_geometry_constants_agree_with_the_extension():
    import aux_cases as ac

    ext = gpu._load()
    assert ext.SAABAS_LDS_BYTES == gpu.SAABAS_LDS_BYTES
    assert ext.PRED_TILE_NODES == ac.PRED_TILE_NODES
    assert gpu.SAABAS_TILE_NODES <= ext.PRED_TILE_NODES
    assert gpu.SAABAS_GLOBAL_GEOMETRY[1] <= ext.PRED_TILE_NODES


FULL_TILE = [c for c in wc.walk_cases()
             if c["forest_name"] in ("fulltile", "tileedges")]


@pytest.mark.parametrize("case", FULL_TILE, ids=_id)
def test_saabas_lds_nodes_with_full_4096_node_tiles(case, monkeypatch):
    """The default 1024-node tile sends these forests (trees of 4095 and
    4093 nodes) to the plain variant; with 4096-node tiles and a smaller
    block the LDS-node kernel stages exactly full tiles."""
    monkeypatch.delenv("RXGB_PREDICT_LDS", raising=False)
    assert case["tiles"] is not None and case["F"] <= 33
    for lds_acc in (True, False):
        got = _saabas(case, tile_nodes=4096, block_threads=128,
                      lds_accumulators=lds_acc)
        assert np.array_equal(got.cpu().numpy(), case["ref_saabas"])


@pytest.mark.parametrize("lds_acc", [None, False])
def test_saabas_into_a_strided_group_slice(lds_acc):
    case = wc.walk_cases()[1]
    n, F = case["n"], case["F"]
    full = torch.full((n, 3, F + 1), 0.125, dtype=torch.float64,
                      device="cuda")
    full[:, 1, :] = torch.from_numpy(case["out0"]).cuda()
    _saabas(case, out=full[:, 1, :], lds_accumulators=lds_acc)
    assert np.array_equal(full[:, 1, :].cpu().numpy(), case["ref_saabas"])
    # the other groups' cells are untouched
    assert (full[:, 0, :] == 0.125).all() and (full[:, 2, :] == 0.125).all()


@pytest.mark.parametrize("idx", [1, 5], ids=lambda i: _id(ALL[i]))
def test_host_out_in_23_row_chunks(idx):
    """Host ``out``, many chunks and a tail: the one-launch result."""
    case = ALL[idx]
    n, F, T = case["n"], case["F"], case["T"]
    assert n % 23 == 1 or n // 23 > 10
    out = torch.from_numpy(case["out0"].copy())
    _saabas(case, out=out, max_out_bytes=23 * 8 * (F + 1))
    assert torch.equal(out, _saabas(case).cpu())
    assert np.array_equal(out.numpy(), case["ref_saabas"])
    # a strided host slice, chunked
    full = torch.full((n, 3, F + 1), 0.125, dtype=torch.float64)
    full[:, 2, :] = torch.from_numpy(case["out0"])
    _saabas(case, out=full[:, 2, :], max_out_bytes=23 * 8 * (F + 1))
    assert np.array_equal(full[:, 2, :].numpy(), case["ref_saabas"])
    assert (full[:, :2, :] == 0.125).all()
    leaves = torch.full((n, T), -7, dtype=torch.int32)
    _leaf(case, out=leaves, max_out_bytes=23 * 4 * T)
    assert np.array_equal(leaves.numpy(), case["ref_leaves"])


def test_one_row_tail_chunk():
    case = WIDE[0]
    n, F = case["n"], case["F"]
    assert n % 23 == 1  # 300 rows = 13 chunks of 23 + a tail of one row
    out = torch.from_numpy(case["out0"].copy())
    _saabas(case, out=out, max_out_bytes=23 * 8 * (F + 1))
    assert np.array_equal(out.numpy(), case["ref_saabas"])
    leaves = torch.full((n, case["T"]), -7, dtype=torch.int32)
    _leaf(case, out=leaves, max_out_bytes=23 * 4 * case["T"])
    assert np.array_equal(leaves.numpy(), case["ref_leaves"])


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


class _Recorder:
    """Wraps an op and counts its calls."""

    def __init__(self, monkeypatch, name):
        self.calls, self.fn = 0, getattr(ops, name)
        monkeypatch.setattr(ops, name, self)

    def __call__(self, *a, **k):
        self.calls += 1
        return self.fn(*a, **k)


def _both(bst, X, **kw):
    return (bst.predict(X, pred_leaf=True, **kw),
            bst.predict(X, pred_contribs=True, approx_contribs=True, **kw))


def _numpy_unreachable(monkeypatch):
    monkeypatch.setattr(booster_mod.Booster, "_predict_leaf_numpy", _boom)
    monkeypatch.setattr(booster_mod.Booster, "_contribs_approx_numpy", _boom)


@pytest.mark.parametrize("n_groups", [1, 3])
def test_large_batches_run_the_kernels(monkeypatch, n_groups):
    case, bst = _small_model(n_groups)
    F = case.F
    X = _big_rows(F)
    assert len(X) == 16384
    monkeypatch.setenv("RXGB_WALK_GPU", "0")
    want_leaf, want_con = _both(bst, X)
    monkeypatch.delenv("RXGB_WALK_GPU")
    _numpy_unreachable(monkeypatch)
    leaf_op = _Recorder(monkeypatch, "predict_leaf")
    saabas_op = _Recorder(monkeypatch, "saabas_contribs")
    got_leaf, got_con = _both(bst, X)
    assert leaf_op.calls == 1 and saabas_op.calls == n_groups
    assert got_leaf.dtype == np.int32
    assert got_leaf.shape == (len(X), len(case.trees))
    assert got_con.dtype == np.float64
    assert got_con.shape == ((len(X), F + 1) if n_groups == 1
                             else (len(X), n_groups, F + 1))
    assert np.array_equal(got_leaf, want_leaf)
    assert np.array_equal(got_con, want_con)
    # the cached forest is dropped with the rest of the derived state
    assert bst._walk_cache is not None
    assert bst.__getstate__()["_walk_cache"] is None
    # with the switch off, the numpy walks are what runs
    monkeypatch.setenv("RXGB_WALK_GPU", "0")
    with pytest.raises(AssertionError):
        bst.predict(X, pred_leaf=True)
    with pytest.raises(AssertionError):
        bst.predict(X, pred_contribs=True, approx_contribs=True)


def test_iteration_range_and_parallel_trees_route(monkeypatch):
    trees = sc.random_forest(41, 3, 2, 4, p_leaf=0.0)
    case = sc.Case("npt", trees, 3, scale=0.5)
    bst = sc.case_booster(case)
    assert bst.num_boosted_rounds() == 2 and bst.num_parallel_tree == 2
    X = _big_rows(3)
    monkeypatch.setenv("RXGB_WALK_GPU", "0")
    want_part = _both(bst, X, iteration_range=(1, 2))
    want_full = _both(bst, X)
    monkeypatch.delenv("RXGB_WALK_GPU")
    _numpy_unreachable(monkeypatch)
    got = _both(bst, X, iteration_range=(1, 2))
    assert got[0].shape == (len(X), 2)
    assert all(np.array_equal(g, w) for g, w in zip(got, want_part))
    assert bst._walk_cache[0] == (1, 2)
    # a different slice rebuilds the cached forest
    got = _both(bst, X)
    assert got[0].shape == (len(X), 4)
    assert all(np.array_equal(g, w) for g, w in zip(got, want_full))
    assert bst._walk_cache[0] == (0, 2)


def test_load_model_drops_the_cached_forest(monkeypatch, tmp_path):
    """Another model of equal round count loaded into a Booster whose
    cache is warm: the device route walks the new forest."""
    _, bst = _small_model()
    other = sc.case_booster(sc.Case(
        "route2", sc.random_forest(77, 3, 2, 2, p_leaf=0.0), 3))
    assert other.num_boosted_rounds() == bst.num_boosted_rounds()
    X = _big_rows(3)
    old = _both(bst, X)
    assert bst._walk_cache is not None
    other.save_model(str(tmp_path / "other.json"))
    bst.load_model(str(tmp_path / "other.json"))
    assert bst._walk_cache is None
    monkeypatch.setenv("RXGB_WALK_GPU", "0")
    want = _both(bst, X)
    monkeypatch.delenv("RXGB_WALK_GPU")
    _numpy_unreachable(monkeypatch)
    got = _both(bst, X)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert not np.array_equal(got[1], old[1])


def test_small_batches_stay_on_the_cpu(monkeypatch):
    case, bst = _small_model()
    before = _both(bst, case.X[:8])
    monkeypatch.setattr(ops, "predict_leaf", _boom)
    monkeypatch.setattr(ops, "saabas_contribs", _boom)
    after = _both(bst, case.X[:8])
    assert all(np.array_equal(a, b) for a, b in zip(after, before))


def test_split_beyond_the_columns_behaves_as_before(monkeypatch):
    """A model that splits on feature 2 given two columns: the numpy walks
    raise IndexError on it, whatever the batch size, and still do."""
    _, bst = _small_model()
    assert max(int(t.feat.max()) for t in bst.trees) == 2
    X = _big_rows(3)[:, :2].copy()
    monkeypatch.setattr(ops, "predict_leaf", _boom)
    monkeypatch.setattr(ops, "saabas_contribs", _boom)
    for kw in ({"pred_leaf": True},
               {"pred_contribs": True, "approx_contribs": True}):
        with pytest.raises(IndexError):
            bst.predict(X[:8], **kw)
        with pytest.raises(IndexError):
            bst.predict(X, **kw)
