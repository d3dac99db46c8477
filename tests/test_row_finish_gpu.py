"""Row-order tree finish on the GPU: ``apply_tree_binned``, the quantize
pass's root sums, and the engine with ``RXGB_ROW_FINISH`` on against off.

Everything here is integer work or one f32 add per row of an identical
operand, so every comparison is exact (``assert_array_equal``); no
tolerance appears anywhere.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MISSING = 255


def _gpu_ops():
    from xgboost_ray_amd.ops import gpu as gpu_ops

    return gpu_ops


def _padded_dev(b):
    """Padded 16-byte-stride layout on the device, pad bytes 255 (the
    layout of ``_padded_dev`` in tests/test_ops_gpu_edges.py)."""
    n, F = b.shape
    full = torch.full((n, (F + 15) // 16 * 16), 255, dtype=torch.uint8,
                      device="cuda")
    full[:, :F] = b.cuda()
    return full[:, :F]


# ---------------------------------------------------------------------------
# trees
# ---------------------------------------------------------------------------
def _finish_tree(feat, left, rng, F):
    """Fill split bins (0 and 254 included), default directions (both ways)
    and leaf values for a (feat, left) skeleton; feat < 0 marks a leaf."""
    feat = np.asarray(feat, np.int32)
    left = np.asarray(left, np.int32)
    n = feat.size
    inner = feat >= 0
    feat = np.where(inner, rng.randint(0, F, n), -1).astype(np.int32)
    sbin = rng.choice(
        np.array([0, 254, 3, 17, 64, 100, 128, 200, 253]), n
    ).astype(np.int32)
    sbin[~inner] = 0
    dl = rng.randint(0, 2, n).astype(np.uint8)
    value = np.where(inner, 0.0, rng.randn(n)).astype(np.float32)
    return dict(feat=feat, split_bin=sbin, left=left, default_left=dl,
                value=value)


def _full_tree(depth, rng, F):
    n = 2 ** (depth + 1) - 1
    ids = np.arange(n)
    inner = ids < 2 ** depth - 1
    return _finish_tree(np.where(inner, 0, -1),
                        np.where(inner, 2 * ids + 1, -1), rng, F)


def _ragged_tree(rng, F):
    """A spine eight levels deep that drops one leaf per level: leaves at
    depths 1 to 8, the side the spine continues on alternating."""
    feat, left = [0], [1]
    spine = 0
    for d in range(1, 9):
        lo = len(feat)
        assert left[spine] == lo
        feat += [-1, -1]
        left += [-1, -1]
        if d < 8:
            spine = lo + (d % 2)
            feat[spine] = 0
            left[spine] = lo + 2
    return _finish_tree(feat, left, rng, F)


def _make_tree(kind, F):
    rng = np.random.RandomState(
        {"root": 1, "depth1": 2, "ragged": 3, "full8": 4, "over_lds": 5}[kind]
        + 100 * F
    )
    if kind == "root":
        return _finish_tree([-1], [-1], rng, F)
    if kind == "depth1":
        return _full_tree(1, rng, F)
    if kind == "ragged":
        return _ragged_tree(rng, F)
    if kind == "full8":
        t = _full_tree(8, rng, F)
        assert t["feat"].size == 511
        return t
    # 16383 nodes: over the 8192-node LDS cap, read from global memory
    return _full_tree(13, rng, F)


def _ref_apply(bins, tree, margin):
    """numpy level walk; ``margin`` float32, updated in place."""
    feat, sbin = tree["feat"], tree["split_bin"]
    left, dl = tree["left"], tree["default_left"]
    cur = np.zeros(bins.shape[0], np.int64)
    for _ in range(feat.size):
        rows = np.nonzero(feat[cur] >= 0)[0]
        if rows.size == 0:
            break
        node = cur[rows]
        b = bins[rows, feat[node]].astype(np.int64)
        go_left = np.where(b == MISSING, dl[node] != 0, b <= sbin[node])
        cur[rows] = left[node] + np.where(go_left, 0, 1)
    assert (feat[cur] < 0).all()
    margin += tree["value"][cur]
    return margin


ROWS = (1, 63, 64, 65, 2049, 100003)
FEATS = (1, 16, 17, 28, 33)
TREES = ("root", "depth1", "ragged", "full8", "over_lds")

_BINS = {}


def _bins(n, F):
    """Host bins with ~10 % missing cells, and their padded device copy;
    built once per shape and never written to."""
    key = (n, F)
    if key not in _BINS:
        rng = np.random.RandomState(7 + 31 * n + F)
        b = rng.randint(0, 255, size=(n, F)).astype(np.uint8)
        b[rng.rand(n, F) < 0.1] = MISSING
        _BINS[key] = (b, _padded_dev(torch.from_numpy(b)))
    return _BINS[key]


def _apply(bins_dev, margin_view, tree):
    _gpu_ops().apply_tree_binned(
        bins_dev, margin_view, tree["feat"], tree["split_bin"], tree["left"],
        tree["default_left"], tree["value"],
    )
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", TREES)
@pytest.mark.parametrize("F", FEATS)
@pytest.mark.parametrize("n", ROWS)
def test_apply_tree_binned_exact(n, F, kind):
    b, b_dev = _bins(n, F)
    assert b_dev.stride(0) == (F + 15) // 16 * 16
    tree = _make_tree(kind, F)
    m0 = np.random.RandomState(n + F).randn(n).astype(np.float32)
    ref = _ref_apply(b, tree, m0.copy())
    margin = torch.from_numpy(m0).cuda()
    _apply(b_dev, margin, tree)
    np.testing.assert_array_equal(margin.cpu().numpy(), ref)


@pytest.mark.parametrize("kind", TREES)
@pytest.mark.parametrize("F", FEATS)
@pytest.mark.parametrize("n", ROWS)
def test_apply_tree_binned_strided_margin(n, F, kind):
    """Column 1 of an [n, 3] margin updated in place; columns 0 and 2 stay."""
    b, b_dev = _bins(n, F)
    tree = _make_tree(kind, F)
    m0 = np.random.RandomState(3 * n + F).randn(n, 3).astype(np.float32)
    ref = m0.copy()
    ref[:, 1] = _ref_apply(b, tree, m0[:, 1].copy())
    margin = torch.from_numpy(m0).cuda()
    _apply(b_dev, margin[:, 1], tree)
    out = margin.cpu().numpy()
    np.testing.assert_array_equal(out[:, 0], m0[:, 0])
    np.testing.assert_array_equal(out[:, 2], m0[:, 2])
    np.testing.assert_array_equal(out, ref)


@pytest.mark.parametrize("kind", ("ragged", "full8", "over_lds"))
@pytest.mark.parametrize("layout", ("dense28", "padded70"))
def test_apply_tree_binned_other_strides(layout, kind):
    """Strides the whole-row register form does not take: a dense 28-byte
    row (no multiple of 16) and an 80-byte row (over 64)."""
    F = 28 if layout == "dense28" else 70
    n = 2049
    b, b_pad = _bins(n, F)
    b_dev = torch.from_numpy(b).cuda() if layout == "dense28" else b_pad
    assert b_dev.stride(0) == (28 if layout == "dense28" else 80)
    tree = _make_tree(kind, F)
    m0 = np.random.RandomState(F).randn(n).astype(np.float32)
    ref = _ref_apply(b, tree, m0.copy())
    margin = torch.from_numpy(m0).cuda()
    _apply(b_dev, margin, tree)
    np.testing.assert_array_equal(margin.cpu().numpy(), ref)


def test_apply_tree_binned_rejects_malformed_tree():
    b, b_dev = _bins(64, 16)
    margin = torch.zeros(64, device="cuda")
    tree = _make_tree("depth1", 16)
    bad = dict(tree, left=np.array([2, -1, -1], np.int32))  # right child = 3
    with pytest.raises(RuntimeError, match="malformed node"):
        _apply(b_dev, margin, bad)
    bad = dict(tree, feat=np.array([16, -1, -1], np.int32))  # feature >= F
    with pytest.raises(RuntimeError, match="malformed node"):
        _apply(b_dev, margin, bad)


# ---------------------------------------------------------------------------
# quantize sums
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ("mixed", "all_max"))
@pytest.mark.parametrize("n", (1, 255, 256, 257, 2 ** 20 + 3))
def test_quantize_gpair_sums_exact(n, case):
    if case == "mixed":
        rng = np.random.RandomState(n % 1000)
        gp = rng.randn(n, 2).astype(np.float32)
        gp[:, 1] = np.abs(gp[:, 1])
        sg, sh = 2.0 ** 28, 2.0 ** 27
    else:
        # every row quantizes to +2^30: the sums leave int32 at n = 2
        gp = np.ones((n, 2), np.float32)
        sg = sh = 2.0 ** 30
    g = torch.from_numpy(gp).cuda()
    gq, sums = _gpu_ops().quantize_gpair(g, sg, sh, return_sums=True)
    plain = _gpu_ops().quantize_gpair(g, sg, sh)
    assert sums.dtype == torch.int64 and tuple(sums.shape) == (2,)
    np.testing.assert_array_equal(gq.cpu().numpy(), plain.cpu().numpy())
    np.testing.assert_array_equal(
        sums.cpu().numpy(), gq.sum(0, dtype=torch.int64).cpu().numpy())
    if case == "all_max":
        assert int(sums[0]) == n * 2 ** 30
    elif n > 1:
        assert (gq[:, 0] < 0).any() and (gq[:, 0] > 0).any()


# ---------------------------------------------------------------------------
# engine: RXGB_ROW_FINISH=1 against =0 in one process
# ---------------------------------------------------------------------------
TREE_FIELDS = ("feat", "thr", "left", "default_left", "value", "gain",
               "cover", "parent")


def _binary_data(n, F, nan_frac=0.0, seed=0):
    rng = np.random.RandomState(seed)
    X = rng.randn(n, F).astype(np.float32)
    y = ((X[:, 0] + 0.5 * X[:, 1 % F] + 0.3 * rng.randn(n)) > 0)
    if nan_frac:
        X[rng.rand(n, F) < nan_frac] = np.nan
    return X, y.astype(np.float32)


def _multi_data(n, F, seed=0):
    rng = np.random.RandomState(seed)
    X = rng.randn(n, F).astype(np.float32)
    s = X[:, 0] + 0.5 * X[:, 1] + 0.3 * rng.randn(n)
    y = np.digitize(s, [-0.5, 0.5]).astype(np.float32)
    return X, y


ENGINE_CASES = {
    "d8": (lambda: _binary_data(20000, 28),
           {"objective": "binary:logistic", "max_depth": 8}),
    "nan_d3": (lambda: _binary_data(5000, 40, nan_frac=0.1, seed=1),
               {"objective": "binary:logistic", "max_depth": 3}),
    "d1": (lambda: _binary_data(5000, 28, seed=2),
           {"objective": "binary:logistic", "max_depth": 1}),
    "early_leaves": (lambda: _binary_data(20000, 28, seed=3),
                     {"objective": "binary:logistic", "max_depth": 8,
                      "min_child_weight": 100.0}),
    "subsample": (lambda: _binary_data(20000, 28, seed=4),
                  {"objective": "binary:logistic", "max_depth": 6,
                   "subsample": 0.5, "seed": 11}),
    "softprob": (lambda: _multi_data(20000, 28, seed=5),
                 {"objective": "multi:softprob", "num_class": 3,
                  "max_depth": 6}),
}


def _run_engine(dm, params, rounds):
    from xgboost_ray_amd.engine.trainer import BoostingEngine

    eng = BoostingEngine(dict(params, tree_method="gpu_hist", eta=0.3), dm)
    trees = []
    for _ in range(rounds):
        trees += eng.update()
    torch.cuda.synchronize()
    return trees, eng.margin.cpu().numpy()


@pytest.mark.parametrize("case", sorted(ENGINE_CASES))
def test_engine_row_finish_matches_legacy(case, monkeypatch):
    from xgboost_ray_amd.engine.quantile import BinnedMatrix

    make, params = ENGINE_CASES[case]
    X, y = make()
    dm = BinnedMatrix.build(
        torch.from_numpy(X).cuda(), label=torch.from_numpy(y).cuda(),
        max_bin=256,
    )
    monkeypatch.setenv("RXGB_ROW_FINISH", "0")
    trees_off, margin_off = _run_engine(dm, params, 5)
    monkeypatch.setenv("RXGB_ROW_FINISH", "1")
    trees_on, margin_on = _run_engine(dm, params, 5)
    assert len(trees_on) == len(trees_off) == 5 * params.get("num_class", 1)
    for t_on, t_off in zip(trees_on, trees_off):
        for f in TREE_FIELDS:
            np.testing.assert_array_equal(
                getattr(t_on, f), getattr(t_off, f), err_msg=f)
    np.testing.assert_array_equal(margin_on, margin_off)
    if case == "early_leaves":
        # fewer nodes than a full depth-8 tree: leaves above the last level
        assert any(1 < t.feat.size < 511 for t in trees_on)
    if case == "d8":
        assert max(t.feat.size for t in trees_on) > 255
