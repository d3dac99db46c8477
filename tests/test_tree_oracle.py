"""The CPU engine's trees against the independent reference grower.

The engine-level tests so far compared the trainer with itself (two switch
settings, or its CPU and GPU runs). Here every tree of every case in
``tests/tree_cases.py`` is held against ``tests/tree_oracle.py``, which
recomputes each node's histogram and sums from the node's own rows and knows
nothing of slot orders, subtraction or partition buffers. All comparisons
are ``array_equal`` or tuple-equal; no tolerance appears anywhere.

The sensitivity checks at the end inject five wrongs into the CPU path and
require the comparison to fail: the evidence that a wrong tree is noticed.
"""

import numpy as np
import pytest
import torch

from tests import op_cases as oc
from tests import tree_cases as tc
from tests import tree_oracle as to


def _ids(cases):
    return [c["id"] for c in cases]


# ---------------------------------------------------------------------------
# a. oracle self-checks
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", oc.split_cases(), ids=_ids(oc.split_cases()))
def test_vectorised_split_choice_equals_brute_force(c):
    want = to.brute_splits(c)
    hist = c["hist"].numpy()
    for k in range(c["K"]):
        got = to.best_split(
            hist[k], int(c["parent_g"][k]), int(c["parent_h"][k]),
            c["feat_bins"].numpy(), c["scale_g"], c["scale_h"],
            c["reg_lambda"], c["reg_alpha"], c["gamma"], c["mcw"],
            gate=None if c["allowed"] is None else c["allowed"][k].numpy() != 0,
            monotone=None if c["monotone"] is None else c["monotone"].numpy(),
            bounds=None if c["bounds"] is None
            else tuple(c["bounds"][k].tolist()))
        gain, f, b, dl, lg, lh = got
        assert np.float32(gain) == want["gain"][k], k
        assert (f, b, dl, lg, lh) == tuple(
            int(want[key][k]) for key in to.KEYS[1:]), k


def _check(case, device="cpu"):
    run = tc.run_engine(case, device)
    _, host = tc.matrix(case, device)
    oracle = tc.run_oracle(case, host, run.draws, run.margins[0])
    tc.compare(run, oracle)
    return run, oracle


def test_raw_threshold_walk_equals_binned_walk():
    """x < thr in float32 (NaN by the default direction) lands every row in
    the leaf of the binned walk, on a matrix with values exactly on cuts."""
    on_cut = 0
    for name in ("plain-b64", "plain-b256", "lossguide-leaves17"):
        case = tc.case_at(name)
        _, host = tc.matrix(case, "cpu")
        X = tc.data(case.n, case.F)["X"]
        for f in range(case.F):
            lo, hi = host["cut_ptr"][f], host["cut_ptr"][f + 1]
            on_cut += int(np.isin(X[:, f], host["cuts_flat"][lo:hi]).sum())
        # the trees come from the oracle alone: margin 0.5, no sampling
        P = tc.oracle_params(case)
        margin = np.full(case.n, 0.5, np.float32)
        y = tc.data(case.n, case.F)["y_bin"]
        used = set()
        for _ in range(tc.ROUNDS):
            g, h = tc.OBJECTIVES["logistic"][0](margin, y)
            root = to.grow_tree(
                host["bins"], host["feat_bins"], host["cuts_flat"],
                host["cut_ptr"], host["n_bins"], np.stack([g, h], axis=1),
                np.arange(case.n), P)
            np.testing.assert_array_equal(to.walk_raw(root, X),
                                          to.walk_binned(root, host["bins"]))
            used |= {nd.feat for nd in to.preorder(root) if nd.feat >= 0}
            to.add_margin(margin, root, host["bins"])
        # the integer column and a column with missing values do split
        assert {tc.COL_INT, tc.COL_NAN30} <= used
        assert tc.COL_DUP not in used and tc.COL_CONST not in used
    assert on_cut > 1000


# ---------------------------------------------------------------------------
# b. the CPU engine against the oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(tc.CASES))
def test_cpu_engine_matches_oracle(name):
    case = tc.case_at(name)
    run, oracle = _check(case)
    assert run.paths == {"lossguide" if tc.is_lossguide(case)
                         else "per_depth"}
    leaves = [tc.n_leaves(t) for t in oracle.trees]
    depths = [tc.depth_of(t) for t in oracle.trees]
    zero = to._bits(0.0)
    if name in ("tiny-n3", "tiny-n1", "zero-g", "zero-h", "zero-gh"):
        assert set(leaves) == {1}  # the root is a leaf
    if name in ("zero-g", "zero-gh"):
        # -0.0 is a zero too: compare the values, not the bits
        assert all(np.int32(t[1]).view(np.float32) == 0 for t in oracle.trees)
    elif name == "zero-h":
        # H = 0 leaves w = -G / lambda, which is not 0 unless G is
        assert all(t[1] != zero for t in oracle.trees)
    elif name == "tiny-n64-d8":
        assert max(depths) < 8 and min(leaves) > 1  # frontier empties early
    elif name == "deep":
        assert all(max(tc.level_widths(t)) >= 512 for t in oracle.trees)
        assert max(depths) == 11
    elif name == "lossguide-leaves17":
        assert set(leaves) == {17} and max(depths) > 4
    elif name == "lossguide-leaves9-d3":
        assert max(depths) == 3 and max(leaves) <= 9
    elif name == "lossguide-d4-gamma1":
        assert max(depths) == 4
    elif name not in ("tiny-n3", "tiny-n1"):
        assert min(leaves) > 8
    if name == "colsample":
        assert all(d["tree_gate"] is not None and d["level_gates"]
                   and d["node_gates"] for d in run.draws)
    if name.startswith("subsample") or name == "multiclass-forest":
        assert all(0 < len(d["rows"]) < case.n for d in run.draws)
    if name == "subsample-gradient":
        assert all(d["mvs_gpair"] is not None for d in run.draws)


@pytest.mark.parametrize("F", [12, 70])
@pytest.mark.parametrize("name", ["plain-b64", "constrained", "colsample"])
def test_cpu_engine_matches_oracle_other_widths(name, F):
    _check(tc.case_at(name, F))


def test_zero_gradient_column_quantises_to_zero():
    """max|g| == 0 must give a finite scale and q == 0 (it used to give
    2^30 / 1e-300 = inf and 0 * inf = NaN)."""
    from xgboost_ray_amd.engine.trainer import BoostingEngine

    case = tc.case_at("zero-g")
    dm, _ = tc.matrix(case, "cpu")
    eng = BoostingEngine({"max_depth": 2}, dm)
    for g, h in ((0.0, 1.0), (1.0, 0.0), (0.0, 0.0)):
        gp = torch.tensor([[g, h]] * case.n, dtype=torch.float32)
        gq, sg, sh = eng._quantize(gp)
        assert np.isfinite(sg) and np.isfinite(sh)
        assert gq[:, 0].tolist() == [int(g * 2**30)] * case.n
        assert gq[:, 1].tolist() == [int(h * 2**30)] * case.n
        q, osg, osh = to.quantize(gp.numpy())
        assert (osg, osh) == (sg, sh)
        np.testing.assert_array_equal(q, gq.numpy())


# ---------------------------------------------------------------------------
# c. sensitivity: each injected wrong must make (b) fail
# ---------------------------------------------------------------------------
def _must_fail(case):
    with pytest.raises(AssertionError):
        _check(case)


def test_sensitivity_missing_rows_routed_against_default(monkeypatch):
    from xgboost_ray_amd.ops import cpu as cpu_ops

    real = cpu_ops.partition_rows

    def wrong(bins, ridx, starts, counts, split_feat, split_bin,
              default_left, gpair_seg=None, bins_t=None):
        return real(bins, ridx, starts, counts, split_feat, split_bin,
                    1 - torch.as_tensor(default_left), gpair_seg, bins_t)

    case = tc.case_at("plain-b64")
    _check(case)
    monkeypatch.setattr(cpu_ops, "partition_rows", wrong)
    _must_fail(case)
    _must_fail(tc.case_at("lossguide-leaves17"))


def test_sensitivity_tie_order_reversed(monkeypatch):
    """default-left 0 wins on equal gain: the two passes tie exactly where
    the winning feature has no missing mass in the node."""
    from xgboost_ray_amd.ops import cpu as cpu_ops

    real = cpu_ops.find_splits

    def wrong(hist, parent_g, parent_h, *a, **kw):
        best = real(hist, parent_g, parent_h, *a, **kw)
        for k in np.nonzero(best["feature"] >= 0)[0]:
            tot = hist[k, int(best["feature"][k])].sum(0)
            if (int(tot[0]), int(tot[1])) == (int(parent_g[k]),
                                              int(parent_h[k])):
                best["default_left"][k] = 0
        return best

    case = tc.case_at("plain-b64")
    monkeypatch.setattr(cpu_ops, "find_splits", wrong)
    _must_fail(case)


def test_sensitivity_left_sums_off_by_one_quantum(monkeypatch):
    from xgboost_ray_amd.ops import cpu as cpu_ops

    real = cpu_ops.find_splits

    def wrong(*a, **kw):
        best = real(*a, **kw)
        best["left_g"] = best["left_g"] + (best["feature"] >= 0)
        return best

    monkeypatch.setattr(cpu_ops, "find_splits", wrong)
    _must_fail(tc.case_at("plain-b64"))
    _must_fail(tc.case_at("lossguide-leaves17"))


def test_sensitivity_threshold_from_previous_cut(monkeypatch):
    import dataclasses

    case = tc.case_at("plain-b64")
    dm, _ = tc.matrix(case, "cpu")  # the oracle keeps the true cuts
    shifted = dataclasses.replace(
        dm.cuts, cuts_flat=torch.roll(dm.cuts.cuts_flat, 1))
    monkeypatch.setattr(dm, "cuts", shifted)
    _must_fail(case)


def test_sensitivity_margin_advanced_on_sampled_rows_only(monkeypatch):
    from xgboost_ray_amd.engine.trainer import BoostingEngine

    real = BoostingEngine._add_tree_margin_raw

    def wrong(self, t, margin_view):
        full = torch.zeros_like(margin_view)
        real(self, t, full)
        rows = torch.from_numpy(self._rec.trees[-1]["rows"])
        margin_view[rows] += full[rows]

    case = tc.case_at("subsample-uniform")
    _check(case)
    monkeypatch.setattr(BoostingEngine, "_add_tree_margin_raw", wrong)
    _must_fail(case)
