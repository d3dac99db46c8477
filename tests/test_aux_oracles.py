"""The project's CPU gradient, metric, ranking and predict paths against the
independent float64 references of ``tests/aux_cases.py``.

No GPU needed. Integer and selection results (AUC histogram, tree walk) are
compared exactly or bitwise; float results within bounds that come from the
reference and the number formats (see "What the auxiliary-kernel tests pin
down" in docs/parity.md). ``tests/test_aux_ops_gpu.py`` runs the HIP kernels
against the same references.
"""

import math

import numpy as np
import pytest
import torch

from tests import aux_cases as ac


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _ids(cases):
    return [c["id"] for c in cases]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---------------------------------------------------------------------------
# references against slower, plainer versions of themselves
# ---------------------------------------------------------------------------
def _lambdarank_loop(m, y, rank, idcg, ndcg):
    """One group, pair by pair, math.fsum for every row sum."""
    L = len(m)
    out = np.zeros((L, 2))
    for i in range(L):
        gs, hs = [], []
        for j in range(L):
            if y[j] == y[i]:
                continue
            w = 1.0
            if ndcg:
                dg = (2.0 ** float(y[i]) - 1.0) - (2.0 ** float(y[j]) - 1.0)
                dd = (1.0 / math.log2(rank[i] + 2.0)
                      - 1.0 / math.log2(rank[j] + 2.0))
                w = abs(dg * dd) / idcg
            hi, lo = (i, j) if y[i] > y[j] else (j, i)
            d = float(np.float32(m[hi]) - np.float32(m[lo]))
            rho = 1.0 / (1.0 + math.exp(d))
            gs.append((-rho if hi == i else rho) * w)
            hs.append(max(rho * (1.0 - rho), 1e-16) * w)
        out[i] = math.fsum(gs), math.fsum(hs)
    return out


@pytest.mark.parametrize("ndcg", [False, True], ids=["pairwise", "ndcg"])
def test_ref_lambdarank_matches_pair_loop(ndcg):
    c = ac.rank_cases()[0]
    ref, S = c["ref", ndcg]
    rank, idcg = c["prep"]
    gp = c["group_ptr"]
    seen = 0
    for g, size in enumerate(c["sizes"]):
        if size > 65:
            continue
        s, e = int(gp[g]), int(gp[g + 1])
        if size < 2 or (ndcg and idcg[g] <= 0):
            want = np.zeros((size, 2))
        else:
            want = _lambdarank_loop(c["margin"][s:e], c["label"][s:e],
                                    rank[s:e], idcg[g], ndcg)
        np.testing.assert_allclose(ref[s:e], want, rtol=0,
                                   atol=1e-13 * max(S[s:e].max(), 1e-300))
        seen += 1
    assert seen >= 7
    # stable order: the all-tied group ranks in row order
    np.testing.assert_array_equal(rank[c["tied_group"]], np.arange(256))


def test_predict_vectorised_walk_matches_row_loop():
    # the generator asserts leaf-by-leaf agreement on the sampled rows;
    # here: the sample is real, bounded, and the per-row sums agree too
    for c in ac.predict_cases():
        assert 1 <= c["rows_checked"] <= 300
        f = c["forest"]
        T = len(f["tree_ptr"]) - 1
        for r in ac.sample_rows(c["n"])[:: max(1, c["rows_checked"] // 8)]:
            acc = np.float32(0.0)
            for t in range(T):
                leaf = ac._leaf_py(c["X"][r], f, t)
                acc = np.float32(acc + f["value"][leaf])
            scaled = np.float32(acc * np.float32(c["w"]))
            want = np.float32(c["out0"][r] + scaled)
            assert _bits(want) == _bits(c["ref_dev"][r]), (c["id"], r)


def test_auc_generator_keeps_rows_off_bin_edges():
    for c in ac.auc_cases():
        assert c["edge_ulps"] > ac.AUC_EDGE_ULPS, c["id"]
    m = (np.random.RandomState(7).randn(70_001) * 3.0).astype(np.float32)
    print("closest row to a bin edge, ulp:",
          ac.auc_edge_distance_ulps(m, 16384))


def test_logloss_generator_margin_bands():
    for c in ac.logloss_cases():
        a = np.abs(c["margin"].astype(np.float64))
        assert ((a <= 20.0) | (a >= 40.0)).all(), c["id"]
        if c["n"] > 1:
            assert np.isinf(c["margin"]).sum() == 2 and (a == 745.0).sum() == 2


# ---------------------------------------------------------------------------
# gradients
# ---------------------------------------------------------------------------
def _cpu_grad(c):
    from xgboost_ray_amd.engine.objectives import Logistic, SquaredError

    obj = Logistic(c["spw"]) if c["mode"] == 1 else SquaredError()
    return obj.gradients(_t(c["margin"]), _t(c["label"]),
                         _t(c["weight"])).numpy()


@pytest.mark.parametrize("c", ac.grad_cases() + ac.grad_nan_cases(),
                         ids=_ids(ac.grad_cases() + ac.grad_nan_cases()))
def test_cpu_gradients_match_reference(c):
    got = _cpu_grad(c)
    ref = ac.ref_grad(c["margin"], c["label"], c["weight"], c["spw"],
                      c["mode"])
    unit = ac.grad_unit(c["label"], c["weight"], c["spw"], c["mode"])
    units = ac.grad_error_units(got, ref, unit)
    print(c["id"], "units of 2^-24:", units)
    assert units <= ac.GRAD_CPU_UNITS[c["mode"]]
    if c["mode"] == 0 and c["kind"] != "nan":
        # IEEE subtract and multiply: no freedom at all
        np.testing.assert_array_equal(
            _bits(got), _bits(ac.grad_f32_mode0(c["margin"], c["label"],
                                                c["weight"])))


# ---------------------------------------------------------------------------
# logloss
# ---------------------------------------------------------------------------
def _cpu_logloss(c):
    from xgboost_ray_amd.engine.metrics import LogLoss

    return LogLoss().local_stats(_t(c["margin"]), _t(c["label"]),
                                 _t(c["weight"]), None, None).numpy()


@pytest.mark.parametrize("c", ac.logloss_cases(), ids=_ids(ac.logloss_cases()))
def test_cpu_logloss_stats_match_reference(c):
    got = _cpu_logloss(c)
    stats, bound = c["ref"]
    print(c["id"], "err", np.abs(got - stats), "bound", bound)
    assert (np.abs(got - stats) <= bound).all()
    if c["wkind"] == "w0":
        assert got[0] == 0.0 and got[1] == 0.0   # compared, never finalized


def test_cpu_logloss_nan_margin_gives_nan():
    c = ac.logloss_nan_case()
    got = _cpu_logloss(c)
    stats, _, _ = ac.ref_logloss(c["margin"], c["label"], c["weight"])
    assert math.isnan(stats[0]) and math.isnan(got[0])
    assert abs(got[1] - stats[1]) <= 1e-12 * stats[1]


# ---------------------------------------------------------------------------
# AUC histogram
# ---------------------------------------------------------------------------
_AUC_CPU = tuple(c for c in ac.auc_cases() if c["B"] == 16384)


@pytest.mark.parametrize("c", _AUC_CPU, ids=_ids(_AUC_CPU))
def test_cpu_auc_histogram_exact(c):
    from xgboost_ray_amd.engine.metrics import _AUC_BINS, AUC

    assert _AUC_BINS == c["B"]
    got = AUC().local_stats(_t(c["margin"]), _t(c["label"]), None, None,
                            None).numpy()
    B = c["B"]
    want = np.concatenate([c["ref"][B:], c["ref"][:B]])  # [pos | neg]
    np.testing.assert_array_equal(got, want.astype(np.float64))
    assert got.sum() == c["n"]


# ---------------------------------------------------------------------------
# lambdarank
# ---------------------------------------------------------------------------
def _cpu_rank(c, ndcg):
    from xgboost_ray_amd.engine.objectives import RankNDCG, RankPairwise

    obj = RankNDCG() if ndcg else RankPairwise()
    return obj.gradients(_t(c["margin"]), _t(c["label"]), None,
                         _t(c["qid"])).numpy().astype(np.float64)


def _rank_cpu_bound(c, S):
    """Pair terms exact to float32 rounding, then a float32 sum of at most L
    of them: L * 2^-24 * S_i, L the row's group length."""
    L = np.repeat(np.asarray(c["sizes"]), c["sizes"]).astype(np.float64)
    return L[:, None] * ac.U24 * S


@pytest.mark.parametrize("ndcg", [False, True], ids=["pairwise", "ndcg"])
@pytest.mark.parametrize("c", ac.rank_cases(), ids=_ids(ac.rank_cases()))
def test_cpu_lambdarank_matches_reference(c, ndcg):
    got = _cpu_rank(c, ndcg)
    ref, S = c["ref", ndcg]
    bound = _rank_cpu_bound(c, S)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        print(c["id"], "largest err/bound:",
              np.nanmax(np.where(bound > 0, err / bound, 0.0)),
              "largest err:", err.max())
    assert (err <= bound).all()
    if "tied_group" in c:
        g = c["tied_group"]            # all margins equal: the stable order
        assert np.abs(ref[g]).max() > 0
        assert (err[g] <= bound[g]).all()


@pytest.mark.parametrize("ndcg", [False, True], ids=["pairwise", "ndcg"])
def test_cpu_lambdarank_round0_all_ties(ndcg):
    # every margin equal, as in round 0 of every ranking run
    c = ac.rank_round0_case()
    got = _cpu_rank(c, ndcg)
    ref, S = c["ref", ndcg]
    assert np.abs(ref).max() > 0
    assert (np.abs(got - ref) <= _rank_cpu_bound(c, S)).all()


# ---------------------------------------------------------------------------
# predict
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", ac.predict_cases(), ids=_ids(ac.predict_cases()))
def test_cpu_predict_trees_bitwise(c):
    from xgboost_ray_amd.ops import cpu as cpu_ops

    f = c["forest"]
    out = _t(c["out0"].copy())
    cpu_ops.predict_trees(_t(c["X"]), _t(f["feat"]), _t(f["thr"]),
                          _t(f["left"]), _t(f["default_left"]),
                          _t(f["value"]), _t(f["tree_ptr"]), out, c["w"])
    np.testing.assert_array_equal(_bits(out.numpy()), _bits(c["ref_cpu"]))
