"""HIP kernels outside the tree loop against independent float64 references.

``grad_fused``, ``eval_logloss``, ``eval_auc_hist``, ``lambdarank_grad`` and
``predict_trees`` (node packing, the LDS-tiled walk and the plain walk) run
on the cases of ``tests/aux_cases.py``. The tree walk, the AUC histogram and
the gradient maxima are compared bitwise or exactly; the float results within
bounds that come from the references and the number formats, never from the
kernels' output (docs/parity.md, "What the auxiliary-kernel tests pin down").
``tests/test_aux_oracles.py`` checks the CPU paths and the references
themselves.
"""

import math

import numpy as np
import pytest
import torch

from tests import aux_cases as ac

pytestmark = pytest.mark.gpu

# The float32 torch composition on the CPU lies within GRAD_CPU_UNITS of the
# float64 reference (measured on the CPU, see tests/aux_cases.py). The kernel
# runs the same float32 operation sequence, but the device's expf and
# division may each differ from the host's by an ulp: it gets twice that.
GRAD_GPU_FACTOR = 2.0
GRAD_GPU_UNITS = {m: GRAD_GPU_FACTOR * u
                  for m, u in ac.GRAD_CPU_UNITS.items()}

# two u32 planes in 160 KiB of dynamic LDS
AUC_MAX_BINS = 160 * 1024 // 8


def _gpu_ops():
    from xgboost_ray_amd.ops import gpu as gpu_ops

    return gpu_ops


def _d(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _ids(cases):
    return [c["id"] for c in cases]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---------------------------------------------------------------------------
# predict
# ---------------------------------------------------------------------------
def _run_predict(c, out):
    f = c["forest"]
    _gpu_ops().predict_trees(
        _d(c["X"]), _d(f["feat"]), _d(f["thr"]), _d(f["left"]),
        _d(f["default_left"]), _d(f["value"]), _d(f["tree_ptr"]), out,
        c["w"])
    torch.cuda.synchronize()
    return out


def _set_lds(monkeypatch, lds):
    if lds is None:
        monkeypatch.delenv("RXGB_PREDICT_LDS", raising=False)
    else:
        monkeypatch.setenv("RXGB_PREDICT_LDS", lds)


@pytest.mark.parametrize("lds", [None, "0"], ids=["lds", "plain"])
@pytest.mark.parametrize("c", ac.predict_cases(), ids=_ids(ac.predict_cases()))
def test_predict_bitwise(c, lds, monkeypatch):
    _set_lds(monkeypatch, lds)
    out = _run_predict(c, _d(c["out0"]))
    np.testing.assert_array_equal(_bits(out.cpu().numpy()),
                                  _bits(c["ref_dev"]))


@pytest.mark.parametrize("kind", ["lds", "plain"])
def test_predict_past_the_grid_cap(kind, monkeypatch):
    _set_lds(monkeypatch, None if kind == "lds" else "0")
    c = ac.predict_gridcap_case(kind)
    out = _run_predict(c, _d(c["out0"]))
    np.testing.assert_array_equal(_bits(out.cpu().numpy()),
                                  _bits(c["ref_dev"]))


def test_predict_into_a_strided_column(monkeypatch):
    _set_lds(monkeypatch, None)
    c = next(x for x in ac.predict_cases()
             if x["forest_name"] == "tileedges" and x["n"] == 2049)
    buf = torch.full((c["n"], 3), 7.0, dtype=torch.float32, device="cuda")
    buf[:, 1] = _d(c["out0"])
    col = buf[:, 1]
    assert not col.is_contiguous()
    _run_predict(c, col)
    got = buf.cpu().numpy()
    np.testing.assert_array_equal(_bits(got[:, 1]), _bits(c["ref_dev"]))
    assert (got[:, 0] == 7.0).all() and (got[:, 2] == 7.0).all()


# ---------------------------------------------------------------------------
# AUC histogram
# ---------------------------------------------------------------------------
def _check_auc(c):
    hist = _gpu_ops().eval_auc_hist(_d(c["margin"]), _d(c["label"]), c["B"])
    got = hist.cpu().numpy()
    assert got.dtype == np.int64 and got.shape == (2 * c["B"],)
    np.testing.assert_array_equal(got, c["ref"])
    assert int(got.sum()) == c["n"]


@pytest.mark.parametrize("c", ac.auc_cases(), ids=_ids(ac.auc_cases()))
def test_auc_hist_exact(c):
    _check_auc(c)


def test_auc_hist_past_the_grid_cap():
    _check_auc(ac.auc_big_case())


_AUC_METRIC = tuple(c for c in ac.auc_cases() if c["B"] == 16384)


@pytest.mark.parametrize("c", _AUC_METRIC, ids=_ids(_AUC_METRIC))
def test_auc_metric_planes(c, monkeypatch):
    from xgboost_ray_amd.engine.metrics import AUC

    monkeypatch.delenv("RXGB_FUSED_EVAL", raising=False)
    got = AUC().local_stats(_d(c["margin"]), _d(c["label"]), None, None,
                            None).cpu().numpy()
    B = c["B"]
    want = np.concatenate([c["ref"][B:], c["ref"][:B]])   # [pos | neg]
    np.testing.assert_array_equal(got, want.astype(np.float64))


def test_auc_hist_rejects_bins_beyond_lds():
    c = ac.auc_cases()[1]
    m, y = _d(c["margin"]), _d(c["label"])
    # the largest legal size still works ...
    hist = _gpu_ops().eval_auc_hist(m, y, AUC_MAX_BINS).cpu().numpy()
    np.testing.assert_array_equal(
        hist, ac.ref_auc_hist(c["margin"], c["label"], AUC_MAX_BINS))
    # ... one more raises before anything is launched
    for bad in (AUC_MAX_BINS + 1, 1 << 20, 0):
        with pytest.raises(RuntimeError, match="n_bins"):
            _gpu_ops().eval_auc_hist(m, y, bad)


# ---------------------------------------------------------------------------
# grad_fused
# ---------------------------------------------------------------------------
def _check_grad(c):
    gp, absmax = _gpu_ops().grad_fused(
        _d(c["margin"]), _d(c["label"]), _d(c["weight"]), c["spw"], c["mode"])
    torch.cuda.synchronize()
    assert gp.shape == (c["n"], 2) and absmax.shape == (2,)
    own = gp.abs().amax(0).cpu().numpy()
    am = absmax.cpu().numpy()
    got = gp.cpu().numpy()
    del gp
    ref = ac.ref_grad(c["margin"], c["label"], c["weight"], c["spw"],
                      c["mode"])
    unit = ac.grad_unit(c["label"], c["weight"], c["spw"], c["mode"])
    units = ac.grad_error_units(got, ref, unit)
    print(c["id"], "units of 2^-24:", units, "absmax", am)
    assert units <= GRAD_GPU_UNITS[c["mode"]]
    nan = np.isnan(ref).any(0)
    # the maxima equal abs().max() of the kernel's own output, +-inf included,
    # and are NaN when a gradient is NaN
    np.testing.assert_array_equal(np.isnan(am), nan)
    np.testing.assert_array_equal(np.isnan(own), nan)
    np.testing.assert_array_equal(_bits(am[~nan]), _bits(own[~nan]))
    if c["mode"] == 0 and c["kind"] != "nan":
        np.testing.assert_array_equal(
            _bits(got), _bits(ac.grad_f32_mode0(c["margin"], c["label"],
                                                c["weight"])))
    return am


@pytest.mark.parametrize("c", ac.grad_cases(), ids=_ids(ac.grad_cases()))
def test_grad_fused_matches_reference(c):
    am = _check_grad(c)
    if c["kind"] == "zero":
        assert am[0] == 0.0 and am[1] == 1.0
    if c["kind"] == "grid" and c["n"] > 1 and c["mode"] == 0:
        assert np.isinf(am[0])     # |+-inf - y| reaches the maximum


@pytest.mark.parametrize("c", ac.grad_nan_cases(),
                         ids=_ids(ac.grad_nan_cases()))
def test_grad_fused_nan_margin(c):
    am = _check_grad(c)
    assert math.isnan(am[0])
    assert math.isnan(am[1]) == (c["mode"] == 1)


def test_grad_fused_past_the_grid_cap():
    _check_grad(ac.grad_big_case())


def test_grad_fused_through_the_objectives():
    # the objective classes hand the kernel's maxima on to the quantiser
    from xgboost_ray_amd.engine.objectives import Logistic, SquaredError

    for c in (x for x in ac.grad_cases()
              if x["id"] in ("n4097-m1-spw3-w", "n4097-m0-spw1-nw")):
        obj = Logistic(c["spw"]) if c["mode"] == 1 else SquaredError()
        gp = obj.gradients(_d(c["margin"]), _d(c["label"]), _d(c["weight"]))
        ref = ac.ref_grad(c["margin"], c["label"], c["weight"], c["spw"],
                          c["mode"])
        unit = ac.grad_unit(c["label"], c["weight"], c["spw"], c["mode"])
        assert ac.grad_error_units(gp.cpu().numpy(), ref, unit) \
            <= GRAD_GPU_UNITS[c["mode"]]
        np.testing.assert_array_equal(
            _bits(gp._rxgb_absmax.cpu().numpy()),
            _bits(gp.abs().amax(0).cpu().numpy()))


# ---------------------------------------------------------------------------
# logloss
# ---------------------------------------------------------------------------
def _gpu_logloss(c):
    got = _gpu_ops().eval_logloss(_d(c["margin"]), _d(c["label"]),
                                  _d(c["weight"]))
    assert got.dtype == torch.float64 and got.shape == (2,)
    return got.cpu().numpy()


@pytest.mark.parametrize("c", ac.logloss_cases(), ids=_ids(ac.logloss_cases()))
def test_logloss_within_reference_bound(c):
    got = _gpu_logloss(c)
    stats, bound = c["ref"]
    print(c["id"], "err", np.abs(got - stats), "bound", bound)
    assert (np.abs(got - stats) <= bound).all()
    if c["wkind"] == "w0":
        assert got[0] == 0.0 and got[1] == 0.0   # compared, never finalized


def test_logloss_past_the_grid_cap():
    c = ac.logloss_big_case()
    got = _gpu_logloss(c)
    stats, bound, _ = ac.ref_logloss(c["margin"], c["label"], c["weight"])
    print(c["id"], "err", np.abs(got - stats), "bound", bound)
    assert (np.abs(got - stats) <= bound).all()
    assert got[1] == c["n"]


def test_logloss_nan_margin_gives_nan(monkeypatch):
    from xgboost_ray_amd.engine.metrics import LogLoss

    c = ac.logloss_nan_case()
    got = _gpu_logloss(c)
    assert math.isnan(got[0])
    wsum = math.fsum(c["weight"].astype(np.float64).tolist())
    assert abs(got[1] - wsum) <= 1e-12 * wsum
    monkeypatch.delenv("RXGB_FUSED_EVAL", raising=False)
    m = LogLoss()
    s = m.local_stats(_d(c["margin"]), _d(c["label"]), _d(c["weight"]), None,
                      None)
    assert math.isnan(m.finalize(s.cpu()))


# ---------------------------------------------------------------------------
# lambdarank
# ---------------------------------------------------------------------------
def _rank_bound(ref, S):
    """float32 store rounding of the result, plus float64 accumulation over
    L <= 1024 terms and an ulp or two of libm difference per term."""
    return 2.0 ** -23 * np.abs(ref) + 1e-12 * S


_RANK_CASES = ac.rank_cases() + (ac.rank_round0_case(),)


@pytest.mark.parametrize("ndcg", [False, True], ids=["pairwise", "ndcg"])
@pytest.mark.parametrize("c", _RANK_CASES, ids=_ids(_RANK_CASES))
def test_lambdarank_kernel_matches_reference(c, ndcg):
    rank, idcg = c["prep"]
    got = _gpu_ops().lambdarank_grad(
        _d(c["margin"]), _d(c["label"]), _d(c["group_ptr"]), _d(rank),
        _d(idcg), ndcg).cpu().numpy().astype(np.float64)
    ref, S = c["ref", ndcg]
    assert got.shape == ref.shape
    err = np.abs(got - ref)
    print(c["id"], "largest err:", err.max())
    assert (err <= _rank_bound(ref, S)).all()


@pytest.mark.parametrize("weighted", [False, True], ids=["nw", "w"])
@pytest.mark.parametrize("ndcg", [False, True], ids=["pairwise", "ndcg"])
@pytest.mark.parametrize("c", _RANK_CASES, ids=_ids(_RANK_CASES))
def test_lambdarank_objective_matches_reference(c, ndcg, weighted):
    from xgboost_ray_amd.engine.objectives import RankNDCG, RankPairwise

    obj = RankNDCG() if ndcg else RankPairwise()
    w = c["weight"] if weighted else None
    got = obj.gradients(_d(c["margin"]), _d(c["label"]), _d(w),
                        _d(c["qid"])).cpu().numpy().astype(np.float64)
    ref, S = c["ref", ndcg]
    bound = _rank_bound(ref, S)
    if weighted:    # one more float32 multiply, by an exact float32 weight
        w64 = w.astype(np.float64)[:, None]
        ref = ref * w64
        bound = bound * w64 + 2.0 ** -23 * np.abs(ref)
    assert (np.abs(got - ref) <= bound).all()
