"""Every device training path against the independent reference grower.

Each case of ``tests/tree_cases.py`` runs through ``BoostingEngine`` on the
device under every path of the table below, and is compared with the CPU
oracle of ``tests/tree_oracle.py``: trees in canonical form, margins and
``pred_leaf`` membership, all exact. The oracle result is computed once per
case (from the draws the first run recorded) and reused across the paths;
every later run must have drawn the same samples. ``last_tree_path`` is
asserted for every row, so a silent fallback cannot pass.
"""

import numpy as np
import pytest
import torch

from tests import tree_cases as tc

pytestmark = pytest.mark.gpu

# path: (switches, F)
PATHS = {
    # F = 28: row stride 32, two 16-feature blocks
    "enqueue": ({}, 28),
    "per-depth-fused-glue": ({"RXGB_TREE_ENQUEUE": "0"}, 28),
    "separate-glue": ({"RXGB_TREE_ENQUEUE": "0", "RXGB_FUSED_GLUE": "0"}, 28),
    "two-sync-partition": ({"RXGB_ONE_SYNC": "0"}, 28),
    "legacy-finish": ({"RXGB_ROW_FINISH": "0"}, 28),
    "depth-step": ({"RXGB_DEPTH_STEP": "1"}, 28),
    # one 16-feature block: no XCD histogram route, so no enqueue
    "single-block-histogram": ({}, 12),
    # row stride 80 > 64: legacy finish by default, parity buffers
    "wide-rows": ({}, 70),
    "hist-multifb": ({"RXGB_HIST_MODE": "multifb"}, 28),
    "hist-base": ({"RXGB_HIST_MODE": "base"}, 28),
}

_ORACLES = {}


def _check(case, env, monkeypatch):
    for k in tc.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    run = tc.run_engine(case, "cuda")
    key = (case.name, case.F)
    if key not in _ORACLES:
        _, host = tc.matrix(case, "cuda")
        _ORACLES[key] = tc.run_oracle(case, host, run.draws, run.margins[0])
    oracle = _ORACLES[key]
    tc.same_draws(run.draws, oracle.draws)
    tc.compare(run, oracle)
    return run, oracle


@pytest.mark.parametrize("name", tc.DEPTHWISE)
@pytest.mark.parametrize("path", list(PATHS))
def test_gpu_path_matches_oracle(path, name, monkeypatch):
    env, F = PATHS[path]
    case = tc.case_at(name, F)
    run, oracle = _check(case, env, monkeypatch)
    want = "enqueue" if path == "enqueue" and case.enqueue_ok else "per_depth"
    assert run.paths == {want}
    if path == "wide-rows":
        dm, _ = tc.matrix(case, "cuda")
        assert dm.bins.stride(0) == 80
    if name == "deep":
        assert all(max(tc.level_widths(t)) >= 512 for t in oracle.trees)
    if name in ("tiny-n3", "tiny-n1", "zero-g", "zero-h", "zero-gh"):
        assert {tc.n_leaves(t) for t in oracle.trees} == {1}
    if name in ("zero-g", "zero-gh"):
        assert all(not t.value.any() for t in run.trees)
    if name == "tiny-n64-d8":
        # the frontier empties early: under the whole-tree enqueue the
        # deeper launches are no-ops
        assert max(tc.depth_of(t) for t in oracle.trees) < 8


@pytest.mark.parametrize("F", [28, 70])
@pytest.mark.parametrize("name", tc.LOSSGUIDE)
def test_gpu_lossguide_matches_oracle(name, F, monkeypatch):
    run, _ = _check(tc.case_at(name, F), {}, monkeypatch)
    assert run.paths == {"lossguide"}


def test_weighted_squarederror_takes_the_fused_gradient(monkeypatch):
    """The built-in route of the weighted-squarederror case really runs
    grad_fused with its fused abs-max (and so quantize_gpair_sums)."""
    from xgboost_ray_amd import ops

    for k in tc.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    case = tc.case_at("weighted-squarederror")
    dm, _ = tc.matrix(case, "cuda")
    margin = torch.full((case.n,), 0.5, dtype=torch.float32, device="cuda")
    out = ops.grad_fused(margin, dm.label, dm.weight, 1.0, mode=0)
    assert out is not None
    gp, mx = out
    d = tc.data(case.n, case.F)
    g = (np.float32(0.5) - d["y_reg"]) * d["w"]
    np.testing.assert_array_equal(gp.cpu().numpy(),
                                  np.stack([g, d["w"]], axis=1))
    np.testing.assert_array_equal(
        mx.cpu().numpy(), np.array([np.abs(g).max(), d["w"].max()]))
