"""reg:quantileerror on the GPU: the leaf_quantile_hist kernel against the
torch CPU oracle (exact), the full select against the sort oracle, and
training against the CPU engine and across world sizes."""

import os

import numpy as np
import pytest
import torch

from tests.quantile_oracle import (bits, key_of, make_case, segment_oracle)
from xgboost_ray_amd import ops
from xgboost_ray_amd.ops import cpu as cpu_ops

pytestmark = pytest.mark.gpu

OBJ = "reg:quantileerror"
ALPHA = 0.5


@pytest.fixture(scope="module", params=[False, True], ids=["unit", "W"])
def case(request):
    """Shared inputs: the CPU case plus a segment longer than two chunks
    and one of chunk+1 rows, split over both ping-pong buffers."""
    resid, W, ridx, starts, counts = make_case(request.param, big=True)
    L = len(starts)
    parity = (np.arange(L) % 2).astype(np.int64)
    # buffer b holds valid rows only for the segments that select it; the
    # rest of each buffer is row 0, so a wrong buffer choice changes sums
    bufs = [np.zeros_like(ridx), np.zeros_like(ridx)]
    for k in range(L):
        s, c = int(starts[k]), int(counts[k])
        bufs[parity[k]][s:s + c] = ridx[s:s + c]
    want = segment_oracle(resid, W, ridx, starts, counts, ALPHA)
    return resid, W, ridx, bufs, parity, starts, counts, want


@pytest.mark.parametrize("pass_idx", [0, 1, 2, 3])
def test_hist_gpu_equals_cpu(case, pass_idx):
    resid, W, ridx, bufs, parity, starts, counts, want = case
    L = len(starts)
    prefix = torch.tensor(
        [0 if q is None else key_of(q) >> (32 - 8 * pass_idx)
         if pass_idx else 0 for q in want], dtype=torch.int64)
    st, ct = torch.from_numpy(starts), torch.from_numpy(counts)
    Wt = None if W is None else torch.from_numpy(W)
    ref = torch.full((L, 256), 3, dtype=torch.int64)  # accumulated into
    cpu_ops.leaf_quantile_hist(
        torch.from_numpy(resid), Wt, torch.from_numpy(bufs[0]), st, ct,
        prefix, pass_idx, ref, ridx_b=torch.from_numpy(bufs[1]),
        parity=parity,
    )
    assert int(ref.sum()) > 3 * L * 256
    out = torch.full((L, 256), 3, dtype=torch.int64, device="cuda")
    ops.leaf_quantile_hist(
        torch.from_numpy(resid).cuda(), None if Wt is None else Wt.cuda(),
        torch.from_numpy(bufs[0]).cuda(), st, ct, prefix, pass_idx, out,
        ridx_b=torch.from_numpy(bufs[1]).cuda(), parity=parity,
    )
    assert torch.equal(out.cpu(), ref)
    # single-buffer form (no parity) over the plain index array
    ref1 = torch.zeros((L, 256), dtype=torch.int64)
    cpu_ops.leaf_quantile_hist(torch.from_numpy(resid), Wt,
                               torch.from_numpy(ridx), st, ct, prefix,
                               pass_idx, ref1)
    out1 = torch.zeros((L, 256), dtype=torch.int64, device="cuda")
    ops.leaf_quantile_hist(
        torch.from_numpy(resid).cuda(), None if Wt is None else Wt.cuda(),
        torch.from_numpy(ridx).cuda(), st, ct, prefix, pass_idx, out1)
    assert torch.equal(out1.cpu(), ref1)


@pytest.mark.parametrize("alpha", [0.05, 0.5, 0.95])
def test_full_select_gpu_matches_sort_oracle(case, alpha):
    resid, W, ridx, bufs, parity, starts, counts, _ = case
    want = segment_oracle(resid, W, ridx, starts, counts, alpha)
    q, W_seg = ops.leaf_quantile_select(
        torch.from_numpy(resid).cuda(),
        None if W is None else torch.from_numpy(W).cuda(),
        torch.from_numpy(bufs[0]).cuda(), starts, counts, alpha,
        ridx_b=torch.from_numpy(bufs[1]).cuda(), parity=parity,
    )
    for k, wq in enumerate(want):
        if wq is None:
            assert int(W_seg[k]) == 0
            continue
        assert bits(q[k]) == bits(wq), (k, q[k], wq)


def _train_data():
    rng = np.random.RandomState(7)
    n, F = 2000, 8
    X = rng.randn(n, F).astype(np.float32)
    X[rng.rand(n, F) < 0.05] = np.nan
    y = (np.nan_to_num(X[:, 0]) * 2 - np.nan_to_num(X[:, 1])
         + rng.randn(n)).astype(np.float32)
    w = (rng.rand(n) * 2).astype(np.float32)
    w[::23] = 0.0
    return X, y, w


@pytest.mark.parametrize("extra", [{}, {"grow_policy": "lossguide",
                                        "max_leaves": 12}],
                         ids=["depthwise", "lossguide"])
def test_training_gpu_equals_cpu(extra):
    from xgboost_ray_amd.engine.quantile import BinnedMatrix
    from xgboost_ray_amd.engine.trainer import run_training

    X, y, w = _train_data()
    params = dict({"objective": OBJ, "quantile_alpha": 0.9, "max_depth": 4,
                   "eta": 0.3}, **extra)
    models = {}
    for dev in ("cpu", "cuda"):
        dm = BinnedMatrix.build(
            torch.from_numpy(X).to(dev), label=torch.from_numpy(y).to(dev),
            weight=torch.from_numpy(w).to(dev), max_bin=256,
        )
        models[dev] = run_training(dict(params), dm, 5)
    a, b = models["cpu"], models["cuda"]
    assert a.base_score == b.base_score
    assert len(a.trees) == len(b.trees) == 5
    for ta, tb in zip(a.trees, b.trees):
        assert np.array_equal(ta.feat, tb.feat)
        assert np.array_equal(ta.left, tb.left)
        assert np.array_equal(bits(ta.thr), bits(tb.thr))
        assert np.array_equal(bits(ta.value), bits(tb.value))


def test_world2_on_one_gpu_equals_single():
    from xgboost_ray_amd import RayDMatrix, RayParams, train

    X, y, w = _train_data()
    params = {"objective": OBJ, "quantile_alpha": 0.9, "max_depth": 4,
              "eta": 0.3, "tree_method": "gpu_hist"}
    raws = []
    for actors, env in ((1, {}), (2, {"RXGB_COLL_BACKEND": "gloo"})):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            bst = train(
                dict(params), RayDMatrix(X, y, weight=w), num_boost_round=5,
                ray_params=RayParams(num_actors=actors, gpus_per_actor=1,
                                     max_actor_restarts=0),
            )
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        raws.append(bst.save_raw("json"))
    assert raws[0] == raws[1]
