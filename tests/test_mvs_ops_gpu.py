"""HIP kernels of gradient-based row sampling against the CPU ops.

Every kernel must be ``array_equal`` to ``ops.cpu`` on every case of
``tests/mvs_cases.py`` (integer arithmetic decides the sample; the
reweighting is one IEEE float64 divide and two multiplies), and two
launches must give identical bytes. ``tests/test_mvs_oracles.py`` checks
``ops.cpu`` itself against the brute force.
"""

import numpy as np
import pytest
import torch

from tests import mvs_cases as mc
from xgboost_ray_amd.ops import cpu

pytestmark = pytest.mark.gpu


def _gpu_ops():
    from xgboost_ray_amd.ops import gpu as gpu_ops

    return gpu_ops


def _t(a):
    return torch.from_numpy(np.array(a))


@pytest.mark.parametrize("case_id", mc.SCORE_IDS)
def test_score_matches_cpu(case_id):
    gpair, mx_g, mx_h = mc.score_case(case_id)
    want = cpu.mvs_score(_t(gpair), mx_g, mx_h).numpy()
    dev = _t(gpair).cuda()
    got = _gpu_ops().mvs_score(dev, mx_g, mx_h)
    assert got.dtype == torch.uint32 and got.is_cuda
    again = _gpu_ops().mvs_score(dev, mx_g, mx_h)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(again.cpu().numpy(), want)


def test_score_zero_maxima_matches_cpu():
    gpair = torch.zeros((130, 2), dtype=torch.float32)
    want = cpu.mvs_score(gpair, 0.0, 0.0).numpy()
    got = _gpu_ops().mvs_score(gpair.cuda(), 0.0, 0.0).cpu().numpy()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("case_id", mc.C_IDS)
def test_stats_and_hist_match_cpu(case_id):
    c = _t(mc.c_case(case_id)[0])
    dev = c.cuda()
    g = _gpu_ops()
    assert np.array_equal(g.mvs_stats(dev).cpu().numpy(),
                          cpu.mvs_stats(c).numpy())
    for prefix, p in mc.radix_path(case_id):
        want = cpu.mvs_hist(c, prefix, p).numpy()
        got = g.mvs_hist(dev, prefix, p)
        assert tuple(got.shape) == (256, 2) and got.dtype == torch.int64
        again = g.mvs_hist(dev, prefix, p)
        assert np.array_equal(got.cpu().numpy(), want), (prefix, p)
        assert np.array_equal(again.cpu().numpy(), want), (prefix, p)


@pytest.mark.parametrize("case_id", mc.C_IDS)
def test_threshold_matches_cpu(case_id):
    c, k, _, _ = mc.c_case(case_id)
    want = cpu.mvs_threshold(_t(c), k)
    got = _gpu_ops().mvs_threshold(_t(c).cuda(), k)
    assert tuple(int(v) for v in got) == tuple(int(v) for v in want)


@pytest.mark.parametrize("case_id", mc.C_IDS)
def test_sample_matches_cpu(case_id):
    c, k, gpair, key = mc.c_case(case_id)
    S, M = cpu.mvs_threshold(_t(c), k)
    want_keep, want_out = cpu.mvs_sample(_t(gpair), _t(c), S, M, key)
    gd, cd = _t(gpair).cuda(), _t(c).cuda()
    keep, out = _gpu_ops().mvs_sample(gd, cd, S, M, key)
    keep2, out2 = _gpu_ops().mvs_sample(gd, cd, S, M, key)
    assert keep.dtype == torch.uint8 and out.dtype == torch.float32
    for kk, oo in ((keep, out), (keep2, out2)):
        assert np.array_equal(kk.cpu().numpy(), want_keep.numpy())
        assert np.array_equal(oo.cpu().numpy().view(np.int32),
                              want_out.numpy().view(np.int32))


@pytest.mark.parametrize("shape", mc.PAST_SLOTS_SHAPES)
def test_hist_past_the_slot_count(shape):
    """More workgroups than histogram copies: copies are shared."""
    c, k = mc.past_slots_case(shape)
    ct = _t(c)
    dev = ct.cuda()
    g = _gpu_ops()
    assert np.array_equal(g.mvs_stats(dev).cpu().numpy(),
                          cpu.mvs_stats(ct).numpy())
    S, M = cpu.mvs_threshold(ct, k)
    assert M > 0 and S < k * (int(c.max()) + 1)  # the select ran
    assert g.mvs_threshold(dev, k) == (S, M)
    t = S // M
    for p in range(4):
        prefix = t >> (32 - 8 * p) if p else 0
        want = cpu.mvs_hist(ct, prefix, p).numpy()
        assert np.array_equal(g.mvs_hist(dev, prefix, p).cpu().numpy(), want)
        assert np.array_equal(g.mvs_hist(dev, prefix, p).cpu().numpy(), want)


def test_dispatch_by_device():
    """``ops.mvs_*`` pick the backend from the tensor's device."""
    from xgboost_ray_amd import ops

    c, k, gpair, key = mc.c_case("cauchy-4097")
    cd = _t(c).cuda()
    S, M = ops.mvs_threshold(cd, k)
    assert (S, M) == tuple(mc.threshold_expected("cauchy-4097")[:2])
    keep, out = ops.mvs_sample(_t(gpair).cuda(), cd, S, M, key)
    assert keep.is_cuda and out.is_cuda
    assert np.array_equal(keep.cpu().numpy(),
                          mc.sample_expected("cauchy-4097")[0])
