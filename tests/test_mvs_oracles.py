"""CPU ops of gradient-based row sampling against the brute-force oracle of
``tests/mvs_cases.py``, plus the properties the contract promises
(docs/parity.md, "Gradient-based sampling")."""

import math

import numpy as np
import pytest
import torch

from tests import mvs_cases as mc
from xgboost_ray_amd.ops import cpu


def _t(a):
    return torch.from_numpy(np.array(a))  # a writable copy


@pytest.mark.parametrize("case_id", mc.SCORE_IDS)
def test_score_equals_brute_force(case_id):
    gpair, mx_g, mx_h = mc.score_case(case_id)
    c = cpu.mvs_score(_t(gpair), mx_g, mx_h)
    assert c.dtype == torch.uint32
    got = c.numpy()
    assert np.array_equal(got, mc.score_expected(case_id))
    assert int(got.max()) <= mc.C_MAX
    # the row that holds both maxima scores 2^30 up to the rounding of sv
    if mx_g > 0 and abs(gpair[0, 0]) == mx_g and gpair[0, 1] == mx_h:
        assert mc.C_MAX - int(got[0]) <= 1


def test_score_zero_maxima_clamp():
    """mx_g = mx_h = 0: sv is inf, 0 * inf is NaN and NaN clamps."""
    gpair = np.zeros((5, 2), np.float32)
    c = cpu.mvs_score(_t(gpair), 0.0, 0.0).numpy()
    assert np.array_equal(c, mc.bf_score(gpair, 0.0, 0.0))
    assert np.array_equal(c, np.full(5, mc.C_MAX, np.uint32))


@pytest.mark.parametrize("case_id", mc.C_IDS)
def test_threshold_equals_brute_force(case_id):
    c, k, _, _ = mc.c_case(case_id)
    S, M, t = mc.threshold_expected(case_id)
    got = cpu.mvs_threshold(_t(c), k)
    assert tuple(int(v) for v in got) == (S, M)
    if S == 0:
        assert M == 0 and int((c > 0).sum()) <= k
        return
    # mu = S / M lies in [t*, t* + 1)
    assert M > 0 and t >= 1
    assert t * M <= S < (t + 1) * M
    # exactly the rows above t* are kept for certain
    ci = c.astype(np.int64)
    assert (ci[ci > t] * M >= S).all()  # c M < 2^61: no overflow
    assert (ci[ci < t] * M < S).all()


@pytest.mark.parametrize("case_id", mc.C_IDS)
@pytest.mark.parametrize("pass_idx", range(4))
def test_hist_equals_definition(case_id, pass_idx):
    c = mc.c_case(case_id)[0].astype(np.int64)
    prefix, _ = mc.radix_path(case_id)[pass_idx]
    h = cpu.mvs_hist(_t(mc.c_case(case_id)[0]), prefix, pass_idx).numpy()
    sel = c if pass_idx == 0 else c[(c >> (32 - 8 * pass_idx)) == prefix]
    digit = (sel >> (24 - 8 * pass_idx)) & 255
    for d in np.unique(digit):
        assert h[d, 0] == int((digit == d).sum())
        assert h[d, 1] == int(sel[digit == d].sum())
    assert int(h[:, 0].sum()) == len(sel)
    assert int(h[:, 1].sum()) == int(sel.sum())


@pytest.mark.parametrize("case_id", mc.C_IDS)
def test_sample_equals_brute_force(case_id):
    c, _, gpair, key = mc.c_case(case_id)
    S, M, _ = mc.threshold_expected(case_id)
    keep, out = cpu.mvs_sample(_t(gpair), _t(c), S, M, key)
    exp_keep, exp_out = mc.sample_expected(case_id)
    assert keep.dtype == torch.uint8 and out.dtype == torch.float32
    assert np.array_equal(keep.numpy(), exp_keep)
    assert np.array_equal(out.numpy().view(np.int32), exp_out.view(np.int32))
    # every kept pair is the float64 formula; every dropped one is zero
    keep = keep.numpy().astype(bool)
    out = out.numpy()
    assert not out[~keep].any()
    assert not keep[c == 0].any()
    if S == 0:
        assert np.array_equal(keep, c > 0)
        assert np.array_equal(out[keep], gpair[keep])
        return
    cm = c.astype(np.int64) * M
    sure = keep & (cm >= S)
    assert np.array_equal(out[sure], gpair[sure])
    assert np.array_equal(sure, (c > 0) & (cm >= S))
    part = keep & ~sure
    f = np.float64(S) / cm[part].astype(np.float64)
    want = (gpair[part].astype(np.float64) * f[:, None]).astype(np.float32)
    assert np.array_equal(out[part], want)


@pytest.mark.parametrize("case_id", mc.C_IDS)
def test_sample_size_within_six_sigma(case_id):
    """The expected sample size is k and its variance sum p (1 - p) <= k."""
    c, k, gpair, _ = mc.c_case(case_id)
    S, M, _ = mc.threshold_expected(case_id)
    if S == 0:
        # no threshold: exactly the rows with c > 0, at most k of them
        keep, _ = cpu.mvs_sample(_t(gpair), _t(c), S, M, 0)
        assert int(keep.sum()) == int((c > 0).sum()) <= k
        return
    # expected size = sum min(1, c M / S), in exact rationals: k
    ci = c.astype(np.int64)
    sure = int((ci * M >= S).sum())
    rest = int(ci[ci * M < S].sum())
    assert rest * M == (k - sure) * S
    for key in range(20):
        keep, _ = cpu.mvs_sample(_t(gpair), _t(c), S, M, key)
        size = int(keep.sum())
        assert abs(size - k) <= 6.0 * math.sqrt(k), (key, size, k)


def test_key_separates_its_ingredients():
    keys = {cpu.mvs_key(s, it, t, r)
            for s in range(3) for it in range(4)
            for t in (0, 1, 101, 102) for r in range(3)}
    assert len(keys) == 3 * 4 * 4 * 3
    assert all(0 <= k < 1 << 64 for k in keys)
    # streams are key + i: neighbouring ingredients must not be neighbours
    ks = sorted(keys)
    assert min(b - a for a, b in zip(ks, ks[1:])) > 1 << 32
