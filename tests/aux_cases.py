"""Cases and independent references for the kernels outside the tree loop.

``tests/test_aux_oracles.py`` (CPU paths vs these references) and
``tests/test_aux_ops_gpu.py`` (HIP kernels vs the same references) both import
this module. It covers the fused gradient, the fused logloss and AUC
statistics, the LambdaRank gradients and the packed-node tree walk.

numpy and Python only: no reference imports ``xgboost_ray_amd.ops`` or an
objective or metric class. Every reference works in float64 and states the
op's contract in its docstring. Every generator asserts that the case really
holds the edge it is named for. Case lists are built once per process.
"""

import functools
import math

import numpy as np

F32 = np.float32
U24 = 2.0 ** -24   # half an ulp of a float32 in [1, 2)
U53 = 2.0 ** -53   # half an ulp of a float64 in [1, 2)
EPS = 1e-16        # hessian floor and probability clamp of the project
HALF_UP = float(np.nextafter(F32(0.5), F32(1.0)))  # next float32 above 0.5
DENORMAL = float(np.float32(1e-41))


def _sigmoid64(x):
    """1 / (1 + exp(-x)) in float64; exp overflow gives exactly 0."""
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


# ---------------------------------------------------------------------------
# grad_fused
# ---------------------------------------------------------------------------
GRAD_SPECIALS = (0.0, -0.0, 1e-8, -1e-8, 16.7, -16.7, 88.0, -88.0, 89.0,
                 -89.0, 104.0, -104.0, np.inf, -np.inf, DENORMAL)
GRAD_NS = (1, 255, 256, 257, 4095, 4096, 4097, 70_001)
GRAD_BIG_N = 16_777_219      # > 4096 blocks * 256 threads * 16 rows


def ref_grad(margin, label, weight, spw, mode):
    """Gradient pair of one row, float64 throughout -> [n, 2].

    mode 1 (binary:logistic): p = 1/(1+exp(-x)), g = p - y,
    h = max(p(1-p), 1e-16), both times 1+(spw-1)*y, then times the weight.
    mode 0 (reg:squarederror): g = x - y, h = 1, then times the weight
    (spw plays no part). NaN in, NaN out - in g and, for mode 1, in h.
    """
    x = np.asarray(margin, np.float64)
    y = np.asarray(label, np.float64)
    with np.errstate(invalid="ignore"):
        if mode == 1:
            p = _sigmoid64(x)
            g = p - y
            h = np.maximum(p * (1.0 - p), EPS)   # np.maximum keeps NaN
            f = 1.0 + (float(spw) - 1.0) * y
            g = g * f
            h = h * f
        else:
            g = x - y
            h = np.ones_like(x)
        if weight is not None:
            w = np.asarray(weight, np.float64)
            g = g * w
            h = h * w
    return np.stack([g, h], axis=1)


# Largest distance of the project's own float32 torch composition (the CPU
# path of Logistic / SquaredError) from ref_grad over grad_cases(), in units
# of 2^-24 * max(1, |w * spw factor|): measured 2.14 for mode 1 and 119.2 for
# mode 0, rounded up. Mode 0 is so much larger because the unit ignores |g|:
# x - y rounds to half an ulp of a result that reaches 2 * 104 before the
# weight is applied. The HIP kernel is allowed twice these
# (tests/test_aux_ops_gpu.py).
GRAD_CPU_UNITS = {0: 120.0, 1: 2.25}


def grad_f32_mode0(margin, label, weight):
    """Mode 0 in float32: f32(x - y), then f32(g * w). IEEE subtraction and
    multiplication are correctly rounded, so host and device agree bitwise."""
    g = np.asarray(margin, F32) - np.asarray(label, F32)
    h = np.ones_like(g)
    if weight is not None:
        with np.errstate(invalid="ignore"):
            g = g * np.asarray(weight, F32)
        h = h * np.asarray(weight, F32)
    return np.stack([g, h], axis=1)


def grad_unit(label, weight, spw, mode):
    """2^-24 * max(1, |w * spw factor|) per row: the unit the float32
    gradient error is counted in."""
    f = np.ones(len(label), np.float64)
    if mode == 1:
        f = 1.0 + (float(spw) - 1.0) * np.asarray(label, np.float64)
    if weight is not None:
        f = f * np.asarray(weight, np.float64)
    return U24 * np.maximum(1.0, np.abs(f))


def grad_error_units(got, ref, unit):
    """max over finite reference entries of |got - ref| / unit; entries whose
    reference is +-inf or NaN must match in kind and are asserted here."""
    got = np.asarray(got, np.float64)
    fin = np.isfinite(ref)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), "NaN pattern differs"
    inf = ~fin & ~nan
    assert np.array_equal(got[inf], ref[inf]), "infinite entries differ"
    if not fin.any():
        return 0.0
    err = np.abs(np.where(fin, got - np.where(fin, ref, 0.0), 0.0))
    return float((err / unit[:, None]).max())


def _labels(n, rng):
    y = (rng.rand(n) < 0.4).astype(F32)
    y[rng.rand(n) < 0.1] = F32(0.3)
    return y


def _grad_case(n, mode, spw, weighted, seed):
    rng = np.random.RandomState(seed)
    m = (rng.randn(n) * 2.0).astype(F32)
    y = _labels(n, rng)
    if n == 1:
        sp_pos = np.array([0])
        m[0] = F32(16.7 if mode == 1 else -88.0)
    else:
        sp_pos = (7 + 13 * np.arange(len(GRAD_SPECIALS))) % n
        assert len(set(sp_pos.tolist())) == len(GRAD_SPECIALS)
        m[sp_pos] = np.asarray(GRAD_SPECIALS, F32)
        y[sp_pos[:6]] = np.asarray([0, 1, 0.3, 1, 0, 1], F32)
        assert m[sp_pos[-1]] != 0 and abs(m[sp_pos[-1]]) < 1.2e-38  # denormal
    w = None
    if weighted:
        w = (rng.rand(n) * 2.0).astype(F32)
        zero = rng.rand(n) < 0.1
        zero[sp_pos] = False          # 0 * inf would make a NaN gradient
        w[zero] = 0.0
        if n > 1:
            w[(sp_pos[0] + 1) % n] = 0.0
            assert (w == 0).any()
    c = {"id": f"n{n}-m{mode}-spw{spw:g}-{'w' if weighted else 'nw'}",
         "n": n, "mode": mode, "spw": float(spw), "margin": m, "label": y,
         "weight": w, "kind": "grid"}
    assert not np.isnan(ref_grad(m, y, w, spw, mode)).any()
    return c


def _grad_peak_case(n, mode, where, seed):
    """The largest |g| and the largest |h| sit at chosen rows: row 0, the
    last row (the tail of the last block) or a lane inside a wave."""
    rng = np.random.RandomState(seed)
    m = (rng.randn(n) * 2.0).astype(F32)
    y = _labels(n, rng)
    w = np.ones(n, F32)
    w[rng.rand(n) < 0.1] = 0.0
    if where == "first":
        pg, ph = 0, n - 1
    elif where == "last":
        pg, ph = n - 1, 0
    else:
        pg, ph = 256 * 5 + 37, 256 * 2 + 101
        assert n > pg and pg % 64 != 0 and ph % 64 != 0
    # g peak: a confidently wrong row with weight 50; h peak: margin 0, w 40
    m[pg], y[pg], w[pg] = (F32(-30.0), F32(1.0), F32(50.0))
    m[ph], y[ph], w[ph] = (F32(0.0), F32(1.0), F32(40.0))
    ref = ref_grad(m, y, w, 1.0, mode)
    assert int(np.abs(ref[:, 0]).argmax()) == pg
    assert int(np.abs(ref[:, 1]).argmax()) == (ph if mode == 1 else pg)
    assert np.abs(ref[:, 0]).max() > 2 * np.sort(np.abs(ref[:, 0]))[-2]
    return {"id": f"peak-{where}-n{n}-m{mode}", "n": n, "mode": mode,
            "spw": 1.0, "margin": m, "label": y, "weight": w, "kind": "peak"}


@functools.lru_cache(maxsize=None)
def grad_cases():
    cases, seed = [], 1000
    for n in GRAD_NS:
        for mode, spw in ((0, 1.0), (1, 1.0), (1, 3.0)):
            for weighted in (False, True):
                seed += 1
                cases.append(_grad_case(n, mode, spw, weighted, seed))
    for n, where in ((257, "first"), (4097, "last"), (4097, "lane"),
                     (70_001, "lane"), (70_001, "last")):
        for mode in (0, 1):
            seed += 1
            cases.append(_grad_peak_case(n, mode, where, seed))
    # every gradient zero: the block maxes must come out as 0, not a seed
    y = _labels(4097, np.random.RandomState(5))
    cases.append({"id": "allzero-n4097-m0", "n": 4097, "mode": 0, "spw": 1.0,
                  "margin": y.copy(), "label": y, "weight": None,
                  "kind": "zero"})
    assert not ref_grad(y, y, None, 1.0, 0)[:, 0].any()
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def grad_nan_cases():
    out = []
    for mode in (0, 1):
        c = dict(_grad_case(4097, mode, 1.0, False, 77 + mode))
        c["margin"] = c["margin"].copy()
        c["margin"][[0, 300, 4096]] = np.nan
        c["id"] = f"nan-n4097-m{mode}"
        c["kind"] = "nan"
        out.append(c)
    return tuple(out)


def grad_big_case():
    """More rows than 4096 blocks of 256 threads cover at 16 rows each, so
    the grid-stride loop runs past its planned trip count. Not cached: the
    arrays are large."""
    n = GRAD_BIG_N
    assert n > 4096 * 256 * 16
    rng = np.random.RandomState(9)
    m = (rng.randn(n) * 2.0).astype(F32)
    y = (rng.rand(n) < 0.4).astype(F32)
    m[-1], y[-1] = F32(-20.0), F32(1.0)     # the peak is the very last row
    return {"id": f"big-n{n}-m1", "n": n, "mode": 1, "spw": 1.0,
            "margin": m, "label": y, "weight": None, "kind": "big"}


# ---------------------------------------------------------------------------
# eval_logloss
# ---------------------------------------------------------------------------
LOGLOSS_NS = (1, 255, 257, 4097, 70_001)
LOGLOSS_BIG_N = 8_388_613    # > 2048 blocks * 256 threads * 16 rows
LOGLOSS_SPECIALS = (40.0, -40.0, 745.0, -745.0, np.inf, -np.inf)


def logloss_adds_per_thread(n):
    """Rows one thread of the kernel's grid adds up (grid = min(ceil(n/4096),
    2048) blocks of 256 threads); any pairwise or blocked host sum is shorter
    than this chain plus the 16 tree steps that follow it."""
    blocks = min(-(-n // 4096), 2048)
    return -(-n // (blocks * 256))


def ref_logloss(margin, label, weight):
    """Logloss statistics [sum w*ll, sum w] in float64 and their error bound.

    ll = -(y log p + (1-y) log(1-p)), p = 1/(1+exp(-x)) clamped to
    [1e-16, 1-1e-16]; w = 1 without a weight. A NaN margin makes the first
    statistic NaN. Sums are exact (math.fsum).

    The bound (a pair, one per statistic) allows 4 ulp of error in p,
    carried through both logarithms row by row, weighted and summed, plus
    (adds per thread + 16) * 2^-53 * sum|w*ll| for the order of summation.
    Rows whose p is clamped carry no error of the first kind.
    """
    x = np.asarray(margin, np.float64)
    y = np.asarray(label, np.float64)
    n = len(x)
    w = np.ones(n) if weight is None else np.asarray(weight, np.float64)
    p_raw = _sigmoid64(x)
    lo, hi = EPS, 1.0 - EPS
    p = np.where(p_raw < lo, lo, np.where(p_raw > hi, hi, p_raw))  # keeps NaN
    with np.errstate(invalid="ignore"):
        ll = -(y * np.log(p) + (1.0 - y) * np.log(1.0 - p))
    wll = w * ll
    stats = np.array([math.fsum(wll.tolist()) if not np.isnan(wll).any()
                      else np.nan, math.fsum(w.tolist())])
    free = (p_raw >= lo) & (p_raw <= hi)
    with np.errstate(invalid="ignore", divide="ignore"):
        odds = np.where(free, p / (1.0 - p), 0.0)
    ulp4 = 4.0 * 2.0 * U53
    e_p = np.where(free, ulp4 * (np.abs(y) + np.abs(1.0 - y) * odds), 0.0)
    # the bound's own sums need no exactness: plain numpy, rounded up
    up = 1.0 + 1e-9
    first = float((np.abs(w) * np.nan_to_num(e_p)).sum()) * up
    k = (logloss_adds_per_thread(n) + 16) * U53
    sum_abs = float(np.abs(np.nan_to_num(wll)).sum()) * up
    bound = np.array([first + k * sum_abs, k * float(np.abs(w).sum()) * up])
    return stats, bound, first


def _logloss_case(n, wkind, seed, big=False):
    rng = np.random.RandomState(seed)
    m = np.clip(rng.randn(n) * 3.0, -20.0, 20.0).astype(F32)
    y = _labels(n, rng)
    if n == 1:
        m[0] = F32(40.0)
    else:
        pos = (5 + 11 * np.arange(len(LOGLOSS_SPECIALS))) % n
        m[pos] = np.asarray(LOGLOSS_SPECIALS, F32)
        y[pos[:3]] = np.asarray([0, 1, 0.3], F32)
    w = None
    if wkind == "w":
        w = (rng.rand(n) * 2.0).astype(F32)
        w[rng.rand(n) < 0.1] = 0.0
        w[0] = 0.0 if n > 1 else w[0]
    elif wkind == "w0":
        w = np.zeros(n, F32)
    # margin bands: free rows within 20, every other row clamps anywhere
    a = np.abs(m.astype(np.float64))
    assert ((a <= 20.0) | (a >= 40.0)).all()
    c = {"id": f"n{n}-{wkind}", "n": n, "margin": m, "label": y, "weight": w,
         "wkind": wkind}
    if not big:
        stats, bound, first = ref_logloss(m, y, w)
        assert first <= 1e-7 * max(abs(stats[0]), 1e-300) or wkind == "w0"
        c["ref"] = (stats, bound)
    return c


@functools.lru_cache(maxsize=None)
def logloss_cases():
    cases, seed = [], 2000
    for n in LOGLOSS_NS:
        for wkind in ("nw", "w"):
            seed += 1
            cases.append(_logloss_case(n, wkind, seed))
    cases.append(_logloss_case(4097, "w0", 2100))
    return tuple(cases)


def logloss_nan_case():
    c = dict(_logloss_case(4097, "w", 2200))
    c["margin"] = c["margin"].copy()
    c["margin"][[1, 4096]] = np.nan
    c["weight"] = c["weight"].copy()
    c["weight"][[1, 4096]] = 1.0
    c["id"] = "nan-n4097-w"
    c.pop("ref")
    return c


def logloss_big_case():
    n = LOGLOSS_BIG_N
    assert n > 2048 * 256 * 16
    return _logloss_case(n, "nw", 2300, big=True)


# ---------------------------------------------------------------------------
# eval_auc_hist
# ---------------------------------------------------------------------------
AUC_NS = (1, 257, 16_385, 70_001)
AUC_BINS = (1, 2, 1000, 16384)
AUC_BIG_N = 4_194_311        # > 256 blocks * 256 threads * 64 rows
AUC_EDGE_ULPS = 16


def ref_auc_hist(margin, label, B):
    """int64 [2B] score histogram, planes [negative | positive].

    A row falls in bin min(trunc(p*B), B-1) with p = 1/(1+exp(-x)) in
    float64, and is positive iff its float32 label is > 0.5.
    """
    p = _sigmoid64(margin)
    b = np.minimum((p * float(B)).astype(np.int64), B - 1)
    pos = (np.asarray(label, F32) > F32(0.5)).astype(np.int64)
    return np.bincount(pos * B + b, minlength=2 * B).astype(np.int64)


def auc_edge_distance_ulps(margin, B):
    """Smallest distance, in ulps of p*B, of a row from an inner bin edge
    (edges 1 .. B-1; the outer two are clamped away). Rows with margin
    exactly 0 are left out: exp(0) = 1 and 1/2 are exact everywhere."""
    m = np.asarray(margin, np.float64)
    t = _sigmoid64(m) * float(B)
    k = np.rint(t)
    inner = (k >= 1) & (k <= B - 1) & (m != 0)
    if not inner.any():
        return np.inf
    return float((np.abs(t - k)[inner] / np.spacing(t[inner])).min())


def _auc_case(n, B, seed, kind="mix"):
    rng = np.random.RandomState(seed)
    if kind == "onebin":
        m = np.zeros(n, F32)
        m[::2] = F32(-0.0)
    elif kind == "ends":
        m = np.where(rng.rand(n) < 0.5, 50.0, -50.0).astype(F32)
        m[:4] = np.asarray([np.inf, -np.inf, 50.0, -50.0], F32)
    else:
        m = (rng.randn(n) * 3.0).astype(F32)
        if n > 1:
            pos = (3 + 17 * np.arange(6)) % n
            m[pos] = np.asarray([np.inf, -np.inf, 50.0, -50.0, 0.0, -0.0],
                                F32)
    y = (rng.rand(n) < 0.4).astype(F32)
    y[rng.rand(n) < 0.1] = F32(0.3)
    y[rng.rand(n) < 0.1] = F32(0.5)
    y[rng.rand(n) < 0.1] = F32(HALF_UP)
    if n == 1:
        y[0] = F32(HALF_UP)
    elif kind != "mix" or n >= 257:
        y[:3] = np.asarray([0.5, HALF_UP, 0.3], F32)
    d = auc_edge_distance_ulps(m, B)
    assert d > AUC_EDGE_ULPS, (n, B, d)
    ref = ref_auc_hist(m, y, B)
    assert int(ref.sum()) == n
    if kind == "onebin":
        assert ref[B // 2] + ref[B + B // 2] == n
    if kind == "ends" and B > 1:
        assert ref[0] + ref[B] > 0 and ref[B - 1] + ref[2 * B - 1] > 0
        assert ref[0] + ref[B] + ref[B - 1] + ref[2 * B - 1] == n
    return {"id": f"{kind}-n{n}-B{B}", "n": n, "B": B, "margin": m,
            "label": y, "ref": ref, "edge_ulps": d, "kind": kind}


@functools.lru_cache(maxsize=None)
def auc_cases():
    cases, seed = [], 3000
    for n in AUC_NS:
        for B in AUC_BINS:
            seed += 1
            cases.append(_auc_case(n, B, seed))
    for B in (2, 16384):
        cases.append(_auc_case(257, B, 3100 + B, "onebin"))
        cases.append(_auc_case(16_385, B, 3200 + B, "ends"))
    # the measurement quoted in docs/parity.md
    m = (np.random.RandomState(7).randn(70_001) * 3.0).astype(F32)
    assert auc_edge_distance_ulps(m, 16384) > 1e5
    return tuple(cases)


def auc_big_case():
    n = AUC_BIG_N
    assert n > 256 * 256 * 64
    return _auc_case(n, 16384, 3300)


# ---------------------------------------------------------------------------
# lambdarank
# ---------------------------------------------------------------------------
RANK_SIZES_A = (1, 2, 3, 63, 64, 65, 255, 256, 257, 700, 1, 40)


def stable_rank_desc(m):
    """0-based rank of each row in the stable descending order of m: ties
    keep their original order."""
    order = np.argsort(-np.asarray(m, np.float64), kind="stable")
    rank = np.empty(len(m), np.int64)
    rank[order] = np.arange(len(m))
    return rank


def ref_rank_prep(margin, label, group_ptr):
    """(rank int32 [n], idcg float64 [G]) as the kernel takes them: rank by
    stable descending margin inside each group; idcg = sum over the
    label-sorted order of (2^y - 1) / log2(k + 2)."""
    n, G = len(margin), len(group_ptr) - 1
    rank = np.zeros(n, np.int32)
    idcg = np.zeros(G, np.float64)
    for g in range(G):
        s, e = int(group_ptr[g]), int(group_ptr[g + 1])
        rank[s:e] = stable_rank_desc(margin[s:e])
        gain = np.sort(np.exp2(np.asarray(label[s:e], np.float64)) - 1.0)[::-1]
        disc = 1.0 / np.log2(np.arange(e - s, dtype=np.float64) + 2.0)
        idcg[g] = math.fsum((gain * disc).tolist())
    return rank, idcg


def ref_lambdarank(margin, label, group_ptr, ndcg):
    """LambdaRank gradient pairs in float64 -> (gpair [n, 2], S [n, 2]).

    Inside a group every ordered pair (i, j) with label_i > label_j adds
    rho = 1/(1+exp(m_i - m_j)) times the pair weight: -rho*w to g_i, +rho*w
    to g_j, and max(rho(1-rho), 1e-16)*w to both hessians (the floor comes
    before the weight). m_i - m_j is formed in float32 and then widened: the
    kernel computes (double)(mi - mj), and that is the contract. Pairs with
    equal labels are skipped. ndcg: w = |dgain * ddisc| / idcg with
    gain = 2^y - 1, disc = 1/log2(rank + 2), rank and idcg as in
    ``ref_rank_prep``; otherwise w = 1. A group with idcg <= 0 (ndcg) or
    fewer than two rows gives zeros.

    S holds, per row, the sum of the absolute pair terms of g and of h: the
    scale every summation-error bound is stated in.
    """
    m32 = np.asarray(margin, F32)
    y32 = np.asarray(label, F32)
    n = len(m32)
    out = np.zeros((n, 2), np.float64)
    S = np.zeros((n, 2), np.float64)
    rank, idcg = ref_rank_prep(m32, y32, group_ptr)
    for gi in range(len(group_ptr) - 1):
        s, e = int(group_ptr[gi]), int(group_ptr[gi + 1])
        if e - s < 2 or (ndcg and not idcg[gi] > 0.0):
            continue
        m, y = m32[s:e], y32[s:e]
        d = (m[:, None] - m[None, :]).astype(np.float64)   # float32 subtract
        win = y[:, None] > y[None, :]
        if not win.any():
            continue
        with np.errstate(over="ignore"):
            rho = 1.0 / (1.0 + np.exp(d))
        hess = np.maximum(rho * (1.0 - rho), EPS)
        if ndcg:
            gain = np.exp2(y.astype(np.float64)) - 1.0
            disc = 1.0 / np.log2(rank[s:e].astype(np.float64) + 2.0)
            w = np.abs((gain[:, None] - gain[None, :])
                       * (disc[:, None] - disc[None, :])) / idcg[gi]
            rho = rho * w
            hess = hess * w
        rho = np.where(win, rho, 0.0)
        hess = np.where(win, hess, 0.0)
        out[s:e, 0] = -rho.sum(1) + rho.sum(0)
        S[s:e, 0] = rho.sum(1) + rho.sum(0)
        out[s:e, 1] = hess.sum(1) + hess.sum(0)
        S[s:e, 1] = out[s:e, 1]
    return out, S


def _rank_case(name, sizes, seed, special=False):
    rng = np.random.RandomState(seed)
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(gp[-1])
    m = rng.randn(n).astype(F32)
    y = rng.randint(0, 5, n).astype(F32)
    c = {"id": name, "n": n, "group_ptr": gp, "sizes": tuple(sizes)}
    if special:
        def grp(size):
            g = list(sizes).index(size)
            return slice(int(gp[g]), int(gp[g + 1]))
        eq_label, eq_margin, wide, big_label = grp(64), grp(256), grp(255), \
            grp(65)
        y[eq_label] = 2.0
        m[eq_margin] = F32(0.25)
        m[wide] = np.linspace(-60.0, 60.0, 255).astype(F32)[
            rng.permutation(255)]
        # badly misordered: the lowest scores carry the highest label, so
        # every pair of such a row is more than 37 apart and its whole
        # hessian is made of floored terms
        y[wide] = np.where(m[wide] < -20.0, 3.0,
                           np.where(m[wide] > 20.0, 0.0, y[wide])).astype(F32)
        y[big_label] = rng.randint(0, 32, 65).astype(F32)
        y[big_label.start] = 31.0
        y[grp(700).start + 3] = 0.5
        y[grp(257)] = rng.randint(0, 3, 257).astype(F32)
        m[grp(257)] = np.round(rng.randn(257) * 2.0).astype(F32)  # many ties
        c["tied_group"] = eq_margin
        c["wide_group"] = wide
        assert len(set(y[eq_label])) == 1 and len(set(m[eq_margin])) == 1
        assert len(set(y[eq_margin])) > 1 and y.max() == 31.0
        assert float(np.ptp(m[wide])) == 120.0
    c["margin"], c["label"] = m, y
    c["qid"] = np.repeat(np.arange(len(sizes)), sizes).astype(np.int64)
    c["weight"] = (rng.rand(n) * 2.0).astype(F32)
    for ndcg in (False, True):
        c["ref", ndcg] = ref_lambdarank(m, y, gp, ndcg)
    c["prep"] = ref_rank_prep(m, y, gp)
    return c


@functools.lru_cache(maxsize=None)
def rank_cases():
    rng = np.random.RandomState(41)
    cases = (
        _rank_case("sizes-a", RANK_SIZES_A, 4001, special=True),
        _rank_case("g5000-small", rng.randint(2, 6, 5000).tolist(), 4002),
        _rank_case("one-row", (1,), 4003),
    )
    a = cases[0]
    assert max(a["sizes"]) > 2 * 256 and 1 in a["sizes"] and 2 in a["sizes"]
    # exp overflows float32 and the hessian floor is live in the wide group
    m, y = a["margin"][a["wide_group"]], a["label"][a["wide_group"]]
    d = np.abs(m[:, None] - m[None, :])
    differ = y[:, None] != y[None, :]
    assert ((d > 89.0) & differ).any()
    assert np.where(differ, d, np.inf).min(1).min() < 1.0 < 37.0 \
        < np.where(differ, d, np.inf).min(1).max()   # all-floored rows exist
    S = a["ref", False][1][a["wide_group"], 1]
    assert 0 < S.min() < 255 * 1.01e-16
    return cases


def rank_round0_case():
    """Round 0 of a ranking run: about 40 groups, every margin equal."""
    rng = np.random.RandomState(4100)
    sizes = rng.randint(2, 60, 40).tolist()
    c = _rank_case("round0-ties", sizes, 4101)
    c["margin"] = np.full(c["n"], 0.5, F32)
    for ndcg in (False, True):
        c["ref", ndcg] = ref_lambdarank(c["margin"], c["label"],
                                        c["group_ptr"], ndcg)
    c["prep"] = ref_rank_prep(c["margin"], c["label"], c["group_ptr"])
    return c


# ---------------------------------------------------------------------------
# predict
# ---------------------------------------------------------------------------
PRED_TILE_NODES = 4096
PRED_NS = (1, 255, 2047, 2048, 2049, 5000)
PRED_FORESTS = {
    "leafroot": (1,),
    "small": (3, 7, 15),
    "fulltile": (4095, 1),
    "tileedges": (4095, 3, 4093, 3, 1),
    "threetiles": (31,) * 300,
    "overtile": (15, 4097, 15),
}
_POOL_SPECIALS = (np.nan, np.inf, -np.inf, 0.0, -0.0)


def value_pool(rng):
    """The few float32 values X and the thresholds are both drawn from, so
    x == thr happens all the time."""
    return np.concatenate([rng.randn(48).astype(F32),
                           np.asarray(_POOL_SPECIALS, F32)])


def make_X(n, F, pool, rng):
    idx = rng.randint(0, len(pool), (n, F))
    special = rng.rand(n, F) < 0.15
    idx[special] = len(pool) - 5 + rng.randint(0, 5, int(special.sum()))
    return pool[idx]


def random_tree(n_nodes, F, rng, pool, root_thr=None):
    """A random binary tree of ``n_nodes`` (odd) nodes whose children are
    allocated as pairs (right = left + 1, indices relative to the root).
    Thresholds come from the non-NaN values of ``pool``."""
    assert n_nodes % 2 == 1
    feat = np.full(n_nodes, -1, np.int32)
    thr = np.zeros(n_nodes, F32)
    left = np.zeros(n_nodes, np.int32)
    dleft = np.zeros(n_nodes, np.uint8)
    value = np.zeros(n_nodes, F32)
    cand = pool[~np.isnan(pool)]
    frontier, nxt = [0], 1
    while nxt < n_nodes:
        node = frontier.pop(int(rng.randint(len(frontier))))
        feat[node] = rng.randint(F)
        thr[node] = cand[rng.randint(len(cand))]
        left[node] = nxt
        dleft[node] = rng.randint(2)
        frontier += [nxt, nxt + 1]
        nxt += 2
    if root_thr is not None and n_nodes > 1:
        thr[0] = F32(root_thr)
    leaves = feat < 0
    nl = int(leaves.sum())
    value[leaves] = (rng.randn(nl) * 10.0 ** rng.randint(-3, 3, nl)).astype(F32)
    return feat, thr, left, dleft, value


def make_forest(node_counts, F, rng, pool):
    parts, forced = [], iter((0.0, np.inf))
    for nn in node_counts:
        parts.append(random_tree(nn, F, rng, pool,
                                 next(forced, None) if nn > 1 else None))
    cat = [np.concatenate([p[i] for p in parts]) for i in range(5)]
    tree_ptr = np.concatenate([[0], np.cumsum(node_counts)]).astype(np.int32)
    return dict(zip(("feat", "thr", "left", "default_left", "value"), cat),
                tree_ptr=tree_ptr)


def lds_tiles(node_counts):
    """Tree ranges the serving kernel stages per tile (greedy, <= 4096 nodes);
    None when one tree is larger than a tile and the plain kernel serves."""
    tiles, t, T = [0], 0, len(node_counts)
    while t < T:
        e, tot = t, 0
        while e < T and tot + node_counts[e] <= PRED_TILE_NODES:
            tot += node_counts[e]
            e += 1
        if e == t:
            return None
        tiles.append(e)
        t = e
    return tiles


def _leaf_py(x, forest, t):
    """Leaf node of tree t for one row, a plain Python walk."""
    base = int(forest["tree_ptr"][t])
    node = base
    while forest["feat"][node] >= 0:
        v = x[forest["feat"][node]]
        if v != v:
            go_left = bool(forest["default_left"][node])
        else:
            go_left = bool(F32(v) < forest["thr"][node])
        node = base + int(forest["left"][node]) + (0 if go_left else 1)
    return node


def _leaves_np(X, forest, stats=None):
    """[T, n] leaf node of every tree for every row, vectorised."""
    n = X.shape[0]
    T = len(forest["tree_ptr"]) - 1
    rows = np.arange(n)
    out = np.empty((T, n), np.int64)
    for t in range(T):
        base = int(forest["tree_ptr"][t])
        cur = np.full(n, base, np.int64)
        while True:
            f = forest["feat"][cur]
            live = f >= 0
            if not live.any():
                break
            x = X[rows, np.maximum(f, 0)]
            th = forest["thr"][cur]
            with np.errstate(invalid="ignore"):
                go_left = np.where(np.isnan(x),
                                   forest["default_left"][cur] != 0, x < th)
            if stats is not None:
                stats["eq"] |= bool((live & (x == th)).any())
                stats["nan"] |= bool((live & np.isnan(x)).any())
                stats["negzero"] |= bool(
                    (live & (th == 0) & (x == 0) & np.signbit(x)).any())
                stats["posinf"] |= bool(
                    (live & np.isposinf(th) & np.isposinf(x)).any())
            nxt = base + forest["left"][cur] + np.where(go_left, 0, 1)
            cur = np.where(live, nxt, cur)
        out[t] = cur
    return out


def sample_rows(n, limit=300):
    """First rows, last rows and the rows next to 256- and 2048-row
    boundaries (the first and last ten boundaries of each kind)."""
    rows = list(range(min(n, 16))) + list(range(max(n - 16, 0), n))
    for step in (2048, 256):
        ks = list(range(step, n + 1, step))
        for k in ks[:10] + ks[-10:]:
            rows += [k - 1, k, k + 1]
    rows = sorted({r for r in rows if 0 <= r < n})
    assert len(rows) <= limit
    return rows


def ref_predict(X, forest, out0, w, leaves=None):
    """Tree-walk prediction -> (device result, CPU-oracle result), float32.

    Each tree sends a row left iff x < thr in float32; a NaN follows
    ``default_left``; right child = left + 1, relative to the tree's base.
    Device contract, bitwise: out = f32(out0 + f32(acc * f32(w))) with acc
    the float32 sum of the leaf values in tree order, starting from 0 (the
    extension is built without FMA contraction). CPU-oracle contract, also
    bitwise: out += f32(value * f32(w)), tree by tree. The two orders round
    differently and are both pinned.
    """
    if leaves is None:
        leaves = _leaves_np(X, forest)
    wf = F32(w)
    acc = np.zeros(X.shape[0], F32)
    cpu = np.asarray(out0, F32).copy()
    for t in range(leaves.shape[0]):
        v = forest["value"][leaves[t]]
        acc = acc + v
        cpu = cpu + v * wf
    dev = np.asarray(out0, F32) + acc * wf
    assert dev.dtype == F32 and cpu.dtype == F32
    return dev, cpu


def _predict_case(fname, n, F, w, out0_kind, seed):
    rng = np.random.RandomState(seed)
    pool = value_pool(rng)
    counts = PRED_FORESTS[fname] if isinstance(fname, str) else fname
    forest = make_forest(counts, F, rng, pool)
    X = make_X(n, F, pool, rng)
    if out0_kind == "zero":
        out0 = np.zeros(n, F32)
    elif out0_kind == "half":
        out0 = np.full(n, 0.5, F32)
    else:
        out0 = rng.randn(n).astype(F32)
    stats = dict(eq=False, nan=False, negzero=False, posinf=False)
    leaves = _leaves_np(X, forest, stats)
    rows = sample_rows(n)
    for r in rows:   # the vectorised walk agrees with the row loop
        for t in range(len(counts)):
            assert _leaf_py(X[r], forest, t) == leaves[t, r], (fname, r, t)
    dev, cpu = ref_predict(X, forest, out0, w, leaves)
    name = fname if isinstance(fname, str) else "x".join(map(str, fname))
    return {"id": f"{name}-n{n}-F{F}-w{w:g}-{out0_kind}", "forest_name": name,
            "n": n, "F": F, "w": w, "X": X, "forest": forest, "out0": out0,
            "ref_dev": dev, "ref_cpu": cpu, "stats": stats,
            "rows_checked": len(rows), "tiles": lds_tiles(list(counts))}


@functools.lru_cache(maxsize=None)
def predict_cases():
    combos = [(f, 2049) for f in PRED_FORESTS]
    combos += [("tileedges", n) for n in PRED_NS if n != 2049]
    combos += [("small", n) for n in PRED_NS if n != 2049]
    combos += [("threetiles", 255), ("overtile", 5000), ("fulltile", 2048)]
    Fs, ws, o0 = (7, 1, 33), (0.3, 1.0), ("rand", "zero", "half")
    cases = tuple(
        _predict_case(f, n, Fs[i % 3], ws[(i // 2) % 2], o0[(i // 3) % 3],
                      5000 + i)
        for i, (f, n) in enumerate(combos))
    # the named edges are present
    assert lds_tiles([4095, 1]) == [0, 2]
    assert lds_tiles([4095, 3, 4093, 3, 1]) == [0, 1, 3, 5]
    assert lds_tiles([31] * 300) == [0, 132, 264, 300]
    assert lds_tiles([15, 4097, 15]) is None
    for f in PRED_FORESTS:
        mine = [c for c in cases if c["forest_name"] == f]
        assert any(c["n"] == 2049 for c in mine)
        if f == "leafroot":
            continue
        for key in ("eq", "nan", "negzero", "posinf"):
            assert any(c["stats"][key] for c in mine), (f, key)
    assert {c["n"] for c in cases if c["forest_name"] == "tileedges"} \
        == set(PRED_NS)
    assert {c["F"] for c in cases} == {1, 7, 33}
    assert {c["w"] for c in cases if c["forest_name"] == "tileedges"} \
        == {0.3, 1.0}
    for c in cases:   # the two accumulation orders really differ somewhere
        if c["forest_name"] == "threetiles":
            assert (c["ref_dev"] != c["ref_cpu"]).any()
    return cases


def predict_gridcap_case(kind):
    """F = 1, two 3-node trees, more rows than the 8192-block grid covers in
    one trip: 2048 rows a block on the LDS path, 256 on the plain one."""
    n = {"lds": 16_777_217, "plain": 2_097_153}[kind]
    assert n > 8192 * {"lds": 2048, "plain": 256}[kind]
    return _predict_case((3, 3), n, 1, 0.3, "half", 5900)
