"""Deterministic small-case generators for the op-level oracle tests.

Plain Python, no fixtures: ``tests/test_op_oracles.py`` (CPU oracle vs brute
force) and ``tests/test_ops_gpu_edges.py`` (HIP kernels vs CPU oracle) both
import it. Every generator returns CPU tensors plus a short id, and asserts
that the case really contains the edge it is named for, so a later edit
cannot silently lose coverage. The case lists are built once per process.
"""

import functools
import math

import numpy as np
import torch

MISSING = 255
POISON = 0x5A5A5A5A  # fills pregathered gradient slots no segment owns

# rows one workgroup covers on each histogram route (kernels.hip): the
# direct/XCD override (512), multifb R*512 for R in {4, 8, 16, 32}, the XCD
# default for K >= 512 (8192) and the base / XCD default (16384)
HIST_CHUNK_SIZES = (512, 2048, 4096, 8192, 16384)
PART_CHUNK = 2048  # partition / update_margins rows per workgroup

# non-power-of-two quantisation scales: (double)q * (1/scale) is inexact
SCALE_G = 2.0**28 / 0.7310586
SCALE_H = 2.0**28 / 0.19661193


def _layout(counts, rng, first=5):
    """Segment starts for ``counts`` with a first start above 0 and gaps;
    returns (starts, n) where n > last end (the tail is owned by nobody)."""
    starts, pos = [], first
    for i, c in enumerate(counts):
        starts.append(pos)
        pos += int(c) + (1 + int(rng.randint(0, 3)) if i % 2 == 0 else 0)
    return np.asarray(starts, np.int64), pos + 3


def padded_bins(b):
    """The engine's layout: a [n, F_pad] buffer of 255 narrowed to [:, :F]."""
    n, F = b.shape
    F_pad = (F + 15) // 16 * 16
    full = torch.full((n, F_pad), MISSING, dtype=torch.uint8)
    full[:, :F] = torch.as_tensor(b)
    return full[:, :F]


# ---------------------------------------------------------------------------
# histogram
# ---------------------------------------------------------------------------
def _hist_counts(layout, rng):
    if layout == "a":
        return np.array([0, 1, 511, 512, 513, 0, 2047, 2049], np.int64)
    if layout == "b":
        return np.array([16385, 3], np.int64)
    c = rng.randint(1, 41, 520).astype(np.int64)
    c[[7, 255, 400]] = 0
    return c


def _hist_case(n_bins, F, layout, seed):
    rng = np.random.RandomState(seed)
    counts = _hist_counts(layout, rng)
    starts, n = _layout(counts, rng)
    assert n <= 40_000
    top = min(n_bins, MISSING)  # bin 255 always means "missing"
    b = rng.randint(0, top, (n, F)).astype(np.uint8)
    b[rng.rand(n, F) < 0.10] = MISSING
    if F >= 3:
        b[:, F - 1] = MISSING      # all-missing feature (partial block)
        b[:, 1] = top - 1          # every row in the same (top) bin
    gq = rng.randint(-(2**20), 2**20, (n, 2)).astype(np.int64)
    big = rng.rand(n, 2) < 0.01
    gq[big] = np.where(rng.rand(int(big.sum())) < 0.5, -(2**30), 2**30)
    gq = gq.astype(np.int32)
    ridx = rng.permutation(n).astype(np.int32)
    gseg = np.full((n, 2), POISON, np.int32)
    for s, c in zip(starts, counts):
        gseg[s:s + c] = gq[ridx[s:s + c]]
    case = {
        "id": f"nb{n_bins}-F{F}-{layout}",
        "layout": layout, "n_bins": n_bins, "F": F, "n": n,
        "bins": padded_bins(b),
        "bins_flat": torch.from_numpy(b.copy()),
        "gq": torch.from_numpy(gq),
        "gseg": torch.from_numpy(gseg),
        "ridx": torch.from_numpy(ridx),
        "starts": torch.from_numpy(starts),
        "counts": torch.from_numpy(counts),
    }
    # self-checks: the named edges are really present
    assert case["bins"].stride(0) % 16 == 0 and starts[0] > 0
    assert int((starts[1:] - (starts[:-1] + counts[:-1])).max()) > 0  # gaps
    assert (np.abs(gq) == 2**30).any() and (gq < 0).any() and (gq > 0).any()
    if F >= 3:
        assert (b[:, F - 1] == MISSING).all() and (b[:, 1] == top - 1).all()
    if layout in "ac":
        assert (counts[:-1] == 0).any()        # empty, and not the last one
        assert (counts == 1).any()             # one-row segment
    return case


def hist_xcd_chunks(case, rows=None):
    """Row-chunk count of the XCD route (its default chunk size unless
    ``rows`` overrides it, as RXGB_HIST_XCD_ROWS does)."""
    if rows is None:
        rows = 8192 if len(case["counts"]) >= 512 else 16384
    return int(((case["counts"] + rows - 1) // rows).sum())


@functools.lru_cache(maxsize=None)
def hist_cases():
    nbs, Fs, layouts = (256, 255, 64, 37), (1, 16, 17, 40), "abc"
    cases = []
    for i, nb in enumerate(nbs):
        for j, F in enumerate(Fs):
            cases.append(_hist_case(nb, F, layouts[(i + j) % 3],
                                    seed=100 + 10 * i + j))
    cases = tuple(cases)
    # every n_bins and every F meets every layout
    for key, vals in (("n_bins", nbs), ("F", Fs)):
        for v in vals:
            assert {c["layout"] for c in cases if c[key] == v} == set("abc")
    # a one-row tail past a full chunk, for each chunk size in use
    for rows in HIST_CHUNK_SIZES:
        assert any(((c["counts"] > rows) & (c["counts"] % rows == 1)).any()
                   for c in cases), rows
    xcd = [c for c in cases if c["F"] > 16]
    assert any(hist_xcd_chunks(c) % 8 != 0 for c in xcd)   # octet tail
    assert any(hist_xcd_chunks(c, 512) % 8 != 0 for c in xcd)
    assert any(len(c["counts"]) >= 512 for c in xcd)       # xcd_rows switch
    assert any(int(c["counts"].max()) > 16384 for c in cases)
    return cases


# ---------------------------------------------------------------------------
# split scan
# ---------------------------------------------------------------------------
def _score(G, H, lam, alpha):
    if alpha > 0:
        t = abs(G) - alpha
        G = math.copysign(t, G) if t > 0 else 0.0
    d = H + lam
    return G * G / d if d > 0 else 0.0


def _weight(G, H, lam, alpha):
    if alpha > 0:
        t = abs(G) - alpha
        G = math.copysign(t, G) if t > 0 else 0.0
    d = H + lam
    return -G / d if d > 0 else 0.0


def split_gain_table(case, k):
    """Every valid candidate of node k as (gain, default_left, f, b), in
    plain Python floats and ints. Used for the generators' self-checks."""
    hist = case["hist"][k].tolist()
    pgq, phq = int(case["parent_g"][k]), int(case["parent_h"][k])
    inv_g, inv_h = 1.0 / case["scale_g"], 1.0 / case["scale_h"]
    lam, alpha = case["reg_lambda"], case["reg_alpha"]
    gamma, mcw = case["gamma"], case["mcw"]
    Gp, Hp = float(pgq) * inv_g, float(phq) * inv_h
    ps = _score(Gp, Hp, lam, alpha)
    out = []
    for f, nb in enumerate(case["feat_bins"].tolist()):
        if case["allowed"] is not None and not int(case["allowed"][k, f]):
            continue
        c = 0 if case["monotone"] is None else int(case["monotone"][f])
        gt = sum(x[0] for x in hist[f])
        ht = sum(x[1] for x in hist[f])
        Gm, Hm = Gp - float(gt) * inv_g, Hp - float(ht) * inv_h
        gl_q = hl_q = 0
        for b in range(len(hist[f])):
            gl_q += hist[f][b][0]
            hl_q += hist[f][b][1]
            if b >= nb - 1:
                continue
            for dl in (1, 0):
                gl, hl = float(gl_q) * inv_g, float(hl_q) * inv_h
                if dl:
                    gl, hl = gl + Gm, hl + Hm
                gr, hr = Gp - gl, Hp - hl
                if hl < mcw or hr < mcw:
                    continue
                if c:
                    lo, up = (float(x) for x in case["bounds"][k])
                    wl = min(max(_weight(gl, hl, lam, alpha), lo), up)
                    wr = min(max(_weight(gr, hr, lam, alpha), lo), up)
                    if (wl > wr) if c > 0 else (wl < wr):
                        continue
                gain = 0.5 * (_score(gl, hl, lam, alpha)
                              + _score(gr, hr, lam, alpha) - ps) - gamma
                out.append((gain, dl, f, b))
    return out


_SPLIT_PARAMS = (  # (lambda, alpha, gamma, mcw)
    (1.0, 0.0, 0.0, 1.0), (0.0, 0.3, 0.05, 0.0), (3.5, 0.0, 0.05, 5.0),
    (0.0, 0.0, 0.0, 0.0), (1.0, 0.3, 0.0, 5.0), (3.5, 0.3, 0.05, 1.0),
)


def _feat_bins(F, B, mixed):
    if not mixed or F < 3:
        return np.full(F, B, np.int32)
    cyc = (B, 2, 1, 0, max(2, B // 2), B)
    return np.asarray([min(B, cyc[f % len(cyc)]) for f in range(F)], np.int32)


def _split_case(name, K, F, B, seed, params, mixed=True, mono=False,
                allowed=False, edge=None, rows=48):
    rng = np.random.RandomState(seed)
    fb = _feat_bins(F, B, mixed and edge is None)
    n = K * rows
    node = np.repeat(np.arange(K), rows)
    bins = np.zeros((n, F), np.int64)
    miss = rng.rand(n, F) < 0.15
    for f in range(F):
        bins[:, f] = rng.randint(0, max(int(fb[f]), 1), n)
    if edge == "no_missing":
        miss[:] = False
    if edge == "empty_bins":
        bins = bins // 3 * 3
    if edge == "dup_feature":
        bins[:, 1], miss[:, 1], fb[1] = bins[:, 0], miss[:, 0], fb[0]
    g = rng.uniform(-0.7310586, 0.7310586, n)
    h = rng.uniform(0.02, 0.19661193, n)
    if edge == "dup_feature":  # the duplicated column carries the signal
        g = np.where(bins[:, 0] < fb[0] // 2, -1.0, 1.0) * np.abs(g)
    gq =np.round(g * SCALE_G).astype(np.int64)
    hq = np.round(h * SCALE_H).astype(np.int64)
    hist = np.zeros((K, F, B, 2), np.int64)
    for f in range(F):
        keep = ~miss[:, f]
        np.add.at(hist[:, f, :, 0], (node[keep], bins[keep, f]), gq[keep])
        np.add.at(hist[:, f, :, 1], (node[keep], bins[keep, f]), hq[keep])
    lam, alpha, gamma, mcw = params
    if edge == "no_valid_split":
        mcw = 1e6  # larger than any child's hessian sum
    case = {
        "id": name, "K": K, "F": F, "B": B, "edge": edge,
        "hist": torch.from_numpy(hist),
        "parent_g": torch.from_numpy(np.bincount(node, gq, K).astype(np.int64)),
        "parent_h": torch.from_numpy(np.bincount(node, hq, K).astype(np.int64)),
        "feat_bins": torch.from_numpy(fb),
        "scale_g": SCALE_G, "scale_h": SCALE_H,
        "reg_lambda": lam, "reg_alpha": alpha, "gamma": gamma, "mcw": mcw,
        "monotone": None, "bounds": None, "allowed": None,
    }
    # exact integer parent sums (bincount went through float64 weights)
    for key, q in (("parent_g", gq), ("parent_h", hq)):
        exact = [int(q[node == k].sum()) for k in range(K)]
        assert case[key].tolist() == exact
    if mono:
        case["monotone"] = torch.tensor(
            [(1, -1, 0)[f % 3] for f in range(F)], dtype=torch.int8)
        ivals = ((-math.inf, math.inf), (-0.05, 0.05), (0.0, math.inf),
                 (-math.inf, -0.01), (0.02, 0.02))
        case["bounds"] = torch.tensor(
            [ivals[k % len(ivals)] for k in range(K)], dtype=torch.float64)
    if allowed:
        a = (rng.rand(K, F) < 0.6).astype(np.uint8)
        a[0, :] = 0  # node 0: every feature disallowed
        case["allowed"] = torch.from_numpy(a)
    case["n_tied"] = _split_edge_check(case)
    return case


def _split_edge_check(case):
    """Number of nodes where the named edge is genuinely present: at least
    two candidates share the maximum gain, or no candidate is valid."""
    edge = case["edge"]
    if edge is None:
        return 0
    hist, pg = case["hist"], case["parent_g"]
    if edge == "no_missing":
        assert torch.equal(hist[..., 0].sum(2), pg.view(-1, 1).expand(
            case["K"], case["F"]))
    if edge == "dup_feature":
        assert torch.equal(hist[:, 0], hist[:, 1])
    if edge == "empty_bins":
        used = hist.abs().sum((0, 1, 3)) != 0
        assert not used[1::3].any() and not used[2::3].any()
    hits = 0
    for k in range(case["K"]):
        tab = split_gain_table(case, k)
        if edge == "no_valid_split":
            assert not tab
            hits += 1
            continue
        assert tab
        best = max(t[0] for t in tab)
        top = [t for t in tab if t[0] == best]
        assert best > -1.0 and len(top) >= 2, (case["id"], k)
        if edge == "no_missing":    # both default-left passes tie
            assert {t[1] for t in top} == {0, 1}
        if edge == "dup_feature":   # lowest feature must win
            assert ({(t[1], t[3]) for t in top if t[2] == 0}
                    == {(t[1], t[3]) for t in top if t[2] == 1} != set())
        if edge == "empty_bins":    # lowest bin must win
            d0, f0 = max((t[1], -t[2]) for t in top)
            assert len({t[3] for t in top
                        if t[1] == d0 and t[2] == -f0}) >= 2
        hits += 1
    return hits


SPLIT_EDGES = ("no_missing", "dup_feature", "empty_bins", "no_valid_split")


@functools.lru_cache(maxsize=None)
def split_cases():
    Ks, Fs, Bs = (1, 3, 5, 67), (1, 3, 5, 17), (2, 5, 37, 64, 65, 255, 256)
    cases = []
    for i in range(28):
        K, B = Ks[i % 4], Bs[i % 7]
        F = Fs[(i + i // 4) % 4]
        mono, allowed = i % 3 == 1, i % 4 == 2
        tag = ("-mono" if mono else "") + ("-allow" if allowed else "")
        cases.append(_split_case(
            f"K{K}-F{F}-B{B}-p{i % 6}{tag}", K, F, B, 500 + i,
            _SPLIT_PARAMS[i % 6], mono=mono, allowed=allowed))
    shapes = ((3, 5, 37), (5, 3, 256), (1, 17, 65))
    for e, edge in enumerate(SPLIT_EDGES):
        for s, (K, F, B) in enumerate(shapes):
            p = _SPLIT_PARAMS[(2 * e + s) % 6]
            if edge != "no_valid_split":
                p = p[:3] + (min(p[3], 1.0),)  # keep candidates alive
            cases.append(_split_case(
                f"{edge}-K{K}-F{F}-B{B}", K, F, B, 700 + 10 * e + s, p,
                edge=edge))
    # many nodes whose two default-left passes tie exactly: an FMA-contracted
    # (GLq * inv + Gmiss) breaks about half of these ties the wrong way
    cases.append(_split_case("no_missing-K67-F3-B64", 67, 3, 64, 790,
                             _SPLIT_PARAMS[0], edge="no_missing"))
    cases = tuple(cases)
    assert len({c["id"] for c in cases}) == len(cases) == 41
    gen = cases[:28]
    assert {c["K"] for c in gen} == set(Ks) and {c["F"] for c in gen} == set(Fs)
    assert {c["B"] for c in gen} == set(Bs)
    assert {c["reg_lambda"] for c in gen} == {0.0, 1.0, 3.5}
    assert {c["mcw"] for c in gen} == {0.0, 1.0, 5.0}
    assert any(set(c["feat_bins"].tolist()) >= {0, 1, 2, c["B"]} for c in gen)
    assert any(c["monotone"] is not None and c["allowed"] is not None
               for c in gen)
    assert all(not c["allowed"][0].any() for c in gen
               if c["allowed"] is not None)
    for edge in SPLIT_EDGES:
        assert all(c["n_tied"] == c["K"] for c in cases if c["edge"] == edge)
    return cases


# ---------------------------------------------------------------------------
# partition
# ---------------------------------------------------------------------------
PART_COUNTS = (0, 1, 2047, 2048, 2049, 300)
PACKED_GAINS = (1.5, 1e-45, 0.0, -1.0, math.inf, math.nan)


def _gain_bits(g):
    return int(np.asarray(g, np.float32).view(np.int32))


def packed_ok(packed):
    """Rows of a packed [K, 6] split table that may move rows: finite f32
    gain > 0 and feature >= 0 (the trainer's host-side predicate)."""
    p = packed.numpy()
    gain = p[:, 0].astype(np.int32).view(np.float32)
    with np.errstate(invalid="ignore"):
        return (gain > 0) & (p[:, 1] >= 0) & np.isfinite(gain)


def _part_case(name, F, counts, seed, kinds, gains=None, feat_neg=()):
    """kinds[k]: 'L' all-left, 'R' all-right, anything else random."""
    rng = np.random.RandomState(seed)
    counts = np.asarray(counts, np.int64)
    K = len(counts)
    starts, n = _layout(counts, rng)
    b = rng.randint(2, MISSING, (n, F)).astype(np.uint8)
    b[rng.rand(n, F) < 0.10] = MISSING
    sf = rng.randint(0, F, K).astype(np.int32)
    sb = rng.randint(40, 215, K).astype(np.int32)
    dl = rng.randint(0, 2, K).astype(np.uint8)
    for k in range(K):
        kind = kinds[k % len(kinds)]
        if kind == "L":
            sb[k], dl[k] = 254, 1
        elif kind == "R":
            sb[k], dl[k] = 1, 0   # below every value; missing goes right
    ridx = rng.permutation(n).astype(np.int32)
    gseg = rng.randint(-(2**30), 2**30, (n, 2)).astype(np.int32)
    case = {
        "id": name, "F": F, "K": K, "n": n,
        "bins": padded_bins(b), "ridx": torch.from_numpy(ridx),
        "starts": torch.from_numpy(starts), "counts": torch.from_numpy(counts),
        "split_feat": torch.from_numpy(sf), "split_bin": torch.from_numpy(sb),
        "default_left": torch.from_numpy(dl), "gseg": torch.from_numpy(gseg),
    }
    if gains is not None:
        feat = sf.astype(np.int64)
        feat[list(feat_neg)] = -1
        packed = np.zeros((K, 6), np.int64)
        packed[:, 0] = [_gain_bits(gains[k % len(gains)]) for k in range(K)]
        packed[:, 1], packed[:, 2], packed[:, 3] = feat, sb, dl
        packed[:, 4:] = rng.randint(-(2**40), 2**40, (K, 2))
        case["packed"] = torch.from_numpy(packed)
    # self-checks
    for k in range(K):
        rows = ridx[starts[k]:starts[k] + counts[k]]
        col = b[rows, sf[k]]
        kind = kinds[k % len(kinds)]
        if kind in "LR" and counts[k] > 0:
            assert counts[k] < 100 or (col == MISSING).any()
            left = np.where(col == MISSING, dl[k] != 0, col <= sb[k])
            assert left.all() if kind == "L" else not left.any()
    return case


@functools.lru_cache(maxsize=None)
def partition_cases():
    cases = []
    for F in (2, 17):
        for v, kinds in enumerate(("xxLRxx", "xxRxLx")):
            cases.append(_part_case(f"F{F}-v{v}", F, PART_COUNTS,
                                    900 + 10 * F + v, kinds))
    big = _part_case("F2-big600k", 2, (600_000,), 990, "x")
    assert -(-600_000 // PART_CHUNK) > 256  # second pass of the prefix loop
    cases.append(big)
    assert len(cases) == 5
    for c in cases[:4]:
        assert c["counts"].tolist() == list(PART_COUNTS)
        assert c["bins"].stride(0) % 16 == 0 and c["starts"][0] > 0
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def packed_cases():
    """Device-planned partition inputs: K in {1, 6, 1500} plus the
    600 000-row node (more than 256 chunks in device-limit mode)."""
    g = PACKED_GAINS
    rng = np.random.RandomState(77)
    cases = [
        _part_case("packed-K1", 17, (777,), 1001, "x", gains=(1.5,)),
        _part_case("packed-K1-leaf", 2, (300,), 1002, "x", gains=(-1.0,)),
        _part_case("packed-K6-v0", 17, PART_COUNTS, 1003, "xxLRxx",
                   gains=(g[2], g[0], g[1], g[0], g[0], g[4]), feat_neg=(5,)),
        _part_case("packed-K6-v1", 2, PART_COUNTS, 1004, "xxRxLx",
                   gains=(g[0], g[5], g[0], g[3], g[1], g[0]), feat_neg=(2,)),
        _part_case("packed-K1500", 17, rng.randint(1, 4, 1500), 1005, "xxxLR",
                   gains=g, feat_neg=range(0, 1500, 12)),
        _part_case("packed-big600k", 2, (600_000,), 1006, "x", gains=(1.5,)),
    ]
    seen = set()
    for c in cases:
        ok = packed_ok(c["packed"])
        p = c["packed"].numpy()
        gain = p[:, 0].astype(np.int32).view(np.float32)
        seen |= {_gain_bits(x) for x in gain}
        # only finite gain > 0 with feature >= 0 may move
        assert not ok[~np.isfinite(gain)].any() and not ok[p[:, 1] < 0].any()
    assert seen == {_gain_bits(x) for x in g}
    k1500 = cases[4]
    assert k1500["K"] > 1024 and int(k1500["counts"].max()) <= 3
    p = k1500["packed"].numpy()
    pos = p[:, 0].astype(np.int32).view(np.float32) > 0
    assert (pos & (p[:, 1] < 0)).any()  # feature -1 with a positive gain
    for c in cases[2:4]:                # big segments split and unsplit
        ok = packed_ok(c["packed"])
        assert ok.any() and not ok.all()
    return tuple(cases)


# ---------------------------------------------------------------------------
# smaller ops
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bin_matrix_cases():
    inf, nan = math.inf, math.nan
    cuts = [[-1.0, 0.0, 0.5, 2.0], [], [0.25], [-3.0, -2.5, 1e30]]
    vals = np.array([
        [-1.0, -1.0, 0.25, -3.0], [0.0, 0.0, 0.2499999, -2.5],
        [0.5, nan, nan, 1e30], [2.0, inf, inf, inf],
        [-inf, -inf, -inf, -inf], [nan, 5.0, 0.2500001, nan],
        [inf, 0.0, 0.0, 3e38], [1.9999999, 1.0, 1.0, -2.9999998],
    ], np.float32)
    cases = [_bin_case("handmade", vals, cuts)]
    rng = np.random.RandomState(31)
    for name, n, F, ncut in (("F17-n1000", 1000, 17, None),
                             ("F70x255-n300", 300, 70, 255)):
        cuts = [np.unique(rng.randn(ncut or rng.randint(0, 40))
                          .astype(np.float32)) for _ in range(F)]
        if ncut:
            cuts = [np.sort(rng.permutation(4096)[:ncut]
                            .astype(np.float32)) / 64 - 32 for _ in range(F)]
        v = (rng.randn(n, F) * (12 if ncut else 1)).astype(np.float32)
        for f in range(F):  # a third of the values sit exactly on a cut
            if len(cuts[f]):
                hit = rng.rand(n) < 0.33
                v[hit, f] = rng.choice(cuts[f], int(hit.sum()))
        v[rng.rand(n, F) < 0.05] = np.nan
        v[rng.rand(n, F) < 0.01] = np.inf
        v[rng.rand(n, F) < 0.01] = -np.inf
        cases.append(_bin_case(name, v, cuts))
    hm, big = cases[0], cases[2]
    assert {0, 1} <= set(np.diff(hm["cut_ptr"].numpy()).tolist())
    assert big["cuts_flat"].numel() * 4 > 64 * 1024  # the non-LDS template
    assert cases[1]["values"].shape == (1000, 17)
    return tuple(cases)


def _bin_case(name, values, cuts):
    ptr = np.concatenate([[0], np.cumsum([len(c) for c in cuts])])
    flat = np.concatenate([np.asarray(c, np.float32) for c in cuts])
    v = np.asarray(values, np.float32)
    on_cut = sum(int(np.isin(v[:, f], cuts[f]).sum()) for f in range(len(cuts)))
    assert on_cut > 0 and np.isnan(v).any()
    assert np.isposinf(v).any() and np.isneginf(v).any()
    return {"id": name, "values": torch.from_numpy(v),
            "cuts_flat": torch.from_numpy(flat.astype(np.float32)),
            "cut_ptr": torch.from_numpy(ptr.astype(np.int64))}


@functools.lru_cache(maxsize=None)
def quantize_cases():
    n = 257
    half = (np.arange(n, dtype=np.float32) - 128.0) + 0.5   # exact k + .5
    gp = np.stack([half, half[::-1] * 3.0], axis=1).astype(np.float32)
    gp[5], gp[6] = (2.0**30, -(2.0**30)), (-(2.0**30), 2.0**30)
    assert (np.modf(gp[:5])[0] != 0).all() and gp.shape == (257, 2)
    rng = np.random.RandomState(41)
    g2 = np.stack([rng.uniform(-0.7310586, 0.7310586, n),
                   rng.uniform(0, 0.19661193, n)], axis=1).astype(np.float32)
    g2[0] = (0.7310586, 0.19661193)
    g2[1] = (-0.7310586, 0.0)
    # an all-zero gradient column with the scales the trainer derives from
    # the column maxima: the scale of a zero maximum must stay finite
    from xgboost_ray_amd.engine.trainer import _quant_scale

    g3 = g2.copy()
    g3[:, 0] = 0.0
    g3[1, 0] = -0.0
    zero_scales = [_quant_scale(float(np.abs(g3[:, j]).max()))
                   for j in (0, 1)]
    assert not g3[:, 0].any() and g3[:, 1].any()
    return (
        {"id": "half-even-2^30", "gpair": torch.from_numpy(gp),
         "scale_g": 1.0, "scale_h": 1.0},
        {"id": "production-scales", "gpair": torch.from_numpy(g2),
         "scale_g": SCALE_G, "scale_h": SCALE_H},
        {"id": "zero-g-column", "gpair": torch.from_numpy(g3),
         "scale_g": zero_scales[0], "scale_h": zero_scales[1]},
    )


@functools.lru_cache(maxsize=None)
def margin_cases():
    """update_margins with two ping-pong row-index buffers and a per-leaf
    parity; ``ridx_sel`` is what a single-buffer oracle should read."""
    rng = np.random.RandomState(51)
    counts = np.array([0, 1, 2047, 2049], np.int64)
    starts, n = _layout(counts, rng)
    perm = rng.permutation(n).astype(np.int32)
    parity = np.array([1, 0, 1, 0], np.int64)
    # each buffer holds the true rows only where its parity selects it and
    # a shifted (wrong) permutation elsewhere
    ra, rb = np.roll(perm, 1).copy(), np.roll(perm, 2).copy()
    for s, c, p in zip(starts, counts, parity):
        (rb if p else ra)[s:s + c] = perm[s:s + c]
    assert {0, 1} == set(parity[counts > 0].tolist())
    return ({
        "id": "parity", "n": n, "ridx_a": torch.from_numpy(ra),
        "ridx_b": torch.from_numpy(rb), "ridx_sel": torch.from_numpy(perm),
        "starts": torch.from_numpy(starts), "counts": torch.from_numpy(counts),
        "parity": torch.from_numpy(parity),
        "leaf_values": rng.randn(4).astype(np.float32),
        "margin": torch.from_numpy(rng.randn(n).astype(np.float32)),
    },)


# ---------------------------------------------------------------------------
# the CPU oracle applied to a case (shared by the CPU and the GPU tests)
# ---------------------------------------------------------------------------
def oracle_hist(c, **kw):
    from xgboost_ray_amd.ops import cpu as cpu_ops

    return cpu_ops.build_histogram(c["bins"], c["gq"], c["ridx"], c["starts"],
                                   c["counts"], c["n_bins"], **kw)


def oracle_splits(c):
    from xgboost_ray_amd.ops import cpu as cpu_ops

    return cpu_ops.find_splits(
        c["hist"], c["parent_g"], c["parent_h"], c["feat_bins"], c["scale_g"],
        c["scale_h"], c["reg_lambda"], c["reg_alpha"], c["gamma"], c["mcw"],
        monotone=c["monotone"], bounds=c["bounds"], allowed=c["allowed"])


def oracle_partition(c, sel=None, with_gseg=True):
    """Partition the segments ``sel`` (default: all); always a 3-tuple
    (ridx, left_counts, gseg or None)."""
    from xgboost_ray_amd.ops import cpu as cpu_ops

    sel = list(range(c["K"])) if sel is None else list(sel)
    ix = torch.as_tensor(sel, dtype=torch.int64)
    args = (c["bins"], c["ridx"], c["starts"][ix], c["counts"][ix],
            c["split_feat"][ix], c["split_bin"][ix], c["default_left"][ix])
    if with_gseg:
        return cpu_ops.partition_rows(*args, gpair_seg=c["gseg"])
    return cpu_ops.partition_rows(*args) + (None,)


def oracle_margins(c):
    from xgboost_ray_amd.ops import cpu as cpu_ops

    return cpu_ops.update_margins(c["margin"].clone(), c["ridx_sel"],
                                  c["starts"], c["counts"], c["leaf_values"])


def oracle_bins(c):
    from xgboost_ray_amd.ops import cpu as cpu_ops

    return cpu_ops.bin_matrix(c["values"], c["cuts_flat"], c["cut_ptr"])


def oracle_quantize(c):
    from xgboost_ray_amd.ops import cpu as cpu_ops

    return cpu_ops.quantize_gpair(c["gpair"], c["scale_g"], c["scale_h"])
