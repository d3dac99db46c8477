"""Hand-built forests and oracles for the path-form TreeSHAP tests.

The trees are built from explicit or seeded-random STRUCTURE, not from
training, so the edge cases are certain to occur: a feature split two and
three times on one path (interval merge, ``miss_ok`` AND), both default
directions, a subtree of cover 0, a root-only tree, a leaf of value 0,
and rows holding NaN, +-inf and values exactly on a threshold.
"""

import math
from itertools import combinations

import numpy as np

from xgboost_ray_amd.booster import Tree, _fill_node_means, _tree_shap

# d: largest |ops.cpu.tree_shap - _tree_shap| over the whole case set
# (every CASES entry, all its 300 rows, wherever the recursion is finite),
# measured on the CPU: 1.7763568394002505e-15, 8 ulp of 1.0, on
# contributions of magnitude <= 4. Both are float64 formulations of the
# same sum and differ by rounding only; test_tree_shap_cpu re-measures it
# and fails if it ever exceeds this constant.
SHAP_D = 1.7763568394002505e-15
# GPU kernel vs ops.cpu: the same algorithm in float64, differing at most
# by FMA contraction and summation grouping. The margin of 64 allows the
# kernel to reassociate where numpy does not; the bound (1.1e-13) stays 8
# orders of magnitude under the 1e-5 of the brute-force check.
SHAP_GPU_TOL = 64 * SHAP_D
# brute-force Shapley comparisons keep the engine test's bound
BRUTE_TOL = 1e-5


def inter_cpu_tol(F):
    """Path-form interactions vs Booster.predict_interactions, both on
    the CPU: an off-diagonal entry is half the difference of two
    recursion passes, each within d of its path-form counterpart, so it
    moves by at most d; a diagonal entry is a contribution (d) minus F
    off-diagonal entries (F * d)."""
    return (F + 1) * SHAP_D


# sum(contribs) + bias vs the tree-walk margin: the sum telescopes over
# <= 64 paths of <= 5 elements with weights <= 1 and |value| <= 4; each
# term carries a few ulp, 64 * 5 * 8 ulp(4) = 2.3e-12 bounds the total.
ADDITIVITY_TOL = 64 * 5 * 8 * 8.9e-16

N_ROWS = 300  # not a multiple of any block or chunk size


def L(value, cover):
    return ("leaf", float(value), float(cover))


def N(feat, thr, default_left, left, right, cover=None):
    return ("node", int(feat), float(thr), int(default_left), left, right,
            cover)


def build_tree(spec):
    """Nested L/N spec -> Tree (children allocated in pairs, covers
    summed bottom-up unless a node pins its own)."""
    feat, thr, left, dl, value, cover, parent = [], [], [], [], [], [], []

    def new(par):
        for a, v in ((feat, -1), (thr, 0.0), (left, -1), (dl, 0),
                     (value, 0.0), (cover, 0.0), (parent, par)):
            a.append(v)
        return len(feat) - 1

    def fill(nid, s):
        if s[0] == "leaf":
            value[nid], cover[nid] = s[1], s[2]
            return
        _, f, th, d, ls, rs, cv = s
        lid = new(nid)
        rid = new(nid)
        feat[nid], thr[nid], dl[nid], left[nid] = f, th, d, lid
        fill(lid, ls)
        fill(rid, rs)
        cover[nid] = cover[lid] + cover[rid] if cv is None else cv

    fill(new(-1), spec)
    n = len(feat)
    return Tree(
        feat=np.asarray(feat, np.int32), thr=np.asarray(thr, np.float32),
        left=np.asarray(left, np.int32),
        default_left=np.asarray(dl, np.uint8),
        value=np.asarray(value, np.float32), gain=np.zeros(n, np.float32),
        cover=np.asarray(cover, np.float32),
        parent=np.asarray(parent, np.int32),
    )


GRID = np.round(np.arange(0.0, 1.01, 0.1), 1).astype(np.float32)


def random_spec(rng, F, depth, p_leaf=0.2, bounds=None):
    """Random subtree. Thresholds stay strictly inside the interval the
    path already allows, so no path is unreachable (trained trees have
    none either)."""
    bounds = bounds or {}
    f = rng.randint(F)
    lo, hi = bounds.get(f, (-np.inf, np.inf))
    cand = GRID[(GRID > lo) & (GRID < hi)][1:-1]
    if depth == 0 or rng.rand() < p_leaf or len(cand) == 0:
        return L(np.float32(rng.randn()), float(rng.randint(1, 20)))
    thr = cand[rng.randint(len(cand))]
    return N(f, thr, rng.randint(2),
             random_spec(rng, F, depth - 1, p_leaf, {**bounds, f: (lo, thr)}),
             random_spec(rng, F, depth - 1, p_leaf, {**bounds, f: (thr, hi)}))


def random_forest(seed, F, depth, n_trees, p_leaf=0.2):
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n_trees):
        spec = random_spec(rng, F, depth, p_leaf)
        if spec[0] == "leaf":  # keep the root a split
            spec = N(rng.randint(F), 0.5, 1, spec, L(rng.randn(), 3.0))
        out.append(build_tree(spec))
    return out


def rows(F, n=N_ROWS, seed=0):
    """Grid values (so x == thr happens), with NaN and +-inf sprinkled."""
    rng = np.random.RandomState(1000 + seed)
    X = GRID[rng.randint(0, len(GRID), size=(n, F))].copy()
    X[rng.rand(n, F) < 0.15] = np.nan
    X[rng.rand(n, F) < 0.04] = np.inf
    X[rng.rand(n, F) < 0.04] = -np.inf
    X[0] = 0.5  # a row sitting exactly on thresholds
    X[1] = np.nan
    X[2] = np.inf
    X[3] = -np.inf
    return np.ascontiguousarray(X, np.float32)


# feature 0 split three times on the path root -> L -> R -> ..., twice on
# root -> R -> R; both default directions; one leaf of value 0
REPEAT = N(0, 0.5, 1,
           N(0, 0.2, 0,
             L(1.0, 3),
             N(0, 0.4, 1, L(-2.0, 2),
               N(1, 0.5, 0, L(0.5, 1), L(3.0, 4)))),
           N(2, 0.7, 1, L(0.0, 5),
             N(0, 0.8, 0, L(-1.5, 2), L(2.5, 1))))
ROOT_ONLY = L(0.75, 10)
# the left subtree has cover 0 throughout (its parent keeps cover 6)
ZERO_COVER = N(1, 0.4, 0,
               N(2, 0.3, 1, L(1.0, 0), L(2.0, 0)),
               N(0, 0.6, 1, L(-1.0, 4), L(0.5, 2)), cover=6.0)
# a leaf of cover 0: rows that reach it keep the recursion finite
ZERO_LEAF = N(1, 0.4, 0, L(1.0, 0),
              N(0, 0.6, 1, L(-1.0, 4), N(2, 0.5, 0, L(0.5, 2), L(1.5, 3))))


class Case:
    def __init__(self, name, trees, F, groups=None, scale=1.0,
                 brute=True):
        self.name, self.trees, self.F = name, trees, F
        self.groups = groups or [0] * len(trees)
        self.n_groups = max(self.groups) + 1
        self.scale = scale
        self.brute = brute  # F <= 5: 2^F subsets are enumerable
        self.X = rows(F, seed=len(name))

    def __repr__(self):
        return self.name


def _cases():
    edge = [build_tree(REPEAT), build_tree(ROOT_ONLY)]
    return [
        Case("edge", edge, 3),
        Case("zero_cover", [build_tree(ZERO_COVER)] + edge, 3),
        Case("zero_leaf", [build_tree(ZERO_LEAF)] + edge, 3),
        Case("edge_scaled", edge + random_forest(3, 3, 3, 2), 3,
             scale=0.5),
        Case("random_f5", random_forest(11, 5, 4, 6), 5),
        Case("random_f4_3groups", random_forest(12, 4, 3, 6), 4,
             groups=[0, 1, 2, 0, 1, 2]),
        Case("repeat_deep_f2", random_forest(13, 2, 5, 4, p_leaf=0.1), 2),
    ]


CASES = _cases()
BRUTE_CASES = [c for c in CASES if c.brute]
# a wider forest for the kernel test only (no brute force at F = 9)
WIDE = Case("wide_f9_d6", random_forest(21, 9, 6, 10, p_leaf=0.1), 9,
            brute=False)


def chain_tree(n_features):
    """A right-leaning chain splitting once on each of n_features."""
    spec = L(1.0, 1)
    for f in range(n_features - 1, -1, -1):
        spec = N(f, 0.5, f % 2, L(0.1 * f - 1.0, 1), spec)
    return build_tree(spec)


def case_booster(case):
    """The case's forest as a Booster (scale 1/k <=> num_parallel_tree k)."""
    from xgboost_ray_amd.booster import Booster

    params = {"objective": "reg:squarederror", "base_score": 0.25,
              "num_feature": case.F}
    if case.n_groups > 1:
        params.update(objective="multi:softprob", num_class=case.n_groups)
    if case.scale != 1.0:
        params["num_parallel_tree"] = int(round(1.0 / case.scale))
    return Booster(params, list(case.trees), list(case.groups))


def case_paths(case):
    from xgboost_ray_amd.ops import cpu

    return cpu.shap_paths(case.trees, case.scale, case.groups)


def recursion_contribs(case, X):
    """[n, n_groups, F+1] from booster._tree_shap (bias column filled)."""
    out = np.zeros((len(X), case.n_groups, case.F + 1), np.float64)
    for t, g in zip(case.trees, case.groups):
        mean_val = np.zeros(t.num_nodes)
        cover = t.cover.astype(np.float64)
        _fill_node_means(t, mean_val, cover)
        for i in range(len(X)):
            _tree_shap(t, X[i], mean_val, cover, out[i, g], case.scale)
    return out


def margins(case, X):
    """[n, n_groups] plain tree-walk sums (float64)."""
    out = np.zeros((len(X), case.n_groups), np.float64)
    for t, g in zip(case.trees, case.groups):
        for i, x in enumerate(X):
            nid = 0
            while t.feat[nid] >= 0:
                fv = x[t.feat[nid]]
                goleft = (t.default_left[nid] if np.isnan(fv)
                          else fv < t.thr[nid])
                nid = int(t.left[nid]) + (0 if goleft else 1)
            out[i, g] += float(t.value[nid] * case.scale)
    return out


def _cond_exp(t, x, S):
    def rec(nid):
        f = t.feat[nid]
        if f < 0:
            return float(t.value[nid])
        l, r = int(t.left[nid]), int(t.left[nid]) + 1
        if f in S:
            fv = x[f]
            if np.isnan(fv):
                return rec(l if t.default_left[nid] else r)
            return rec(l if fv < t.thr[nid] else r)
        cl, cr = float(t.cover[l]), float(t.cover[r])
        tot = cl + cr if cl + cr > 0 else 1.0
        return (cl * rec(l) + cr * rec(r)) / tot

    return rec(0)


def brute_force_contribs(case, X):
    """Shapley values by enumeration: cover-weighted conditional
    expectation over all 2^F subsets. [n, n_groups, F] (no bias)."""
    F = case.F
    out = np.zeros((len(X), case.n_groups, F), np.float64)
    for i, x in enumerate(X):
        for t, g in zip(case.trees, case.groups):
            val = {}
            for k in range(F + 1):
                for S in combinations(range(F), k):
                    val[frozenset(S)] = _cond_exp(t, x, set(S))
            for f in range(F):
                others = [j for j in range(F) if j != f]
                for k in range(F):
                    wgt = (math.factorial(k) * math.factorial(F - k - 1)
                           / math.factorial(F))
                    for S in combinations(others, k):
                        s = frozenset(S)
                        out[i, g, f] += wgt * case.scale * (
                            val[s | {f}] - val[s])
    return out
