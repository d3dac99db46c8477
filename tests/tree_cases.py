"""Cases and the harness of the tree-growing oracle tests.

``tests/test_tree_oracle.py`` (CPU engine) and
``tests/test_tree_oracle_gpu.py`` (every device path) both run the cases
below through ``BoostingEngine`` and hold the result against
``tests/tree_oracle.py``. The sampling draws are not the oracle's business
(they have their own tests): they are recorded from the engine by wrapping
methods on the instance and handed to the oracle. Every comparison is exact.
"""

import dataclasses
import functools
from dataclasses import dataclass, field

import numpy as np
import torch

from tests import tree_oracle as to

ROUNDS = 3

# every switch the engine-level tests clear, and every histogram knob
SWITCHES = ("RXGB_ONE_SYNC", "RXGB_ROW_FINISH", "RXGB_DEPTH_STEP",
            "RXGB_FUSED_GLUE", "RXGB_TREE_ENQUEUE", "RXGB_HIST_FB",
            "RXGB_HIST_MULTIFB", "RXGB_HIST_MODE", "RXGB_HIST_XCD_ROWS",
            "RXGB_HIST_DIRECT_ROWS", "RXGB_HIST_MULTIFB_R",
            "RXGB_HIST_XCD_THREADS", "RXGB_FUSED_GRAD")

# special columns of the feature matrix
COL_INT, COL_SRC, COL_DUP, COL_CONST, COL_ALLNAN, COL_NAN10, COL_NAN30 = (
    2, 3, 4, 5, 6, 7, 8)


@functools.lru_cache(maxsize=None)
def data(n, F):
    """float32 normal features; one column rounded to integers (heavy ties,
    values sitting on cuts), one duplicated (the lowest feature wins the
    tie), one constant (one bin), one all-NaN, two with 10 % / 30 % NaN."""
    assert F >= 12
    rng = np.random.RandomState(1000 * F + n)
    X = rng.randn(n, F).astype(np.float32)
    X[:, COL_INT] = np.rint(2.0 * X[:, COL_INT])
    X[:, COL_DUP] = X[:, COL_SRC]
    X[:, COL_CONST] = 1.5
    X[:, COL_ALLNAN] = np.nan
    X[rng.rand(n) < 0.10, COL_NAN10] = np.nan
    X[rng.rand(n) < 0.30, COL_NAN30] = np.nan
    z = (X[:, 0] - 0.5 * X[:, 1] + 0.3 * X[:, COL_INT] + 0.8 * X[:, COL_SRC]
         + 0.7 * np.nan_to_num(X[:, COL_NAN10])
         + 0.5 * np.nan_to_num(X[:, COL_NAN30])
         + 0.9 * np.isnan(X[:, COL_NAN30]) + 0.4 * X[:, F - 1]
         + 0.3 * rng.randn(n))
    out = {
        "X": X,
        "y_bin": (z > 0).astype(np.float32),
        "y_reg": z.astype(np.float32),
        "y_cls": np.digitize(z, [-0.7, 0.7]).astype(np.float32),
        "w": rng.uniform(0.5, 2.0, n).astype(np.float32),
    }
    for v in out.values():
        v.setflags(write=False)
    return out


# ---------------------------------------------------------------------------
# gradients: numpy float64 from the margin, cast to float32
# ---------------------------------------------------------------------------
def _logistic(m, y):
    p = 1.0 / (1.0 + np.exp(-m.astype(np.float64)))
    return (p - y).astype(np.float32), (p * (1.0 - p)).astype(np.float32)


def _softmax3(m, y):
    m = m.astype(np.float64)
    e = np.exp(m - m.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    onehot = np.eye(3)[y.astype(np.int64)]
    return ((p - onehot).astype(np.float32),
            (2.0 * p * (1.0 - p)).astype(np.float32))


def _squared(m, y):
    g = (m.astype(np.float64) - y).astype(np.float32)
    return g, np.ones(m.shape, np.float32)


def _zero_g(m, y):
    return np.zeros(m.shape, np.float32), np.ones(m.shape, np.float32)


def _zero_h(m, y):
    return _logistic(m, y)[0], np.zeros(m.shape, np.float32)


def _zero_gh(m, y):
    return np.zeros(m.shape, np.float32), np.zeros(m.shape, np.float32)


# objective name -> (gradient function or None for the built-in, label key)
OBJECTIVES = {
    "logistic": (_logistic, "y_bin"),
    "softmax3": (_softmax3, "y_cls"),
    "squared": (_squared, "y_reg"),
    "zero_g": (_zero_g, "y_bin"),
    "zero_h": (_zero_h, "y_bin"),
    "zero_gh": (_zero_gh, "y_bin"),
    # built-in reg:squarederror with row weights: g = (m - y) * w and
    # h = 1 * w in float32, every operation correctly rounded on its own
    "sqerr_w": (None, "y_reg"),
}


@dataclass(frozen=True)
class Case:
    name: str
    params: dict = field(hash=False, compare=False)
    n: int = 3000
    F: int = 28
    max_bin: int = 64
    objective: str = "logistic"
    # the whole-tree enqueue may take the tree (no per-depth host input,
    # depth <= 10); otherwise the default switches must give "per_depth"
    enqueue_ok: bool = True


def _mono(F):
    m = [0] * F
    m[0], m[1], m[2], m[COL_NAN10] = 1, -1, 1, -1
    return m


def _inter(F):
    return [[0, 1, 2, 3, 4, COL_NAN10], [2, 3, COL_NAN30, 9, 10, 11],
            [0, COL_NAN30] + list(range(11, F))]


def _cases(F):
    reg = {"reg_alpha": 0.5, "gamma": 0.5, "min_child_weight": 3,
           "max_delta_step": 0.4}
    # F = 28 (row stride 32, two 16-feature blocks) is where the whole-tree
    # enqueue exists; F = 12 is one block (single-block histogram) and
    # F = 70 has row stride 80 (legacy finish by default, parity buffers)
    enq = F == 28
    cs = [
        Case("plain-b64", {"max_depth": 6}),
        Case("plain-b256", {"max_depth": 6}, max_bin=256),
        Case("regularised", dict(reg, max_depth=6)),
        Case("tiny-n64-d8", {"max_depth": 8, "min_child_weight": 0.1}, n=64),
        Case("tiny-n3", {"max_depth": 6}, n=3),
        Case("tiny-n1", {"max_depth": 6}, n=1),
        Case("subsample-uniform", {"max_depth": 6, "subsample": 0.5}),
        Case("subsample-gradient",
             {"max_depth": 6, "subsample": 0.3,
              "sampling_method": "gradient_based"}),
        Case("colsample", {"max_depth": 6, "colsample_bytree": 0.5,
                           "colsample_bylevel": 0.5,
                           "colsample_bynode": 0.5}, enqueue_ok=False),
        Case("constrained",
             {"max_depth": 6, "monotone_constraints": _mono(F),
              "interaction_constraints": _inter(F)}, enqueue_ok=False),
        Case("multiclass", {"max_depth": 4, "num_class": 3},
             objective="softmax3"),
        Case("multiclass-forest",
             {"max_depth": 4, "num_class": 3, "num_parallel_tree": 2,
              "subsample": 0.5}, objective="softmax3"),
        Case("weighted-squarederror",
             {"max_depth": 6, "objective": "reg:squarederror"},
             objective="sqerr_w"),
        Case("deep", {"max_depth": 11, "reg_lambda": 0.1}, n=6000,
             objective="squared",
             enqueue_ok=False),
        Case("zero-g", {"max_depth": 6}, objective="zero_g"),
        Case("zero-h", {"max_depth": 6}, objective="zero_h"),
        Case("zero-gh", {"max_depth": 6}, objective="zero_gh"),
        Case("lossguide-leaves17",
             {"grow_policy": "lossguide", "max_leaves": 17, "max_depth": 0}),
        Case("lossguide-leaves9-d3",
             {"grow_policy": "lossguide", "max_leaves": 9, "max_depth": 3}),
        Case("lossguide-d4-gamma1",
             {"grow_policy": "lossguide", "max_leaves": 0, "max_depth": 4,
              "gamma": 1.0}),
    ]
    return {c.name: dataclasses.replace(
        c, F=F, enqueue_ok=c.enqueue_ok and enq) for c in cs}


_BY_F = {F: _cases(F) for F in (12, 28, 70)}
CASES = _BY_F[28]


def case_at(name, F=28):
    return _BY_F[F][name]


LOSSGUIDE = sorted(k for k, c in CASES.items()
                   if c.params.get("grow_policy") == "lossguide")
DEPTHWISE = sorted(k for k in CASES if k not in LOSSGUIDE)


def is_lossguide(case):
    return case.params.get("grow_policy") == "lossguide"


# ---------------------------------------------------------------------------
# the engine side
# ---------------------------------------------------------------------------
_DMS = {}


def matrix(case, device):
    """(BinnedMatrix on ``device``, host arrays for the oracle), cached."""
    key = (case.n, case.F, case.max_bin, case.objective, str(device))
    if key not in _DMS:
        from xgboost_ray_amd.engine.quantile import BinnedMatrix

        d = data(case.n, case.F)
        label = d[OBJECTIVES[case.objective][1]]
        weight = d["w"] if case.objective == "sqerr_w" else None
        dm = BinnedMatrix.build(
            torch.from_numpy(d["X"].copy()).to(device),
            label=torch.from_numpy(label.copy()).to(device),
            weight=None if weight is None
            else torch.from_numpy(weight.copy()).to(device),
            max_bin=case.max_bin)
        host = {
            "bins": np.ascontiguousarray(dm.bins.cpu().numpy()),
            "feat_bins": dm.cuts.feat_bins().cpu().numpy(),
            "cuts_flat": dm.cuts.cuts_flat.cpu().numpy().copy(),
            "cut_ptr": dm.cuts.cut_ptr.cpu().numpy().copy(),
            "n_bins": int(dm.cuts.max_bins),
        }
        _DMS[key] = (dm, host)
    return _DMS[key]


def _np(t):
    return None if t is None else t.detach().cpu().numpy().copy()


class Recorder:
    """Wraps the engine's sampling methods on the INSTANCE and keeps what
    they return, one record per grown tree."""

    def __init__(self, eng):
        self.trees = []
        eng._rec = self
        grow, rows = eng._grow_tree, eng._sample_rows
        feats, bynode, mvs = (eng._sample_features, eng._bynode_mask,
                              eng._mvs_sample)

        def grow_w(gpair, it, cls, ptree=0):
            self.trees.append({"it": it, "cls": cls, "ptree": ptree,
                               "rows": None, "tree_gate": None,
                               "level_gates": [], "node_gates": [],
                               "mvs_gpair": None})
            return grow(gpair, it, cls, ptree=ptree)

        def rows_w(it, cls):
            out = rows(it, cls)
            self.trees[-1]["rows"] = _np(out).astype(np.int64)
            return out

        def feats_w(it, cls, level=None):
            out = feats(it, cls, level=level)
            if out is not None:
                if level is None:
                    self.trees[-1]["tree_gate"] = _np(out).astype(bool)
                else:
                    lg = self.trees[-1]["level_gates"]
                    assert level == len(lg)
                    lg.append(_np(out).astype(bool))
            return out

        def bynode_w(KK, it, cls, depth):
            out = bynode(KK, it, cls, depth)
            ng = self.trees[-1]["node_gates"]
            assert depth == len(ng)
            ng.append(_np(out))
            return out

        def mvs_w(gpair, it, tree):
            out = mvs(gpair, it, tree)
            self.trees[-1]["mvs_gpair"] = _np(out)
            return out

        eng._grow_tree, eng._sample_rows = grow_w, rows_w
        eng._sample_features, eng._bynode_mask = feats_w, bynode_w
        eng._mvs_sample = mvs_w


@dataclass
class Run:
    eng: object
    draws: list          # Recorder.trees
    trees: list          # engine Tree objects, in growth order
    margins: list        # eng.margin before every round and after the last
    gpairs: list         # what the custom objective returned, per round
    paths: set
    pred_leaf: np.ndarray


def run_engine(case, device, rounds=ROUNDS):
    from xgboost_ray_amd.engine.trainer import BoostingEngine

    dm, _ = matrix(case, device)
    fn, label_key = OBJECTIVES[case.objective]
    y = data(case.n, case.F)[label_key]
    gpairs = []
    obj = None
    if fn is not None:
        def obj(preds, dtrain):
            g, h = fn(np.asarray(preds), y)
            gpairs.append((g.copy(), h.copy()))
            return g, h

    params = dict({"eta": 0.3, "max_bin": case.max_bin,
                   "tree_method": "gpu_hist" if str(device) != "cpu"
                   else "hist"}, **case.params)
    eng = BoostingEngine(params, dm, custom_objective=obj)
    rec = Recorder(eng)
    trees, margins, paths = [], [], set()
    for _ in range(rounds):
        margins.append(_np(eng.margin))
        trees += eng.update()
        paths.add(eng.last_tree_path)
    if eng.margin.is_cuda:
        torch.cuda.synchronize()
    margins.append(_np(eng.margin))
    leaf = eng.booster.predict(data(case.n, case.F)["X"], pred_leaf=True)
    return Run(eng, rec.trees, trees, margins, gpairs, paths,
               np.asarray(leaf))


# ---------------------------------------------------------------------------
# the oracle side
# ---------------------------------------------------------------------------
def oracle_params(case):
    p = case.params
    ic = p.get("interaction_constraints")
    return to.Params(
        eta=0.3, max_depth=int(p.get("max_depth", 6)),
        reg_lambda=float(p.get("reg_lambda", 1.0)),
        reg_alpha=float(p.get("reg_alpha", 0.0)),
        gamma=float(p.get("gamma", 0.0)),
        min_child_weight=float(p.get("min_child_weight", 1.0)),
        max_delta_step=float(p.get("max_delta_step", 0.0)),
        grow_policy=p.get("grow_policy", "depthwise"),
        max_leaves=int(p.get("max_leaves", 0)),
        monotone=p.get("monotone_constraints"),
        interaction_sets=None if ic is None
        else [frozenset(int(f) for f in g) for g in ic],
    )


@dataclass
class OracleRun:
    trees: list          # canonical tuples, in growth order
    leaf_ids: np.ndarray  # [n, trees] canonical leaf id of every row
    margins: list        # before every round and after the last
    gpairs: list         # the gradients it computed itself, per round
    draws: list


def run_oracle(case, host, draws, margin0, rounds=ROUNDS):
    """Grow ``rounds`` rounds from ``margin0`` with the recorded draws. The
    gradients of every round come from the oracle's OWN margin."""
    P = oracle_params(case)
    fn, label_key = OBJECTIVES[case.objective]
    d = data(case.n, case.F)
    y = d[label_key]
    n_class = int(case.params.get("num_class", 0)) or 1
    per_round = n_class * int(case.params.get("num_parallel_tree", 1))
    assert len(draws) == rounds * per_round
    lossguide = is_lossguide(case)
    margin = margin0.copy()
    assert margin.dtype == np.float32
    trees, leaf_ids, margins, gpairs = [], [], [], []
    it_draws = iter(draws)
    for it in range(rounds):
        margins.append(margin.copy())
        if fn is not None:
            g, h = fn(margin, y)
        else:
            g = (margin - y) * d["w"]
            h = np.float32(1.0) * d["w"]
            assert g.dtype == h.dtype == np.float32
        gpairs.append((g, h))
        for _ in range(per_round):
            dr = next(it_draws)
            assert dr["it"] == it
            cls = dr["cls"]
            gp = dr["mvs_gpair"]
            if gp is None:
                gp = np.stack([g, h], axis=-1)
                gp = gp if n_class == 1 else gp[:, cls, :]
            root = to.grow_tree(
                host["bins"], host["feat_bins"], host["cuts_flat"],
                host["cut_ptr"], host["n_bins"],
                np.ascontiguousarray(gp, np.float32), dr["rows"], P,
                tree_gate=dr["tree_gate"],
                level_gates=None if lossguide or not dr["level_gates"]
                else dr["level_gates"],
                node_gates=None if lossguide or not dr["node_gates"]
                else dr["node_gates"])
            to.add_margin(margin if n_class == 1 else margin[:, cls], root,
                          host["bins"])
            trees.append(to.canonical(root))
            leaf_ids.append(to.walk_binned(root, host["bins"]))
    margins.append(margin.copy())
    return OracleRun(trees, np.stack(leaf_ids, axis=1), margins, gpairs,
                     draws)


def same_draws(a, b):
    """The recorded draws of two runs are the same draws."""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x["it"], x["cls"], x["ptree"]) == (y["it"], y["cls"],
                                                   y["ptree"])
        for key in ("rows", "tree_gate", "mvs_gpair"):
            assert (x[key] is None) == (y[key] is None), key
            if x[key] is not None:
                np.testing.assert_array_equal(x[key], y[key], err_msg=key)
        for key in ("level_gates", "node_gates"):
            assert len(x[key]) == len(y[key]), key
            for p, q in zip(x[key], y[key]):
                np.testing.assert_array_equal(p, q, err_msg=key)


def compare(run, oracle):
    """The engine run against the oracle run: margins before every round
    (bitwise, first), the recorded gradients, every tree in canonical form,
    the final margins and the pred_leaf membership."""
    per_round = len(run.trees) // (len(run.margins) - 1)
    assert len(run.trees) == len(oracle.trees) > 0
    for r in range(len(run.margins) - 1):
        np.testing.assert_array_equal(
            run.margins[r].view(np.int32), oracle.margins[r].view(np.int32),
            err_msg=f"margin before round {r}")
        if run.gpairs:
            for j in (0, 1):
                np.testing.assert_array_equal(
                    run.gpairs[r][j], oracle.gpairs[r][j],
                    err_msg=f"gradients of round {r}")
        for i in range(r * per_round, (r + 1) * per_round):
            t = run.trees[i]
            to.check_well_formed(t.feat, t.left, t.parent)
            got = to.canonical_arrays(t.feat, t.thr, t.left, t.default_left,
                                      t.value, t.gain, t.cover)
            assert got == oracle.trees[i], f"tree {i} (round {r})"
    np.testing.assert_array_equal(
        run.margins[-1].view(np.int32), oracle.margins[-1].view(np.int32),
        err_msg="final margin")
    assert run.pred_leaf.shape == oracle.leaf_ids.shape
    for i, t in enumerate(run.trees):
        np.testing.assert_array_equal(
            to.preorder_arrays(t.feat, t.left)[run.pred_leaf[:, i]],
            oracle.leaf_ids[:, i], err_msg=f"pred_leaf of tree {i}")


def n_leaves(canon):
    if canon[0] == "leaf":
        return 1
    return n_leaves(canon[5]) + n_leaves(canon[6])


def depth_of(canon):
    if canon[0] == "leaf":
        return 0
    return 1 + max(depth_of(canon[5]), depth_of(canon[6]))


def level_widths(canon):
    """Number of nodes on every level of a canonical tree."""
    out, level = [], [canon]
    while level:
        out.append(len(level))
        level = [ch for nd in level if nd[0] != "leaf" for ch in nd[5:7]]
    return out
