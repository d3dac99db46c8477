"""The boosting engine: depth-wise GPU histogram tree growing.

MI355X-native replacement for XGBoost's ``gpu_hist`` updater + training
loop (the reference delegates this entirely to ``xgb.train``, reference
main.py:745; SURVEY.md #2.3 row 2 calls it the centerpiece). Per round:

  grad/hess kernel -> int64 fixed-point quantization -> per-depth
  LDS-tiled histogram build (smaller child only; sibling derived by the
  histogram-subtraction trick) -> RCCL AllReduce of the built histograms
  over xGMI -> best-split scan -> stable row partition -> next depth.

Int64 fixed-point gradients make every reduction an integer sum:
bitwise-deterministic regardless of GPU atomic ordering, feature-block
schedule, or world size - which is what makes checkpoint-resume models
exactly reproducible (reference test_fault_tolerance.py:401-449).
"""

import math
import os
import time
from dataclasses import dataclass, field
from typing import (Callable, Dict, List, NamedTuple, Optional, Sequence,
                    Tuple, Union)

import numpy as np
import torch

from xgboost_ray_amd import ops
from xgboost_ray_amd.booster import Booster, Tree
from xgboost_ray_amd.engine.collective import Collective
from xgboost_ray_amd.engine.metrics import get_metric
from xgboost_ray_amd.engine.objectives import Objective, get_objective
from xgboost_ray_amd.engine.quantile import BinnedMatrix, HistogramCuts

_QUANT_BITS = 30

# The row-order tree finish (RXGB_ROW_FINISH) is selected up to this row
# stride of the binned matrix, in bytes: there apply_tree_binned holds the
# whole row in registers and streams the matrix once. Wider rows take one
# byte load per level from scattered sectors of a long row and keep the
# legacy finish (numbers: profiles/README.md, round-3 pass 1).
_ROW_FINISH_MAX_STRIDE = 64


@dataclass
class TrainParams:
    objective: Union[str, Callable] = "reg:squarederror"
    eta: float = 0.3
    max_depth: int = 6
    max_bin: int = 256
    reg_lambda: float = 1.0
    reg_alpha: float = 0.0
    gamma: float = 0.0
    min_child_weight: float = 1.0
    max_delta_step: float = 0.0
    subsample: float = 1.0
    sampling_method: str = "uniform"  # or "gradient_based"
    num_parallel_tree: int = 1
    colsample_bytree: float = 1.0
    colsample_bylevel: float = 1.0
    colsample_bynode: float = 1.0
    scale_pos_weight: float = 1.0
    base_score: Optional[float] = None
    num_class: int = 0
    eval_metric: List[str] = field(default_factory=list)
    seed: int = 0
    grow_policy: str = "depthwise"
    max_leaves: int = 0
    monotone_constraints: object = None
    interaction_constraints: object = None
    tweedie_variance_power: float = 1.5
    aft_loss_distribution: str = "normal"
    aft_loss_distribution_scale: float = 1.0
    quantile_alpha: object = None  # float | list | "[a,b]" (reg:quantileerror)
    # rank:pairwise / rank:ndcg pair truncation: "all", or "topk" with
    # k = lambdarank_num_pair_per_sample (default 32)
    lambdarank_pair_method: str = "all"
    lambdarank_num_pair_per_sample: Optional[int] = None
    tree_method: str = "hist"
    booster: str = "gbtree"
    # DART (booster="dart") dropout parameters (xgboost semantics)
    rate_drop: float = 0.0
    skip_drop: float = 0.0
    one_drop: bool = False
    normalize_type: str = "tree"
    sample_type: str = "uniform"  # or "weighted" (xgboost dart.cc)
    verbosity: int = 1
    nthread: int = 0
    disable_default_eval_metric: bool = False

    @classmethod
    def from_dict(cls, params: Dict) -> "TrainParams":
        p = cls()
        alias = {
            "learning_rate": "eta",
            "lambda": "reg_lambda",
            "alpha": "reg_alpha",
            "min_split_loss": "gamma",
            "random_state": "seed",
            "n_jobs": "nthread",
        }
        for k, v in (params or {}).items():
            k = alias.get(k, k)
            if k == "eval_metric":
                p.eval_metric = [v] if isinstance(v, str) else list(v)
            elif hasattr(p, k):
                setattr(p, k, v)
            # unknown params are accepted silently (xgboost behavior)
        p.eta = float(p.eta)
        p.max_depth = int(p.max_depth)
        p.max_bin = int(p.max_bin)
        p.num_class = int(p.num_class or 0)
        p.seed = int(p.seed or 0)
        p.num_parallel_tree = max(1, int(p.num_parallel_tree or 1))
        p.subsample = 1.0 if p.subsample is None else float(p.subsample)
        p.sampling_method = p.sampling_method or "uniform"
        if not 0.0 < p.subsample <= 1.0:
            raise ValueError(
                f"subsample must be in (0, 1], got {p.subsample}")
        if p.sampling_method not in ("uniform", "gradient_based"):
            raise ValueError(
                "sampling_method must be 'uniform' or 'gradient_based', "
                f"got {p.sampling_method!r}")
        if (p.sampling_method == "gradient_based"
                and p.objective == "reg:quantileerror"):
            raise ValueError(
                "sampling_method='gradient_based' is not supported with "
                "reg:quantileerror: adaptive leaves take unweighted "
                "residual quantiles of the sampled rows")
        p.lambdarank_pair_method = p.lambdarank_pair_method or "all"
        if p.lambdarank_pair_method not in ("all", "topk"):
            raise ValueError(
                "lambdarank_pair_method must be 'all' or 'topk' (sampled "
                f"pairs, 'mean', are not supported), got "
                f"{p.lambdarank_pair_method!r}")
        k = p.lambdarank_num_pair_per_sample
        if p.lambdarank_pair_method == "all":
            if k is not None:
                raise ValueError(
                    "lambdarank_num_pair_per_sample needs "
                    "lambdarank_pair_method='topk'; 'all' uses every pair")
        else:
            if p.objective == "rank:map":
                raise ValueError(
                    "lambdarank_pair_method='topk' is not supported with "
                    "rank:map; use rank:pairwise or rank:ndcg")
            k = 32 if k is None else k
            try:  # parameter dicts often carry numbers as strings
                kf = float(k)
            except (TypeError, ValueError):
                kf = 0.0
            if isinstance(k, bool) or not (
                    1.0 <= kf < 2.0**31 and kf == math.floor(kf)):
                raise ValueError(
                    "lambdarank_num_pair_per_sample must be an integer "
                    f">= 1, got {k!r}")
            p.lambdarank_num_pair_per_sample = int(kf)
        if isinstance(p.monotone_constraints, str):
            txt = p.monotone_constraints.strip().strip("()")
            p.monotone_constraints = [
                int(x) for x in txt.split(",") if x.strip()
            ]
        if isinstance(p.interaction_constraints, str):
            import ast

            p.interaction_constraints = ast.literal_eval(
                p.interaction_constraints
            )
        return p


@dataclass
class EvalPack:
    """One eval set: raw features + incremental margin state."""

    name: str
    X: Optional[torch.Tensor]  # None => the training matrix itself
    label: Optional[torch.Tensor] = None
    weight: Optional[torch.Tensor] = None
    qid: Optional[torch.Tensor] = None
    base_margin: Optional[torch.Tensor] = None
    margin: Optional[torch.Tensor] = None


class _TreeArrays:
    """Growable SoA node storage for depthwise growth (replaces python
    lists of per-node appends; fields are written by vectorized numpy
    fancy-indexing per depth)."""

    __slots__ = ("feat", "thr", "split_bin", "left", "dl", "val", "gain",
                 "cover", "parent", "n", "cap")
    _FIELDS = (
        ("feat", -1, np.int64), ("thr", 0.0, np.float64),
        # bin index behind thr ("bin <= split_bin" goes left): the binned
        # row-order walk needs it; it is not part of the Tree
        ("split_bin", 0, np.int64),
        ("left", -1, np.int64), ("dl", 0, np.int64),
        ("val", 0.0, np.float64), ("gain", 0.0, np.float64),
        ("cover", 0.0, np.float64), ("parent", -1, np.int64),
    )

    def __init__(self, cap: int = 64):
        self.cap = int(cap)
        self.n = 1  # root preallocated (all defaults)
        for name, fill, dt in self._FIELDS:
            setattr(self, name, np.full(self.cap, fill, dt))

    def ensure(self, need: int):
        if need <= self.cap:
            return
        cap = self.cap
        while cap < need:
            cap *= 2
        for name, fill, dt in self._FIELDS:
            old = getattr(self, name)
            new = np.full(cap, fill, dt)
            new[: self.n] = old[: self.n]
            setattr(self, name, new)
        self.cap = cap

    def record_splits(self, nids, feat, sbin, dl, gain, cover,
                      cuts_flat, cut_ptr):
        """Turn nodes ``nids`` into splits and append their children.
        Returns the left child ids, in scan-slot order (matches the
        sequential numbering the list-based builder produced)."""
        base = self.n
        n_split = nids.size
        lids = base + 2 * np.arange(n_split, dtype=np.int64)
        self.ensure(base + 2 * n_split)
        self.feat[nids] = feat
        # split after bin b: left iff bin <= b; bin b covers
        # [cut[b-1], cut[b]) so "bin <= b" <=> v < cut[b] = thr.
        self.thr[nids] = cuts_flat[cut_ptr[feat] + sbin].astype(np.float64)
        self.split_bin[nids] = sbin
        self.left[nids] = lids
        self.dl[nids] = dl
        self.gain[nids] = gain
        self.cover[nids] = cover
        self.parent[lids] = nids
        self.parent[lids + 1] = nids
        self.n = base + 2 * n_split
        return lids

    def to_tree(self) -> Tree:
        n = self.n
        return Tree(
            feat=self.feat[:n].astype(np.int32),
            thr=self.thr[:n].astype(np.float32),
            left=self.left[:n].astype(np.int32),
            default_left=self.dl[:n].astype(np.uint8),
            value=self.val[:n].astype(np.float32),
            gain=self.gain[:n].astype(np.float32),
            cover=self.cover[:n].astype(np.float32),
            parent=np.where(
                self.parent[:n] < 0, 2147483647, self.parent[:n]
            ).astype(np.int32),
        )


def _interleave(left, right, dtype=np.int64):
    """[l0, r0, l1, r1, ...]: children sit next to their sibling."""
    out = np.empty(2 * left.size, dtype)
    out[0::2] = left
    out[1::2] = right
    return out


class _Frontier:
    """SoA frontier of depthwise growth: one numpy array per field.
    Children are always appended as (left, right) pairs, so siblings sit
    at positions 2i / 2i+1 and the build/derive pairing vectorizes.

    ``in_build_order`` returns the same nodes in scan-slot order and sets
    the three build fields; they are None on a frontier in child order."""

    __slots__ = ("nid", "start", "count", "sumg", "sumh", "pslot", "wlo",
                 "whi", "paths", "K", "derive_pslot", "derive_sib_pos")

    def __init__(self, nid, start, count, sumg, sumh, pslot, wlo, whi,
                 paths):
        self.nid, self.start, self.count = nid, start, count
        self.sumg, self.sumh = sumg, sumh  # quantized
        self.pslot = pslot  # parent's scan slot in the previous depth
        self.wlo, self.whi = wlo, whi  # monotone weight bounds
        # split features on each root path (sorted tuples), or None when
        # there are no interaction constraints
        self.paths = paths
        self.K = self.derive_pslot = self.derive_sib_pos = None

    @classmethod
    def root(cls, n_rows, sumg, sumh, track_paths):
        return cls(
            np.zeros(1, np.int64), np.zeros(1, np.int64),
            np.array([n_rows], np.int64), np.array([sumg], np.int64),
            np.array([sumh], np.int64), np.zeros(1, np.int64),
            np.full(1, -np.inf), np.full(1, np.inf),
            [()] if track_paths else None,
        )

    @property
    def size(self):
        return self.nid.size

    def in_build_order(self, depth):
        """Scan-slot order: per sibling pair build the globally smaller
        child (quantized hessian sum as the size proxy - identical on
        every rank; local counts are not), derive the sibling by
        subtraction. Built block = the ``K`` leading slots (one
        AllReduce, batched subtraction for the rest); derived slot K + j
        is its parent's histogram (slot ``derive_pslot[j]`` of the previous
        depth) minus built slot ``derive_sib_pos[j]``."""
        if depth == 0:
            order = np.zeros(1, np.int64)
            K = 1
            derive_pslot = np.zeros(0, np.int64)
        else:
            ia = np.arange(0, self.size, 2)
            ib = ia + 1
            small_is_a = self.sumh[ia] <= self.sumh[ib]
            idx_small = np.where(small_is_a, ia, ib)
            idx_big = np.where(small_is_a, ib, ia)
            order = np.concatenate([idx_small, idx_big])
            K = idx_small.size
            derive_pslot = self.pslot[idx_big]
        lvl = _Frontier(
            self.nid[order], self.start[order], self.count[order],
            self.sumg[order], self.sumh[order], self.pslot[order],
            self.wlo[order], self.whi[order],
            None if self.paths is None else [self.paths[i] for i in order],
        )
        lvl.K = K
        lvl.derive_pslot = derive_pslot
        lvl.derive_sib_pos = np.arange(derive_pslot.size, dtype=np.int64)
        return lvl

    def meta(self):
        """One depth's control data as a single int64 vector: {sum_g |
        sum_h | start | count} per scan slot, then {derive_pslot |
        derive_sib_pos}."""
        return np.concatenate(
            [self.sumg, self.sumh, self.start, self.count,
             self.derive_pslot, self.derive_sib_pos]
        )

    def bounds(self):
        """[size, 2] float64 monotone weight bounds."""
        return torch.from_numpy(
            np.ascontiguousarray(np.stack([self.wlo, self.whi], axis=1))
        )

    def children(self, ok, lids, feat, lc, left_g, left_h, mono=None):
        """The next frontier: both children of the split slots ``ok`` of
        this level (ascending), given their left child ids, split
        features, left row counts and left sums. ``mono``: (per-feature
        constraint, scale_g, scale_h, lambda, alpha) or None."""
        l_start = self.start[ok]
        r_sumg = self.sumg[ok] - left_g
        r_sumh = self.sumh[ok] - left_h
        # monotone child bounds (exact op order of the scalar path)
        wlo_p = self.wlo[ok]
        whi_p = self.whi[ok]
        l_wlo = r_wlo = wlo_p
        l_whi = r_whi = whi_p
        if mono is not None:
            mono_np, scale_g, scale_h, lam, alpha = mono
            cvec = mono_np[feat]
            act = cvec != 0
            if act.any():
                wl = np.maximum(wlo_p, np.minimum(
                    whi_p, _calc_weight_vec(
                        left_g / scale_g, left_h / scale_h, lam, alpha
                    )))
                wr = np.maximum(wlo_p, np.minimum(
                    whi_p, _calc_weight_vec(
                        r_sumg / scale_g, r_sumh / scale_h, lam, alpha
                    )))
                mid = 0.5 * (wl + wr)
                pos = act & (cvec > 0)
                neg = act & (cvec < 0)
                l_whi = np.where(pos, np.minimum(whi_p, mid), whi_p)
                r_wlo = np.where(pos, np.maximum(wlo_p, mid), wlo_p)
                l_wlo = np.where(neg, np.maximum(wlo_p, mid), wlo_p)
                r_whi = np.where(neg, np.minimum(whi_p, mid), whi_p)
        paths = None
        if self.paths is not None:
            paths = []
            for k_i, f_i in zip(ok.tolist(), feat.tolist()):
                cp = tuple(sorted(set(self.paths[k_i]) | {int(f_i)}))
                paths += [cp, cp]
        return _Frontier(
            _interleave(lids, lids + 1),
            _interleave(l_start, l_start + lc),
            _interleave(lc, self.count[ok] - lc),
            _interleave(left_g, r_sumg),
            _interleave(left_h, r_sumh),
            _interleave(ok, ok),
            _interleave(l_wlo, r_wlo, np.float64),
            _interleave(l_whi, r_whi, np.float64),
            paths,
        )


class _Route(NamedTuple):
    """How one depthwise tree gets its splits (decided once per tree)."""

    use_fused_loop: bool  # one-sync loop with ping-pong row-id buffers
    row_finish: bool  # margins by one row-order walk of the finished tree
    fused_glue: bool  # derive/reduce/plan fused into scan and partition
    tree_enq: bool  # every level enqueued by one call
    use_depth_step: bool  # one C++ call per depth


class _LevelSplits(NamedTuple):
    """Best split of every scan slot of one level, as host arrays."""

    gain: np.ndarray
    feature: np.ndarray
    bin: np.ndarray
    default_left: np.ndarray
    left_g: np.ndarray
    left_h: np.ndarray
    # left row counts of the slots that split, ascending, when the level's
    # partition already ran on the device; None: the caller partitions
    left_counts: Optional[np.ndarray]
    # ping-pong row-id buffer the level was read from by that partition
    # (0 when there is none)
    in_buf: int


def _decode_pull(arr, KK, lc_off, in_buf, with_counts=True):
    """A pulled {packed [KK, 6] | left counts at ``lc_off``} int64 block."""
    return _LevelSplits(
        *_unpack_splits(arr[: 6 * KK].reshape(KK, 6)),
        arr[lc_off : lc_off + KK].copy() if with_counts else None,
        in_buf,
    )


class _PhaseTimer:
    """RXGB_PROFILE_ENGINE: wall time per phase of one tree, every tick
    behind a device synchronize, printed as one ``PROF`` dict. Does
    nothing when the variable is unset."""

    def __init__(self, device):
        self.on = bool(os.environ.get("RXGB_PROFILE_ENGINE"))
        self.cuda = device.type == "cuda"
        self.phases = {}
        self.last = None
        self.tick(None)

    def tick(self, name):
        if not self.on:
            return
        if self.cuda:
            torch.cuda.synchronize()
        now = time.perf_counter()
        if self.last is not None:
            self.phases[name] = self.phases.get(name, 0.0) + now - self.last
        self.last = now

    def report(self):
        if self.on:
            print("PROF", {k: round(v * 1000, 2)
                           for k, v in self.phases.items()}, flush=True)


class _TreeGrow:
    """What the per-depth steps of one depthwise tree share."""

    def __init__(self, it, cls, route, scale_g, scale_h, feat_mask, ridx,
                 gseg, prof):
        self.it, self.cls, self.route = it, cls, route
        self.scale_g, self.scale_h = scale_g, scale_h
        self.feat_mask = feat_mask  # colsample_bytree gate, or None
        # row ids and their segment-ordered gradient pairs: the partition
        # scatter permutes both each depth, so no per-depth gather pass
        self.ridx, self.gseg = ridx, gseg
        # the ping-pong ridx buffers exist ONLY for the one-sync loop - the
        # 2-sync path reassigns ridx to fresh clones each depth, which
        # would leave buffer 0 stale for the margin update
        self.ridx_bufs = (
            [ridx, torch.empty_like(ridx)] if route.use_fused_loop else None
        )
        self.cur_buf = 0
        self.prev_hist: Optional[torch.Tensor] = None
        self.enq_pull = None  # pinned pull slots of the whole-tree enqueue
        self.prof = prof
        self.ta = None  # _TreeArrays the levels write into
        self.cuts = None  # host copies of (cuts_flat, cut_ptr)
        # (constraint per feature, scale_g, scale_h, lambda, alpha) for
        # _Frontier.children, or None without monotone constraints
        self.mono = None

    def flip(self):
        """A partition read ``cur_buf`` and wrote the other buffer: make
        that one current and return the one that was read."""
        read = self.cur_buf
        self.cur_buf = 1 - read
        return read


def _hip():
    """The loaded HIP extension, for the bindings ``ops`` does not wrap."""
    from xgboost_ray_amd.ops import gpu

    return gpu._load()


def _quant_scale(mx: float) -> float:
    """Fixed-point scale of one gradient column: 2^30 / max|x|. An all-zero
    column takes scale 1 (every q is 0 under any finite scale; dividing by
    the maximum would give inf, and 0 * inf = NaN has no defined int32)."""
    return float(2.0**_QUANT_BITS) / mx if mx > 0.0 else 1.0


def _unpack_splits(pk):
    """Columns of a pulled ``packed`` [K, 6] int64 block (f32 gain bits,
    feature, bin, default_left, left_g, left_h) as owned arrays."""
    return (
        pk[:, 0].astype(np.int32).view(np.float32).copy(),
        pk[:, 1].astype(np.int32),
        pk[:, 2].astype(np.int32),
        pk[:, 3].astype(np.uint8),
        pk[:, 4].copy(),
        pk[:, 5].copy(),
    )


def _calc_weight_vec(G, H, lam, alpha):
    """Vectorized _calc_weight with the identical operation order (the
    scalar path's results are part of the bitwise determinism contract)."""
    denom = H + lam
    if alpha > 0:
        G = np.copysign(np.maximum(np.abs(G) - alpha, 0.0), G)
    bad = denom <= 0
    return np.where(bad, 0.0, -G / np.where(bad, 1.0, denom))


class CallbackList:
    def __init__(self, callbacks):
        self.callbacks = list(callbacks or [])

    def before_iteration(self, booster, iteration, evals_log) -> bool:
        stop = False
        for cb in self.callbacks:
            if hasattr(cb, "before_iteration"):
                stop |= bool(cb.before_iteration(booster, iteration, evals_log))
        return stop

    def after_iteration(self, booster, iteration, evals_log) -> bool:
        stop = False
        for cb in self.callbacks:
            if hasattr(cb, "after_iteration"):
                stop |= bool(cb.after_iteration(booster, iteration, evals_log))
            elif callable(cb):
                stop |= bool(cb(booster, iteration, evals_log))
        return stop

    def after_training(self, booster, iteration, evals_log):
        """End-of-training hook. Accepts both this engine's 3-arg form
        (booster, final_iteration, log) and xgboost's 1-arg
        TrainingCallback.after_training(model) signature."""
        import inspect

        for cb in self.callbacks:
            fn = getattr(cb, "after_training", None)
            if fn is None:
                continue
            try:
                n_params = len(inspect.signature(fn).parameters)
            except (TypeError, ValueError):
                n_params = 3
            if n_params >= 3:
                fn(booster, iteration, evals_log)
            else:
                fn(booster)


class BoostingEngine:
    """Single-rank engine; collectives make it data-parallel."""

    def __init__(
        self,
        params: Dict,
        dtrain: BinnedMatrix,
        collective: Optional[Collective] = None,
        rank: int = 0,
        custom_objective: Optional[Callable] = None,
    ):
        self.p = TrainParams.from_dict(params)
        self.raw_params = dict(params or {})
        self.dtrain = dtrain
        self.coll = collective or Collective()
        self.rank = rank
        self.device = dtrain.bins.device
        # pinned double-use staging buffers for tiny per-depth H2D pushes
        # (pageable copies block the host in the driver's staging path);
        # each slot is drained by a stream-ordered D2H pull before reuse
        self._pin_bufs = {}
        obj_spec = custom_objective or self.p.objective
        self.obj: Objective = get_objective(
            obj_spec, self.p.num_class, float(self.p.scale_pos_weight),
            float(self.p.tweedie_variance_power),
            quantile_alpha=self.p.quantile_alpha,
        )
        # xgboost defaults max_delta_step to 0.7 for Poisson regression
        if (self.p.objective == "count:poisson"
                and not self.p.max_delta_step):
            self.p.max_delta_step = 0.7
        from xgboost_ray_amd.engine.objectives import AFT, LambdaRankBase

        if isinstance(self.obj, AFT):
            self.obj.dist = str(self.p.aft_loss_distribution)
            self.obj.sigma = float(self.p.aft_loss_distribution_scale)
        if (isinstance(self.obj, LambdaRankBase)
                and self.p.lambdarank_pair_method == "topk"):
            self.obj.pair_method = "topk"
            self.obj.topk = self.p.lambdarank_num_pair_per_sample
        # output groups: classes, or one per quantile alpha
        self.n_class = max(
            1, self.p.num_class, getattr(self.obj, "n_target", 1)
        )
        self._adaptive = self.obj.adaptive_alpha(0) is not None
        self._adaptive_resid = None
        self._int_weight_cache = None
        # gradient-based sampling: the kept rows of the tree being grown
        # (None: uniform sampling), and the size of the last row sample
        self._mvs_ridx = None
        self.last_sample_rows = None
        if self._adaptive and self.p.monotone_constraints and any(
            int(c) for c in self.p.monotone_constraints
        ):
            raise ValueError(
                "monotone_constraints are not supported with "
                f"{self.obj.name}: adaptive leaves ignore the weight bounds"
            )
        if self.p.base_score is None:
            self.p.base_score = (
                self._quantile_intercept() if self._adaptive else 0.5
            )
        self.base_margin_const = self.obj.prob_to_margin(self.p.base_score)

        n = dtrain.n_rows
        shape = (n,) if self.n_class == 1 else (n, self.n_class)
        self.margin = torch.full(
            shape, self.base_margin_const, dtype=torch.float32, device=self.device
        )
        if dtrain.base_margin is not None:
            bm = dtrain.base_margin.reshape(shape)
            self.margin = self.margin + bm
        if dtrain.label is not None:
            self.obj.validate_label(dtrain.label)
        self._train_label = dtrain.label
        if isinstance(self.obj, AFT):
            yl = getattr(dtrain, "label_lower_bound", None)
            yu = getattr(dtrain, "label_upper_bound", None)
            if yl is None or yu is None:
                if dtrain.label is None:
                    raise ValueError(
                        "survival:aft needs label_lower_bound/"
                        "label_upper_bound (or a plain label for the "
                        "uncensored case)"
                    )
                yl = yu = dtrain.label
            self._train_label = torch.stack(
                [yl.float(), yu.float()], dim=1
            )
        self.feat_bins = dtrain.cuts.feat_bins().to(self.device)
        self.n_bins = dtrain.cuts.max_bins
        # tree_method="approx": the cuts are re-sketched for every tree
        # with the hessians as weights (_resketch); the histogram stride
        # stays at the bin budget so no buffer shape moves between trees
        self._approx = (
            str(self.p.tree_method) in ("approx", "gpu_approx")
            and self.p.booster != "gblinear"
        )
        if self._approx:
            if getattr(dtrain, "raw_X", None) is None:
                raise ValueError(
                    "tree_method=approx needs the raw feature matrix - "
                    "build the BinnedMatrix with keep_raw=True (streaming "
                    "matrices are not supported for approx)"
                )
            self.n_bins = max(self.n_bins, min(self.p.max_bin, 255))
            self._col_max = self._global_col_max(dtrain.raw_X)
        self.mono = None
        mc = self.p.monotone_constraints
        if mc:
            arr = np.zeros(dtrain.n_features, dtype=np.int8)
            for i, c in enumerate(list(mc)[: dtrain.n_features]):
                arr[i] = int(c)
            if arr.any():
                self.mono = torch.from_numpy(arr).to(self.device)
                if self.p.grow_policy == "lossguide":
                    raise ValueError(
                        "monotone_constraints are not supported with "
                        "grow_policy=lossguide yet"
                    )
        # interaction constraints: list of feature-index groups
        # (reference defers to xgboost's `interaction_constraints`;
        # semantics: a split feature must share a constraint set with
        # every feature already used on the node's root path)
        self.interaction_sets = None
        ic = self.p.interaction_constraints
        if ic:
            self.interaction_sets = [frozenset(int(f) for f in g)
                                     for g in ic]
        self.lin_w = None
        if self.p.booster == "gblinear":
            raw = getattr(dtrain, "raw_X", None)
            if raw is None:
                raise ValueError(
                    "booster=gblinear needs the raw feature matrix - "
                    "build the BinnedMatrix with keep_raw=True (streaming "
                    "matrices are not supported for gblinear)"
                )
            self.lin_w = torch.zeros(
                (dtrain.n_features + 1, self.n_class),
                dtype=torch.float64, device=self.device,
            )
        elif self.p.booster not in ("gbtree", "dart", ""):
            raise ValueError(
                f"Unsupported booster: {self.p.booster!r} "
                "(gbtree/dart/gblinear)"
            )
        self.iteration = 0
        self.booster = Booster(
            params={
                "objective": getattr(self.obj, "name", "custom"),
                "base_score": self.p.base_score,
                "num_class": self.p.num_class,
                "num_feature": dtrain.n_features,
                "max_depth": self.p.max_depth,
                "eta": self.p.eta,
                "num_parallel_tree": self.p.num_parallel_tree,
                # retained so predict() can route to GPU actors
                # (_is_gpu_params reads the model's tree_method)
                "tree_method": self.p.tree_method,
                "booster": self.p.booster,
            }
        )
        if self._adaptive:
            self.booster.params["num_target"] = self.obj.n_target
            self.booster.params["quantile_alpha"] = (
                "[" + ",".join(repr(a) for a in self.obj.alphas) + "]"
            )

    # -- adaptive (exact weighted quantile) leaves -----------------------------
    def _int_weights(self) -> Optional[torch.Tensor]:
        """Integer row weights of the quantile select: None for unit
        weights, else llrint(w * 2^30 / w_max) with the global w_max (one
        MAX allreduce per engine, as _quantize derives its scales)."""
        w = self.dtrain.weight
        if w is None:
            return None
        if self._int_weight_cache is None:
            mx = (w.max() if w.numel() else w.new_zeros(())).double().reshape(1)
            if self.coll.is_distributed:
                mx_d = mx.to(self.device) if self.device.type == "cuda" else mx
                self.coll.allreduce_(mx_d, op="max")
                mx = mx_d.cpu()
            w_max = max(float(mx[0]), 1e-300)
            self._int_weight_cache = torch.round(
                w.double() * float(2.0 ** _QUANT_BITS) / w_max
            ).to(torch.int64)
        return self._int_weight_cache

    def _allreduce_hook(self):
        return self.coll.allreduce_ if self.coll.is_distributed else None

    # -- tree_method="approx": per-tree hessian-weighted cuts -----------------
    def _global_col_max(self, X: torch.Tensor) -> torch.Tensor:
        """f32 [F]: the largest non-NaN value of every column over all
        ranks, NaN for an all-missing one (once per matrix, one MAX
        allreduce)."""
        nan = torch.isnan(X)
        neg_inf = torch.full_like(X[:1], float("-inf"))
        mx = torch.where(nan, neg_inf, X).amax(0) if X.shape[0] else neg_inf[0]
        packed = torch.stack([mx, (~nan).any(0).float()])
        if self.coll.is_distributed:
            self.coll.allreduce_(packed, op="max")
        return torch.where(packed[1] > 0, packed[0],
                           torch.full_like(packed[0], float("nan")))

    def _install_cuts(self, cuts: HistogramCuts):
        """Make ``cuts`` the training matrix's cuts: re-bin the raw features
        into the resident bin storage, refresh its column-major copy and the
        engine's per-feature bin counts. ``n_bins`` (the histogram stride)
        does not move. The growers read the host copies of the cut values
        from ``dtrain.cuts`` at the start of each tree, after this."""
        dm = self.dtrain
        dm.cuts = cuts
        ops.bin_matrix(dm.raw_X, cuts.cuts_flat, cuts.cut_ptr, out=dm.bins)
        if getattr(dm, "bins_t", None) is not None:
            dm.bins_t.copy_(dm.bins.t())
        self.feat_bins = cuts.feat_bins().to(self.device)

    def _resketch(self, gq: torch.Tensor):
        """One exact weighted sketch with this tree's quantized hessians as
        row weights (int32 on a global scale, so world-consistent; every row
        counts, sampled or not), then ``_install_cuts``."""
        cuts = ops.weighted_cuts(
            self.dtrain.raw_X, gq[:, 1], self.p.max_bin, self._col_max,
            allreduce=self._allreduce_hook(),
        )
        self._install_cuts(cuts)

    def _add_tree_margin_by_value(self, t: Tree, margin_view):
        """Add one tree's leaf values by walking the raw features: under
        approx the bins belong to the latest tree only, and thresholds are
        cut values, so "x < thr" is the routing every tree was grown with."""
        n = self.dtrain.n_rows
        add = torch.zeros(n, dtype=torch.float32, device=self.device)
        ops.predict_trees(
            self.dtrain.raw_X,
            torch.from_numpy(t.feat).to(self.device),
            torch.from_numpy(t.thr).to(self.device),
            torch.from_numpy(t.left).to(self.device),
            torch.from_numpy(t.default_left).to(self.device),
            torch.from_numpy(t.value).to(self.device),
            torch.tensor([0, t.num_nodes], dtype=torch.int32),
            add,
        )
        margin_view += add

    def _quantile_intercept(self) -> float:
        """Mean over alphas of the global alpha-quantile of the labels: the
        leaf select over one segment covering all rows, residual = label."""
        label = self.dtrain.label
        if label is None:
            return 0.5
        n = int(label.shape[0])
        ridx = torch.arange(n, dtype=torch.int32, device=self.device)
        resid = label.to(torch.float32).contiguous()
        qs = []
        for k in range(self.obj.n_target):
            q, W = ops.leaf_quantile_select(
                resid, self._int_weights(), ridx, [0], [n],
                self.obj.adaptive_alpha(k), allreduce=self._allreduce_hook(),
            )
            qs.append(float(q[0]) if int(W[0]) > 0 else 0.5)
        return float(np.mean(np.asarray(qs, np.float64)))

    def _adaptive_leaf_values(self, cls, ridx, ridx_b, parity):
        """Re-fit the finished leaves in _leaf_segs to eta * (exact global
        weighted alpha-quantile of their residuals). Returns the new
        float64 leaf values (Newton value kept where the leaf is globally
        empty) and rewrites _leaf_segs; the caller stores them per node."""
        segs = self._leaf_segs
        resid = self._adaptive_resid
        if resid.dim() == 2:
            resid = resid[:, cls].contiguous()
        q, W = ops.leaf_quantile_select(
            resid, self._int_weights(), ridx,
            [s for (s, c, v, bp) in segs], [c for (s, c, v, bp) in segs],
            self.obj.adaptive_alpha(cls), ridx_b=ridx_b, parity=parity,
            allreduce=self._allreduce_hook(),
        )
        old = np.asarray([v for (s, c, v, bp) in segs], np.float64)
        new = np.where(W > 0, self.p.eta * q.astype(np.float64), old)
        self._leaf_segs = [
            (s, c, float(nv), bp) for (s, c, v, bp), nv in zip(segs, new)
        ]
        return new

    # -- resume ------------------------------------------------------------
    def load_model(self, model: Booster):
        """Continue training from an existing model (xgb_model kwarg)."""
        self.booster = model
        self.iteration = model.num_boosted_rounds()
        # restore the dart weight ledger (weighted dropout resume)
        dw = model.attr("dart_weights")
        if dw:
            self._dart_w = [float(x) for x in dw.split(",") if x]
        # recompute margins through the binned matrix (thresholds are exact
        # cut values for models we trained, so binned replay is exact)
        n = self.dtrain.n_rows
        shape = (n,) if self.n_class == 1 else (n, self.n_class)
        base = self.obj.prob_to_margin(model.base_score)
        self.base_margin_const = base
        self.margin = torch.full(
            shape, base, dtype=torch.float32, device=self.device
        )
        if self.dtrain.base_margin is not None:
            self.margin = self.margin + self.dtrain.base_margin.reshape(shape)
        if getattr(model, "linear_weights", None) is not None:
            # gblinear resume: restore weights, recompute margins exactly
            self.lin_w = torch.from_numpy(
                np.asarray(model.linear_weights, np.float64)
            ).to(self.device).reshape(self.dtrain.n_features + 1,
                                      self.n_class)
            X = self.dtrain.raw_X
            w32 = self.lin_w.float()
            m = X @ w32[:-1] + w32[-1]
            self.margin = (
                self.margin + (m[:, 0] if self.n_class == 1 else m)
            )
            return
        self._replay_trees_binned(model)

    def _replay_trees_binned(self, model: Booster):
        if self._approx:
            for i, t in enumerate(model.trees):
                cls = model.tree_info[i] if i < len(model.tree_info) else 0
                self._add_tree_margin_by_value(
                    t, self.margin if self.n_class == 1
                    else self.margin[:, cls])
            return
        cuts = self.dtrain.cuts
        cut_ptr = cuts.cut_ptr.cpu().numpy()
        cuts_np = cuts.cuts_flat.cpu().numpy()
        for i, t in enumerate(model.trees):
            cls = model.tree_info[i] if i < len(model.tree_info) else 0
            split_bin = np.zeros(t.num_nodes, dtype=np.int32)
            for nid in range(t.num_nodes):
                if t.feat[nid] >= 0:
                    f = int(t.feat[nid])
                    lo, hi = cut_ptr[f], cut_ptr[f + 1]
                    # stored thr == cut[b] for a "bin <= b" split, so the
                    # bin index is exactly the position of thr in the cuts
                    b = np.searchsorted(cuts_np[lo:hi], t.thr[nid], side="left")
                    split_bin[nid] = b
            margin_view = (
                self.margin if self.n_class == 1 else self.margin[:, cls]
            )
            self._add_tree_margin_binned(t, split_bin, margin_view)

    def _add_tree_margin_binned(self, t: Tree, split_bin, margin_view):
        bins = self.dtrain.bins
        n = bins.shape[0]
        if bins.is_cuda:
            # one HIP row-order walk (same predicate, same f32 add) in
            # place of the per-level torch loop below, which stays as the
            # CPU path
            ops.apply_tree_binned(
                bins, margin_view, t.feat, split_bin, t.left,
                t.default_left, t.value,
            )
            return
        cur = torch.zeros(n, dtype=torch.int64, device=self.device)
        feat = torch.from_numpy(t.feat.astype(np.int64)).to(self.device)
        sbin = torch.as_tensor(split_bin, dtype=torch.int64, device=self.device)
        left = torch.from_numpy(t.left.astype(np.int64)).to(self.device)
        dl = torch.from_numpy(t.default_left.astype(np.uint8)).to(self.device)
        val = torch.from_numpy(t.value).to(self.device)
        while True:
            f = feat[cur]
            active = f >= 0
            if not bool(active.any()):
                break
            rows = torch.nonzero(active).flatten()
            fa = f[rows]
            bv = bins[rows, fa].long()
            miss = bv == ops.MISSING_BIN
            go_left = bv <= sbin[cur[rows]]
            go_left = torch.where(miss, dl[cur[rows]].bool(), go_left)
            cur[rows] = torch.where(go_left, left[cur[rows]], left[cur[rows]] + 1)
        margin_view += val[cur]

    # -- one boosting round --------------------------------------------------
    def update(self):
        it = self.iteration
        label = self._train_label
        dart_ctx = None
        if self.p.booster == "dart":
            dart_ctx = self._dart_dropout(it)
        gpair = self.obj.gradients(
            self.margin, label, self.dtrain.weight, self.dtrain.qid
        )
        if self._adaptive and self.p.booster != "gblinear":
            # residuals of the margin the gradients saw (dart dropout
            # respected; every tree of this round fits the same ones)
            y = label if self.margin.dim() == 1 else label.unsqueeze(1)
            self._adaptive_resid = (y.float() - self.margin) + 0.0
        if self.p.booster == "gblinear":
            self._update_linear(gpair)
            self.iteration += 1
            return []
        trees, classes = [], []
        # per-class maxima from ops.softmax_grad: each class slice carries
        # its own, so _quantize / _mvs_sample skip their reductions
        mx_cls = getattr(gpair, "_rxgb_absmax_cls", None)
        for cls in range(self.n_class):
            gp = gpair if self.n_class == 1 else gpair[:, cls, :]
            if mx_cls is not None:
                # the slice is contiguous, so gp.contiguous() below is gp
                gp._rxgb_absmax = mx_cls[cls]
            # num_parallel_tree > 1: boosted random forest - k trees per
            # round on the same gradients with independent row/column
            # samples (XGBoost GBTree::BoostNewTrees semantics)
            for ptree in range(self.p.num_parallel_tree):
                tree = self._grow_tree(
                    gp.contiguous(), it, cls, ptree=ptree
                )
                trees.append(tree)
                classes.append(cls)
        self.booster.append_round(trees, classes)
        if dart_ctx is not None:
            self._dart_commit(dart_ctx, trees, classes)
        self.iteration += 1
        return trees


    def _update_linear(self, gpair):
        """One gblinear round: preconditioned full-batch coordinate step.

        The reference reaches gblinear through xgboost's booster param
        passthrough (reference main.py:745 xgb.train(params...); exercised
        by reference tests/test_sklearn.py test_sklearn_api_gblinear).

        Deterministic replacement for xgboost's gblinear updaters
        (shotgun is non-deterministic; this is a damped Jacobi update
        with the same per-coordinate Newton preconditioner, L2 on
        weights and L1 soft-thresholding, eta-damped). Distributed: one
        fp64 AllReduce of [X^T g | (X*X)^T h | sum_g | sum_h] per class.
        """
        X = self.dtrain.raw_X
        n, F = X.shape
        lam = float(self.p.reg_lambda)
        alpha = float(self.p.reg_alpha)
        eta = float(self.p.eta)
        deltas = []
        mx_cls = getattr(gpair, "_rxgb_absmax_cls", None)
        for cls in range(self.n_class):
            gp = gpair if self.n_class == 1 else gpair[:, cls, :]
            if mx_cls is not None:
                gp._rxgb_absmax = mx_cls[cls]
            # chunked fp64 accumulation: fixed chunk order -> identical
            # sums on every rank layout of the same data
            sg = torch.zeros(F, dtype=torch.float64, device=self.device)
            sh = torch.zeros(F, dtype=torch.float64, device=self.device)
            sb = torch.zeros(2, dtype=torch.float64, device=self.device)
            CH = 1 << 20
            for s0 in range(0, n, CH):
                Xc = X[s0 : s0 + CH].double()
                gc = gp[s0 : s0 + CH, 0].double()
                hc = gp[s0 : s0 + CH, 1].double()
                sg += Xc.t() @ gc
                sh += (Xc * Xc).t() @ hc
                sb[0] += gc.sum()
                sb[1] += hc.sum()
            if self.coll.is_distributed:
                packed = torch.cat([sg, sh, sb])
                self.coll.allreduce_(packed)
                sg, sh, sb = packed[:F], packed[F : 2 * F], packed[2 * F :]
            w = self.lin_w[:F, cls]
            denom = sh + lam
            full = w - (sg + lam * w) / denom
            if alpha > 0.0:
                thr = alpha / denom
                full = torch.sign(full) * torch.clamp(
                    full.abs() - thr, min=0.0
                )
            dw = eta * (full - w)
            db = eta * (-sb[0] / (sb[1] + lam))
            self.lin_w[:F, cls] += dw
            self.lin_w[F, cls] += db
            dwf = dw.float()
            mv = self.margin if self.n_class == 1 else self.margin[:, cls]
            for s0 in range(0, n, CH):
                mv[s0 : s0 + CH] += X[s0 : s0 + CH] @ dwf
            mv += float(db)
            deltas.append((dwf, float(db)))
        self._lin_deltas = deltas
        self.booster.linear_weights = self.lin_w.cpu().numpy()
        self.booster.linear_rounds = self.iteration + 1
        self.booster.params["booster"] = "gblinear"


    # -- DART (dropout) ----------------------------------------------------
    def _dart_predict_trees(self, tree_ids):
        """Margin contribution of the given trees on the training rows."""
        contrib = torch.zeros_like(self.margin)
        for ti in tree_ids:
            t = self.booster.trees[ti]
            cls = self.booster.tree_info[ti]
            mv = contrib if self.n_class == 1 else contrib[:, cls]
            self._add_tree_margin_raw(t, mv)
        return contrib

    def _add_tree_margin_raw(self, t, margin_view):
        """Add one tree's predictions via the binned matrix (exact)."""
        if self._approx:
            return self._add_tree_margin_by_value(t, margin_view)
        cuts = self.dtrain.cuts
        cut_ptr = cuts.cut_ptr.cpu().numpy()
        cuts_np = cuts.cuts_flat.cpu().numpy()
        split_bin = np.zeros(t.num_nodes, dtype=np.int32)
        for nid in range(t.num_nodes):
            if t.feat[nid] >= 0:
                f = int(t.feat[nid])
                lo, hi = cut_ptr[f], cut_ptr[f + 1]
                split_bin[nid] = np.searchsorted(
                    cuts_np[lo:hi], t.thr[nid], side="left"
                )
        self._add_tree_margin_binned(t, split_bin, margin_view)

    def _dart_dropout(self, it):
        """Pick the dropped-tree set and remove it from the margins.

        The reference reaches DART through xgboost's booster="dart"
        passthrough (reference main.py:745); semantics follow xgboost
        dart.cc (rate_drop/skip_drop/one_drop/normalize_type).

        Deterministic: seeded by (seed, iteration), identical on every
        rank. Returns (dropped_ids, dropped_contrib) or a no-drop marker.
        """
        n_trees = len(self.booster.trees)
        rng = np.random.RandomState(
            (int(self.p.seed) * 77003 + it * 9973) % (2**31)
        )
        if n_trees == 0 or rng.rand() < float(self.p.skip_drop):
            return ([], None)
        if self.p.sample_type == "weighted":
            # xgboost dart.cc weighted selection: drop probability
            # proportional to the tree's current weight,
            # p_i = w_i * rate_drop * n / sum(w), clamped to 1
            w = np.asarray(self._dart_weights(n_trees), dtype=np.float64)
            sw = float(w.sum())
            if sw <= 0:
                p_i = np.full(n_trees, float(self.p.rate_drop))
            else:
                p_i = np.clip(
                    w * float(self.p.rate_drop) * n_trees / sw, 0.0, 1.0
                )
            drop = np.nonzero(rng.rand(n_trees) < p_i)[0]
        else:
            drop = np.nonzero(
                rng.rand(n_trees) < float(self.p.rate_drop)
            )[0]
        if drop.size == 0 and self.p.one_drop:
            drop = np.array([int(rng.randint(n_trees))])
        if drop.size == 0:
            return ([], None)
        dropped = [int(d) for d in drop]
        contrib = self._dart_predict_trees(dropped)
        self.margin -= contrib
        return (dropped, contrib)

    def _dart_weights(self, n_trees):
        """Per-tree weights for weighted dropout. Scales are baked into
        leaf values at commit time, so the weight ledger is maintained
        alongside (new trees enter at their new_scale; dropped trees are
        rescaled by old_scale; untouched trees keep weight 1 from their
        no-drop round)."""
        w = getattr(self, "_dart_w", None)
        if w is None:
            w = []
            self._dart_w = w
        while len(w) < n_trees:
            w.append(1.0)
        return w  # the LIVE ledger (callers mutate it in place)

    def _dart_commit(self, dart_ctx, trees, classes):
        """Scale the new + dropped trees (xgboost normalize_type) and
        restore margins. Scales are baked into leaf values so predict
        and serialization need no per-tree weight array."""
        dropped, contrib = dart_ctx
        k = len(dropped)
        if k == 0:
            return
        # xgboost dart.cc NormalizeTrees: leaves already carry eta, the
        # weights below redistribute mass between new and dropped trees
        lr = float(self.p.eta) / max(1, len(trees) // self.n_class)
        if self.p.normalize_type == "forest":
            new_scale = 1.0 / (1.0 + lr)
            old_scale = 1.0 / (1.0 + lr)
        else:  # "tree"
            new_scale = 1.0 / (k + lr)
            old_scale = k / (k + lr)
        # scale the just-built trees' leaves (and their margin effect,
        # which update() already added at full weight)
        delta = torch.zeros_like(self.margin)
        for t, cls in zip(trees, classes):
            mv = delta if self.n_class == 1 else delta[:, cls]
            self._add_tree_margin_raw(t, mv)
            t.value *= new_scale
        self.margin += (new_scale - 1.0) * delta
        self.booster._flat_cache = None
        self.booster._walk_cache = None  # node means follow the leaf values
        # scale the dropped trees and re-add their shrunk contribution
        for ti in dropped:
            self.booster.trees[ti].value *= old_scale
        self.margin += old_scale * contrib
        # weight ledger for sample_type="weighted"; persisted as a
        # booster attribute so checkpoint/resume reproduces the same
        # weighted-dropout probabilities (fuzz-found)
        wl = self._dart_weights(len(self.booster.trees))
        for ti in dropped:
            wl[ti] *= old_scale
        for i in range(len(trees)):
            wl[len(self.booster.trees) - len(trees) + i] = new_scale
        self.booster.set_attr(
            dart_weights=",".join(repr(w) for w in wl)
        )

    def _quantize(self, gpair: torch.Tensor) -> Tuple[torch.Tensor, float, float]:
        fused_mx = getattr(gpair, "_rxgb_absmax", None)
        if fused_mx is not None:
            # grad_fused already reduced |g|/|h| maxes in its single pass
            # (f32 max is order-free, so the value equals abs().max())
            mx = fused_mx.double()
        else:
            mx = torch.stack(
                [gpair[:, 0].abs().max(), gpair[:, 1].abs().max()]
            ).double()
        if self.coll.is_distributed:
            mx_d = mx.to(self.device) if self.device.type == "cuda" else mx
            self.coll.allreduce_(mx_d, op="max")
            mx = mx_d.cpu()
        scale_g = _quant_scale(float(mx[0]))
        scale_h = _quant_scale(float(mx[1]))
        self._gq_sum = None
        if gpair.is_cuda:
            # the quantize pass emits the column sums of what it writes:
            # the root totals of an unsampled tree, without re-reading gq
            gq, self._gq_sum = ops.quantize_gpair_sums(
                gpair, scale_g, scale_h
            )
            return gq, scale_g, scale_h
        return ops.quantize_gpair(gpair, scale_g, scale_h), scale_g, scale_h

    def _mvs_sample(self, gpair: torch.Tensor, it: int, tree: int):
        """sampling_method="gradient_based": keep row i with probability
        ~ sqrt(g^2 + 0.1 h^2), expected sample size k = subsample * n
        (per rank), and divide a kept row's pair by that probability.
        Returns the reweighted pairs (dropped rows zero); the ascending
        kept row ids go to ``_sample_rows`` through ``_mvs_ridx``. Integer
        arithmetic decides the sample: CPU and GPU draw the same rows."""
        fused_mx = getattr(gpair, "_rxgb_absmax", None)
        if fused_mx is not None:
            mx = fused_mx.double()
        else:
            mx = torch.stack(
                [gpair[:, 0].abs().max(), gpair[:, 1].abs().max()]
            ).double()
        if self.coll.is_distributed:
            mx_d = mx.to(self.device) if self.device.type == "cuda" else mx
            self.coll.allreduce_(mx_d, op="max")
            mx = mx_d
        mx = mx.cpu()
        k = max(1, int(self.p.subsample * self.dtrain.n_rows))
        c = ops.mvs_score(gpair, float(mx[0]), float(mx[1]))
        S, M = ops.mvs_threshold(c, k)
        keep, gpair_w = ops.mvs_sample(
            gpair, c, S, M,
            ops.mvs_key(self.p.seed, it, tree, self.rank),
        )
        self._mvs_ridx = torch.nonzero(keep).flatten().to(torch.int32)
        return gpair_w

    def _sample_rows(self, it: int, cls: int) -> torch.Tensor:
        ridx = self._sample_rows_impl(it, cls)
        self.last_sample_rows = int(ridx.numel())
        return ridx

    def _sample_rows_impl(self, it: int, cls: int) -> torch.Tensor:
        n = self.dtrain.n_rows
        if self._mvs_ridx is not None:
            return self._mvs_ridx
        if self.p.subsample >= 1.0:
            return torch.arange(n, dtype=torch.int32, device=self.device)
        gen = torch.Generator(device="cpu")
        gen.manual_seed(
            (self.p.seed * 2654435761 + it * 97 + cls * 31 + self.rank) % (2**63)
        )
        mask = torch.rand(n, generator=gen) < self.p.subsample
        return torch.nonzero(mask.to(self.device)).flatten().to(torch.int32)

    def _sample_features(
        self, it: int, cls: int, level: Optional[int] = None
    ) -> Optional[torch.Tensor]:
        """Feature mask for this tree (level=None) or depth level.

        Seeded identically on every rank (global seed, no rank term) so
        all workers mask the same features. feature_weights bias the
        selection (xgboost semantics)."""
        F = self.dtrain.n_features
        frac = (
            self.p.colsample_bytree if level is None else self.p.colsample_bylevel
        )
        if frac >= 1.0:
            return None
        k = max(1, int(round(F * frac)))
        gen = torch.Generator(device="cpu")
        salt = 7 if level is None else 1009 + level
        gen.manual_seed(
            (self.p.seed * 2654435761 + it * 97 + cls * 31 + salt) % (2**63)
        )
        fw = getattr(self.dtrain, "feature_weights", None)
        if fw is not None:
            w = fw.cpu().double().clamp(min=0)
            if float(w.sum()) > 0:
                perm = torch.multinomial(
                    w, k, replacement=False, generator=gen
                )
            else:
                perm = torch.randperm(F, generator=gen)[:k]
        else:
            perm = torch.randperm(F, generator=gen)[:k]
        mask = torch.zeros(F, dtype=torch.bool)
        mask[perm] = True
        return mask.to(self.device)


    def _stage_i64(self, arr, slot):
        """Pinned H2D staging for a small int64 numpy vector (GPU only)."""
        arr = np.ascontiguousarray(arr, dtype=np.int64).reshape(-1)
        n = arr.size
        buf = self._pin_bufs.get(slot)
        if buf is None or buf.numel() < n:
            cap = max(4096, 1 << max(0, (n - 1)).bit_length())
            buf = torch.empty(cap, dtype=torch.int64, pin_memory=True)
            self._pin_bufs[slot] = buf
        view = buf[:n]
        view.copy_(torch.from_numpy(arr))
        return view.to(self.device, non_blocking=True)


    def _bynode_mask(self, KK, it, cls, depth):
        """[KK, F] uint8 per-node feature gate for colsample_bynode.
        Multiplies with colsample_bytree/bylevel (those zero feat_bins)
        and interaction constraints (ANDed by the caller)."""
        F = self.dtrain.n_features
        k = max(1, int(round(float(self.p.colsample_bynode) * F)))
        rng = np.random.RandomState(
            (self.p.seed * 48271 + it * 2246822519
             + cls * 3266489917 + depth * 668265263) % (2**31)
        )
        m = np.zeros((KK, F), np.uint8)
        for row in range(KK):
            m[row, rng.choice(F, size=k, replace=False)] = 1
        return torch.from_numpy(m)

    def _allowed_mask(self, paths):
        """[K, F] uint8 gate from interaction constraints (None if off).

        ``paths``: per node, the tuple of split features on its root
        path. A feature is allowed iff some constraint set contains the
        whole path and the feature (xgboost semantics; at the root every
        feature may open a path).
        """
        if self.interaction_sets is None:
            return None
        F = self.dtrain.n_features
        m = np.zeros((len(paths), F), np.uint8)
        for i, path in enumerate(paths):
            pf = set(path)
            if not pf:
                m[i, :] = 1  # root: any feature may open the path
            else:
                allow = set()
                for cs in self.interaction_sets:
                    if pf <= cs:
                        allow |= cs
                for f in allow:
                    if 0 <= f < F:
                        m[i, f] = 1
        return torch.from_numpy(m)

    def _or_empty(self, t, dtype, shape=(0,)):
        """``t`` on the device as ``dtype``, or the empty placeholder the
        C++ entry points take for "absent"."""
        if t is None:
            return torch.zeros(shape, dtype=dtype, device=self.device)
        return t.to(self.device).to(dtype).contiguous()

    def _gated_feat_bins(self, mask):
        """Per-feature bin counts with the features outside ``mask`` zeroed
        (a feature without bins offers no split)."""
        if mask is None:
            return self.feat_bins
        return torch.where(
            mask, self.feat_bins, torch.zeros_like(self.feat_bins)
        )

    def _tree_rows(self, gq, it, key):
        """Row sample of one tree: (row ids, their gradient pairs in that
        order, global quantized root sums)."""
        ridx = self._sample_rows(it, key)
        n_local = int(ridx.numel())
        if n_local == self.dtrain.n_rows:
            gseg = gq  # identity order (partition clones before writing)
        else:
            gseg = gq[ridx.long()].contiguous()
        if n_local == 0:
            root_sum = torch.zeros(2, dtype=torch.int64, device=self.device)
        elif n_local == self.dtrain.n_rows:
            # no row sampling: ridx is the identity - skip the per-row
            # gather; on GPU the quantize pass already summed gq
            root_sum = getattr(self, "_gq_sum", None)
            if root_sum is None:
                root_sum = gq.sum(dim=0, dtype=torch.int64)
        else:
            root_sum = gq[ridx.long()].sum(dim=0, dtype=torch.int64)
        if self.coll.is_distributed:
            self.coll.allreduce_(root_sum)
        return ridx, gseg, root_sum

    def _finish_tree(self, tree, split_bin, cls, n_local, row_finish,
                     ridx, ridx_b=None):
        """Advance the training margins by the finished tree. ``ridx``
        (and ``ridx_b``, the second ping-pong buffer) hold the final row
        order the leaf segments in _leaf_segs index."""
        mv = self.margin if self.n_class == 1 else self.margin[:, cls]
        if row_finish:
            # one row-order walk of the finished tree over the binned
            # matrix: each row lands in the leaf the partition chose (or,
            # on the last level, would have chosen) and takes the same
            # single f32 add of the same float32(eta * w). Covers the
            # sampled and the unsampled rows alike.
            ops.apply_tree_binned(
                self.dtrain.bins, mv, tree.feat, split_bin, tree.left,
                tree.default_left, tree.value,
            )
        elif n_local < self.dtrain.n_rows:
            # row sampling: EVERY row's margin must advance (xgboost
            # UpdatePredictionCache semantics) - the leaf-segment
            # scatter only covers the sampled rows, which left
            # out-of-sample gradients on stale margins (fuzz-found in
            # round 2; also broke resume==continuous under subsample).
            # The binned tree walk lands each row in the identical leaf
            # the partition chose, so sampled rows get the same bits.
            self._add_tree_margin_raw(tree, mv)
        elif self._leaf_segs:
            # every row's final node is its segment's node; the leaf
            # finalization collected (start, count, value, buffer) segs
            starts, counts, vals, parity = zip(*self._leaf_segs)
            ops.update_margins(
                mv, ridx,
                torch.tensor(starts, dtype=torch.int64),
                torch.tensor(counts, dtype=torch.int64),
                np.asarray(vals, dtype=np.float32),
                ridx_b=ridx_b,
                parity=list(parity) if ridx_b is not None else None,
            )
        self._leaf_segs = []

    def _tree_route(self, n_local) -> _Route:
        """Read the route switches (per tree: tests toggle them inside one
        process). Each restores its legacy route exactly when set to 0."""
        gpu = self.device.type == "cuda"
        env = os.environ.get
        use_fused_loop = gpu and env("RXGB_ONE_SYNC", "1") != "0"
        # row-order finish: the margin update is one apply_tree_binned
        # walk over the binned matrix in row order, so the last level
        # launches no partition at all - its children are leaves, and
        # nothing but the scattered per-segment margin update ever read
        # the permuted ridx/gseg or the child row counts. Adaptive
        # objectives (reg:quantileerror) need the per-leaf row lists and
        # keep the legacy finish. RXGB_ROW_FINISH=2 lifts the row-stride
        # rule (measurement only).
        rf = env("RXGB_ROW_FINISH", "1")
        row_finish = (
            gpu
            and not self._adaptive
            and rf != "0"
            and (rf == "2"
                 or self.dtrain.bins.stride(0) <= _ROW_FINISH_MAX_STRIDE)
        )
        # fused per-depth glue: the sibling histograms are derived inside
        # the split scan, the per-node reduce and the partition plan are
        # one kernel, the partition needs no zero fills and one pull
        # brings {splits | left counts} to the host. RXGB_FUSED_GLUE=0
        # restores the separate torch/kernel composition.
        fused_glue = gpu and env("RXGB_FUSED_GLUE", "1") != "0"
        # depth_step (one C++ call per depth) measures SLOWER than the
        # python-orchestrated fused loop in a same-box interleaved A/B:
        # 2.75-2.96 vs 2.53-2.62 ms/round with the fused glue in both
        # arms (3.23-3.36 vs 3.20-3.21 before the row-order finish and
        # the fused glue). Per-depth python/torch dispatch is not on the
        # critical path, and depth_step still partitions the last level,
        # which the row-order finish skips in the python loop. Kept
        # opt-in (RXGB_DEPTH_STEP=1).
        want_depth_step = env("RXGB_DEPTH_STEP") == "1"
        use_depth_step = (
            use_fused_loop and not self.coll.is_distributed
            and want_depth_step
        )
        # whole-tree enqueue: ONE call puts every level's launches on the
        # stream - depth d+1 reads its frontier from what a device kernel
        # planned at depth d - and the host only replays each depth's
        # bookkeeping from that depth's pinned pull, behind the GPU.
        # Taken only where no per-depth host input exists (no monotone /
        # interaction constraints, no per-level or per-node column
        # sampling, single process) and the frontier bound 2^depth fits
        # the single-workgroup plan kernels.
        tree_enq = (
            use_fused_loop and row_finish and fused_glue
            and env("RXGB_TREE_ENQUEUE", "1") != "0"
            and not want_depth_step
            and not self.coll.is_distributed
            and self.mono is None
            and self.interaction_sets is None
            and self.p.colsample_bylevel >= 1.0
            and self.p.colsample_bynode >= 1.0
            and 1 <= self.p.max_depth <= 10
            and n_local > 0
        )
        if tree_enq:
            tree_enq = bool(_hip().tree_enqueue_config(
                self.dtrain.bins, self.n_bins)[0])
        return _Route(use_fused_loop, row_finish, fused_glue, tree_enq,
                      use_depth_step)

    def _grow_tree(
        self, gpair: torch.Tensor, it: int, cls: int, ptree: int = 0
    ) -> Tree:
        prof = _PhaseTimer(self.device)
        key = cls + 101 * ptree  # this tree's row/column sampling stream
        self._mvs_ridx = None
        if (self.p.sampling_method == "gradient_based"
                and self.p.subsample < 1.0):
            # sample first: the reweighted pairs are what gets quantised
            gpair = self._mvs_sample(gpair, it, key)
            prof.tick("mvs_sample")
        gq, scale_g, scale_h = self._quantize(gpair)
        prof.tick("quantize")
        if self._approx:
            self._resketch(gq)
            prof.tick("sketch")
        self._scale_g_cur = scale_g
        self._leaf_segs = []
        self._leaf_nids = []
        if self.p.grow_policy == "lossguide":
            self.last_tree_path = "lossguide"
            return self._grow_tree_lossguide(gq, scale_g, scale_h, it, cls, ptree)
        ridx, gseg, root_sum = self._tree_rows(gq, it, key)
        feat_mask = self._sample_features(it, key)
        n_local = int(ridx.numel())

        route = self._tree_route(n_local)
        self.last_tree_path = "enqueue" if route.tree_enq else "per_depth"
        st = _TreeGrow(it, cls, route, scale_g, scale_h, feat_mask, ridx,
                       gseg, prof)
        st.ta = _TreeArrays(max(64, 2 ** min(self.p.max_depth + 2, 16)))
        st.cuts = (self.dtrain.cuts.cuts_flat.cpu().numpy(),
                   self.dtrain.cuts.cut_ptr.cpu().numpy())
        if self.mono is not None:
            st.mono = (self.mono.cpu().numpy().astype(np.int64), scale_g,
                       scale_h, float(self.p.reg_lambda),
                       float(self.p.reg_alpha))
        track_paths = self.interaction_sets is not None
        if route.tree_enq:
            # the root sums stay on the device and ride the depth-0 pull
            fr = _Frontier.root(n_local, 0, 0, track_paths)
            st.enq_pull = self._enqueue_tree(st, root_sum)
        else:
            fr = _Frontier.root(n_local, int(root_sum[0]),
                                int(root_sum[1]), track_paths)

        for depth in range(self.p.max_depth):
            fr = self._grow_level(st, fr, depth)
            if fr is None:  # no node of the level split
                break
        if fr is not None:
            # remaining frontier nodes (max depth reached) become leaves
            self._finalize_leaves_soa(st.ta, fr, None, scale_h,
                                      parity=st.cur_buf)
        ridx_a, ridx_b = st.ridx_bufs or (st.ridx, None)
        if self._adaptive and self._leaf_segs:
            st.ta.val[np.asarray(self._leaf_nids, np.int64)] = (
                self._adaptive_leaf_values(
                    cls, ridx_a, ridx_b,
                    [bp for (s, c, v, bp) in self._leaf_segs]
                    if ridx_b is not None else None,
                )
            )
        prof.tick("leaf_host")
        tree = st.ta.to_tree()
        self._finish_tree(tree, st.ta.split_bin[: st.ta.n], cls, n_local,
                          route.row_finish, ridx_a, ridx_b)
        prof.tick("margins")
        prof.report()
        return tree

    def _grow_level(self, st, fr, depth):
        """One depth: best splits of the frontier by the tree's route, leaf
        and split bookkeeping, and the children as the next frontier (None
        when no node split)."""
        route = st.route
        lvl = fr.in_build_order(depth)
        fb, allowed_m = self._level_gates(st, lvl, depth)
        # row-order finish: this level's children are leaves, so only
        # the histogram, the scan and the split pull run for it
        last_level = (
            route.row_finish and not route.use_depth_step
            and depth == self.p.max_depth - 1
        )
        # (the whole-tree enqueue owns its two ping-pong histograms)
        all_hist = None if route.tree_enq else torch.empty(
            (lvl.size, self.dtrain.n_features, self.n_bins, 2),
            dtype=torch.int64, device=self.device,
        )
        if route.tree_enq:
            sp = self._splits_enqueued(st, lvl, depth, last_level)
        elif route.use_depth_step:
            sp = self._splits_depth_step(st, lvl, fb, allowed_m, all_hist)
        else:
            self._level_histogram(st, lvl, all_hist)
            sp = self._scan_and_partition(st, lvl, fb, allowed_m, all_hist,
                                          last_level)

        # ---- vectorized split/leaf decision for the whole frontier
        splits_ok = (sp.gain > 0) & (sp.feature >= 0) & np.isfinite(sp.gain)
        okf = np.nonzero(splits_ok)[0]  # ascending == scan-slot order
        leaf_idx = np.nonzero(~splits_ok)[0]
        if okf.size == 0:
            self._finalize_leaves_soa(st.ta, lvl, leaf_idx, st.scale_h,
                                      parity=sp.in_buf)
            return None

        sf32 = sp.feature[okf].astype(np.int32)
        finish_partition = None
        if sp.left_counts is None and not last_level:
            # launch the partition's count+prefix FIRST (GPU): the leaf
            # finalization and tree-array writes below then run on the
            # host while those kernels execute, and the children
            # bookkeeping after the finish overlaps the scatter
            finish_partition = self._deferred_partition(
                st, lvl, okf, sf32, sp.bin[okf].astype(np.int32),
                sp.default_left[okf].astype(np.uint8),
            )
        self._finalize_leaves_soa(st.ta, lvl, leaf_idx, st.scale_h,
                                  parity=sp.in_buf)
        lids = st.ta.record_splits(
            lvl.nid[okf], sp.feature[okf].astype(np.int64),
            sp.bin[okf].astype(np.int64), sp.default_left[okf],
            sp.gain[okf].astype(np.float64),
            lvl.sumh[okf].astype(np.float64) / st.scale_h, *st.cuts,
        )
        st.prof.tick("tree_host")
        if sp.left_counts is not None:
            # the partition already ran on device; its per-split-node
            # left counts rode the single pull, in the same
            # ascending-okf order the plan kernel compacted
            lc = sp.left_counts[: okf.size].astype(np.int64)
        elif last_level:
            # no partition ran: the leaf children's segment starts and
            # counts are placeholders nothing reads
            lc = np.zeros(okf.size, np.int64)
        else:
            lc = finish_partition()
        st.prof.tick("partition")
        st.prev_hist = all_hist
        return lvl.children(okf, lids, sf32, lc, sp.left_g[okf],
                            sp.left_h[okf], st.mono)

    def _level_gates(self, st, lvl, depth):
        """(per-feature bin counts, [KK, F] uint8 per-node gate or None) of
        one level: column sampling and interaction constraints."""
        mask = st.feat_mask
        if self.p.colsample_bylevel < 1.0:
            lvl_mask = self._sample_features(st.it, st.cls, level=depth)
            mask = lvl_mask if mask is None else (mask & lvl_mask)
        # (the whole-tree enqueue took its gate when it was launched)
        fb = (self.feat_bins if st.route.tree_enq
              else self._gated_feat_bins(mask))
        allowed_m = (
            self._allowed_mask(lvl.paths) if lvl.paths is not None else None
        )
        if self.p.colsample_bynode < 1.0:
            # per-node feature sampling (xgboost colsample_bynode):
            # deterministic in (seed, iteration, class, depth) and
            # in scan-slot order, so every rank draws the same masks
            node_m = self._bynode_mask(lvl.size, st.it, st.cls, depth)
            allowed_m = (
                node_m if allowed_m is None
                else (allowed_m.to(torch.uint8) & node_m)
            )
        return fb, allowed_m

    def _enqueue_tree(self, st, root_sum):
        """Launch every level of the tree; returns the pinned pull all
        depths write to (``_splits_enqueued`` reads one slot per depth)."""
        fb_tree = self._gated_feat_bins(st.feat_mask)
        return _hip().tree_enqueue(
            self.dtrain.bins,
            self._or_empty(getattr(self.dtrain, "bins_t", None),
                           torch.uint8),
            st.gseg, st.ridx_bufs[0], st.ridx_bufs[1], root_sum,
            self.p.max_depth,
            fb_tree.to(self.device).to(torch.int32).contiguous(),
            st.scale_g, st.scale_h, self.p.reg_lambda, self.p.reg_alpha,
            self.p.gamma, self.p.min_child_weight, self.n_bins,
        ).numpy()

    def _splits_enqueued(self, st, lvl, depth, last_level):
        """Whole-tree enqueue: everything is already on the stream. Wait
        for THIS depth's pull (its own pinned slot and event) and decode
        it while the GPU runs the deeper levels."""
        _hip().tree_enqueue_wait(depth)
        KKb = 1 << depth  # the slot is laid out on the bound
        if depth == 0:
            lvl.sumg[0] = st.enq_pull[0]
            lvl.sumh[0] = st.enq_pull[1]
        arr = st.enq_pull[2 + 7 * (KKb - 1): 2 + 7 * (2 * KKb - 1)]
        # the last level of the row-order finish was not partitioned
        sp = _decode_pull(arr, lvl.size, 6 * KKb,
                          0 if last_level else st.flip(),
                          with_counts=not last_level)
        st.prof.tick("scan_pull")
        return sp

    def _splits_depth_step(self, st, lvl, fb, allowed_m, all_hist):
        """One C++ call per depth: stage + zero + hist + derive + scan +
        device-planned partition + pull + scatter. The ~30 per-depth
        python/torch dispatches were ~0.8 ms of wall per round at depth 8
        (and still it measures slower: see ``_tree_route``)."""
        KK, K = lvl.size, lvl.K
        has_mono = self.mono is not None
        chunk_bound = (int(lvl.count.sum()) + 2047) // 2048 + KK
        # C++ find_splits takes raw pointers: everything must already be
        # the right dtype ON DEVICE
        st.ridx, st.gseg, pull = _hip().depth_step(
            self.dtrain.bins,
            self._or_empty(getattr(self.dtrain, "bins_t", None),
                           torch.uint8),
            self._or_empty(st.gseg, torch.int32, (0, 2)),
            st.ridx, st.ridx_bufs[1 - st.cur_buf],
            st.prev_hist if st.prev_hist is not None else all_hist,
            all_hist, torch.from_numpy(lvl.meta()), KK,
            int(lvl.derive_sib_pos.size), K,
            torch.from_numpy(np.ascontiguousarray(lvl.start[:K])),
            torch.from_numpy(np.ascontiguousarray(lvl.count[:K])),
            fb.to(self.device).to(torch.int32), st.scale_g, st.scale_h,
            self.p.reg_lambda, self.p.reg_alpha, self.p.gamma,
            self.p.min_child_weight,
            self._or_empty(self.mono, torch.int8),
            self._or_empty(lvl.bounds() if has_mono else None,
                           torch.float64, (0, 2)),
            self._or_empty(allowed_m, torch.uint8),
            self.n_bins, chunk_bound, st.route.fused_glue,
        )
        in_buf = st.flip()
        st.prof.tick("scan")
        _hip().wait_pull_event()
        sp = _decode_pull(pull[: 7 * KK].numpy(), KK, 6 * KK, in_buf)
        st.prof.tick("scan_pull")
        return sp

    def _level_histogram(self, st, lvl, all_hist):
        """Build the level's K built histograms into ``all_hist[:K]`` and
        allreduce them."""
        K = lvl.K
        F = self.dtrain.n_features
        starts = torch.from_numpy(np.ascontiguousarray(lvl.start[:K]))
        counts = torch.from_numpy(np.ascontiguousarray(lvl.count[:K]))
        hist = all_hist[:K]  # built block (contiguous slice)
        hist.zero_()  # derived rows overwritten by the sub
        overlap = self.coll.is_distributed and (
            (
                self.device.type == "cuda"
                and self.dtrain.bins.stride(0) % 16 == 0
                and F > 16
            )
            or os.environ.get("RXGB_FORCE_OVERLAP_ALLREDUCE") == "1"
        )
        if overlap:
            # overlap the RCCL AllReduce of each finished feature block
            # with the build of the next (BASELINE north-star: side-
            # stream collective over xGMI behind the histogram build)
            n_chunks = min(4, (F + 31) // 32)
            step = ((F + n_chunks - 1) // n_chunks + 15) // 16 * 16
            pending = []
            f0 = 0
            while f0 < F:
                f1 = min(f0 + step, F)
                ops.build_histogram(
                    self.dtrain.bins, st.gseg, st.ridx, starts, counts,
                    self.n_bins, f_range=(f0, f1), out=hist,
                    pregathered=True,
                )
                sl = hist[:, f0:f1].contiguous()
                pending.append((self.coll.allreduce_async(sl), sl, f0, f1))
                f0 = f1
            for h, sl, c0, c1 in pending:
                h.wait()
                hist[:, c0:c1].copy_(sl)
        else:
            ops.build_histogram(
                self.dtrain.bins, st.gseg, st.ridx, starts, counts,
                self.n_bins, out=hist, pregathered=True,
            )
            st.prof.tick("hist")
            if self.coll.is_distributed:
                self.coll.allreduce_(hist)
        st.prof.tick("allreduce")

    def _scan_and_partition(self, st, lvl, fb, allowed_m, all_hist,
                            last_level):
        """Stage the level's control data, derive the sibling histograms,
        scan for the best splits and - in the one-sync loop - partition
        the rows by them on the device."""
        KK, K = lvl.size, lvl.K
        nd = lvl.derive_sib_pos.size
        fused_glue = st.route.fused_glue
        if self.device.type == "cuda":
            # ONE H2D for this depth's control data
            depth_meta = self._stage_i64(lvl.meta(), "depth_meta")
            pg, ph = depth_meta[:KK], depth_meta[KK : 2 * KK]
            d_starts = depth_meta[2 * KK : 3 * KK]
            d_counts = depth_meta[3 * KK : 4 * KK]
            pslots = depth_meta[4 * KK : 4 * KK + nd]
            spos = depth_meta[4 * KK + nd :]
        else:
            pg = torch.from_numpy(lvl.sumg)
            ph = torch.from_numpy(lvl.sumh)
            pslots = torch.from_numpy(lvl.derive_pslot)
            spos = torch.from_numpy(lvl.derive_sib_pos)
        derive_kw = {}
        if nd and fused_glue:
            # sibling = parent - built inside the scan kernel,
            # which stores the derived rows for the next depth
            derive_kw = dict(
                prev_hist=st.prev_hist, pslots=pslots, spos=spos
            )
        elif nd:
            # sibling = parent - built, batched over all pairs
            torch.sub(
                st.prev_hist.index_select(0, pslots),
                all_hist.index_select(0, spos),
                out=all_hist[K:],
            )
        st.prof.tick("stack")
        scan_args = (
            all_hist, pg, ph, fb, st.scale_g, st.scale_h,
            self.p.reg_lambda, self.p.reg_alpha, self.p.gamma,
            self.p.min_child_weight,
        )
        scan_kw = dict(
            monotone=self.mono,
            bounds=lvl.bounds() if self.mono is not None else None,
            allowed=allowed_m, **derive_kw,
        )
        if not st.route.use_fused_loop or last_level:
            # 2-sync / CPU / unpartitioned last level: pull the splits;
            # the caller partitions by them where children need rows
            best = ops.find_splits(*scan_args, **scan_kw)
            st.prof.tick("scan")
            st.prof.tick("scan_pull")
            return _LevelSplits(
                best["gain"], best["feature"], best["bin"],
                best["default_left"], best["left_g"], best["left_h"],
                None, 0,
            )
        # single-sync fused path (GPU, default): the split scan's
        # packed output feeds a device-planned partition directly;
        # ONE pinned D2H brings {splits | left_counts} to the host,
        # which replays the identical split predicate for
        # bookkeeping. The pull is enqueued BEFORE the scatter and
        # the host waits on an inter-launch EVENT, so it wakes
        # right after count+prefix and every piece of bookkeeping
        # overlaps the scatter: measured d8 3.56-3.61 vs 3.72-3.73
        # ms/round for the 2-sync structure (the first version
        # synced past the scatter and was SLOWER - see
        # profiles/README.md pass 5/8). RXGB_ONE_SYNC=0 restores
        # the 2-sync path.
        packed_dev = ops.find_splits(
            *scan_args, pull=False, reduce=not fused_glue, **scan_kw
        )
        st.prof.tick("scan")
        # grid BOUND: every split node adds at most one
        # partial chunk (PART_CHUNK = 2048 rows/workgroup)
        chunk_bound = (int(lvl.count.sum()) + 2047) // 2048 + KK
        # fused glue: packed_dev is the (node, feature) scan
        # tuple, reduced inside the partition's plan kernel
        part_fn = (
            ops.partition_rows_from_kf if fused_glue
            else ops.partition_rows_from_packed
        )
        part_kw = {} if fused_glue else {"fused_glue": False}
        st.ridx, st.gseg, pull, pull_ev = part_fn(
            self.dtrain.bins, st.ridx, d_starts, d_counts, packed_dev,
            st.gseg, getattr(self.dtrain, "bins_t", None), chunk_bound,
            ridx_dest=st.ridx_bufs[1 - st.cur_buf], **part_kw,
        )
        in_buf = st.flip()
        # event recorded between the pull D2H and the scatter:
        # the host wakes before the scatter and every piece of
        # bookkeeping in the caller overlaps it
        pull_ev.synchronize()
        sp = _decode_pull(pull[: 7 * KK].numpy(), KK, 6 * KK, in_buf)
        st.prof.tick("scan_pull")
        return sp

    def _deferred_partition(self, st, lvl, okf, sf32, sb32, sdl8):
        """Partition the rows of the split slots ``okf`` where the scan
        did not (2-sync GPU route, CPU). On the GPU the count+prefix
        kernels are launched here. Returns the function that completes
        the partition (left-totals pull + scatter; the whole partition on
        the CPU) and returns the left counts."""
        args = (
            self.dtrain.bins, st.ridx,
            torch.from_numpy(np.ascontiguousarray(lvl.start[okf])),
            torch.from_numpy(np.ascontiguousarray(lvl.count[okf])),
            torch.from_numpy(sf32), torch.from_numpy(sb32),
            torch.from_numpy(sdl8),
        )
        kw = dict(gpair_seg=st.gseg,
                  bins_t=getattr(self.dtrain, "bins_t", None))
        if self.device.type == "cuda":
            ctx = ops.partition_begin(*args, **kw)

            def finish():
                st.ridx, left_counts, st.gseg = ops.partition_finish(ctx)
                return left_counts.numpy().astype(np.int64)
        else:
            def finish():
                st.ridx, left_counts, st.gseg = ops.partition_rows(
                    *args, **kw)
                return left_counts.cpu().numpy().astype(np.int64)
        return finish

    # which loop grew the last tree: "enqueue" (whole-tree enqueue),
    # "per_depth" or "lossguide"
    last_tree_path: Optional[str] = None
    _leaf_segs: List[Tuple[int, int, float]] = []
    _leaf_nids: List[int] = []  # node id of each _leaf_segs entry


    def _finalize_leaves_soa(self, ta, fr, idx, scale_h, parity=0):
        """Make the nodes ``fr[idx]`` (all of ``fr`` for None) leaves: same
        math/op order as the scalar _calc_weight, writing into _TreeArrays
        and collecting (start, count, value, ridx buffer) margin
        segments."""
        sel = slice(None) if idx is None else idx
        nids = fr.nid[sel]
        if nids.size == 0:
            return
        starts, counts = fr.start[sel], fr.count[sel]
        wlo, whi = fr.wlo[sel], fr.whi[sel]
        G = fr.sumg[sel].astype(np.float64) / self._scale_g_cur
        H = fr.sumh[sel].astype(np.float64) / scale_h
        lam = self.p.reg_lambda
        alpha = self.p.reg_alpha
        denom = H + lam
        Gs = G
        if alpha > 0:
            Gs = np.copysign(np.maximum(np.abs(G) - alpha, 0.0), G)
        w = np.where(denom > 0, -Gs / np.where(denom > 0, denom, 1.0), 0.0)
        if self.mono is not None:
            w = np.clip(w, wlo, whi)
        if self.p.max_delta_step > 0:
            w = np.clip(w, -self.p.max_delta_step, self.p.max_delta_step)
        v = self.p.eta * w
        ta.val[nids] = v
        ta.cover[nids] = H
        self._leaf_nids.extend(nids.tolist())
        self._leaf_segs.extend(
            zip(starts.tolist(), counts.tolist(), v.tolist(),
                [parity] * int(nids.size))
        )

    # -- evaluation ----------------------------------------------------------
    def eval_sets(self, evals: Sequence[EvalPack], feval=None) -> Dict[str, Dict[str, float]]:
        metric_names = list(self.p.eval_metric)
        if not metric_names and not self.p.disable_default_eval_metric:
            metric_names = [self.obj.default_metric]
        out: Dict[str, Dict[str, float]] = {}
        local_stats = []
        specs = []
        for ev in evals:
            margin = self.margin if ev.X is None else ev.margin
            label = self._train_label if ev.X is None else ev.label
            weight = self.dtrain.weight if ev.X is None else ev.weight
            qid = self.dtrain.qid if ev.X is None else ev.qid
            for mname in metric_names:
                m = get_metric(mname)
                st = m.local_stats(margin, label, weight, qid, self.obj)
                local_stats.append(st)
                specs.append((ev.name, m))
        if specs:
            flat = torch.cat([s.flatten() for s in local_stats])
            if self.coll.is_distributed:
                flat_d = flat.to(self.device) if self.device.type == "cuda" else flat
                self.coll.allreduce_(flat_d)
                flat = flat_d.cpu()
            pos = 0
            for (ename, m), st in zip(specs, local_stats):
                sz = st.numel()
                val = m.finalize(flat[pos : pos + sz])
                pos += sz
                out.setdefault(ename, {})[m.name] = val
        if feval is not None:
            for ev in evals:
                margin = self.margin if ev.X is None else ev.margin
                label = self.dtrain.label if ev.X is None else ev.label

                class _Shim:
                    def __init__(self, l):
                        self._l = l

                    def get_label(self):
                        return self._l

                name, val = feval(
                    margin.cpu().numpy(),
                    _Shim(None if label is None else label.cpu().numpy()),
                )
                val = float(val)
                if self.coll.is_distributed:
                    # a custom feval sees only the local shard; average
                    # across ranks so every rank's early-stopping decision
                    # is identical (rank-divergent stops break collectives)
                    t = torch.tensor(
                        [val], dtype=torch.float64,
                        device=self.device
                        if self.device.type == "cuda" else "cpu",
                    )
                    self.coll.allreduce_(t)
                    val = float(t[0]) / self.coll.world_size
                out.setdefault(ev.name, {})[name] = val
        return out

    def update_eval_margins(self, evals: Sequence[EvalPack], trees, classes):
        """Incrementally add the new round's trees to eval-set margins."""
        if self.p.booster == "dart":
            # _dart_commit rescales previously-added and dropped trees'
            # leaf values in place every round, so incremental margins
            # would drift from the real model (eval logloss reported
            # ~0.18 where the true model scored ~0.24 in a 20-round run).
            # Recompute from the booster: exact by construction, and dart
            # eval sets are small relative to training data.
            for ev in evals:
                if ev.X is None:
                    continue
                pm = self.booster.predict_margin_tensor(ev.X).to(
                    torch.float32
                )
                if ev.base_margin is not None:
                    pm = pm + ev.base_margin.reshape(pm.shape)
                ev.margin = pm
            return
        if self.p.booster == "gblinear":
            for ev in evals:
                if ev.X is None:
                    continue
                for cls, (dwf, db) in enumerate(self._lin_deltas):
                    mv = (ev.margin if self.n_class == 1
                          else ev.margin[:, cls])
                    mv += ev.X @ dwf.to(ev.X.device)
                    mv += db
            return
        for ev in evals:
            if ev.X is None:
                continue
            for t, cls in zip(trees, classes):
                mv = ev.margin if self.n_class == 1 else ev.margin[:, cls]
                flat_feat = torch.from_numpy(t.feat).to(ev.X.device)
                ops.predict_trees(
                    ev.X,
                    flat_feat,
                    torch.from_numpy(t.thr).to(ev.X.device),
                    torch.from_numpy(t.left).to(ev.X.device),
                    torch.from_numpy(t.default_left).to(ev.X.device),
                    torch.from_numpy(t.value).to(ev.X.device),
                    torch.tensor([0, t.num_nodes], dtype=torch.int32),
                    mv,
                )

    def init_eval_margins(self, evals: Sequence[EvalPack], model: Optional[Booster]):
        for ev in evals:
            if ev.X is None:
                continue
            n = ev.X.shape[0]
            shape = (n,) if self.n_class == 1 else (n, self.n_class)
            ev.margin = torch.full(
                shape,
                self.base_margin_const,
                dtype=torch.float32,
                device=ev.X.device,
            )
            if ev.base_margin is not None:
                ev.margin += ev.base_margin.reshape(shape)
            if model is not None and model.trees:
                pm = model.predict_margin_tensor(ev.X)
                ev.margin = pm.to(torch.float32) + (
                    ev.base_margin.reshape(shape) if ev.base_margin is not None else 0
                )

    def _grow_tree_lossguide(self, gq, scale_g, scale_h, it, cls, ptree):
        """Leaf-wise (best-gain-first) growth - grow_policy=lossguide with
        max_leaves (XGBoost/LightGBM semantics). Each expansion partitions
        one leaf segment and histograms the smaller child (sibling by
        subtraction); the expansion order is driven by the globally
        identical scan gains, so all ranks grow the same tree."""
        import heapq

        ridx, gseg, root_sum = self._tree_rows(gq, it, cls + 101 * ptree)
        n_local = int(ridx.numel())
        fb = self._gated_feat_bins(
            self._sample_features(it, cls + 101 * ptree))
        cuts_flat_cpu = self.dtrain.cuts.cuts_flat.cpu().numpy()
        cut_ptr_cpu = self.dtrain.cuts.cut_ptr.cpu().numpy()
        max_leaves = self.p.max_leaves or (1 << 30)
        max_depth = self.p.max_depth if self.p.max_depth > 0 else 64

        feat_l, thr_l = [-1], [0.0]
        left_l, dl_l, val_l, gain_l, cover_l = [-1], [0], [0.0], [0.0], [0.0]
        parent_l = [-1]

        def scan_nodes(hists, sums, paths=None):
            best = ops.find_splits(
                hists,
                torch.tensor([sg for sg, sh in sums], dtype=torch.int64,
                             device=self.device),
                torch.tensor([sh for sg, sh in sums], dtype=torch.int64,
                             device=self.device),
                fb, scale_g, scale_h, self.p.reg_lambda, self.p.reg_alpha,
                self.p.gamma, self.p.min_child_weight,
                allowed=self._allowed_mask(paths)
                if paths is not None and self.interaction_sets is not None
                else None,
            )
            return best

        # root
        root_hist = ops.build_histogram(
            self.dtrain.bins, gseg, ridx,
            torch.tensor([0], dtype=torch.int64),
            torch.tensor([n_local], dtype=torch.int64),
            self.n_bins, pregathered=True,
        )
        if self.coll.is_distributed:
            self.coll.allreduce_(root_hist)
        rbest = scan_nodes(root_hist, [(int(root_sum[0]), int(root_sum[1]))],
                           paths=[()])
        heap = []
        counter = [0]

        def push(nid, depth, start, count, sg, sh, hist, best_k, path=()):
            gain = float(best_k["gain"])
            rec = {
                "nid": nid, "depth": depth, "start": start, "count": count,
                "sg": sg, "sh": sh, "hist": hist, "path": path,
                "feature": int(best_k["feature"]), "bin": int(best_k["bin"]),
                "dl": int(best_k["default_left"]),
                "lg": int(best_k["left_g"]), "lh": int(best_k["left_h"]),
            }
            if gain > 0 and np.isfinite(gain) and rec["feature"] >= 0:
                heapq.heappush(heap, (-gain, counter[0], rec))
                counter[0] += 1
            else:
                self._finalize_leaf_rec(rec, val_l, cover_l, scale_h)

        def best_row(best, k):
            return {key: best[key][k] for key in best}

        push(0, 0, 0, n_local, int(root_sum[0]), int(root_sum[1]),
             root_hist[0], best_row(rbest, 0))
        n_leaves = 1
        while heap and n_leaves < max_leaves:
            neg_gain, _cnt, rec = heapq.heappop(heap)
            nid = rec["nid"]
            f, b = rec["feature"], rec["bin"]
            thr = float(cuts_flat_cpu[cut_ptr_cpu[f] + b])
            lid = len(feat_l)
            feat_l[nid] = f
            thr_l[nid] = thr
            left_l[nid] = lid
            dl_l[nid] = rec["dl"]
            gain_l[nid] = -neg_gain
            cover_l[nid] = rec["sh"] / scale_h
            for _i in range(2):
                feat_l.append(-1)
                thr_l.append(0.0)
                left_l.append(-1)
                dl_l.append(0)
                val_l.append(0.0)
                gain_l.append(0.0)
                cover_l.append(0.0)
                parent_l.append(nid)
            ridx, left_counts, gseg = ops.partition_rows(
                self.dtrain.bins, ridx,
                torch.tensor([rec["start"]], dtype=torch.int64),
                torch.tensor([rec["count"]], dtype=torch.int64),
                torch.tensor([f], dtype=torch.int32),
                torch.tensor([b], dtype=torch.int32),
                torch.tensor([rec["dl"]], dtype=torch.uint8),
                gpair_seg=gseg,
                bins_t=getattr(self.dtrain, "bins_t", None),
            )
            lcount = int(left_counts[0])
            lsums = (rec["lg"], rec["lh"])
            rsums = (rec["sg"] - rec["lg"], rec["sh"] - rec["lh"])
            lseg = (rec["start"], lcount)
            rseg = (rec["start"] + lcount, rec["count"] - lcount)
            children = [
                (lid, rec["depth"] + 1) + lseg + lsums,
                (lid + 1, rec["depth"] + 1) + rseg + rsums,
            ]
            # build the (globally) smaller child, derive the sibling
            small_i = 0 if lsums[1] <= rsums[1] else 1
            sc = children[small_i]
            sh_hist = ops.build_histogram(
                self.dtrain.bins, gseg, ridx,
                torch.tensor([sc[2]], dtype=torch.int64),
                torch.tensor([sc[3]], dtype=torch.int64),
                self.n_bins, pregathered=True,
            )
            if self.coll.is_distributed:
                self.coll.allreduce_(sh_hist)
            other_hist = rec["hist"] - sh_hist[0]
            rec["hist"] = None
            if small_i == 0:
                hists = torch.stack([sh_hist[0], other_hist])
            else:
                hists = torch.stack([other_hist, sh_hist[0]])
            child_path = tuple(sorted(set(rec.get("path", ())) | {f}))
            cbest = scan_nodes(
                hists, [(children[0][4], children[0][5]),
                        (children[1][4], children[1][5])],
                paths=[child_path, child_path],
            )
            for ci, ch in enumerate(children):
                if ch[1] >= max_depth:
                    self._finalize_leaf_rec(
                        {"start": ch[2], "count": ch[3], "sg": ch[4],
                         "sh": ch[5]}, val_l, cover_l, scale_h, nid=ch[0],
                    )
                else:
                    push(ch[0], ch[1], ch[2], ch[3], ch[4], ch[5],
                         hists[ci], best_row(cbest, ci), path=child_path)
            n_leaves += 1

        # drain remaining candidates as leaves
        while heap:
            _, _, rec = heapq.heappop(heap)
            self._finalize_leaf_rec(rec, val_l, cover_l, scale_h)

        if self._adaptive and self._leaf_segs:
            new_vals = self._adaptive_leaf_values(cls, ridx, None, None)
            for nid_i, nv in zip(self._leaf_nids, new_vals.tolist()):
                val_l[nid_i] = nv
        tree = Tree(
            feat=np.asarray(feat_l, np.int32),
            thr=np.asarray(thr_l, np.float32),
            left=np.asarray(left_l, np.int32),
            default_left=np.asarray(dl_l, np.uint8),
            value=np.asarray(val_l, np.float32),
            gain=np.asarray(gain_l, np.float32),
            cover=np.asarray(cover_l, np.float32),
            parent=np.asarray(
                [2147483647 if pp < 0 else pp for pp in parent_l], np.int32
            ),
        )
        self._finish_tree(tree, None, cls, n_local, False, ridx)
        return tree

    def _finalize_leaf_rec(self, rec, val_l, cover_l, scale_h, nid=None):
        nid = rec["nid"] if nid is None else nid
        G = rec["sg"] / self._scale_g_cur
        H = rec["sh"] / scale_h
        w = _calc_weight(G, H, self.p.reg_lambda, self.p.reg_alpha)
        if self.p.max_delta_step > 0:
            w = max(-self.p.max_delta_step, min(self.p.max_delta_step, w))
        val_l[nid] = self.p.eta * w
        cover_l[nid] = H
        self._leaf_segs.append(
            (rec["start"], rec["count"], self.p.eta * w, 0)
        )
        self._leaf_nids.append(nid)

    # quantization scale of the current tree (set in _grow_tree via _quantize)
    _scale_g_cur: float = 1.0


def _calc_weight(G: float, H: float, reg_lambda: float, reg_alpha: float) -> float:
    if H + reg_lambda <= 0:
        return 0.0
    if reg_alpha > 0:
        G = math.copysign(max(abs(G) - reg_alpha, 0.0), G)
    return -G / (H + reg_lambda)


def run_training(
    params: Dict,
    dtrain: BinnedMatrix,
    num_boost_round: int,
    evals: Sequence[EvalPack] = (),
    collective: Optional[Collective] = None,
    rank: int = 0,
    xgb_model: Optional[Booster] = None,
    callbacks=None,
    early_stopping_rounds: Optional[int] = None,
    verbose_eval: Union[bool, int] = False,
    obj: Optional[Callable] = None,
    feval: Optional[Callable] = None,
    maximize: Optional[bool] = None,
    evals_result: Optional[Dict] = None,
) -> Booster:
    """The per-rank training loop (reference: xgb.train inside
    RayXGBoostActor.train, reference main.py:722-752)."""
    engine = BoostingEngine(
        params, dtrain, collective, rank, custom_objective=obj
    )
    if xgb_model is not None:
        engine.load_model(xgb_model)
    engine.init_eval_margins(evals, xgb_model)
    cb = CallbackList(callbacks)
    log: Dict[str, Dict[str, List[float]]] = {}
    best_score, best_iter, stall = None, None, 0
    # explicit maximize (xgboost.train kwarg) wins; otherwise inferred
    # from the last builtin metric, defaulting to False for custom feval
    start_iter = engine.iteration

    for rnd in range(num_boost_round):
        it = engine.iteration
        if cb.before_iteration(engine.booster, it, log):
            break
        trees = engine.update()
        classes = engine.booster.tree_info[-len(trees):] if trees else []
        engine.update_eval_margins(evals, trees, classes)
        if evals:
            results = engine.eval_sets(evals, feval)
            for ename, md in results.items():
                for mname, v in md.items():
                    log.setdefault(ename, {}).setdefault(mname, []).append(v)
            if verbose_eval and rank == 0:
                interval = 1 if verbose_eval is True else int(verbose_eval)
                if it % interval == 0:
                    msg = "\t".join(
                        f"{e}-{m}:{v:.5f}"
                        for e, md in results.items()
                        for m, v in md.items()
                    )
                    print(f"[{it}]\t{msg}", flush=True)
            if early_stopping_rounds:
                last_eval = list(results.keys())[-1]
                last_metric = list(results[last_eval].keys())[-1]
                score = results[last_eval][last_metric]
                if maximize is None:
                    try:
                        maximize = get_metric(
                            last_metric.split("@")[0]
                        ).higher_better
                    except ValueError:
                        maximize = False  # custom feval: assume loss-like
                improved = (
                    best_score is None
                    or (score > best_score if maximize else score < best_score)
                )
                if improved:
                    best_score, best_iter, stall = score, it, 0
                else:
                    stall += 1
                    if stall >= early_stopping_rounds:
                        engine.booster.best_iteration = best_iter
                        engine.booster.best_score = best_score
                        engine.booster.set_attr(
                            best_iteration=str(best_iter),
                            best_score=str(best_score),
                        )
                        break
        if cb.after_iteration(engine.booster, it, log):
            break

    if best_iter is not None and engine.booster.best_iteration is None:
        engine.booster.best_iteration = best_iter
        engine.booster.best_score = best_score
        engine.booster.set_attr(
            best_iteration=str(best_iter), best_score=str(best_score)
        )
    if evals_result is not None:
        evals_result.update(log)
    cb.after_training(engine.booster, engine.iteration - 1, log)
    return engine.booster
