"""Evaluation metrics, designed for distributed evaluation.

Each metric reduces its local shard to a small float64 stats vector that is
summed across workers with one AllReduce (reference semantics: XGBoost's
per-round metric AllReduce inside Rabit), then
finalized identically on every rank. AUC is computed from a fixed
score-histogram (16384 bins) so it needs no global sort; mAP/NDCG reduce
per-query sums.
"""

from typing import Optional

import torch

from xgboost_ray_amd.engine.objectives import rank_hip_layout, sigmoid_sizeinv

_AUC_BINS = 16384


def _fused_eval_ok(margin, max_dim=1):
    """GPU fused metric kernels: one pass instead of 4-6 f64 torch
    kernels over the shard (RXGB_FUSED_EVAL=0 disables). ``max_dim=2``
    admits the [n, K] margin of a multi-target quantile model."""
    import os

    return (
        margin.is_cuda
        and 1 <= margin.dim() <= max_dim
        and os.environ.get("RXGB_FUSED_EVAL") != "0"
    )


def _fused_pointwise(margin, label, weight, obj, kind, param=0.0,
                     on_pred=True):
    """``ops.eval_pointwise`` sums f64 [sum w * loss, sum w] when the margin
    is a float32 GPU vector with a label vector of its length, else None.
    ``on_pred``: the metric is defined on predictions, so the objective's
    ``eval_transform`` stands in for ``_eval_pred``; an objective without a
    named transform keeps the torch metric."""
    transform = "identity"
    if on_pred and obj is not None:
        transform = getattr(obj, "eval_transform", None)
    if (transform is None or not _fused_eval_ok(margin)
            or margin.dtype != torch.float32
            or label.dtype != torch.float32
            or label.shape != margin.shape):
        return None
    from xgboost_ray_amd import ops

    return ops.eval_pointwise(margin, label, weight, kind, transform, param)


class Metric:
    name = "base"
    higher_better = False

    def local_stats(self, margin, label, weight, qid, obj) -> torch.Tensor:
        raise NotImplementedError

    def finalize(self, stats: torch.Tensor) -> float:
        raise NotImplementedError


def _w(label, weight):
    if weight is None:
        return torch.ones_like(label, dtype=torch.float64)
    return weight.double()


def _eval_pred(margin, obj):
    """xgboost's EvalTransform semantics: metrics defined on predictions
    (rmse/mae/mphe) receive the objective's transformed output — sigmoid for
    logistic, exp for log-link objectives — before the metric is computed
    (XGBoost learner.cc EvalOneIter -> obj_->EvalTransform). Falls back to
    the raw margin when no objective is known or the transform changes the
    shape (multiclass prob matrices, custom objectives)."""
    p = margin.double()
    if obj is None:
        return p
    try:
        t = obj.transform_prediction(p)
    except Exception:
        return p
    return t.double() if t.shape == p.shape else p


class RMSE(Metric):
    name = "rmse"

    def local_stats(self, margin, label, weight, qid, obj):
        fused = _fused_pointwise(margin, label, weight, obj, "se")
        if fused is not None:
            return fused
        pred = _eval_pred(margin, obj)
        w = _w(label, weight)
        se = (w * (pred - label.double()) ** 2).sum()
        return torch.stack([se, w.sum()])

    def finalize(self, s):
        return float(torch.sqrt(s[0] / s[1]))


class MAE(Metric):
    name = "mae"

    def local_stats(self, margin, label, weight, qid, obj):
        fused = _fused_pointwise(margin, label, weight, obj, "ae")
        if fused is not None:
            return fused
        w = _w(label, weight)
        pred = _eval_pred(margin, obj)
        return torch.stack(
            [(w * (pred - label.double()).abs()).sum(), w.sum()]
        )

    def finalize(self, s):
        return float(s[0] / s[1])


class LogLoss(Metric):
    name = "logloss"

    def local_stats(self, margin, label, weight, qid, obj):
        if _fused_eval_ok(margin):
            from xgboost_ray_amd.ops import gpu

            return gpu.eval_logloss(margin, label, weight)
        p = sigmoid_sizeinv(margin.double()).clamp(1e-16, 1 - 1e-16)
        y = label.double()
        w = _w(label, weight)
        ll = -(y * torch.log(p) + (1 - y) * torch.log(1 - p))
        return torch.stack([(w * ll).sum(), w.sum()])

    def finalize(self, s):
        return float(s[0] / s[1])


class BinaryError(Metric):
    name = "error"

    def __init__(self, threshold: float = 0.5):
        self.threshold = threshold
        if threshold != 0.5:
            self.name = f"error@{threshold}"

    def local_stats(self, margin, label, weight, qid, obj):
        p = sigmoid_sizeinv(margin.double())
        w = _w(label, weight)
        wrong = (p > self.threshold).double() != label.double()
        return torch.stack([(w * wrong).sum(), w.sum()])

    def finalize(self, s):
        return float(s[0] / s[1])


def _auc_multiclass_stats(margin, label, weight):
    """Stats of an [n, K] margin: the one-vs-rest score histograms of
    ``ops.eval_auc_multiclass`` as float64, [pos | neg] per class. A GPU
    margin takes the HIP kernels; a CPU margin, and RXGB_FUSED_EVAL=0 (which
    copies the margin to the host: the correctness route, not the fast one),
    take ``ops.cpu``."""
    from xgboost_ray_amd import ops

    if _fused_eval_ok(margin, max_dim=2):
        hist = ops.eval_auc_multiclass(margin, label, weight, _AUC_BINS)
    else:
        hist = ops.cpu.eval_auc_multiclass(
            margin.cpu(), label.cpu(),
            None if weight is None else weight.cpu(), _AUC_BINS,
        ).to(margin.device)
    # kernel layout [neg | pos] -> metric layout [pos | neg]
    return hist.flip(1).reshape(-1).double()


def _binned_roc_auc(pos, neg):
    # iterate bins ascending: AUC = sum over bins of
    # neg_below * pos_here + 0.5 * neg_here * pos_here
    cneg = torch.cumsum(neg, 0) - neg
    auc = (cneg * pos).sum() + 0.5 * (neg * pos).sum()
    denom = pos.sum() * neg.sum()
    return float(auc / denom) if denom > 0 else 0.5


def _binned_pr_auc(pos, neg):
    tot_pos = pos.sum()
    if float(tot_pos) <= 0:
        return 0.0
    # descending-score sweep: cumulative TP/FP from the top bin down
    tp = torch.flip(torch.cumsum(torch.flip(pos, [0]), 0), [0])
    fp = torch.flip(torch.cumsum(torch.flip(neg, [0]), 0), [0])
    recall = tp / tot_pos
    prec = tp / torch.clamp(tp + fp, min=1e-300)
    # integrate precision d(recall) over bins, descending threshold:
    # recall increases as the threshold drops
    r = torch.flip(recall, [0])
    p = torch.flip(prec, [0])
    dr = torch.diff(r, prepend=torch.zeros(1, dtype=r.dtype,
                                           device=r.device))
    return float((p * dr).sum())


def _one_vs_rest(s, area, empty):
    """``area(pos, neg)`` of a stats vector: the binary value for one pair of
    planes; for K pairs the average weighted by each class's positive mass,
    over the classes that have both positive and negative mass (``empty`` if
    none has)."""
    K = s.numel() // (2 * _AUC_BINS)
    if K <= 1:
        return area(s[:_AUC_BINS], s[_AUC_BINS:])
    total = mass = 0.0
    for c in s.reshape(K, 2, _AUC_BINS):
        p, n = float(c[0].sum()), float(c[1].sum())
        if p > 0 and n > 0:
            total += p * area(c[0], c[1])
            mass += p
    return total / mass if mass > 0 else empty


class AUC(Metric):
    """Binned ROC AUC: weighted pos/neg histograms over sigmoid(margin); for
    an [n, K] margin the prevalence-weighted one-vs-rest average over the
    softmax probabilities."""

    name = "auc"
    higher_better = True

    def local_stats(self, margin, label, weight, qid, obj):
        if margin.dim() == 2:
            return _auc_multiclass_stats(margin, label, weight)
        if weight is None and _fused_eval_ok(margin):
            from xgboost_ray_amd.ops import gpu

            hist = gpu.eval_auc_hist(margin, label, _AUC_BINS)
            # kernel layout [neg | pos] -> metric layout [pos | neg]
            return torch.cat(
                [hist[_AUC_BINS:], hist[:_AUC_BINS]]
            ).double()
        p = sigmoid_sizeinv(margin.double())
        b = torch.clamp((p * _AUC_BINS).long(), max=_AUC_BINS - 1)
        if weight is None:
            # unweighted: integer scatter (native u64 atomics on GPU -
            # the f64 scatter goes through CAS loops and is ~50x slower).
            # One fused scatter into [neg plane | pos plane]: boolean
            # fancy-indexing (b[ypos]) costs a nonzero + sort + two
            # gathers per eval round.
            idx = b + (label > 0.5).long() * _AUC_BINS
            hist = torch.zeros(
                2 * _AUC_BINS, dtype=torch.int64, device=margin.device
            )
            src = torch.ones(
                (), dtype=torch.int64, device=margin.device
            ).expand(idx.shape)
            hist.scatter_add_(0, idx, src)
            return torch.cat([hist[_AUC_BINS:], hist[:_AUC_BINS]]).double()
        w = _w(label, weight)
        pos = torch.zeros(_AUC_BINS, dtype=torch.float64, device=margin.device)
        neg = torch.zeros(_AUC_BINS, dtype=torch.float64, device=margin.device)
        y = label.double()
        pos.scatter_add_(0, b, w * y)
        neg.scatter_add_(0, b, w * (1 - y))
        return torch.cat([pos, neg])

    def finalize(self, s):
        return _one_vs_rest(s, _binned_roc_auc, 0.5)


class AUCPR(Metric):
    """Binned PR AUC: precision-recall area via the same score bins as AUC
    (xgboost `aucpr`; reference passes eval_metric through, SURVEY #2.3)."""

    name = "aucpr"
    higher_better = True

    def local_stats(self, margin, label, weight, qid, obj):
        return AUC.local_stats(self, margin, label, weight, qid, obj)

    def finalize(self, s):
        return _one_vs_rest(s, _binned_pr_auc, 0.0)


def _fused_multiclass(margin, label, weight):
    """``ops.eval_multiclass`` sums f64 [sum w*nll, sum w*wrong, sum w] when
    the margin is a 2-D GPU tensor (RXGB_FUSED_EVAL=0 disables), else None."""
    import os

    if (not margin.is_cuda or margin.dim() != 2
            or os.environ.get("RXGB_FUSED_EVAL") == "0"):
        return None
    from xgboost_ray_amd import ops

    return ops.eval_multiclass(margin, label, weight)


class MLogLoss(Metric):
    name = "mlogloss"

    def local_stats(self, margin, label, weight, qid, obj):
        fused = _fused_multiclass(margin, label, weight)
        if fused is not None:
            return fused[::2]
        logp = torch.log_softmax(margin.double(), dim=1)
        w = _w(label, weight)
        ll = -logp[torch.arange(len(label), device=margin.device), label.long()]
        return torch.stack([(w * ll).sum(), w.sum()])

    def finalize(self, s):
        return float(s[0] / s[1])


class MError(Metric):
    name = "merror"

    def local_stats(self, margin, label, weight, qid, obj):
        fused = _fused_multiclass(margin, label, weight)
        if fused is not None:
            return fused[1:]
        pred = margin.argmax(dim=1)
        w = _w(label, weight)
        wrong = (pred != label.long()).double()
        return torch.stack([(w * wrong).sum(), w.sum()])

    def finalize(self, s):
        return float(s[0] / s[1])


class _PerGroupMetric(Metric):
    """Mean of a per-group score. On the GPU the scores of all groups come
    from one HIP launch (``ops.rank_group_stats``); the per-group torch loop
    serves CPU tensors, groups longer than ``ops.RANK_LDS_MAX_GROUP`` and
    RXGB_RANK_GPU=0. ``last_route`` names the one that ran."""

    higher_better = True
    last_route = None
    hip_k = 0  # truncation level handed to rank_group_stats

    def group_score(self, m, y) -> float:
        raise NotImplementedError

    def hip_scores(self, stats) -> torch.Tensor:
        """Per-group scores from the [G, 4] rank_group_stats sums."""
        raise NotImplementedError

    def local_stats(self, margin, label, weight, qid, obj):
        layout = rank_hip_layout(margin, qid)
        if layout is None:
            self.last_route = "torch"
            return self._local_stats_torch(margin, label, weight, qid, obj)
        from xgboost_ray_amd import ops

        y = label.contiguous().float()
        _, stats = ops.rank_group_stats(
            margin.contiguous().float(), y, layout[0],
            ops.rank_disc_table(margin.device), self.hip_k,
            max_len=layout[1])
        scores = self.hip_scores(stats)
        self.last_route = "hip"
        return torch.stack([scores.sum(), scores.new_tensor(len(scores))])

    def _local_stats_torch(self, margin, label, weight, qid, obj):
        if qid is None:
            qid = torch.zeros(len(label), dtype=torch.int64, device=margin.device)
        total = torch.zeros(2, dtype=torch.float64, device=margin.device)
        change = torch.ones_like(qid, dtype=torch.bool)
        change[1:] = qid[1:] != qid[:-1]
        starts = torch.nonzero(change).flatten().tolist() + [len(qid)]
        for gi in range(len(starts) - 1):
            s, e = starts[gi], starts[gi + 1]
            total[0] += self.group_score(margin[s:e], label[s:e])
            total[1] += 1
        return total

    def finalize(self, s):
        return float(s[0] / s[1]) if s[1] > 0 else 0.0


class NDCG(_PerGroupMetric):
    name = "ndcg"

    def __init__(self, k: Optional[int] = None):
        self.k = k
        self.hip_k = k or 0
        if k:
            self.name = f"ndcg@{k}"

    def hip_scores(self, stats):
        dcg, idcg = stats[:, 0], stats[:, 1]
        return torch.where(idcg > 0, dcg / idcg, torch.ones_like(dcg))

    def group_score(self, m, y):
        n = len(y)
        k = min(self.k or n, n)
        order = torch.argsort(m.double(), descending=True, stable=True)
        gains = torch.pow(2.0, y.double()) - 1.0
        disc = 1.0 / torch.log2(
            torch.arange(n, device=m.device, dtype=torch.float64) + 2.0
        )
        dcg = (gains[order][:k] * disc[:k]).sum()
        ideal, _ = torch.sort(gains, descending=True)
        idcg = (ideal[:k] * disc[:k]).sum()
        return float(dcg / idcg) if idcg > 0 else 1.0


class MAP(_PerGroupMetric):
    name = "map"

    def hip_scores(self, stats):
        # ap >= 1 / L with a relevant row, and exactly 0 without one
        ap = stats[:, 3]
        return torch.where(ap > 0, ap, torch.ones_like(ap))

    def group_score(self, m, y):
        order = torch.argsort(m.double(), descending=True, stable=True)
        rel = (y[order] > 0).double()
        if rel.sum() == 0:
            return 1.0
        csum = torch.cumsum(rel, 0)
        ranks = torch.arange(1, len(y) + 1, device=m.device, dtype=torch.float64)
        ap = ((csum / ranks) * rel).sum() / rel.sum()
        return float(ap)



class PoissonNLogLik(Metric):
    name = "poisson-nloglik"
    higher_better = False

    def local_stats(self, margin, label, weight, qid, obj):
        fused = _fused_pointwise(margin, label, weight, obj, "poisson",
                                 on_pred=False)
        if fused is not None:
            return fused
        mu = torch.exp(margin.double()).clamp(min=1e-16)
        y = label.double()
        nll = mu - y * torch.log(mu) + torch.lgamma(y + 1.0)
        w = _w(label, weight)
        return torch.stack([(w * nll).sum(), w.sum()])

    def finalize(self, s):
        return float(s[0] / s[1])


class GammaNLogLik(Metric):
    name = "gamma-nloglik"
    higher_better = False

    def local_stats(self, margin, label, weight, qid, obj):
        fused = _fused_pointwise(margin, label, weight, obj, "gamma",
                                 on_pred=False)
        if fused is not None:
            return fused
        mu = torch.exp(margin.double()).clamp(min=1e-16)
        y = label.double()
        nll = y / mu + torch.log(mu)
        w = _w(label, weight)
        return torch.stack([(w * nll).sum(), w.sum()])

    def finalize(self, s):
        return float(s[0] / s[1])


class TweedieNLogLik(Metric):
    higher_better = False

    def __init__(self, rho: float = 1.5):
        self.rho = float(rho)
        self.name = f"tweedie-nloglik@{self.rho}"

    def local_stats(self, margin, label, weight, qid, obj):
        fused = _fused_pointwise(margin, label, weight, obj, "tweedie",
                                 self.rho, on_pred=False)
        if fused is not None:
            return fused
        m = margin.double()
        y = label.double()
        r = self.rho
        nll = -y * torch.exp((1.0 - r) * m) / (1.0 - r) + torch.exp(
            (2.0 - r) * m
        ) / (2.0 - r)
        w = _w(label, weight)
        return torch.stack([(w * nll).sum(), w.sum()])

    def finalize(self, s):
        return float(s[0] / s[1])


class RMSLE(Metric):
    name = "rmsle"
    higher_better = False

    def local_stats(self, margin, label, weight, qid, obj):
        fused = _fused_pointwise(margin, label, weight, obj, "sle")
        if fused is not None:
            return fused
        p = torch.clamp(_eval_pred(margin, obj), min=-1.0 + 1e-6)
        d = torch.log1p(p) - torch.log1p(label.double())
        w = _w(label, weight)
        return torch.stack([(w * d * d).sum(), w.sum()])

    def finalize(self, s):
        import math

        return float(math.sqrt(s[0] / s[1]))



class AFTNLogLik(Metric):
    """survival:aft negative log likelihood; label is the [n, 2]
    (lower, upper) bound stack the engine builds for AFT training."""

    name = "aft-nloglik"
    higher_better = False

    def local_stats(self, margin, label, weight, qid, obj):
        from xgboost_ray_amd.engine.objectives import AFT

        o = obj if isinstance(obj, AFT) else AFT()
        if _fused_eval_ok(margin):
            from xgboost_ray_amd import ops

            return ops.eval_aft(margin, label, weight, o.dist, o.sigma)
        nll = o.nll(margin.double(), label[:, 0].double(),
                    label[:, 1].double())
        w = _w(label[:, 0], weight)
        return torch.stack([(w * nll).sum(), w.sum()])

    def finalize(self, s):
        return float(s[0] / s[1])



class CoxNLogLik(Metric):
    """Breslow negative partial log likelihood per event (local shard)."""

    name = "cox-nloglik"
    higher_better = False

    def local_stats(self, margin, label, weight, qid, obj):
        if _fused_eval_ok(margin):
            from xgboost_ray_amd import ops

            return ops.eval_cox(margin, ops.cox_layout(label))
        t = label.abs().double()
        event = label > 0
        m = margin.double()
        shift = m.max()
        eta = torch.exp(m - shift)
        order = torch.argsort(-t, stable=True)
        eta_s = eta[order]
        ev_s = event[order]
        m_s = m[order]
        cum = torch.cumsum(eta_s, 0)
        ll = (m_s[ev_s] - shift - torch.log(
            torch.clamp(cum[ev_s], min=1e-300)
        )).sum()
        n_ev = ev_s.sum()
        return torch.stack([-ll, n_ev.double()])

    def finalize(self, s):
        return float(s[0] / max(float(s[1]), 1.0))



class MAPE(Metric):
    """Mean absolute percentage error (xgboost `mape`)."""

    name = "mape"
    higher_better = False

    def local_stats(self, margin, label, weight, qid, obj):
        fused = _fused_pointwise(margin, label, weight, obj, "ape")
        if fused is not None:
            return fused
        pred = _eval_pred(margin, obj)
        y = label.double()
        w = _w(label, weight)
        ape = (pred - y).abs() / y.abs().clamp(min=1e-10)
        return torch.stack([(w * ape).sum(), w.sum()])

    def finalize(self, s):
        return float(s[0] / s[1])


class MPHE(Metric):
    """Mean pseudo-Huber error (delta = 1)."""

    name = "mphe"
    higher_better = False

    def local_stats(self, margin, label, weight, qid, obj):
        fused = _fused_pointwise(margin, label, weight, obj, "mphe",
                                 on_pred=False)
        if fused is not None:
            return fused
        r = (margin - label).double()
        loss = torch.sqrt(1.0 + r * r) - 1.0
        w = _w(label, weight)
        return torch.stack([(w * loss).sum(), w.sum()])

    def finalize(self, s):
        return float(s[0] / s[1])


class Quantile(Metric):
    """Weighted pinball loss averaged over rows and alphas (xgboost
    `quantile`); the alphas come from the reg:quantileerror objective."""

    name = "quantile"
    higher_better = False

    def local_stats(self, margin, label, weight, qid, obj):
        alphas = getattr(obj, "alphas", None)
        if not alphas:
            raise ValueError(
                "eval_metric 'quantile' needs objective reg:quantileerror "
                "with quantile_alpha"
            )
        if (_fused_eval_ok(margin, max_dim=2)
                and margin.dtype == torch.float32
                and label.dtype == torch.float32 and label.dim() == 1
                and margin.numel() == label.numel() * len(alphas)):
            from xgboost_ray_amd import ops

            if len(alphas) <= ops.QUANTILE_MAX_TARGETS:
                return ops.eval_pointwise(margin, label, weight, "pinball",
                                          param=alphas)
        pred = margin.double().reshape(margin.shape[0], -1)
        a = torch.tensor(alphas, dtype=torch.float64, device=margin.device)
        d = label.double().unsqueeze(1) - pred
        loss = torch.where(d >= 0, a * d, (a - 1.0) * d)
        w = _w(label, weight)
        return torch.stack(
            [(w.unsqueeze(1) * loss).sum() / len(alphas), w.sum()]
        )

    def finalize(self, s):
        return float(s[0] / s[1])


def get_metric(name: str) -> Metric:
    if name.startswith("error@"):
        return BinaryError(float(name.split("@")[1]))
    if name.startswith("ndcg@"):
        return NDCG(int(name.split("@")[1]))
    if name.startswith("tweedie-nloglik"):
        parts = name.split("@")
        return TweedieNLogLik(float(parts[1]) if len(parts) > 1 else 1.5)
    table = {
        "rmse": RMSE,
        "mae": MAE,
        "logloss": LogLoss,
        "error": BinaryError,
        "auc": AUC,
        "aucpr": AUCPR,
        "mlogloss": MLogLoss,
        "merror": MError,
        "ndcg": NDCG,
        "map": MAP,
        "poisson-nloglik": PoissonNLogLik,
        "gamma-nloglik": GammaNLogLik,
        "rmsle": RMSLE,
        "aft-nloglik": AFTNLogLik,
        "cox-nloglik": CoxNLogLik,
        "mphe": MPHE,
        "mape": MAPE,
        "quantile": Quantile,
    }
    if name not in table:
        raise ValueError(f"Unsupported eval_metric: {name}")
    return table[name]()
