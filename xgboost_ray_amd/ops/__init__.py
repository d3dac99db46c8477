"""Device-dispatched compute primitives for the boosting engine.

Each op has two implementations:

- a pure-PyTorch CPU reference (``ops.cpu``) used for CPU training and as the
  numerics oracle in tests, and
- a hand-written CDNA4 HIP kernel (``ops.gpu`` -> ``xgboost_ray_amd/csrc``)
  used whenever tensors live on a GPU.

On a machine with a GPU the HIP extension is REQUIRED: if a CUDA tensor
reaches an op and the extension is not importable, we raise instead of
silently falling back to slow eager code (this is the MI355X-native compute
path, reference-equivalent of XGBoost's CUDA gpu_hist updater, see
reference main.py:745 / SURVEY.md #2.3).

Histogram determinism: gradients are quantized to int64 fixed point before
histogram accumulation, so per-bin sums are integer adds - associative and
therefore bitwise-identical regardless of atomic ordering, row partition
order, or world size. This is what makes checkpoint-resume and
elastic-restart models deterministic (reference test_fault_tolerance.py
testSameResultWithAndWithoutError semantics).
"""

import torch

from xgboost_ray_amd.ops import cpu as _cpu

MISSING_BIN = 255  # uint8 marker for "value missing" in the binned matrix

_gpu_mod = None
_gpu_checked = False


def _gpu():
    """Load the HIP extension, failing loudly if unavailable."""
    global _gpu_mod, _gpu_checked
    if not _gpu_checked:
        _gpu_checked = True
        from xgboost_ray_amd.ops import gpu as gpu_backend

        _gpu_mod = gpu_backend
    if _gpu_mod is None:  # pragma: no cover
        raise RuntimeError("GPU op requested but HIP extension failed to load")
    return _gpu_mod


def _impl(t: torch.Tensor):
    return _gpu() if t.is_cuda else _cpu


def quantize_gpair(gpair: torch.Tensor, scale_g: float, scale_h: float) -> torch.Tensor:
    """fp32 [n,2] gradient pairs -> int32 [n,2] fixed point (|q| <= 2^30
    by scale construction; int64 accumulators hold any sum)."""
    return _impl(gpair).quantize_gpair(gpair, scale_g, scale_h)


def quantize_gpair_sums(gpair, scale_g, scale_h):
    """GPU only: ``quantize_gpair`` that also returns the int64 [2] column
    sums of its output (== ``gq.sum(0, dtype=int64)``, integer and so
    order-free) from the same pass over the data."""
    return _gpu().quantize_gpair(gpair, scale_g, scale_h, return_sums=True)


def apply_tree_binned(bins, margin, feat, split_bin, left, default_left,
                      value):
    """GPU only: add one tree's leaf values into ``margin`` in row order.

    Every row of ``bins`` (uint8 [n, F], any row stride) walks the tree:
    at a split node go left iff ``bin <= split_bin`` (missing bin 255
    follows ``default_left``), right child = left + 1; at the leaf
    ``margin[row] += value[leaf]`` (one f32 add). ``feat < 0`` marks a
    leaf; the tree arrays live on the host. ``margin`` is an f32 vector or
    a strided column view of a [n, C] matrix, updated in place.
    """
    return _gpu().apply_tree_binned(
        bins, margin, feat, split_bin, left, default_left, value)


def bin_matrix(values, cuts_flat, cut_ptr):
    """fp32 [n, F] feature matrix -> uint8 [n, F] bin indices.

    bin = number of cut points strictly below the value, clamped to the
    feature's bin count - 1; NaN -> MISSING_BIN.
    """
    return _impl(values).bin_matrix(values, cuts_flat, cut_ptr)


def build_histogram(bins, gpair_q, ridx, starts, counts, n_bins,
                    f_range=None, out=None, pregathered=False):
    """Accumulate per-(node, feature, bin) int64 gradient-pair histograms.

    bins: uint8 [n, F]; gpair_q: int32 [n, 2] packed pairs; ridx: int32 [n]
    row index array partitioned into contiguous per-node segments;
    starts/counts: int64 [K] segment descriptors for the K nodes to build.
    f_range=(f_lo, f_hi) builds only that feature slice (into ``out``,
    which the caller allocates zeroed) so the driver can overlap the
    AllReduce of one block with the build of the next.
    Returns int64 [K, F, n_bins, 2]. Missing values (bin==MISSING_BIN) are
    skipped; their mass is recovered as node_total - feature_sum.
    """
    return _impl(bins).build_histogram(
        bins, gpair_q, ridx, starts, counts, n_bins, f_range, out,
        pregathered
    )


def find_splits(
    hist,
    parent_g,
    parent_h,
    feat_bins,
    scale_g,
    scale_h,
    reg_lambda,
    reg_alpha,
    gamma,
    min_child_weight,
    monotone=None,
    bounds=None,
    allowed=None,
    pull=True,
    prev_hist=None,
    pslots=None,
    spos=None,
    reduce=True,
):
    """Best-split scan over histograms.

    hist: int64 [K, F, B, 2]; parent_g/parent_h: int64 [K] quantized node
    sums; feat_bins: int32 [F] per-feature bin counts.
    Returns dict of tensors (on hist.device) each [K]:
      gain f32, feature i32, bin i32, default_left u8,
      left_g/left_h int64 (quantized left-child sums incl. missing if
      default_left).

    GPU only: ``prev_hist``/``pslots``/``spos`` derive the trailing
    sibling rows of ``hist`` inside the scan kernel, ``reduce=False``
    returns the (node, feature) scan arrays for ``partition_rows_from_kf``
    (see ops.gpu.find_splits).
    """
    kw = {}
    if hist.is_cuda:
        kw["pull"] = pull  # CPU impl always returns host arrays
        kw["prev_hist"] = prev_hist
        kw["pslots"] = pslots
        kw["spos"] = spos
        kw["reduce"] = reduce
    elif prev_hist is not None or not reduce:
        raise ValueError("in-kernel sibling derivation is GPU only")
    return _impl(hist).find_splits(
        hist,
        parent_g,
        parent_h,
        feat_bins,
        scale_g,
        scale_h,
        reg_lambda,
        reg_alpha,
        gamma,
        min_child_weight,
        monotone,
        bounds,
        allowed,
        **kw,
    )


def partition_begin(bins, ridx, starts, counts, split_feat, split_bin,
                    default_left, gpair_seg=None, bins_t=None):
    """Two-phase partition, phase 1 (GPU only): see ops.gpu."""
    from xgboost_ray_amd.ops import gpu

    return gpu.partition_begin(bins, ridx, starts, counts, split_feat,
                               split_bin, default_left, gpair_seg, bins_t)


def partition_finish(ctx):
    """Two-phase partition, phase 2 (GPU only): see ops.gpu."""
    from xgboost_ray_amd.ops import gpu

    return gpu.partition_finish(ctx)


def partition_rows_from_packed(bins, ridx, starts_ord, counts_ord, packed,
                               gseg, bins_t, chunk_bound, ridx_dest=None,
                               fused_glue=None):
    """Single-sync fused partition (GPU only): see ops.gpu."""
    from xgboost_ray_amd.ops import gpu

    return gpu.partition_rows_from_packed(
        bins, ridx, starts_ord, counts_ord, packed, gseg, bins_t,
        chunk_bound, ridx_dest, fused_glue,
    )


def partition_rows_from_kf(bins, ridx, starts_ord, counts_ord, kf, gseg,
                           bins_t, chunk_bound, ridx_dest=None):
    """Single-sync fused partition fed by ``find_splits(reduce=False)``
    (GPU only): see ops.gpu."""
    from xgboost_ray_amd.ops import gpu

    return gpu.partition_rows_from_kf(
        bins, ridx, starts_ord, counts_ord, kf, gseg, bins_t, chunk_bound,
        ridx_dest,
    )


def partition_rows(bins, ridx, starts, counts, split_feat, split_bin,
                   default_left, gpair_seg=None, bins_t=None):
    """Stable partition of each node's ridx segment by its split.

    Rows with bin <= split_bin (or missing & default_left) go left. When
    ``gpair_seg`` (int32 [n,2], segment-ordered gradient pairs) is given
    it is permuted alongside ridx - fusing the next depth's gradient
    gather into the scatter.
    Returns (ridx_out, left_counts[, gpair_seg_out]).
    """
    return _impl(bins).partition_rows(
        bins, ridx, starts, counts, split_feat, split_bin, default_left,
        gpair_seg, bins_t
    )


def predict_trees(
    X, feat, thr, left, default_left, value, tree_ptr, out, tree_weight=1.0
):
    """Accumulate tree-walk predictions for a forest slice into ``out``.

    X: fp32 [n, F] raw features (NaN = missing). Tree arrays are flat SoA
    concatenations with tree_ptr: int32 [T+1] node offsets.
    feat: int32 (-1 => leaf), thr: f32, left: int32 (right = left + 1),
    default_left: u8, value: f32 leaf weight. out: f32 [n] updated in place.
    Decision rule (XGBoost semantics): go left iff x < thr; missing follows
    default_left.
    """
    return _impl(X).predict_trees(
        X, feat, thr, left, default_left, value, tree_ptr, out, tree_weight
    )


def predict_leaf(X, feat, thr, left, default_left, tree_ptr, out, **kw):
    """Leaf reached by every row in every tree of a forest slice.

    X: fp32 [n, F] raw features (NaN = missing). The forest is the flat SoA
    of ``predict_trees`` without ``value``; ``tree_ptr`` is an int32 [T+1]
    HOST vector. out: int32 [n, T], overwritten with the node index of the
    leaf reached in tree t, relative to ``tree_ptr[t]`` (0 for a tree
    whose root is a leaf) - the index ``Booster.predict_leaf`` and xgboost
    return. Decision rule exactly as in ``predict_trees``: left iff
    x < thr in float32, NaN follows default_left, right child = left + 1.
    A forest whose walk could leave its arrays (split feature >= F,
    children outside their tree or not after their parent) is a
    ValueError.

    Dispatches on X's device. On the GPU ``out`` may live on the host or
    be strided: rows are processed in chunks whose device output stays
    under ``max_out_bytes`` (keyword, default ``ops.gpu.WALK_OUT_BYTES``),
    each chunk copied out before the next one runs.
    """
    return _impl(X).predict_leaf(
        X, feat, thr, left, default_left, tree_ptr, out, **kw)


def saabas_contribs(X, feat, thr, left, default_left, node_mean, tree_ptr,
                    out, **kw):
    """Saabas (approximate) feature contributions, accumulated into ``out``.

    X and the forest as in ``predict_leaf``. node_mean: float64 [n_nodes],
    the cover-weighted expected value of every node
    (``booster._fill_node_means``), flattened like the other arrays. out:
    float64 [n, F+1], unit column stride, any row stride. Per row, for each
    tree in order: ``out[row, F] = out[row, F] + node_mean[root]``, then for
    each split on the row's walk from the root down
    ``out[row, feat] = out[row, feat] + (node_mean[child] - node_mean[node])``.
    Every operation is an IEEE float64 add or subtract in exactly this
    sequence, and the sums START from the values ``out`` holds on entry, so
    the result is bitwise defined and equal on every backend.

    Dispatches on X's device. On the GPU a host ``out`` is processed in row
    chunks under ``max_out_bytes`` (keyword, default
    ``ops.gpu.WALK_OUT_BYTES``): each chunk of ``out`` is copied to the
    device, accumulated into and copied back. ``lds_accumulators``
    (keyword, GPU): None keeps a row's sums in LDS when F+1 columns fit,
    False accumulates in global memory, True makes a misfit an error; the
    result is the same bytes either way.
    """
    return _impl(X).saabas_contribs(
        X, feat, thr, left, default_left, node_mean, tree_ptr, out, **kw)


SHAP_MAX_PATH_LEN = _cpu.SHAP_MAX_PATH_LEN


def tree_shap(X, paths, n_groups, out, **kw):
    """Exact TreeSHAP feature contributions in path form.

    X: fp32 [n, F] row-major raw features (NaN = missing). paths: the
    dict ``ops.cpu.shap_paths`` builds from a forest (one path per leaf,
    one element per unique feature; longest path <= SHAP_MAX_PATH_LEN,
    else ValueError - callers fall back to the recursion). out: float64
    [n, n_groups, F+1] tensor, ACCUMULATED into: for every element i of
    every path, out[row, group, feature_i] +=
    unwound_sum(path, i) * (one_i - zero_i) * value. Only feature columns
    are written; the bias column (``paths["bias"]`` + base margin) is the
    caller's. All arithmetic is float64 and each row's sums run in path
    order, so the result is bitwise repeatable.

    Dispatches on X's device. On the GPU ``out`` may live on the host:
    rows are processed in chunks whose device output stays under
    ``max_out_bytes`` (keyword, default ``ops.gpu.SHAP_OUT_BYTES``), each
    chunk copied out before the next one runs.
    """
    return _impl(X).tree_shap(X, paths, n_groups, out, **kw)


def tree_shap_interactions(X, paths, out, **kw):
    """Raw off-diagonal SHAP interaction terms in path form.

    X, paths as in ``tree_shap`` (single output group). out: float64
    [n, F+1, F+1] tensor, ACCUMULATED into: for a path with elements E,
    every c in E and j in E \\ {c} adds
    (one_c - zero_c) / 2 * unwound_sum(E \\ {c}, j) * (one_j - zero_j) * value
    to out[row, feature_c, feature_j]. The diagonal, the bias row/column
    and the (M + M^T) / 2 symmetrisation are the caller's
    (``Booster.predict_interactions``). Same dispatch, chunking
    (``max_out_bytes``, default ``ops.gpu.SHAP_INTER_OUT_BYTES``) and
    repeatability as ``tree_shap``.
    """
    return _impl(X).tree_shap_interactions(X, paths, out, **kw)


def update_margins(margin, ridx, starts, counts, leaf_values,
                   ridx_b=None, parity=None):
    """margin[ridx[seg_k]] += leaf_values[k] for each final-leaf segment.

    ridx_b/parity (GPU): ping-pong leaf buffers - parity[k] selects the
    buffer node k's rows last landed in."""
    if margin.is_cuda:
        from xgboost_ray_amd.ops import gpu

        return gpu.update_margins(
            margin, ridx, starts, counts, leaf_values,
            ridx_b=ridx_b, parity=parity,
        )
    return _impl(margin).update_margins(
        margin, ridx, starts, counts, leaf_values
    )


def leaf_quantile_hist(resid, weight, ridx, starts, counts, prefix, pass_idx,
                       out, ridx_b=None, parity=None):
    """One MSB-first radix-select pass over leaf segments.

    out[k, digit] += W[row] for the rows of segment k whose order-preserving
    uint32 key (see ``ops.cpu.quantile_keys``) equals ``prefix[k]`` in its
    top ``8 * pass_idx`` bits; digit = the next 8 key bits.
    resid: f32 [n] by row id; weight: int64 [n] or None (unit weights);
    ridx/ridx_b/starts/counts/parity: the ``update_margins`` segment
    descriptors; prefix: int64 [L]; out: int64 [L, 256], accumulated into.
    Integer sums: CPU and GPU agree exactly, in any row order.
    """
    return _impl(resid).leaf_quantile_hist(
        resid, weight, ridx, starts, counts, prefix, pass_idx, out,
        ridx_b=ridx_b, parity=parity,
    )


def leaf_quantile_select(resid, weight, ridx, starts, counts, alpha,
                         ridx_b=None, parity=None, allreduce=None):
    """Exact weighted lower alpha-quantile of ``resid`` in every segment.

    Four ``leaf_quantile_hist`` passes; after each, ``allreduce`` (if given:
    an in-place int64 SUM over ranks) makes the histograms global and every
    segment keeps the first digit whose running sum reaches its remaining
    threshold T = clamp(ceil(alpha * W_seg), 1, W_seg). int64 arithmetic
    only. Returns (q f32 [L], W_seg int64 [L]) as numpy arrays; q is
    meaningless where W_seg == 0.
    """
    import numpy as np

    L = len(starts)
    starts = torch.as_tensor(starts, dtype=torch.int64)
    counts = torch.as_tensor(counts, dtype=torch.int64)
    prefix = np.zeros(L, np.int64)
    T = None
    W_seg = None
    for p in range(4):
        hist = torch.zeros((L, 256), dtype=torch.int64, device=resid.device)
        leaf_quantile_hist(resid, weight, ridx, starts, counts,
                           torch.from_numpy(prefix), p, hist,
                           ridx_b=ridx_b, parity=parity)
        if allreduce is not None:
            allreduce(hist)
        h = hist.cpu().numpy()
        cum = np.cumsum(h, axis=1)
        if p == 0:
            W_seg = cum[:, 255].copy()
            T = np.ceil(float(alpha) * W_seg.astype(np.float64)).astype(
                np.int64)
            T = np.minimum(np.maximum(T, 1), W_seg)
        digit = np.argmax(cum >= T[:, None], axis=1).astype(np.int64)
        rows = np.arange(L)
        T = T - (cum[rows, digit] - h[rows, digit])
        prefix = (prefix << 8) | digit
    key = prefix.astype(np.uint32)
    bits = np.where(key & np.uint32(0x80000000),
                    key ^ np.uint32(0x80000000), ~key)
    return bits.astype(np.uint32).view(np.float32), W_seg


mvs_key = _cpu.mvs_key  # uint64 stream key from (seed, iteration, tree, rank)


def mvs_score(gpair, mx_g, mx_h):
    """Gradient-based sampling, step 1: integer row scores.

    gpair: f32 [n, 2]; mx_g / mx_h: the (global) maxima of |g| and |h|.
    With sv = 2^60 / max(mx_g^2 + 0.1 mx_h^2, 1e-300) (float64, host), per
    row in float64 without contraction: v = g*g + 0.1*(h*h),
    V = rne(v * sv) clamped to 2^60 (NaN clamps too), c = floor(sqrt(V))
    as an exact integer square root. Returns uint32 [n], c in [0, 2^30];
    c / 2^30 is sqrt(g^2 + 0.1 h^2) relative to its largest possible value.
    """
    return _impl(gpair).mvs_score(gpair, mx_g, mx_h)


def mvs_hist(c, prefix, pass_idx):
    """One MSB-first radix pass over the scores: int64 [256, 2] of
    (count, sum c) per digit, over the rows whose top ``8 * pass_idx`` bits
    equal ``prefix`` (digit = the next 8 bits). Integer sums: CPU and GPU
    agree exactly."""
    return _impl(c).mvs_hist(c, prefix, pass_idx)


def mvs_threshold(c, k):
    """Gradient-based sampling, step 2: the threshold for an expected
    sample of k rows, as Python ints (S, M) with mu = S / M.

    With A(t) = sum of c_i < t and N(t) = #{c_i >= t}: (0, 0) if at most k
    scores are non-zero (keep them all, unweighted). Otherwise t* is the
    largest integer t >= 1 with A(t) >= (k - N(t)) * t,
    S = sum of c_i <= t*, M = k - #{c_i > t*}; a row is then kept with
    probability min(1, c_i * M / S). If t* exceeds max c the answer is the
    closed form (sum c, k); else t* comes from four ``mvs_hist`` passes,
    the digit chosen on the host after each.
    """
    return _impl(c).mvs_threshold(c, k)


def mvs_sample(gpair, c, S, M, key):
    """Gradient-based sampling, step 3: draw the sample.

    Row i is kept iff c_i > 0 and (S == 0 or c_i*M >= S or
    u_i*S < c_i*M*2^32) with u_i = splitmix64(key + i) >> 32 (uint64,
    wrapping) - integer arithmetic only. A row kept with probability < 1
    gets f32(f64(g) * (f64(S) / f64(c_i*M))) (same for h); one kept for
    certain keeps its pair; a dropped row gets (0, 0).
    Returns (keep uint8 [n], gpair_w f32 [n, 2]).
    """
    return _impl(gpair).mvs_sample(gpair, c, S, M, key)


def grad_fused(margin, label, weight, scale_pos_weight, mode):
    """Fused objective gradient + |g|/|h| max for the hot objectives
    (mode 0 = reg:squarederror, 1 = binary:logistic). GPU only: returns
    (fp32 gpair [n,2], f32 absmax [2]) or None on CPU (the torch
    composition is the CPU path and the numerics oracle)."""
    import os

    if not margin.is_cuda or os.environ.get("RXGB_FUSED_GRAD") == "0":
        return None
    from xgboost_ray_amd.ops import gpu

    return gpu.grad_fused(margin, label, weight, scale_pos_weight, mode)
