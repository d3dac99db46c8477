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


def bin_matrix(values, cuts_flat, cut_ptr, out=None):
    """fp32 [n, F] feature matrix -> uint8 [n, F] bin indices.

    bin = number of cut points strictly below the value, clamped to the
    feature's bin count - 1; NaN -> MISSING_BIN. ``out`` (uint8 [n, F],
    unit column stride, any row stride) receives the bins in place: the
    per-tree re-bin of tree_method="approx" into the resident matrix.
    """
    if out is None:
        return _impl(values).bin_matrix(values, cuts_flat, cut_ptr)
    if values.is_cuda:
        return _gpu().rebin(values, cuts_flat, cut_ptr, out)
    out.copy_(_cpu.bin_matrix(values, cuts_flat, cut_ptr))
    return out


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


def sketch_pass(X, W, table, n_slots, pass_idx, S, out):
    """One MSB-first radix-select pass of the weighted quantile sketch.

    X: f32 [n, F] row-major contiguous (a view may start off a 16-byte
    boundary: it takes scalar loads, not a copy); W: int32 or int64 [n], any
    stride, entries <= 0 count as 0. table: int32 [F, S], row f holding the
    feature's ``n_slots[f]`` active key prefixes (the top ``8 * pass_idx``
    bits of ``ops.cpu.quantile_keys``), ascending and distinct; both are
    unread in pass 0, where every feature has the one slot 0. For every
    non-NaN X[row, f] whose prefix is table[f, slot]:
    ``out[f * S + slot, digit] += W[row]`` with digit = the next 8 key bits.
    out: int64 [F * S, 256], accumulated into, so several row shards may
    share it. Integer sums: CPU and GPU agree exactly, in any row order.
    """
    return _impl(X).sketch_pass(X, W, table, n_slots, int(pass_idx), int(S),
                                out)


def weighted_cuts(X, W, max_bin, col_max, allreduce=None):
    """Exact weighted quantile cuts of every feature, world-size invariant.

    X, W as in ``sketch_pass``, or equally long sequences of row shards,
    whose passes accumulate into one histogram; col_max: f32 [F], the
    global largest non-NaN value of each column (NaN: all missing);
    allreduce as in ``leaf_quantile_select``, applied to each pass's
    histogram. With nb = min(max_bin, 255), Wf the weight of feature f's
    non-missing rows and T_j = ceil(j * Wf / nb) for j = 1 .. nb-1, v_j is the
    smallest value whose cumulative weight in key order reaches T_j (none
    when Wf == 0). The feature's cuts are the ascending distinct v_j, then
    nextafter(col_max[f]), deduplicated; none for an all-missing column.

    Four ``sketch_pass`` launches per shard. Between them the select runs
    as torch int64 ops on X's device: a cumulative sum over the digits of
    each target's slot, the first digit that reaches the remaining target,
    then the next prefix tables (a feature's targets ascend with j, so its
    prefixes are sorted already) and remaining targets. Nothing is pulled to
    the host before the final cut count. Equal multisets of (value, weight)
    pairs give equal bytes on any sharding and either backend;
    ``ops.cpu.weighted_cuts`` is the sort-based oracle.
    """
    from xgboost_ray_amd.engine.quantile import HistogramCuts

    Xs = list(X) if isinstance(X, (list, tuple)) else [X]
    Ws = list(W) if isinstance(W, (list, tuple)) else [W]
    dev = Xs[0].device
    F = Xs[0].shape[1]
    nb = min(int(max_bin), 255)
    S = max(nb - 1, 1)
    j = torch.arange(1, S + 1, dtype=torch.int64, device=dev)
    prefix = torch.zeros((F, S), dtype=torch.int64, device=dev)
    slot = torch.zeros((F, S), dtype=torch.int64, device=dev)
    table = torch.zeros((F, S), dtype=torch.int32, device=dev)
    n_slots = torch.ones(F, dtype=torch.int32, device=dev)
    rem = valid = None
    for p in range(4):
        out = torch.zeros((F * S, 256), dtype=torch.int64, device=dev)
        for Xp, Wp in zip(Xs, Ws):
            sketch_pass(Xp, Wp, table, n_slots, p, S, out)
        if allreduce is not None:
            allreduce(out)
        h = out.view(F, S, 256)
        if p == 0:
            Wf = h[:, 0, :].sum(1)
            valid = (Wf > 0) & (nb > 1)
            # ceil(j * Wf / nb) without forming j * Wf
            q = (Wf // nb)[:, None]
            r = (Wf % nb)[:, None]
            rem = j * q + (j * r + (nb - 1)) // nb
        hj = h.gather(1, slot[:, :, None].expand(F, S, 256))
        cum = hj.cumsum(2)
        digit = (cum < rem[:, :, None]).sum(2).clamp(max=255)[:, :, None]
        rem = rem - (cum.gather(2, digit) - hj.gather(2, digit))[:, :, 0]
        prefix = (prefix << 8) | digit[:, :, 0]
        first = torch.ones((F, S), dtype=torch.bool, device=dev)
        first[:, 1:] = prefix[:, 1:] != prefix[:, :-1]
        first &= valid[:, None]
        if p < 3:
            slot = (first.cumsum(1) - 1).clamp(min=0)
            n_slots = first.sum(1).to(torch.int32)
            table = torch.zeros((F, S), dtype=torch.int32, device=dev)
            table.scatter_(1, slot, prefix.to(torch.int32))
    cmax = col_max.to(dev).float()
    above = torch.nextafter(cmax, torch.full_like(cmax, float("inf")))
    vals = torch.cat([_cpu.keys_to_float(prefix), above[:, None]], 1)
    keep = torch.cat([first, ~torch.isnan(cmax)[:, None]], 1)
    keep[:, :S] &= keep[:, S:]  # an all-missing column has no cuts at all
    # v_j <= col_max < above unless col_max is +inf, its own successor
    last_v = torch.where(first, vals[:, :S], vals.new_tensor(float("nan")))
    keep[:, S] &= ~(last_v == above[:, None]).any(1)
    counts = keep.sum(1)
    ptr = torch.zeros(F + 1, dtype=torch.int64, device=dev)
    ptr[1:] = counts.cumsum(0)
    return HistogramCuts(
        cuts_flat=vals[keep],
        cut_ptr=ptr,
        max_bins=int(counts.max()) or 1,
    )


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


RANK_LDS_MAX_GROUP = _cpu.RANK_LDS_MAX_GROUP


def rank_gpu_enabled():
    """RXGB_RANK_GPU=0 keeps the ranking objectives and metrics on their
    torch routes (the HIP ranking kernels are on by default)."""
    import os

    return os.environ.get("RXGB_RANK_GPU") != "0"


def rank_disc_table(device):
    """float64 [RANK_LDS_MAX_GROUP] DCG discounts 1 / log2(r + 2) on
    ``device``: computed on the host with numpy, uploaded once and cached,
    so no device log2 enters a DCG."""
    if torch.device(device).type == "cuda":
        return _gpu().rank_disc_table(device)
    return torch.from_numpy(_cpu.rank_disc_table())


def rank_group_stats(margin, label, group_ptr, disc, k, max_len=None, **kw):
    """Stable descending rank of every row inside its query group, and the
    DCG / AP sums of every group.

    margin, label: f32 [n]; group_ptr: int64 [G+1] row offsets of the
    groups (rows of a group are contiguous); disc: ``rank_disc_table``;
    k: truncation level, 0 = whole group. No group may be longer than
    RANK_LDS_MAX_GROUP; ``max_len``, the longest group, saves the GPU route
    a sync when the caller knows it.
    Returns (rank i32 [n], stats f64 [G, 4]). rank orders by descending
    margin, ties (-0.0 == +0.0 included) in row order. With
    gain = 2^label - 1 in float64, stats[g] = [dcg@k, idcg@k, idcg, ap]:
    dcg@k sums gain * disc[rank] over ranks < min(k, L); idcg@k and idcg
    are the same sums over the gains sorted descending; ap is the average
    over relevant rows (label > 0) of (relevant rows at ranks <= p) /
    (p + 1), 0 without a relevant row. On the GPU every sum has a fixed
    order, so equal inputs give equal bytes.
    """
    return _impl(margin).rank_group_stats(
        margin, label, group_ptr, disc, k, max_len, **kw)


def lambdamap_grad(margin, label, group_ptr, max_len=None, **kw):
    """rank:map gradient pairs f32 [n, 2] (unweighted).

    With rank, rel = label > 0, R = #rel, prefix[p] = #rel at ranks <= p,
    t[p] = prefix[p] / (p + 1) and S[p] = sum_{q <= p} rel_q / (q + 1) per
    group as in ``rank_group_stats``: every ordered pair with
    label_i > label_j has rho = 1 / (1 + exp(m_i - m_j)) (difference in
    float32, the rest float64), delta = |t[hi] - t[lo] - (S[hi-1] - S[lo])|
    / R at lo / hi = the smaller / larger of the two ranks, and adds
    -rho * delta to g_i, +rho * delta to g_j and
    max(rho (1 - rho), 1e-16) * delta to both hessians. Groups with R = 0
    or fewer than two rows give zeros.
    """
    return _impl(margin).lambdamap_grad(margin, label, group_ptr, max_len,
                                        **kw)


def lambdarank_topk_grad(margin, label, group_ptr, disc, k, ndcg,
                         max_len=None, **kw):
    """rank:pairwise (``ndcg`` false) / rank:ndcg gradient pairs f32 [n, 2]
    (unweighted) with top-k pair truncation.

    margin, label, group_ptr, disc, max_len as in ``rank_group_stats``;
    k >= 1. With rank the stable descending order of the float32 margins
    inside a group, a pair (i, j) with label_i > label_j counts iff
    min(rank_i, rank_j) < k. A counted pair has
    rho = 1 / (1 + exp(m_i - m_j)) (difference in float32, the rest
    float64), hess = max(rho (1 - rho), 1e-16) and weight w = 1, or for ndcg
    w = |dgain * ddisc| / idcg with gain = 2^label - 1, disc = disc[rank]
    and idcg over the whole group, not truncated. It adds -rho w to g_i,
    +rho w to g_j and hess w to both hessians. A group of fewer than two
    rows and an ndcg group with idcg <= 0 give zeros; a row without a
    counted pair gets exactly (0, 0); k >= the group's length is the
    all-pairs gradient. Row weights are the caller's. NaN margins have no
    defined result, but no address depends on a margin. On the GPU every
    sum has a fixed order and nothing is atomic: equal inputs give equal
    bytes.
    """
    return _impl(margin).lambdarank_topk_grad(
        margin, label, group_ptr, disc, k, ndcg, max_len, **kw)


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


# KC of the GPU multiclass kernels: a margin with K <= KC classes is one LDS
# chunk per row tile, a wider one is walked in chunks of KC
SOFTMAX_CHUNK_CLASSES = _cpu.SOFTMAX_CHUNK_CLASSES


def softmax_grad(margin, label, weight=None, **kw):
    """multi:softprob / multi:softmax gradient pairs and their per-class
    maxima, one pass over the margin.

    margin: f32 [n, K] contiguous, K >= 2; label: f32 [n] class indices;
    weight: f32 [n] or None. Returns (gpair, absmax): gpair f32 of shape
    [n, K, 2], stored class-major ([K, n, 2], permuted), so every
    ``gpair[:, cls, :]`` is contiguous; absmax f32 [K, 2] with
    absmax[cls, c] == gpair[:, cls, c].abs().max() bitwise.

    Per row, in float64 from the float32 inputs and with no step fused into
    the next: m = max_k x_k (compared in float32), d_k = x_k - m,
    e_k = exp(d_k), s = sum_k e_k in ascending class order, p_k = e_k / s,
    g_k = float32(p_k - [k == y]), h_k = float32(max(2 p_k (1 - p_k),
    1e-16)); with a weight both are then multiplied by it in float32. The
    label, truncated toward zero as ``.long()`` does, is only compared with
    k and never forms an address: outside [0, K) it gives g_k = p_k. A NaN
    margin makes its row's outputs NaN, and absmax keeps the NaN.

    On the GPU a margin with K > SOFTMAX_CHUNK_CLASSES is walked in
    chunks and s is a running sum, rescaled by exp(m_old - m_new) whenever
    the running maximum grows: such a K is held to the error bound
    |out - ref| <= 2^-23 |ref| + 2^-40 max(1, w), not to the bits of the
    plain sum. Each K takes one route and nothing is atomic: equal inputs
    give equal bytes. ``ops.cpu.softmax_grad`` is the numpy float64 form and
    the oracle. The torch composition in ``SoftmaxBase.gradients`` remains
    the CPU training path.
    """
    return _impl(margin).softmax_grad(margin, label, weight, **kw)


def eval_multiclass(margin, label, weight=None, **kw):
    """f64 [3] = [sum w * nll, sum w * wrong, sum w] of a multiclass margin
    (inputs as in ``softmax_grad``; w = 1 without weights). Per row in
    float64, with m, d and s as in ``softmax_grad``: nll = log(s) - d_y (NaN
    for a label outside [0, K)); wrong = 1 unless the lowest index attaining
    the maximum equals the label. On the GPU the sums run in a fixed order
    (a thread's rows in order, a butterfly inside a wave, wave order, then a
    sum over the workgroups' partials)."""
    return _impl(margin).eval_multiclass(margin, label, weight, **kw)


def eval_auc_multiclass(margin, label, weight=None, n_bins=16384, **kw):
    """int64 [K, 2, n_bins] one-vs-rest score histograms of a multiclass
    margin, planes [negative | positive] per class: what ``auc`` and
    ``aucpr`` reduce an [n, K] margin to.

    margin: f32 [n, K] contiguous, K >= 2; label: f32 [n]; weight: f32 [n]
    or None; 1 <= n_bins <= 16384, anything else raises before any launch.
    Per row, p_k is the softmax of ``softmax_grad``'s contract in its
    one-chunk form, for every K: m = max_k x_k (compared in float32),
    d_k = (double)x_k - (double)m, e_k = exp(d_k), s = sum_k e_k in ascending
    class order, p_k = e_k / s, nothing contracted. b_k = min(trunc(p_k *
    n_bins), n_bins - 1), and 0 unless p_k * n_bins >= 1: a NaN row lands in
    bin 0 of every class and no address depends on a NaN. Row i is a
    positive of class k iff its label, truncated toward zero as ``.long()``
    does, equals k; the label is only compared and never forms an address,
    and outside [0, K) the row is a negative of every class. Each row adds 1
    to ``hist[k, positive, b_k]`` for every k, or with weights
    W = llrint((double)w * 2^20); n * 2^20 * max(w) must stay below 2^53
    (checked on the host, only when weights are given).

    All sums are integer: two launches, any world size and any sharding give
    equal bytes. On the GPU two kernels run (docs/parity.md "Multiclass AUC
    on the device"): one pass over the margin writes a u16 code per (class,
    row), class-major; a grid of row segments x classes counts the codes
    into LDS histograms. ``max_out_bytes`` (keyword, GPU, default
    ``ops.gpu.WALK_OUT_BYTES``) bounds the code buffer of one row chunk and
    ``count_rows`` the rows of a counting workgroup.
    ``ops.cpu.eval_auc_multiclass`` is the numpy float64 form and the
    oracle; its integers match the kernels'.
    """
    return _impl(margin).eval_auc_multiclass(margin, label, weight, n_bins,
                                             **kw)


# Sorted positions per workgroup of the GPU Cox kernels (asserted equal to
# the module's on load): the sizes around it are where their paths change
COX_TILE_ROWS = _cpu.COX_TILE_ROWS


def aft_grad(margin, label, weight, dist, sigma):
    """survival:aft gradient pairs and their maxima, one pass.

    margin: f32 [n]; label: f32 [n, 2] (lower, upper); weight: f32 [n] or
    None; dist: "normal", "logistic" or "extreme"; sigma: host float.
    Returns (gpair f32 [n, 2], absmax f32 [2]) with absmax[c] ==
    gpair[:, c].abs().max() bitwise.

    Per row, in float64 from the float32 inputs, the contract of
    ``AFT.gradients``: lo = log(max(yl, 1e-16)), hi likewise, zl and zu
    clamped to [-15, 15]; the row is uncensored if yl == yu, else
    right-censored if isinf(yu), else left-censored if yl <= 0, else an
    interval; D >= 1e-300 and h >= 1e-6; g and h are cast to float32 and
    then multiplied by the weight in float32. The normal distribution goes
    through erfc (S(z) = erfc(z / sqrt 2) / 2). On the GPU a row evaluates
    its own branch only, and the maxima leave the kernel without atomics.
    A NaN margin makes its row's pair NaN, and absmax keeps the NaN.
    ``ops.cpu.aft_grad`` is the float64 torch form and the oracle."""
    return _impl(margin).aft_grad(margin, label, weight, dist, sigma)


def eval_aft(margin, label, weight, dist, sigma):
    """f64 [2] = [sum w * nll, sum w] with nll as ``AFT.nll`` (inputs as in
    ``aft_grad``; w = 1 without weights); fixed-order sums on the GPU."""
    return _impl(margin).eval_aft(margin, label, weight, dist, sigma)


def cox_layout(label):
    """What survival:cox needs of its labels alone (``ops.cpu.cox_layout``):
    built once per label tensor and cached on it as ``_rxgb_cox_layout``,
    keyed on its ``_version`` and device, as ``_rxgb_rank_layout`` is on
    qid. A caller that passes the same tensor object every round, as the
    trainer does, pays the sort once per data set."""
    hit = getattr(label, "_rxgb_cox_layout", None)
    if hit is not None and hit[:2] == (label._version, label.device):
        return hit[2]
    lay = _impl(label).cox_layout(label)
    label._rxgb_cox_layout = (label._version, label.device, lay)
    return lay


def cox_grad(margin, layout, weight=None):
    """survival:cox (Breslow) gradient pairs and their maxima.

    margin: f32 [n]; layout: ``cox_layout(label)``; weight: f32 [n] or None.
    Returns (gpair f32 [n, 2] in row order, absmax f32 [2]). With s a row's
    sorted position: shift = max margin (float32), eta = exp(double(m) -
    shift), R_s = max(C[last(s)], 1e-300) with C the inclusive prefix sum of
    eta, a = ev / R, b = ev / R^2, A_s = SufA[first(s)] with SufA the
    inclusive suffix sum of a (B likewise), g = -ev + eta A, h = max(eta A -
    eta^2 B, 1e-6); cast to float32, then the weight in float32. A NaN
    margin makes every output NaN. On the GPU the sums are a reduce-then-
    scan over tiles of COX_TILE_ROWS positions, in both directions, with
    one fixed grouping: equal inputs give equal bytes. The grouping is not
    the sequential one, so the GPU is held to the error bound of
    docs/parity.md, not to the oracle's bits."""
    return _impl(margin).cox_grad(margin, layout, weight)


def eval_cox(margin, layout):
    """f64 [2] = [-ll, number of events] of cox-nloglik: ll sums, over event
    rows, m - shift - log(max(C_s, 1e-300)) (C_s itself, not tie-adjusted,
    as ``CoxNLogLik`` has it)."""
    return _impl(margin).eval_cox(margin, layout)


# Targets that the GPU quantile kernels serve (asserted equal to the
# module's on load); a wider reg:quantileerror stays on torch
QUANTILE_MAX_TARGETS = _cpu.QUANTILE_MAX_TARGETS
POINTWISE_GRAD_KINDS = _cpu.POINTWISE_GRAD_KINDS
POINTWISE_EVAL_KINDS = _cpu.POINTWISE_EVAL_KINDS


def pointwise_grad(margin, label, weight, kind, param=0.0, **kw):
    """Gradient pairs of a pointwise regression objective and their maxima,
    one pass.

    margin, label: f32 [n]; weight: f32 [n] or None; kind: one of
    POINTWISE_GRAD_KINDS; param: rho for "tweedie", huber_slope for
    "pseudohuber". Returns (gpair [n, 2], absmax [2]).

    On the GPU the result is float32 and holds the bytes of the objective
    class's torch composition on the same tensors: the same float32
    operation order with one rounding per torch op, the same clamps and
    constants, Python scalars rounded to float32 where torch rounds them, a
    division by a Python scalar as the product with its float32 reciprocal,
    ``** 2`` as a product, and the weight's two float32 multiplies last. NaN
    goes where torch sends it: through exp, log and sqrt it stays NaN,
    ``sign`` turns it into 0, hinge's comparison is false so the row gets
    (0, 1e-16). absmax == gpair.abs().amax(0) bitwise, NaN kept. A margin
    view that starts off a 16-byte boundary takes scalar loads, not a copy.
    ``max_blocks`` caps the grid (tests force grid-stride turns with it).

    On CPU tensors this is ``ops.cpu.pointwise_grad``: the numpy float64
    form, returned as float64, the high-precision reference."""
    return _impl(margin).pointwise_grad(margin, label, weight, kind, param,
                                        **kw)


def quantile_grad(margin, label, weight, alphas, **kw):
    """reg:quantileerror pairs and maxima: g = 1 - a_k where m - y >= 0,
    else -a_k (so for NaN), with a_k rounded to float32 first; h = 1; then
    the weight in float32. margin f32 [n] gives (gpair [n, 2], absmax [2]).
    margin f32 [n, K] row-major, K = len(alphas) <= QUANTILE_MAX_TARGETS,
    gives gpair [n, K, 2] stored target-major ([K, n, 2], permuted), so
    every ``gpair[:, k, :]`` is contiguous, and absmax [K, 2]. On the GPU
    the bytes equal ``QuantileError.gradients``'s torch composition."""
    return _impl(margin).quantile_grad(margin, label, weight, alphas, **kw)


def eval_pointwise(margin, label, weight, kind, transform="identity",
                   param=0.0, **kw):
    """f64 [2] = [sum w * loss, sum w] of a regression metric (w = 1 without
    weights), per row in float64 from the float32 inputs.

    kind: one of POINTWISE_EVAL_KINDS, the loss of rmse, mae, mape, rmsle,
    mphe, poisson-nloglik, gamma-nloglik, tweedie-nloglik (param = rho) and
    quantile (kind "pinball": margin [n, K] or [n], param = the alpha list,
    loss = the mean over the row's targets), with the clamps of the metric
    classes. transform: "identity", "exp" or "sigmoid", the objective's
    prediction transform for the kinds defined on predictions (se, ae, ape,
    sle); the others take the margin itself. On the GPU the sums run in a
    fixed order (a thread's rows in order, a butterfly inside a wave, wave
    order, then a sum over the workgroups' partials) with no atomics: equal
    inputs give equal bytes. ``ops.cpu.eval_pointwise`` sums with
    ``math.fsum`` and is the reference."""
    return _impl(margin).eval_pointwise(margin, label, weight, kind,
                                        transform, param, **kw)
