"""GPU op implementations backed by the hand-written CDNA4 HIP extension.

The extension (``xgboost_ray_amd/csrc``) is compiled in-tree for gfx950
(``__graft_entry__.build()`` / ``python setup.py build_ext --inplace``).
On a GPU machine it is REQUIRED - there is no silent eager fallback for
CUDA tensors: if the .so is missing, ops raise immediately.
"""

import os

import torch

_ext = None
_load_error = None


def _load():
    global _ext, _load_error
    if _ext is not None:
        return _ext
    try:
        import importlib

        _ext = importlib.import_module("xgboost_ray_amd._hip_ops")
    except ImportError as e:
        _load_error = e
        raise RuntimeError(
            "xgboost_ray_amd HIP extension (_hip_ops) is not built. "
            "Run `python -m xgboost_ray_amd.build` or "
            "`python __graft_entry__.py build` to compile it for gfx950. "
            f"Original error: {e}"
        ) from e
    return _ext


def quantize_gpair(gpair, scale_g, scale_h, return_sums=False):
    if return_sums:
        # (gq, int64 [2] device == gq.sum(0)) from the one quantize pass
        gq, sums = _load().quantize_gpair_sums(
            gpair.contiguous(), scale_g, scale_h)
        return gq, sums
    return _load().quantize_gpair(gpair.contiguous(), scale_g, scale_h)


def apply_tree_binned(bins, margin, feat, split_bin, left, default_left,
                      value):
    """margin[r] += value[leaf(r)], the leaf found by walking the tree over
    row r's bin bytes. Tree arrays are host numpy/torch vectors (feat < 0
    marks a leaf); ``margin`` may be a strided column view (updated in
    place, no contiguous round trip)."""
    _load().apply_tree_binned(
        bins, margin,
        torch.as_tensor(feat, dtype=torch.int32),
        torch.as_tensor(split_bin, dtype=torch.int32),
        torch.as_tensor(left, dtype=torch.int32),
        torch.as_tensor(default_left, dtype=torch.uint8),
        torch.as_tensor(value, dtype=torch.float32),
    )
    return margin


def bin_matrix(values, cuts_flat, cut_ptr):
    return _load().bin_matrix(
        values.contiguous(),
        cuts_flat.to(values.device),
        cut_ptr.to(values.device),
    )


def build_histogram(bins, gpair_q, ridx, starts, counts, n_bins,
                    f_range=None, out=None, pregathered=False):
    K = len(starts)
    F = bins.shape[1]
    if out is None:
        out = torch.zeros(
            (K, F, int(n_bins), 2), dtype=torch.int64, device=bins.device
        )
    f_lo, f_hi = (0, F) if f_range is None else f_range
    return _load().build_histogram(
        bins,
        gpair_q,
        ridx,
        starts,
        counts,
        int(n_bins),
        int(f_lo),
        int(f_hi),
        out,
        bool(pregathered),
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
    """``prev_hist``/``pslots``/``spos``: derive the last ``len(pslots)``
    rows of ``hist`` inside the scan kernel as
    ``prev_hist[pslots] - hist[spos]`` (stored into ``hist``) instead of
    materializing them beforehand. ``reduce=False`` returns the (node,
    feature) scan arrays ``(gain, bin, dl, lg, lh)`` on device for
    ``partition_rows_from_kf``, which folds the per-node reduce into the
    partition plan."""
    import numpy as np

    dev = hist.device
    if monotone is None:
        monotone = torch.zeros(0, dtype=torch.int8, device=dev)
        bounds = torch.zeros((0, 2), dtype=torch.float64, device=dev)
    if allowed is None:
        allowed = torch.zeros(0, dtype=torch.uint8, device=dev)
    else:
        allowed = allowed.to(dev).to(torch.uint8).contiguous()
    derive = (None, None, None)
    if prev_hist is not None and pslots is not None and len(pslots):
        derive = (prev_hist, pslots.to(dev), spos.to(dev))
    args = (
        hist,
        parent_g.to(dev),
        parent_h.to(dev),
        feat_bins.to(dev),
        float(scale_g),
        float(scale_h),
        float(reg_lambda),
        float(reg_alpha),
        float(gamma),
        float(min_child_weight),
        monotone.to(dev).to(torch.int8),
        bounds.to(dev).to(torch.float64),
        allowed,
    )
    if not reduce:
        return tuple(_load().find_splits_kf(*args, *derive))
    (packed,) = _load().find_splits(*args, pull, *derive)
    if not pull:
        return packed  # device [K,6] for the fused single-sync partition
    arr = packed.cpu().numpy()  # ONE D2H for the whole depth's splits
    return {
        "gain": arr[:, 0].astype(np.int32).view(np.float32),
        "feature": arr[:, 1].astype(np.int32),
        "bin": arr[:, 2].astype(np.int32),
        "default_left": arr[:, 3].astype(np.uint8),
        "left_g": arr[:, 4].copy(),
        "left_h": arr[:, 5].copy(),
    }


def partition_rows(bins, ridx, starts, counts, split_feat, split_bin,
                   default_left, gpair_seg=None, bins_t=None):
    dev = bins.device
    if bins_t is None:
        bins_t = torch.zeros(0, dtype=torch.uint8, device=dev)
    if gpair_seg is None:
        gpair_seg = torch.zeros((0, 2), dtype=torch.int32, device=dev)
        r, lc, _ = _load().partition_rows(
            bins, ridx, starts, counts, split_feat, split_bin,
            default_left, gpair_seg, bins_t,
        )
        return r, lc
    return _load().partition_rows(
        bins, ridx, starts, counts, split_feat, split_bin, default_left,
        gpair_seg, bins_t,
    )


def predict_trees(X, feat, thr, left, default_left, value, tree_ptr, out, tree_weight=1.0):
    dev = X.device
    target = out if out.is_contiguous() else out.contiguous()
    _load().predict_trees(
        X.contiguous(),
        feat.to(dev),
        thr.to(dev),
        left.to(dev),
        default_left.to(dev),
        value.to(dev),
        tree_ptr.to(dev),
        target,
        float(tree_weight),
    )
    if target is not out:
        out.copy_(target)
    return out


# -- leaf indices and Saabas contributions -----------------------------------
# Rows per launch are bounded: the device output of one launch stays under
# this size, and the grid of a launch covers exactly its rows.
WALK_OUT_BYTES = 1 << 30
# saabas_contribs launch geometry (measured, docs/parity.md). A workgroup's
# LDS holds one node tile (16 B node + 8 B mean each) and the F+1 float64
# sums of each of its rows: 8 waves with a 1024-node tile at F <= 33, fewer
# rows per workgroup for wider inputs. Where not even 64 rows fit, the sums
# are updated in global memory, which wants few resident rows and big tiles.
SAABAS_LDS_BYTES = 160 * 1024
SAABAS_THREADS = 512
SAABAS_TILE_NODES = 1024
SAABAS_GLOBAL_GEOMETRY = (256, 4096)


def saabas_block_threads(F, tile_nodes=SAABAS_TILE_NODES):
    """Rows per workgroup for F features: the largest multiple of 64, up to
    SAABAS_THREADS, whose sums fit in LDS next to a node tile (0: none)."""
    room = SAABAS_LDS_BYTES - 24 * tile_nodes
    return min(SAABAS_THREADS, room // (8 * (F + 1)) // 64 * 64)


def saabas_lds_max_features():
    """Largest F whose sums stay in LDS."""
    return (SAABAS_LDS_BYTES - 24 * SAABAS_TILE_NODES) // (8 * 64) - 1


def _walk_pack(op, X, feat, thr, left, default_left, tree_ptr, tile_nodes):
    """Check the forest and pack it on X's device: once per op call,
    shared by every row chunk of the call."""
    from xgboost_ray_amd.ops import cpu

    tree_ptr = torch.as_tensor(tree_ptr).to("cpu", torch.int32).contiguous()
    err = cpu.walk_forest_error(feat.cpu().numpy(), left.cpu().numpy(),
                                tree_ptr.numpy(), X.shape[1])
    if err:
        raise ValueError(f"{op}: {err}")
    dev = X.device
    return _load().walk_pack(
        feat.to(dev).contiguous(), thr.to(dev).contiguous(),
        left.to(dev).contiguous(), default_left.to(dev).contiguous(),
        tree_ptr, int(tile_nodes)), len(tree_ptr) - 1


def _row_chunks(n, row_bytes, max_out_bytes):
    chunk = max(1, int(WALK_OUT_BYTES if max_out_bytes is None
                       else max_out_bytes) // max(1, row_bytes))
    return [(s, min(n, s + chunk)) for s in range(0, n, chunk)]


def predict_leaf(X, feat, thr, left, default_left, tree_ptr, out,
                 max_out_bytes=None):
    dev = X.device
    X = X.contiguous()
    forest, T = _walk_pack("predict_leaf", X, feat, thr, left, default_left,
                           tree_ptr, _load().PRED_TILE_NODES)
    n = X.shape[0]
    if tuple(out.shape) != (n, T) or out.dtype != torch.int32:
        raise ValueError(f"predict_leaf: out must be int32 {(n, T)}")
    for s, e in _row_chunks(n, 4 * T, max_out_bytes):
        # the kernel stores through both strides of a device out
        buf = out[s:e] if out.is_cuda else torch.empty(
            (e - s, T), dtype=torch.int32, device=dev)
        _load().predict_leaf(X[s:e], forest, buf)
        if not out.is_cuda:
            # copy this chunk out before the next one runs
            out[s:e] = buf.cpu()
    return out


def saabas_contribs(X, feat, thr, left, default_left, node_mean, tree_ptr,
                    out, max_out_bytes=None, lds_accumulators=None,
                    block_threads=None, tile_nodes=None):
    """``block_threads`` / ``tile_nodes`` override the launch geometry
    (benchmarks/bench_ops.py sweeps them)."""
    dev = X.device
    X = X.contiguous()
    n, F = X.shape
    if tuple(out.shape) != (n, F + 1) or out.dtype != torch.float64:
        raise ValueError(f"saabas_contribs: out must be float64 {(n, F + 1)}")
    mean = node_mean.to(dev).contiguous()
    lds_acc = -1 if lds_accumulators is None else int(bool(lds_accumulators))
    threads, tile = saabas_block_threads(F), SAABAS_TILE_NODES
    if lds_acc == 0 or (threads == 0 and lds_acc < 0):
        threads, tile = SAABAS_GLOBAL_GEOMETRY
    threads = int(block_threads or threads or 64)  # 64: the misfit error
    forest, _ = _walk_pack("saabas_contribs", X, feat, thr, left,
                           default_left, tree_ptr, tile_nodes or tile)
    direct = out.is_cuda and (n == 0 or out.stride(1) == 1)
    for s, e in _row_chunks(n, 8 * (F + 1), max_out_bytes):
        # the sums start from what out holds: a chunk that is not
        # accumulated in place goes to the device first and comes back
        buf = out[s:e] if direct else out[s:e].to(dev).contiguous()
        _load().saabas_contribs(X[s:e], forest, mean, buf, lds_acc, threads)
        if not direct:
            out[s:e] = buf.to(out.device)
    return out


def lambdarank_grad(margin, label, group_ptr, rank, idcg, use_ndcg):
    return _load().lambdarank_grad(
        margin, label, group_ptr, rank, idcg, bool(use_ndcg)
    )


def update_margins(margin, ridx, starts, counts, leaf_values,
                   ridx_b=None, parity=None):
    # starts/counts/leaf_values stay on the HOST: the extension stages
    # all control data through ONE pinned H2D (a .to(dev) here forced a
    # pointless H2D + synchronizing D2H round-trip per round).
    # ridx_b/parity: ping-pong leaf buffers (parity[k] selects which
    # buffer node k's rows last landed in).
    lv = torch.as_tensor(leaf_values, dtype=torch.float32)
    rb = ridx_b if ridx_b is not None else torch.zeros(
        0, dtype=torch.int32, device=margin.device)
    par = (torch.as_tensor(parity, dtype=torch.int64)
           if parity is not None
           else torch.zeros(0, dtype=torch.int64))
    target = margin if margin.is_contiguous() else margin.contiguous()
    _load().update_margins(target, ridx, starts, counts, lv, rb, par)
    if target is not margin:
        margin.copy_(target)
    return margin


def leaf_quantile_hist(resid, weight, ridx, starts, counts, prefix, pass_idx,
                       out, ridx_b=None, parity=None):
    # starts/counts/parity/prefix stay on the HOST (one pinned H2D, as in
    # update_margins).
    dev = resid.device
    w = weight if weight is not None else torch.zeros(
        0, dtype=torch.int64, device=dev)
    rb = ridx_b if ridx_b is not None else torch.zeros(
        0, dtype=torch.int32, device=dev)
    par = (torch.as_tensor(parity, dtype=torch.int64)
           if parity is not None and ridx_b is not None
           else torch.zeros(0, dtype=torch.int64))
    _load().leaf_quantile_hist(
        resid, w, ridx, rb,
        torch.as_tensor(starts, dtype=torch.int64),
        torch.as_tensor(counts, dtype=torch.int64),
        par, torch.as_tensor(prefix, dtype=torch.int64),
        int(pass_idx), out,
    )
    return out


# -- gradient-based row sampling ---------------------------------------------
def mvs_score(gpair, mx_g, mx_h):
    from xgboost_ray_amd.ops import cpu

    return _load().mvs_score(gpair.contiguous(), cpu.mvs_scale(mx_g, mx_h))


def mvs_stats(c):
    return _load().mvs_stats(c)


def mvs_hist(c, prefix, pass_idx):
    return _load().mvs_hist(c, int(prefix), int(pass_idx))


def mvs_threshold(c, k):
    # the digit choice is the oracle's host code over this backend's kernels
    from xgboost_ray_amd.ops import cpu

    return cpu.mvs_threshold(c, k, stats=mvs_stats, hist=mvs_hist)


def mvs_sample(gpair, c, S, M, key):
    key = int(key) & ((1 << 64) - 1)
    if key >= 1 << 63:
        key -= 1 << 64  # the uint64 bits, passed as int64
    keep, out = _load().mvs_sample(gpair.contiguous(), c, int(S), int(M), key)
    return keep, out


def grad_fused(margin, label, weight, scale_pos_weight, mode):
    w = weight if weight is not None else torch.zeros(
        0, dtype=torch.float32, device=margin.device)
    gpair, absmax = _load().grad_fused(
        margin.contiguous(), label.contiguous().float(),
        w.contiguous().float() if w.numel() else w,
        float(scale_pos_weight), int(mode),
    )
    return gpair, absmax


# partition chunk geometry (PART_THREADS * PART_ROWS_PER_THREAD in
# kernels.hip); the python side needs it only to BOUND the fused
# partition grid
PART_CHUNK = 2048


def fused_glue_enabled():
    """RXGB_FUSED_GLUE (default on; "0" restores the separate derive /
    reduce / plan / fill / pull composition). Read per call, so callers
    decide per tree and tests can toggle it within one process."""
    return os.environ.get("RXGB_FUSED_GLUE", "1") != "0"


def _partition_args(bins, gseg, bins_t, ridx_dest):
    dev = bins.device
    if bins_t is None:
        bins_t = torch.zeros(0, dtype=torch.uint8, device=dev)
    if gseg is None:
        gseg = torch.zeros((0, 2), dtype=torch.int32, device=dev)
    rd = ridx_dest if ridx_dest is not None else torch.zeros(
        0, dtype=torch.int32, device=bins.device)
    return gseg, bins_t, rd


def _scatter_after_pull(ridx, gseg, out, chunk_bound):
    # out: [ridx_out, gseg_out, pull, meta, scalars, left_before,
    #       node_left_total, flags, chunk_bound]
    ev = torch.cuda.Event()
    ev.record()  # after plan+count+prefix+pull, BEFORE the scatter
    _load().partition_scatter_planned(
        ridx, out[0], gseg, out[1], out[3], out[4], out[5], out[6],
        out[7], int(chunk_bound),
    )
    return out[0], out[1], out[2], ev


def partition_rows_from_packed(bins, ridx, starts_ord, counts_ord, packed,
                               gseg, bins_t, chunk_bound, ridx_dest=None,
                               fused_glue=None):
    """Single-sync partition: consumes find_splits' device packed output
    (plan + count + prefix + scatter all device-planned); returns
    (ridx_out, gseg_out, pull, ev) where `pull` is a pinned i64 [7K]
    buffer [packed rows | left_counts] valid once `ev` has completed.
    ``fused_glue`` (default: RXGB_FUSED_GLUE) drops the zero fills and
    takes the shuffle-scan prefix kernel."""
    if fused_glue is None:
        fused_glue = fused_glue_enabled()
    gseg, bins_t, rd = _partition_args(bins, gseg, bins_t, ridx_dest)
    out = _load().partition_rows_from_packed(
        bins, ridx, starts_ord, counts_ord, packed, gseg, bins_t,
        int(chunk_bound), rd, bool(fused_glue),
    )
    return _scatter_after_pull(ridx, gseg, out, chunk_bound)


def partition_rows_from_kf(bins, ridx, starts_ord, counts_ord, kf, gseg,
                           bins_t, chunk_bound, ridx_dest=None):
    """partition_rows_from_packed fed by ``find_splits(reduce=False)``:
    the per-node reduce and the partition plan run as one kernel, `packed`
    and the left totals share one device buffer and reach the host in one
    copy. Same return value."""
    gseg, bins_t, rd = _partition_args(bins, gseg, bins_t, ridx_dest)
    out = _load().partition_rows_from_kf(
        bins, ridx, starts_ord, counts_ord, *kf, gseg, bins_t,
        int(chunk_bound), rd,
    )
    return _scatter_after_pull(ridx, gseg, out, chunk_bound)


def reduce_plan(kf, starts_ord, counts_ord, fused=True):
    """Per-node best split + partition plan from the (node, feature) scan
    arrays; returns (packed [K,6], meta, scalars [2]) on device."""
    fn = _load().reduce_plan_fused if fused else _load().reduce_plan_legacy
    return tuple(fn(*kf, starts_ord, counts_ord))


def partition_begin(bins, ridx, starts, counts, split_feat, split_bin,
                    default_left, gpair_seg=None, bins_t=None,
                    gseg_full_rewrite=True):
    """Launch the partition's count+prefix kernels and return a context
    immediately: host bookkeeping between begin and finish overlaps
    them (and the tree writes after finish overlap the scatter)."""
    dev = bins.device
    if bins_t is None:
        bins_t = torch.zeros(0, dtype=torch.uint8, device=dev)
    if gpair_seg is None:
        gpair_seg = torch.zeros((0, 2), dtype=torch.int32, device=dev)
    st = _load().partition_rows_begin(
        bins, ridx, starts, counts, split_feat, split_bin, default_left,
        gpair_seg, bins_t, bool(gseg_full_rewrite),
    )
    return (ridx, gpair_seg, st)


def partition_finish(ctx):
    ridx, gseg, st = ctx
    if len(st) == 6:  # no chunks: nothing moved
        import torch as _t

        return st[0], _t.zeros(
            st[2].numel(), dtype=_t.int64
        ), st[1]
    r, lc, g = _load().partition_rows_finish(
        ridx, st[0], gseg, st[1], st[2], st[3], st[4], st[5], st[6]
    )
    return r, lc, g


def eval_logloss(margin, label, weight=None):
    w = weight if weight is not None else torch.zeros(
        0, dtype=torch.float32, device=margin.device)
    return _load().eval_logloss(
        margin.contiguous(), label.contiguous().float(),
        w.contiguous().float() if w.numel() else w,
    )


def eval_auc_hist(margin, label, n_bins):
    return _load().eval_auc_hist(
        margin.contiguous(), label.contiguous().float(), int(n_bins)
    )


# -- path-form TreeSHAP ------------------------------------------------------
# Rows per launch are bounded: the float64 device output of one launch
# stays under these sizes (interactions write (F+1)^2 values per row) and
# each chunk is added into ``out`` before the next one runs.
SHAP_OUT_BYTES = 1 << 30
SHAP_INTER_OUT_BYTES = 1 << 28


def shap_tile_elems():
    """Path elements one LDS tile of the kernel holds."""
    return int(_load().SHAP_TILE_ELEMS)


def _shap_device_paths(paths, dev):
    """Upload (once per device) the path arrays in the kernel's packing."""
    import numpy as np

    key = str(dev)
    cache = paths.setdefault("_device", {})
    if key not in cache:
        E = len(paths["feature"])
        elem = np.zeros((E, 4), np.int32)
        elem[:, 0] = paths["feature"] | (
            paths["miss_ok"].astype(np.int32) << 31)
        elem[:, 1] = paths["lo"].view(np.int32)
        elem[:, 2] = paths["hi"].view(np.int32)
        cache[key] = (
            torch.from_numpy(elem).to(dev),
            torch.from_numpy(paths["zero_fraction"]).to(dev),
            torch.from_numpy(np.ascontiguousarray(paths["path_ptr"])),
            torch.from_numpy(paths["value"]).to(dev),
            torch.from_numpy(paths["group"]).to(dev),
        )
    return cache[key]


def _tree_shap_chunked(X, paths, n_groups, out, interactions, max_out_bytes):
    from xgboost_ray_amd.ops import cpu

    cpu._shap_check(X, paths, n_groups)
    dev = X.device
    X = X.contiguous()
    n = X.shape[0]
    elem, zf, ptr, val, grp = _shap_device_paths(paths, dev)
    per_row = out[0].numel() if n else 1
    chunk = max(1, int(max_out_bytes) // (8 * per_row))
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        direct = out.is_cuda and out.is_contiguous()
        buf = out[s:e] if direct else torch.zeros(
            (e - s,) + tuple(out.shape[1:]), dtype=torch.float64, device=dev)
        _load().tree_shap(X[s:e], elem, zf, ptr, val, grp, buf,
                          int(n_groups), bool(interactions))
        if not direct:
            # copy this chunk out before the next one runs
            out[s:e] += buf.to(out.device)
    return out


def tree_shap(X, paths, n_groups, out, max_out_bytes=None):
    expect = (X.shape[0], int(n_groups), X.shape[1] + 1)
    if tuple(out.shape) != expect or out.dtype != torch.float64:
        raise ValueError(f"tree_shap: out must be float64 {expect}")
    return _tree_shap_chunked(
        X, paths, n_groups, out, False,
        SHAP_OUT_BYTES if max_out_bytes is None else max_out_bytes)


def tree_shap_interactions(X, paths, out, max_out_bytes=None):
    expect = (X.shape[0], X.shape[1] + 1, X.shape[1] + 1)
    if tuple(out.shape) != expect or out.dtype != torch.float64:
        raise ValueError(f"tree_shap_interactions: out must be float64 "
                         f"{expect}")
    return _tree_shap_chunked(
        X, paths, 1, out, True,
        SHAP_INTER_OUT_BYTES if max_out_bytes is None else max_out_bytes)
