"""Pure-PyTorch CPU reference implementations of the engine ops.

These are the numerics oracle: the HIP kernels in ``csrc/`` are tested for
bitwise (integer ops) / close (float ops) agreement against these functions.
Integer fixed-point histogram accumulation makes the CPU and GPU training
paths produce identical trees.
"""

import torch

MISSING_BIN = 255


def quantize_gpair(gpair: torch.Tensor, scale_g: float, scale_h: float) -> torch.Tensor:
    # int32 packed pairs: |q| <= 2^30 by scale construction; accumulators
    # are int64 so any sum is exact
    out = torch.empty(gpair.shape, dtype=torch.int32, device=gpair.device)
    out[:, 0] = torch.round(gpair[:, 0].double() * scale_g).to(torch.int32)
    out[:, 1] = torch.round(gpair[:, 1].double() * scale_h).to(torch.int32)
    return out


def bin_matrix(values: torch.Tensor, cuts_flat: torch.Tensor, cut_ptr: torch.Tensor):
    n, F = values.shape
    out = torch.empty((n, F), dtype=torch.uint8, device=values.device)
    for f in range(F):
        lo, hi = int(cut_ptr[f]), int(cut_ptr[f + 1])
        nb = hi - lo
        col = values[:, f]
        if nb == 0:
            out[:, f] = torch.where(
                torch.isnan(col),
                torch.tensor(MISSING_BIN, dtype=torch.uint8),
                torch.tensor(0, dtype=torch.uint8),
            )
            continue
        cuts = cuts_flat[lo:hi].contiguous()
        # XGBoost HistogramCuts::SearchBin semantics: bin = count of cuts
        # <= value (upper_bound), clamped to nb - 1. Bin b covers
        # [cut[b-1], cut[b]), so a split after bin b <=> "v < cut[b] goes
        # left" - exactly the float threshold rule used at predict time.
        b = torch.searchsorted(cuts, col.contiguous(), side="right")
        b = torch.clamp(b, max=nb - 1).to(torch.uint8)
        b = torch.where(torch.isnan(col), torch.full_like(b, MISSING_BIN), b)
        out[:, f] = b
    return out


def build_histogram(bins, gpair_q, ridx, starts, counts, n_bins,
                    f_range=None, out=None, pregathered=False):
    K = len(starts)
    n, F = bins.shape
    hist = out
    if hist is None:
        hist = torch.zeros(
            (K, F, n_bins, 2), dtype=torch.int64, device=bins.device
        )
    f_lo, f_hi = (0, F) if f_range is None else f_range
    return _build_histogram_range(
        bins, gpair_q, ridx, starts, counts, n_bins, f_lo, f_hi, hist,
        pregathered
    )


def _build_histogram_range(bins, gpair_q, ridx, starts, counts, n_bins,
                           f_lo, f_hi, hist, pregathered=False):
    K = len(starts)
    n, F = bins.shape
    foff = torch.arange(f_lo, f_hi, dtype=torch.int64) * n_bins
    for k in range(K):
        s, c = int(starts[k]), int(counts[k])
        if c == 0:
            continue
        idx = ridx[s : s + c].long()
        rb = bins[idx][:, f_lo:f_hi].long()  # [c, fr]
        valid = rb != MISSING_BIN
        flat = foff.unsqueeze(0) + rb  # [c, F]
        gsrc = gpair_q[s : s + c] if pregathered else gpair_q[idx]
        g = gsrc[:, 0].long().unsqueeze(1).expand_as(flat)
        h = gsrc[:, 1].long().unsqueeze(1).expand_as(flat)
        hk = hist[k].view(F * n_bins, 2)
        fidx = flat[valid]
        hk[:, 0].scatter_add_(0, fidx, g[valid])
        hk[:, 1].scatter_add_(0, fidx, h[valid])
    return hist


def _calc_score(G, H, reg_lambda, reg_alpha):
    """XGBoost split score: ThresholdL1(G, alpha)^2 / (H + lambda)."""
    if reg_alpha > 0:
        G = torch.sign(G) * torch.clamp(G.abs() - reg_alpha, min=0.0)
    denom = H + reg_lambda
    return torch.where(denom > 0, G * G / denom, torch.zeros_like(G))


def _calc_weight_t(G, H, reg_lambda, reg_alpha):
    if reg_alpha > 0:
        G = torch.sign(G) * torch.clamp(G.abs() - reg_alpha, min=0.0)
    denom = H + reg_lambda
    return torch.where(denom > 0, -G / denom, torch.zeros_like(G))


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
):
    K, F, B, _ = hist.shape
    dev = hist.device
    # Dequantize to double for the scan: scan math must be identical on CPU
    # and GPU, and the quantized ints are exactly representable in f64.
    # Multiply by the (identically computed) reciprocal instead of dividing:
    # f64 division is ~10x the cost of multiply on CDNA4 and the GPU kernel
    # mirrors this exact op order.
    inv_g = 1.0 / scale_g
    inv_h = 1.0 / scale_h
    gq = hist[..., 0]
    hq = hist[..., 1]

    # Left-sum prefixes are computed in INT64 (exact under any summation
    # order) and dequantized once per bin: every bin's gain is then
    # independent of its neighbours, which is what lets the GPU scan run
    # one 64-lane wave per (node, feature) with a parallel int wave-scan
    # and still be bitwise-identical to this oracle.
    GLq = torch.cumsum(gq, dim=2)
    HLq = torch.cumsum(hq, dim=2)
    GL = GLq.double() * inv_g
    HL = HLq.double() * inv_h
    Gp = (parent_g.double() * inv_g).view(K, 1, 1)
    Hp = (parent_h.double() * inv_h).view(K, 1, 1)
    # Missing mass per (node, feature) = parent - feature total.
    Gmiss = Gp - GL[:, :, -1:].clone()
    Hmiss = Hp - HL[:, :, -1:].clone()

    parent_score = _calc_score(Gp, Hp, reg_lambda, reg_alpha)

    # Candidate split after bin b (left = bins <= b); last bin excluded.
    bin_idx = torch.arange(B, device=dev).view(1, 1, B)
    valid_bin = bin_idx < (feat_bins.to(dev).view(1, F, 1) - 1)

    best = {
        "gain": torch.full((K,), -1.0, dtype=torch.float64, device=dev),
        "feature": torch.full((K,), -1, dtype=torch.int32, device=dev),
        "bin": torch.zeros((K,), dtype=torch.int32, device=dev),
        "default_left": torch.zeros((K,), dtype=torch.uint8, device=dev),
        "left_g": torch.zeros((K,), dtype=torch.int64, device=dev),
        "left_h": torch.zeros((K,), dtype=torch.int64, device=dev),
    }

    for default_left in (1, 0):
        if default_left:
            gl, hl = GL + Gmiss, HL + Hmiss
        else:
            gl, hl = GL, HL
        gr, hr = Gp - gl, Hp - hl
        ok = (
            valid_bin
            & (hl >= min_child_weight)
            & (hr >= min_child_weight)
        )
        if allowed is not None:
            # interaction constraints: per-(node, feature) gate
            ok = ok & (allowed.to(dev) != 0).view(K, F, 1)
        if monotone is not None:
            # monotone constraints: clamp child weights into the node's
            # bound interval, then require the constrained ordering
            c = monotone.to(dev).view(1, F, 1)
            lo = bounds[:, 0].to(dev).view(K, 1, 1)
            up = bounds[:, 1].to(dev).view(K, 1, 1)
            wl = torch.clamp(
                _calc_weight_t(gl, hl, reg_lambda, reg_alpha), lo, up
            )
            wr = torch.clamp(
                _calc_weight_t(gr, hr, reg_lambda, reg_alpha), lo, up
            )
            ok = ok & torch.where(
                c > 0, wl <= wr, torch.where(c < 0, wl >= wr,
                                             torch.ones_like(ok)),
            )
        gain = (
            0.5
            * (
                _calc_score(gl, hl, reg_lambda, reg_alpha)
                + _calc_score(gr, hr, reg_lambda, reg_alpha)
                - parent_score
            )
            - gamma
        )
        gain = torch.where(ok, gain, torch.full_like(gain, -float("inf")))
        flat = gain.view(K, F * B)
        mx, arg = flat.max(dim=1)
        upd = mx > best["gain"]
        f_sel = (arg // B).to(torch.int32)
        b_sel = (arg % B).to(torch.int32)
        best["gain"] = torch.where(upd, mx, best["gain"])
        best["feature"] = torch.where(upd, f_sel, best["feature"])
        best["bin"] = torch.where(upd, b_sel, best["bin"])
        best["default_left"] = torch.where(
            upd,
            torch.full((K,), default_left, dtype=torch.uint8, device=dev),
            best["default_left"],
        )
        karange = torch.arange(K, device=dev)
        lgq = GLq[karange, f_sel.long(), b_sel.long()]
        lhq = HLq[karange, f_sel.long(), b_sel.long()]
        if default_left:
            # left child also receives the missing mass (exact in quantized
            # space: parent_q - feature_total_q).
            lgq = lgq + (parent_g - GLq[:, :, -1][karange, f_sel.long()])
            lhq = lhq + (parent_h - HLq[:, :, -1][karange, f_sel.long()])
        best["left_g"] = torch.where(upd, lgq, best["left_g"])
        best["left_h"] = torch.where(upd, lhq, best["left_h"])

    # contract: outputs are host numpy arrays (the driver consumes them on
    # the host; returning numpy makes the GPU path's single packed D2H
    # transfer natural)
    return {
        "gain": best["gain"].float().cpu().numpy(),
        "feature": best["feature"].cpu().numpy(),
        "bin": best["bin"].cpu().numpy(),
        "default_left": best["default_left"].cpu().numpy(),
        "left_g": best["left_g"].cpu().numpy(),
        "left_h": best["left_h"].cpu().numpy(),
    }


def partition_rows(bins, ridx, starts, counts, split_feat, split_bin,
                   default_left, gpair_seg=None, bins_t=None):
    K = len(starts)
    out = ridx.clone()
    gout = None if gpair_seg is None else gpair_seg.clone()
    left_counts = torch.zeros(K, dtype=torch.int64)
    for k in range(K):
        s, c = int(starts[k]), int(counts[k])
        if c == 0:
            continue
        idx = ridx[s : s + c]
        fv = bins[idx.long(), int(split_feat[k])]
        miss = fv == MISSING_BIN
        go_left = fv <= int(split_bin[k])
        if int(default_left[k]):
            go_left = go_left | miss
        else:
            go_left = go_left & ~miss
        out[s : s + c] = torch.cat([idx[go_left], idx[~go_left]])
        if gout is not None:
            gseg = gpair_seg[s : s + c]
            gout[s : s + c] = torch.cat([gseg[go_left], gseg[~go_left]])
        left_counts[k] = int(go_left.sum())
    if gout is None:
        return out, left_counts
    return out, left_counts, gout


def predict_trees(X, feat, thr, left, default_left, value, tree_ptr, out, tree_weight=1.0):
    n = X.shape[0]
    T = len(tree_ptr) - 1
    rows = torch.arange(n)
    for t in range(T):
        base = int(tree_ptr[t])
        cur = torch.full((n,), base, dtype=torch.int64)
        while True:
            f = feat[cur].long()
            is_leaf = f < 0
            if bool(is_leaf.all()):
                break
            # full-width level step with self-looping leaves: the
            # boolean-mask variant paid a nonzero + gather + clone per
            # level, several times this version's cost
            x = X[rows, f.clamp(min=0)]
            go_left = torch.where(
                torch.isnan(x), default_left[cur].bool(), x < thr[cur]
            )
            la = left[cur].long()
            nxt = torch.where(go_left, la, la + 1) + base
            cur = torch.where(is_leaf, cur, nxt)
        out += value[cur] * tree_weight
    return out


def walk_forest_error(feat, left, tree_ptr, n_features):
    """Why the tree walks cannot take this forest, or None: an empty
    tree, a split feature outside ``[0, n_features)``, or a child pair
    that lies outside its tree or does not come after its parent (every
    walk then ends, and every index it forms is in range)."""
    import numpy as np

    feat, left = np.asarray(feat), np.asarray(left)
    ptr = np.asarray(tree_ptr, dtype=np.int64)
    if len(ptr) < 1 or ptr[0] != 0 or ptr[-1] != len(feat):
        return "tree_ptr does not span the node arrays"
    if len(left) != len(feat):
        return "forest arrays differ in length"
    sizes = np.diff(ptr)
    if (sizes <= 0).any():
        return "a tree has no nodes"
    split = feat >= 0
    if (feat[split] >= n_features).any():
        return (f"forest splits on feature {int(feat.max())}, X has "
                f"{n_features} columns")
    rel = np.arange(len(feat)) - np.repeat(ptr[:-1], sizes)
    size = np.repeat(sizes, sizes)
    lc = left[split].astype(np.int64)
    if ((lc <= rel[split]) | (lc + 1 >= size[split])).any():
        return "a split's children lie outside its tree or before it"
    return None


def _walk_check(op, X, feat, left, tree_ptr):
    err = walk_forest_error(_as_numpy(feat), _as_numpy(left),
                            _as_numpy(tree_ptr), X.shape[1])
    if err:
        raise ValueError(f"{op}: {err}")


def _walk_levels(X, feat, thr, left, default_left, base):
    """One tree, level by level: yields (rows still at a split, their node,
    the child they move to), node indices absolute."""
    import numpy as np

    cur = np.full(X.shape[0], base, np.int64)
    rows = np.arange(X.shape[0])
    while True:
        rows = rows[feat[cur[rows]] >= 0]
        if not len(rows):
            return
        node = cur[rows]
        x = X[rows, feat[node]]
        with np.errstate(invalid="ignore"):
            go_left = np.where(np.isnan(x), default_left[node] != 0,
                               x < thr[node])
        child = base + left[node] + np.where(go_left, 0, 1)
        yield rows, node, child
        cur[rows] = child


def predict_leaf(X, feat, thr, left, default_left, tree_ptr, out,
                 max_out_bytes=None):
    """Numerics oracle of the leaf-index walk (contract: ``ops.predict_leaf``),
    numpy on the host."""
    import numpy as np

    _walk_check("predict_leaf", X, feat, left, tree_ptr)
    Xn, o = _as_numpy(X), _as_numpy(out)
    arrs = [_as_numpy(a) for a in (feat, thr, left, default_left)]
    ptr = _as_numpy(tree_ptr)
    if o.shape != (Xn.shape[0], len(ptr) - 1) or o.dtype != np.int32:
        raise ValueError("predict_leaf: out must be int32 [n, T]")
    for t in range(len(ptr) - 1):
        base = int(ptr[t])
        o[:, t] = 0
        for rows, _, child in _walk_levels(Xn, *arrs, base):
            o[rows, t] = child - base
    return out


def saabas_contribs(X, feat, thr, left, default_left, node_mean, tree_ptr,
                    out, max_out_bytes=None, lds_accumulators=None):
    """Numerics oracle of the Saabas walk (contract: ``ops.saabas_contribs``),
    numpy on the host. A row meets one split per level, so each level's
    fancy-indexed add touches a cell once and the per-cell order is the
    tree-then-depth order of the contract."""
    import numpy as np

    _walk_check("saabas_contribs", X, feat, left, tree_ptr)
    Xn, o, mean = _as_numpy(X), _as_numpy(out), _as_numpy(node_mean)
    arrs = [_as_numpy(a) for a in (feat, thr, left, default_left)]
    ptr = _as_numpy(tree_ptr)
    F = Xn.shape[1]
    if o.shape != (Xn.shape[0], F + 1) or o.dtype != np.float64:
        raise ValueError("saabas_contribs: out must be float64 [n, F+1]")
    if mean.dtype != np.float64 or mean.shape != arrs[0].shape:
        raise ValueError("saabas_contribs: node_mean must be float64 "
                         "[n_nodes]")
    for t in range(len(ptr) - 1):
        base = int(ptr[t])
        o[:, F] = o[:, F] + mean[base]
        for rows, node, child in _walk_levels(Xn, *arrs, base):
            f = arrs[0][node]
            o[rows, f] = o[rows, f] + (mean[child] - mean[node])
    return out


def update_margins(margin, ridx, starts, counts, leaf_values):
    for k in range(len(starts)):
        s, c = int(starts[k]), int(counts[k])
        if c:
            margin[ridx[s : s + c].long()] += float(leaf_values[k])
    return margin


def quantile_keys(resid):
    """fp32 -> order-preserving uint32 keys (held in int64): ``-0.0`` folds
    into ``+0.0``, non-negatives get the sign bit set, negatives are
    bit-inverted."""
    u = (resid.float() + 0.0).contiguous().view(torch.int32).long() & 0xFFFFFFFF
    neg = u >= 0x80000000
    return torch.where(neg, u ^ 0xFFFFFFFF, u | 0x80000000)


def leaf_quantile_hist(resid, weight, ridx, starts, counts, prefix, pass_idx,
                       out, ridx_b=None, parity=None):
    """Numerics oracle of the radix-select pass: plain torch, int64 sums."""
    keys = quantile_keys(resid)
    hi_shift = 32 - 8 * pass_idx
    lo_shift = 24 - 8 * pass_idx
    for k in range(len(starts)):
        s, c = int(starts[k]), int(counts[k])
        if not c:
            continue
        src = ridx_b if (parity is not None and int(parity[k])) else ridx
        rows = src[s : s + c].long()
        kk = keys[rows]
        w = (weight[rows] if weight is not None
             else torch.ones(c, dtype=torch.int64))
        if pass_idx:
            m = (kk >> hi_shift) == int(prefix[k])
            kk, w = kk[m], w[m]
        out[k].index_add_(0, (kk >> lo_shift) & 255, w)
    return out


def sketch_pass(X, W, table, n_slots, pass_idx, S, out):
    """One radix-select pass of the weighted sketch (``ops.sketch_pass``),
    feature by feature in plain torch; int64 sums."""
    keys = quantile_keys(X)
    w_all = W.long().clamp(min=0)
    flat = out.view(-1)
    hi_shift = 32 - 8 * pass_idx
    lo_shift = 24 - 8 * pass_idx
    for f in range(X.shape[1]):
        ok = ~torch.isnan(X[:, f])
        kk, w = keys[ok, f], w_all[ok]
        slot = torch.zeros_like(kk)
        if pass_idx:
            tab = table[f, : int(n_slots[f])].long()
            if tab.numel() == 0:
                continue
            pfx = kk >> hi_shift
            slot = torch.searchsorted(tab, pfx).clamp(max=tab.numel() - 1)
            hit = tab[slot] == pfx
            kk, w, slot = kk[hit], w[hit], slot[hit]
        flat.index_add_(
            0, (f * S + slot) * 256 + ((kk >> lo_shift) & 255), w)
    return out


def keys_to_float(keys):
    """Inverse of ``quantile_keys``: int64 keys -> the f32 values."""
    bits = torch.where(keys >= 0x80000000, keys ^ 0x80000000,
                       keys ^ 0xFFFFFFFF)
    bits = bits - ((bits >> 31) << 32)  # wrap into int32
    return bits.to(torch.int32).view(torch.float32)


def weighted_cuts(X, W, max_bin, col_max):
    """Oracle of ``ops.weighted_cuts``: per feature a stable numpy sort by
    key, an int64 cumsum and a searchsorted of the targets."""
    import numpy as np

    from xgboost_ray_amd.engine.quantile import HistogramCuts

    nb = min(int(max_bin), 255)
    Xc = X.detach().cpu().float()
    keys = quantile_keys(Xc).numpy()
    nan = torch.isnan(Xc).numpy()
    w_all = np.maximum(W.detach().cpu().numpy().astype(np.int64), 0)
    cmax = col_max.detach().cpu().numpy().astype(np.float32)
    cuts_list = []
    for f in range(Xc.shape[1]):
        if np.isnan(cmax[f]):
            cuts_list.append(np.zeros(0, np.float32))
            continue
        k, w = keys[~nan[:, f], f], w_all[~nan[:, f]]
        order = np.argsort(k, kind="stable")
        k, cw = k[order], np.cumsum(w[order])
        Wf = int(cw[-1]) if cw.size else 0
        vals = np.zeros(0, np.float32)
        if Wf > 0 and nb > 1:
            q, r = divmod(Wf, nb)
            j = np.arange(1, nb, dtype=np.int64)
            T = j * q + (j * r + nb - 1) // nb
            picked = np.unique(k[np.searchsorted(cw, T, side="left")])
            vals = keys_to_float(torch.from_numpy(picked)).numpy()
        above = np.nextafter(cmax[f], np.float32(np.inf))
        cuts_list.append(
            np.unique(np.concatenate([vals, [above]]).astype(np.float32)))
    ptr = np.zeros(len(cuts_list) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(c) for c in cuts_list])
    flat = (np.concatenate(cuts_list) if ptr[-1] > 0
            else np.zeros(0, dtype=np.float32))
    return HistogramCuts(
        cuts_flat=torch.from_numpy(flat.astype(np.float32)),
        cut_ptr=torch.from_numpy(ptr),
        max_bins=int(max((len(c) for c in cuts_list), default=1)) or 1,
    )


# ---------------------------------------------------------------------------
# Gradient-based row sampling (minimal-variance sampling)
# ---------------------------------------------------------------------------
# Which rows are kept is decided in integer arithmetic only, so these
# oracles and the HIP kernels agree bit for bit (docs/parity.md).
MVS_LAMBDA = 0.1  # weight of h^2 in the score, as in xgboost's sampler
MVS_VMAX = 1 << 60
_U64 = (1 << 64) - 1


def _splitmix64_int(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & _U64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _U64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _U64
    return z ^ (z >> 31)


def mvs_key(seed: int, iteration: int, tree: int, rank: int) -> int:
    """uint64 stream key of one tree on one rank. Row i draws
    ``splitmix64(key + i)``, so the four ingredients are hashed one after
    the other: keys that differ in any of them are far apart."""
    key = 0
    for part in (seed, iteration, tree, rank):
        key = _splitmix64_int((key + int(part)) & _U64)
    return key


def mvs_scale(mx_g: float, mx_h: float) -> float:
    """sv = 2^60 / max(mx_g^2 + 0.1 mx_h^2, 1e-300) in float64 (inf when
    both maxima are zero: every score then clamps to 2^30)."""
    import numpy as np

    mg, mh = np.float64(mx_g), np.float64(mx_h)
    with np.errstate(over="ignore", invalid="ignore"):
        d = mg * mg + np.float64(MVS_LAMBDA) * (mh * mh)
        return float(np.float64(MVS_VMAX) / max(d, np.float64(1e-300)))


def mvs_score(gpair, mx_g, mx_h):
    """c = isqrt(clamp(rne((g^2 + 0.1 h^2) * sv), 2^60)) as uint32 [n],
    sv = ``mvs_scale(mx_g, mx_h)``."""
    import numpy as np

    sv = mvs_scale(mx_g, mx_h)
    gp = gpair.detach().cpu().numpy().astype(np.float64)
    g, h = gp[:, 0], gp[:, 1]
    with np.errstate(over="ignore", invalid="ignore"):
        v = g * g + np.float64(MVS_LAMBDA) * (h * h)
        x = v * np.float64(sv)
        V = np.full(len(x), MVS_VMAX, np.int64)
        m = x < np.float64(MVS_VMAX)  # False for NaN
        V[m] = np.rint(x[m]).astype(np.int64)  # half to even
    V = np.maximum(V, 0)
    # integer square root: float start, then corrected
    r = np.sqrt(V.astype(np.float64)).astype(np.int64)
    for _ in range(4):
        r -= r * r > V
    for _ in range(4):
        r += (r + 1) * (r + 1) <= V
    return torch.from_numpy(r.astype(np.uint32))


def _mvs_c(c):
    import numpy as np

    return c.detach().cpu().numpy().astype(np.int64)


def mvs_stats(c):
    """int64 [3]: (#{c > 0}, max c, sum c)."""
    v = _mvs_c(c)
    if not len(v):
        return torch.zeros(3, dtype=torch.int64)
    return torch.tensor(
        [int((v > 0).sum()), int(v.max()), int(v.sum())], dtype=torch.int64)


def mvs_hist(c, prefix, pass_idx):
    """int64 [256, 2]: per digit (count, sum c) of the rows whose top
    ``8 * pass_idx`` bits equal ``prefix``; digit = the next 8 bits."""
    import numpy as np

    v = _mvs_c(c)
    if pass_idx:
        v = v[(v >> (32 - 8 * pass_idx)) == int(prefix)]
    d = (v >> (24 - 8 * pass_idx)) & 255
    out = np.zeros((256, 2), np.int64)
    np.add.at(out[:, 0], d, 1)
    np.add.at(out[:, 1], d, v)
    return torch.from_numpy(out)


def mvs_threshold(c, k, stats=None, hist=None):
    """(S, M) of the sampling threshold as Python ints - see
    ``ops.mvs_threshold``. ``stats`` / ``hist`` are the backend's
    ``mvs_stats`` / ``mvs_hist`` (default: the oracles above); the digit
    choice after each pass runs here, on the host, in Python ints."""
    stats = stats or mvs_stats
    hist = hist or mvs_hist
    k = int(k)
    n_pos, mx, total = (int(x) for x in stats(c).cpu().tolist())
    if n_pos <= k:
        return 0, 0
    if total >= k * (mx + 1):
        # P(max c + 1) holds: t* > max c, every row is below the threshold
        return total, k
    # MSB-first radix select of t* = the largest t with
    # P(t): A(t) >= (k - N(t)) * t. At a candidate t on a digit boundary
    # A and N follow from the bins below / from the digit on.
    prefix = 0
    below_sum = 0  # sum of c over rows below the prefix's range
    above_cnt = 0  # rows above the prefix's range
    for p in range(4):
        h = hist(c, prefix, p).cpu().numpy()
        cnt, sm = h[:, 0].tolist(), h[:, 1].tolist()
        shift = 24 - 8 * p
        a, nn = below_sum, above_cnt + sum(cnt)
        best = (0, a, nn)  # P holds at the prefix itself (or at t = 0)
        for d in range(256):
            t = ((prefix << 8) | d) << shift
            if a >= (k - nn) * t:
                best = (d, a, nn)
            a += sm[d]
            nn -= cnt[d]
        d, a_t, n_t = best
        below_sum = a_t
        above_cnt = n_t - cnt[d]
        prefix = (prefix << 8) | d
    eq = n_t - above_cnt  # rows with c == t*
    return a_t + eq * prefix, k - above_cnt


def mvs_sample(gpair, c, S, M, key):
    """(keep uint8 [n], reweighted gpair f32 [n, 2]) - see ops.mvs_sample."""
    import numpy as np

    gp = gpair.detach().cpu().numpy().astype(np.float32)
    cc = c.detach().cpu().numpy().astype(np.uint64)
    n = len(cc)
    S, M = int(S), int(M)
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) + np.uint64(int(key) & _U64)
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    u = z >> np.uint64(32)
    cm = cc * np.uint64(M)
    sure = (cc > 0) & (np.bool_(S == 0) | (cm >= np.uint64(S)))
    # floor(u * S / 2^32) < c * M  <=>  u * S < (c * M) * 2^32
    q = u * np.uint64(S >> 32) + (
        (u * np.uint64(S & 0xFFFFFFFF)) >> np.uint64(32))
    prob = (cc > 0) & ~sure & (q < cm)
    out = np.zeros((n, 2), np.float32)
    out[sure] = gp[sure]
    f = np.float64(S) / cm[prob].astype(np.float64)
    out[prob] = (gp[prob].astype(np.float64) * f[:, None]).astype(np.float32)
    keep = (sure | prob).astype(np.uint8)
    return torch.from_numpy(keep), torch.from_numpy(out)


# ---------------------------------------------------------------------------
# Exact TreeSHAP in path form
# ---------------------------------------------------------------------------
# longest root-to-leaf path, counted in UNIQUE features, the path-form ops
# accept (the HIP kernel sizes its per-row weight column by it)
SHAP_MAX_PATH_LEN = 32


def _as_numpy(a):
    return a.detach().numpy() if isinstance(a, torch.Tensor) else a


def shap_paths(trees, scales=1.0, groups=None):
    """Flatten a forest into independent root-to-leaf paths (the
    GPUTreeShap formulation of Lundberg's TreeSHAP).

    One path per leaf, one ELEMENT per unique feature on it. Repeated
    splits on a feature merge into one element carrying

    - ``feature``        int32
    - ``lo``, ``hi``     float32 half-open interval of thresholds, from
      (-inf, +inf): going left at ``thr`` sets hi = min(hi, thr), going
      right sets lo = max(lo, thr). ``hi == +inf`` means "no upper bound"
      (a row value of +inf takes every right branch, so it lies inside)
    - ``miss_ok``        uint8, AND over the merged splits of "default
      direction == direction taken"
    - ``zero_fraction``  float64 product of cover[child] / c with
      c = cover[parent] if cover[parent] > 0 else 1.0, multiplied in
      split order exactly as ``booster._tree_shap`` does.

    Elements are ordered by the LAST split on their feature, the order
    ``_tree_shap`` holds them in. Per path: ``path_ptr`` int32 [P+1]
    offsets into the element arrays, ``value`` float64 leaf value x the
    tree's scale, ``group`` int32 output group. ``bias`` float64
    [n_groups] sums mean_val[0] * scale per group. ``max_len`` is the
    longest path in elements; the ops refuse > SHAP_MAX_PATH_LEN.

    scales / groups: one number for all trees, or one per tree.
    """
    import numpy as np

    from xgboost_ray_amd.booster import _fill_node_means

    T = len(trees)
    scales = [float(scales)] * T if np.isscalar(scales) else list(scales)
    groups = [0] * T if groups is None else [int(g) for g in groups]
    n_groups = max(groups) + 1 if groups else 1
    feature, lo, hi, miss_ok, zf = [], [], [], [], []
    ptr, value, group, tree_id = [0], [], [], []
    bias = np.zeros(n_groups, np.float64)
    n_features = 0
    for ti, t in enumerate(trees):
        scale = scales[ti]
        cover = t.cover.astype(np.float64)
        mean_val = np.zeros(t.num_nodes, np.float64)
        _fill_node_means(t, mean_val, cover)
        bias[groups[ti]] += mean_val[0] * scale
        stack = [(0, ())]
        while stack:
            nid, elems = stack.pop()
            f = int(t.feat[nid])
            if f < 0:
                for e in elems:
                    feature.append(e[0])
                    lo.append(e[1])
                    hi.append(e[2])
                    miss_ok.append(e[3])
                    zf.append(e[4])
                ptr.append(len(feature))
                # same arithmetic as _tree_shap's ``value * scale``
                value.append(float(t.value[nid] * scale))
                group.append(groups[ti])
                tree_id.append(ti)
                continue
            n_features = max(n_features, f + 1)
            left = int(t.left[nid])
            c = cover[nid] if cover[nid] > 0 else 1.0
            thr = np.float32(t.thr[nid])
            dleft = bool(t.default_left[nid])
            old = next((e for e in elems if e[0] == f), None)
            rest = tuple(e for e in elems if e[0] != f)
            if old is None:
                old = (f, np.float32(-np.inf), np.float32(np.inf), True, 1.0)
            # right child pushed first so leaves come out left to right
            stack.append((left + 1, rest + ((
                f, max(old[1], thr), old[2], old[3] and not dleft,
                old[4] * cover[left + 1] / c),)))
            stack.append((left, rest + ((
                f, old[1], min(old[2], thr), old[3] and dleft,
                old[4] * cover[left] / c),)))
    path_ptr = np.asarray(ptr, np.int32)
    lens = np.diff(path_ptr)
    return {
        "feature": np.asarray(feature, np.int32),
        "lo": np.asarray(lo, np.float32),
        "hi": np.asarray(hi, np.float32),
        "miss_ok": np.asarray(miss_ok, np.uint8),
        "zero_fraction": np.asarray(zf, np.float64),
        "path_ptr": path_ptr,
        "value": np.asarray(value, np.float64),
        "group": np.asarray(group, np.int32),
        "tree": np.asarray(tree_id, np.int32),
        "bias": bias,
        "n_groups": n_groups,
        "n_features": n_features,
        "max_len": int(lens.max()) if len(lens) else 0,
    }


def _shap_check(X, paths, n_groups):
    if paths["max_len"] > SHAP_MAX_PATH_LEN:
        raise ValueError(
            f"tree_shap: a path has {paths['max_len']} unique features, "
            f"the path-form op supports {SHAP_MAX_PATH_LEN}"
        )
    if paths["n_features"] > X.shape[1]:
        raise ValueError(
            f"tree_shap: forest splits on feature {paths['n_features'] - 1}"
            f" but X has {X.shape[1]} columns"
        )
    if paths["n_groups"] > n_groups:
        raise ValueError("tree_shap: path group outside n_groups")


def _shap_one_fractions(Xn, paths, e0, e1):
    """[m, n] float64: 1 where the row follows the element's splits."""
    import numpy as np

    x = Xn[:, paths["feature"][e0:e1]].T  # [m, n] float32
    lo = paths["lo"][e0:e1, None]
    hi = paths["hi"][e0:e1, None]
    inside = (x >= lo) & ((x < hi) | np.isposinf(hi))
    miss = paths["miss_ok"][e0:e1, None].astype(bool)
    return np.where(np.isnan(x), miss, inside).astype(np.float64)


def _shap_extend(z, o):
    """Permutation weights of a whole path: ``_tree_shap``'s EXTEND run
    over the dummy root element and then every element. [m+1, n]."""
    import numpy as np

    m, n = o.shape
    w = np.zeros((m + 1, n), np.float64)
    w[0] = 1.0
    for k in range(1, m + 1):
        pz, po = z[k - 1], o[k - 1]
        ln = k + 1
        for i in range(k - 1, -1, -1):
            w[i + 1] += po * w[i] * (i + 1) / ln
            w[i] = pz * w[i] * (ln - 1 - i) / ln
    return w


def _shap_unwound_sum(w, ln, pz, po):
    """``_tree_shap``'s unwind_sum for an element (pz scalar, po [n] of
    0/1) of a path with weights w[0..ln]; both branches, selected by po."""
    import numpy as np

    hot = np.zeros(w.shape[1], np.float64)
    nxt = w[ln]
    for j in range(ln - 1, -1, -1):
        tmp = nxt * (ln + 1) / ((j + 1) * 1.0)
        hot = hot + tmp
        nxt = w[j] - tmp * pz * (ln - j) / (ln + 1)
    cold = np.zeros(w.shape[1], np.float64)
    for j in range(ln):
        cold = cold + w[j] * (ln + 1) / (pz * (ln - j))
    return np.where(po != 0.0, hot, cold)


def _shap_unwind(w, ln, pz, po):
    """Weights of the path with one element removed ([ln, n])."""
    import numpy as np

    hot = np.empty((ln, w.shape[1]), np.float64)
    cold = np.empty_like(hot)
    nxt = w[ln]
    for j in range(ln - 1, -1, -1):
        tmp = nxt * (ln + 1) / ((j + 1) * 1.0)
        nxt = w[j] - tmp * pz * (ln - j) / (ln + 1)
        hot[j] = tmp
        cold[j] = w[j] * (ln + 1) / (pz * (ln - j))
    return np.where(po[None, :] != 0.0, hot, cold)


def tree_shap(X, paths, n_groups, out, max_out_bytes=None):
    """Path-form exact TreeSHAP, float64 numpy, vectorised over rows:
    the numerics oracle of the HIP kernel (contract: ``ops.tree_shap``).

    A path on which some element has one_fraction == 0 AND
    zero_fraction == 0 contributes nothing for that row (every subset
    term carries one of the two factors) and is skipped - the recursion
    divides 0 by 0 there. ``max_out_bytes`` is the GPU wrapper's chunk
    bound and means nothing here."""
    import numpy as np

    Xn, outn = _as_numpy(X), _as_numpy(out)
    _shap_check(Xn, paths, n_groups)
    ptr, zf = paths["path_ptr"], paths["zero_fraction"]
    with np.errstate(divide="ignore", invalid="ignore"):
        for p in range(len(ptr) - 1):
            e0, e1 = int(ptr[p]), int(ptr[p + 1])
            m = e1 - e0
            if m == 0:
                continue
            z = zf[e0:e1]
            o = _shap_one_fractions(Xn, paths, e0, e1)
            dead = ((o == 0.0) & (z[:, None] == 0.0)).any(axis=0)
            w = _shap_extend(z, o)
            v = paths["value"][p]
            dest = outn[:, int(paths["group"][p]), :]
            for i in range(m):
                s = _shap_unwound_sum(w, m, z[i], o[i])
                dest[:, int(paths["feature"][e0 + i])] += np.where(
                    dead, 0.0, s * (o[i] - z[i]) * v)
    return out


def tree_shap_interactions(X, paths, out, max_out_bytes=None):
    """Raw off-diagonal SHAP interaction terms in path form (contract:
    ``ops.tree_shap_interactions``). For a path with elements E and leaf
    value v, every c in E and j in E \\ {c} adds
    (one_c - zero_c) / 2 * unwound_sum(E \\ {c}, j) * (one_j - zero_j) * v
    to out[:, feature_c, feature_j] - what ``_tree_shap`` yields as
    (condition=+1 pass - condition=-1 pass) / 2."""
    import numpy as np

    Xn, outn = _as_numpy(X), _as_numpy(out)
    _shap_check(Xn, paths, 1)
    ptr, zf = paths["path_ptr"], paths["zero_fraction"]
    with np.errstate(divide="ignore", invalid="ignore"):
        for p in range(len(ptr) - 1):
            e0, e1 = int(ptr[p]), int(ptr[p + 1])
            m = e1 - e0
            if m < 2:
                continue
            z = zf[e0:e1]
            o = _shap_one_fractions(Xn, paths, e0, e1)
            dead = ((o == 0.0) & (z[:, None] == 0.0)).any(axis=0)
            w = _shap_extend(z, o)
            v = paths["value"][p]
            feat = paths["feature"][e0:e1]
            for c in range(m):
                w2 = _shap_unwind(w, m, z[c], o[c])
                half = (o[c] - z[c]) / 2.0
                for j in range(m):
                    if j == c:
                        continue
                    s = _shap_unwound_sum(w2, m - 1, z[j], o[j])
                    outn[:, int(feat[c]), int(feat[j])] += np.where(
                        dead, 0.0, half * s * (o[j] - z[j]) * v)
    return out


# ---------------------------------------------------------------------------
# Ranking: per-group stable descending ranks, DCG / AP sums and the rank:map
# lambdas (contract: docs/parity.md "Ranking on the device"). Plain numpy,
# one group at a time - the twins of the HIP kernels, not a fast path.
# ---------------------------------------------------------------------------
# longest query group the HIP kernels sort in LDS
RANK_LDS_MAX_GROUP = 2048


def rank_disc_table(length=RANK_LDS_MAX_GROUP):
    """float64 [length] DCG discounts, disc[r] = 1 / log2(r + 2)."""
    import numpy as np

    return 1.0 / np.log2(np.arange(length, dtype=np.float64) + 2.0)


def _rank_order(m):
    """Stable descending order of float32 margins; -0.0 ties with +0.0."""
    import numpy as np

    return np.argsort(-m.astype(np.float64), kind="stable")


def rank_group_stats(margin, label, group_ptr, disc, k, max_len=None):
    import numpy as np

    m = np.asarray(_as_numpy(margin), np.float32)
    y = np.asarray(_as_numpy(label), np.float32)
    gp = np.asarray(_as_numpy(group_ptr), np.int64)
    disc = np.asarray(_as_numpy(disc), np.float64)
    G = len(gp) - 1
    rank = np.zeros(len(m), np.int32)
    stats = np.zeros((G, 4), np.float64)
    for g in range(G):
        s, e = int(gp[g]), int(gp[g + 1])
        L = e - s
        if L == 0:
            continue
        kk = L if k <= 0 or k > L else int(k)
        order = _rank_order(m[s:e])
        rank[s + order] = np.arange(L, dtype=np.int32)
        gain = np.exp2(y[s:e].astype(np.float64)) - 1.0
        d = disc[:L]
        ideal = np.sort(gain)[::-1] * d
        rel = (y[s:e][order] > 0).astype(np.float64)
        R = rel.sum()
        ap = (np.cumsum(rel) / np.arange(1, L + 1) * rel).sum()
        stats[g] = ((gain[order] * d)[:kk].sum(), ideal[:kk].sum(),
                    ideal.sum(), ap / R if R > 0 else 0.0)
    return torch.from_numpy(rank), torch.from_numpy(stats)


def lambdamap_grad(margin, label, group_ptr, max_len=None):
    import numpy as np

    m32 = np.asarray(_as_numpy(margin), np.float32)
    y32 = np.asarray(_as_numpy(label), np.float32)
    gp = np.asarray(_as_numpy(group_ptr), np.int64)
    out = np.zeros((len(m32), 2), np.float64)
    for g in range(len(gp) - 1):
        s, e = int(gp[g]), int(gp[g + 1])
        L = e - s
        m, y = m32[s:e], y32[s:e]
        win = y[:, None] > y[None, :]
        order = _rank_order(m)
        rel = (y[order] > 0).astype(np.float64)
        R = rel.sum()
        if L < 2 or R == 0 or not win.any():
            continue
        rank = np.empty(L, np.int64)
        rank[order] = np.arange(L)
        pos = np.arange(1, L + 1, dtype=np.float64)
        t = np.cumsum(rel) / pos
        S = np.cumsum(rel / pos)
        lo = np.minimum(rank[:, None], rank[None, :])
        hi = np.maximum(rank[:, None], rank[None, :])
        delta = np.abs(t[hi] - t[lo] - (S[np.maximum(hi - 1, 0)] - S[lo])) / R
        with np.errstate(over="ignore"):
            rho = 1.0 / (1.0 + np.exp((m[:, None] - m[None, :]).astype(
                np.float64)))
        lam = np.where(win, rho * delta, 0.0)
        hess = np.where(win, np.maximum(rho * (1.0 - rho), 1e-16) * delta, 0.0)
        out[s:e, 0] = -lam.sum(1) + lam.sum(0)
        out[s:e, 1] = hess.sum(1) + hess.sum(0)
    return torch.from_numpy(out.astype(np.float32))


def lambdarank_topk_grad(margin, label, group_ptr, disc, k, ndcg,
                         max_len=None):
    """float64 numpy form of ``ops.lambdarank_topk_grad``: all pairs of a
    group as [L, L] matrices, masked by min(rank_i, rank_j) < k."""
    import numpy as np

    m32 = np.asarray(_as_numpy(margin), np.float32)
    y32 = np.asarray(_as_numpy(label), np.float32)
    gp = np.asarray(_as_numpy(group_ptr), np.int64)
    disc = np.asarray(_as_numpy(disc), np.float64)
    k = int(k)
    if k < 1:
        raise ValueError(f"lambdarank_topk_grad: k must be >= 1, got {k}")
    out = np.zeros((len(m32), 2), np.float64)
    for g in range(len(gp) - 1):
        s, e = int(gp[g]), int(gp[g + 1])
        L = e - s
        if L < 2:
            continue
        m, y = m32[s:e], y32[s:e]
        rank = np.empty(L, np.int64)
        rank[_rank_order(m)] = np.arange(L)
        win = (y[:, None] > y[None, :]) & (
            np.minimum(rank[:, None], rank[None, :]) < k)
        with np.errstate(over="ignore"):
            rho = 1.0 / (1.0 + np.exp((m[:, None] - m[None, :]).astype(
                np.float64)))
        hess = np.maximum(rho * (1.0 - rho), 1e-16)
        if ndcg:
            gain = np.exp2(y.astype(np.float64)) - 1.0
            idcg = (np.sort(gain)[::-1] * disc[:L]).sum()
            if not idcg > 0.0:
                continue
            d = disc[rank]
            w = np.abs((gain[:, None] - gain[None, :])
                       * (d[:, None] - d[None, :])) / idcg
            rho, hess = rho * w, hess * w
        lam = np.where(win, rho, 0.0)
        hess = np.where(win, hess, 0.0)
        out[s:e, 0] = -lam.sum(1) + lam.sum(0)
        out[s:e, 1] = hess.sum(1) + hess.sum(0)
    return torch.from_numpy(out.astype(np.float32))


# ---------------------------------------------------------------------------
# Multiclass: the softmax gradient and the mlogloss / merror sums (contract:
# docs/parity.md "Multiclass on the device"). Plain numpy float64 - the twins
# of the HIP kernels and their oracle, not the CPU training path.
# ---------------------------------------------------------------------------
# classes per LDS chunk of the HIP kernels (K <= KC: one chunk per row tile)
SOFTMAX_CHUNK_CLASSES = 16


def _softmax_rows(margin, label):
    """(d = x - max, e = exp(d), s = ascending sum of e, label class or -1)
    of every row, float64 from the float32 inputs."""
    import numpy as np

    x = np.asarray(_as_numpy(margin), np.float32)
    if x.ndim != 2 or x.shape[1] < 2:
        raise ValueError("multiclass ops need a margin [n, K] with K >= 2")
    y = np.asarray(_as_numpy(label), np.float32)
    K = x.shape[1]
    with np.errstate(invalid="ignore"):
        d = x.astype(np.float64) - x.max(axis=1, keepdims=True).astype(
            np.float64)
        e = np.exp(d)
        # truncated toward zero as .long() does; outside [0, K): no class
        yi = np.where((y > -1) & (y < K), np.trunc(y), -1).astype(np.int64)
    s = np.zeros(len(x), np.float64)
    for k in range(K):  # ascending class order, not numpy's pairwise sum
        s = s + e[:, k]
    return d, e, s, yi


def softmax_grad(margin, label, weight=None):
    import numpy as np

    d, e, s, yi = _softmax_rows(margin, label)
    n, K = e.shape
    with np.errstate(invalid="ignore"):
        p = e / s[:, None]
        hit = yi[:, None] == np.arange(K)[None, :]
        g = (p - hit).astype(np.float32)
        h = np.maximum(2.0 * p * (1.0 - p), 1e-16).astype(np.float32)
        if weight is not None:
            w = np.asarray(_as_numpy(weight), np.float32)[:, None]
            g, h = g * w, h * w  # float32: the second rounding
    store = np.stack([g.T, h.T], axis=-1)  # class-major [K, n, 2]
    absmax = (np.abs(store).max(axis=1) if n
              else np.zeros((K, 2), np.float32))
    return (torch.from_numpy(np.ascontiguousarray(store)).permute(1, 0, 2),
            torch.from_numpy(absmax.astype(np.float32)))


def eval_multiclass(margin, label, weight=None):
    import numpy as np

    d, e, s, yi = _softmax_rows(margin, label)
    n = len(s)
    w = (np.ones(n, np.float64) if weight is None
         else np.asarray(_as_numpy(weight), np.float32).astype(np.float64))
    rows = np.arange(n)
    with np.errstate(invalid="ignore", divide="ignore"):
        nll = np.where(yi >= 0, np.log(s) - d[rows, np.maximum(yi, 0)],
                       np.nan)
    # the lowest index attaining the maximum is where d first reaches 0
    wrong = (np.argmax(d == 0.0, axis=1) != yi).astype(np.float64)
    return torch.from_numpy(
        np.array([(w * nll).sum(), (w * wrong).sum(), w.sum()], np.float64))


AUC_MAX_BINS = 16384     # a bin is 14 bits of the HIP kernels' u16 code
AUC_WEIGHT_SCALE = 2.0 ** 20


def auc_multiclass_check(n, weight, n_bins):
    """What ``eval_auc_multiclass`` refuses, on either backend, before any
    work: a bin count outside [1, AUC_MAX_BINS], and weights whose integer
    mass n * 2^20 * max |w| could reach 2^53 (NaN weights included)."""
    if not 1 <= int(n_bins) <= AUC_MAX_BINS:
        raise ValueError(
            f"eval_auc_multiclass: n_bins must lie in [1, {AUC_MAX_BINS}], "
            f"got {n_bins}")
    if weight is not None and n:
        bound = float(n) * AUC_WEIGHT_SCALE * float(weight.abs().max())
        if not bound < 2.0 ** 53:
            raise ValueError(
                "eval_auc_multiclass: n * 2^20 * max(weight) must stay below "
                f"2^53, got {bound:g}")


def eval_auc_multiclass(margin, label, weight=None, n_bins=16384):
    """int64 [K, 2, n_bins] one-vs-rest score histograms, planes [neg | pos]
    (contract: ``ops.eval_auc_multiclass``). Plain numpy float64, the oracle
    of the HIP kernels; the integers match theirs."""
    import numpy as np

    n_bins = int(n_bins)
    wt = None if weight is None else torch.as_tensor(_as_numpy(weight))
    auc_multiclass_check(len(label), wt, n_bins)
    d, e, s, yi = _softmax_rows(margin, label)
    n, K = e.shape
    with np.errstate(invalid="ignore"):
        t = (e / s[:, None]) * float(n_bins)
        # NaN fails the comparison: bin 0
        b = np.where(t >= 1.0, np.minimum(np.trunc(t), n_bins - 1),
                     0).astype(np.int64)
    if weight is None:
        W = np.ones(n, np.float64)
    else:
        w = np.asarray(_as_numpy(weight), np.float32).astype(np.float64)
        W = np.rint(w * AUC_WEIGHT_SCALE)  # integers: sums below 2^53 exact
    hist = np.zeros((K, 2, n_bins), np.int64)
    for k in range(K):
        pos = yi == k
        for plane, rows in ((0, ~pos), (1, pos)):
            hist[k, plane] = np.bincount(
                b[rows, k], weights=W[rows], minlength=n_bins
            ).astype(np.int64)
    return torch.from_numpy(hist)


# --- survival (contract: docs/parity.md "Survival on the device") ----------
# Float64 torch forms written from the formulae, not from the objective
# classes; tests/test_survival_ops_cpu.py pins them to those classes.

COX_TILE_ROWS = 2048  # sorted positions per workgroup of the GPU Cox kernels
AFT_DISTS = ("normal", "logistic", "extreme")


def _aft_terms(dist, z):
    """(f, dlogf, S, F) of the clamped z: density, d log f / dz, survival in
    its no-cancellation form, and the cdf as the metric takes it."""
    if dist == "logistic":
        s = 1.0 / (1.0 + torch.exp(-z))
        return s * (1.0 - s), 1.0 - 2.0 * s, 1.0 / (1.0 + torch.exp(z)), s
    if dist == "extreme":
        ez = torch.exp(torch.clamp(z, max=15.0))
        S = torch.exp(-ez)
        return ez * S, 1.0 - ez, S, 1.0 - S
    if dist != "normal":
        raise ValueError(f"unknown AFT distribution {dist!r}")
    r = 0.7071067811865476  # 1 / sqrt(2)
    f = torch.exp(-0.5 * z * z) / 2.5066282746310002  # sqrt(2 pi)
    return (f, -z, 0.5 * torch.special.erfc(z * r),
            0.5 * torch.special.erfc(-z * r))


def _aft_rows(margin, label, sigma):
    yl, yu = label[:, 0].float(), label[:, 1].float()
    m = margin.float().double()
    lo = torch.log(torch.clamp(yl.double(), min=1e-16))
    hi = torch.log(torch.clamp(yu.double(), min=1e-16))
    zl = torch.clamp((lo - m) / sigma, min=-15.0, max=15.0)
    zu = torch.clamp((hi - m) / sigma, min=-15.0, max=15.0)
    unc = yl == yu
    right = torch.isinf(yu) & ~unc
    left = (yl <= 0) & ~unc & ~right
    return lo, zl, zu, unc, right, left


def _weighted_pair(g, h, weight):
    g, h = g.float(), h.float()
    if weight is not None:
        g, h = g * weight.float(), h * weight.float()  # second rounding
    gp = torch.stack([g, h], dim=-1)
    absmax = (gp.abs().amax(0) if len(gp)
              else torch.zeros(2, dtype=torch.float32))
    return gp, absmax


def aft_grad(margin, label, weight, dist, sigma):
    sig = float(sigma)
    s2 = sig * sig
    lo, zl, zu, unc, right, left = _aft_rows(margin, label, sig)
    fl, dl, Sl, _ = _aft_terms(dist, zl)
    fu, du, Su, Fu = _aft_terms(dist, zu)
    # uncensored
    g = dl / sig
    if dist == "logistic":
        s = 1.0 / (1.0 + torch.exp(-zl))
        h = 2.0 * s * (1.0 - s) / s2
    elif dist == "extreme":
        h = torch.exp(torch.clamp(zl, max=15.0)) / s2
    else:
        h = torch.full_like(zl, 1.0 / s2)
    # right-censored: hazard f / S at zl
    if dist == "logistic":
        hz = 1.0 / (1.0 + torch.exp(-zl))
        dhz = hz * (1.0 - hz)
    elif dist == "extreme":
        hz = torch.exp(torch.clamp(zl, max=15.0))
        dhz = hz
    else:
        hz = fl / torch.clamp(Sl, min=1e-300)
        dhz = hz * (hz - zl)
    g = torch.where(right, -hz / sig, g)
    h = torch.where(right, dhz / s2, h)
    # left-censored: reversed hazard f / F at zu
    if dist == "logistic":
        rh = Su
        drh = -rh * (1.0 - rh)
    elif dist == "extreme":
        rh = fu / torch.clamp(1.0 - Su, min=1e-300)
        drh = rh * (du - rh)
    else:
        rh = fu / torch.clamp(Fu, min=1e-300)
        drh = rh * (-zu - rh)
    g = torch.where(left, rh / sig, g)
    h = torch.where(left, -drh / s2, h)
    # interval
    D = torch.clamp(Sl - Su, min=1e-300)
    df = fu - fl
    interval = ~(unc | right | left)
    g = torch.where(interval, df / (sig * D), g)
    h = torch.where(interval,
                    (df * df / (D * D) - (fu * du - fl * dl) / D) / s2, h)
    return _weighted_pair(g, torch.clamp(h, min=1e-6), weight)


def aft_nll_rows(margin, label, dist, sigma):
    """Per-row aft-nloglik term, float64."""
    import math

    sig = float(sigma)
    lo, zl, zu, unc, right, left = _aft_rows(margin, label, sig)
    fl, _, _, Fl = _aft_terms(dist, zl)
    Fu = _aft_terms(dist, zu)[3]
    D = torch.where(right, 1.0 - Fl, torch.where(left, Fu, Fu - Fl))
    return torch.where(
        unc, -torch.log(torch.clamp(fl, min=1e-12)) + math.log(sig) + lo,
        -torch.log(torch.clamp(D, min=1e-12)))


def eval_aft(margin, label, weight, dist, sigma):
    nll = aft_nll_rows(margin, label, dist, sigma)
    w = (torch.ones_like(nll) if weight is None
         else weight.float().double())
    return torch.stack([(w * nll).sum(), w.sum()])


def cox_layout(label):
    """What survival:cox needs of the labels alone, on label's device: the
    stable descending-time order (int32), for every sorted position the
    first and last position of its tie block (int32), and the event flag in
    sorted order (uint8)."""
    from collections import namedtuple

    lay = namedtuple("CoxLayout", "order first last event")
    n = label.numel()
    dev = label.device
    if n == 0:
        e = torch.zeros(0, dtype=torch.int32, device=dev)
        return lay(e, e, e, e.to(torch.uint8))
    if n > 2 ** 31 - 1:
        raise ValueError("survival:cox layout holds at most 2^31 - 1 rows")
    lab = label.float()
    order = torch.argsort(-lab.abs(), stable=True)
    t_s = lab.abs()[order]
    pos = torch.arange(n, dtype=torch.int32, device=dev)
    # The blocks are those of ``Cox.gradients`` as it stands, so that the
    # GPU route computes what the torch route does: its block id is the
    # inclusive count of positions whose successor has another time, which
    # opens a block AT the last row of a run of equal times, not after it.
    # With distinct times every row is its own block either way.
    change = torch.ones(n, dtype=torch.bool, device=dev)
    change[:-1] = t_s[:-1] != t_s[1:]
    start = change.clone()
    start[0] = True
    end = torch.ones(n, dtype=torch.bool, device=dev)
    end[:-1] = start[1:]
    first = torch.cummax(torch.where(start, pos, 0), 0).values
    last = torch.cummin(
        torch.where(end, pos, n - 1).flip(0), 0).values.flip(0)
    return lay(order.to(torch.int32).contiguous(),
               first.to(torch.int32).contiguous(),
               last.to(torch.int32).contiguous(),
               (lab > 0)[order].to(torch.uint8).contiguous())


def cox_terms(margin, layout):
    """Float64 (m - shift, eta, C, A, B, ev) in sorted order: the pieces of
    the Cox contract, shared by the forms below and by the tests' bounds."""
    m32 = margin.float()
    m = m32.double() - m32.max().double()
    o = layout.order.long()
    m_s = m[o]
    eta = torch.exp(m_s)
    ev = layout.event.double()
    C = torch.cumsum(eta, 0)
    R = torch.clamp(C[layout.last.long()], min=1e-300)
    first = layout.first.long()
    A = torch.flip(torch.cumsum(torch.flip(ev / R, [0]), 0), [0])[first]
    B = torch.flip(torch.cumsum(torch.flip(ev / (R * R), [0]), 0), [0])[first]
    return m_s, eta, C, A, B, ev


def cox_grad(margin, layout, weight=None):
    if margin.numel() == 0:
        return torch.zeros(0, 2), torch.zeros(2)
    _, eta, _, A, B, ev = cox_terms(margin, layout)
    o = layout.order.long()
    g = torch.empty_like(eta)
    h = torch.empty_like(eta)
    g[o] = -ev + eta * A
    h[o] = torch.clamp(eta * A - eta * eta * B, min=1e-6)
    return _weighted_pair(g, h, weight)


def eval_cox(margin, layout):
    if margin.numel() == 0:
        return torch.zeros(2, dtype=torch.float64)
    m_s, _, C, _, _, ev = cox_terms(margin, layout)
    e = ev > 0
    ll = (m_s[e] - torch.log(torch.clamp(C[e], min=1e-300))).sum()
    return torch.stack([-ll, ev.sum()])


# --- pointwise regression (contract: docs/parity.md "Regression on the
# device") -------------------------------------------------------------------
# numpy float64 forms written from the formulae, not from the objective and
# metric classes; tests/test_pointwise_ops_cpu.py pins them to those classes.

POINTWISE_GRAD_KINDS = ("absoluteerror", "poisson", "gamma", "tweedie",
                        "squaredlogerror", "pseudohuber", "hinge")
POINTWISE_EVAL_KINDS = ("se", "ae", "ape", "sle", "mphe", "poisson", "gamma",
                        "tweedie", "pinball")
POINTWISE_TRANSFORMS = ("identity", "exp", "sigmoid")
QUANTILE_MAX_TARGETS = 16  # targets the GPU quantile kernels serve


def _f64(a):
    import numpy as np

    return np.asarray(_as_numpy(a), np.float32).astype(np.float64)


def pointwise_terms(margin, label, kind, param=0.0):
    """Float64 (g, h, scale_g, scale_h) of every row, unweighted. scale is
    the largest addend that a float32 chain rounds on its way to the value
    (for squaredlogerror at least 1: rounding m + 1 moves the log by an
    absolute 2^-24); the tests' bounds are built from it."""
    import numpy as np

    m, y = _f64(margin), _f64(label)
    one = np.ones_like(m)
    with np.errstate(all="ignore"):
        if kind == "absoluteerror":
            g, h = np.sign(m - y), one
            g = np.where(np.isnan(g), 0.0, g)  # torch.sign(NaN) is 0
            sg, sh = one, one
        elif kind == "poisson":
            mu = np.exp(m)
            g, h = mu - y, mu
            sg, sh = np.maximum(mu, np.abs(y)), mu
        elif kind == "gamma":
            ratio = y * np.exp(-m)
            g, h = 1.0 - ratio, ratio
            sg, sh = np.maximum(1.0, np.abs(ratio)), np.abs(ratio)
        elif kind == "tweedie":
            rho = float(param)
            a, b = np.exp((1.0 - rho) * m), np.exp((2.0 - rho) * m)
            g = -y * a + b
            h = -y * (1.0 - rho) * a + (2.0 - rho) * b
            sg = np.maximum(np.abs(y * a), b)
            sh = np.maximum(np.abs(y * (1.0 - rho) * a),
                            np.abs((2.0 - rho) * b))
        elif kind == "squaredlogerror":
            p = np.maximum(m + 1.0, 1e-6)
            lp, ly = np.log(p), np.log(np.maximum(y + 1.0, 1e-6))
            d = lp - ly
            g = d / p
            h = np.maximum((1.0 - d) / (p * p), 1e-6)
            sd = np.maximum(1.0, np.maximum(np.abs(lp), np.abs(ly)))
            sg, sh = sd / p, sd / (p * p)
        elif kind == "pseudohuber":
            r = m - y
            z = 1.0 + (r / float(param)) ** 2
            sq = np.sqrt(z)
            g, h = r / sq, np.maximum(1.0 / (z * sq), 1e-16)
            sg, sh = np.abs(g), np.abs(h)
        elif kind == "hinge":
            t = 2.0 * y - 1.0
            active = m * t < 1.0
            g = np.where(active, -t, 0.0)
            h = np.where(active, 1.0, 1e-16)
            sg, sh = one, one
        else:
            raise ValueError(f"unknown pointwise gradient kind {kind!r}")
    return g, h, sg, sh


def _pair_f64(g, h, weight):
    """(gpair f64 [..., 2], absmax f64 over the rows); NaN kept."""
    import numpy as np

    if weight is not None:
        w = _f64(weight).reshape((-1,) + (1,) * (g.ndim - 1))
        g, h = g * w, h * w
    gp = np.stack([g, h], axis=-1)
    absmax = np.abs(gp).max(axis=0) if len(gp) else np.zeros(gp.shape[1:])
    return torch.from_numpy(gp), torch.from_numpy(absmax)


def pointwise_grad(margin, label, weight, kind, param=0.0):
    g, h, _, _ = pointwise_terms(margin, label, kind, param)
    return _pair_f64(g, h, weight)


def quantile_grad(margin, label, weight, alphas):
    """g = 1 - a_k where m - y >= 0, else -a_k, with a_k rounded to float32
    first; h = 1. margin [n] gives [n, 2], margin [n, K] gives [n, K, 2]."""
    import numpy as np

    m, y = _f64(margin), _f64(label)
    a = np.asarray(list(alphas), np.float32).astype(np.float64)
    if m.ndim == 1:
        a = a[0]
    else:
        y = y[:, None]
    with np.errstate(invalid="ignore"):
        g = np.where(m - y >= 0, 1.0 - a, -a)  # false, so -a, for NaN
    return _pair_f64(g, np.ones_like(m), weight)


def pointwise_loss_rows(margin, label, kind, transform="identity", param=0.0):
    """Per-row loss of a metric kind, float64 from the float32 inputs; for
    pinball the mean over the row's targets (param is the alpha list)."""
    import numpy as np

    m, y = _f64(margin), _f64(label)
    with np.errstate(all="ignore"):
        if kind == "pinball":
            a = np.asarray(list(param), np.float64)
            d = y[:, None] - m.reshape(len(m), -1)
            return np.where(d >= 0, a * d, (a - 1.0) * d).sum(axis=1) / len(a)
        if transform == "exp":
            pred = np.exp(m)
        elif transform == "sigmoid":
            pred = 1.0 / (1.0 + np.exp(-m))
        elif transform == "identity":
            pred = m
        else:
            raise ValueError(f"unknown transform {transform!r}")
        if kind == "se":
            return (pred - y) ** 2
        if kind == "ae":
            return np.abs(pred - y)
        if kind == "ape":
            return np.abs(pred - y) / np.maximum(np.abs(y), 1e-10)
        if kind == "sle":
            d = np.log1p(np.maximum(pred, -1.0 + 1e-6)) - np.log1p(y)
            return d * d
        if kind == "mphe":  # the metric subtracts in float32
            r = (np.asarray(_as_numpy(margin), np.float32)
                 - np.asarray(_as_numpy(label), np.float32)).astype(np.float64)
            return np.sqrt(1.0 + r * r) - 1.0
        mu = np.maximum(np.exp(m), 1e-16)
        if kind == "poisson":
            return mu - y * np.log(mu) + torch.lgamma(
                torch.from_numpy(y + 1.0)).numpy()
        if kind == "gamma":
            return y / mu + np.log(mu)
        if kind == "tweedie":
            rho = float(param)
            return (-y * np.exp((1.0 - rho) * m) / (1.0 - rho)
                    + np.exp((2.0 - rho) * m) / (2.0 - rho))
    raise ValueError(f"unknown pointwise metric kind {kind!r}")


def eval_pointwise(margin, label, weight, kind, transform="identity",
                   param=0.0):
    """f64 [2] = [sum w * loss, sum w], both by ``math.fsum``."""
    import math

    import numpy as np

    loss = pointwise_loss_rows(margin, label, kind, transform, param)
    w = np.ones_like(loss) if weight is None else _f64(weight)
    return torch.tensor([math.fsum(w * loss), math.fsum(w)],
                        dtype=torch.float64)
