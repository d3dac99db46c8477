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
