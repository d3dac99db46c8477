"""Per-op steady-state microbenchmark on the HIGGS shape (GPU).

Times each engine op in isolation (20 reps, synced) to separate kernel
time from host-side overhead. Run on an MI355X box.
"""

import os as _os
import sys as _sys

_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))


import time

import numpy as np
import torch

from xgboost_ray_amd.engine.quantile import BinnedMatrix
from xgboost_ray_amd import ops


def timeit(name, fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps * 1000
    print(f"{name:24s} {dt:9.3f} ms", flush=True)
    return dt


def bench_leaf_quantile(n=11_000_000, K=256, F=28, n_round=2_000_000):
    """leaf_quantile_hist: the four radix-select passes over K leaf
    segments (both LDS schemes, unit and int64 weights), against
    update_margins over the same segments - both make one pass over ridx
    with a gathered 4-byte access - and a reg:quantileerror round against
    a reg:squarederror round of the same shape."""
    from xgboost_ray_amd.engine.trainer import BoostingEngine

    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    resid = torch.randn(n, device=dev, generator=gen)
    W = torch.randint(0, 2**30 + 1, (n,), device=dev, generator=gen)
    ridx = torch.randperm(n, device=dev).to(torch.int32)
    cut = torch.sort(
        torch.randint(1, n - 1, (K - 1,), generator=gen, device=dev)
    )[0].cpu()
    starts = torch.cat([torch.tensor([0]), cut]).long()
    counts = torch.cat([cut, torch.tensor([n])]).long() - starts
    lv = np.random.RandomState(0).randn(K).astype(np.float32)
    m = torch.zeros(n, device=dev)
    t_um = timeit("update_margins K=%d" % K,
                  lambda: ops.update_margins(m, ridx, starts, counts, lv))
    # prefixes of the real select (median of every leaf)
    q, _ = ops.leaf_quantile_select(resid, None, ridx, starts, counts, 0.5)
    key = q.view(np.uint32).astype(np.int64)
    key = np.where(key & 0x80000000, key ^ 0xFFFFFFFF, key | 0x80000000)
    hist = torch.zeros((K, 256), dtype=torch.int64, device=dev)
    for wname, wt, nbytes in (("unit", None, 8), ("int64 W", W, 16)):
        total = 0.0
        for p in range(4):
            prefix = torch.from_numpy(
                (key >> (32 - 8 * p)) if p else np.zeros(K, np.int64))
            dt = timeit(
                f"lqh {wname} pass{p}",
                lambda: ops.leaf_quantile_hist(
                    resid, wt, ridx, starts, counts, prefix, p, hist),
            )
            # pass 0 touches ridx + resid (+ W) of every row; later
            # passes skip W for the rows that fail the prefix test
            if p == 0:
                print(f"    achieved {n * nbytes / dt / 1e6:8.1f} GB/s "
                      f"({nbytes} B/row)")
            total += dt
        print(f"  lqh {wname}: 4 passes {total:.3f} ms = "
              f"{total / t_um:.2f} x update_margins")

    X = torch.randn(n_round, F, device=dev, generator=gen)
    y = X[:, 0] * 2 - X[:, 1] + torch.randn(n_round, device=dev, generator=gen)
    dm = BinnedMatrix.build(X, label=y, max_bin=256)
    per_round = {}
    for obj, extra in (("reg:squarederror", {}),
                       ("reg:quantileerror", {"quantile_alpha": 0.9})):
        eng = BoostingEngine(
            dict({"objective": obj, "max_depth": 8, "eta": 0.3,
                  "tree_method": "gpu_hist"}, **extra), dm)
        per_round[obj] = timeit(f"round {obj}", eng.update, reps=10)
    print("quantile round / squarederror round: %.2f" % (
        per_round["reg:quantileerror"] / per_round["reg:squarederror"]))


def bench_mvs(n=11_000_000, F=28, subsample=0.2, rounds=20, depth=8):
    """Gradient-based sampling: each kernel at n rows with its achieved
    GB/s over the compulsory bytes, the whole sampler against the
    host-side uniform one, and a depth-``depth`` binary:logistic round on
    n x F with no sampling / uniform / gradient_based (training logloss
    after ``rounds`` rounds next to each)."""
    from xgboost_ray_amd.engine.trainer import BoostingEngine
    from xgboost_ray_amd.ops import gpu as gpu_ops

    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)

    def rate(name, fn, nbytes, reps=20):
        dt = timeit(name, fn, reps=reps)
        print(f"    achieved {n * nbytes / dt / 1e6:8.1f} GB/s "
              f"({nbytes} B/row)")
        return dt

    k = max(1, int(subsample * n))
    y = (torch.rand(n, device=dev, generator=gen) < 0.4).float()
    p = torch.sigmoid(2.0 * torch.randn(n, device=dev, generator=gen))
    # logistic pairs take the closed form (t* > max c); squared-error
    # pairs with Cauchy-tailed residuals force the four select passes
    r = torch.tan(3.14159 * (torch.rand(n, device=dev, generator=gen) - 0.5))
    shapes = (
        ("logistic", torch.stack([p - y, p * (1 - p)], 1).contiguous()),
        ("cauchy", torch.stack([r, torch.ones_like(r)], 1).contiguous()),
    )
    del p, r
    for name, gp in shapes:
        print(f"-- mvs kernels, {name} pairs, n={n}, k={k}")
        mx = (float(gp[:, 0].abs().max()), float(gp[:, 1].abs().max()))
        c = ops.mvs_score(gp, *mx)
        rate("mvs_score", lambda: ops.mvs_score(gp, *mx), 12)
        rate("mvs_stats", lambda: gpu_ops.mvs_stats(c), 4)
        S, M = ops.mvs_threshold(c, k)
        closed = S == int(gpu_ops.mvs_stats(c)[2]) and M == k
        print(f"    threshold: S={S} M={M} closed_form={closed}")
        # the select's own prefixes: the leading bytes of t* = S // M
        t = min(S // M, int(gpu_ops.mvs_stats(c)[1])) if M else 0
        total = 0.0
        for ps in range(4):
            prefix = (t >> (32 - 8 * ps)) if ps else 0
            total += rate(f"mvs_hist pass{ps}",
                          lambda: ops.mvs_hist(c, prefix, ps), 4)
        print(f"    4 passes {total:.3f} ms")
        timeit("mvs_threshold (pulls)", lambda: ops.mvs_threshold(c, k))
        rate("mvs_sample", lambda: ops.mvs_sample(gp, c, S, M, 12345), 21)
        keep, _ = ops.mvs_sample(gp, c, S, M, 12345)
        print(f"    sample size {int(keep.sum())} (k = {k})")
        timeit("nonzero -> int32 ridx",
               lambda: torch.nonzero(keep).flatten().to(torch.int32))

        def sampler():
            cc = ops.mvs_score(gp, *mx)
            s, m = ops.mvs_threshold(cc, k)
            kp, gw = ops.mvs_sample(gp, cc, s, m, 12345)
            return torch.nonzero(kp).flatten().to(torch.int32), gw

        timeit("whole gradient sampler", sampler)
        del c, keep

    def uniform_host():
        g = torch.Generator(device="cpu")
        g.manual_seed(7)
        mask = torch.rand(n, generator=g) < subsample
        return torch.nonzero(mask.to(dev)).flatten().to(torch.int32)

    timeit("host uniform sampler", uniform_host, reps=5)
    del shapes, gp

    X = torch.randn(n, F, device=dev, generator=gen)
    y = ((X[:, 0] + 0.5 * X[:, 1]
          + 0.5 * torch.randn(n, device=dev, generator=gen)) > 0).float()
    dm = BinnedMatrix.build(X, label=y, max_bin=256)
    del X
    print(f"-- rounds, {n} x {F}, depth {depth}, binary:logistic")
    for name, extra in (
            ("subsample=1", {}),
            (f"uniform {subsample}", {"subsample": subsample}),
            (f"gradient_based {subsample}",
             {"subsample": subsample, "sampling_method": "gradient_based"})):
        eng = BoostingEngine(
            dict({"objective": "binary:logistic", "max_depth": depth,
                  "eta": 0.3, "tree_method": "gpu_hist", "seed": 0},
                 **extra), dm)
        eng.update()
        eng.update()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(rounds - 2):
            eng.update()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / (rounds - 2) * 1000
        m = eng.margin.double()
        ll = float((torch.nn.functional.softplus(m) - y.double() * m).mean())
        print(f"round {name:22s} {dt:9.3f} ms   logloss after {rounds} "
              f"rounds {ll:.6f}   sample rows {eng.last_sample_rows}",
              flush=True)


def _trained_forest(n, F, rounds, depth):
    """n x F normal rows on the device and ``rounds`` trees of depth
    ``depth`` trained on them."""
    from xgboost_ray_amd.engine.trainer import BoostingEngine

    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn(n, F, device=dev, generator=gen)
    y = (X[:, 0] * X[:, 1] + X[:, 2:6].sum(1)
         + torch.randn(n, device=dev, generator=gen))
    eng = BoostingEngine(
        {"objective": "reg:squarederror", "max_depth": depth, "eta": 0.3,
         "tree_method": "gpu_hist"},
        BinnedMatrix.build(X, label=y, max_bin=256))
    for _ in range(rounds):
        eng.update()
    return X, eng.booster


def bench_tree_shap(n=1_000_000, F=28, rounds=100, depth=8,
                    n_inter=65_536, n_host=64):
    """Path-form TreeSHAP: contributions of n rows and interactions of
    n_inter rows through ``rounds`` trees of depth ``depth``, against
    predict_trees on the same input and against the host recursion
    (``booster._tree_shap``) on n_host of the rows."""
    dev = torch.device("cuda")
    X, bst = _trained_forest(n, F, rounds, depth)
    paths = ops.cpu.shap_paths(bst.trees, 1.0)
    lens = np.diff(paths["path_ptr"]).astype(np.int64)
    print(f"forest: {len(bst.trees)} trees, {len(lens)} paths, "
          f"{int(lens.sum())} elements, longest path {paths['max_len']}")
    # nominal float64 operations per row, a division counted as one:
    # EXTEND 8 per inner step (m(m+1)/2 steps), unwound_sum 7 per step on
    # a followed element (m steps for each of the m elements)
    print(f"inner steps per row: EXTEND {int((lens * (lens + 1) // 2).sum())}"
          f", unwound_sum {int((lens * lens).sum())}")
    flop_c = float((8 * lens * (lens + 1) // 2 + 7 * lens * lens).sum())
    flop_i = float((8 * lens * (lens + 1) // 2 + 7 * lens * lens
                    + 7 * lens * (lens - 1) * (lens - 1)).sum())

    flat = bst._flat_trees(dev)
    margin = torch.zeros(n, device=dev)
    t_pred = timeit("predict_trees", lambda: ops.predict_trees(
        X, flat["feat"], flat["thr"], flat["left"], flat["default_left"],
        flat["value"], flat["tree_ptr"], margin))

    out = torch.zeros((n, 1, F + 1), dtype=torch.float64, device=dev)
    t_c = timeit("tree_shap", lambda: ops.tree_shap(X, paths, 1, out),
                 reps=3)
    print(f"  contribs: {n / t_c / 1e3:8.3f} M rows/s, "
          f"{flop_c * n / t_c / 1e9:6.2f} TFLOP/s float64 nominal "
          f"({100 * flop_c * n / t_c / 1e9 / 78.6:.1f} % of the 78.6 TF "
          f"vector peak), {t_c / t_pred:.0f} x predict_trees")
    Xi = X[:n_inter].contiguous()
    out_i = torch.zeros((n_inter, F + 1, F + 1), dtype=torch.float64,
                        device=dev)
    t_i = timeit(f"interactions n={n_inter}",
                 lambda: ops.tree_shap_interactions(Xi, paths, out_i),
                 reps=3)
    print(f"  interactions: {n_inter / t_i / 1e3:8.3f} M rows/s, "
          f"{flop_i * n_inter / t_i / 1e9:6.2f} TFLOP/s float64 nominal, "
          f"{t_i / n_inter / (t_pred / n):.0f} x predict_trees per row")

    # the public route at the threshold batch, host copies included
    Xh = X[:16384].cpu().numpy()
    t0 = time.perf_counter()
    bst.predict(Xh, pred_contribs=True)
    t_route = time.perf_counter() - t0
    t0 = time.perf_counter()
    bst.predict(Xh[:n_host], pred_contribs=True)  # small batch: recursion
    t_host = time.perf_counter() - t0
    print(f"  Booster.predict(pred_contribs) 16384 rows on the device: "
          f"{t_route:.3f} s ({16384 / t_route:.0f} rows/s, paths built "
          f"in this call)")
    print(f"  host recursion, {n_host} rows: {t_host:.2f} s "
          f"({n_host / t_host:.1f} rows/s) -> 16384 rows would take "
          f"{t_host / n_host * 16384:.0f} s, "
          f"{t_host / n_host * 16384 / t_route:.0f} x the device route")


def _clock(fn, reps=3):
    """Median wall time of ``fn`` in seconds (host code, copies included)."""
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2]


def bench_walk(modes=("predict_leaf", "saabas"), n=1_000_000, F=28,
               rounds=100, depth=8, n_host=65_536, n_route=16_384):
    """``ops.predict_leaf`` and ``ops.saabas_contribs`` on the shape and
    model of ``bench_tree_shap`` (output kept on the device), against
    predict_trees on the same rows, against the numpy walks on the first
    n_host rows, and the public route at n_route rows with the device route
    on and off."""
    dev = torch.device("cuda")
    X, bst = _trained_forest(n, F, rounds, depth)
    walk = bst._flatten_for_walk(range(len(bst.trees)))
    T = len(bst.trees)
    forest = [walk[k] for k in ("feat", "thr", "left", "default_left")]
    print(f"forest: {T} trees, {len(walk['feat'])} nodes, largest tree "
          f"{int(np.diff(walk['tree_ptr'].numpy()).max())} nodes")
    flat = bst._flat_trees(dev)
    margin = torch.zeros(n, device=dev)
    t_pred = timeit("predict_trees", lambda: ops.predict_trees(
        X, flat["feat"], flat["thr"], flat["left"], flat["default_left"],
        flat["value"], flat["tree_ptr"], margin))
    Xh = X[:n_host].cpu().numpy()
    Xr = np.ascontiguousarray(Xh[:n_route])

    def route(**kw):
        """Public route at n_route rows, RXGB_WALK_GPU unset and 0."""
        _os.environ.pop("RXGB_WALK_GPU", None)
        bst.predict(Xr, **kw)  # builds the cached forest
        t_dev = _clock(lambda: bst.predict(Xr, **kw))
        _os.environ["RXGB_WALK_GPU"] = "0"
        t_np = _clock(lambda: bst.predict(Xr, **kw))
        t_np_host = _clock(lambda: bst.predict(Xh, **kw), reps=1)
        _os.environ.pop("RXGB_WALK_GPU", None)
        print(f"  Booster.predict {n_route} rows: device route "
              f"{t_dev * 1e3:.1f} ms, numpy route {t_np * 1e3:.1f} ms "
              f"({t_np / t_dev:.1f} x); numpy route on {n_host} rows "
              f"{t_np_host:.2f} s ({n_host / t_np_host / 1e3:.1f} k rows/s)")

    if "predict_leaf" in modes:
        row_bytes = 4 * F + 4 * T
        out = torch.zeros((n, T), dtype=torch.int32, device=dev)
        scratch = torch.zeros((T, n), dtype=torch.int32, device=dev)

        def direct():
            ops.predict_leaf(X, *forest, walk["tree_ptr"], out)

        def tree_major():
            # coalesced stores into a [T, n] buffer, then a transposing copy
            ops.predict_leaf(X, *forest, walk["tree_ptr"], scratch.t())
            out.copy_(scratch.t())

        for label, fn in (("predict_leaf [n,T] stores", direct),
                          ("predict_leaf [T,n]+transp", tree_major)):
            t = timeit(label, fn, reps=10)
            print(f"  {n / t / 1e3:8.1f} M rows/s, {row_bytes} B/row -> "
                  f"{n * row_bytes / t / 1e6:7.1f} GB/s, "
                  f"{t / t_pred:.2f} x predict_trees")
        route(pred_leaf=True)

    if "saabas" in modes:
        row_bytes = 4 * F + 2 * 8 * (F + 1)
        out = torch.zeros((n, F + 1), dtype=torch.float64, device=dev)

        def run(label, **kw):
            t = timeit(label, lambda: ops.saabas_contribs(
                X, *forest, walk["node_mean"], walk["tree_ptr"], out, **kw),
                reps=5)
            print(f"  {n / t / 1e3:8.1f} M rows/s, {row_bytes} B/row -> "
                  f"{n * row_bytes / t / 1e6:7.1f} GB/s, "
                  f"{t / t_pred:.2f} x predict_trees")
            return t

        t_def = run("saabas default")
        for threads in (64, 128, 256, 384, 512, 576, 640):
            for tile in (512, 1024, 2048, 4096):
                lds = 24 * tile + 8 * (F + 1) * threads
                if lds > ops.gpu.SAABAS_LDS_BYTES:
                    continue
                per_cu = min(ops.gpu.SAABAS_LDS_BYTES // lds,
                             2048 // threads)
                run(f"saabas {threads}thr tile{tile}", block_threads=threads,
                    tile_nodes=tile)
                print(f"    LDS {lds / 1024:.0f} KiB, {per_cu} workgroups = "
                      f"{per_cu * threads // 64} waves per CU")
        run("saabas global sums", lds_accumulators=False)
        run("saabas global 512thr 1024", lds_accumulators=False,
            block_threads=512, tile_nodes=1024)
        _os.environ["RXGB_PREDICT_LDS"] = "0"
        for threads in (256, 512, 1024):
            run(f"saabas plain {threads}thr", block_threads=threads)
        run("saabas plain global sums", lds_accumulators=False)
        _os.environ.pop("RXGB_PREDICT_LDS")
        paths = ops.cpu.shap_paths(bst.trees, 1.0)
        exact = torch.zeros((n, 1, F + 1), dtype=torch.float64, device=dev)
        t_exact = timeit("tree_shap (exact)", lambda: ops.tree_shap(
            X, paths, 1, exact), reps=1)
        print(f"  exact / approx on {n} rows: {t_exact / t_def:.0f} x")
        route(pred_contribs=True, approx_contribs=True)
        t_exact_r = _clock(lambda: bst.predict(Xr, pred_contribs=True))
        print(f"  Booster.predict(pred_contribs) exact, {n_route} rows: "
              f"{t_exact_r * 1e3:.1f} ms")


def _spread(fn, reps=5, inner=3):
    """(median, min, max) ms per call over ``reps`` synced windows of
    ``inner`` calls, after one warm-up window."""
    ts = []
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / inner * 1e3)
    ts = sorted(ts[1:])
    return ts[len(ts) // 2], ts[0], ts[-1]


def _spread_alt(fns, reps=5, inner=3):
    """``_spread`` of several routes whose windows alternate, so that a
    drift of the clocks falls on all of them alike."""
    ts = [[] for _ in fns]
    for r in range(reps + 1):
        for t, fn in zip(ts, fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) / inner * 1e3)
    ts = [sorted(t[1:]) for t in ts]
    return [(t[len(t) // 2], t[0], t[-1]) for t in ts]


def bench_rank(shapes=((10_000_000, 100), (1_000_000, 1000),
                       (6_400_000, 64)), sub_groups=2000):
    """The HIP ranking kernels against the torch routes they replace, in one
    process, alternating. The per-group torch loops (rank:map gradient, the
    metrics) run on the first ``sub_groups`` groups and are reported per
    group. The groups-of-64 shape is where both ``rank_group_stats``
    variants can run: it measures the boundary between them."""
    from xgboost_ray_amd.engine.metrics import get_metric
    from xgboost_ray_amd.engine.objectives import RankMAP, RankNDCG

    dev = torch.device("cuda")

    def show(name, t, groups=None):
        per = f"  {t[0] / groups * 1e3:9.3f} us/group" if groups else ""
        print(f"  {name:34s} {t[0]:10.3f} ms  [{t[1]:.3f}, {t[2]:.3f}]{per}",
              flush=True)
        return t[0]

    for n, glen in shapes:
        gen = torch.Generator(device=dev).manual_seed(11)
        margin = torch.randn(n, device=dev, generator=gen)
        label = torch.randint(0, 5, (n,), device=dev, generator=gen).float()
        qid = torch.arange(n, device=dev) // glen
        G = n // glen
        group_ptr = torch.arange(G + 1, device=dev) * glen
        disc = ops.rank_disc_table(dev)
        ndcg = RankNDCG()
        print(f"rank: {n} rows in {G} groups of {glen}")
        variants = [("auto", {})]
        if glen <= 64:
            variants.append(("workgroup/group", {"variant": 2}))
        for block in (64, 128, 256):
            variants.append((f"block {block}", {"block": block}))
        for name, kw in variants:
            show(f"rank_group_stats {name}", _spread(
                lambda: ops.rank_group_stats(margin, label, group_ptr, disc,
                                             0, max_len=glen, **kw)))
        show("torch preparation (parent)", _spread(
            lambda: ndcg._prep_torch(margin, label, qid)))
        rank, stats = ops.rank_group_stats(margin, label, group_ptr, disc, 0,
                                           max_len=glen)
        idcg = stats[:, 2].contiguous()
        show("lambdarank_grad (ndcg), for scale", _spread(
            lambda: ops.gpu.lambdarank_grad(margin, label, group_ptr, rank,
                                            idcg, True)))
        # top-k pair truncation against the all-pairs route it shortens,
        # windows alternating; k = glen is the all-pairs gradient on the
        # new kernel
        def all_ndcg():
            r, s = ops.rank_group_stats(margin, label, group_ptr, disc, 0,
                                        max_len=glen)
            return ops.gpu.lambdarank_grad(margin, label, group_ptr, r,
                                           s[:, 2].contiguous(), True)

        def topk(k, nd, **kw):
            return lambda: ops.lambdarank_topk_grad(
                margin, label, group_ptr, disc, k, nd, max_len=glen, **kw)

        rows = [("rank_group_stats + lambdarank_grad", all_ndcg),
                ("lambdarank_grad (pairwise)",
                 lambda: ops.gpu.lambdarank_grad(margin, label, group_ptr,
                                                 rank, idcg, False))]
        for k in (8, 32, glen):
            for nd in (True, False):
                tag = f"k={k} {'ndcg' if nd else 'pairwise'}"
                rows.append((f"lambdarank_topk_grad {tag}", topk(k, nd)))
                if glen <= 64:  # both variants can run: their boundary
                    rows.append((f"  workgroup/group {tag}",
                                 topk(k, nd, variant=2)))
                    rows.append((f"  wave/group {tag}",
                                 topk(k, nd, variant=1)))
                    assert torch.allclose(rows[-1][1](), rows[-2][1](),
                                          rtol=1e-6, atol=1e-12)
        for (name, _), t in zip(rows, _spread_alt([f for _, f in rows])):
            show(name, t)
        for block in (64, 128, 256):
            show(f"lambdarank_topk_grad k=32 ndcg block {block}", _spread(
                topk(32, True, block=block)))
        for block in (0, 64, 128, 256):
            show(f"lambdamap_grad block {block or 'auto'}", _spread(
                lambda: ops.lambdamap_grad(margin, label, group_ptr,
                                           max_len=glen, block=block)))
        # public routes, new against RXGB_RANK_GPU=0
        ns = sub_groups * glen
        full = (margin, label, None, qid)
        sub = (margin[:ns], label[:ns], None, qid[:ns].clone())
        for route in ("hip", "torch"):
            _os.environ["RXGB_RANK_GPU"] = "0" if route == "torch" else "1"
            loop = sub if route == "torch" else full  # per-group torch loops
            runs = [(RankNDCG(), "gradients", full),
                    (RankMAP(), "gradients", loop),
                    (get_metric("ndcg@10"), "local_stats", loop),
                    (get_metric("map"), "local_stats", loop)]
            for who, what, a in runs:
                fn = getattr(who, what)
                args = a if what == "gradients" else a + (None,)
                quick = a is full
                show(f"{who.name} {what} [{route}]", _spread(
                    lambda: fn(*args), reps=5 if quick else 1,
                    inner=3 if quick else 1), groups=len(a[0]) // glen)
                assert who.last_route == route
        _os.environ.pop("RXGB_RANK_GPU")


def bench_softmax(shapes=((11_000_000, 3), (11_000_000, 10),
                          (1_000_000, 100), (1_000_000, None)),
                  train_shape=(2_000_000, 28, 10)):
    """The HIP multiclass kernels against the torch routes they replace, in
    one process, windows alternating. The torch gradient line includes what
    the trainer does with its result: K ``.contiguous()`` class slices and
    2K ``abs().max()``. Rates are against the compulsory traffic, 4K + 4
    bytes in and 8K out per row for the gradient, 4K + 4 in for the metric.
    The last shape is one K above KC."""
    from xgboost_ray_amd.engine.metrics import get_metric
    from xgboost_ray_amd.engine.objectives import SoftProb
    from xgboost_ray_amd.engine.trainer import BoostingEngine, EvalPack

    dev = torch.device("cuda")
    KC = ops.SOFTMAX_CHUNK_CLASSES

    def show(name, t, nbytes=None):
        rate = f"  {nbytes / t[0] / 1e9:8.3f} TB/s" if nbytes else ""
        print(f"  {name:38s} {t[0]:9.3f} ms  [{t[1]:.3f}, {t[2]:.3f}]{rate}",
              flush=True)

    def switches(on):
        for name in ("RXGB_FUSED_GRAD", "RXGB_FUSED_EVAL"):
            if on:
                _os.environ.pop(name, None)
            else:
                _os.environ[name] = "0"

    for n, K in shapes:
        K = K or KC + 1
        gen = torch.Generator(device=dev).manual_seed(7)
        margin = torch.randn(n, K, device=dev, generator=gen) * 3
        label = torch.randint(0, K, (n,), device=dev, generator=gen).float()
        obj, metrics = SoftProb(K), [get_metric("mlogloss"),
                                     get_metric("merror")]
        print(f"softmax: {n} x {K} (KC = {KC})")

        def grad(on):
            def run():
                switches(on)
                gp = obj.gradients(margin, label)
                mx = getattr(gp, "_rxgb_absmax_cls", None)
                for c in range(K):  # the trainer's use of the result
                    sl = gp[:, c, :].contiguous()
                    if mx is None:
                        sl[:, 0].abs().max(), sl[:, 1].abs().max()
            return run

        def metric(on):
            def run():
                switches(on)
                for m in metrics:
                    m.local_stats(margin, label, None, None, obj)
            return run

        g_bytes, e_bytes = n * (12 * K + 4), n * (4 * K + 4)
        hip, tor = _spread_alt([grad(True), grad(False)])
        show("softmax_grad [hip]", hip, g_bytes)
        show("gradients + slices + maxima [torch]", tor)
        hip, tor = _spread_alt([metric(True), metric(False)])
        show("mlogloss + merror [hip, 2 launches]", hip, 2 * e_bytes)
        show("mlogloss + merror [torch]", tor)
        switches(True)
        # tile constants: rows R and chunk KC that the launch may take
        for chunk in (16, 32, 64):
            for rows in (64, 128, 192, 256):
                try:
                    t = _spread(lambda: ops.softmax_grad(
                        margin, label, chunk=chunk, rows=rows))
                except RuntimeError:
                    continue  # this tile does not fit the LDS budget
                show(f"softmax_grad chunk {chunk} rows {rows}", t, g_bytes)
        del margin, label

    n, F, K = train_shape
    gen = torch.Generator(device=dev).manual_seed(9)
    X = torch.randn(n, F, device=dev, generator=gen)
    y = torch.bucketize(X[:, 0] + 0.5 * X[:, 1],
                        torch.linspace(-1.5, 1.5, K - 1, device=dev)).float()
    dm = BinnedMatrix.build(X, label=y, max_bin=256)
    del X
    print(f"multi:softprob round, {n} x {F}, K = {K}, depth 6, mlogloss "
          f"every round; 10 rounds after 2 of warm-up")
    for run in range(2):
        for on in (True, False):
            switches(on)
            eng = BoostingEngine(
                {"objective": "multi:softprob", "num_class": K,
                 "max_depth": 6, "tree_method": "gpu_hist",
                 "eval_metric": ["mlogloss"]}, dm)
            for it in range(12):
                if it == 2:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                eng.update()
                loss = eng.eval_sets([EvalPack(name="train", X=None)])
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / 10 * 1e3
            print(f"  run {run} [{'hip' if on else 'torch'}] {ms:9.3f} "
                  f"ms/round  mlogloss {loss['train']['mlogloss']:.6f}",
                  flush=True)
    switches(True)


def bench_auc_multi(shapes=((11_000_000, 10), (2_000_000, 100)), n_bins=16384,
                    sweep=True):
    """``ops.eval_auc_multiclass``: its two kernels apart, the whole op,
    ``eval_multiclass`` on the same margin as the floor (one pass over
    [n, K]) and a torch composition of the same contract (float64 softmax,
    K integer ``scatter_add_``), windows alternating. GB/s is the compulsory
    traffic over the median: 4Kn read + 2Kn written for the row kernel, 2Kn
    read (+ 4n per class and plane with weights) for the count kernel."""
    from xgboost_ray_amd.ops import gpu

    dev = torch.device("cuda")

    def show(name, t, nbytes=None):
        rate = f"  {nbytes / t[0] / 1e6:8.1f} GB/s" if nbytes else ""
        print(f"  {name:42s} {t[0]:9.3f} ms  [{t[1]:.3f}, {t[2]:.3f}]{rate}",
              flush=True)

    for n, K in shapes:
        gen = torch.Generator(device=dev).manual_seed(11)
        margin = torch.randn(n, K, device=dev, generator=gen) * 3
        label = torch.randint(0, K, (n,), device=dev, generator=gen).float()
        wts = torch.rand(n, device=dev, generator=gen) * 2
        empty = torch.zeros(0, device=dev)
        codes = gpu.auc_bin_rows(margin, label, n_bins)
        hist = torch.zeros((K, 2, n_bins), dtype=torch.int64, device=dev)

        def torch_form(w):
            def run():
                p = torch.softmax(margin.double(), dim=1)
                b = (p * n_bins).long().clamp_(max=n_bins - 1)
                b += (label.long()[:, None] == torch.arange(
                    K, device=dev)[None, :]) * n_bins
                src = (torch.ones(n, dtype=torch.int64, device=dev)
                       if w is None else
                       torch.round(w.double() * 2.0 ** 20).long())
                h = torch.zeros((K, 2 * n_bins), dtype=torch.int64,
                                device=dev)
                for k in range(K):
                    h[k].scatter_add_(0, b[:, k], src)
                return h
            return run

        for w, tag in ((None, "unweighted"), (wts, "weighted")):
            print(f"auc_multi: {n} x {K}, {n_bins} bins, {tag}")
            wk = empty if w is None else w
            planes = 1 if w is None else 2
            ts = _spread_alt([
                lambda: gpu.auc_bin_rows(margin, label, n_bins),
                lambda: gpu.auc_count(codes, n, wk, hist),
                lambda: ops.eval_auc_multiclass(margin, label, w, n_bins),
                lambda: ops.eval_multiclass(margin, label, w),
                torch_form(w),
            ])
            c_bytes = planes * n * K * (2 + (0 if w is None else 4))
            show("auc_bin_rows_kernel", ts[0], 6 * n * K + 4 * n)
            show("auc_count_kernel", ts[1], c_bytes)
            show("eval_auc_multiclass (whole op)", ts[2],
                 6 * n * K + 4 * n + c_bytes)
            show("eval_multiclass (floor: one pass)", ts[3], 4 * n * K + 4 * n)
            show("torch: f64 softmax + K scatter_add_", ts[4])
        if sweep:
            for chunk in (16, 32):
                for rows in (128, 192, 256):
                    try:
                        t = _spread(lambda: gpu.auc_bin_rows(
                            margin, label, n_bins, chunk, rows))
                    except RuntimeError:
                        continue  # this tile does not fit the LDS budget
                    show(f"auc_bin_rows chunk {chunk} rows {rows}", t)
            for threads in (256, 512, 1024):
                for count_rows in (1 << 16, 1 << 18, 1 << 20, 0):
                    t = _spread(lambda: gpu.auc_count(
                        codes, n, empty, hist, count_rows, threads))
                    show(f"auc_count threads {threads} rows {count_rows}", t)
        del margin, label, wts, codes, hist


def bench_survival(sizes=(1_000_000, 10_000_000),
                   train_shape=(2_000_000, 28)):
    """The HIP survival kernels against the torch routes they replace, on the
    same tensors in one process, windows alternating. The torch gradient
    lines include the two ``abs().max()`` that ``_quantize`` then needs. Cox:
    distinct times, and ties in runs of about 10; AFT (normal): 30 %
    right-censored, and an even mix of the four kinds. Then one full round
    of each objective with and without the switches."""
    from xgboost_ray_amd.engine.metrics import get_metric
    from xgboost_ray_amd.engine.objectives import AFT, Cox
    from xgboost_ray_amd.engine.trainer import BoostingEngine, EvalPack

    dev = torch.device("cuda")

    def show(name, t):
        print(f"  {name:38s} {t[0]:9.3f} ms  [{t[1]:.3f}, {t[2]:.3f}]",
              flush=True)

    def switches(on):
        for name in ("RXGB_FUSED_GRAD", "RXGB_FUSED_EVAL"):
            if on:
                _os.environ.pop(name, None)
            else:
                _os.environ[name] = "0"

    def routes(obj, metric, margin, label):
        def grad(on):
            def run():
                switches(on)
                gp = obj.gradients(margin, label)
                if getattr(gp, "_rxgb_absmax", None) is None:
                    gp[:, 0].abs().max(), gp[:, 1].abs().max()
            return run

        def ev(on):
            def run():
                switches(on)
                metric.local_stats(margin, label, None, None, obj)
            return run

        hip, tor = _spread_alt([grad(True), grad(False)])
        show(f"{obj.name} gradients [hip]", hip)
        show(f"{obj.name} gradients + maxima [torch]", tor)
        hip, tor = _spread_alt([ev(True), ev(False)])
        show(f"{metric.name} [hip]", hip)
        show(f"{metric.name} [torch]", tor)
        switches(True)

    for n in sizes:
        gen = torch.Generator(device=dev).manual_seed(7)
        margin = torch.randn(n, device=dev, generator=gen) * 2
        u = torch.rand(n, device=dev, generator=gen)
        sign = torch.where(torch.rand(n, device=dev, generator=gen) < 0.7,
                           1.0, -1.0)
        for what, t in (("distinct times",
                         torch.randperm(n, device=dev, generator=gen) + 1.0),
                        ("ties in runs of ~10",
                         torch.floor(u * (n // 10)) + 1.0)):
            print(f"survival:cox, {n} rows, {what} "
                  f"(tile {ops.COX_TILE_ROWS})")
            routes(Cox(), get_metric("cox-nloglik"), margin, t * sign)
        lo = torch.exp(torch.randn(n, device=dev, generator=gen))
        for what, kind in (("30 % right-censored", (u < 0.3).long()),
                           ("even mix of the four kinds",
                            (u * 4).long().clamp(max=3))):
            hi = torch.where(kind == 1, float("inf"),
                             torch.where(kind == 3, lo * 2.5, lo))
            label = torch.stack(
                [torch.where(kind == 2, 0.0, lo),
                 torch.where(kind == 2, lo, hi)], dim=1).contiguous()
            print(f"survival:aft (normal), {n} rows, {what}")
            routes(AFT(), get_metric("aft-nloglik"), margin, label)

    n, F = train_shape
    gen = torch.Generator(device=dev).manual_seed(9)
    X = torch.randn(n, F, device=dev, generator=gen)
    t = torch.exp(0.7 * X[:, 0] + 0.3 * torch.randn(n, device=dev,
                                                    generator=gen))
    cens = torch.rand(n, device=dev, generator=gen) < 0.3
    dm = BinnedMatrix.build(X, max_bin=256)
    del X
    for objective, metric in (("survival:cox", "cox-nloglik"),
                              ("survival:aft", "aft-nloglik")):
        if objective == "survival:cox":
            dm.label = torch.where(cens, -t, t)
        else:
            dm.label = None
            dm.label_lower_bound = t
            dm.label_upper_bound = torch.where(cens, float("inf"), t)
        print(f"{objective} round, {n} x {F}, depth 6, {metric} every "
              f"round; 10 rounds after 2 of warm-up")
        for run in range(2):
            for on in (True, False):
                switches(on)
                eng = BoostingEngine(
                    {"objective": objective, "max_depth": 6,
                     "tree_method": "gpu_hist"}, dm)
                for it in range(12):
                    if it == 2:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                    eng.update()
                    loss = eng.eval_sets([EvalPack(name="train", X=None)])
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) / 10 * 1e3
                print(f"  run {run} [{'hip' if on else 'torch'}] {ms:9.3f} "
                      f"ms/round  {metric} {loss['train'][metric]:.6f}",
                      flush=True)
    switches(True)


def bench_pointwise(n=11_000_000, train_shape=(2_000_000, 28), K=3):
    """The HIP pointwise regression kernels against the torch routes they
    replace, on the same tensors in one process, windows alternating,
    unweighted and weighted. The torch gradient lines include the two
    ``abs().max()`` that ``_quantize`` then needs. ``pointwise train`` runs
    the end-to-end rounds alone."""
    from xgboost_ray_amd.engine import objectives as O
    from xgboost_ray_amd.engine.metrics import get_metric
    from xgboost_ray_amd.engine.trainer import BoostingEngine, EvalPack

    dev = torch.device("cuda")

    def show(name, t):
        print(f"  {name:46s} {t[0]:9.3f} ms  [{t[1]:.3f}, {t[2]:.3f}]"
              f"{'  outside' if len(t) > 3 and t[3] else ''}", flush=True)

    def switches(on):
        for name in ("RXGB_FUSED_GRAD", "RXGB_FUSED_EVAL"):
            if on:
                _os.environ.pop(name, None)
            else:
                _os.environ[name] = "0"

    def pair(name, fn):
        def route(on):
            def run():
                switches(on)
                fn()
            return run
        hip, tor = _spread_alt([route(True), route(False)])
        # the hip route earns its default only outside the torch spread
        show(f"{name} [hip]", hip + (hip[0] < tor[1] or hip[0] > tor[2],))
        show(f"{name} [torch]", tor)
        switches(True)

    def grad(obj, margin, label, weight):
        def run():
            gp = obj.gradients(margin, label, weight)
            if (getattr(gp, "_rxgb_absmax", None) is None
                    and getattr(gp, "_rxgb_absmax_cls", None) is None):
                gp[..., 0].abs().amax(0), gp[..., 1].abs().amax(0)
        return run

    if _sys.argv[2:3] != ["train"]:
        gen = torch.Generator(device=dev).manual_seed(7)
        margin = torch.randn(n, device=dev, generator=gen)
        margin_k = torch.randn(n, K, device=dev, generator=gen)
        pos = torch.rand(n, device=dev, generator=gen) * 3 + 0.2
        labels = {"count:poisson": torch.floor(2 * pos),
                  "binary:hinge": (pos > 1.5).float()}
        wts = torch.rand(n, device=dev, generator=gen) * 3 + 0.25
        alphas = [0.1, 0.5, 0.9][:K]
        for what, w in (("unweighted", None), ("weighted", wts)):
            print(f"pointwise gradients, {n} rows, {what}")
            for name in ("reg:absoluteerror", "count:poisson", "reg:gamma",
                         "reg:tweedie", "reg:squaredlogerror",
                         "reg:pseudohubererror", "binary:hinge"):
                obj = O.get_objective(name)
                pair(name, grad(obj, margin, labels.get(name, pos), w))
            pair("reg:quantileerror K=1",
                 grad(O.QuantileError(alphas[:1]), margin, pos, w))
            pair(f"reg:quantileerror K={K}",
                 grad(O.QuantileError(alphas), margin_k, pos, w))
            print(f"pointwise metrics, {n} rows, {what}")
            for metric, name in (("rmse", "reg:squarederror"),
                                 ("rmse", "binary:logistic"),
                                 ("mae", "reg:absoluteerror"),
                                 ("mape", "reg:gamma"),
                                 ("rmsle", "reg:squaredlogerror"),
                                 ("mphe", "reg:pseudohubererror"),
                                 ("poisson-nloglik", "count:poisson"),
                                 ("gamma-nloglik", "reg:gamma"),
                                 ("tweedie-nloglik@1.5", "reg:tweedie")):
                obj, m = O.get_objective(name), get_metric(metric)
                y = labels.get(name, pos)
                pair(f"{metric} ({obj.eval_transform})",
                     lambda: m.local_stats(margin, y, w, None, obj))
            for a, mk in ((alphas[:1], margin), (alphas, margin_k)):
                obj, m = O.QuantileError(a), get_metric("quantile")
                pair(f"quantile K={len(a)}",
                     lambda: m.local_stats(mk, pos, w, None, obj))
        del margin, margin_k, wts, labels, pos

    n, F = train_shape
    gen = torch.Generator(device=dev).manual_seed(9)
    X = torch.randn(n, F, device=dev, generator=gen)
    y = torch.exp(0.7 * X[:, 0] + 0.3 * torch.randn(n, device=dev,
                                                    generator=gen))
    dm = BinnedMatrix.build(X, label=y, max_bin=256)
    del X
    for objective, extra in (("reg:tweedie", {}),
                             ("reg:quantileerror", {"quantile_alpha": 0.5})):
        for with_eval in (False, True):
            print(f"{objective} round, {n} x {F}, depth 8, "
                  f"{'default metric every round' if with_eval else 'no eval'}"
                  f"; 10 rounds after 2 of warm-up")
            for run in range(2):
                for on in (True, False):
                    switches(on)
                    eng = BoostingEngine(
                        {"objective": objective, "max_depth": 8,
                         "tree_method": "gpu_hist", **extra}, dm)
                    for it in range(12):
                        if it == 2:
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                        eng.update()
                        if with_eval:
                            eng.eval_sets([EvalPack(name="train", X=None)])
                    torch.cuda.synchronize()
                    ms = (time.perf_counter() - t0) / 10 * 1e3
                    print(f"  run {run} [{'hip' if on else 'torch'}] "
                          f"{ms:9.3f} ms/round", flush=True)
    switches(True)


def bench_sketch(shapes=((11_000_000, 28), (1_000_000, 200)),
                 train_shape=(2_000_000, 28)):
    """The HIP weighted sketch (tree_method="approx"): every radix pass
    alone on the tables the real select produced, the whole
    ``weighted_cuts`` (passes + select), the re-bin into the resident
    matrix and the ``bins_t`` refresh; and, windows alternating in the same
    process, sketch + re-bin against the torch ``build_cuts`` +
    ``bin_matrix`` of the hist route on the same data. ``sketch train``
    runs approx against hist rounds alone."""
    from xgboost_ray_amd.engine.quantile import build_cuts
    from xgboost_ray_amd.engine.trainer import BoostingEngine

    dev = torch.device("cuda")

    def show(name, t):
        print(f"  {name:46s} {t[0]:9.3f} ms  [{t[1]:.3f}, {t[2]:.3f}]",
              flush=True)

    for n, F in (() if _sys.argv[2:3] == ["train"] else shapes):
        print(f"sketch, {n} x {F}, max_bin 256, hessian-like int32 weights")
        gen = torch.Generator(device=dev).manual_seed(3)
        X = torch.randn(n, F, device=dev, generator=gen)
        p = torch.sigmoid(torch.randn(n, device=dev, generator=gen))
        gq = torch.stack([p, p * (1 - p) * 4], 1).mul_(2.0 ** 30).round_().to(
            torch.int32)
        W = gq[:, 1]
        col_max = X.amax(0)
        calls = []
        real_pass = ops.sketch_pass
        ops.sketch_pass = lambda *a: (calls.append(a), real_pass(*a))[1]
        cuts = ops.weighted_cuts(X, W, 256, col_max)
        ops.sketch_pass = real_pass
        passes = 0.0
        for a in calls:
            out = torch.zeros_like(a[6])
            t = _spread(lambda: real_pass(*a[:6], out))
            show(f"pass {a[4]} ({int(a[3].sum())} slots)", t)
            passes += t[0]
        del out, calls
        whole = _spread(lambda: ops.weighted_cuts(X, W, 256, col_max))
        show("weighted_cuts (4 passes + select)", whole)
        print(f"  {'select and glue (whole - passes)':46s} "
              f"{whole[0] - passes:9.3f} ms")
        bins = ops.bin_matrix(X, cuts.cuts_flat, cuts.cut_ptr)
        bins_t = bins.t().contiguous()
        show("re-bin (bin_matrix out=)", _spread(lambda: ops.bin_matrix(
            X, cuts.cuts_flat, cuts.cut_ptr, out=bins)))
        show("bins_t refresh", _spread(lambda: bins_t.copy_(bins.t())))

        def hip():
            c = ops.weighted_cuts(X, W, 256, col_max)
            ops.bin_matrix(X, c.cuts_flat, c.cut_ptr, out=bins)

        def parent():
            c = build_cuts(X, 256)
            ops.bin_matrix(X, c.cuts_flat, c.cut_ptr)

        th, tp = _spread_alt([hip, parent], reps=3, inner=1)
        show("sketch + re-bin [hip, weighted]", th)
        show("build_cuts + bin_matrix [torch, unweighted]", tp)
        del X, W, gq, bins, bins_t

    n, F = train_shape
    gen = torch.Generator(device=dev).manual_seed(9)
    X = torch.randn(n, F, device=dev, generator=gen)
    y = (X[:, 0] + 0.5 * X[:, 1] > 0).float()
    dms = {"gpu_approx": BinnedMatrix.build(X, label=y, max_bin=256,
                                            keep_raw=True),
           "gpu_hist": BinnedMatrix.build(X, label=y, max_bin=256)}
    print(f"binary:logistic round, {n} x {F}, depth 8; 10 rounds after 2 of "
          f"warm-up (approx: per-depth path unless the enqueue applies)")
    for run in range(2):
        for tm in ("gpu_approx", "gpu_hist"):
            eng = BoostingEngine({"objective": "binary:logistic",
                                  "max_depth": 8, "tree_method": tm},
                                 dms[tm])
            for it in range(12):
                if it == 2:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                eng.update()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / 10 * 1e3
            print(f"  run {run} [{tm}, {eng.last_tree_path}] "
                  f"{ms:9.3f} ms/round", flush=True)


def main():
    if _sys.argv[1:2] == ["sketch"]:
        return bench_sketch()
    if _sys.argv[1:2] == ["pointwise"]:
        return bench_pointwise()
    if _sys.argv[1:2] == ["survival"]:
        return bench_survival()
    if _sys.argv[1:2] == ["softmax"]:
        return bench_softmax()
    if _sys.argv[1:2] == ["auc_multi"]:
        return bench_auc_multi()
    if _sys.argv[1:2] == ["rank"]:
        return bench_rank()
    if _sys.argv[1:2] == ["leaf_quantile"]:
        return bench_leaf_quantile()
    if _sys.argv[1:2] in (["predict_leaf"], ["saabas"]):
        return bench_walk(modes=(_sys.argv[1],))
    if _sys.argv[1:2] == ["walk"]:
        return bench_walk()
    if _sys.argv[1:2] == ["tree_shap"]:
        return bench_tree_shap()
    if _sys.argv[1:2] == ["mvs"]:  # mvs [rows]
        return bench_mvs(*(int(a) for a in _sys.argv[2:3]))
    n, F = 11_000_000, 28
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn(n, F, device=dev, generator=gen)
    y = (X[:, 0] > 0).float()
    dm = BinnedMatrix.build(X, label=y, max_bin=256)
    del X
    bins = dm.bins
    print("bins stride:", bins.stride(0), "shape", tuple(bins.shape))

    gp = torch.stack([y - 0.5, torch.ones(n, device=dev)], dim=1)
    gq = ops.quantize_gpair(gp, 2.0**28, 2.0**27)
    ridx = torch.randperm(n, device=dev).to(torch.int32)

    # depth-8-like frontier: 128 nodes to build
    K = 128
    cut = torch.sort(
        torch.randint(1, n - 1, (K - 1,), generator=gen, device=dev)
    )[0].cpu()
    starts = torch.cat([torch.tensor([0]), cut]).long()
    ends = torch.cat([cut, torch.tensor([n])]).long()
    counts = ends - starts

    timeit("quantize", lambda: ops.quantize_gpair(gp, 2.0**28, 2.0**27))
    timeit(
        "hist K=1",
        lambda: ops.build_histogram(
            bins, gq, ridx, torch.tensor([0]), torch.tensor([n]),
            dm.cuts.max_bins,
        ),
    )
    timeit(
        "hist K=128",
        lambda: ops.build_histogram(
            bins, gq, ridx, starts, counts, dm.cuts.max_bins
        ),
    )
    hist = ops.build_histogram(bins, gq, ridx, starts, counts, dm.cuts.max_bins)
    pg = hist[:, 0, :, 0].sum(1).contiguous()
    ph = hist[:, 0, :, 1].sum(1).contiguous()
    timeit(
        "find_splits K=128",
        lambda: ops.find_splits(
            hist, pg, ph, dm.cuts.feat_bins().cuda(), 2.0**28, 2.0**27,
            1.0, 0.0, 0.0, 1.0,
        ),
    )
    small_hist = hist[:2].contiguous()
    timeit(
        "find_splits K=2",
        lambda: ops.find_splits(
            small_hist, pg[:2].contiguous(), ph[:2].contiguous(),
            dm.cuts.feat_bins().cuda(), 2.0**28, 2.0**27, 1.0, 0.0, 0.0, 1.0,
        ),
    )
    sf = torch.randint(0, F, (K,), dtype=torch.int32)
    sb = torch.randint(0, 100, (K,), dtype=torch.int32)
    dl = torch.randint(0, 2, (K,), dtype=torch.uint8)
    timeit(
        "partition K=128",
        lambda: ops.partition_rows(bins, ridx, starts, counts, sf, sb, dl),
    )
    lv = np.random.randn(K).astype(np.float32)
    m = torch.zeros(n, device=dev)
    timeit(
        "update_margins",
        lambda: ops.update_margins(m, ridx, starts, counts, lv),
    )
    # torch glue pieces
    timeit("stack 128 hists", lambda: torch.stack([hist[i] for i in range(K)]))
    timeit("root_sum gather", lambda: gq[ridx.long()].sum(dim=0))
    timeit(
        "gradients(sigmoid)",
        lambda: torch.sigmoid(m),
    )

    # serving: packed-node tree-walk over a realistic 100-tree depth-8 model
    from xgboost_ray_amd.engine.trainer import run_training

    small = BinnedMatrix.build(
        torch.randn(500_000, F, device=dev, generator=gen),
        label=(torch.rand(500_000, device=dev, generator=gen) > 0.5).float(),
        max_bin=256,
    )
    bst = run_training(
        {"objective": "binary:logistic", "max_depth": 8, "eta": 0.1}, small, 100
    )
    Xp = torch.randn(2_000_000, F, device=dev, generator=gen)
    flat = bst._flat_trees(dev)
    out = torch.zeros(2_000_000, device=dev)
    from xgboost_ray_amd.ops import gpu as gops

    dt = timeit(
        "predict 2M x 100 trees",
        lambda: gops.predict_trees(
            Xp, flat["feat"], flat["thr"], flat["left"],
            flat["default_left"], flat["value"], flat["tree_ptr"], out,
        ),
        reps=10,
    )
    print(f"serving throughput: {2_000_000 / dt * 1000 / 1e6:.1f} M rows/s "
          f"(100 trees, depth 8)")
    del Xp, out, small, dm, bins, gq, gp, hist, m
    bench_leaf_quantile()


if __name__ == "__main__":
    main()
