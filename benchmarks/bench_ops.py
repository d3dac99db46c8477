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


def main():
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
