"""Flagship benchmark: HIGGS-class distributed gpu_hist training.

Measures the BASELINE.json headline metric - boosting rounds/sec (+ AUC)
on an 11M x 28 binary:logistic workload, tree_method gpu_hist, depth 8,
max_bin 256 - on N MI355X GPUs (weak scaling: 11M rows per GPU, synthetic
data of the HIGGS shape, random-init trees; no network for the real CSV).
The train AUC is reported for the SYNTHETIC task and is not comparable to
real-HIGGS AUC numbers; the rounds/s timing is the measured metric.

A plain run sets up, warms up, times ``--steps`` rounds and prints ONE JSON
line. With ``--full`` on a single GPU the emitted JSON also carries
``config.secondary_config``: the 100M x 200 reg:squarederror single-GPU
form of BASELINE config 3, measured back-to-back in the same process
(stdout stays ONE JSON line, per the driver contract).

``--dump-outputs DIR`` writes what the last timed round computed - the
tree it returned and the training margins it left behind - as
``DIR/<name>.npy`` so two builds can be compared output for output (the
synthetic inputs are seeded, so equal arguments give equal inputs).

Single process: `python bench.py --gpus 1 --steps K --warmup W`.
Multi-GPU: launched by the driver as one rank per GPU via
`python -m torch.distributed.run --nproc-per-node N bench.py ...`
(reads RANK/WORLD_SIZE/MASTER_* from the env; backend nccl == RCCL over
xGMI).
"""

import argparse
import json
import os
import time

import numpy as np
import torch


def synth_higgs(n_rows: int, n_features: int, device, seed: int):
    """Synthetic HIGGS-shaped binary task (fp32, learnable signal).

    Generated directly on the target device so 100M x 200-class shapes
    never materialize on the host (80 GB fits in 288 GB HBM, not in RAM).
    """
    gen = torch.Generator(device=device).manual_seed(seed)
    X = torch.empty(n_rows, n_features, dtype=torch.float32, device=device)
    X.normal_(generator=gen)
    w = torch.randn(n_features, generator=gen, device=device) * 0.5
    logits = X @ w + 0.4 * (X[:, 0] * X[:, 1]) - 0.2 * X[:, 2] ** 2
    noise = torch.randn(n_rows, generator=gen, device=device)
    y = (logits + noise > 0).to(torch.float32)
    return X, y


# --dump-outputs budget: 64 MB in all; the margins get 48 MB of it and
# the single tree of the last round is a few hundred KB at most
DUMP_MARGIN_MAX_ELEMS = 12_000_000
DUMP_SAMPLE_SEED = 20240607


def dump_outputs(dump_dir: str, trees, margin: torch.Tensor):
    """Write the last timed round's results as float32/float64 .npy files.

    `trees` is what BoostingEngine.update() returned in that round and
    `margin` the per-row training margins after it. Margins larger than
    the budget are written as a fixed seeded sample of their (flattened)
    elements, with the sampled positions alongside.
    """
    os.makedirs(dump_dir, exist_ok=True)
    flat = margin.detach().reshape(-1)
    if flat.numel() > DUMP_MARGIN_MAX_ELEMS:
        rng = np.random.RandomState(DUMP_SAMPLE_SEED)
        idx = np.sort(rng.randint(
            0, flat.numel(), size=DUMP_MARGIN_MAX_ELEMS // 4
        ).astype(np.int64))
        sel = flat[torch.from_numpy(idx).to(flat.device)]
        np.save(os.path.join(dump_dir, "margin_sample_index.npy"),
                idx.astype(np.float64))
        np.save(os.path.join(dump_dir, "margin_sample.npy"),
                sel.cpu().numpy().astype(np.float32))
    else:
        np.save(os.path.join(dump_dir, "margin.npy"),
                flat.cpu().numpy().astype(np.float32))
    for i, t in enumerate(trees):
        for field in ("feat", "thr", "left", "default_left", "value",
                      "gain", "cover"):
            np.save(
                os.path.join(dump_dir, f"last_tree{i}_{field}.npy"),
                np.asarray(getattr(t, field)).astype(np.float32),
            )


def run_config(
    coll,
    device,
    use_gpu: bool,
    rank: int,
    world: int,
    rows: int,
    features: int,
    objective: str,
    max_depth: int,
    max_bin: int,
    steps: int,
    warmup: int,
    dump_dir=None,
):
    """Train `steps` timed rounds on one synthetic config; returns the
    result dict (rank 0) or None. With `dump_dir`, rank 0 also writes the
    last timed round's outputs there (after the timed region)."""
    from xgboost_ray_amd.engine.metrics import get_metric
    from xgboost_ray_amd.engine.quantile import BinnedMatrix
    from xgboost_ray_amd.engine.trainer import BoostingEngine

    # weak scaling: each rank owns `rows` of its own synthetic shard
    X, y = synth_higgs(rows, features, device, seed=1234 + rank)
    if objective == "reg:squarederror":
        # regression target: the underlying continuous signal
        gen = torch.Generator(device=device).manual_seed(99 + rank)
        y = (X[:, 0] * 2 - X[:, 1] +
             0.1 * torch.randn(rows, generator=gen, device=device))
    if use_gpu:
        torch.cuda.synchronize()

    build_t0 = time.perf_counter()
    dm = BinnedMatrix.build(
        X, label=y, max_bin=max_bin, collective=coll, seed=0
    )
    del X
    if use_gpu:
        torch.cuda.synchronize()
    build_s = time.perf_counter() - build_t0

    params = {
        "objective": objective,
        "tree_method": "gpu_hist" if use_gpu else "hist",
        "max_depth": max_depth,
        "max_bin": max_bin,
        "eta": 0.1,
    }
    engine = BoostingEngine(params, dm, collective=coll, rank=rank)

    for _ in range(warmup):
        engine.update()

    coll.barrier()
    if use_gpu:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    last_trees = []
    for _ in range(steps):
        last_trees = engine.update()
    if use_gpu:
        torch.cuda.synchronize()
    coll.barrier()
    elapsed = time.perf_counter() - t0

    # MAX over ranks
    el_t = torch.tensor(
        [elapsed], dtype=torch.float64,
        device=device if use_gpu else "cpu",
    )
    if world > 1:
        coll.allreduce_(el_t, op="max")
    elapsed_max = float(el_t[0])

    if dump_dir and rank == 0:
        dump_outputs(dump_dir, last_trees, engine.margin)

    # final train quality (the metric's second half; rmse for regression)
    quality_name = "auc" if objective == "binary:logistic" else "rmse"
    m = get_metric(quality_name)
    st = m.local_stats(engine.margin, dm.label, None, None, None)
    if world > 1:
        st_d = st.to(device) if use_gpu else st
        coll.allreduce_(st_d)
        st = st_d.cpu()
    quality = m.finalize(st.cpu())

    rounds_per_sec = steps / elapsed_max
    is_higgs = (objective == "binary:logistic"
                and rows == 11_000_000 and features == 28)
    out = {
        "metric": "boost_rounds_per_sec",
        "value": rounds_per_sec,
        "unit": "rounds/s",
        "n_gpus": world if use_gpu else 0,
        "steps": steps,
        "warmup": warmup,
        "ms_per_step": elapsed_max * 1000.0 / steps,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "fp32",
        "data": "synthetic-higgs-shape",
        "config": {
            "model": (
                "higgs-11m-x28-binary-logistic-gpu-hist" if is_higgs
                else f"synthetic-{rows}x{features}-{objective}-gpu-hist"
            ),
            "global_batch": rows * world,
            "seq_len": features,
            "parallelism": f"dp{world}",
            "n_rows_per_gpu": rows,
            "n_features": features,
            "max_depth": max_depth,
            "max_bin": max_bin,
            f"train_{quality_name}": quality,
            "quality_caveat": (
                "synthetic normal features of the HIGGS shape; the "
                "quality value is for the synthetic task and is NOT "
                "comparable to real-HIGGS numbers"
            ),
            "matrix_build_s": build_s,
            "rows_per_sec": rows * world * rounds_per_sec,
        },
    }
    # free GPU memory for any follow-up config in the same process
    del engine, dm
    if use_gpu:
        torch.cuda.empty_cache()
    return out if rank == 0 else None


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    # defaults sized so the timed region spans multiple seconds: the
    # driver samples rocm-smi busy% around the run, and a sub-second
    # region reads 0.0 (round-1 lesson)
    p.add_argument("--steps", type=int, default=400)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--rows", type=int, default=11_000_000)
    p.add_argument("--features", type=int, default=28)
    p.add_argument("--max-depth", type=int, default=8)
    p.add_argument("--max-bin", type=int, default=256)
    p.add_argument("--objective", default="binary:logistic",
                   choices=["binary:logistic", "reg:squarederror"])
    p.add_argument("--cpu", action="store_true", help="force CPU (debug)")
    p.add_argument("--full", action="store_true",
                   help="also measure the 100Mx200 secondary config "
                        "(1 GPU, default shape)")
    p.add_argument("--skip-secondary", action="store_true",
                   help="with --full: skip the 100Mx200 secondary config")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write the last timed round's outputs (tree + "
                        "training margins) as DIR/<name>.npy")
    args = p.parse_args()
    if args.steps < 1:
        p.error("--steps must be >= 1")

    import torch.distributed as dist

    from xgboost_ray_amd.engine.collective import Collective

    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local_rank = int(os.environ.get("LOCAL_RANK", rank))

    use_gpu = torch.cuda.is_available() and not args.cpu
    if use_gpu:
        # modulo: several ranks may share one GPU (gloo-staged transport
        # experiments on a 1-GPU box)
        dev_id = local_rank % max(1, torch.cuda.device_count())
        torch.cuda.set_device(dev_id)
        device = torch.device("cuda", dev_id)
    else:
        device = torch.device("cpu")

    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # RXGB_COLL_BACKEND=gloo: host-staged transport with GPU compute
        # (e.g. several ranks sharing one MI355X, where RCCL refuses
        # duplicate devices in a communicator)
        backend = os.environ.get("RXGB_COLL_BACKEND") or (
            "nccl" if use_gpu else "gloo"
        )
        dist.init_process_group(
            backend=backend,
            init_method="env://",
            rank=rank,
            world_size=world,
        )
    coll = Collective(rank=rank, world_size=world, device=device)

    out = run_config(
        coll, device, use_gpu, rank, world,
        rows=args.rows, features=args.features, objective=args.objective,
        max_depth=args.max_depth, max_bin=args.max_bin,
        steps=args.steps, warmup=args.warmup,
        dump_dir=args.dump_outputs,
    )

    # Secondary config (single-GPU form of BASELINE config 3), --full only:
    # 100M x 200 reg:squarederror. Only on 1 GPU at default shape, so
    # multi-GPU SCALE runs stay a single clean timed region.
    run_secondary = (
        args.full and use_gpu and world == 1 and not args.skip_secondary
        and args.rows == 11_000_000 and args.features == 28
        and args.objective == "binary:logistic"
    )
    if run_secondary:
        try:
            sec = run_config(
                coll, device, use_gpu, rank, world,
                rows=100_000_000, features=200,
                objective="reg:squarederror",
                max_depth=args.max_depth, max_bin=args.max_bin,
                steps=min(args.steps, 40), warmup=min(args.warmup, 5),
            )
            if out is not None and sec is not None:
                out["config"]["secondary_config"] = sec
        except Exception as e:  # OOM on smaller dev GPUs: keep headline
            if out is not None:
                out["config"]["secondary_error"] = repr(e)

    if rank == 0 and out is not None:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
