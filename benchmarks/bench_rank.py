"""Ranking flagship: rank:ndcg lambdarank rounds/s on synthetic groups.

Usage: python benchmarks/bench_rank.py [--rows N] [--group G] [--steps K]
       [--eval]   (also evaluate ndcg@10 on the training set every round)
       [--topk K] (lambdarank_pair_method="topk" with K pairs per sample)
(BASELINE configs list 'RayXGBRanker rank:ndcg on synthetic MSLR-style
groups'; this measures the engine-level round time on one GPU.)
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import numpy as np
import torch

from xgboost_ray_amd.engine.quantile import BinnedMatrix
from xgboost_ray_amd.engine.trainer import BoostingEngine, EvalPack


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--features", type=int, default=136)  # MSLR-style
    ap.add_argument("--group", type=int, default=100)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--eval", action="store_true",
                    help="evaluate ndcg@10 on the training set each round")
    ap.add_argument("--topk", type=int, default=0,
                    help="top-k pair truncation with this k (0: all pairs)")
    args = ap.parse_args()
    dev = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    g = torch.Generator(device=dev).manual_seed(7)
    X = torch.randn(args.rows, args.features, generator=g, device=dev)
    rel = (X[:, 0] * 2 + X[:, 1] + 0.5 * torch.randn(
        args.rows, generator=g, device=dev)).clamp(0, 4)
    y = rel.round().float()
    qid = torch.arange(args.rows, device=dev) // args.group
    dm = BinnedMatrix.build(X, label=y, qid=qid, max_bin=256)
    del X
    params = {"objective": "rank:ndcg", "max_depth": 8, "eta": 0.1,
              "eval_metric": ["ndcg@10"]}
    if args.topk:
        params.update(lambdarank_pair_method="topk",
                      lambdarank_num_pair_per_sample=args.topk)
    eng = BoostingEngine(params, dm)
    train = [EvalPack(name="train", X=None)]

    def step():
        eng.update()
        return eng.eval_sets(train) if args.eval else None

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize() if dev.type == "cuda" else None
    t0 = time.perf_counter()
    for _ in range(args.steps):
        res = step()
    torch.cuda.synchronize() if dev.type == "cuda" else None
    dt = (time.perf_counter() - t0) / args.steps
    print(f"rank:ndcg {args.rows}x{args.features} group={args.group} "
          f"pairs={'top-%d' % args.topk if args.topk else 'all'}: "
          f"{dt * 1000:.2f} ms/round = {1 / dt:.1f} rounds/s"
          + (f", train {res['train']}" if args.eval else ""))


if __name__ == "__main__":
    main()
