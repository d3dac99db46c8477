"""Prediction intervals with reg:quantileerror: one model, three quantiles.

Each alpha gets its own tree per round; every finished leaf is re-fitted to
the exact weighted alpha-quantile of the residuals that landed in it, so the
model is the same for any number of actors.
"""

import argparse

import numpy as np

from xgboost_ray_amd import RayDMatrix, RayParams, predict, train


def main(cpus_per_actor, num_actors):
    rng = np.random.RandomState(1234)
    n, f = 50_000, 8
    X = rng.randn(n, f).astype(np.float32)
    # heteroscedastic noise: the interval must widen with |x1|
    y = (2 * X[:, 0] + (0.5 + np.abs(X[:, 1])) * rng.randn(n)).astype(
        np.float32
    )
    alphas = [0.05, 0.5, 0.95]
    ray_params = RayParams(num_actors=num_actors,
                           cpus_per_actor=cpus_per_actor)
    train_set = RayDMatrix(X, label=y)
    evals_result = {}
    bst = train(
        {"objective": "reg:quantileerror", "quantile_alpha": alphas,
         "max_depth": 5, "eta": 0.2},
        train_set,
        num_boost_round=40,
        evals=[(train_set, "train")],
        evals_result=evals_result,
        verbose_eval=False,
        ray_params=ray_params,
    )
    pred = predict(bst, RayDMatrix(X), ray_params=ray_params)  # [n, 3]
    lo, mid, hi = pred[:, 0], pred[:, 1], pred[:, 2]
    print("pinball loss: {:.4f}".format(evals_result["train"]["quantile"][-1]))
    print("90% interval coverage: {:.3f}".format(
        float(((y >= lo) & (y <= hi)).mean())))
    print("mean width, |x1| < 0.5: {:.2f}   |x1| > 1.5: {:.2f}".format(
        float((hi - lo)[np.abs(X[:, 1]) < 0.5].mean()),
        float((hi - lo)[np.abs(X[:, 1]) > 1.5].mean())))
    print("median MAE: {:.3f}".format(float(np.abs(y - mid).mean())))


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--num-actors", type=int, default=2)
    parser.add_argument("--cpus-per-actor", type=int, default=1)
    args = parser.parse_args()
    main(args.cpus_per_actor, args.num_actors)
