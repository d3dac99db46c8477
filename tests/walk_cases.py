"""Cases and references for the leaf-index and Saabas tree walks
(``ops.predict_leaf`` / ``ops.saabas_contribs``).

The forests, rows and edge-case asserts are those of
``aux_cases.predict_cases()``; this module adds the float64 node means,
the non-zero ``out`` the Saabas walk accumulates into, and the two
references. It imports neither ``ops`` nor ``booster``.

Every comparison made with these references is exact: a leaf index is an
integer, and the Saabas sums are float64 adds and subtracts in one fixed
sequence per row - for each tree in order ``out[F] += mean[root]``, then
per split from the root down ``out[feat] += mean[child] - mean[node]`` -
starting from what ``out`` holds.
"""

import functools

import numpy as np

import aux_cases as ac


def ref_leaves(X, forest):
    """int32 [n, T]: leaf of every row in every tree, relative to the
    tree's root."""
    leaves = ac._leaves_np(X, forest)
    return (leaves - forest["tree_ptr"][:-1, None].astype(np.int64)).T \
        .astype(np.int32)


def saabas_row_py(x, forest, node_mean, out_row, order=None):
    """The stated sequence for one row, plain Python, in place."""
    F = len(x)
    T = len(forest["tree_ptr"]) - 1
    for t in (range(T) if order is None else order):
        base = int(forest["tree_ptr"][t])
        node = base
        out_row[F] = out_row[F] + node_mean[base]
        while forest["feat"][node] >= 0:
            f = int(forest["feat"][node])
            v = x[f]
            if v != v:
                go_left = bool(forest["default_left"][node])
            else:
                go_left = bool(np.float32(v) < forest["thr"][node])
            child = base + int(forest["left"][node]) + (0 if go_left else 1)
            out_row[f] = out_row[f] + (node_mean[child] - node_mean[node])
            node = child
    return out_row


def ref_saabas(X, forest, node_mean, out0, order=None):
    """float64 [n, F+1]: the stated sequence for every row, vectorised over
    rows (a row meets one split per level, so a level's fancy-indexed
    update touches each cell once)."""
    n, F = X.shape
    T = len(forest["tree_ptr"]) - 1
    out = np.array(out0, np.float64)
    rows_all = np.arange(n)
    for t in (range(T) if order is None else order):
        base = int(forest["tree_ptr"][t])
        out[:, F] = out[:, F] + node_mean[base]
        cur = np.full(n, base, np.int64)
        while True:
            live = forest["feat"][cur] >= 0
            if not live.any():
                break
            rows, node = rows_all[live], cur[live]
            f = forest["feat"][node]
            x = X[rows, f]
            with np.errstate(invalid="ignore"):
                go_left = np.where(np.isnan(x),
                                   forest["default_left"][node] != 0,
                                   x < forest["thr"][node])
            child = base + forest["left"][node] + np.where(go_left, 0, 1)
            out[rows, f] = out[rows, f] + (node_mean[child] - node_mean[node])
            cur[rows] = child
    return out


def _magnitudes(rng, shape):
    """Random float64 of magnitude 1e-3 .. 1e3, never zero."""
    v = rng.randn(*shape) * 10.0 ** rng.uniform(-3, 3, shape)
    v[v == 0] = 1.0
    return v


def _walk_case(c, seed):
    X, forest = c["X"], c["forest"]
    n, F = X.shape
    T = len(forest["tree_ptr"]) - 1
    leaves = ref_leaves(X, forest)
    assert leaves.shape == (n, T) and leaves.dtype == np.int32
    # The order of the sums must be visible in the bits, or an exact
    # comparison would not test it: reversed tree order has to change the
    # result. With a single row that is a matter of the draw, so draw
    # again (a fixed seed sequence) until it does.
    for attempt in range(8):
        rng = np.random.RandomState(seed + 1000 * attempt)
        node_mean = _magnitudes(rng, (len(forest["feat"]),))
        out0 = _magnitudes(rng, (n, F + 1))
        saabas = ref_saabas(X, forest, node_mean, out0)
        if T == 1 or not np.array_equal(
                ref_saabas(X, forest, node_mean, out0,
                           order=range(T - 1, -1, -1)), saabas):
            break
    else:
        raise AssertionError(f"{c['id']}: tree order never shows")
    assert (out0 != 0).all()          # bias column included
    assert 1e-3 < np.abs(node_mean).max() and np.abs(node_mean).min() < 1e3
    for r in ac.sample_rows(n)[::7]:  # the vectorised walk is the row loop
        row = saabas_row_py(X[r], forest, node_mean, out0[r].copy())
        assert np.array_equal(row, saabas[r]), (c["id"], r)
    return {"id": c["id"], "forest_name": c["forest_name"], "n": n, "F": F,
            "T": T, "X": X, "forest": forest, "tiles": c["tiles"],
            "node_mean": node_mean, "out0": out0, "ref_leaves": leaves,
            "ref_saabas": saabas}


@functools.lru_cache(maxsize=None)
def walk_cases():
    cases = tuple(_walk_case(c, 7000 + i)
                  for i, c in enumerate(ac.predict_cases()))
    assert {c["forest_name"] for c in cases} == set(ac.PRED_FORESTS)
    assert {c["n"] for c in cases} == set(ac.PRED_NS)
    assert {c["F"] for c in cases} == {1, 7, 33}
    # a tree whose root is a leaf gives 0
    for c in cases:
        if c["forest_name"] == "leafroot":
            assert not c["ref_leaves"].any()
    return cases


@functools.lru_cache(maxsize=None)
def wide_cases(Fs):
    """A three-tree forest on 300 rows (more than one block) for each
    feature count in ``Fs`` - the widths at which the Saabas kernel
    changes its block size or leaves the LDS accumulators."""
    return tuple(
        _walk_case(ac._predict_case((3, 7, 15), 300, F, 1.0, "zero", 7100 + i),
                   7200 + i)
        for i, F in enumerate(Fs))


def torch_forest(forest):
    """The forest's arrays as the CPU tensors the ops take."""
    import torch

    return {k: torch.from_numpy(np.ascontiguousarray(forest[k]))
            for k in ("feat", "thr", "left", "default_left", "tree_ptr")}
