"""The CPU oracle (``ops/cpu.py``) against independent brute-force references.

The GPU tests trust ``ops/cpu.py``; this file checks that trust on every
generated case of ``tests/op_cases.py`` with references that are a different
algorithm: Python ints and ``float`` loops, one row / one candidate at a
time. All comparisons are exact. Runs on any machine (no GPU).

Brute-force cap: a histogram or partition case is looped row by row only
when its segments hold at most ``BRUTE_MAX_ROWS`` rows, and a split case only
when ``K*F*B <= BRUTE_MAX_CELLS``. The caps are sized so that exactly three
shapes fall outside: the 16 385-row histogram layout, the K = 520 histogram
layout and the 600 000-row partition. Those are checked through the oracle's
invariants instead (and the histograms also against ``np.add.at``).
"""

import math

import numpy as np
import pytest
import torch

from tests import op_cases as oc
from tests.tree_oracle import KEYS, brute_splits
from xgboost_ray_amd.ops import cpu as cpu_ops

BRUTE_MAX_ROWS = 8000
BRUTE_MAX_CELLS = 300_000

def _ids(cases):
    return [c["id"] for c in cases]


def _brutable_hist(c):
    return c["layout"] == "a"


# ---------------------------------------------------------------------------
# build_histogram
# ---------------------------------------------------------------------------
def _brute_hist(c):
    F, nb = c["F"], c["n_bins"]
    bins = c["bins_flat"].tolist()
    gq = c["gq"].tolist()
    ridx = c["ridx"].tolist()
    K = len(c["starts"])
    flat = [0] * (K * F * nb * 2)
    for k, (s, cnt) in enumerate(zip(c["starts"].tolist(),
                                     c["counts"].tolist())):
        for pos in range(s, s + cnt):
            r = ridx[pos]
            g, h = gq[r]
            row = bins[r]
            for f in range(F):
                b = row[f]
                if b != 255:
                    at = ((k * F + f) * nb + b) * 2
                    flat[at] += g
                    flat[at + 1] += h
    return torch.tensor(flat, dtype=torch.int64).view(K, F, nb, 2)


def _addat_hist(c):
    F, nb, K = c["F"], c["n_bins"], len(c["starts"])
    bins, gq, ridx = (c[k].numpy() for k in ("bins_flat", "gq", "ridx"))
    out = np.zeros((K, F, nb, 2), np.int64)
    for k, (s, cnt) in enumerate(zip(c["starts"].tolist(),
                                     c["counts"].tolist())):
        rows = ridx[s:s + cnt]
        for f in range(F):
            keep = bins[rows, f] != 255
            np.add.at(out[k, f], bins[rows, f][keep],
                      gq[rows][keep].astype(np.int64))
    return torch.from_numpy(out)


@pytest.mark.parametrize("c", oc.hist_cases(), ids=_ids(oc.hist_cases()))
def test_build_histogram_oracle(c):
    rows = int(c["counts"].sum())
    assert _brutable_hist(c) == (rows <= BRUTE_MAX_ROWS)
    ref = oc.oracle_hist(c)
    if _brutable_hist(c):
        want = _brute_hist(c)
    else:
        want = _addat_hist(c)
        # invariant: column sums == segment sums of the non-missing rows
        bins, gq, ridx = c["bins_flat"].long(), c["gq"].long(), c["ridx"].long()
        for k, (s, cnt) in enumerate(zip(c["starts"].tolist(),
                                         c["counts"].tolist())):
            r = ridx[s:s + cnt]
            keep = (bins[r] != 255).long()           # [cnt, F]
            seg = keep.t() @ gq[r]                   # [F, 2]
            assert torch.equal(ref[k].sum(1), seg), (c["id"], k)
    assert ref.dtype == torch.int64 and torch.equal(ref, want)
    # pregathered gradients (poison outside the segments) give the same
    pre = cpu_ops.build_histogram(c["bins"], c["gseg"], c["ridx"], c["starts"],
                                  c["counts"], c["n_bins"], pregathered=True)
    assert torch.equal(pre, want)
    # the unpadded byte layout too
    flat = cpu_ops.build_histogram(c["bins_flat"], c["gq"], c["ridx"],
                                   c["starts"], c["counts"], c["n_bins"])
    assert torch.equal(flat, want)
    # f_range composition into one out= buffer
    if c["F"] > 16:
        out = torch.zeros_like(want)
        for lo in range(0, c["F"], 16):
            got = oc.oracle_hist(c, f_range=(lo, min(lo + 16, c["F"])), out=out)
            assert got is out
        assert torch.equal(out, want)


# ---------------------------------------------------------------------------
# find_splits
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", oc.split_cases(), ids=_ids(oc.split_cases()))
def test_find_splits_oracle(c):
    assert c["K"] * c["F"] * c["B"] <= BRUTE_MAX_CELLS
    ref, want = oc.oracle_splits(c), brute_splits(c)
    for key in KEYS:
        assert ref[key].dtype == want[key].dtype, key
        np.testing.assert_array_equal(ref[key], want[key], err_msg=key)
    if c["edge"] == "no_valid_split" or c["allowed"] is not None:
        k = 0  # nothing valid / every feature disallowed: the sentinel
        assert ref["gain"][k] == -1.0 and ref["feature"][k] == -1
        assert not (ref["bin"][k] or ref["default_left"][k]
                    or ref["left_g"][k] or ref["left_h"][k])
    if c["edge"] == "no_missing":
        assert (ref["default_left"] == 1).all()
    if c["edge"] == "dup_feature":
        assert (ref["feature"] == 0).all()
    if c["edge"] == "empty_bins":
        assert (ref["bin"] % 3 == 0).all()


def test_split_edge_counts():
    """Each named edge is genuine in every node of its cases."""
    for edge in oc.SPLIT_EDGES:
        cs = [c for c in oc.split_cases() if c["edge"] == edge]
        assert len(cs) >= 3 and all(c["n_tied"] == c["K"] for c in cs)


# ---------------------------------------------------------------------------
# partition_rows
# ---------------------------------------------------------------------------
def _brute_partition(c, sel):
    bins = c["bins"].tolist()
    ridx, gseg = c["ridx"].tolist(), c["gseg"].tolist()
    out, gout, lcs = list(ridx), [list(x) for x in gseg], []
    for k in sel:
        s, cnt = int(c["starts"][k]), int(c["counts"][k])
        f, sb = int(c["split_feat"][k]), int(c["split_bin"][k])
        dl = int(c["default_left"][k])
        left, right = [], []
        for pos in range(s, s + cnt):
            b = bins[ridx[pos]][f]
            go_left = bool(dl) if b == 255 else b <= sb
            (left if go_left else right).append(pos)
        for j, pos in enumerate(left + right):
            out[s + j], gout[s + j] = ridx[pos], gseg[pos]
        lcs.append(len(left))
    return (torch.tensor(out, dtype=torch.int32), lcs,
            torch.tensor(gout, dtype=torch.int32))


_PART = oc.partition_cases() + oc.packed_cases()


@pytest.mark.parametrize("c", _PART, ids=_ids(_PART))
def test_partition_rows_oracle(c):
    sel = list(range(c["K"]))
    if "packed" in c:  # only finite gain > 0 with feature >= 0 may move
        sel = np.nonzero(oc.packed_ok(c["packed"]))[0].tolist()
    rows = int(c["counts"].sum())
    assert (rows <= BRUTE_MAX_ROWS) == (rows != 600_000)
    r, lc, g = oc.oracle_partition(c, sel)
    r2, lc2, _ = oc.oracle_partition(c, sel, with_gseg=False)
    assert torch.equal(r, r2) and torch.equal(lc, lc2)
    if rows <= BRUTE_MAX_ROWS:
        wr, wlc, wg = _brute_partition(c, sel)
        assert torch.equal(r, wr) and torch.equal(g, wg)
        assert lc.tolist() == wlc
        return
    # invariants: a stable permutation with the reported left count
    bins = c["bins"]
    for j, k in enumerate(sel):
        s, cnt = int(c["starts"][k]), int(c["counts"][k])
        f, sb = int(c["split_feat"][k]), int(c["split_bin"][k])
        src, dst = c["ridx"][s:s + cnt].long(), r[s:s + cnt].long()
        col = bins[:, f]
        goes_left = torch.where(col == 255,
                                torch.tensor(bool(c["default_left"][k])),
                                col <= sb)
        nl = int(lc[j])
        assert nl == int(goes_left[src].sum())
        assert goes_left[dst[:nl]].all() and not goes_left[dst[nl:]].any()
        # stable: each side keeps the source order
        where = torch.empty(c["n"], dtype=torch.int64)
        where[src] = torch.arange(cnt)
        assert (where[dst[:nl]].diff() > 0).all()
        assert (where[dst[nl:]].diff() > 0).all()
        assert torch.equal(dst.sort().values, src.sort().values)
        assert torch.equal(g[s:s + cnt], c["gseg"][s:s + cnt][where[dst]])
    untouched = torch.ones(c["n"], dtype=torch.bool)
    for k in sel:
        s, cnt = int(c["starts"][k]), int(c["counts"][k])
        untouched[s:s + cnt] = False
    assert torch.equal(r[untouched], c["ridx"][untouched])


# ---------------------------------------------------------------------------
# update_margins, bin_matrix, quantize_gpair
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("c", oc.margin_cases(), ids=_ids(oc.margin_cases()))
def test_update_margins_oracle(c):
    want = c["margin"].numpy().copy()
    for k in range(len(c["starts"])):
        src = c["ridx_b"] if int(c["parity"][k]) else c["ridx_a"]
        s, cnt = int(c["starts"][k]), int(c["counts"][k])
        for pos in range(s, s + cnt):
            r = int(src[pos])
            want[r] = np.float32(want[r]) + np.float32(c["leaf_values"][k])
    np.testing.assert_array_equal(oc.oracle_margins(c).numpy(), want)


@pytest.mark.parametrize("c", oc.bin_matrix_cases(),
                         ids=_ids(oc.bin_matrix_cases()))
def test_bin_matrix_oracle(c):
    v, cuts, ptr = (c[k].numpy() for k in ("values", "cuts_flat", "cut_ptr"))
    want = np.empty(v.shape, np.uint8)
    for f in range(v.shape[1]):
        cf = cuts[ptr[f]:ptr[f + 1]]
        for i in range(v.shape[0]):
            x = v[i, f]
            if math.isnan(x):
                want[i, f] = 255
            elif len(cf) == 0:
                want[i, f] = 0
            else:  # linear count of cuts <= x, clamped to the last bin
                want[i, f] = min(int((cf <= x).sum()), len(cf) - 1)
    np.testing.assert_array_equal(oc.oracle_bins(c).numpy(), want)


@pytest.mark.parametrize("c", oc.quantize_cases(),
                         ids=_ids(oc.quantize_cases()))
def test_quantize_gpair_oracle(c):
    # Python's round() on a float is round-half-to-even, like llrint
    want = [[round(float(g) * c["scale_g"]), round(float(h) * c["scale_h"])]
            for g, h in c["gpair"].tolist()]
    got = oc.oracle_quantize(c)
    assert got.dtype == torch.int32 and got.tolist() == want
    if c["id"] == "zero-g-column":
        assert math.isfinite(c["scale_g"]) and not got[:, 0].any()
        assert got[:, 1].abs().max() == 2**30
    elif c["scale_g"] == 1.0:
        assert got[:5, 0].tolist() == [-128, -126, -126, -124, -124]
        assert got[5].tolist() == [2**30, -(2**30)]
