"""The whole-tree enqueue (``RXGB_TREE_ENQUEUE``): the device kernel that
plans depth d+1 from depth d's splits against a numpy transcription of the
trainer's host bookkeeping, the device-limit forms of the histogram, scan
and reduce+plan kernels against their exact-argument forms, and the engine
with the switch on against off.

Everything here is integer work or a selection among given values, so every
comparison is exact (``assert_array_equal``); no tolerance appears anywhere.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS_PER_WG = 16384  # the XCD histogram's default rows per workgroup
ONE = int(np.float32(1.0).view(np.int32))
NEG = int(np.float32(-1.0).view(np.int32))
ZERO = int(np.float32(0.0).view(np.int32))


def _ext():
    from xgboost_ray_amd.ops import gpu as gpu_ops

    return gpu_ops._load()


def _gpu_ops():
    from xgboost_ray_amd.ops import gpu as gpu_ops

    return gpu_ops


def _dev(a, size=None):
    """int64 device vector; ``size`` pads it with zeros to a bound-sized
    buffer (the limit forms size their metadata for the bound)."""
    a = np.ascontiguousarray(a, dtype=np.int64)
    if size is not None and a.ndim == 1 and a.size < size:
        a = np.concatenate([a, np.zeros(size - a.size, np.int64)])
    return torch.from_numpy(a).cuda()


def _eq(got, want, msg=""):
    np.testing.assert_array_equal(
        got.cpu().numpy() if torch.is_tensor(got) else got,
        want.cpu().numpy() if torch.is_tensor(want) else want,
        err_msg=msg,
    )


# ---------------------------------------------------------------------------
# 1. plan_next_depth_kernel against the trainer's host code
# ---------------------------------------------------------------------------
def _host_plan_next(packed, sumg_ord, sumh_ord, start_ord, count_ord,
                    lc_full, rows_per_wg):
    """What trainer.py computes between one depth's pull and the next
    depth's launches: the split predicate, the children after
    ``_tick("partition")``, the "build order" pairing, the scan meta and
    the histogram meta. Returns (dmeta, hmeta, limits) as int64 vectors."""
    gain = packed[:, 0].astype(np.int32).view(np.float32)
    bfeat = packed[:, 1].astype(np.int32)
    blg, blh = packed[:, 4], packed[:, 5]
    splits_ok = (gain > 0) & (bfeat >= 0) & np.isfinite(gain)
    okf = np.nonzero(splits_ok)[0]
    n_split = int(okf.size)
    if n_split == 0:
        return (np.zeros(0, np.int64), np.zeros(1, np.int64),
                np.zeros(3, np.int64))
    lc = lc_full[:n_split].astype(np.int64)
    l_start = start_ord[okf]
    l_sumg = blg[okf]
    l_sumh = blh[okf]
    r_start = l_start + lc
    r_count = count_ord[okf] - lc
    r_sumg = sumg_ord[okf] - l_sumg
    r_sumh = sumh_ord[okf] - l_sumh
    n2 = 2 * n_split

    def pair(a, b):
        out = np.empty(n2, np.int64)
        out[0::2] = a
        out[1::2] = b
        return out

    fr_start = pair(l_start, r_start)
    fr_count = pair(lc, r_count)
    fr_sumg = pair(l_sumg, r_sumg)
    fr_sumh = pair(l_sumh, r_sumh)
    fr_pslot = pair(okf, okf)
    # build order
    ia = np.arange(0, n2, 2)
    ib = ia + 1
    small_is_a = fr_sumh[ia] <= fr_sumh[ib]
    idx_small = np.where(small_is_a, ia, ib)
    idx_big = np.where(small_is_a, ib, ia)
    order_idx = np.concatenate([idx_small, idx_big])
    K = idx_small.size
    derive_pslot = fr_pslot[idx_big]
    derive_sib_pos = np.arange(K, dtype=np.int64)
    start_ord2 = fr_start[order_idx]
    count_ord2 = fr_count[order_idx]
    dmeta = np.concatenate([fr_sumg[order_idx], fr_sumh[order_idx],
                            start_ord2, count_ord2, derive_pslot,
                            derive_sib_pos])
    counts = count_ord2[:K]
    chunk_off = np.zeros(K + 1, np.int64)
    chunk_off[1:] = np.cumsum((counts + rows_per_wg - 1) // rows_per_wg)
    hmeta = np.concatenate([start_ord2[:K], counts, chunk_off])
    limits = np.array([K, 2 * K, chunk_off[-1]], np.int64)
    return dmeta, hmeta, limits


def _node(gbits, feat, count, lc, sumh, lh, sumg=0, lg=0):
    return dict(gbits=gbits, feat=feat, count=count, lc=lc, sumh=sumh, lh=lh,
                sumg=sumg, lg=lg)


def _frontier_case(name):
    R = ROWS_PER_WG
    if name == "KK1":
        return [_node(ONE, 3, 5000, 1234, 900, 300, sumg=-77, lg=-100)]
    if name == "KK6_nonsplit_between":
        return [
            _node(ONE, 0, 4000, 1000, 800, 500, sumg=40, lg=90),
            _node(ZERO, 2, 3000, 0, 600, 0),       # gain bits == 0
            _node(ONE, 5, 2000, 1999, 500, 100, sumg=-5, lg=-9),
            _node(ONE, -1, 1000, 0, 400, 0),       # feature -1
            _node(NEG, 1, 500, 0, 300, 0),         # gain -1
            _node(ONE, 27, 700, 350, 200, 150, sumg=11, lg=4),
        ]
    if name == "sumh_tie":
        # lh == sumh - lh: the left child must be built
        return [_node(ONE, 1, 3000, 1000, 800, 400, sumg=10, lg=7),
                _node(ONE, 2, 3000, 2000, 801, 400, sumg=10, lg=7)]
    if name == "lc_edges":
        # lc == 0 and lc == count, each once as the built and once as
        # the derived child
        return [_node(ONE, 0, 900, 0, 100, 10),
                _node(ONE, 0, 900, 0, 100, 90),
                _node(ONE, 0, 900, 900, 100, 10),
                _node(ONE, 0, 900, 900, 100, 90)]
    if name == "chunk_edges":
        # built child counts R, R + 1, 2R, 2R + 1, R - 1 and 0
        return [_node(ONE, 0, 3 * R, R, 100, 10),
                _node(ONE, 0, 3 * R, R + 1, 100, 10),
                _node(ONE, 0, 5 * R, 3 * R, 100, 90),      # right built: 2R
                _node(ONE, 0, 5 * R, 3 * R - 1, 100, 90),  # right: 2R + 1
                _node(ONE, 0, 2 * R, R - 1, 100, 10),
                _node(ONE, 0, 2 * R, 0, 100, 10)]
    if name == "KK1024":
        rng = np.random.RandomState(1024)
        nodes = []
        for i in range(1024):
            count = int(rng.choice([0, 1, 2, 100, R, R + 1, 3 * R + 5]))
            sumh = int(rng.randint(0, 2**40))
            split = rng.rand() < 0.8
            nodes.append(_node(
                ONE if split else int(rng.choice([ZERO, NEG])),
                int(rng.randint(0, 28)) if rng.rand() < 0.95 else -1,
                count, int(rng.randint(0, count + 1)), sumh,
                sumh // 2 if rng.rand() < 0.2 else int(rng.randint(0, sumh + 1)),
                sumg=int(rng.randint(-2**40, 2**40)),
                lg=int(rng.randint(-2**40, 2**40))))
        return nodes
    if name == "n_split0":
        return [_node(NEG, 0, 100, 0, 50, 0), _node(ZERO, 1, 200, 0, 60, 0),
                _node(ONE, -1, 300, 0, 70, 0)]
    raise KeyError(name)


@pytest.mark.parametrize("case", [
    "KK1", "KK6_nonsplit_between", "sumh_tie", "lc_edges", "chunk_edges",
    "KK1024", "n_split0"])
def test_plan_next_depth_matches_host(case):
    nodes = _frontier_case(case)
    KK = len(nodes)
    packed = np.array([[nd["gbits"], nd["feat"], 17, 1, nd["lg"], nd["lh"]]
                       for nd in nodes], np.int64)
    sumg = np.array([nd["sumg"] for nd in nodes], np.int64)
    sumh = np.array([nd["sumh"] for nd in nodes], np.int64)
    count = np.array([nd["count"] for nd in nodes], np.int64)
    start = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int64)
    gain = packed[:, 0].astype(np.int32).view(np.float32)
    ok = (gain > 0) & (packed[:, 1] >= 0)
    # the partition stores the left totals in compact split order and
    # zeroes the rest of the bound
    lc_full = np.zeros(KK, np.int64)
    lc_ok = np.array([nd["lc"] for nd, o in zip(nodes, ok) if o], np.int64)
    lc_full[: lc_ok.size] = lc_ok
    want_dm, want_hm, want_lim = _host_plan_next(
        packed, sumg, sumh, start, count, lc_full, ROWS_PER_WG)
    if case == "n_split0":
        assert want_lim[0] == 0
    elif case == "KK6_nonsplit_between":
        assert want_lim[0] == 3
    elif case == "sumh_tie":
        # the tie builds the left child: its count is lc
        assert want_hm[2] == 1000
    # the previous depth's scan meta: here every node counts as built
    dmeta = np.concatenate([sumg, sumh, start, count])
    limits = np.array([KK, KK, 0], np.int64)
    got_dm, got_hm, got_lim = _ext().plan_next_depth(
        _dev(packed), _dev(dmeta), _dev(limits), _dev(lc_full), ROWS_PER_WG)
    torch.cuda.synchronize()
    _eq(got_lim, want_lim, "limits")
    Kn = int(want_lim[0])
    _eq(got_dm[: 10 * Kn], want_dm, "scan meta")
    _eq(got_hm[: 3 * Kn + 1], want_hm, "histogram meta")
    # nothing past the next frontier's true size
    assert (got_dm[10 * Kn:] == -1).all()
    assert (got_hm[3 * Kn + 1:] == -1).all()


# ---------------------------------------------------------------------------
# 2. device-limit forms of the histogram, scan and reduce+plan kernels
# ---------------------------------------------------------------------------
_LIMIT_INPUTS = {}


def _limit_inputs():
    """3,000 rows x 28 features (two feature blocks, row stride 32): four
    parent segments, each cut in two children. Scan slots: the four left
    children are built, the four right ones derived."""
    if _LIMIT_INPUTS:
        return _LIMIT_INPUTS
    gpu = _gpu_ops()
    n, F, B = 3000, 28, 256
    rng = np.random.RandomState(11)
    b = rng.randint(0, 255, size=(n, F)).astype(np.uint8)
    b[rng.rand(n, F) < 0.05] = 255
    full = torch.full((n, 32), 255, dtype=torch.uint8, device="cuda")
    full[:, :F] = torch.from_numpy(b).cuda()
    bins = full[:, :F]
    assert bins.stride(0) == 32
    ridx = torch.from_numpy(rng.permutation(n).astype(np.int32)).cuda()
    gseg_np = np.stack([rng.randint(-2**20, 2**20, n),
                        rng.randint(1, 2**20, n)], axis=1).astype(np.int32)
    gseg = torch.from_numpy(gseg_np).cuda()
    psize = np.array([1000, 1, 1499, 500], np.int64)
    pstart = np.concatenate([[0], np.cumsum(psize)[:-1]])
    lsize = np.array([400, 0, 1000, 499], np.int64)
    starts8 = np.concatenate([pstart, pstart + lsize])     # built, derived
    counts8 = np.concatenate([lsize, psize - lsize])
    g64 = gseg_np.astype(np.int64)
    sums8 = np.array([g64[s:s + c].sum(axis=0)
                      for s, c in zip(starts8, counts8)], np.int64)
    prev = gpu.build_histogram(bins, gseg, ridx, torch.from_numpy(pstart),
                               torch.from_numpy(psize), B, pregathered=True)
    _LIMIT_INPUTS.update(
        n=n, F=F, B=B, bins=bins, ridx=ridx, gseg=gseg, starts8=starts8,
        counts8=counts8, sums8=sums8, prev=prev,
        feat_bins=torch.full((F,), B, dtype=torch.int32, device="cuda"))
    return _LIMIT_INPUTS


def _hist_meta(starts, counts):
    chunk_off = np.zeros(starts.size + 1, np.int64)
    chunk_off[1:] = np.cumsum((counts + ROWS_PER_WG - 1) // ROWS_PER_WG)
    return np.concatenate([starts, counts, chunk_off]), int(chunk_off[-1])


def test_histogram_limits_form():
    c = _limit_inputs()
    gpu, ext = _gpu_ops(), _ext()
    supported, rows = ext.tree_enqueue_config(c["bins"], c["B"])
    assert supported == 1 and rows == ROWS_PER_WG
    K = 8
    want = gpu.build_histogram(
        c["bins"], c["gseg"], c["ridx"], torch.from_numpy(c["starts8"]),
        torch.from_numpy(c["counts8"]), c["B"], pregathered=True)
    hmeta, chunks = _hist_meta(c["starts8"], c["counts8"])
    assert chunks == 7  # the empty node has no chunk
    got = torch.zeros((4 * K, c["F"], c["B"], 2), dtype=torch.int64,
                      device="cuda")
    ext.build_histogram_limits(
        c["bins"], c["gseg"], c["ridx"], _dev(hmeta, 3 * 4 * K + 1),
        _dev([K, 2 * K, chunks]), c["B"], got, 2 * chunks)
    torch.cuda.synchronize()
    assert int(want.abs().sum()) > 0
    _eq(got[:K], want, "histogram of the true nodes")
    assert not got[K:].any(), "rows past the true K were written"


def _scan_args(c):
    return (c["feat_bins"], float(2**20), float(2**20), 1.0, 0.0, 0.0, 1.0,
            torch.zeros(0, dtype=torch.int8, device="cuda"),
            torch.zeros((0, 2), dtype=torch.float64, device="cuda"),
            torch.zeros(0, dtype=torch.uint8, device="cuda"))


def _scan_both(c):
    """(kf exact, hist exact, kf limits, hist limits, dmeta, limits)."""
    gpu, ext = _gpu_ops(), _ext()
    KK, Kb, F, B = 8, 4, c["F"], c["B"]
    built = gpu.build_histogram(
        c["bins"], c["gseg"], c["ridx"], torch.from_numpy(c["starts8"][:Kb]),
        torch.from_numpy(c["counts8"][:Kb]), B, pregathered=True)
    pslots = np.array([0, 1, 2, 3], np.int64)
    spos = np.arange(Kb, dtype=np.int64)
    hist_a = torch.full((KK, F, B, 2), 7, dtype=torch.int64, device="cuda")
    hist_a[:Kb] = built
    kf_a = ext.find_splits_kf(
        hist_a, _dev(c["sums8"][:, 0]), _dev(c["sums8"][:, 1]),
        *_scan_args(c), c["prev"], _dev(pslots), _dev(spos))
    hist_b = torch.full((4 * KK, F, B, 2), 7, dtype=torch.int64,
                        device="cuda")
    hist_b[:Kb] = built
    dmeta = _dev(np.concatenate([c["sums8"][:, 0], c["sums8"][:, 1],
                                 c["starts8"], c["counts8"], pslots, spos]),
                 5 * 4 * KK)
    limits = _dev([Kb, KK, 0])
    empty = torch.zeros(0, dtype=torch.int64, device="cuda")
    kf_b = ext.find_splits_kf(
        hist_b, empty, empty, *_scan_args(c), c["prev"], None, None,
        limits, dmeta)
    torch.cuda.synchronize()
    return kf_a, hist_a, kf_b, hist_b, dmeta, limits


def test_scan_limits_form():
    c = _limit_inputs()
    KK, F = 8, c["F"]
    kf_a, hist_a, kf_b, hist_b, _, _ = _scan_both(c)
    assert (kf_a[0] > 0).any()  # some (node, feature) has a real candidate
    for a, b, name in zip(kf_a, kf_b, ("gain", "bin", "dl", "lg", "lh")):
        _eq(b[: KK * F], a, f"kf_{name}")
    _eq(hist_b[:KK], hist_a, "built and derived rows")
    assert (hist_b[KK:] == 7).all(), "rows past the true K were written"


def test_reduce_plan_limits_form():
    c = _limit_inputs()
    gpu, ext = _gpu_ops(), _ext()
    KK = 8
    kf_a, _, kf_b, _, dmeta, limits = _scan_both(c)
    want = gpu.reduce_plan(tuple(kf_a), _dev(c["starts8"]),
                           _dev(c["counts8"]), fused=True)
    packed, meta, scalars, pullbuf = ext.reduce_plan_limits(
        *kf_b, dmeta, limits, 4 * KK)
    torch.cuda.synchronize()
    n_split = int(want[2][0])
    assert 0 < n_split <= KK
    _eq(packed[:KK], want[0], "packed")
    _eq(scalars, want[2], "scalars")
    _eq(meta[: 6 * n_split + 1], want[1][: 6 * n_split + 1], "meta")
    # packed is the head of the pull record, on the bound's layout
    _eq(pullbuf[: 6 * KK], want[0].reshape(-1), "pull record")


# ---------------------------------------------------------------------------
# 3. engine: RXGB_TREE_ENQUEUE=1 against =0 in one process
# ---------------------------------------------------------------------------
TREE_FIELDS = ("feat", "thr", "left", "default_left", "value", "gain",
               "cover", "parent")
SWITCHES = ("RXGB_ONE_SYNC", "RXGB_ROW_FINISH", "RXGB_DEPTH_STEP",
            "RXGB_FUSED_GLUE", "RXGB_TREE_ENQUEUE")

_DMS = {}


def _dm(n, max_bin):
    key = (n, max_bin)
    if key not in _DMS:
        from xgboost_ray_amd.engine.quantile import BinnedMatrix

        rng = np.random.RandomState(n + max_bin)
        F = 28
        X = rng.randn(n, F).astype(np.float32)
        y = ((X[:, 0] - 0.5 * X[:, 1] + 0.4 * X[:, 17]
              + 0.3 * rng.randn(n)) > 0).astype(np.float32)
        X[rng.rand(n) < 0.05, 1] = np.nan
        X[rng.rand(n) < 0.05, 20] = np.nan
        _DMS[key] = BinnedMatrix.build(
            torch.from_numpy(X).cuda(), label=torch.from_numpy(y).cuda(),
            max_bin=max_bin)
    return _DMS[key]


def _run_engine(dm, params, rounds=3):
    from xgboost_ray_amd.engine.trainer import BoostingEngine

    eng = BoostingEngine(dict(params, tree_method="gpu_hist", eta=0.3), dm)
    trees, paths = [], set()
    for _ in range(rounds):
        trees += eng.update()
        paths.add(eng.last_tree_path)
    torch.cuda.synchronize()
    return trees, eng.margin.cpu().numpy(), paths


def _node_depths(tree):
    depth = np.zeros(tree.feat.size, np.int64)
    for i in range(1, tree.feat.size):  # a parent's id is below its child's
        depth[i] = depth[tree.parent[i]] + 1
    return depth


def _run_both(dm, params, monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("RXGB_TREE_ENQUEUE", "1")
    on = _run_engine(dm, params)
    monkeypatch.setenv("RXGB_TREE_ENQUEUE", "0")
    off = _run_engine(dm, params)
    assert off[2] == {"per_depth"}
    assert len(on[0]) == len(off[0]) == 3
    for t_on, t_off in zip(on[0], off[0]):
        for f in TREE_FIELDS:
            np.testing.assert_array_equal(
                getattr(t_on, f), getattr(t_off, f), err_msg=f)
    np.testing.assert_array_equal(on[1], off[1])
    return on, off


ENQUEUE_CASES = {
    "plain": (5000, 256, {}),
    "subsample_gamma": (5000, 256, {"subsample": 0.5, "gamma": 1.0}),
    "rows64": (64, 256, {}),
    "max_bin64": (5000, 64, {}),
}


@pytest.mark.parametrize("case", sorted(ENQUEUE_CASES))
def test_engine_tree_enqueue_matches_per_depth(case, monkeypatch):
    n, max_bin, extra = ENQUEUE_CASES[case]
    params = dict({"objective": "binary:logistic", "max_depth": 8}, **extra)
    on, off = _run_both(_dm(n, max_bin), params, monkeypatch)
    assert on[2] == {"enqueue"}
    depths = [_node_depths(t) for t in off[0]]
    if case == "subsample_gamma":
        # some node stops early: a non-root leaf above the last level
        assert any(((t.feat < 0) & (d > 0) & (d < 8)).any()
                   for t, d in zip(off[0], depths))
    elif case == "rows64":
        # the frontier empties early: the deeper launches are no-ops
        assert all(d.max() < 8 for d in depths)
    else:
        assert max(d.max() for d in depths) >= 6  # the trees did grow


FALLBACK_CASES = {
    "monotone": {"max_depth": 6,
                 "monotone_constraints": [1, -1] + [0] * 26},
    "depth11": {"max_depth": 11},
}


@pytest.mark.parametrize("case", sorted(FALLBACK_CASES))
def test_engine_tree_enqueue_falls_back(case, monkeypatch):
    params = dict({"objective": "binary:logistic"}, **FALLBACK_CASES[case])
    on, _ = _run_both(_dm(2000, 256), params, monkeypatch)
    assert on[2] == {"per_depth"}
