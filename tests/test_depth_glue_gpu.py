"""The fused per-depth glue (``RXGB_FUSED_GLUE``) against the composition
it replaces: the sibling histogram derived inside the split scan, the
per-node reduce and the partition plan as one kernel, the partition without
its zero fills and with one pull, the shuffle-scan chunk prefix, and the
engine with the switch on against off.

Everything here is integer work or a selection among given values, so every
comparison is exact (``assert_array_equal``); no tolerance appears anywhere.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PART_CHUNK = 2048


def _gpu_ops():
    from xgboost_ray_amd.ops import gpu as gpu_ops

    return gpu_ops


def _eq(got, want, msg=""):
    np.testing.assert_array_equal(
        got.cpu().numpy() if torch.is_tensor(got) else got,
        want.cpu().numpy() if torch.is_tensor(want) else want,
        err_msg=msg,
    )


def _padded_dev(b):
    """Padded 16-byte-stride layout on the device, pad bytes 255."""
    n, F = b.shape
    full = torch.full((n, (F + 15) // 16 * 16), 255, dtype=torch.uint8,
                      device="cuda")
    full[:, :F] = b.cuda()
    return full[:, :F]


# ---------------------------------------------------------------------------
# 1. sibling histogram derived inside find_splits
# ---------------------------------------------------------------------------
# (slots of prev_hist, K_built, pslots, spos)
DERIVE_SHAPES = {
    "built2_nd2": (4, 2, [3, 1], [0, 1]),   # parent slots out of order
    "built1_nd1": (2, 1, [1], [0]),
    "nd0": (2, 3, [], []),
}


def _rand_i64(rng, shape, lo, hi):
    return torch.from_numpy(rng.randint(lo, hi, size=shape, dtype=np.int64))


def _derive_inputs(F, B, shape):
    P, K_built, pslots, spos = DERIVE_SHAPES[shape]
    nd = len(pslots)
    K = K_built + nd
    rng = np.random.RandomState(1000 * F + B + 7 * K)
    # g anywhere in +-2^45; h of a built row in [0, 2^44) and the parent's
    # h above its child's, so a derived h is a valid (non-negative) sum
    hist = torch.empty((K, F, B, 2), dtype=torch.int64)
    hist[..., 0] = _rand_i64(rng, (K, F, B), -2**45, 2**45)
    hist[..., 1] = _rand_i64(rng, (K, F, B), 0, 2**44)
    hist[K_built:] = 7  # stale contents the derivation must overwrite
    prev = torch.empty((P, F, B, 2), dtype=torch.int64)
    prev[..., 0] = _rand_i64(rng, (P, F, B), -2**45, 2**45)
    prev[..., 1] = _rand_i64(rng, (P, F, B), 0, 2**44)
    ps = torch.tensor(pslots, dtype=torch.int64)
    sp = torch.tensor(spos, dtype=torch.int64)
    if nd:
        prev[ps, ..., 1] += hist[sp, ..., 1]
    composed = hist.clone()
    if nd:
        composed[K_built:] = prev.index_select(0, ps) - hist.index_select(0, sp)
        assert (composed[K_built:, ..., 0].sum(dim=2) < 0).any()
        assert composed.abs().max() < 2**46
    feat_bins = torch.full((F,), B, dtype=torch.int32)
    feat_bins[F // 2] = B // 2  # bins past nb hold mass and are still derived
    # node sums: feature 0's total plus some missing-value mass
    parent_g = composed[:, 0, :, 0].sum(dim=1) + _rand_i64(rng, (K,), -2**40, 2**40)
    parent_h = composed[:, 0, :, 1].sum(dim=1) + _rand_i64(rng, (K,), 0, 2**40)
    return dict(hist=hist, prev=prev, pslots=ps, spos=sp, composed=composed,
                feat_bins=feat_bins, parent_g=parent_g, parent_h=parent_h,
                K=K, K_built=K_built, nd=nd)


@pytest.mark.parametrize("with_allowed", [False, True],
                         ids=["ungated", "allowed_mask"])
@pytest.mark.parametrize("shape", sorted(DERIVE_SHAPES))
@pytest.mark.parametrize("FB", [(3, 256), (17, 256), (5, 64)],
                         ids=["F3_B256", "F17_B256", "F5_B64"])
def test_derive_in_scan(FB, shape, with_allowed):
    gpu = _gpu_ops()
    F, B = FB
    c = _derive_inputs(F, B, shape)
    K, K_built = c["K"], c["K_built"]
    allowed = None
    if with_allowed:
        allowed = torch.ones((K, F), dtype=torch.uint8)
        allowed[K - 1, F - 1] = 0  # a derived (node, feature) when nd > 0
        allowed[0, 0] = 0
    scale = float(2**30)
    args = (c["parent_g"].cuda(), c["parent_h"].cuda(), c["feat_bins"].cuda(),
            scale, scale, 1.0, 0.0, 0.0, 1.0)
    want_packed = gpu.find_splits(c["composed"].cuda(), *args,
                                  allowed=allowed, pull=False)
    hist = c["hist"].cuda()
    got_packed = gpu.find_splits(
        hist, *args, allowed=allowed, pull=False, prev_hist=c["prev"].cuda(),
        pslots=c["pslots"].cuda(), spos=c["spos"].cuda())
    _eq(hist[K_built:], c["composed"][K_built:], "derived rows of hist")
    _eq(hist[:K_built], c["hist"][:K_built], "built rows must stay")
    _eq(got_packed, want_packed, "packed splits")
    # some node must actually split, or the scan comparison says nothing
    assert (want_packed[:, 1] >= 0).any()
    # the pulled form and the unreduced form see the same derived values
    hist2 = c["hist"].cuda()
    best = gpu.find_splits(
        hist2, *args, allowed=allowed, prev_hist=c["prev"].cuda(),
        pslots=c["pslots"].cuda(), spos=c["spos"].cuda())
    _eq(best["feature"], want_packed[:, 1].cpu().numpy().astype(np.int32))
    _eq(best["left_g"], want_packed[:, 4])
    _eq(hist2, c["composed"], "derived rows, pull=True")


# ---------------------------------------------------------------------------
# 2. reduce + plan in one kernel against the two kernels
# ---------------------------------------------------------------------------
GAIN_POOL = np.array(
    [-1.0, -1.0, 0.5, 0.5, 0.5, 1.25, 1.25, 2.0, 0.0, -0.0, np.nan, np.inf,
     np.inf, 1e-3, -0.25, 3.5], np.float64)


def _kf_inputs(K, F, mode):
    rng = np.random.RandomState(31 * K + F + (0 if mode == "mixed" else 5))
    if mode == "mixed":
        gain = rng.choice(GAIN_POOL, size=(K, F))
        gain[rng.rand(K) < 0.15] = -1.0          # nodes with no candidate
        if K > 2:
            gain[2] = 1.25                       # one value everywhere
        if K > 3:
            gain[3] = np.nan
    else:
        # nothing splits: no gain above zero
        gain = rng.choice(np.array([-1.0, 0.0, -0.0, np.nan, -0.25]),
                          size=(K, F))
    dl = rng.randint(0, 2, size=(K, F)).astype(np.uint8)
    if mode == "mixed" and K > 4:
        dl[4] = 0
    kf = (
        torch.from_numpy(gain.reshape(-1)),
        torch.from_numpy(rng.randint(0, 255, K * F).astype(np.int32)),
        torch.from_numpy(dl.reshape(-1)),
        _rand_i64(rng, (K * F,), -2**45, 2**45),
        _rand_i64(rng, (K * F,), 0, 2**45),
    )
    counts = rng.choice(np.array([0, 1, 2047, 2048, 2049, 5000, 70000]), K)
    counts = counts.astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    return (tuple(t.cuda() for t in kf), torch.from_numpy(starts).cuda(),
            torch.from_numpy(counts).cuda())


@pytest.mark.parametrize("mode", ["mixed", "nosplit"])
@pytest.mark.parametrize("F", [1, 28, 65])
@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 1024, 1025])
def test_reduce_plan_matches_two_kernels(K, F, mode):
    gpu = _gpu_ops()
    kf, starts, counts = _kf_inputs(K, F, mode)
    want = gpu.reduce_plan(kf, starts, counts, fused=False)
    got = gpu.reduce_plan(kf, starts, counts, fused=True)
    torch.cuda.synchronize()
    n_split = int(want[2][0])
    if mode == "nosplit":
        assert n_split == 0
    elif K >= 63:
        assert 0 < n_split < K
    _eq(got[0], want[0], "packed")
    _eq(got[2], want[2], "scalars")
    _eq(got[1][: 6 * n_split + 1], want[1][: 6 * n_split + 1], "meta")


# ---------------------------------------------------------------------------
# 3/4. partition without fills, one pull
# ---------------------------------------------------------------------------
def _packed_rows(feat, sbin, dl, splits):
    one = int(np.float32(1.0).view(np.int32))
    neg = int(np.float32(-1.0).view(np.int32))
    rows = [[one if s else neg, f if s else -1, b if s else 0,
             d if s else 0, 11 * (i + 1) if s else 0, 13 * (i + 1) if s else 0]
            for i, (f, b, d, s) in enumerate(zip(feat, sbin, dl, splits))]
    return torch.tensor(rows, dtype=torch.int64)


def _kf_from_packed(packed, F):
    """(node, feature) scan arrays whose reduce gives exactly ``packed``."""
    K = packed.shape[0]
    gain = np.full((K, F), -1.0)
    kbin = np.zeros((K, F), np.int32)
    dl = np.zeros((K, F), np.uint8)
    lg = np.zeros((K, F), np.int64)
    lh = np.zeros((K, F), np.int64)
    for k, (gb, f, b, d, g, h) in enumerate(packed.tolist()):
        if f >= 0:
            gain[k, f] = float(np.int32(gb).view(np.float32))
            kbin[k, f], dl[k, f], lg[k, f], lh[k, f] = b, d, g, h
    return tuple(torch.from_numpy(a.reshape(-1)).cuda()
                 for a in (gain, kbin, dl, lg, lh))


PART_CALLS = (
    # sizes on the PART_CHUNK edges; (feat, bin, dl, splits)
    dict(sizes=[1, 2048, 2049, 5000, 4096], feat=[0, 3, 1, 2, 3],
         sbin=[100, 0, 254, 128, 17], dl=[1, 0, 1, 0, 1],
         splits=[True] * 5),
    dict(sizes=[2049, 5000, 1], feat=[2, 1, 0], sbin=[64, 200, 3],
         dl=[0, 1, 0], splits=[True, False, True]),
)


def _run_partition_calls(how):
    """Both calls back to back, in one process, through one route."""
    gpu = _gpu_ops()
    outs = []
    F = 4
    for ci, call in enumerate(PART_CALLS):
        sizes = np.asarray(call["sizes"], np.int64)
        n, K = int(sizes.sum()), sizes.size
        rng = np.random.RandomState(50 + ci)
        b = rng.randint(0, 255, size=(n, F)).astype(np.uint8)
        b[rng.rand(n, F) < 0.1] = 255
        bins = _padded_dev(torch.from_numpy(b))
        ridx = torch.from_numpy(rng.permutation(n).astype(np.int32)).cuda()
        gseg = torch.from_numpy(
            rng.randint(-2**30, 2**30, size=(n, 2)).astype(np.int32)).cuda()
        starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        packed = _packed_rows(call["feat"], call["sbin"], call["dl"],
                              call["splits"])
        dest = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        chunk_bound = (n + PART_CHUNK - 1) // PART_CHUNK + K
        common = (bins, ridx, torch.from_numpy(starts).cuda(),
                  torch.from_numpy(sizes).cuda())
        if how == "kf":
            r, g, pull, ev = gpu.partition_rows_from_kf(
                *common, _kf_from_packed(packed, F), gseg, None, chunk_bound,
                ridx_dest=dest)
        else:
            r, g, pull, ev = gpu.partition_rows_from_packed(
                *common, packed.cuda(), gseg, None, chunk_bound,
                ridx_dest=dest, fused_glue=(how == "fused"))
        ev.synchronize()
        arr = pull[: 7 * K].numpy().copy()
        torch.cuda.synchronize()
        segs = [(int(s), int(c)) for s, c, ok in
                zip(starts, sizes, call["splits"]) if ok]
        outs.append(dict(ridx=r.cpu().numpy(), gseg=g.cpu().numpy(),
                         pull=arr, segs=segs, packed=packed.numpy(), K=K))
    return outs


_PART_REF = {}


def _partition_ref():
    if not _PART_REF:
        _PART_REF["legacy"] = _run_partition_calls("legacy")
    return _PART_REF["legacy"]


@pytest.mark.parametrize("how", ["fused", "kf"])
def test_partition_without_fills(how):
    want = _partition_ref()
    got = _run_partition_calls(how)
    for ci, (g, w) in enumerate(zip(got, want)):
        K = w["K"]
        np.testing.assert_array_equal(g["ridx"], w["ridx"], f"call {ci} ridx")
        for s, c in w["segs"]:  # gseg is defined on the split segments only
            np.testing.assert_array_equal(g["gseg"][s:s + c],
                                          w["gseg"][s:s + c],
                                          f"call {ci} gseg at {s}")
        np.testing.assert_array_equal(g["pull"], w["pull"], f"call {ci} pull")
        np.testing.assert_array_equal(g["pull"][: 6 * K],
                                      w["packed"].reshape(-1))
        n_split = len(w["segs"])
        assert (g["pull"][6 * K + n_split:] == 0).all()
        assert (w["ridx"] != -7).sum() == sum(c for _, c in w["segs"])


# ---------------------------------------------------------------------------
# 5. shuffle-scan chunk prefix
# ---------------------------------------------------------------------------
def test_prefix_against_cumsum():
    gpu = _gpu_ops()
    chunks = np.array([1, 255, 256, 257, 600], np.int64)
    sizes = chunks * PART_CHUNK - 37  # last chunk of every node partial
    K, n = chunks.size, int(sizes.sum())
    rng = np.random.RandomState(3)
    b = rng.randint(0, 255, size=(n, 1)).astype(np.uint8)
    b[rng.rand(n, 1) < 0.1] = 255
    sbin = [10, 100, 128, 200, 250]
    dl = [1, 0, 1, 0, 1]
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    packed = _packed_rows([0] * K, sbin, dl, [True] * K)
    ridx = torch.arange(n, dtype=torch.int32, device="cuda")
    empty_g = torch.zeros((0, 2), dtype=torch.int32, device="cuda")
    empty_b = torch.zeros(0, dtype=torch.uint8, device="cuda")
    total_chunks = int(chunks.sum())
    # host reference: per-chunk left counts, exclusive cumsum within a node
    want_before, want_total = [], []
    for k in range(K):
        col = b[starts[k]: starts[k] + sizes[k], 0]
        left = np.where(col == 255, dl[k] != 0, col <= sbin[k])
        pad = np.zeros(chunks[k] * PART_CHUNK, np.int64)
        pad[: left.size] = left
        per_chunk = torch.from_numpy(pad.reshape(-1, PART_CHUNK).sum(axis=1))
        incl = torch.cumsum(per_chunk, dim=0)
        want_before.append(incl - per_chunk)
        want_total.append(int(incl[-1]))
    want_before = torch.cat(want_before)
    for fused in (True, False):
        out = gpu._load().partition_rows_from_packed(
            _padded_dev(torch.from_numpy(b)), ridx,
            torch.from_numpy(starts).cuda(), torch.from_numpy(sizes).cuda(),
            packed.cuda(), empty_g, empty_b, total_chunks + K,
            torch.empty_like(ridx), fused)
        torch.cuda.synchronize()
        _eq(out[5][:total_chunks], want_before, f"left_before fused={fused}")
        _eq(out[6], torch.tensor(want_total), f"left totals fused={fused}")


# ---------------------------------------------------------------------------
# engine: RXGB_FUSED_GLUE unset against =0 in one process
# ---------------------------------------------------------------------------
TREE_FIELDS = ("feat", "thr", "left", "default_left", "value", "gain",
               "cover", "parent")

ENGINE_VARIANTS = {
    "plain": ({}, {}),
    "constrained": (
        {"monotone_constraints": [1, -1] + [0] * 18,
         "interaction_constraints": [[0, 1, 2, 3, 4, 5, 6, 7, 8, 9],
                                     [8, 9, 10, 11, 12, 13, 14, 15, 16, 17,
                                      18, 19]],
         "colsample_bynode": 0.5}, {}),
    "two_sync": ({}, {"RXGB_ONE_SYNC": "0"}),
    "legacy_finish": ({}, {"RXGB_ROW_FINISH": "0"}),
    "depth_step": ({}, {"RXGB_DEPTH_STEP": "1"}),
}

_ENGINE_DM = {}


def _engine_dm():
    if not _ENGINE_DM:
        from xgboost_ray_amd.engine.quantile import BinnedMatrix

        rng = np.random.RandomState(0)
        n, F = 20000, 20  # F = 20: two 16-feature histogram blocks
        X = rng.randn(n, F).astype(np.float32)
        y = ((X[:, 0] - 0.5 * X[:, 1] + 0.4 * X[:, 11]
              + 0.3 * rng.randn(n)) > 0).astype(np.float32)
        X[rng.rand(n, F) < 0.1] = np.nan
        _ENGINE_DM["dm"] = BinnedMatrix.build(
            torch.from_numpy(X).cuda(), label=torch.from_numpy(y).cuda(),
            max_bin=256)
    return _ENGINE_DM["dm"]


def _run_engine(dm, params, rounds):
    from xgboost_ray_amd.engine.trainer import BoostingEngine

    eng = BoostingEngine(dict(params, tree_method="gpu_hist", eta=0.3), dm)
    trees = []
    for _ in range(rounds):
        trees += eng.update()
    torch.cuda.synchronize()
    return trees, eng.margin.cpu().numpy()


@pytest.mark.parametrize("variant", sorted(ENGINE_VARIANTS))
def test_engine_fused_glue_matches_legacy(variant, monkeypatch):
    extra, env = ENGINE_VARIANTS[variant]
    params = dict({"objective": "binary:logistic", "max_depth": 5}, **extra)
    dm = _engine_dm()
    for k in ("RXGB_ONE_SYNC", "RXGB_ROW_FINISH", "RXGB_DEPTH_STEP",
              "RXGB_FUSED_GLUE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    trees_on, margin_on = _run_engine(dm, params, 3)
    monkeypatch.setenv("RXGB_FUSED_GLUE", "0")
    trees_off, margin_off = _run_engine(dm, params, 3)
    assert len(trees_on) == len(trees_off) == 3
    for t_on, t_off in zip(trees_on, trees_off):
        for f in TREE_FIELDS:
            np.testing.assert_array_equal(
                getattr(t_on, f), getattr(t_off, f), err_msg=f)
    np.testing.assert_array_equal(margin_on, margin_off)
    assert max(t.feat.size for t in trees_on) > 15  # the trees did grow
