"""HIP kernels vs the CPU oracle on every kernel route and edge shape.

``tests/test_ops_gpu.py`` checks each op at one large point; this file runs
the small generated cases of ``tests/op_cases.py`` through every histogram
route, every split-scan parameter combination and every partition entry
point. All comparisons are exact (integer ops, and a split scan engineered
to be bitwise equal), so no tolerance appears anywhere. The oracle itself is
checked against brute force in ``tests/test_op_oracles.py``.
"""

import numpy as np
import pytest
import torch

from tests import op_cases as oc

pytestmark = pytest.mark.gpu

KEYS = ("gain", "feature", "bin", "default_left", "left_g", "left_h")

# every knob build_histogram reads per call; cleared so "default" is default
HIST_KNOBS = ("RXGB_HIST_FB", "RXGB_HIST_MULTIFB", "RXGB_HIST_MODE",
              "RXGB_HIST_XCD_ROWS", "RXGB_HIST_DIRECT_ROWS",
              "RXGB_HIST_MULTIFB_R", "RXGB_HIST_XCD_THREADS")


def _gpu_ops():
    from xgboost_ray_amd.ops import gpu as gpu_ops

    return gpu_ops


def _ids(cases):
    return [c["id"] for c in cases]


def _padded_dev(b):
    """Padded 16-byte-stride layout on the device (``.cuda()`` of a narrowed
    view would densify it)."""
    n, F = b.shape
    full = torch.full((n, (F + 15) // 16 * 16), 255, dtype=torch.uint8,
                      device="cuda")
    full[:, :F] = b.cuda()
    return full[:, :F]


_CACHE = {}


def _memo(c, key, fn):
    k = (c["id"], key)
    if k not in _CACHE:
        _CACHE[k] = fn()
    return _CACHE[k]


def _dev(c, key):
    if key == "bins":
        return _memo(c, "dev-bins", lambda: _padded_dev(c["bins"]))
    return _memo(c, "dev-" + key, lambda: c[key].cuda())


def _eq(got, want, msg):
    np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy(),
                                  err_msg=msg)


# ---------------------------------------------------------------------------
# histogram variant matrix
# ---------------------------------------------------------------------------
def _wide(c):
    return c["F"] > 16


def _any(c):
    return True


_MFB = {"RXGB_HIST_MODE": "multifb"}
HIST_ROUTES = {
    # route: (env, applies-to, bins layout)
    "default": ({}, _any, "bins"),                 # xcd<512> / kernel<16>
    "xcd-1024-threads": ({"RXGB_HIST_XCD_THREADS": "1024"}, _wide, "bins"),
    "xcd-512-rows": ({"RXGB_HIST_XCD_ROWS": "512"}, _wide, "bins"),
    "multifb-R4": (dict(_MFB, RXGB_HIST_MULTIFB_R="4"), _wide, "bins"),
    "multifb-R8": (dict(_MFB, RXGB_HIST_MULTIFB_R="8"), _wide, "bins"),
    "multifb-R16": (dict(_MFB, RXGB_HIST_MULTIFB_R="16"), _wide, "bins"),
    "multifb-R32": (dict(_MFB, RXGB_HIST_MULTIFB_R="32"), _wide, "bins"),
    "base": ({"RXGB_HIST_MODE": "base"}, _wide, "bins"),
    "fb8": ({"RXGB_HIST_FB": "8"}, _any, "bins"),  # kernel<8>
    # unpadded rows whose stride is no multiple of 16: kernel<0>
    "byte": ({}, lambda c: c["F"] % 16 != 0, "bins_flat"),
    "direct-default": ({"RXGB_HIST_DIRECT_ROWS": "512"}, _any, "bins"),
    "direct-base": ({"RXGB_HIST_DIRECT_ROWS": "512",
                     "RXGB_HIST_MODE": "base"}, _wide, "bins"),
}


def _set_hist_env(monkeypatch, env):
    for k in HIST_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _hist_gpu(c, layout, pregathered, **kw):
    gpu = _gpu_ops()
    grad = _dev(c, "gseg" if pregathered else "gq")
    return gpu.build_histogram(
        _dev(c, layout), grad, _dev(c, "ridx"), c["starts"], c["counts"],
        c["n_bins"], pregathered=pregathered, **kw)


@pytest.mark.parametrize("pregathered", [False, True],
                         ids=["gather", "pregathered"])
@pytest.mark.parametrize("route", list(HIST_ROUTES))
def test_build_histogram_route(route, pregathered, monkeypatch):
    env, applies, layout = HIST_ROUTES[route]
    _set_hist_env(monkeypatch, env)
    cases = [c for c in oc.hist_cases() if applies(c)]
    assert {c["layout"] for c in cases} == set("abc")
    assert {c["n_bins"] for c in cases} == {256, 255, 64, 37}
    for c in cases:
        if layout == "bins_flat":
            assert c["bins_flat"].stride(0) % 16 != 0
        ref = _memo(c, "hist-ref", lambda: oc.oracle_hist(c))
        out = _hist_gpu(c, layout, pregathered)
        _eq(out, ref, f"{route} {c['id']}")


@pytest.mark.parametrize("pregathered", [False, True],
                         ids=["gather", "pregathered"])
def test_build_histogram_f_range_composition(pregathered, monkeypatch):
    """16-aligned feature ranges accumulated into one ``out=`` buffer, vs
    the CPU oracle's single full build."""
    _set_hist_env(monkeypatch, {})
    cases = [c for c in oc.hist_cases() if c["F"] == 40]
    assert len(cases) == 4
    for c in cases:
        ref = _memo(c, "hist-ref", lambda: oc.oracle_hist(c))
        for ranges in (((0, 16), (16, 32), (32, 40)), ((0, 16), (16, 40)),
                       ((0, 32), (32, 40))):
            out = torch.zeros(ref.shape, dtype=torch.int64, device="cuda")
            for fr in ranges:
                got = _hist_gpu(c, "bins", pregathered, f_range=fr, out=out)
                assert got.data_ptr() == out.data_ptr()
            _eq(out, ref, f"{c['id']} {ranges}")


# ---------------------------------------------------------------------------
# split scan
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", oc.split_cases(), ids=_ids(oc.split_cases()))
def test_find_splits_case(c):
    gpu = _gpu_ops()
    ref = oc.oracle_splits(c)
    args = (c["hist"].cuda(), c["parent_g"].cuda(), c["parent_h"].cuda(),
            c["feat_bins"].cuda(), c["scale_g"], c["scale_h"],
            c["reg_lambda"], c["reg_alpha"], c["gamma"], c["mcw"])
    kw = dict(monotone=c["monotone"], bounds=c["bounds"],
              allowed=c["allowed"])
    out = gpu.find_splits(*args, **kw)
    for key in KEYS:
        assert out[key].dtype == ref[key].dtype, key
        np.testing.assert_array_equal(out[key], ref[key], err_msg=key)
    # the device-resident packed form, decoded the way the trainer does
    packed = gpu.find_splits(*args, pull=False, **kw)
    assert packed.is_cuda and tuple(packed.shape) == (c["K"], 6)
    pk = packed.cpu().numpy()
    dec = {
        "gain": pk[:, 0].astype(np.int32).view(np.float32).copy(),
        "feature": pk[:, 1].astype(np.int32),
        "bin": pk[:, 2].astype(np.int32),
        "default_left": pk[:, 3].astype(np.uint8),
        "left_g": pk[:, 4].copy(),
        "left_h": pk[:, 5].copy(),
    }
    for key in KEYS:
        np.testing.assert_array_equal(dec[key], out[key], err_msg=key)


# ---------------------------------------------------------------------------
# partition
# ---------------------------------------------------------------------------
def _part_inputs(c, with_gseg, with_bins_t):
    bins = _dev(c, "bins")
    gseg = _dev(c, "gseg") if with_gseg else None
    bins_t = (_memo(c, "dev-bins_t", lambda: bins.t().contiguous())
              if with_bins_t else None)
    return bins, gseg, bins_t


def _segments_equal(got, want, c, sel, msg):
    for k in sel:
        s, n = int(c["starts"][k]), int(c["counts"][k])
        _eq(got[s:s + n], want[s:s + n], f"{msg} segment {k}")


@pytest.mark.parametrize("with_bins_t", [False, True], ids=["rowmajor", "colT"])
@pytest.mark.parametrize("with_gseg", [False, True], ids=["nogseg", "gseg"])
@pytest.mark.parametrize("c", oc.partition_cases(),
                         ids=_ids(oc.partition_cases()))
def test_partition_entry_points(c, with_gseg, with_bins_t):
    gpu = _gpu_ops()
    bins, gseg, bins_t = _part_inputs(c, with_gseg, with_bins_t)
    ref_r, ref_lc, ref_g = _memo(c, "part-ref",
                                 lambda: oc.oracle_partition(c))
    args = (bins, _dev(c, "ridx"), c["starts"], c["counts"], c["split_feat"],
            c["split_bin"], c["default_left"])
    sel = range(c["K"])

    out = gpu.partition_rows(*args, gpair_seg=gseg, bins_t=bins_t)
    _eq(out[0], ref_r, "partition_rows ridx")
    _eq(out[1], ref_lc, "partition_rows left counts")
    if with_gseg:
        _eq(out[2], ref_g, "partition_rows gseg")

    for full_rewrite in (False, True):
        ctx = gpu.partition_begin(*args, gpair_seg=gseg, bins_t=bins_t,
                                  gseg_full_rewrite=full_rewrite)
        r, lc, g = gpu.partition_finish(ctx)
        tag = f"begin/finish full_rewrite={full_rewrite}"
        _eq(r, ref_r, tag + " ridx")
        _eq(lc, ref_lc, tag + " left counts")
        if with_gseg and full_rewrite:
            # only the split segments are rewritten; the rest is undefined
            _segments_equal(g, ref_g, c, sel, tag + " gseg")
        elif with_gseg:
            _eq(g, ref_g, tag + " gseg")


@pytest.mark.parametrize("with_bins_t", [False, True], ids=["rowmajor", "colT"])
@pytest.mark.parametrize("with_gseg", [False, True], ids=["nogseg", "gseg"])
@pytest.mark.parametrize("c", oc.packed_cases(), ids=_ids(oc.packed_cases()))
def test_partition_rows_from_packed(c, with_gseg, with_bins_t):
    """The default training loop's device-planned partition: plan, count and
    prefix in device-limit mode, scatter into the ping-pong buffer."""
    gpu = _gpu_ops()
    bins, gseg, bins_t = _part_inputs(c, with_gseg, with_bins_t)
    K, n = c["K"], c["n"]
    ok = oc.packed_ok(c["packed"])
    sel = np.nonzero(ok)[0].tolist()
    ref_r, ref_lc, ref_g = _memo(c, "packed-ref",
                                 lambda: oc.oracle_partition(c, sel))
    rows = int(c["counts"].sum())
    chunk_bound = (rows + 2047) // 2048 + K   # as the trainer bounds it
    dest = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    r, g, pull, ev = gpu.partition_rows_from_packed(
        bins, _dev(c, "ridx"), _dev(c, "starts"), _dev(c, "counts"),
        _dev(c, "packed"), gseg, bins_t, chunk_bound, ridx_dest=dest)
    ev.synchronize()
    arr = pull[: 7 * K].numpy().copy()
    torch.cuda.synchronize()

    np.testing.assert_array_equal(arr[: 6 * K],
                                  c["packed"].numpy().reshape(-1))
    np.testing.assert_array_equal(arr[6 * K: 6 * K + len(sel)],
                                  ref_lc.numpy())
    assert r.data_ptr() == dest.data_ptr()
    want = torch.full((n,), -7, dtype=torch.int32)
    for k in sel:
        s, cnt = int(c["starts"][k]), int(c["counts"][k])
        want[s:s + cnt] = ref_r[s:s + cnt]
    _eq(r, want, "ridx_out (unsplit segments must stay -7)")
    if with_gseg:
        _segments_equal(g, ref_g, c, sel, "gseg_out")


# ---------------------------------------------------------------------------
# update_margins parity, bin_matrix, quantize_gpair
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", oc.margin_cases(), ids=_ids(oc.margin_cases()))
def test_update_margins_parity(c):
    gpu = _gpu_ops()
    ref = oc.oracle_margins(c)
    m = c["margin"].cuda()
    gpu.update_margins(m, c["ridx_a"].cuda(), c["starts"], c["counts"],
                       c["leaf_values"], ridx_b=c["ridx_b"].cuda(),
                       parity=c["parity"])
    _eq(m, ref, "two buffers + parity")
    m = c["margin"].cuda()
    gpu.update_margins(m, c["ridx_sel"].cuda(), c["starts"], c["counts"],
                       c["leaf_values"])
    _eq(m, ref, "single buffer")


@pytest.mark.parametrize("c", oc.bin_matrix_cases(),
                         ids=_ids(oc.bin_matrix_cases()))
def test_bin_matrix_case(c):
    gpu = _gpu_ops()
    out = gpu.bin_matrix(c["values"].cuda(), c["cuts_flat"].cuda(),
                         c["cut_ptr"].cuda())
    _eq(out, oc.oracle_bins(c), c["id"])
    n, F = c["values"].shape
    F_pad = (F + 15) // 16 * 16
    assert out.stride(0) == F_pad and out.stride(1) == 1
    full = out.as_strided((n, F_pad), (F_pad, 1), 0).cpu()
    assert (full[:, F:] == 255).all(), "pad bytes must read as missing"
    _eq(full[:, :F], out, "as_strided view covers the same storage")


@pytest.mark.parametrize("c", oc.quantize_cases(),
                         ids=_ids(oc.quantize_cases()))
def test_quantize_gpair_case(c):
    gpu = _gpu_ops()
    out = gpu.quantize_gpair(c["gpair"].cuda(), c["scale_g"], c["scale_h"])
    assert out.dtype == torch.int32
    _eq(out, oc.oracle_quantize(c), c["id"])
    if c["id"] == "zero-g-column":
        assert not out[:, 0].any()
