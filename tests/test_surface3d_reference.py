"""Distance transform and boundary distances of whole volumes without a device: the restatements of tests/surface3d_cases.py
agree with each other and with scipy on every case -- the integer brute-force minimum, scipy's transform, the kernel's own
three-axis decomposition, scipy's erosion border -- every planted defect is seen by at least one named case (otherwise the case
list would prove nothing), the slice-wise answer differs from the volume's, and the host side of the native path: ABI 42, the
exports, the struct sizes the binding derives from the header, the workspace function and the refusals made before any launch.
CPU only."""
import ctypes
import inspect

import numpy as np
import pytest

import surface3d_cases as s3
import surface_cases as sc
from score_cases import bits as _bits


# ---------------------------------------------------------------------------------- distance transform
@pytest.mark.parametrize("name", sorted(s3.transform_cases()))
def test_brute_force_equals_scipy_and_the_decomposition(name):
    vols, level = s3.transform_cases()[name]
    for v in s3.foreground(vols, level):
        sq = s3.edt3_brute(v)
        if v.all():
            assert (sq == -1).all() and (s3.edt3_separable(v) == -1).all()
            continue
        assert _bits(s3.edt3_scipy(v), np.sqrt(sq.astype(np.float64))), name      # scipy = the correctly rounded root of the integer
        assert np.array_equal(s3.edt3_scipy_exact(v), sq), name
        assert np.array_equal(s3.edt3_separable(v), sq), name                      # the kernel's decomposition
        assert (sq[~v] == 0).all() and (sq[v] > 0).all() and sq.max() < 2 ** 31


def test_transform_cases_reach_what_they_are_for():
    c = s3.transform_cases()
    corner = s3.edt3_brute(c["corner17x19x23"][0][0] > 0)
    assert np.array_equal(corner, s3.corner_closed_form((17, 19, 23))) and corner.max() == 16 ** 2 + 18 ** 2 + 22 ** 2
    assert c["one_fg"][0].all() and c["all_fg_mid"][0][1].all() and not c["all_fg_mid"][0][0].all()
    assert np.isnan(c["level_nan"][0]).sum() == 3 and c["level_nan"][1] != 0.0
    assert c["wide6x37x300"][0].shape[-1] > 256 and c["long2x3x4100"][0].shape[-1] > 4096
    assert {c[f"ytile2x{h}x9"][0].shape[2] for h in (s3.Y_TILE - 1, s3.Y_TILE, s3.Y_TILE + 1)} == {s3.Y_TILE - 1, s3.Y_TILE, s3.Y_TILE + 1}
    _, steps_y, steps_x = s3.edt3_separable(c["sparse9x12x33"][0][0] > 0, return_steps=True)
    assert steps_y / (9 * 12 * 33) > 2 and steps_x / (9 * 12 * 33) > 2                        # the walks are long
    plane = c["plane1x9x70"][0][0, 0] > 0
    assert np.array_equal(s3.edt3_brute(plane[None])[0], sc.edt2_brute(plane))                # D = 1: the plane transform


TRANSFORM_DEFECTS = {                                        # defect -> (keywords of edt3_separable, the case that sees it)
    "y pass skipped": (dict(skip_y=True), "dense3x4x5"),
    "y pass in place, unstaged": (dict(inplace_y=True), "sparse9x12x33"),
    "search cap of 8": (dict(cap=8), "corner17x19x23"),
}


@pytest.mark.parametrize("defect", sorted(TRANSFORM_DEFECTS))
def test_planted_transform_defects_are_seen(defect):
    kw, name = TRANSFORM_DEFECTS[defect]
    v = s3.foreground(*s3.transform_cases()[name])[0]
    assert not np.array_equal(s3.edt3_separable(v, **kw), s3.edt3_brute(v)), (defect, name)


def test_walk_bounded_by_k_is_seen_in_the_steps_not_in_the_values():
    """k < best lets a lane walk on after k^2 >= best: k <= k^2, so it looks at a superset and the minimum is the same -- the
    defect costs steps, which the restatement counts (tools/bench_surface3d.py reports the kernel's mean walk the same way)."""
    v = s3.foreground(*s3.transform_cases()["sparse9x12x33"])[0]
    good, gy, gx = s3.edt3_separable(v, return_steps=True)
    bad, by, bx = s3.edt3_separable(v, bound="k", return_steps=True)
    assert np.array_equal(good, bad) and by > gy and bx > gx


# ---------------------------------------------------------------------------------- boundary distances
@pytest.mark.parametrize("name", sorted(s3.surface_cases()))
def test_surface_restatements_agree(name):
    pred, ref = s3.surface_cases()[name]
    for (p, r), (k, f, npct) in zip(s3.pairs_of(pred, ref), s3.surface_expected(name)):
        for m in (p, r):                                                                      # the border: scipy's erosion, and by hand
            inner = np.pad(m, 1)
            by_hand = m & ~(inner[:-2, 1:-1, 1:-1] & inner[2:, 1:-1, 1:-1] & inner[1:-1, :-2, 1:-1] & inner[1:-1, 2:, 1:-1] &
                            inner[1:-1, 1:-1, :-2] & inner[1:-1, 1:-1, 2:])
            assert np.array_equal(s3.border6(m), by_hand)
        bp, br, d_pr, d_rp = s3.directed(p, r)
        if bp.any() and br.any():                                                             # scipy's indices = the brute force = the kernel's passes
            assert np.array_equal(d_pr, s3.edt3_brute(~br)[bp]) and np.array_equal(d_rp, s3.edt3_separable(~bp)[br])
        for key in ("counts", "max2", "p95"):
            assert _bits(np.asarray(k[key]), np.asarray(f[key])), (name, key)
        assert k["status"] == f["status"]
        if k["status"]:
            assert np.isnan(k["mean"]).all() and np.isnan(k["p95"]).all() and (k["max2"] == -1).all()
            continue
        for d in range(2):                                                                    # fixed-order sum against fsum: n * 2^-52 relative
            assert abs(k["mean"][d] - f["mean"][d]) <= k["counts"][d] * 2.0 ** -52 * f["mean"][d], (name, d)
        for got, want in zip(k["p95"], npct):
            assert sc.ulps(got, want) <= 8, (name, got, want)


def test_surface_cases_reach_what_they_are_for():
    e = {name: s3.surface_expected(name) for name in s3.surface_cases()}
    assert [k["status"] for k, _, _ in e["empties"]] == [0, 1, 2, 3] and [k["status"] for k, _, _ in e["batch3_shared"]] == [0, 0, 0]
    assert all((k["max2"] == 0).all() and (k["p95"] == 0).all() for k, _, _ in e["identical"])
    assert (e["corners"][0][0]["counts"] == 1).all() and (e["corners"][0][0]["max2"] == 36 + 64 + 100).all()      # n = 1
    assert e["all_fg"][0][0]["counts"][0] == 5 * 6 * 7 - 3 * 4 * 5                            # the six faces
    p, r = s3.pairs_of(*s3.surface_cases()["one_slice"])[0]
    assert e["one_slice"][0][0]["counts"].tolist() == [int(p.sum()), int(r.sum())]            # D = 1: every foreground voxel
    assert e["one_slice"][0][0]["counts"][0] > sc.surface_ref(p[0], r[0])["counts"][0]        # ... which the plane border is not
    assert (e["noise8x32x40"][0][0]["counts"] > 4 * 1024).all()
    assert any((19 * (int(n) - 1)) % 20 for k, _, _ in e["blobs12x20x24"] for n in (*k["counts"], k["counts"].sum()))


def test_slicewise_answer_differs_from_the_volume():
    p, r = s3.pairs_of(*s3.surface_cases()["slice_shift"])[0]
    vol = s3.surface_expected("slice_shift")[0][0]["hd95"]
    planes = s3.slicewise_hd95(p, r)
    assert vol == 1.0 and planes == 0.0                      # the same box one slice up: nearest outline on slice z +- 1


SURFACE_DEFECTS = {                                          # defect -> (keywords of surface3d_ref, the case that sees it, the key)
    "border by 26 neighbours": (dict(structure=s3.CUBE), "blobs12x20x24", "counts"),
    "border without the z neighbours": (dict(structure=s3.IN_PLANE), "blobs12x20x24", "counts"),
    "z faces not treated as outside": (dict(z_outside=False), "all_fg", "counts"),
    "y pass skipped": (dict(transform=dict(skip_y=True)), "blobs12x20x24", "max2"),
    "y pass in place, unstaged": (dict(transform=dict(inplace_y=True)), "blobs12x20x24", "p95"),
    "search cap of 8": (dict(transform=dict(cap=8)), "corners", "max2"),
    "thread-strided order": (dict(mean=s3._mean_voxel_strided), "blobs12x20x24", "mean"),
    "wrong percentile for the pooled leg": (dict(pooled="one_direction"), "one_slice", "p95"),
}


@pytest.mark.parametrize("defect", sorted(SURFACE_DEFECTS))
def test_planted_surface_defects_are_seen(defect):
    kw, name, key = SURFACE_DEFECTS[defect]
    p, r = s3.pairs_of(*s3.surface_cases()[name])[0]
    good = s3.surface_expected(name)[0][0]
    bad = s3.surface3d_ref(p, r, **dict(dict(mean=s3._mean_ranks), **kw))
    assert not _bits(np.asarray(good[key]), np.asarray(bad[key])), (defect, name, key)


# ---------------------------------------------------------------------------------- the native path, host side
def test_abi_42_exports_and_struct_sizes():
    from anoddpm_amd import _lib
    L = _lib.lib()
    assert _lib.ABI_VERSION >= 42 and L.anoddpm_abi_version() == _lib.ABI_VERSION
    for name in ("anoddpm_distance_transform3d", "anoddpm_surface_distance3d", "anoddpm_surface3d_workspace_bytes"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
    # derived from the header, no hand-written binding
    for cname, st, fields in ((b"anoddpm_distance3d_args", _lib.Distance3dArgs, ("src", "sq", "dist", "workspace", "workspace_bytes", "src_stride", "S", "D", "H", "W", "level")),
                              (b"anoddpm_surface3d_args", _lib.Surface3dArgs, ("pred", "ref", "workspace", "workspace_bytes", "counts", "max2", "mean", "p95", "status",
                                                                                "pred_stride", "ref_stride", "S", "D", "H", "W", "level"))):
        assert st in _lib._STRUCTS and L.anoddpm_struct_size(cname) == ctypes.sizeof(st) and tuple(f for f, _ in st._fields_) == fields
    assert "Distance3dArgs" not in inspect.getsource(_lib) and "Surface3dArgs" not in inspect.getsource(_lib)


def test_workspace_function():
    from anoddpm_amd import _lib
    ws = _lib.lib().anoddpm_surface3d_workspace_bytes
    assert ws(1, 46342, 1, 1) == -1 and ws(1, 1, 46342, 1) == -1 and ws(1, 1, 1, 46342) == -1      # (D-1)^2 reaches 2^31
    assert ws(1, 46341, 1, 1) == 16 * 46341 + 16 * 46341 + 8
    for bad in ((0, 4, 4, 4), (1, 0, 4, 4), (1, 4, 0, 4), (1, 4, 4, 0), (-1, 4, 4, 4)):
        assert ws(*bad) == -1, bad
    assert ws(1, 2048, 1024, 1024) == -1                                                          # D * H * W = 2^31
    assert ws(1, 32769, 1, 32769) == -1 and ws(1, 32768, 1, 32768) > 0                            # 2 * 32768^2 = 2^31: the squares summed
    assert ws(1, 32768, 32768, 1) == -1                                                           # 2 * S * D * H rows: a grid too large
    assert ws(4, 155, 240, 240) == 16 * 4 * 155 * 240 * 240 + 16 * 4 * 155 * 240 + 8 * 4
    # the transform's stated share: half of the voxel part
    for S, D, H, W in ((1, 1, 1, 1), (3, 5, 7, 9)):
        assert 8 * S * D * H * W == (ws(S, D, H, W) - 16 * S * D * H - 8 * S) // 2
    for call in (c for cs in s3.contract_calls().values() for c in cs):
        sc_ = call["scalars"]
        assert s3.TABLE[call["entry"]]["ws_min"](sc_) <= ws(sc_["S"], sc_["D"], sc_["H"], sc_["W"])


def _args(L, cls, over):
    from anoddpm_amd import _lib
    a = getattr(_lib, cls)()
    for f, _ in a._fields_:
        if f not in ("workspace_bytes", "S", "D", "H", "W", "level") and not f.endswith("_stride"):
            setattr(a, f, 4096)                              # never dereferenced: every call below is refused before a launch
    a.S, a.D, a.H, a.W, a.level = 2, 3, 4, 5, 0.0
    for f in ("src_stride", "pred_stride", "ref_stride"):
        if hasattr(a, f):
            setattr(a, f, 60)
    a.workspace_bytes = 1 << 20
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_refusals_are_made_before_any_launch():
    from anoddpm_amd import _lib
    L = _lib.lib()
    dt, sd = L.anoddpm_distance_transform3d, L.anoddpm_surface_distance3d
    for fn, cls, over, text in (
            (dt, "Distance3dArgs", dict(src=None), b"null pointer"), (dt, "Distance3dArgs", dict(sq=None), b"null pointer"),
            (dt, "Distance3dArgs", dict(workspace=None), b"null pointer"), (dt, "Distance3dArgs", dict(D=0), b">= 1"),
            (dt, "Distance3dArgs", dict(src_stride=59), b"volumes overlap"),
            (dt, "Distance3dArgs", dict(workspace_bytes=8 * 2 * 60 - 1), b"distance_transform3d: workspace too small"),
            (sd, "Surface3dArgs", dict(status=None), b"null pointer"), (sd, "Surface3dArgs", dict(ref=None), b"null pointer"),
            (sd, "Surface3dArgs", dict(W=46343), b"below 2^31"), (sd, "Surface3dArgs", dict(pred_stride=59), b"volumes overlap"),
            (sd, "Surface3dArgs", dict(ref_stride=7), b"ref_stride"),
            (sd, "Surface3dArgs", dict(workspace_bytes=L.anoddpm_surface3d_workspace_bytes(2, 3, 4, 5) - 1), b"surface_distance3d: workspace too small")):
        assert fn(ctypes.byref(_args(L, cls, over)), None) == -1, over
        assert text in L.anoddpm_last_error(), (over, L.anoddpm_last_error())
    assert dt(None, None) == -1 and sd(None, None) == -1


def test_python_surface_names_and_signatures():
    import evaluation
    from anoddpm_amd import metrics
    assert str(inspect.signature(metrics.distance_transform3d)) == "(x, level=0.0, squared=False, batched=None)"
    assert str(inspect.signature(metrics.surface_distance3d)) == "(pred, ref, level=0.0, return_status=False)"
    assert str(inspect.signature(metrics.HD95_volume)) == "(real_mask, pred_mask)"
    assert inspect.signature(metrics.anomaly_metrics_volume_surface) == inspect.signature(metrics.anomaly_metrics_volume)
    for name in ("distance_transform3d", "surface_distance3d", "HD95_volume", "anomaly_metrics_volume_surface"):
        assert name in metrics.__all__ and getattr(evaluation, name) is getattr(metrics, name)
    with pytest.raises(TypeError):
        metrics.distance_transform3d(np.zeros((2, 4, 4), np.float32))
    import torch
    with pytest.raises(ValueError):
        metrics.distance_transform3d(torch.zeros(4, 4))
    with pytest.raises(TypeError):
        metrics.surface_distance3d(torch.zeros(2, 4, 4), np.zeros((2, 4, 4), np.float32))
    with pytest.raises(ValueError):
        metrics.surface_distance3d(torch.zeros(2, 2, 4, 4), torch.zeros(4, 4))
