"""-m gpu: the distance transform and the boundary distances of whole volumes (anoddpm_distance_transform3d /
anoddpm_surface_distance3d of csrc/surface3d.hip) through the C ABI and through metrics.distance_transform3d / surface_distance3d /
HD95_volume / anomaly_metrics_volume_surface, against the restatements of tests/surface3d_cases.py: squared distances equal to the
integer brute-force minimum, distances bit-equal to scipy.ndimage.distance_transform_edt, border counts and largest squared
distances equal, percentiles bit-equal to the header's definition and within 8 ulp of numpy.percentile, means bit-equal to the
rank-order restatement and within n * 2^-52 relative of math.fsum, the same bits on every launch, whatever the workspace held and
wherever a volume sits in a batch; and every buffer of the entry points in guarded arenas (contract_cases' method)."""
import ctypes
import gc

import numpy as np
import pytest
import torch

import contract_cases as cc
import surface3d_cases as s3
import surface_cases as sc
from score_cases import bits_any_nan as _bits, host as _host

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PARENT_VOLUME_KEYS = ("dice", "precision", "recall", "FPR", "AUC", "AP", "best_dice", "best_threshold", "AUC_status")
SURFACE_KEYS = ("HD", "HD95", "ASSD", "surface_status")


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _expected_transform(vols, level):
    fg = s3.foreground(vols, level)
    sq = np.stack([s3.edt3_brute(f) for f in fg]).astype(np.int32)
    dist = np.stack([s3.edt3_scipy(f) if not f.all() else np.full(f.shape, np.inf) for f in fg])
    return fg, sq, dist


# ---------------------------------------------------------------------------------- distance transform
@pytest.mark.parametrize("name", sorted(s3.transform_cases()))
def test_transform_equals_brute_force_and_scipy(name):
    from anoddpm_amd import metrics
    vols, level = s3.transform_cases()[name]
    fg, want_sq, want = _expected_transform(vols, level)
    x = _dev(vols)
    sq = metrics.distance_transform3d(x, level=level, squared=True)
    dist = metrics.distance_transform3d(x, level=level)
    assert sq.dtype == torch.int32 and dist.dtype == torch.float64 and sq.is_cuda and dist.is_cuda
    assert tuple(sq.shape) == vols.shape == tuple(dist.shape)
    bad = np.flatnonzero(_host(sq).reshape(-1) != want_sq.reshape(-1))
    assert bad.size == 0, (name, bad[:8], _host(sq).reshape(-1)[bad[:8]], want_sq.reshape(-1)[bad[:8]])
    assert _bits(_host(dist), want), name
    assert _bits(_host(metrics.distance_transform3d(x, level=level)), _host(dist))
    if name == "one_fg":
        assert (_host(sq) == -1).all() and np.isinf(_host(dist)).all()
    if name == "plane1x9x70":                                # one slice: the plane transform, bit for bit
        assert _bits(_host(dist)[0, 0], _host(metrics.distance_transform(x[0, 0], level=level)))
    if name == "corner17x19x23":
        assert int(sq.max()) == 16 ** 2 + 18 ** 2 + 22 ** 2 and np.array_equal(_host(sq)[0], s3.corner_closed_form((17, 19, 23)))
    if name == "all_fg_mid":
        assert (_host(sq)[1] == -1).all() and np.isinf(_host(dist)[1]).all() and (_host(sq)[[0, 2]] >= 0).all()
        for s in (0, 2):                                     # a volume on its own gives what it gives inside the batch
            assert _bits(_host(metrics.distance_transform3d(x[s], level=level)), _host(dist)[s])
        assert _bits(_host(metrics.distance_transform3d(x[[2, 1, 0]], level=level))[0], _host(dist)[2])


def test_transform_through_the_abi_with_a_strided_source():
    from anoddpm_amd import _lib
    L = _lib.lib()
    vols, level = s3.transform_cases()["level_nan"]
    S, D, H, W = vols.shape
    n, stride = D * H * W, D * H * W + 13                    # an odd gap between the volumes
    _, want_sq, want = _expected_transform(vols, level)
    buf = torch.full((S * stride,), float("inf"), device=DEV)
    for s in range(S):
        buf[s * stride:s * stride + n] = _dev(vols[s]).reshape(-1)
    sq = torch.empty((S, D, H, W), dtype=torch.int32, device=DEV)
    dist = torch.empty((S, D, H, W), dtype=torch.float64, device=DEV)
    ws = torch.empty((2 * S * n,), dtype=torch.int32, device=DEV)
    a = _lib.Distance3dArgs()
    a.src, a.sq, a.dist, a.workspace, a.workspace_bytes = buf.data_ptr(), sq.data_ptr(), dist.data_ptr(), ws.data_ptr(), 8 * S * n
    a.src_stride, a.S, a.D, a.H, a.W, a.level = stride, S, D, H, W, level
    with torch.cuda.device(DEV):
        assert L.anoddpm_distance_transform3d(ctypes.byref(a), _lib.current_stream()) == 0, L.anoddpm_last_error()
    assert np.array_equal(_host(sq), want_sq) and _bits(_host(dist), want)
    a.dist = None                                            # the optional output
    sq.fill_(7)
    with torch.cuda.device(DEV):
        assert L.anoddpm_distance_transform3d(ctypes.byref(a), _lib.current_stream()) == 0
    assert np.array_equal(_host(sq), want_sq)


# ---------------------------------------------------------------------------------- boundary distances
def _check_pair(g, want, tag):
    """One pair's outputs (host arrays) against (surface3d_fp64, surface3d_ref, numpy percentiles)."""
    order, ref, npct = want
    print(tag, {k: np.asarray(g[k]).tolist() for k in ("counts", "max2", "mean", "p95", "status")})
    assert int(g["status"]) == ref["status"], tag
    assert np.array_equal(g["counts"], ref["counts"]) and np.array_equal(g["max2"], ref["max2"]), (tag, g["counts"], ref["counts"], g["max2"], ref["max2"])
    if ref["status"]:
        assert np.isnan(g["mean"]).all() and np.isnan(g["p95"]).all() and all(np.isnan(g[k]) for k in ("hd", "hd95", "assd")), tag
        return
    assert _bits(g["p95"], ref["p95"]), (tag, g["p95"], ref["p95"])
    assert _bits(g["mean"], order["mean"]), (tag, g["mean"], order["mean"])
    for d in range(2):
        assert abs(g["mean"][d] - ref["mean"][d]) <= float(ref["counts"][d]) * 2.0 ** -52 * ref["mean"][d], (tag, d)
    for q, w in zip(g["p95"], npct):
        assert sc.ulps(q, w) <= 8, (tag, q, w)
    assert _bits(g["hd"], np.float64(ref["hd"])) and _bits(g["hd95"], np.float64(ref["hd95"])) and _bits(g["assd"], np.float64(order["assd"])), tag


def _surface_abi(pred, ref, fill):
    """anoddpm_surface_distance3d through the ABI with the workspace pre-filled with the byte `fill` -> host outputs."""
    from anoddpm_amd import _lib
    L = _lib.lib()
    S, D, H, W = pred.shape
    n = D * H * W
    need = L.anoddpm_surface3d_workspace_bytes(S, D, H, W)
    ws = torch.full((need,), fill, dtype=torch.uint8, device=DEV)
    p, r = _dev(pred), _dev(ref)
    out = {"counts": torch.full((S, 2), -7, dtype=torch.int32, device=DEV), "max2": torch.full((S, 2), -7, dtype=torch.int32, device=DEV),
           "mean": torch.full((S, 2), -7.0, dtype=torch.float64, device=DEV), "p95": torch.full((S, 3), -7.0, dtype=torch.float64, device=DEV),
           "status": torch.full((S,), -7, dtype=torch.int32, device=DEV)}
    a = _lib.Surface3dArgs()
    a.pred, a.ref, a.workspace, a.workspace_bytes = p.data_ptr(), r.data_ptr(), ws.data_ptr(), need
    for k, t in out.items():
        setattr(a, k, t.data_ptr())
    a.pred_stride, a.ref_stride, a.S, a.D, a.H, a.W, a.level = n, (n if ref.ndim == 4 and S > 1 else 0), S, D, H, W, 0.0
    with torch.cuda.device(DEV):
        assert L.anoddpm_surface_distance3d(ctypes.byref(a), _lib.current_stream()) == 0, L.anoddpm_last_error()
    return {k: _host(t) for k, t in out.items()}


@pytest.mark.parametrize("name", sorted(s3.surface_cases()))
def test_surface_distance_against_the_restatements(name):
    from anoddpm_amd import metrics
    pred, ref = s3.surface_cases()[name]
    want = s3.surface_expected(name)
    got = metrics.surface_distance3d(_dev(pred), _dev(ref))
    assert tuple(got["status"].shape) == (pred.shape[0],) and tuple(got["p95"].shape) == (pred.shape[0], 3)
    first = {k: _host(v) for k, v in got.items()}
    for s in range(pred.shape[0]):
        _check_pair({k: v[s] for k, v in first.items()}, want[s], f"{name}[{s}]")
    # the same bits on a second launch, and through the ABI whatever the workspace held before
    again = {k: _host(v) for k, v in metrics.surface_distance3d(_dev(pred), _dev(ref)).items()}
    assert all(_bits(again[k], first[k]) for k in first), name
    for fill in (0x00, 0xa5):
        raw = _surface_abi(pred, ref, fill)
        assert all(_bits(raw[k], first[k]) for k in raw), (name, hex(fill))
    if name == "empties":                                    # pair 0 is untouched by its empty neighbours: what it is alone
        alone = {k: _host(v) for k, v in metrics.surface_distance3d(_dev(pred[0]), _dev(ref[0])).items()}
        assert all(_bits(alone[k], first[k][0]) for k in alone)
        assert first["status"].tolist() == [0, 1, 2, 3] and (first["max2"][1:] == -1).all() and first["counts"][1].tolist() == [0, 34]
    if name == "batch3_shared":                              # a pair's bits do not depend on its place, nor on the shared form
        full = np.broadcast_to(ref, pred.shape).copy()
        own = {k: _host(v) for k, v in metrics.surface_distance3d(_dev(pred[::-1].copy()), _dev(full)).items()}
        assert all(_bits(own[k][::-1], first[k]) for k in own)
    if name == "slice_shift":
        p, r = s3.pairs_of(pred, ref)[0]
        assert first["hd95"][0] == 1.0 and s3.slicewise_hd95(p, r) == 0.0
    if name == "one_slice":                                  # D = 1 is not the plane case
        plane = metrics.surface_distance(_dev(pred[0, 0]), _dev(ref[0, 0]))
        assert int(first["counts"][0, 0]) == int(pred.sum()) > int(_host(plane["counts"])[0])


def test_hd95_volume_averages_the_valid_volumes():
    from anoddpm_amd import metrics
    pred, ref = s3.surface_cases()["batch3_shared"]
    pred = pred.copy()
    pred[1] = 0                                              # one empty volume
    full = np.broadcast_to(ref, pred.shape).copy()
    want = [s3.surface3d_fp64(p, r)["hd95"] for p, r in s3.pairs_of(pred, full)]
    assert np.isnan(want[1])
    got = metrics.HD95_volume(_dev(full), _dev(pred))
    assert isinstance(got, float) and got == (want[0] + want[2]) / 2
    assert np.isnan(metrics.HD95_volume(_dev(full[1]), _dev(pred[1])))


# ---------------------------------------------------------------------------------- hostile buffers
_SIGNED = {1: np.uint8, 4: np.int32, 8: np.int64}
_stop = []                                                   # why nothing further may be launched


def _launch(call, ws_fill=0, refuse=False):
    """One call on fresh arenas -> (return code, arenas before, arenas after); tests/test_gpu_contract.py's, for this table."""
    from anoddpm_amd import _lib
    L = _lib.lib()
    if _stop:
        pytest.fail(f"not started: {_stop[0]}")
    before = cc.build_arenas(call, cc.workspace_bytes(call, L), ws_fill)
    dev = {f: torch.from_numpy(a.bits.view(_SIGNED[a.bits.dtype.itemsize])).to(DEV) for f, a in before.items()}
    a = cc.fill_struct(call, before, {f: t.data_ptr() for f, t in dev.items()}, ws_short=1 if refuse else 0)
    try:
        with torch.cuda.device(DEV):
            code = getattr(L, "anoddpm_" + call["entry"])(ctypes.byref(a), _lib.current_stream())
            torch.cuda.synchronize()
        after = {f: x.copy(dev[f].cpu().numpy()) for f, x in before.items()}
    except Exception as e:                                   # a device error: nothing of this module runs after it
        _stop.append(f"{call['entry']} {call['id']}: {e}")
        raise
    if code != 0 and not refuse:
        _stop.append(f"{call['entry']} {call['id']}: error code {code}: {L.anoddpm_last_error()}")
        pytest.fail(_stop[0])
    return code, before, after


@pytest.mark.parametrize("entry", sorted(s3.TABLE))
def test_entry_point_keeps_its_contract_on_hostile_buffers(entry):
    from anoddpm_amd import _lib
    calls = s3.contract_calls()[entry]
    problems = []
    with s3.registered():
        _, _, after = _launch(calls[-1])
        left = after["workspace"].get().tobytes()            # the first case gets what the last one leaves
        for call in calls:
            expected = cc.expected_of(call)
            first = None
            for i, fill in enumerate((0, 0xff, left)):
                _, before, after = _launch(call, fill)
                found = cc.check(call, before, after, expected, reference=first)
                if first is not None:
                    found += [f for f in cc.check(call, before, after, expected) if f[0] not in ("wrong_value", "status")]
                problems += [(call["id"], f"launch {i}") + f for f in found]
                first = after if first is None else first
            left = after["workspace"].get().tobytes()
            code, before, after = _launch(call, 0xff, refuse=True)           # a workspace one byte short: refused, nothing launched
            assert code != 0 and s3.TABLE[entry]["too_small"] in _lib.lib().anoddpm_last_error(), call["id"]
            touched = [f for f in before if not np.array_equal(before[f].bits, after[f].bits)]
            assert not touched, (call["id"], "a refused call wrote to", touched)
    for p in problems[:40]:
        print(p)
    assert not problems, f"{len(problems)} finding(s); the first: {problems[0]}"


# ---------------------------------------------------------------------------------- the Python surface
def _scene():
    """(real, recon, mask) [2][6][24][28]: the reconstruction is off by 1 on a box per volume and on scattered voxels; the mask is
    the box moved by one voxel."""
    rng = np.random.default_rng(4242)
    shape = (2, 6, 24, 28)
    real = (rng.random(shape, dtype=np.float32) * np.float32(0.5) - np.float32(0.25)).astype(np.float32)
    recon, mask = real.copy(), np.zeros(shape, np.float32)
    for v, (z, y, x) in enumerate(((1, 5, 6), (2, 9, 12))):
        recon[v, z:z + 3, y:y + 6, x:x + 7] += np.float32(1)
        mask[v, z + 1:z + 4, y + 1:y + 7, x:x + 7] = 1
    recon[rng.random(shape) < 0.004] += np.float32(1)
    return real, recon, mask


def _same_number(a, b):
    return (a != a and b != b) or np.float64(a).tobytes() == np.float64(b).tobytes()


@pytest.mark.parametrize("with_pp", (False, True))
def test_anomaly_metrics_volume_surface_adds_the_boundary_distances(with_pp):
    from anoddpm_amd import metrics
    real, recon, mask = _scene()
    dr, dc, dm = _dev(real), _dev(recon), _dev(mask)
    pp = metrics.VolumePostProcess(median=3, erode=0, min_size=7, connectivity=1) if with_pp else None
    plain = metrics.anomaly_metrics_volume(dr, dc, dm, postprocess=pp)
    out = metrics.anomaly_metrics_volume_surface(dr, dc, dm, postprocess=pp)
    sfx = ("", "_pp") if with_pp else ("",)
    for v, (r0, r) in enumerate(zip(plain, out)):
        assert set(r0) == {k + s for k in PARENT_VOLUME_KEYS for s in sfx} | {"maps"}                     # the parent's key set exactly
        assert set(r) == set(r0) | {k + s for k in SURFACE_KEYS for s in sfx}
        assert all(_same_number(r[k], r0[k]) for k in r0 if k != "maps")                                  # and its bits
        for s in sfx:
            pred = _host(r["maps"]["pred" + s]) > 0
            want = s3.surface3d_fp64(pred, mask[v] > 0)
            assert r["surface_status" + s] == want["status"] == 0 and isinstance(r["surface_status" + s], int)
            for k, w in (("HD", want["hd"]), ("HD95", want["hd95"]), ("ASSD", want["assd"])):
                assert _same_number(r[k + s], w), (v, k + s, r[k + s], w)
    empty = metrics.anomaly_metrics_volume_surface(dr[0], dc[0], torch.zeros_like(dm[0]))                 # no border in the mask: NaN
    assert empty["surface_status"] == 2 and all(np.isnan(empty[k]) for k in ("HD", "HD95", "ASSD"))


def test_surface_distance3d_is_capturable():
    from anoddpm_amd import metrics
    pred, ref = s3.surface_cases()["batch3_shared"]
    other = np.roll(pred, 1, axis=3)
    x, r = _dev(pred), _dev(ref)
    keys = ("counts", "max2", "mean", "p95", "status", "hd", "hd95", "assd")

    def run():
        o = metrics.surface_distance3d(x, r)
        return [o[k] for k in keys]

    eager = [_host(t) for t in run()]
    x.copy_(_dev(other))
    eager_other = [_host(t) for t in run()]
    x.copy_(_dev(pred))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    gc.collect()
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()                                             # no collection of older graphs inside the capture
    try:
        with torch.cuda.graph(g):
            captured = run()
    finally:
        if was_enabled:
            gc.enable()
    g.replay()
    torch.cuda.synchronize()
    assert all(_bits(_host(t), e) for t, e in zip(captured, eager))
    x.copy_(_dev(other))
    g.replay()
    torch.cuda.synchronize()
    assert all(_bits(_host(t), e) for t, e in zip(captured, eager_other))
