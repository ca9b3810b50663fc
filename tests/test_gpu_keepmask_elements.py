"""-m gpu: anoddpm_keep_mask (csrc/keepmask.hip) through the C ABI on every case of tests/keepmask_cases.py -- keep
bytes, stitched words, counts and status words bit for bit against the numpy restatement and, without a roi, against the
composition the library offered before -- with every output buffer poisoned before the launch (0xFF bytes, NaN, -1), at
pointers that are not 16-byte aligned, without the optional stitch, launched twice, and through `metrics.keep_mask`."""
import ctypes

import numpy as np
import pytest
import torch

import keepmask_cases as kc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_BUILT = {}


def built(c):
    """(arrays, restatement) of a case: computed once, shared by the tests, left unchanged."""
    if c["name"] not in _BUILT:
        d = kc.make_case(c)
        _BUILT[c["name"]] = (d, kc.restate(c, d))
    return _BUILT[c["name"]]


def dev_at(x, offset, dtype=None):
    """A device copy of host array x that starts `offset` elements into its allocation (allocations are 256-byte aligned)."""
    t = torch.from_numpy(np.ascontiguousarray(x).reshape(-1))
    buf = torch.empty(t.numel() + offset, dtype=t.dtype, device=DEV)
    buf[offset:].copy_(t)
    return buf[offset:]


def launch(c, d, offset=0, stitch=None):
    """One call of the entry point on poisoned outputs -> (dict of host arrays as `restate` returns them, the device tensors)."""
    from anoddpm_amd import _lib
    S, C, H, W = c["S"], c["C"], c["H"], c["W"]
    stitch = c["stitch"] if stitch is None else stitch
    t = {"score": dev_at(d["buf"], offset), "thr": dev_at(d["thr"], offset)}
    if d["roi"] is not None:
        t["roi"] = dev_at(d["roi"], offset)
    if stitch:
        t["real"], t["recon"] = dev_at(d["real"], offset), dev_at(d["recon"], offset)
        t["stitched"] = torch.full((S * C * H * W + offset,), float("nan"), device=DEV)[offset:]
    t["keep"] = torch.full((S * H * W + offset,), 0xFF, dtype=torch.uint8, device=DEV)[offset:]
    t["regen"] = torch.full((S + offset,), -1, dtype=torch.int32, device=DEV)[offset:]
    t["status"] = torch.full((S + offset,), -1, dtype=torch.int32, device=DEV)[offset:]
    if offset:
        assert all(x.data_ptr() % 16 != 0 for k, x in t.items() if k != "keep") and t["keep"].data_ptr() % 4 != 0
    a = _lib.KeepMaskArgs()
    a.score, a.threshold, a.keep, a.regen_count, a.status = (t[k].data_ptr() for k in ("score", "thr", "keep", "regen", "status"))
    a.roi = t["roi"].data_ptr() if "roi" in t else None
    if stitch:
        a.real, a.recon, a.stitched = t["real"].data_ptr(), t["recon"].data_ptr(), t["stitched"].data_ptr()
    a.score_stride, a.thr_stride = H * W + c["pad"], c["thr_stride"]
    a.roi_stride = H * W if c["roi"] == "plane" else 0
    a.real_stride = C * H * W if c["real_per_plane"] else 0
    a.S, a.H, a.W, a.C, a.r = S, H, W, C, c["r"]
    _lib.check(_lib.lib().anoddpm_keep_mask(ctypes.byref(a), _lib.current_stream()), "keep_mask")
    got = dict(keep=t["keep"].cpu().numpy().reshape(S, H, W), regen=t["regen"].cpu().numpy(), status=t["status"].cpu().numpy(),
               stitched=t["stitched"].cpu().numpy().reshape(S, C, H, W) if stitch else None)
    return got, t


@pytest.mark.parametrize("c", kc.CASES, ids=[c["name"] for c in kc.CASES])
def test_case_through_the_c_abi(c):
    d, want = built(c)
    got, t = launch(c, d)
    kc.compare(got, want, c["name"])
    if c["roi"] is None:                                             # and against what the library could compose before
        S, C, H, W = c["S"], c["C"], c["H"], c["W"]
        score = t["score"].as_strided((S, H, W), (H * W + c["pad"], W, 1))
        real = t["real"].reshape(-1, C, H, W) if c["stitch"] else None
        keep, stitched, regen = kc.composition_torch(score, t["thr"], c["r"], real, t["recon"].reshape(S, C, H, W) if c["stitch"] else None)
        comp = dict(keep=keep.cpu().numpy(), stitched=stitched.cpu().numpy() if c["stitch"] else None, regen=regen.cpu().numpy(),
                    status=want["status"])                           # the composition reports no status
        kc.compare(got, comp, c["name"] + " against the composition")


RAGGED = [c for c in kc.CASES if (c["H"], c["W"]) in ((17, 33), (40, 70)) and c["S"] == 3]


@pytest.mark.parametrize("c", RAGGED[::3], ids=[c["name"] for c in RAGGED[::3]])
def test_pointers_that_are_not_16_byte_aligned(c):
    d, want = built(c)
    kc.compare(launch(c, d, offset=1)[0], want, c["name"])


@pytest.mark.parametrize("c", RAGGED[1::3], ids=[c["name"] for c in RAGGED[1::3]])
def test_without_the_optional_stitch(c):
    d, want = built(c)
    got, _ = launch(c, d, stitch=False)
    kc.compare(got, dict(want, stitched=None), c["name"])


@pytest.mark.parametrize("c", RAGGED[2::3], ids=[c["name"] for c in RAGGED[2::3]])
def test_two_launches_give_the_same_bits(c):
    d, want = built(c)
    first, second = launch(c, d)[0], launch(c, d)[0]
    kc.compare(second, first, c["name"])
    kc.compare(first, want, c["name"])


@pytest.mark.parametrize("c", [c for c in kc.CASES if c["pad"] == 0][::4], ids=lambda c: c["name"])
def test_metrics_keep_mask(c):
    """The wrapper: shapes, the threshold as a tensor and (one value) as a Python number, the status, no host values in between."""
    from anoddpm_amd import metrics
    d, want = built(c)
    S, C, H, W = c["S"], c["C"], c["H"], c["W"]
    up = {k: torch.from_numpy(d[k]).to(DEV) if d[k] is not None else None for k in ("score", "thr", "roi", "real", "recon")}
    stitch = dict(real=up["real"], recon=up["recon"]) if c["stitch"] else {}
    for thr in [up["thr"]] + ([float(d["thr"][0])] if d["thr"].size == 1 else []):
        o = metrics.keep_mask(up["score"], thr, c["r"], up["roi"], return_status=True, **stitch)
        assert o["keep"].shape == (S, 1, H, W) and o["regen"].shape == (S,) and o["regen"].is_cuda
        assert o["stitched"] is None or o["stitched"].shape == (S, C, H, W)
        kc.compare({k: (v.cpu().numpy() if v is not None else None) for k, v in o.items()}, want, c["name"])
    assert "status" not in metrics.keep_mask(up["score"], up["thr"], c["r"], up["roi"])
