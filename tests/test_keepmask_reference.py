"""No device: the numpy restatement of anoddpm_keep_mask (tests/keepmask_cases.py) against scipy on every case, the planted defects
the comparison function has to catch, the struct and the refusals of the entry point, and the argument errors of
`metrics.keep_mask` / `detection_two_pass` that need no device."""
import ctypes

import numpy as np
import pytest
import torch

import keepmask_cases as kc


@pytest.fixture(scope="module")
def built():
    """(case, arrays, restatement) of every case, computed once and left unchanged."""
    out = []
    for c in kc.CASES:
        d = kc.make_case(c)
        out.append((c, d, kc.restate(c, d)))
    return out


def test_case_list_covers_every_parameter_value():
    cs = kc.CASES
    assert len({c["name"] for c in cs}) == len(cs)
    assert {(c["H"], c["W"], c["r"]) for c in cs} >= {(h, w, r) for h, w in kc.SHAPES for r in range(kc.R_MAX + 1)}
    for key, values in (("S", {1, 3}), ("C", {1, 3}), ("thr_stride", {0, 1}), ("roi", {None, "shared", "plane"}),
                        ("real_per_plane", {False, True}), ("pad", {0, 5}), ("stitch", {False, True}), ("pattern", set(kc.PATTERNS))):
        assert {c[key] for c in cs} == values, key
    for pattern in kc.PATTERNS:                                      # every pattern with several planes, per-plane thresholds, big radius
        assert any(c["pattern"] == pattern and c["S"] == 3 and c["thr_stride"] == 1 and c["r"] == 8 and (c["H"], c["W"]) == (40, 70) for c in cs)
    assert any(c["S"] == 3 and c["pad"] > 0 and c["roi"] is None for c in cs)
    spans = {min(t_x, max(1, c["S"] * t_x * t_y // 2048)) for c in cs for t_x, t_y in [(-(-c["W"] // 32), -(-c["H"] // 16))]}
    assert spans == {1, 2, 3}                                         # tiles per workgroup (csrc/keepmask.hip): every path, one ragged
    assert any(-(-c["W"] // 32) % 3 and c["S"] * -(-c["W"] // 32) * -(-c["H"] // 16) // 2048 == 3 for c in cs)


def test_restatement_equals_scipy_on_every_case(built):
    """`binary_dilation(seed, iterations=r)` with scipy's defaults, bit for bit; scipy treats iterations=0 as "until nothing
    changes", so r = 0 is stated as the identity."""
    from scipy import ndimage as ndi
    for c, d, want in built:
        S, r = c["S"], c["r"]
        thr = np.broadcast_to(d["thr"], (S,))
        inside = np.ones(d["score"].shape, bool) if d["roi"] is None else np.broadcast_to(d["roi"] == 1, d["score"].shape)
        for p in range(S):
            with np.errstate(invalid="ignore"):
                seed = (d["score"][p] > thr[p]) & inside[p]
            grown = ndi.binary_dilation(seed, iterations=r) if r > 0 else seed
            regen = grown & inside[p]
            assert np.array_equal(want["keep"][p], (~regen).astype(np.uint8)), c["name"]
            assert want["regen"][p] == regen.sum()
            if c["stitch"]:
                real = np.broadcast_to(d["real"], d["recon"].shape)[p]
                assert np.array_equal(want["stitched"][p].view(np.uint32), np.where(regen[None], d["recon"][p], real).view(np.uint32)), c["name"]


def test_l1_ball_equals_the_iterated_cross():
    from scipy import ndimage as ndi
    rng = np.random.default_rng(9790)
    for h, w in kc.SHAPES:
        seed = rng.random((h, w)) < 0.03
        seed[h // 2, w // 2] = True
        assert np.array_equal(kc.dilate_numpy(seed, 0), seed)
        for r in range(1, kc.R_MAX + 1):
            assert np.array_equal(kc.dilate_numpy(seed, r), ndi.binary_dilation(seed, iterations=r)), (h, w, r)


def test_patterns_exercise_what_they_are_named_for(built):
    by = {}
    for c, d, want in built:
        by.setdefault(c["pattern"], []).append((c, d, want))
    for c, d, want in by["all_above"]:
        if c["roi"] is None:
            assert not want["keep"].any() and (want["regen"] == c["H"] * c["W"]).all()
    for c, d, want in by["none_above"] + [x for x in by["nan_thr"] if x[0]["thr_stride"] == 0]:
        assert want["keep"].all() and not want["regen"].any()
    for c, d, want in by["nan_thr"]:
        assert (want["status"] & kc.ROC_NAN).any() and want["keep"][c["S"] // 2].all()
    for c, d, want in by["nan_score"]:
        assert (want["status"] & kc.ROC_NAN).tolist() == [int(p == c["S"] // 2) for p in range(c["S"])]
    for c, d, want in by["bad_roi"]:
        assert (want["status"] & kc.ROC_BAD_MASK).any()
    for c, d, want in by["strict"]:
        assert (d["score"] == d["thr"][0]).any()
    for c, d, want in by["negzero"]:
        if c["roi"] is None and c["r"] == 0:
            assert np.array_equal(want["keep"][0] == 0, d["score"][0] > 0) and want["keep"][1:].all()
    for c, d, want in by["isolation"]:
        assert np.isnan(d["recon"]).any() or want["keep"].min() == 0
        assert np.isfinite(want["stitched"]).all()
    for c, d, want in by["corners"]:
        if c["roi"] is None:
            assert (want["keep"][:, 0, 0] == 0).all() and (want["keep"][:, -1, -1] == 0).all()


@pytest.mark.parametrize("defect", kc.DEFECTS)
def test_planted_defect_is_caught(built, defect):
    """Each defect changes what the restatement writes on at least one case, and `compare` refuses the result there."""
    caught = 0
    for c, d, want in built:
        bad = kc.restate(c, d, defect)
        try:
            kc.compare(bad, want, c["name"])
        except AssertionError:
            caught += 1
    assert caught > 0, defect
    for c, d, want in built[:8]:
        kc.compare(kc.restate(c, d), want, c["name"])                # and it accepts the restatement itself


def test_reflected_border_cannot_differ_from_the_empty_one():
    """Why the border defect planted above is "the outside counts as set" (the border `1 - erode(1 - a)` has) and not a reflected
    border: the mirror image of a seed is never nearer to a pixel than the seed itself, so a dilation over a reflected plane IS
    the dilation with nothing outside -- no test can tell them apart."""
    rng = np.random.default_rng(9791)
    for h, w in kc.SHAPES:
        seed = rng.random((h, w)) < 0.1
        for r in range(kc.R_MAX + 1):
            ph, pw = min(r, h), min(r, w)                            # numpy reflects at most one plane width
            p = np.pad(seed, ((ph, ph), (pw, pw)), mode="symmetric")
            assert np.array_equal(kc.dilate_numpy(p, r)[ph:ph + h, pw:pw + w], kc.dilate_numpy(seed, r)), (h, w, r)


# ------------------------------------------------------------------ ABI


def test_abi_of_the_keep_mask_entry_point():
    from anoddpm_amd import _lib
    L = _lib.lib()
    assert _lib.ABI_VERSION >= 40 and L.anoddpm_abi_version() == _lib.ABI_VERSION
    assert L.anoddpm_struct_size(b"anoddpm_keep_mask_args") == ctypes.sizeof(_lib.KeepMaskArgs) == 9 * 8 + 4 * 8 + 5 * 4 + 4
    assert [n for n, _ in _lib.KeepMaskArgs._fields_] == ["score", "threshold", "roi", "real", "recon", "keep", "stitched", "regen_count", "status",
                                                          "score_stride", "thr_stride", "roi_stride", "real_stride", "S", "H", "W", "C", "r"]
    assert [t for _, t in _lib.KeepMaskArgs._fields_] == [ctypes.c_void_p] * 9 + [ctypes.c_int64] * 4 + [ctypes.c_int32] * 5
    assert L.anoddpm_keep_mask.argtypes == [ctypes.POINTER(_lib.KeepMaskArgs), ctypes.c_void_p]
    assert _lib.KEEP_DILATE_MAX == kc.R_MAX == 8 and (_lib.ROC_NAN, _lib.ROC_BAD_MASK) == (kc.ROC_NAN, kc.ROC_BAD_MASK)


def valid_args(S=3, H=17, W=33, C=2, fake=0x1000):
    from anoddpm_amd import _lib
    a = _lib.KeepMaskArgs()
    for f in ("score", "threshold", "roi", "real", "recon", "keep", "stitched", "regen_count", "status"):
        setattr(a, f, fake)
    a.score_stride, a.thr_stride, a.roi_stride, a.real_stride = H * W + 3, 1, H * W, C * H * W
    a.S, a.H, a.W, a.C, a.r = S, H, W, C, 2
    return a


REFUSED = [("null " + f, {f: None}) for f in ("score", "threshold", "keep", "regen_count", "status")] + [
    ("r below 0", {"r": -1}), ("r above 8", {"r": 9}), ("S < 1", {"S": 0}), ("H < 1", {"H": 0}), ("W < 1", {"W": -3}), ("C < 1", {"C": 0}),
    ("S * tiles at 2^31", {"S": 2 ** 31 - 1, "score_stride": 2 ** 40}),
    ("S * tiles at 2^31, big plane", {"S": 2 ** 10, "H": 16 * 2 ** 11, "W": 32 * 2 ** 10, "score_stride": 2 ** 40, "roi_stride": 0, "real_stride": 0}),
    ("planes overlap", {"score_stride": 17 * 33 - 1}), ("thr_stride 2", {"thr_stride": 2}), ("thr_stride -1", {"thr_stride": -1}),
    ("roi_stride", {"roi_stride": 17 * 33 + 1}), ("real_stride", {"real_stride": 17 * 33}),
    ("only real", {"recon": None, "stitched": None}), ("only recon", {"real": None, "stitched": None}),
    ("no stitched", {"stitched": None}), ("no real", {"real": None}), ("no recon", {"recon": None}),
]


def test_refused_arguments_without_a_device():
    """Every refusal happens on the host before anything is cleared or launched: EINVAL and a text, with pointers never read."""
    from anoddpm_amd import _lib
    L = _lib.lib()
    assert L.anoddpm_keep_mask(None, None) == _lib.EINVAL and b"keep_mask" in L.anoddpm_last_error()
    for what, change in REFUSED:
        a = valid_args()
        for k, v in change.items():
            setattr(a, k, v)
        assert L.anoddpm_keep_mask(ctypes.byref(a), None) == _lib.EINVAL, what
        assert b"keep_mask" in L.anoddpm_last_error(), what


# ------------------------------------------------------------------ host logic


def test_keep_mask_argument_errors():
    from anoddpm_amd import metrics
    s = torch.zeros(3, 4, 5)
    with pytest.raises(TypeError, match="score"):
        metrics.keep_mask(np.zeros((4, 5), np.float32), 0.5)
    with pytest.raises(TypeError, match="threshold"):
        metrics.keep_mask(s, "0.5")
    with pytest.raises(TypeError, match="threshold"):
        metrics.keep_mask(s, None)
    with pytest.raises(ValueError, match="threshold"):
        metrics.keep_mask(s, torch.zeros(2))
    for bad in (-1, 9, 1.5, True):
        with pytest.raises(ValueError, match="dilate"):
            metrics.keep_mask(s, 0.5, dilate=bad)
    with pytest.raises(ValueError, match="score"):
        metrics.keep_mask(torch.zeros(5), 0.5)
    with pytest.raises(ValueError, match="score"):
        metrics.keep_mask(torch.zeros(0, 4, 5), 0.5)
    with pytest.raises(ValueError, match="roi"):
        metrics.keep_mask(s, 0.5, roi=torch.zeros(2, 4, 5))
    with pytest.raises(TypeError, match="roi"):
        metrics.keep_mask(s, 0.5, roi=np.zeros((4, 5)))
    with pytest.raises(ValueError, match="real and recon"):
        metrics.keep_mask(s, 0.5, real=torch.zeros(3, 1, 4, 5))
    with pytest.raises(ValueError, match="recon"):
        metrics.keep_mask(s, 0.5, real=torch.zeros(3, 1, 4, 5), recon=torch.zeros(2, 1, 4, 5))
    with pytest.raises(ValueError, match="real"):
        metrics.keep_mask(s, 0.5, real=torch.zeros(2, 1, 4, 5), recon=torch.zeros(3, 1, 4, 5))
    with pytest.raises(TypeError, match="recon"):
        metrics.keep_mask(s, 0.5, real=torch.zeros(3, 1, 4, 5), recon=[1])
    assert "keep_mask" in metrics.__all__


def test_detection_two_pass_argument_errors():
    import GaussianDiffusion as GD
    d = GD.GaussianDiffusionModel([8, 12], GD.get_beta_schedule(100, "linear"), noise="gauss")
    x = torch.zeros(1, 1, 8, 12)
    ok = dict(threshold=0.5, t_first=6, t_second=[3, 5], total_avg=2)
    with pytest.raises(ValueError, match="one image"):
        d.detection_two_pass(None, torch.zeros(2, 1, 8, 12), None, **ok)
    for key, bad in (("t_first", 100), ("t_first", -1), ("t_second", [3, 100]), ("t_second", 250), ("t_second", [2.5]), ("t_first", True)):
        with pytest.raises(ValueError, match=key):
            d.detection_two_pass(None, x, None, **dict(ok, **{key: bad}))
    with pytest.raises(ValueError, match="denoise_fn"):
        d.detection_two_pass(None, x, None, denoise_fn="simplex", **ok)
    for bad in (-1, 9, 2.0, True):
        with pytest.raises(ValueError, match="dilate"):
            d.detection_two_pass(None, x, None, dilate=bad, **ok)
    with pytest.raises(ValueError, match="total_avg"):
        d.detection_two_pass(None, x, None, **dict(ok, total_avg=0))
    with pytest.raises(TypeError, match="resampling"):
        d.detection_two_pass(None, x, None, resampling=(2, 2), **ok)
    d.sampler = GD.StridedSampler(2)
    with pytest.raises(ValueError, match="strided sampler is refused"):
        d.detection_two_pass(None, x, None, resampling=GD.Resampling(2, 2), **ok)
    assert GD.GaussianDiffusionModel.detection_two_pass is d.detection_two_pass.__func__
