"""CPU: the audit of what the fifteen workgroup-era metric entry points read and write (tests/contract_cases.py) -- the table
against the header, what the cases claim to be, the checker on simulated calls with planted defects, and the host side of the
library (workspace sizes, refused calls).  The entry points themselves run in tests/test_gpu_contract.py."""
import ctypes

import numpy as np
import pytest
from scipy import ndimage

import contract_cases as cc
import pro_cases as prc
import roc_cases as rc
import smooth_cases as smc
import ssim_cases as ssc
import surface_cases as sfc
from anoddpm_amd import _lib

ISSUE_LIST = ("roc_auc", "pro_auc", "component_areas", "ssim", "distance_transform", "surface_distance", "median2d", "erode2d",
              "small_components", "gauss2d", "map_scores", "median3d", "erode3d", "small_components3d", "component_areas3d")
ALL = [(e, i) for e in cc.ENTRY_POINTS for i in range(len(cc.cases(e)))]


def _id(p):
    return f"{p[0]}-{cc.cases(p[0])[p[1]]['id']}"


@pytest.fixture(params=ALL, ids=_id)
def call(request):
    return cc.cases(request.param[0])[request.param[1]]


# ---------------------------------------------------------------------------------------------------- the table
def test_table_names_the_fifteen_entry_points_and_the_library_exports_them():
    assert sorted(cc.TABLE) == sorted(ISSUE_LIST) == sorted(cc.CASES)
    for e, t in cc.TABLE.items():
        assert "anoddpm_" + e in _lib.SYMBOLS and t["struct"] in _lib._C_STRUCTS
        assert t["ws_fn"] is None or t["ws_fn"] in _lib.SYMBOLS
    assert (cc.ROC_NAN, cc.ROC_INF, cc.ROC_NEGATIVE, cc.ROC_BAD_MASK, cc.ROC_TRUNCATED, cc.SURFACE_EMPTY_PRED) == \
        (_lib.ROC_NAN, _lib.ROC_INF, _lib.ROC_NEGATIVE, _lib.ROC_BAD_MASK, _lib.ROC_CURVE_TRUNCATED, _lib.SURFACE_EMPTY_PRED)


@pytest.mark.parametrize("entry", cc.ENTRY_POINTS)
def test_every_pointer_field_of_the_struct_is_classified(entry):
    """A pointer field added to the header without a classification fails here; so does a wrong element type or stride field."""
    t = cc.TABLE[entry]
    fields = _lib._C_STRUCTS[t["struct"]]
    pointers = {n: b for n, b, p in fields if p}
    scalars = {n for n, b, p in fields if not p}
    assert set(t["fields"]) == set(pointers), (sorted(set(pointers) - set(t["fields"])), sorted(set(t["fields"]) - set(pointers)))
    ctype = {"f4": "float", "f8": "double", "i4": "int32_t", "i8": "int64_t"}
    for n, f in t["fields"].items():
        assert f["kind"] in ("in", "out", "ws")
        if f["kind"] == "ws":
            assert n == "workspace" and pointers[n] == "void" and "workspace_bytes" in scalars
            continue
        assert pointers[n] == ctype[f["dtype"]], (n, pointers[n])
        if f["kind"] == "in":
            assert f["stride"] is None or f["stride"] in scalars, n
            assert not f["zero_ok"] or f["stride"], n
        else:
            assert f["written"] in ("all", "curve")
            assert (f["written"] == "curve") == (n.startswith("curve_") and n != "curve_len"), n
    assert t["status"] is None or t["fields"][t["status"]]["kind"] == "out"
    # every case passes the pointers the table does not call optional, and only scalars the struct has
    for c in cc.cases(entry):
        passed = set(c["inputs"]) | set(cc.expected_of(c)) | ({"workspace"} if cc.has_workspace(entry) else set())
        assert {n for n, f in t["fields"].items() if not f.get("optional")} <= passed <= set(t["fields"]), c["id"]
        assert set(c["scalars"]) <= scalars, c["id"]


# ---------------------------------------------------------------------------------------------------- what the cases claim to be
def test_every_case_has_three_segments_and_a_clean_outside(call):
    t = cc.TABLE[call["entry"]]
    e = cc.expected_of(call)
    assert call["scalars"]["S"] == 3 and all(v["value"].shape[0] == 3 for v in e.values())
    assert call["skip"] <= {1}
    if t["status"]:
        st = e[t["status"]]["value"]
        allowed = cc.ROC_TRUNCATED if "curve_cap" in call["scalars"] else 0
        assert (st[[0, 2]] & ~allowed == 0).all(), st                     # the outer segments never break a precondition
        planted = any(w in call["id"] for w in ("nan-middle", "negative-middle", "emptypred-middle"))
        assert (st[1] & ~allowed != 0) == planted, st                     # the middle one only where the case says so
    for name, x in call["inputs"].items():                                # odd gaps: the stride of every strided input is n + 7
        if np.asarray(x).ndim == 2:
            assert cc.build_arenas(call)[name].stride == np.asarray(x).shape[1] + cc.GAP and cc.GAP % 2 == 1


def test_roc_cases_are_what_they_claim():
    seen = set()
    for c in cc.cases("roc_auc"):
        e, n, v = cc.expected_of(c), c["scalars"]["n"], c["variant"]
        seen.add((n, v["extra"], v["all"], v["small"], np.asarray(c["inputs"]["mask"]).ndim == 1))
        if n == 63:
            assert (e["counts"]["value"][[0, 2], 3] == 63).all()          # R = n: the sentinel is the last word of its buffer
            assert (63 + 1) % 64 == 0
        if not v["curve"]:
            assert e["status"]["value"].tolist() == [0, cc.ROC_NAN, 0] and c["skip"] == {1}
            continue
        length, cap = e["curve_len"]["value"], c["scalars"]["curve_cap"]
        if v["small"]:
            assert cap == 2 and n > 2 and (length[[0, 2]] > cap).all(), (c["id"], length)     # really truncating
            assert (e["status"]["value"][[0, 2]] == cc.ROC_TRUNCATED).all()
            assert not e["curve_fps"]["written"].reshape(-1)[-1:].all() or length[2] >= cap
        else:
            assert cap == max(n, 2) and (length <= cap).all() and (e["status"]["value"] == 0).all()
        if np.asarray(c["inputs"]["mask"]).ndim == 2:
            assert e["counts"]["value"][1, 0] == 0 and np.isnan(e["auc"]["value"][1])        # the middle segment: P = 0
            if v["extra"]:
                assert np.isnan(e["ap"]["value"][1]) and np.isnan(e["best_dice"]["value"][1])
        else:
            assert e["counts"]["value"][1, 3] == 1                        # one run
        assert (e["curve_fps"]["written"].sum(axis=1) == np.minimum(length, cap)).all()
    for n in (1, 63, 64, 65, 1025):
        assert {(n, False, False), (n, True, False), (n, True, True)} <= {s[:3] for s in seen}, n       # plain, EXTRA, CURVE_ALL
    assert {s[3] for s in seen} == {s[4] for s in seen} == {True, False}


def test_roc_restatement_agrees_with_scipy_ranks_at_the_new_shapes():
    """AUC = the Mann-Whitney statistic with mid-ranks, as tests/test_roc_reference.py compares it; the fixtures have no entry for
    these inputs."""
    from scipy import stats
    for c in cc.cases("roc_auc"):
        for s in (0, 2):
            score, mask = cc._seg(c["inputs"]["score"], s), cc._seg(c["inputs"]["mask"], s)
            r = rc.roc_numpy(mask, score)
            if r["P"] == 0 or r["N"] == 0:
                continue
            ranks = stats.rankdata(score.astype(np.float64))
            u = ranks[mask != 0].sum() - r["P"] * (r["P"] + 1) / 2
            assert abs(u / (r["P"] * r["N"]) - r["auc"]) <= rc.auc_tolerance(score.size), c["id"]


def test_pro_cases_are_what_they_claim():
    seen = set()
    for c in cc.cases("pro_auc"):
        e, sc = cc.expected_of(c), c["scalars"]
        n = sc["planes_per_segment"] * sc["H"] * sc["W"]
        shared = np.asarray(c["inputs"]["area"]).ndim == 1
        seen.add((sc["H"], sc["planes_per_segment"], shared, "mask" in c["inputs"], sc.get("curve_cap")))
        if not c["variant"]["curve"]:
            assert e["status"]["value"].tolist() == [0, cc.ROC_NEGATIVE, 0]
            continue
        length = e["curve_len"]["value"]
        if (sc["H"], sc["W"]) == (8, 8):
            assert (length[[0, 2]] == n).all()                            # every score distinct: R = n, n = 64 = seg_words for one plane
        if sc["curve_cap"] == 3:
            assert (length[[0, 2]] > 3).all() and (e["status"]["value"][[0, 2]] == cc.ROC_TRUNCATED).all()
        else:
            assert sc["curve_cap"] == n and (e["status"]["value"] == 0).all()
        if shared:
            assert length[1] == 1 and np.asarray(c["inputs"]["region_counts"]).size == sc["planes_per_segment"]
        else:
            assert e["counts"]["value"][1, 0] == 0 and np.isnan(e["aupro"]["value"][1])      # K = 0
            assert np.isnan(e["curve_pro"]["value"][1][e["curve_pro"]["written"][1]]).all()
        assert np.isfinite(e["aupro"]["value"][[0, 2]]).all()
        # the kernel-order restatement against the exact one, by the bound of tests/test_pro_reference.py
        for s in (0, 2):
            mask = cc._seg(c["aux"]["mask"], s).reshape(sc["planes_per_segment"], sc["H"], sc["W"])
            score = c["inputs"]["score"][s]
            prc.check_against_exact(prc.pro_fp64(mask, score, 0.3, 2), prc.pro_exact(mask, score, 0.3, 2), c["id"])
    assert {(8, 1), (8, 2), (5, 1), (5, 2)} == {s[:2] for s in seen}
    assert {s[2] for s in seen} == {s[3] for s in seen} == {True, False}


def test_component_area_cases_feed_the_pro_cases():
    by_id = {c["id"]: c for c in cc.cases("component_areas")}
    for H, W in ((8, 8), (5, 13)):
        areas = cc.expected_of(by_id[f"{H}x{W}-c2-pro-masks"])
        pro = next(c for c in cc.cases("pro_auc") if c["id"].startswith(f"{H}x{W}-m1-ownarea-mask-cap"))
        assert np.array_equal(areas["area"]["value"].reshape(3, -1), pro["inputs"]["area"])
        assert np.array_equal(areas["counts"]["value"], pro["inputs"]["region_counts"])
    for c in cc.cases("component_areas") + cc.cases("small_components"):
        e = cc.expected_of(c)
        found = e["counts"]["value"].reshape(3, -1)[:, 0]
        assert found[1] == 0 and (found[[0, 2]] > (1 if "pro-masks" in c["id"] else 3)).all()       # the empty middle plane
        # scipy's labelling at the new shapes, as tests/test_postproc_reference.py compares it
        sc = c["scalars"]
        for s in range(3):
            b = c["inputs"]["src"][s].reshape(sc["H"], sc["W"]) > np.float32(sc["level"])
            lab, m = ndimage.label(b, ndimage.generate_binary_structure(2, sc["connectivity"]))
            assert m == e["counts"]["value"].reshape(3, -1)[s, 0]
            if c["entry"] == "component_areas":
                size = np.bincount(lab.ravel())
                size[0] = 0
                assert np.array_equal(size[lab], e["area"]["value"][s])


def test_components3d_cases_agree_with_scipy():
    for c in cc.cases("component_areas3d") + cc.cases("small_components3d"):
        e, sc = cc.expected_of(c), c["scalars"]
        assert (e["counts"]["value"][1] == 0).all()
        for s in range(3):
            b = c["inputs"]["src"][s].reshape(sc["D"], sc["H"], sc["W"]) > np.float32(sc["level"])
            lab, m = ndimage.label(b, ndimage.generate_binary_structure(3, sc["connectivity"]))
            assert m == e["counts"]["value"].reshape(3, -1)[s, 0] and (s == 1 or m > 3)
            size = np.bincount(lab.ravel())
            size[0] = 0
            if c["entry"] == "component_areas3d":
                assert np.array_equal(size[lab], e["area"]["value"][s])
            else:
                assert np.array_equal((size[lab] >= sc["min_size"]).astype(np.float32), e["dst"]["value"][s])
                assert 0 < e["counts"]["value"][s, 1] < m or s == 1       # the filter removes some and keeps some


def test_filter_cases_agree_with_scipy():
    for c in cc.cases("median2d") + cc.cases("median3d"):
        e, sc = cc.expected_of(c), c["scalars"]
        shape = ((sc["D"],) if "D" in sc else ()) + (sc["H"], sc["W"])
        for s in set(range(3)) - c["skip"]:
            want = ndimage.median_filter(c["inputs"]["src"][s].reshape(shape), size=sc["k"], mode="reflect")
            if "roi" in c["inputs"]:
                roi = np.asarray(c["inputs"]["roi"]).reshape((-1,) + shape[-2:])
                assert 0 < (roi == 0).sum() < roi.size
                want = np.where(np.broadcast_to(roi if len(shape) == 3 else roi[0], shape) == 0, np.float32(0), want)
            assert rc.bits_equal(want.astype(np.float32), e["dst"]["value"][s]), c["id"]
        if c["skip"]:
            assert e["status"]["value"].tolist() in ([0, cc.ROC_NEGATIVE, 0], [0, cc.ROC_NAN, 0])
    for c in cc.cases("erode2d") + cc.cases("erode3d"):
        e, sc = cc.expected_of(c), c["scalars"]
        shape = ((sc["D"],) if "D" in sc else ()) + (sc["H"], sc["W"])
        for s in range(3):
            b = c["inputs"]["src"][s].reshape(shape) > np.float32(sc["level"])
            assert np.array_equal(ndimage.binary_erosion(b, iterations=sc["n"]), e["dst"]["value"][s] != 0), c["id"]
        assert 0 < e["dst"]["value"][1].sum() < e["dst"]["value"][1].size         # the full middle loses its rim only
    for c in cc.cases("gauss2d"):
        e, sc = cc.expected_of(c), c["scalars"]
        assert sc["radius"] in (2, 16) and (sc["radius"] > sc["H"]) == (sc["radius"] == 16)
        for s in range(3):
            want = ndimage.gaussian_filter(c["inputs"]["src"][s].reshape(sc["H"], sc["W"]), c["aux"]["sigma"], truncate=4.0)
            assert rc.bits_equal(want, e["dst"]["value"][s]), c["id"]


def test_distance_and_surface_cases_are_what_they_claim():
    for c in cc.cases("distance_transform"):
        e, sc = cc.expected_of(c), c["scalars"]
        assert (e["sq"]["value"][1] == -1).all() and (e["sq"]["value"][[0, 2]] >= 0).all()
        for s in (0, 2):
            fg = c["inputs"]["src"][s].reshape(sc["H"], sc["W"]) > np.float32(sc["level"])
            assert 0 < fg.sum() < fg.size
            if c["variant"]["dist"]:
                assert rc.bits_equal(sfc.edt_scipy(fg), e["dist"]["value"][s])
        if c["variant"]["dist"]:
            assert np.isposinf(e["dist"]["value"][1]).all()
        if sc["W"] == 4100:
            assert e["sq"]["value"].max() > 2048 ** 2
    shared = set()
    for c in cc.cases("surface_distance"):
        e = cc.expected_of(c)
        shared.add(np.asarray(c["inputs"]["ref"]).ndim == 1)
        assert e["status"]["value"].tolist() == [0, cc.SURFACE_EMPTY_PRED, 0]
        assert e["counts"]["value"][1, 0] == 0 and e["counts"]["value"][1, 1] > 0 and (e["max2"]["value"][1] == -1).all()
        assert np.isnan(e["mean"]["value"][1]).all() and np.isnan(e["p95"]["value"][1]).all()
        assert np.isfinite(e["mean"]["value"][[0, 2]]).all() and (e["counts"]["value"][[0, 2]] > 4).all()
    assert shared == {True, False}


def test_ssim_and_score_cases_are_what_they_claim():
    seen = set()
    for c in cc.cases("ssim"):
        e, sc = cc.expected_of(c), c["scalars"]
        shared = np.asarray(c["inputs"]["real"]).ndim == 1
        seen.add((c["aux"]["window"], shared, c["variant"]["map"]))
        assert (sc["C"], sc["H"], sc["W"]) == (2, 17, 33) and sc["H"] > 16 and sc["W"] > 32         # 2 x 2 ragged tiles
        if not shared:
            assert e["mssim"]["value"][1] == 1.0                          # identical images
        for s in range(3):                                                # the definition with scipy's filters, as test_ssim_reference.py
            real = cc._seg(c["inputs"]["real"], s).reshape(2, 17, 33)
            want, smap = ssc.ssim_expected(real, c["inputs"]["recon"][s].reshape(2, 17, 33), c["aux"]["window"])
            assert abs(want - e["mssim"]["value"][s]) <= ssc.MSSIM_TOL, c["id"]
            if c["variant"]["map"]:
                assert np.abs(smap - e["map"]["value"][s]).max() <= ssc.MAP_TOL, c["id"]
    assert {s[0] for s in seen} == {3, 15, "gauss"} and {s[1] for s in seen} == {s[2] for s in seen} == {True, False}
    for c in cc.cases("map_scores"):
        e, sc = cc.expected_of(c), c["scalars"]
        if c["skip"]:
            assert e["status"]["value"].tolist() == [0, cc.ROC_NEGATIVE, 0]
            continue
        assert e["max"]["value"][1] == 0 and e["mean"]["value"][1] == 0
        for s in (0, 2):
            v = np.sort(c["inputs"]["src"][s].astype(np.float64))
            assert e["max"]["value"][s] == v[-1] and smc.within(e["mean"]["value"][s], v.mean(), sc["n"])
            assert smc.within(e["topk_mean"]["value"][s], v[sc["n"] - sc["k"]:].mean(), sc["k"])
    assert {(c["scalars"]["n"], c["scalars"]["k"]) for c in cc.cases("map_scores")} >= {(1, 1), (1023, 1), (1023, 1023), (1025, 1), (1025, 1025)}


# ---------------------------------------------------------------------------------------------------- the checker on simulated calls
def test_clean_simulation_gives_no_finding(call):
    before, after = cc.simulate(call)
    assert cc.check(call, before, after, cc.expected_of(call)) == []
    # the fills are what the module says: no output poison is a value a kernel writes, every guard is wider than a stride + 4096
    for a in before.values():
        assert a.guard >= a.stride + cc.GUARD_EXTRA and (a.guard * a.item.itemsize) % 256 == 0
        if a.kind == "out":
            assert (a.bits == cc.POISON[a.item.str[1:]]).all()
    if "workspace" in before:
        assert before["workspace"].n == cc.workspace_bytes(call) and (before["workspace"].get() == 0).all()


@pytest.mark.parametrize("defect", cc.DEFECTS)
def test_every_planted_defect_gives_its_finding(call, defect):
    want = cc.defect_finding(call, defect)
    if want is None:                                                      # nothing this defect could touch: said by the table, not a skip
        assert defect in ("before_workspace", "dirty_workspace", "curve_at_cap", "drop_status")
        return
    expected = cc.expected_of(call)
    if defect == "dirty_workspace":
        before0, after0 = cc.simulate(call, defect, ws_fill=0)
        assert cc.check(call, before0, after0, expected) == []           # zero pages hide it
        before, after = cc.simulate(call, defect, ws_fill=0xff)
        got = cc.names(cc.check(call, before, after, expected, reference=after0))
    else:
        before, after = cc.simulate(call, defect)
        got = cc.names(cc.check(call, before, after, expected))
    assert got and set(got) <= want and (len(want) > 1 or got == sorted(want)), (call["id"], defect, got)


def test_every_defect_is_planted_somewhere_for_every_entry_point():
    for e in cc.ENTRY_POINTS:
        for d in cc.DEFECTS:
            applies = any(cc.defect_finding(c, d) is not None for c in cc.cases(e))
            needs = {"before_workspace": cc.has_workspace(e), "dirty_workspace": cc.has_workspace(e), "curve_at_cap": e in ("roc_auc", "pro_auc"),
                     "drop_status": cc.TABLE[e]["status"] is not None}.get(d, True)
            assert applies == needs, (e, d)
    assert {n for c in cc.cases("roc_auc") + cc.cases("pro_auc") + cc.cases("median2d") for d in cc.DEFECTS
            for n in (cc.defect_finding(c, d) or ())} | {"workspace_dependent"} == set(cc.FINDINGS)


# ---------------------------------------------------------------------------------------------------- the host side of the library
def _host_call(call, ws_short=0, S=None):
    """The call on host arenas: only for calls the library must refuse before it launches anything."""
    L = _lib.lib()
    arenas = cc.build_arenas(call, cc.workspace_bytes(call, L))
    a = cc.fill_struct(call, arenas, {f: x.bits.ctypes.data for f, x in arenas.items()}, ws_short)
    if S is not None:
        a.S = S
    before = {f: x.bits.copy() for f, x in arenas.items()}
    code = getattr(L, "anoddpm_" + call["entry"])(ctypes.byref(a), None)
    assert all(np.array_equal(before[f], x.bits) for f, x in arenas.items())
    return code, L.anoddpm_last_error()


def test_workspace_size_and_refused_calls(call):
    L = _lib.lib()
    t = cc.TABLE[call["entry"]]
    code, msg = _host_call(call, S=0)
    assert code != 0 and msg, call["id"]                                  # S = 0 is refused
    if not cc.has_workspace(call["entry"]):
        return
    nbytes = cc.workspace_bytes(call, L)
    sc = call["scalars"]
    assert nbytes > 0 and nbytes >= t["ws_min"](sc) and nbytes % t["ws_align"] == 0, (nbytes, t["ws_min"](sc))
    if t["ws_fn"]:
        for key in ("S", "n", "C", "D", "H", "W", "planes_per_segment"):
            if key in sc:
                more = getattr(L, t["ws_fn"])(*t["ws_args"](dict(sc, **{key: sc[key] + 1})))
                assert more >= nbytes, (key, more, nbytes)
        assert getattr(L, t["ws_fn"])(*t["ws_args"](dict(sc, S=0))) == -1
    code, msg = _host_call(call, ws_short=1)
    assert code != 0 and t["too_small"] in msg, (call["id"], msg)
