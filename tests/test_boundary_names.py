"""Static proof of the drop-in boundary: every name the reference's CALLERS take from the six module names
this repo shadows (`helpers`, `evaluation`, `dataset`, `GaussianDiffusion`, `UNet`, `simplex`) is exported by the shim of
that name at the repo root -- or sits on the committed allow-list of names SURVEY section 2 puts out of scope.

The names come from tests/golden/boundary_names.json, recorded by tests/golden/make_golden.py (gen_boundary_names), which
parses the callers (`detection.py`, `diffusion_training.py`, `evaluation.py`, `generate_images.py`, and `GaussianDiffusion.py`
for what it takes from `simplex` / `evaluation` / `helpers`) with `ast`, never importing or executing them.  Three kinds of
use are recorded:
  * `from M import a, b`                         -> (M, a), (M, b)
  * `M.attr` after `import M`                    -> (M, attr)
  * `from helpers import *` + a free name        -> (helpers, name) for every name of the reference helpers' namespace the
                                                    importer loads without binding it itself (the leaked torch / os / json /
                                                    defaultdict included -- GaussianDiffusion.py:8 relies on them)
together with the reference helpers' public namespace and, for the two classes behind the boundary, the methods / attributes
the callers reach through their instances (`diff.detection_B`, `unet.load_state_dict`, ...).
"""
import importlib
import json
import os
import sys

from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODS = ("helpers", "evaluation", "dataset", "GaussianDiffusion", "UNet", "simplex")

# Names deliberately NOT provided, each with the SURVEY row that scopes it out.  Anything else missing is a failure.
ALLOW = {
    ("dataset", "AnomalousMRIDataset"): "SURVEY 2 row 6: private Edinburgh MRI data + cv2 / nibabel host I/O",
    ("dataset", "DAGM"): "SURVEY 2 row 6: DAGM texture dataset loader (cv2)",
    ("dataset", "MVTec"): "SURVEY 2 row 6: MVTec dataset loader (cv2)",
    ("dataset", "load_CIFAR10"): "SURVEY 2 row 6: torchvision CIFAR download",
    ("dataset", "load_image_mask"): "SURVEY 2 row 8: missing UPSTREAM too (detection.py:64 calls a function dataset.py never defines)",
    ("helpers", "torchvision"): "SURVEY 2 row 5: plotting dependency (make_grid); leaked by `import torchvision.utils`, used by no caller",
}

with open(os.path.join(GOLDEN, "boundary_names.json")) as _f:
    NAMES = json.load(_f)


def collect_uses():
    """-> {(module, name): [caller, ...]}"""
    uses = {(m, n): list(callers) for m, n, callers in NAMES["uses"]}
    assert all(m in MODS for m, _ in uses), "fixture names a module this repo does not shadow"
    return uses


def _shim(name):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    mod = importlib.import_module(name)
    assert os.path.dirname(os.path.abspath(mod.__file__)) == ROOT, f"`import {name}` did not resolve to this repo's shim: {mod.__file__}"
    return mod


def test_every_name_the_reference_callers_import_is_exported():
    uses = collect_uses()
    # the scan must see what SURVEY 8b lists, otherwise it proves nothing
    for must in (("helpers", "load_parameters"), ("helpers", "torch"),
                 ("helpers", "defaultdict_from_json"), ("helpers", "gridify_output"), ("evaluation", "testing"),
                 ("evaluation", "heatmap"), ("UNet", "update_ema_params"), ("simplex", "Simplex_CLASS"),
                 ("GaussianDiffusion", "get_beta_schedule"), ("dataset", "init_datasets"), ("dataset", "cycle")):
        assert must in uses, f"scan lost {must}"
    missing, stale_allow = [], []
    for (mod, name), callers in sorted(uses.items()):
        have = hasattr(_shim(mod), name)
        if (mod, name) in ALLOW:
            if have:
                stale_allow.append((mod, name))
            continue
        if not have:
            missing.append(f"{mod}.{name}  (used by {sorted(set(callers))})")
    assert not missing, "names the reference callers use but the shims do not export:\n  " + "\n  ".join(missing)
    assert not stale_allow, f"allow-listed names that ARE exported (drop them from ALLOW): {stale_allow}"
    unused = [k for k in ALLOW if k not in uses and k != ("helpers", "torchvision")]
    assert not unused, f"allow-list entries no caller uses: {unused}"


def test_star_import_of_helpers_hands_on_the_same_names():
    """`from helpers import *` must leak what upstream leaks (minus the allow-list): the shim's `__all__` covers the
    reference helpers' whole public namespace except its `main` stub."""
    ns = set(NAMES["helpers_namespace"]) - {"main"}
    shim = _shim("helpers")
    exported = set(getattr(shim, "__all__"))
    lost = {n for n in ns if n not in exported and ("helpers", n) not in ALLOW}
    assert not lost, f"upstream `from helpers import *` provides {sorted(lost)}; the shim's __all__ does not"
    scope = {}
    exec("from helpers import *", scope)
    for n in ns - {"torchvision"}:
        assert n in scope, n


def test_instance_members_the_callers_reach_exist():
    """Methods / attributes the callers use on the objects behind the boundary (variable names as upstream spells them)."""
    diff_names, unet_names = set(NAMES["diff_names"]), set(NAMES["unet_names"])
    assert {"forward_backward", "detection_B", "p_loss", "calc_total_vlb", "num_timesteps"} <= diff_names
    import numpy as np
    GD, UN = _shim("GaussianDiffusion"), _shim("UNet")
    d = GD.GaussianDiffusionModel([32, 32], GD.get_beta_schedule(1000, "linear"))
    lost = sorted(n for n in diff_names if not hasattr(d, n))
    assert not lost, f"GaussianDiffusionModel lacks {lost}"
    u = UN.UNetModel(32, 32)
    lost = sorted(n for n in unet_names if not hasattr(u, n))
    assert not lost, f"UNetModel lacks {lost}"
    assert np.isfinite(d.betas).all()
