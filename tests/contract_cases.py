"""What the fifteen workgroup-era metric and post-processing entry points read and write: the table, the arenas, the checker.

Shared by tests/test_contract_reference.py (CPU: the table, the cases, the checker on simulated calls, the host side of the
library) and tests/test_gpu_contract.py (the entry points themselves through the C ABI).  The other GPU tests reach these entry
points through anoddpm_amd.metrics, whose outputs and workspaces come from the caching allocator: a store one word outside a
buffer, a load one element outside a plane, an output element that is never written or a workspace that must be cleared cannot
fail a test there.  Here every buffer of a call is an ARENA inside an allocation of its own,

    [guard | segment 0 | gap | segment 1 | gap | segment 2 | guard]

with a guard of at least one segment stride + 4096 elements on either side (an index that is off by a segment or by a tile row
still lands inside the allocation; nothing is placed at the end of an allocation to make an overrun fault), odd gaps between
the segments of a strided input, and a fill that tells what happened to it:
  inputs     NaN in the gaps and guards of fp32 / fp64 inputs, 0x7f5a5a5a / 0x7f5a5a5a5a5a5a5a for int32 / int64.  An input that
             is only compared with a level (erode, components, distances) cannot see a NaN -- it is background, like everything
             outside the image -- so those inputs alternate NaN with +inf (foreground)
  outputs    a poison no kernel produces: fp32 0x7fc5a5a5, fp64 0x7ff8a5a5a5a5a5a5 (the kernels write the canonical NaN),
             integers 0xa5a5...; whatever still holds it was not written
  workspace  exactly the reported size between guards, 256-byte aligned, pre-filled by the caller of `build_arenas`
`check` compares the arenas before and after a call with the numpy restatements tests/*_cases.py already hold and names what it
finds (FINDINGS).  `simulate` is a numpy stand-in for the device that can plant one of DEFECTS, so that the checker itself is
tested without a GPU.

What this method cannot see: a stray LOAD whose value is discarded.  A load that lands inside a guard or a gap and influences no
output and no status word leaves no trace; only loads that are used (they change a result or raise a status bit) and all stores
are observable.

The global loads and stores of csrc/roc.hip, pro.hip, pro_shared.h, ssim.hip, surface.hip, postproc.hip, postproc3d.hip,
cc_shared.h and smooth.hip were read before the first run: every access through an argument pointer has the width of the
pointer's element type (no vector loads, no buffer loads), so odd segment strides are legal for every input.  The only accesses
wider than four bytes go to the workspace: anoddpm_pro_auc keeps the fp64 PRO values of the curve points at the start of each
segment's share of it and anoddpm_ssim its fp64 partial sums, so those two workspaces must be 8-byte aligned (`ws_align` in the
table, stated in the header); the others hold 32-bit words.

A new entry point registers itself with one TABLE entry (its struct, its workspace function, a classification of every pointer
field) and one `_<name>_cases` function in CASES; tests/test_contract_reference.py fails for a pointer field without one."""
import itertools

import numpy as np

import postproc3d_cases as p3c
import postproc_cases as ppc
import pr_cases as pc
import pro_cases as prc
import roc_cases as rc
import smooth_cases as smc
import ssim_cases as ssc
import surface_cases as sfc

S = 3                                                        # segments of every case; the middle one differs in kind
GAP = 7                                                      # elements between the segments of a strided input (odd)
GUARD_EXTRA = 4096
WS_ALIGN = 256
ROC_NAN, ROC_INF, ROC_NEGATIVE, ROC_BAD_MASK, ROC_TRUNCATED = 1, 2, 4, 8, 16          # checked against the header by the reference test
SURFACE_EMPTY_PRED = 1

FINDINGS = ("guard_written", "input_modified", "gap_written", "unwritten_output", "wrote_outside_written_set", "wrong_value", "status",
            "workspace_dependent")

IN_FILL = {"f4": 0x7fc00000, "f8": 0x7ff8000000000000, "i4": 0x7f5a5a5a, "i8": 0x7f5a5a5a5a5a5a5a}
IN_FILL_ABOVE = 0x7f800000                                   # +inf: the second fill of an input that is compared with a level
POISON = {"f4": 0x7fc5a5a5, "f8": 0x7ff8a5a5a5a5a5a5, "i4": 0xa5a5a5a5, "i8": 0xa5a5a5a5a5a5a5a5}
WS_GUARD_BYTE = 0x5a
WS_LEFT_BYTE = 0x3c                                          # what `simulate` leaves in the workspace


# ---------------------------------------------------------------------------------------------------- the table
def inp(dtype, extent, stride=None, zero_ok=False, level=False):
    """An input: element type, elements per segment (text), the struct's stride field, whether stride 0 (one operand for every
    segment) is allowed, whether the kernel only compares it with a level."""
    return {"kind": "in", "dtype": dtype, "extent": extent, "stride": stride, "zero_ok": zero_ok, "level": level}


def out(dtype, shape, written="all"):
    """An output: element type, shape (text) and its written set: "all", or "curve" = [s][0 .. min(curve_len[s], curve_cap))."""
    return {"kind": "out", "dtype": dtype, "shape": shape, "written": written}


def opt(spec):
    return dict(spec, optional=True)


WS = {"kind": "ws"}


def _cdiv(a, b):
    return -(-a // b)


TABLE = {
    "roc_auc": {
        "struct": "anoddpm_roc_args", "status": "status", "ws_align": 4,
        "ws_fn": "anoddpm_roc_workspace_bytes", "ws_args": lambda c: (c["S"], c["n"]), "ws_min": lambda c: 12 * c["S"] * (c["n"] + 1),
        "too_small": b"roc_auc: workspace too small",
        "fields": {"score": inp("f4", "n", "score_stride"), "mask": inp("f4", "n", "mask_stride", zero_ok=True), "workspace": WS,
                   "auc": out("f8", "[S]"), "counts": out("i8", "[S][4]"), "status": out("i4", "[S]"),
                   "curve_fps": opt(out("i4", "[S][curve_cap]", "curve")), "curve_tps": opt(out("i4", "[S][curve_cap]", "curve")),
                   "curve_thr": opt(out("f4", "[S][curve_cap]", "curve")), "curve_len": opt(out("i4", "[S]")),
                   "ap": opt(out("f8", "[S]")), "best_dice": opt(out("f8", "[S]")), "best_thr": opt(out("f4", "[S]")),
                   "best_counts": opt(out("i8", "[S][2]"))}},
    "pro_auc": {
        "struct": "anoddpm_pro_args", "status": "status", "ws_align": 8,          # fp64 PRO values at the start of a segment's share
        "ws_fn": "anoddpm_pro_workspace_bytes", "ws_args": lambda c: (c["S"], c["planes_per_segment"] * c["H"] * c["W"]),
        "ws_min": lambda c: 24 * c["S"] * c["planes_per_segment"] * c["H"] * c["W"],
        "too_small": b"pro_auc: workspace too small",
        "fields": {"score": inp("f4", "m*H*W", "score_stride"), "area": inp("i4", "m*H*W", "area_stride", zero_ok=True),
                   "region_counts": inp("i8", "S*m, or m when area_stride is 0"), "mask": opt(inp("f4", "m*H*W", "mask_stride", zero_ok=True)),
                   "workspace": WS, "aupro": out("f8", "[S]"), "counts": out("i8", "[S][4]"), "status": out("i4", "[S]"),
                   "curve_fps": opt(out("i4", "[S][curve_cap]", "curve")), "curve_pro": opt(out("f8", "[S][curve_cap]", "curve")),
                   "curve_thr": opt(out("f4", "[S][curve_cap]", "curve")), "curve_len": opt(out("i4", "[S]"))}},
    "component_areas": {
        "struct": "anoddpm_component_areas_args", "status": None, "ws_align": 4,
        "ws_fn": "anoddpm_small_components_workspace_bytes", "ws_args": lambda c: (c["S"], c["H"], c["W"]),
        "ws_min": lambda c: 8 * c["S"] * c["H"] * c["W"], "too_small": b"component_areas: workspace too small",
        "fields": {"src": inp("f4", "H*W", "src_stride", level=True), "area": out("i4", "[S][H][W]"), "counts": out("i8", "[S]"), "workspace": WS}},
    "ssim": {
        "struct": "anoddpm_ssim_args", "status": None, "ws_align": 8,
        "ws_fn": "anoddpm_ssim_workspace_bytes", "ws_args": lambda c: (c["S"], c["C"], c["H"], c["W"]),
        "ws_min": lambda c: 8 * c["S"] * c["C"] * _cdiv(c["H"], 16) * _cdiv(c["W"], 32), "too_small": b"ssim: workspace too small",
        "fields": {"real": inp("f4", "C*H*W", "real_stride", zero_ok=True), "recon": inp("f4", "C*H*W", "recon_stride"), "workspace": WS,
                   "mssim": out("f8", "[S]"), "map": opt(out("f4", "[S][C][H][W]"))}},
    "distance_transform": {
        "struct": "anoddpm_distance_args", "status": None, "ws_align": 4,
        "ws_fn": None, "ws_args": None, "ws_min": lambda c: 4 * c["S"] * c["H"] * c["W"],            # the header's formula
        "too_small": b"distance_transform: workspace too small",
        "fields": {"src": inp("f4", "H*W", "src_stride", level=True), "sq": out("i4", "[S][H][W]"), "dist": opt(out("f8", "[S][H][W]")),
                   "workspace": WS}},
    "surface_distance": {
        "struct": "anoddpm_surface_args", "status": "status", "ws_align": 4,
        "ws_fn": "anoddpm_surface_workspace_bytes", "ws_args": lambda c: (c["S"], c["H"], c["W"]),
        "ws_min": lambda c: 16 * c["S"] * c["H"] * c["W"], "too_small": b"surface_distance: workspace too small",
        "fields": {"pred": inp("f4", "H*W", "pred_stride", level=True), "ref": inp("f4", "H*W", "ref_stride", zero_ok=True, level=True),
                   "workspace": WS, "counts": out("i4", "[S][2]"), "max2": out("i4", "[S][2]"), "mean": out("f8", "[S][2]"),
                   "p95": out("f8", "[S][3]"), "status": out("i4", "[S]")}},
    "median2d": {
        "struct": "anoddpm_median_args", "status": "status", "ws_fn": None, "ws_min": None,
        "fields": {"src": inp("f4", "H*W", "src_stride"), "roi": opt(inp("f4", "H*W", "roi_stride", zero_ok=True)),
                   "dst": out("f4", "[S][H][W]"), "status": out("i4", "[S]")}},
    "erode2d": {
        "struct": "anoddpm_erode_args", "status": None, "ws_fn": None, "ws_min": None,
        "fields": {"src": inp("f4", "H*W", "src_stride", level=True), "dst": out("f4", "[S][H][W]")}},
    "small_components": {
        "struct": "anoddpm_components_args", "status": None, "ws_align": 4,
        "ws_fn": "anoddpm_small_components_workspace_bytes", "ws_args": lambda c: (c["S"], c["H"], c["W"]),
        "ws_min": lambda c: 8 * c["S"] * c["H"] * c["W"], "too_small": b"small_components: workspace too small",
        "fields": {"src": inp("f4", "H*W", "src_stride", level=True), "dst": out("f4", "[S][H][W]"), "counts": out("i8", "[S][2]"), "workspace": WS}},
    "gauss2d": {
        "struct": "anoddpm_gauss_args", "status": None, "ws_fn": None, "ws_min": None,
        "fields": {"src": inp("f4", "H*W", "src_stride"), "dst": out("f4", "[S][H][W]"), "w": inp("f8", "radius + 1, one table")}},
    "map_scores": {
        "struct": "anoddpm_map_scores_args", "status": "status", "ws_fn": None, "ws_min": None,
        "fields": {"src": inp("f4", "n", "src_stride"), "max": out("f4", "[S]"), "mean": out("f8", "[S]"), "topk_mean": out("f8", "[S]"),
                   "status": out("i4", "[S]")}},
    "median3d": {
        "struct": "anoddpm_median3d_args", "status": "status", "ws_fn": None, "ws_min": None,
        "fields": {"src": inp("f4", "D*H*W", "src_stride"), "roi": opt(inp("f4", "H*W or D*H*W (roi_slice_stride)", "roi_stride", zero_ok=True)),
                   "dst": out("f4", "[S][D][H][W]"), "status": out("i4", "[S]")}},
    "erode3d": {
        "struct": "anoddpm_erode3d_args", "status": None, "ws_fn": None, "ws_min": None,
        "fields": {"src": inp("f4", "D*H*W", "src_stride", level=True), "dst": out("f4", "[S][D][H][W]")}},
    "small_components3d": {
        "struct": "anoddpm_components3d_args", "status": None, "ws_align": 4,
        "ws_fn": "anoddpm_components3d_workspace_bytes", "ws_args": lambda c: (c["S"], c["D"], c["H"], c["W"]),
        "ws_min": lambda c: 8 * c["S"] * c["D"] * c["H"] * c["W"], "too_small": b"small_components3d: workspace too small",
        "fields": {"src": inp("f4", "D*H*W", "src_stride", level=True), "dst": out("f4", "[S][D][H][W]"), "counts": out("i8", "[S][2]"),
                   "workspace": WS}},
    "component_areas3d": {
        "struct": "anoddpm_component_areas3d_args", "status": None, "ws_align": 4,
        "ws_fn": "anoddpm_components3d_workspace_bytes", "ws_args": lambda c: (c["S"], c["D"], c["H"], c["W"]),
        "ws_min": lambda c: 8 * c["S"] * c["D"] * c["H"] * c["W"], "too_small": b"component_areas3d: workspace too small",
        "fields": {"src": inp("f4", "D*H*W", "src_stride", level=True), "area": out("i4", "[S][D][H][W]"), "counts": out("i8", "[S]"),
                   "workspace": WS}},
}
ENTRY_POINTS = tuple(TABLE)


def has_workspace(entry):
    return "workspace" in TABLE[entry]["fields"]


# ---------------------------------------------------------------------------------------------------- arenas
def _up(x, m):
    return (x + m - 1) // m * m


class Arena:
    """One buffer of a call inside an allocation of its own; `bits` is the whole allocation as unsigned words."""

    def __init__(self, name, kind, dtype, n, segs=1, level=False):
        self.name, self.kind, self.item, self.n, self.segs = name, kind, np.dtype(dtype), int(n), int(segs)
        self.word = np.dtype("u%d" % self.item.itemsize)
        self.stride = self.n + GAP if segs > 1 else self.n
        if kind == "ws":
            self.guard = _up(self.n + 4 * GUARD_EXTRA, WS_ALIGN)
        else:
            self.guard = _up(self.stride + GUARD_EXTRA, 64)          # a multiple of 256 bytes: element 0 keeps the allocation's alignment
        size = 2 * self.guard + (self.segs - 1) * self.stride + self.n
        code = "f8" if dtype == "f8" else dtype
        if kind == "ws":
            self.bits = np.full(size, WS_GUARD_BYTE, np.uint8)
        elif kind == "in":
            self.bits = np.full(size, IN_FILL[code], self.word)
            if level:
                self.bits[1::2] = IN_FILL_ABOVE
        else:
            self.bits = np.full(size, POISON[code], self.word)

    def lo(self, s=0):
        return self.guard + s * self.stride

    def seg(self, s=0):
        return slice(self.lo(s), self.lo(s) + self.n)

    def put(self, s, values):
        v = np.ascontiguousarray(values, self.item).reshape(-1)
        assert v.size == self.n, (self.name, v.size, self.n)
        self.bits[self.seg(s)] = v.view(self.word)

    def get(self, s=0):
        return self.bits[self.seg(s)].view(self.item)

    def regions(self):
        """Boolean masks over `bits`: (inside a segment, inside a gap, inside a guard)."""
        seg = np.zeros(self.bits.size, bool)
        for s in range(self.segs):
            seg[self.seg(s)] = True
        guard = np.zeros(self.bits.size, bool)
        guard[:self.guard] = True
        guard[self.bits.size - self.guard:] = True
        return seg, ~seg & ~guard, guard

    @property
    def offset_bytes(self):
        return self.guard * self.item.itemsize

    def copy(self, bits=None):
        c = Arena.__new__(Arena)
        c.__dict__.update(self.__dict__)
        c.bits = self.bits.copy() if bits is None else np.ascontiguousarray(bits).view(self.bits.dtype).reshape(self.bits.shape).copy()
        return c


def workspace_bytes(call, L=None):
    """The workspace of `call`: what the library reports, or (L None: simulated calls) the header's formula."""
    t = TABLE[call["entry"]]
    if not has_workspace(call["entry"]):
        return None
    if L is None or t["ws_fn"] is None:
        return t["ws_min"](call["scalars"])
    return int(getattr(L, t["ws_fn"])(*t["ws_args"](call["scalars"])))


def build_arenas(call, ws_bytes=None, ws_fill=0, inputs=None):
    """field -> Arena for every pointer of the call that is not NULL.  ws_fill: a byte value, or bytes that are repeated /
    cut to the workspace's size (what another call left behind)."""
    t = TABLE[call["entry"]]
    inputs = call["inputs"] if inputs is None else inputs
    arenas = {}
    for name, x in inputs.items():
        f = t["fields"][name]
        x = np.asarray(x)
        if x.ndim == 2:
            a = Arena(name, "in", f["dtype"], x.shape[1], x.shape[0], f["level"])
            for s in range(x.shape[0]):
                a.put(s, x[s])
        else:                                                # one operand for every segment (stride 0), or a table without a stride
            assert f["zero_ok"] or f["stride"] is None, name
            a = Arena(name, "in", f["dtype"], x.size, 1, f["level"])
            a.put(0, x)
        arenas[name] = a
    for name, e in expected_of(call).items():
        arenas[name] = Arena(name, "out", t["fields"][name]["dtype"], e["value"].size)
    if has_workspace(call["entry"]):
        n = workspace_bytes(call) if ws_bytes is None else ws_bytes
        a = Arena("workspace", "ws", "u1", n)
        if isinstance(ws_fill, (bytes, bytearray, np.ndarray)):
            left = np.frombuffer(bytes(ws_fill), np.uint8)
            a.bits[a.seg()] = np.resize(left, n) if left.size else 0
        else:
            a.bits[a.seg()] = ws_fill
        arenas["workspace"] = a
    return arenas


def fill_struct(call, arenas, base, ws_short=0):
    """The argument struct of the call: `base[field]` is the address of the arena's allocation.  ws_short: bytes taken off
    workspace_bytes (a call that must be refused)."""
    from anoddpm_amd import _lib
    t = TABLE[call["entry"]]
    a = getattr(_lib, _lib._PYNAME[t["struct"]])()
    for k, v in call["scalars"].items():
        setattr(a, k, v)
    for name, ar in arenas.items():
        setattr(a, name, base[name] + ar.offset_bytes)
        f = t["fields"][name]
        if f["kind"] == "in" and f["stride"]:
            setattr(a, f["stride"], ar.stride if ar.segs > 1 else 0)
    if "workspace" in arenas:
        a.workspace_bytes = arenas["workspace"].n - ws_short
    return a


# ---------------------------------------------------------------------------------------------------- expected values
def _e(value, dtype, rule="bits", written=None):
    value = np.ascontiguousarray(value, dtype)
    return {"value": value, "rule": rule, "written": np.ones(value.shape, bool) if written is None else written}


def expected_of(call):
    if "_expected" not in call:
        call["_expected"] = call["restate"](call, call["inputs"])
    return call["_expected"]


def _seg(x, s):
    x = np.asarray(x)
    return x[s] if x.ndim == 2 else x


def _score_status(v):
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        return (ROC_NAN if np.isnan(v).any() else 0) | (ROC_INF if np.isinf(v).any() else 0) | (ROC_NEGATIVE if (v < 0).any() else 0)


def _mask_status(m):
    m = np.asarray(m, np.float32)
    return 0 if ((m == 0) | (m == 1)).all() else ROC_BAD_MASK


def _curve(rows, cap, dtype):
    """rows: one array of points per segment -> ([S][cap] values, written mask, lengths)."""
    value = np.zeros((len(rows), cap), dtype)
    written = np.zeros((len(rows), cap), bool)
    for s, r in enumerate(rows):
        k = min(len(r), cap)
        value[s, :k] = np.asarray(r)[:k]
        written[s, :k] = True
    return value, written


def _restate_roc(call, inputs):
    c, v = call["scalars"], call["variant"]
    n, cap = c["n"], c.get("curve_cap", 0)
    auc, counts, status = np.zeros(S), np.zeros((S, 4), np.int64), np.zeros(S, np.int32)
    ap, dice, thr, bc = np.zeros(S), np.zeros(S), np.zeros(S, np.float32), np.zeros((S, 2), np.int64)
    fps, tps, cth, skip = [], [], [], set()
    for s in range(S):
        score, mask = _seg(inputs["score"], s), _seg(inputs["mask"], s)
        status[s] = _score_status(score) | _mask_status(mask)
        if status[s]:
            skip.add(s)
            fps.append([]), tps.append([]), cth.append([])
            continue
        r = rc.roc_numpy(mask, score)
        auc[s], counts[s] = r["auc"], (r["P"], r["N"], r["twoU"], r["R"])
        p = pc.pr_numpy(mask, score) if v["extra"] or v["all"] else None
        pts = p if v["all"] else r
        fps.append(pts["fps"]), tps.append(pts["tps"]), cth.append(pts["thresholds"])
        if v["curve"] and len(pts["fps"]) > cap:
            status[s] |= ROC_TRUNCATED
        if p is not None:
            ap[s], dice[s], thr[s], bc[s] = p["ap"], p["best_dice"], p["best_threshold"], (p["best_tp"], p["best_fp"])
    out_ = {"auc": _e(auc, "f8", rc.auc_tolerance(n)), "counts": _e(counts, "i8"), "status": _e(status, "i4")}
    if v["curve"]:
        for name, rows, dt in (("curve_fps", fps, "i4"), ("curve_tps", tps, "i4"), ("curve_thr", cth, "f4")):
            value, written = _curve(rows, cap, dt)
            out_[name] = _e(value, dt, written=written)
        out_["curve_len"] = _e([len(r) for r in fps], "i4")
    if v["extra"]:
        out_.update(ap=_e(ap, "f8"), best_dice=_e(dice, "f8"), best_thr=_e(thr, "f4"), best_counts=_e(bc, "i8"))
    call["skip"] = skip
    return out_


def _restate_pro(call, inputs):
    c = call["scalars"]
    m, H, W, cap = c["planes_per_segment"], c["H"], c["W"], c.get("curve_cap", 0)
    aupro, counts, status = np.zeros(S), np.zeros((S, 4), np.int64), np.zeros(S, np.int32)
    fps, pro, thr, skip = [], [], [], set()
    for s in range(S):
        score, mask = _seg(inputs["score"], s), _seg(call["aux"]["mask"], s).reshape(m, H, W)
        status[s] = _score_status(score) | (_mask_status(_seg(inputs["mask"], s)) if "mask" in inputs else 0)
        if status[s]:
            skip.add(s)
            fps.append([]), pro.append([]), thr.append([])
            continue
        r = prc.pro_fp64(mask, score, c["limit"], call["aux"]["connectivity"])
        aupro[s], counts[s] = r["aupro"], (r["K"], r["N"], r["P"], r["fps"].size)
        fps.append(r["fps"]), pro.append(r["pro"]), thr.append(r["thresholds"])
        if call["variant"]["curve"] and r["fps"].size > cap:
            status[s] |= ROC_TRUNCATED
    out_ = {"aupro": _e(aupro, "f8"), "counts": _e(counts, "i8"), "status": _e(status, "i4")}
    if call["variant"]["curve"]:
        for name, rows, dt in (("curve_fps", fps, "i4"), ("curve_pro", pro, "f8"), ("curve_thr", thr, "f4")):
            value, written = _curve(rows, cap, dt)
            out_[name] = _e(value, dt, written=written)
        out_["curve_len"] = _e([len(r) for r in fps], "i4")
    call["skip"] = skip
    return out_


def _planes(call, inputs, name="src"):
    c = call["scalars"]
    shape = ((c["D"],) if "D" in c else ()) + (c["H"], c["W"])
    return [np.asarray(_seg(inputs[name], s), np.float32).reshape(shape) for s in range(S)]


def _areas2d(plane, connectivity, level):
    with np.errstate(invalid="ignore"):
        b = plane > np.float32(level)
    lab = ppc.labels_numpy(b, connectivity)
    sizes = np.bincount(lab[lab >= 0], minlength=lab.size)
    return np.where(b, sizes[np.maximum(lab, 0)], 0).astype(np.int32), int((sizes > 0).sum())


def _restate_component_areas(call, inputs):
    c = call["scalars"]
    r = [_areas2d(p, c["connectivity"], c["level"]) for p in _planes(call, inputs)]
    return {"area": _e(np.stack([a for a, _ in r]), "i4"), "counts": _e([k for _, k in r], "i8")}


def _restate_ssim(call, inputs):
    c, window = call["scalars"], call["aux"]["window"]
    shape = (c["C"], c["H"], c["W"])
    r = [ssc.ssim_kernel_numpy(_seg(inputs["real"], s).reshape(shape), _seg(inputs["recon"], s).reshape(shape), window, c["data_range"])
         for s in range(S)]
    exact = window != "gauss"                                # the rule of tests/test_gpu_ssim.py: bit for bit for the uniform windows
    out_ = {"mssim": _e([v for v, _ in r], "f8", "bits" if exact else ssc.MSSIM_TOL)}
    if call["variant"]["map"]:
        out_["map"] = _e(np.stack([m for _, m in r]).astype(np.float32 if exact else np.float64), "f4", "bits" if exact else ssc.MAP_TOL)
        if not exact:
            out_["map"]["want64"] = np.stack([m for _, m in r])
    return out_


def _restate_distance(call, inputs):
    c = call["scalars"]
    sq = np.stack([sfc.edt2_brute(sfc.foreground(p, c["level"])) for p in _planes(call, inputs)])
    out_ = {"sq": _e(sq, "i4")}
    if call["variant"]["dist"]:
        with np.errstate(invalid="ignore"):
            out_["dist"] = _e(np.where(sq < 0, np.inf, np.sqrt(np.maximum(sq, 0).astype(np.float64))), "f8")
    return out_


def _restate_surface(call, inputs):
    c = call["scalars"]
    pred, ref = _planes(call, inputs, "pred"), _planes(call, inputs, "ref")
    want = [sfc.surface_fp64(sfc.foreground(p, c["level"]), sfc.foreground(r, c["level"])) for p, r in zip(pred, ref)]
    return {"counts": _e([w["counts"] for w in want], "i4"), "max2": _e([w["max2"] for w in want], "i4"),
            "mean": _e([w["mean"] for w in want], "f8"), "p95": _e([w["p95"] for w in want], "f8"),
            "status": _e([w["status"] for w in want], "i4")}


def _roi_of(call, inputs, s, shape):
    if "roi" not in inputs:
        return None
    roi = np.asarray(_seg(inputs["roi"], s), np.float32)
    return np.broadcast_to(roi.reshape((-1,) + shape[-2:]), shape) if roi.size != int(np.prod(shape)) else roi.reshape(shape)


def _restate_median(call, inputs):
    c = call["scalars"]
    planes = _planes(call, inputs)
    dst, status, skip = np.zeros((S,) + planes[0].shape, np.float32), np.zeros(S, np.int32), set()
    for s, p in enumerate(planes):
        roi = _roi_of(call, inputs, s, p.shape)
        status[s] = _score_status(p) | (0 if roi is None else _mask_status(roi))
        if status[s]:
            skip.add(s)
            continue
        dst[s] = p3c.median3d_numpy(p, c["k"]) if "D" in c else ppc.median_numpy(p, c["k"])
        if roi is not None:
            dst[s] = np.where(roi == 0, np.float32(0), dst[s])
    call["skip"] = skip
    return {"dst": _e(dst, "f4"), "status": _e(status, "i4")}


def _restate_erode(call, inputs):
    c = call["scalars"]
    f = p3c.erode3d_numpy if "D" in c else ppc.erode_numpy
    with np.errstate(invalid="ignore"):
        return {"dst": _e(np.stack([f(p, c["n"], c["level"]) for p in _planes(call, inputs)]), "f4")}


def _restate_components(call, inputs):
    c = call["scalars"]
    f = p3c.components3d_numpy if "D" in c else ppc.components_numpy
    with np.errstate(invalid="ignore"):
        r = [f(p, c["min_size"], c["connectivity"], c["level"]) for p in _planes(call, inputs)]
    return {"dst": _e(np.stack([d for d, _ in r]), "f4"), "counts": _e([k for _, k in r], "i8")}


def _restate_areas3d(call, inputs):
    c = call["scalars"]
    with np.errstate(invalid="ignore"):
        r = [p3c.areas3d_numpy(p, c["connectivity"], c["level"]) for p in _planes(call, inputs)]
    return {"area": _e(np.stack([a for a, _ in r]), "i4"), "counts": _e([k for _, k in r], "i8")}


def _restate_gauss(call, inputs):
    # the weight table is an operand: the restatement forms its own from sigma, and a table that differs is a defect of the CASE
    table = smc.weights_numpy(call["aux"]["sigma"])[:call["scalars"]["radius"] + 1]
    assert np.array_equal(np.asarray(inputs["w"]).view(np.uint64), table.view(np.uint64))
    with np.errstate(invalid="ignore"):
        return {"dst": _e(np.stack([smc.gaussian_numpy(p, call["aux"]["sigma"]) for p in _planes(call, inputs)]), "f4")}


def _restate_scores(call, inputs):
    c = call["scalars"]
    mx, mean, topk, status, skip = np.zeros(S, np.float32), np.zeros(S), np.zeros(S), np.zeros(S, np.int32), set()
    for s in range(S):
        v = _seg(inputs["src"], s)
        status[s] = _score_status(v)
        if status[s]:
            skip.add(s)
            continue
        mx[s], mean[s], topk[s] = smc.scores_numpy(v, c["k"])
    call["skip"] = skip
    return {"max": _e(mx, "f4"), "mean": _e(mean, "f8"), "topk_mean": _e(topk, "f8"), "status": _e(status, "i4")}


# ---------------------------------------------------------------------------------------------------- cases
def _call(entry, cid, scalars, inputs, restate, variant=None, aux=None):
    return {"entry": entry, "id": cid, "scalars": dict(scalars, S=S), "inputs": inputs, "restate": restate, "variant": variant or {},
            "aux": aux or {}, "skip": set()}


def _rng(*key):
    return np.random.default_rng([7919] + [int(k) for k in key])


def _roc_cases():
    cases = []
    # (kernel / curve mode, curve_cap small, mask shared): the plain kernel, the EXTRA one (ap + best_*) and CURVE_ALL
    plans = list(itertools.product(("plain", "extra", "all"), (False, True), (False, True)))
    for n in (1, 63, 64, 65, 1025):
        for i, (mode, small, shared) in enumerate(plans):
            if small and n == 1:
                continue                                     # one point: nothing to truncate
            rng = _rng(1, n, i)
            score = rng.random((S, n)).astype(np.float32)
            if n != 63:
                score[0] = np.round(score[0] * 16) / 16      # ties; n63 keeps every score distinct: R = n
            mask = (rng.random((S, n)) < 0.4).astype(np.float32)
            if n > 1:
                mask[0, :2], mask[2, :2] = (0, 1), (1, 0)    # both classes in the outer segments
            if shared:
                mask = mask[0]
                score[1] = np.float32(0.25)                  # the middle segment: one run
            else:
                mask[1] = 0                                  # the middle segment: P = 0
            cap = 2 if small else max(n, 2)
            sc = {"n": n, "curve_cap": cap, "curve_mode": 1 if mode == "all" else 0}
            variant = {"curve": True, "extra": mode != "plain", "all": mode == "all", "small": small}
            cases.append(_call("roc_auc", f"n{n}-{mode}-cap{cap}-{'shared' if shared else 'own'}mask", sc, {"score": score, "mask": mask},
                               _restate_roc, variant))
    rng = _rng(1, 99)
    score, mask = rng.random((S, 65)).astype(np.float32), (rng.random((S, 65)) < 0.5).astype(np.float32)
    score[1, 40] = np.nan
    cases.append(_call("roc_auc", "n65-nocurve-nan-middle", {"n": 65, "curve_mode": 0}, {"score": score, "mask": mask}, _restate_roc,
                       {"curve": False, "extra": False, "all": False, "small": False}))
    return cases


def _pro_masks(rng, m, H, W):
    """[S][m][H][W] 0 / 1 with a few regions per plane and a background; segment 1 is left to the caller."""
    mask = np.zeros((S, m, H, W), np.float32)
    for s in range(S):
        for p in range(m):
            mask[s, p, 1:3, 1 + s:3 + s] = 1
            mask[s, p, H - 2, W - 3 + p:W - 1 + p] = 1
            mask[s, p, rng.integers(0, H), rng.integers(0, W)] = 1
    return mask


def _pro_cases():
    cases = []
    plans = list(itertools.product((False, True), (True, False), (False, True)))                       # area shared, with mask, cap small
    for (H, W), m in itertools.product(((8, 8), (5, 13)), (1, 2)):
        for i, (shared, with_mask, small) in enumerate(plans):
            rng = _rng(2, H, W, m, i)
            n = m * H * W
            mask = _pro_masks(rng, m, H, W)
            score = rng.permutation(S * n).reshape(S, n).astype(np.float32) / np.float32(S * n) if (H, W) == (8, 8) else \
                (np.round(rng.random((S, n)) * 32) / 32).astype(np.float32)
            score = score + mask.reshape(S, n) * np.float32(0.25 if (H, W) == (5, 13) else 0)
            if shared:
                mask = mask[0]
                score[1] = np.float32(0.5)                   # the middle segment: one curve point
            else:
                mask[1] = 0                                  # the middle segment: no region (K = 0)
            cases.append(_pro_call(f"{H}x{W}-m{m}-{'shared' if shared else 'own'}area-{'mask' if with_mask else 'nomask'}-cap{3 if small else n}",
                                   mask, score, m, H, W, with_mask, 3 if small else n))
    rng = _rng(2, 99)
    mask = _pro_masks(rng, 1, 5, 13)
    score = rng.random((S, 65)).astype(np.float32)
    score[1, 7] = np.float32(-0.5)
    cases.append(_pro_call("5x13-m1-ownarea-mask-nocurve-negative-middle", mask, score, 1, 5, 13, True, None))
    return cases


def _pro_call(cid, mask, score, m, H, W, with_mask, cap, connectivity=2):
    n = m * H * W
    flat = mask.reshape(-1, m, H, W)                         # [S or 1][m][H][W]
    reg = [prc.regions(f, connectivity) for f in flat]
    area = np.stack([a.reshape(n) for a, _ in reg]).astype(np.int32)
    counts = np.concatenate([k for _, k in reg]).astype(np.int64)
    per_segment = mask.ndim == 4
    inputs = {"score": score, "area": area if per_segment else area[0], "region_counts": counts}
    if with_mask:
        inputs["mask"] = mask.reshape(S, n) if per_segment else mask.reshape(n)
    sc = {"planes_per_segment": m, "H": H, "W": W, "limit": 0.3}
    if cap is not None:
        sc["curve_cap"] = cap
    return _call("pro_auc", cid, sc, inputs, _restate_pro, {"curve": cap is not None},
                 {"mask": mask.reshape(S, n) if per_segment else mask.reshape(n), "connectivity": connectivity})


def _blobs(rng, shape, density=0.45):
    """fp32 planes in [0, 1) whose part above 0.5 makes components of many sizes; the middle one is left to the caller."""
    x = rng.random((S,) + shape).astype(np.float32)
    return np.where(x < density, x / np.float32(density) * np.float32(0.5) + np.float32(0.5), x * np.float32(0.5)).astype(np.float32)


def _smooth_blobs(rng, shape):
    """fp32 planes in [0, 1] whose part above 0.5 is a few blobs some pixels across: borders that lie several pixels apart."""
    from scipy import ndimage
    x = np.stack([ndimage.gaussian_filter(rng.random(shape), 1.5) for _ in range(S)])
    lo, hi = x.min(axis=(1, 2), keepdims=True), x.max(axis=(1, 2), keepdims=True)
    return ((x - lo) / (hi - lo)).astype(np.float32)


def _flat(x):
    return np.ascontiguousarray(x).reshape(S, -1)


def _component_areas_cases():
    cases = []
    for conn in (1, 2):
        x = _blobs(_rng(3, conn), (17, 33))
        x[1] = np.float32(0.25)                              # the middle plane: no foreground
        cases.append(_call("component_areas", f"17x33-c{conn}-empty-middle", {"H": 17, "W": 33, "connectivity": conn, "level": 0.5},
                           {"src": _flat(x)}, _restate_component_areas))
    for H, W in ((8, 8), (5, 13)):                           # the masks of the PRO cases: what feeds anoddpm_pro_auc
        mask = _pro_masks(_rng(2, H, W, 1, 0), 1, H, W)
        mask[1] = 0
        cases.append(_call("component_areas", f"{H}x{W}-c2-pro-masks", {"H": H, "W": W, "connectivity": 2, "level": 0.0},
                           {"src": _flat(mask)}, _restate_component_areas))
    return cases


def _ssim_cases():
    cases = []
    C, H, W = 2, 17, 33
    for i, (window, shared, want_map) in enumerate(itertools.product((3, 15, "gauss"), (False, True), (True, False))):
        rng = _rng(4, i)
        real = (rng.random((S, C, H, W)) * 2 - 1).astype(np.float32)
        recon = np.clip(real + (rng.random((S, C, H, W)) - 0.5).astype(np.float32) * np.float32(0.5), -1, 1).astype(np.float32)
        if shared:
            real = real[0]
            recon[1] = np.float32(0.125)                     # the middle segment: a constant image
        else:
            recon[1] = real[1]                               # the middle segment: identical images
        win = ssc.win_of(window)
        sc = {"C": C, "H": H, "W": W, "win": win, "mode": 1 if window == "gauss" else 0, "data_range": ssc.DATA_RANGE, "K1": ssc.K1,
              "K2": ssc.K2, "cn": 1.0 if window == "gauss" else win * win / (win * win - 1.0)}
        cases.append(_call("ssim", f"win{window}-{'shared' if shared else 'own'}real-{'map' if want_map else 'nomap'}", sc,
                           {"real": real.reshape(-1) if shared else _flat(real), "recon": _flat(recon)}, _restate_ssim,
                           {"map": want_map}, {"window": window}))
    return cases


def _distance_cases():
    cases = []
    for H, W, dist in ((9, 33, True), (9, 33, False), (1, 4100, True)):
        x = (_rng(5, H, W).random((S, H, W)) * np.float32(0.9) + np.float32(0.05)).astype(np.float32)
        if W == 4100:
            x[:] = 1
            x[0, 0, 5] = x[0, 0, 4000] = x[2, 0, 2050] = 0   # distances far beyond one workgroup's columns
        x[1] = 1                                             # the middle plane: no background (sq -1, dist +inf)
        cases.append(_call("distance_transform", f"{H}x{W}-{'dist' if dist else 'nodist'}-allfg-middle", {"H": H, "W": W, "level": 0.25},
                           {"src": _flat(x)}, _restate_distance, {"dist": dist}))
    return cases


def _surface_cases():
    cases = []
    for shared in (False, True):
        rng = _rng(6, shared)
        pred, ref = _smooth_blobs(rng, (12, 19)), _smooth_blobs(rng, (12, 19))
        pred[1] = np.float32(0.125)                          # the middle pair: an empty prediction
        cases.append(_call("surface_distance", f"12x19-{'shared' if shared else 'own'}ref-emptypred-middle", {"H": 12, "W": 19, "level": 0.5},
                           {"pred": _flat(pred), "ref": ref[0].reshape(-1) if shared else _flat(ref)}, _restate_surface))
    return cases


def _median_cases():
    cases = []
    H, W = 17, 33
    for k, with_roi in itertools.product((3, 7), (True, False)):
        rng = _rng(7, k, with_roi)
        x = (np.round(rng.random((S, H, W)) * 64) / 64).astype(np.float32)
        x[1] = np.float32(0.375)                             # the middle plane: constant
        inputs = {"src": _flat(x)}
        if with_roi:
            inputs["roi"] = (rng.random(H * W) < 0.7).astype(np.float32)
        cases.append(_call("median2d", f"17x33-k{k}-{'sharedroi' if with_roi else 'noroi'}", {"H": H, "W": W, "k": k}, inputs, _restate_median))
    x = _rng(7, 99).random((S, H, W)).astype(np.float32)
    x[1, 16, 32] = np.float32(-1.0)
    cases.append(_call("median2d", "17x33-k3-noroi-negative-middle", {"H": H, "W": W, "k": 3}, {"src": _flat(x)}, _restate_median))
    return cases


def _erode_cases():
    cases = []
    for n in (1, 8):
        x = _blobs(_rng(8, n), (17, 33), 0.97 if n == 1 else 1.0)
        if n == 8:                                           # only row 8, columns 8 ... 24 can survive: a hole near them in both outer planes
            x[0, 3, 20] = x[2, 8, 2] = np.float32(0.25)
        x[1] = 1                                             # the middle plane: all foreground, only the image border goes
        cases.append(_call("erode2d", f"17x33-n{n}", {"H": 17, "W": 33, "n": n, "level": 0.5}, {"src": _flat(x)}, _restate_erode))
    return cases


def _small_components_cases():
    cases = []
    for conn in (1, 2):
        x = _blobs(_rng(9, conn), (17, 33))
        x[1] = np.float32(0.25)                              # the middle plane: no foreground
        cases.append(_call("small_components", f"17x33-c{conn}-empty-middle", {"H": 17, "W": 33, "min_size": 3, "connectivity": conn, "level": 0.5},
                           {"src": _flat(x)}, _restate_components))
    return cases


def _gauss_cases():
    cases = []
    for sigma in (0.5, 4.0):
        r = smc.radius_of(sigma)                             # 2 and 16: the plane of 5 rows is narrower than the second
        x = _rng(10, r).random((S, 5, 33)).astype(np.float32)
        x[1] = np.float32(0.7)                               # the middle plane: constant
        cases.append(_call("gauss2d", f"5x33-r{r}", {"H": 5, "W": 33, "radius": r}, {"src": _flat(x), "w": smc.weights_numpy(sigma)[:r + 1].copy()},
                           _restate_gauss, aux={"sigma": sigma}))
    return cases


def _map_scores_cases():
    cases = []
    for n, k in ((1, 1), (1023, 1), (1023, 1023), (1025, 1), (1025, 1025)):
        x = (np.round(_rng(11, n, k).random((S, n)) * 256) / 256).astype(np.float32)
        x[1] = 0                                             # the middle segment: all zero
        cases.append(_call("map_scores", f"n{n}-k{k}", {"n": n, "k": k}, {"src": x}, _restate_scores))
    x = _rng(11, 99).random((S, 1025)).astype(np.float32)
    x[1, 1024] = np.float32(-0.25)
    cases.append(_call("map_scores", "n1025-k7-negative-middle", {"n": 1025, "k": 7}, {"src": x}, _restate_scores))
    return cases


def _median3d_cases():
    cases = []
    plans = list(itertools.product((3, 5), ((1, 7, 9), (5, 9, 33)), ("plane", "volume", None)))
    for i, (k, (D, H, W), roi) in enumerate(plans):
        rng = _rng(12, i)
        x = (np.round(rng.random((S, D, H, W)) * 64) / 64).astype(np.float32)
        x[1] = np.float32(0.375)                             # the middle volume: constant
        inputs = {"src": _flat(x)}
        if roi:
            inputs["roi"] = (rng.random(H * W if roi == "plane" else D * H * W) < 0.7).astype(np.float32)
        sc = {"D": D, "H": H, "W": W, "k": k, "roi_slice_stride": H * W if roi == "volume" else 0}
        cases.append(_call("median3d", f"{D}x{H}x{W}-k{k}-{roi or 'no'}roi", sc, inputs, _restate_median))
    x = _rng(12, 99).random((S, 1, 7, 9)).astype(np.float32)
    x[1, 0, 6, 8] = np.nan
    cases.append(_call("median3d", "1x7x9-k3-noroi-nan-middle", {"D": 1, "H": 7, "W": 9, "k": 3, "roi_slice_stride": 0}, {"src": _flat(x)},
                       _restate_median))
    return cases


def _erode3d_cases():
    cases = []
    for n in (1, 3):
        x = _blobs(_rng(13, n), (9, 17, 33), 0.97 if n == 1 else 0.9995)
        x[1] = 1                                             # the middle volume: all foreground
        cases.append(_call("erode3d", f"9x17x33-n{n}", {"D": 9, "H": 17, "W": 33, "n": n, "level": 0.5}, {"src": _flat(x)}, _restate_erode))
    return cases


def _components3d_inputs(conn):
    x = _blobs(_rng(14, conn), (3, 9, 33), 0.12)
    x[1] = np.float32(0.25)                                  # the middle volume: no foreground
    return {"src": _flat(x)}


def _small_components3d_cases():
    return [_call("small_components3d", f"3x9x33-c{c}-empty-middle", {"D": 3, "H": 9, "W": 33, "min_size": 3, "connectivity": c, "level": 0.5},
                  _components3d_inputs(c), _restate_components) for c in (1, 2, 3)]


def _component_areas3d_cases():
    return [_call("component_areas3d", f"3x9x33-c{c}-empty-middle", {"D": 3, "H": 9, "W": 33, "connectivity": c, "level": 0.5},
                  _components3d_inputs(c), _restate_areas3d) for c in (1, 2, 3)]


CASES = {"roc_auc": _roc_cases, "pro_auc": _pro_cases, "component_areas": _component_areas_cases, "ssim": _ssim_cases,
         "distance_transform": _distance_cases, "surface_distance": _surface_cases, "median2d": _median_cases, "erode2d": _erode_cases,
         "small_components": _small_components_cases, "gauss2d": _gauss_cases, "map_scores": _map_scores_cases, "median3d": _median3d_cases,
         "erode3d": _erode3d_cases, "small_components3d": _small_components3d_cases, "component_areas3d": _component_areas3d_cases}
_BUILT = {}


def cases(entry):
    """The calls of one entry point; built once, with their expected values, and shared by every test that needs them."""
    if entry not in _BUILT:
        _BUILT[entry] = CASES[entry]()
        for c in _BUILT[entry]:
            expected_of(c)
    return _BUILT[entry]


# ---------------------------------------------------------------------------------------------------- the checker
def _rows(shape, skip):
    """Elements of an [S, ...] output that belong to a segment whose outputs are compared."""
    keep = np.ones(shape, bool)
    for s in skip:
        keep[s] = False
    return keep


def check(call, arenas_before, arenas_after, expected, reference=None):
    """The findings of one call, as (name, field, detail) triples.  `reference`: the arenas after an earlier launch of the same
    call that was checked by value; the outputs are then compared with it bit for bit instead (`workspace_dependent`)."""
    t = TABLE[call["entry"]]
    found = []

    def add(name, field, where):
        idx = np.flatnonzero(where)
        found.append((name, field, f"{idx.size} element(s), first at {int(idx[0])}"))

    for field, b in arenas_before.items():
        a = arenas_after[field]
        diff = b.bits != a.bits
        seg, gap, guard = b.regions()
        if (diff & guard).any():
            add("guard_written", field, diff & guard)
        if b.kind == "in":
            if (diff & seg).any():
                add("input_modified", field, diff & seg)
            if (diff & gap).any():
                add("gap_written", field, diff & gap)
        if b.kind != "out":
            continue
        e = expected[field]
        shape = e["value"].shape
        is_status = field == t["status"]
        rows = _rows(shape, () if is_status else call["skip"])
        got = a.bits[b.seg()].reshape(shape)
        before = b.bits[b.seg()].reshape(shape)
        left = (got == before) & e["written"] & rows         # `before` is the poison
        if left.any():
            add("unwritten_output", field, left)
        outside = (got != before) & ~e["written"] & rows
        if outside.any():
            add("wrote_outside_written_set", field, outside)
        live = e["written"] & rows & ~left
        if reference is not None:
            other = reference[field].bits[b.seg()].reshape(shape)
            if ((got != other) & rows).any():
                add("workspace_dependent", field, (got != other) & rows)
            continue
        if e["rule"] == "bits":
            bad = (got != e["value"].reshape(shape).view(b.word)) & live
        else:
            g = got.view(b.item).astype(np.float64)
            w = e.get("want64", e["value"]).astype(np.float64)
            with np.errstate(invalid="ignore"):
                bad = ~((np.isnan(g) & np.isnan(w)) | (np.abs(g - w) <= e["rule"])) & live
        if bad.any():
            add("status" if is_status else "wrong_value", field, bad)
    return found


def names(findings):
    return sorted({f[0] for f in findings})


# ---------------------------------------------------------------------------------------------------- simulated calls
DEFECTS = ("past_output", "before_workspace", "skip_last", "curve_at_cap", "read_gap", "modify_input", "dirty_workspace", "write_gap",
           "drop_status")


def _first_output(call, expected):
    t = TABLE[call["entry"]]
    return next(f for f in expected if f != t["status"])


def _strided_input(call, arenas):
    return next((f for f, a in arenas.items() if a.kind == "in" and a.segs > 1), None)


def defect_finding(call, defect):
    """The findings `simulate(call, defect)` must give: a set of admissible names (one of them, and nothing else), or None where
    the call has nothing the defect could touch."""
    expected = expected_of(call)
    if defect in ("past_output", "before_workspace"):
        return {"guard_written"} if defect == "past_output" or has_workspace(call["entry"]) else None
    if defect == "skip_last":
        return {"unwritten_output"}
    if defect == "curve_at_cap":
        if "curve_len" not in expected:
            return None
        s, at_cap = _curve_target(call, expected)
        return {"guard_written"} if at_cap else {"wrote_outside_written_set"}
    if defect == "read_gap":
        return {"wrong_value", "status"}                     # a read of the fill changes a result or raises a status bit
    if defect == "modify_input":
        return {"input_modified"}
    if defect == "dirty_workspace":
        return {"workspace_dependent"} if has_workspace(call["entry"]) else None
    if defect == "write_gap":
        return {"gap_written"}
    if defect == "drop_status":
        return {"status"} if TABLE[call["entry"]]["status"] and expected[TABLE[call["entry"]]["status"]]["value"].any() else None
    raise KeyError(defect)


def _curve_target(call, expected):
    """The segment whose curve gets one entry too many: the first one with room in its row, else the last (its entry at index
    curve_cap lies behind the array)."""
    cap = call["scalars"]["curve_cap"]
    length = expected["curve_len"]["value"]
    for s in range(S):
        if s not in call["skip"] and length[s] < cap:
            return s, False
    return S - 1, True


def simulate(call, defect=None, ws_fill=0):
    """(arenas before, arenas after) of a numpy stand-in for the device that runs the restatement, optionally with one defect."""
    before = build_arenas(call, ws_fill=ws_fill)
    after = {f: a.copy() for f, a in before.items()}
    expected = expected_of(call)
    result = expected
    if defect == "read_gap":                                 # the first strided input with a stride one element too small: the word
        field = _strided_input(call, before)                 # in front of segment 1 is its first element (segment 2 is off by two)
        a = before[field]
        inputs = dict(call["inputs"])
        x = np.array(inputs[field])
        for s in range(1, a.segs):
            x[s] = a.bits[a.lo(s) - s:a.lo(s) - s + a.n].view(a.item)
        inputs[field] = x
        ghost = dict(call, skip=set())
        ghost.pop("_expected", None)
        result = call["restate"](ghost, inputs)
    for field, e in result.items():
        a = after[field]
        body = a.bits[a.seg()].reshape(e["value"].shape)
        written = expected[field]["written"]                 # a segment that went wrong still gets its elements written
        body[written] = e["value"].view(a.word)[written]
        a.bits[a.seg()] = body.reshape(-1)
    if "workspace" in after:
        after["workspace"].bits[after["workspace"].seg()] = WS_LEFT_BYTE             # unspecified on exit
    if defect in (None, "read_gap"):
        return before, after
    first = after[_first_output(call, expected)]
    if defect == "past_output":
        first.bits[first.lo() + first.n] ^= 1
    elif defect == "before_workspace":
        after["workspace"].bits[after["workspace"].lo() - 1] ^= 0xff
    elif defect == "skip_last":
        e = expected[first.name]
        live = np.flatnonzero((e["written"] & _rows(e["value"].shape, call["skip"])).reshape(-1))
        first.bits[first.lo() + live[-1]] = POISON[first.item.str[1:]]
    elif defect == "curve_at_cap":
        s, _ = _curve_target(call, expected)
        cap, length = call["scalars"]["curve_cap"], int(expected["curve_len"]["value"][s])
        a = after["curve_fps"]
        a.bits[a.lo() + s * cap + min(length, cap)] = 12345
    elif defect == "modify_input":
        a = after[next(f for f, x in after.items() if x.kind == "in")]
        a.bits[a.lo()] ^= 1
    elif defect == "write_gap":
        a = after[_strided_input(call, after)]
        a.bits[a.lo(0) + a.n] ^= 1
    elif defect == "dirty_workspace":                        # a word that is accumulated into without being cleared first
        first.bits[first.lo()] ^= int(before["workspace"].bits[before["workspace"].lo()]) & 1
    elif defect == "drop_status":
        a = after[TABLE[call["entry"]]["status"]]
        a.bits[a.seg()] = 0
    else:
        raise KeyError(defect)
    return before, after
