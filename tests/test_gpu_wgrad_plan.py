"""-m gpu: the weight-gradient launches of the training plan against fp64, per block of 64 output x 32 input channels and per
image (tests/wgrad_cases.py).

A. Walk cases of the Winograd-domain kernel (algo 1, csrc/wgrad43.hip) in which workgroups walk several patches: image changes,
   skipped images, the prefetch past the end, the affine table at B = 15.  Accumulating into a non-zero dw / dbias as the plan
   does; bit-identical on a second run and with the two-launch fold (variant 8).
B. Replay of the plan's own OP_WGRAD3 / OP_WGRAD1 / OP_COLSUM_FOLD launches -- their tilings (band, span, algo, workspace sizes)
   kept, only the pointers replaced by recipe tensors, the workspace, colsum and dimg filled with NaN -- through anoddpm_run_ops.
C. algo 1 refuses B = 16.

Bars (those of test_conv3x3_wgrad_winograd_domain, test_conv3x3_wgrad and test_wgrad_pointwise): 1e-4 for algo 1, 2e-5 for the
direct 3x3 and the 1x1 kernels, 1e-5 for the column sums; the fp64 reference is exact to ~1e-15, so the whole bar is the
kernel's.  Every figure is printed before it is asserted (-s)."""
import ctypes
import gc

import pytest
import torch

import wgrad_cases as wc

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BAR3_WINO, BAR3_DIRECT, BAR1, BAR_CS = 1e-4, 2e-5, 2e-5, 1e-5


def _start(N, K, seed, taps=9):
    """Finite non-zero gradients to accumulate into: dw [N, K(, 3, 3)] and dbias [N]."""
    g = torch.Generator().manual_seed(seed)
    shape = (N, K, 3, 3) if taps == 9 else (N, K)
    return 0.5 * torch.randn(*shape, generator=g), torch.randn(N, generator=g)


# ---------------------------------------------------------------------------------------------------- A. walk cases
@pytest.mark.parametrize("name", list(wc.WALK_CASES))
def test_wgrad43_walk(name):
    import hipops
    from anoddpm_amd._lib import lib
    B, (c0, c1), N, H, W, a_mode = wc.WALK_CASES[name]
    K = c0 + c1
    walk = wc.walk(K, N, B, H, W)
    # the launcher's grouping is the one the case was chosen for: a change to it fails here instead of making this a one-patch test
    assert lib().anoddpm_wgrad43_groups(K, N, B, H, W) == walk["PG"] == wc.WALK_CLAIMS[name]["PG"]
    assert lib().anoddpm_wgrad43_colsum_items(K, N, B, H, W) == 2 * walk["PG"]
    srcs, dy, scale, shift = wc.recipe(B, c0, c1, N, H, W, a_mode, seed=1 + list(wc.WALK_CASES).index(name))
    dw0, db0 = _start(N, K, seed=5)
    dsrcs = [s.to(DEV).contiguous() for s in srcs]
    ddy, gn = dy.to(DEV).contiguous(), (scale.to(DEV).contiguous(), shift.to(DEV).contiguous())

    def run():
        dw = dw0.to(DEV).clone()
        bo = {"dbias": db0.to(DEV).clone()}
        hipops.conv_wgrad(dsrcs, ddy, gn=gn, act=1, a_mode=a_mode, accumulate_into=dw, colsum_out=[], algo=1, bias_out=bo)
        return dw.cpu(), bo["dimg"].cpu(), bo["dbias"].cpu()

    dw, dimg, dbias = run()
    ref_dw, ref_dimg = wc.wgrad3(wc.operand(srcs, a_mode, scale, shift, act=1), dy)
    e_dw, where = wc.block_err(dw, ref_dw, dw0)
    e_dimg = wc.row_err(dimg, ref_dimg)
    e_db = wc.row_err(dbias, ref_dimg.sum(dim=0), db0)
    print(f"\n{name} B={B} K={c0}+{c1} N={N} {H}x{W} a_mode={a_mode} PG={walk['PG']} patches/wg={walk['min']}..{walk['max']}: "
          f"dw {e_dw:.3e} (block n0,k0={where}, bar {BAR3_WINO:g})  dimg {e_dimg:.3e}  dbias {e_db:.3e} (bar {BAR_CS:g})")
    assert e_dw < BAR3_WINO, (e_dw, where)
    assert e_dimg < BAR_CS and e_db < BAR_CS, (e_dimg, e_db)
    # a fixed-order fold without atomics: the same bits again, and the same bits from the two-launch fold
    again = run()
    assert all(torch.equal(a, b) for a, b in zip(again, (dw, dimg, dbias)))
    lib().anoddpm_internal_variant(8, 1)
    try:
        two = run()
    finally:
        lib().anoddpm_internal_variant(8, 0)
    assert all(torch.equal(a, b) for a, b in zip(two, (dw, dimg, dbias)))


# ---------------------------------------------------------------------------------------------------- B. replay of the plan
PLANS = {
    "c3_b4": (dict(img_size=256, base_channels=128, n_heads=2, attention_resolutions="16,8"), 4),
    "c3_b1": (dict(img_size=256, base_channels=128, n_heads=2, attention_resolutions="16,8"), 1),
    "m64_b15": (dict(img_size=64, base_channels=32, n_heads=1), 15),
    "m64_b16": (dict(img_size=64, base_channels=32, n_heads=1), 16),
}


def _key(st):
    """Non-pointer fields of a launch struct (and which pointers are set)."""
    return tuple((n, bool(getattr(st, n)) if t is ctypes.c_void_p else getattr(st, n)) for n, t in st._fields_)


def _plan_launches(kw, B):
    """Forward + backward of one batch on the native training plan; the distinct weight-gradient launches of its backward list
    as (code, struct copy, colsum-fold struct copy or None)."""
    from anoddpm_amd import _lib
    from anoddpm_amd.unet import UNetModel
    torch.manual_seed(0)
    model = UNetModel(**kw).to(DEV).train()
    S = kw["img_size"]
    x = torch.randn(B, 1, S, S, device=DEV)
    t = torch.randint(0, 1000, (B,), device=DEV)
    model(x, t).square().mean().backward()
    torch.cuda.synchronize()
    (plan,) = model._tplans.values()
    bops = plan.bops
    out, seen = [], set()
    for i, (code, st) in enumerate(bops):
        fold = None
        if code == _lib.OP_COLSUM_FOLD:
            # folds the column sums of the direct 3x3 launch in front of it (replayed together with it)
            assert bops[i - 1][0] == _lib.OP_WGRAD3 and bops[i - 1][1].algo == 0 and bops[i - 1][1].colsum == st.colsum
            continue
        if code == _lib.OP_WGRAD3 and st.algo == 0:
            assert bops[i + 1][0] == _lib.OP_COLSUM_FOLD and bops[i + 1][1].colsum == st.colsum
            fold = type(bops[i + 1][1]).from_buffer_copy(bops[i + 1][1])
        if code not in (_lib.OP_WGRAD3, _lib.OP_WGRAD1):
            continue
        c = type(st).from_buffer_copy(st)
        k = (code, _key(c), _key(fold) if fold is not None else None)
        if k not in seen:
            seen.add(k)
            out.append((code, c, fold))
    return out


def _images(B, bs, seed, dy=False):
    g = torch.Generator().manual_seed(seed)
    return (wc.dy_rows if dy else wc.image_rows)(B, bs, g)


def _view(buf, B, P, ld, c):
    """[B, P, c] view of a [B, bs] buffer with rows of length ld (what the kernel reads)."""
    return buf[:, :P * ld].reshape(B, P, ld)[..., :c]


def _inputs(st, Psrc, Pdy, seed):
    """Recipe inputs of a replayed launch, its pointers patched to them: the sources and dY as [B, batch stride] buffers with rows of
    length ld, the affines [B, gn_ld] when the launch reads a GroupNorm operand.  Returns the device tensors, the [B, P, c] views
    of the sources and of dY that the kernel reads, and the (scale, shift) of its K channels or None."""
    B, K = st.B, st.c0 + st.c1
    host, srcs = {}, []
    for i, (name, c, bs, ld) in enumerate((("a0", st.c0, st.a0_bs, st.a0_ld), ("a1", st.c1, st.a1_bs, st.a1_ld))):
        if c:
            assert bs >= Psrc * ld
            host[name] = _images(B, bs, seed + i)
            srcs.append(_view(host[name], B, Psrc, ld, c))
    assert st.dy_bs >= Pdy * st.dy_ld
    host["dy"] = _images(B, st.dy_bs, seed + 2, dy=True)
    gn = None
    if st.gn_scale:
        host["scale"], host["shift"] = wc.affines(B, st.gn_ld, torch.Generator().manual_seed(seed + 3))
        gn = (host["scale"][:, :K], host["shift"][:, :K])
    d = {n: v.to(DEV).contiguous() for n, v in host.items()}
    st.a0, st.a1, st.dy = d["a0"].data_ptr(), d["a1"].data_ptr() if st.c1 else None, d["dy"].data_ptr()
    if gn is not None:
        st.gn_scale, st.gn_shift = d["scale"].data_ptr(), d["shift"].data_ptr()
    return d, srcs, _view(host["dy"], B, Pdy, st.dy_ld, st.N), gn


def _replay3(st, fold, seed):
    from anoddpm_amd import _lib
    from anoddpm_amd._lib import lib
    from anoddpm_amd.train_plan import _op_array
    st = type(st).from_buffer_copy(st)
    B, c0, c1, N, H, W = st.B, st.c0, st.c1, st.N, st.H, st.W
    K = c0 + c1
    Hs, Ws = wc.source_size(H, W, st.a_mode)
    d, srcs, dy, gn = _inputs(st, Hs * Ws, H * W, seed)
    srcs = [s.reshape(B, Hs, Ws, s.shape[2]) for s in srcs]
    dy = dy.reshape(B, H, W, N)
    dw0, db0 = _start(N, K, seed + 4)
    rows = lib().anoddpm_wgrad43_colsum_items(K, N, B, H, W) if st.algo == 1 else fold.ipb
    d["dw"], d["dbias"] = dw0.to(DEV), db0.to(DEV)
    d["ws"] = torch.full((st.ws_floats,), float("nan"), device=DEV)
    d["colsum"] = torch.full((B * rows * N,), float("nan"), device=DEV)
    d["dimg"] = torch.full((B, N), float("nan"), device=DEV)
    assert st.colsum
    st.dw, st.ws, st.colsum = d["dw"].data_ptr(), d["ws"].data_ptr(), d["colsum"].data_ptr()
    ops = [(_lib.OP_WGRAD3, st)]
    if fold is None:                                         # algo 1: the fold launch of the kernel folds the column sums
        assert st.dimg
        has_db = bool(st.dbias)
        st.dimg, st.dbias = d["dimg"].data_ptr(), d["dbias"].data_ptr() if has_db else None
    else:
        fold = type(fold).from_buffer_copy(fold)
        assert fold.B == B and fold.N == N
        has_db = bool(fold.dbias)
        fold.colsum, fold.dimg, fold.dbias = d["colsum"].data_ptr(), d["dimg"].data_ptr(), d["dbias"].data_ptr() if has_db else None
        ops.append((_lib.OP_COLSUM_FOLD, fold))
    _lib.check(lib().anoddpm_run_ops(_op_array(ops), len(ops), _lib.current_stream()), "weight-gradient replay")
    torch.cuda.synchronize()
    ref_dw, ref_dimg = wc.wgrad3(wc.operand(srcs, st.a_mode, *(gn or (None, None)), act=st.act), dy)
    errs = {"dw": wc.block_err(d["dw"].cpu(), ref_dw, dw0 if st.accumulate else None)[0],
            "dimg": wc.row_err(d["dimg"].cpu(), ref_dimg)}
    if has_db:
        errs["dbias"] = wc.row_err(d["dbias"].cpu(), ref_dimg.sum(dim=0), db0)
    bars = {"dw": BAR3_WINO if st.algo == 1 else BAR3_DIRECT, "dimg": BAR_CS, "dbias": BAR_CS}
    name = (f"WGRAD3 algo={st.algo} B={B} K={c0}+{c1} N={N} {H}x{W} a_mode={st.a_mode} act={st.act} gn={int(gn is not None)} "
            f"band={st.band} ws={st.ws_floats}" + (f" ipb={fold.ipb}" if fold is not None else ""))
    return name, errs, bars


def _replay1(st, seed):
    from anoddpm_amd import _lib
    from anoddpm_amd._lib import lib
    from anoddpm_amd.train_plan import _op_array
    st = type(st).from_buffer_copy(st)
    B, c0, c1, N, P = st.B, st.c0, st.c1, st.N, st.P
    d, srcs, dy, gn = _inputs(st, P, P, seed)
    dw0, db0 = _start(N, c0 + c1, seed + 4, taps=1)
    d["dw"], d["dbias"] = dw0.to(DEV), db0.to(DEV)
    d["ws"] = torch.full((st.ws_floats,), float("nan"), device=DEV)
    has_db = bool(st.dbias)
    st.dw, st.ws, st.dbias = d["dw"].data_ptr(), d["ws"].data_ptr(), d["dbias"].data_ptr() if has_db else None
    _lib.check(lib().anoddpm_run_ops(_op_array([(_lib.OP_WGRAD1, st)]), 1, _lib.current_stream()), "weight-gradient replay")
    torch.cuda.synchronize()
    ref_dw, ref_db = wc.wgrad1(wc.pointwise_operand(srcs, *(gn or (None, None)), act=st.act), dy)
    errs = {"dw": wc.block_err(d["dw"].cpu(), ref_dw, dw0 if st.accumulate else None)[0]}
    if has_db:
        errs["dbias"] = wc.row_err(d["dbias"].cpu(), ref_db, db0)
    bars = {"dw": BAR1, "dbias": BAR_CS}
    name = f"WGRAD1 B={B} K={c0}+{c1} N={N} P={P} act={st.act} gn={int(gn is not None)} span={st.span} ws={st.ws_floats}"
    return name, errs, bars


def _coverage(name, launches):
    from anoddpm_amd import _lib
    w3 = [st for code, st, _ in launches if code == _lib.OP_WGRAD3]
    wino = [st for st in w3 if st.algo == 1]
    if name == "c3_b4":
        assert {st.H for st in wino} >= {256, 128, 64, 32, 16}, sorted({st.H for st in wino})
        assert any(st.c1 > 0 for st in wino) and any(st.a_mode == 1 for st in wino)
        assert any(st.algo == 0 for st in w3)
        assert any(st.P == 65536 for code, st, _ in launches if code == _lib.OP_WGRAD1)
    elif name == "m64_b16":
        assert not wino                                      # algo 1 holds the affines of at most 15 images (B <= 15 in the plan)
    elif name == "m64_b15":
        assert wino


@pytest.mark.parametrize("name", list(PLANS))
def test_plan_weight_gradient_launches(name):
    from anoddpm_amd import _lib
    kw, B = PLANS[name]
    launches = _plan_launches(kw, B)
    gc.collect()
    torch.cuda.empty_cache()                                 # the model and the plan are gone before the replays
    _coverage(name, launches)
    print(f"\nplan {name}: {len(launches)} distinct weight-gradient launches")
    bad = []
    for i, (code, st, fold) in enumerate(launches):
        if code == _lib.OP_WGRAD3:
            what, errs, bars = _replay3(st, fold, seed=100 + 10 * i)
        else:
            what, errs, bars = _replay1(st, seed=100 + 10 * i)
        line = "  ".join(f"{k} {v:.3e} (bar {bars[k]:g})" for k, v in errs.items())
        print(f"  {what}: {line}")
        bad += [(what, k, v) for k, v in errs.items() if not v < bars[k]]
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------- C. refusal
def test_wgrad43_refuses_batch_16():
    import hipops
    srcs, dy, scale, shift = wc.recipe(16, 32, 0, 64, 16, 16, 0, seed=3)
    gn = (scale.to(DEV), shift.to(DEV))
    with pytest.raises(Exception, match="batch > 15"):
        hipops.conv_wgrad([srcs[0].to(DEV)], dy.to(DEV), gn=gn, act=1, algo=1)
    # the direct kernel takes the same launch
    dw = hipops.conv_wgrad([srcs[0].to(DEV)], dy.to(DEV), gn=gn, act=1, algo=0)
    ref, _ = wc.wgrad3(wc.operand(srcs, 0, scale, shift, act=1), dy)
    assert wc.block_err(dw.cpu(), ref)[0] < BAR3_DIRECT
