"""-m gpu: the device weight packers (csrc/pack_items.h through anoddpm_pack_weights / anoddpm_pack_conv3x3, anoddpm_pack_batch with
anoddpm_pack_job_blocks, anoddpm_pack_wino43_bf16x3) straight through the C ABI on the jobs of tests/pack_cases.py, every element
against the numpy fp64 restatement of the header's layouts.

Permutation layouts (kinds 0, 2, 3, 4, both directions) are bit for bit; the Winograd layouts (kinds 1, 5) are within
2^-24 |U64| + 2^-45 S per element; the bf16 planes meet |f - (h + m + l)| <= 2^-24 |f|, |f - h| <= 2^-8 |f|, |m| <= 2^-8 |f|,
|l| <= 2^-16 |f| and are bit for bit the nearest-even split of their own sum, which is within the Winograd bar of U64.  Every output
is NaN-filled with 64 NaN elements behind it: no NaN may remain inside, the guard comes back untouched.  anoddpm_pack_batch runs job
tables of 1, 2 and 13 jobs into one NaN arena with NaN gaps: each job's output is bit-identical to the single-job launch and within
the bars, the gaps stay NaN, and block0 is built from anoddpm_pack_job_blocks, itself equal to ceil(items / 256) of the header's item
counts.  The packed buffers of the i32_b2 inference plan and of the training plan of the same model are decoded after one forward
and compared with the restatement of their parameter (the job tables name the right kind, N and K).

Measured on an MI355X: kinds 0, 2, 3, 4 bit for bit in every job, table and plan buffer; kinds 1 and 5, both directions, at most
1.000 of 2^-24 |U64| + 2^-45 S (one rounding); the planes' sum is exactly the kind 5 fp32 value in all three bf16 cases; no guard or
gap element written.  Two findings, both fixed in csrc/pack_items.h (`dot3`, `wino43_u_row`):
  * anoddpm_pack_batch and anoddpm_pack_weights disagreed in 14 .. 23 of ~74 000 kind 5 values of a weight (kind5-fwd-260x8,
    kind5-bwd-64x32), each by one fp32 place: those U are, in exact arithmetic, ties between two fp32 neighbours, the fp64 value falls
    a last bit to one side, and the compiler contracted the same source differently in the two kernels.  The transform now has one
    evaluation order (explicit fused multiply-adds) and the two launches are bit-identical.
  * the bf16 packer carried its own copy of the transform and so split values that were, at such ties, not the fp32 layout's; it now
    calls the same function.
Wall time of the module on the device: 3.2 s for the 57 items."""
import ctypes

import numpy as np
import pytest
import torch

import pack_cases as pc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
FAULT = []                  # the first launch that raised: nothing more is launched after it
WORST = {}


def L():
    from anoddpm_amd import _lib
    return _lib, _lib.lib()


@pytest.fixture(scope="module", autouse=True)
def ledger():
    yield
    print()
    for key in sorted(WORST):
        print(f"worst kind {key[0]} {'bwd' if key[1] else 'fwd'}: {WORST[key][0]:.3f} of the bar at {WORST[key][1]}")


def _guarded(fn):
    assert not FAULT, f"not launched: an earlier launch raised ({FAULT[0]})"
    try:
        out = fn()
        torch.cuda.synchronize()
        return out
    except BaseException as err:
        FAULT.append(repr(err))
        raise


def _struct(job, w, out):
    _lib, _ = L()
    st = _lib.PackArgs()
    st.w, st.out = w.data_ptr(), out.data_ptr()
    st.kind, st.bwd, st.N, st.K, st.k0, st.kc = job
    return st


def _single(job, w):
    """One anoddpm_pack_weights launch into a NaN buffer with a guard -> (fp32 numpy of the output, failures)."""
    _lib, lib = L()
    n = pc.out_floats(job)
    out = torch.full((n + pc.GUARD,), NAN, device=DEV)
    wd = torch.from_numpy(w).to(DEV)
    st = _struct(job, wd, out)
    _guarded(lambda: _lib.check(lib.anoddpm_pack_weights(ctypes.byref(st), _lib.current_stream()), "pack_weights"))
    fails = [] if torch.isnan(out[n:]).all() else ["elements behind the buffer's end were written"]
    return out[:n].cpu().numpy(), fails


def _note(job, w, got, where):
    r = pc.worst_ulp(job, w, got)
    key = (job[0], job[1])
    WORST[key] = max(WORST.get(key, (0.0, where)), (r, where))
    return r


@pytest.mark.parametrize("job", pc.single_jobs(), ids=pc.job_id)
def test_pack_weights(job):
    _lib, lib = L()
    w = pc.weights(job)
    got, fails = _single(job, w)
    fails += pc.judge(job, w, got)
    print(f"{pc.job_id(job)}: {got.size} floats, {_note(job, w, got, pc.job_id(job)):.3f} of the bar, {pc.items(job)} items")
    st = _struct(job, torch.zeros(1), torch.zeros(1))
    assert lib.anoddpm_pack_job_blocks(ctypes.byref(st)) == pc.blocks(job)
    if job[0] in (0, 1, 5):                                   # the older entry point of the same kernel
        n = pc.out_floats(job)
        out = torch.full((n + pc.GUARD,), NAN, device=DEV)
        wd = torch.from_numpy(w).to(DEV)
        mode = {0: 0, 1: 1, 5: 2}[job[0]]
        _guarded(lambda: _lib.check(lib.anoddpm_pack_conv3x3(wd.data_ptr(), out.data_ptr(), job[2], job[3], mode, job[1], _lib.current_stream()), "pack_conv3x3"))
        if not np.array_equal(out[:n].cpu().numpy().view(np.uint32), got.view(np.uint32)) or not torch.isnan(out[n:]).all():
            fails.append("anoddpm_pack_conv3x3 and anoddpm_pack_weights differ")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("N,K", pc.BF16_SHAPES)
def test_bf16_planes(N, K):
    _lib, lib = L()
    w = pc.weights((5, 0, N, K, 0, 0))
    n = 3 * 36 * N * K
    out = torch.full((n + 2 * pc.GUARD,), -1, dtype=torch.int16, device=DEV)          # 0xFFFF: a bf16 NaN
    wd = torch.from_numpy(w).to(DEV)
    _guarded(lambda: _lib.check(lib.anoddpm_pack_wino43_bf16x3(wd.data_ptr(), out.data_ptr(), N, K, _lib.current_stream()), "pack_wino43_bf16x3"))
    planes = out[:n].cpu().numpy().view(np.uint16)
    fails = pc.judge_bf16(N, K, w, planes)
    if not (out[n:] == -1).all():
        fails.append("elements behind the planes' end were written")
    # the planes split the fp32 values of the kind 5 layout of the same weight, bit for bit (one statement of the transform)
    job = (5, 0, N, K, 0, 0)
    f32, f1 = _single(job, w)
    h, m, lo = (pc.widen(planes[i * (n // 3):(i + 1) * (n // 3)]).astype(np.float64) for i in range(3))
    total = (h + m + lo).reshape(36, K // 8, N, 2, 4).transpose(0, 1, 3, 2, 4).reshape(-1)           # [xi][k / 8][n][k % 8] -> [xi][k / 4][n][4]
    if not np.array_equal(total.astype(np.float32).view(np.uint32), f32.view(np.uint32)):
        fails.append(f"h + m + l is not the kind 5 fp32 value at {int((total.astype(np.float32) != f32).sum())} of {f32.size} elements")
    fails += f1 + pc.judge(job, w, f32)
    assert not fails, "\n".join(fails)


def _table(jobs):
    """The arena, the per-job regions and the device job table of one anoddpm_pack_batch launch."""
    _lib, lib = L()
    offs, at = [], pc.GUARD
    for job in jobs:
        offs.append(at)
        at += -(-pc.out_floats(job) // 4) * 4 + pc.GUARD                                 # 16-byte aligned outputs, NaN gaps between
    arena = torch.full((at,), NAN, device=DEV)
    ws = [pc.weights(job, seed=j) for j, job in enumerate(jobs)]
    wd = [torch.from_numpy(w).to(DEV) for w in ws]
    arr = (_lib.PackArgs * len(jobs))()
    block0 = [0]
    for j, job in enumerate(jobs):
        st = _struct(job, wd[j], arena[offs[j]:])
        ctypes.memmove(ctypes.addressof(arr[j]), ctypes.addressof(st), ctypes.sizeof(_lib.PackArgs))
        nb = lib.anoddpm_pack_job_blocks(ctypes.byref(st))
        assert nb == pc.blocks(job), (job, nb)
        block0.append(block0[-1] + nb)
    raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    b0 = torch.tensor(block0, dtype=torch.int32, device=DEV)
    pb = _lib.PackBatchArgs()
    pb.jobs, pb.block0, pb.njobs, pb.nblocks = raw.data_ptr(), b0.data_ptr(), len(jobs), block0[-1]
    return arena, offs, ws, wd, pb, (raw, b0)


@pytest.mark.parametrize("jobs", pc.JOB_TABLES, ids=lambda t: f"{len(t)}jobs")
def test_pack_batch(jobs):
    _lib, lib = L()
    arena, offs, ws, wd, pb, keep = _table(jobs)
    _guarded(lambda: _lib.check(lib.anoddpm_pack_batch(ctypes.byref(pb), _lib.current_stream()), "pack_batch"))
    host = arena.cpu().numpy()
    fails, written = [], np.zeros(host.size, dtype=bool)
    for j, job in enumerate(jobs):
        n = pc.out_floats(job)
        got = host[offs[j]:offs[j] + n]
        written[offs[j]:offs[j] + n] = True
        single, f1 = _single((job[0], job[1], job[2], job[3], job[4], job[5]), ws[j])
        fails += [f"job {j} {pc.job_id(job)} (single launch): {f}" for f in f1 + pc.judge(job, ws[j], single)]
        fails += [f"job {j} {pc.job_id(job)}: {f}" for f in pc.judge(job, ws[j], got)]
        if not np.array_equal(got.view(np.uint32), single.view(np.uint32)):
            fails.append(f"job {j} {pc.job_id(job)}: the batched launch and the single-job launch differ in "
                         f"{int((got.view(np.uint32) != single.view(np.uint32)).sum())} of {n} elements")
        print(f"job {j} {pc.job_id(job)}: blocks {pc.blocks(job)}, {_note(job, ws[j], got, f'batch of {len(jobs)} job {j}'):.3f} of the bar")
    if not np.isnan(host[~written]).all():
        fails.append(f"{int((~np.isnan(host[~written])).sum())} elements of the gaps between the jobs' outputs were written")
    assert not fails, "\n".join(fails)


def _job_of(st):
    return (st.kind, st.bwd, st.N, st.K, st.k0, st.kc)


def _param_as(job, p):
    kind, _, N, K, _, _ = job
    w = p.detach().cpu().numpy()
    return w.reshape(N, K, 3, 3) if kind in (0, 1, 3, 5) else w.reshape(N, K)


def test_plans_pack_what_their_tables_name(monkeypatch):
    """The i32_b2 inference plan of tests/test_gpu_forward_ledger.py and the training plan of the same model: after one forward every
    buffer of _pack_jobs / _bf16_jobs and of the training plan's pack table holds the restatement of its parameter."""
    import test_gpu_forward_ledger as fwd
    from anoddpm_amd import _lib
    model, x, t = fwd._model("i32_b2", monkeypatch, torch.device(DEV))
    B, S = x.shape[0], x.shape[2]
    named = dict(model.named_parameters())
    by_ptr = {p.data_ptr(): k for k, p in named.items()}
    fails, seen = [], set()

    def check(what, key, job, buf):
        w = _param_as(job, named[key])
        got = buf.reshape(-1)[:pc.out_floats(job)].cpu().numpy()
        seen.add((what, job[0], job[1]))
        for f in pc.judge(job, w, got):
            fails.append(f"{what} {key} {pc.job_id(job)}: {f}")
        _note(job, w, got, f"{what} {key}")

    def tensors(plan):
        return {tt.data_ptr(): tt for tt in plan.keep if isinstance(tt, torch.Tensor) and tt.dtype == torch.float32}

    _guarded(lambda: model.forward_hip(x, t))
    plan = model._plan_for(B, S, x.device)
    bufs = tensors(plan)
    assert plan._pack_jobs
    for key, st in plan._pack_jobs:
        check("inference", key, _job_of(st), bufs[st.out])
    for key, dst, N, K in plan._bf16_jobs:
        w = named[key].detach().cpu().numpy()
        fails += [f"inference {key} bf16 planes: {f}" for f in pc.judge_bf16(N, K, w, dst.view(torch.int16)[:108 * N * K].cpu().numpy().view(np.uint16))]
    model.train()
    tp = model._train_plan_for(B, S, x.device, False, 0.0)
    _guarded(lambda: tp.run_forward(x.contiguous(), t.contiguous()))
    bufs = tensors(tp)
    assert tp.pack_ops
    for code, st in tp.pack_ops:
        assert code == _lib.OP_PACK
        check("training", by_ptr[st.w], _job_of(st), bufs[st.out])
    print("layouts the plans pack:", sorted(seen))
    assert {k for _, k, _ in seen} >= {0, 2, 3, 4} and any(b for w_, _, b in seen if w_ == "training"), sorted(seen)
    assert not fails, "\n".join(fails[:20])
