"""CPU: the layout restatements and bars of tests/pack_cases.py, which tests/test_gpu_pack_elements.py holds the device weight packers
to.  Each restatement against the host packers of tests/hipops.py (_pack_conv, _pack_wino, _pack_wino43; the data-gradient layouts
through the flipped and transposed weight), against a convolution identity (a direct fp64 3x3 correlation equals the Winograd
evaluation through the restated U, for F(2x2,3x3) and F(4x4,3x3), forward and data gradient), the item counts against the layouts,
the job tables against what they are there for, and the bf16 checks on correct, truncated, swapped and missing planes."""
import numpy as np
import pytest
import torch

import pack_cases as pc


def test_job_lists():
    jobs = pc.single_jobs()
    assert len(set(jobs)) == len(jobs)
    assert {(k, b) for k, b, *_ in jobs} == {(0, 0), (0, 1), (1, 0), (1, 1), (5, 0), (5, 1), (2, 0), (2, 1), (3, 0), (4, 0)}
    conv = {(N, K, b) for k, b, N, K, _, _ in jobs if k == 5}
    assert conv == {(4, 4, 0), (4, 4, 1), (64, 32, 0), (64, 32, 1), (96, 36, 0), (96, 36, 1), (12, 20, 0), (12, 20, 1), (260, 8, 0), (260, 8, 1), (3, 8, 0)}
    assert pc.items((5, 0, 4, 4, 0, 0)) == 4                     # one input-channel quad: four items (one per filter), one block
    assert pc.items((5, 0, 260, 8, 0, 0)) == 520 and pc.blocks((5, 0, 260, 8, 0, 0)) == 3
    assert [len(t) for t in pc.JOB_TABLES] == [1, 2, 13]
    table = pc.JOB_TABLES[2]
    assert {(k, b) for k, b, *_ in table} == {(0, 0), (0, 1), (1, 0), (1, 1), (5, 0), (5, 1), (2, 0), (2, 1), (3, 0), (4, 0)}
    counts = [pc.blocks(j) for j in table]
    assert {1, 2, 3} <= set(counts) and max(counts) >= 9
    assert counts[0] == 1 and counts[-1] == 1 and any(n >= 3 for n in counts[1:-1])
    for job in jobs + list(table):
        v, S = pc.restate(job, pc.weights(job))
        assert v.size == pc.out_floats(job) and (S is None) == (job[0] in (0, 2, 3, 4))


@pytest.mark.parametrize("job", pc.conv_jobs(), ids=pc.job_id)
def test_conv_layouts_are_the_host_packers(job):
    from hipops import _pack_conv, _pack_wino, _pack_wino43
    kind, bwd = job[:2]
    w = pc.weights(job)
    wp = torch.from_numpy(np.ascontiguousarray(pc.effective(w, bwd)).astype(np.float32))       # a permutation of fp32 values: exact
    host = {0: _pack_conv, 1: _pack_wino, 5: _pack_wino43}[kind](wp).numpy().reshape(-1)
    assert not pc.judge(job, w, host), pc.judge(job, w, host)
    want, S = pc.restate(job, w)
    if S is None:
        assert np.array_equal(host.view(np.uint32), want.astype(np.float32).view(np.uint32))
    print(f"{pc.job_id(job)}: host packer at {pc.worst_ulp(job, w, host):.3f} of the bar")


def test_pointwise_small_and_copy_layouts():
    from hipops import _pack_conv
    for job in pc.single_jobs():
        kind, bwd, N, K, k0, kc = job
        w = pc.weights(job)
        want = pc.restate(job, w)[0].astype(np.float32)
        if kind == 2 and not bwd:
            assert np.array_equal(want, _pack_conv(torch.from_numpy(w).view(N, K, 1, 1)).numpy().reshape(-1))
        elif kind == 2:
            wt = torch.from_numpy(w)[:, k0:k0 + kc].t().contiguous()                           # W'[o][i = n]
            assert np.array_equal(want, _pack_conv(wt.view(kc, N, 1, 1)).numpy().reshape(-1))
        elif kind == 3:
            assert np.array_equal(want, torch.from_numpy(w).permute(2, 3, 1, 0).reshape(-1).numpy())
        elif kind == 4:
            assert np.array_equal(want, w.reshape(-1))


def _correlate(d, g):
    """d [I][h][w], g [O][I][3][3] -> valid correlation [O][h - 2][w - 2], fp64."""
    h, w = d.shape[1] - 2, d.shape[2] - 2
    out = np.zeros((g.shape[0], h, w))
    for a in range(3):
        for b in range(3):
            out += np.einsum("oi,ihw->ohw", g[:, :, a, b], d[:, a:a + h, b:b + w])
    return out


@pytest.mark.parametrize("kind,BT,AT", [(1, pc.BT23, pc.AT23), (5, pc.BT43, pc.AT43)], ids=["F(2x2,3x3)", "F(4x4,3x3)"])
@pytest.mark.parametrize("bwd", [0, 1])
def test_winograd_layout_evaluates_the_convolution(kind, BT, AT, bwd):
    """Y = A^T [U o (B^T d B)] A summed over the input channels, U read back out of the restated layout [xi][i / 4][o][i % 4], is
    the direct 3x3 correlation of the tile with W' (forward: w; data gradient: the flipped, transposed w)."""
    job = (kind, bwd, 12, 20, 0, 0)
    w = pc.weights(job)
    U, S = pc.restate(job, w)
    O, I = (20, 12) if bwd else (12, 20)
    n = BT.shape[0]
    U = U.reshape(n, n, I // 4, O, 4).transpose(0, 1, 3, 2, 4).reshape(n, n, O, I)
    d = np.random.default_rng(3).standard_normal((I, n, n))
    V = np.einsum("ua,iab,vb->uvi", BT, d, BT)
    Y = np.einsum("ku,uvo,lv->okl", AT, np.einsum("uvoi,uvi->uvo", U, V), AT)
    direct = _correlate(d, pc.effective(w, bwd))
    assert Y.shape == direct.shape and np.abs(Y - direct).max() <= 1e-12 * np.abs(direct).max()


def test_data_gradient_weights_are_the_gradient_of_the_forward():
    """W'[k][n][a][b] = w[n][k][2 - a][2 - b]: correlating dy (zero-padded by one) with W' is autograd's gradient of
    conv2d(x, w, padding=1) with respect to x."""
    job = (0, 1, 12, 20, 0, 0)
    w = pc.weights(job)
    x = torch.zeros(1, 20, 5, 7, dtype=torch.float64, requires_grad=True)
    dy = torch.from_numpy(np.random.default_rng(4).standard_normal((1, 12, 5, 7)))
    torch.nn.functional.conv2d(x, torch.from_numpy(w).double(), padding=1).backward(dy)
    got = _correlate(np.pad(dy[0].numpy(), ((0, 0), (1, 1), (1, 1))), pc.effective(w, 1))
    assert np.abs(got - x.grad[0].numpy()).max() <= 1e-12 * np.abs(got).max()


def _planes(N, K, w, split):
    U, _ = pc.bf16_restate(N, K, w)
    h, m, lo = split(U.astype(np.float32))
    return [(p.view(np.uint32) >> 16).astype(np.uint16) for p in (h, m, lo)]


def _truncating(f):
    h = (f.view(np.uint32) & 0xFFFF0000).view(np.float32)
    r = f - h
    m = (r.view(np.uint32) & 0xFFFF0000).view(np.float32)
    r2 = r - m
    return h, m, (r2.view(np.uint32) & 0xFFFF0000).view(np.float32)


@pytest.mark.parametrize("N,K", pc.BF16_SHAPES)
def test_bf16_checks(N, K):
    """The nearest-even split passes; a truncating split is not the nearest-even statement; swapped, missing and copied planes fail."""
    w = pc.weights((5, 0, N, K, 0, 0))
    h, m, lo = _planes(N, K, w, pc.split3)
    assert not pc.judge_bf16(N, K, w, np.concatenate([h, m, lo]))
    assert pc.judge_bf16(N, K, w, np.concatenate(_planes(N, K, w, _truncating)))
    z = np.zeros_like(lo)
    for what, planes in (("mid and lo swapped", [h, lo, m]), ("hi and mid swapped", [m, h, lo]), ("lo missing", [h, m, z]),
                         ("mid missing", [h, z, lo]), ("lo a copy of mid", [h, m, m])):
        assert pc.judge_bf16(N, K, w, np.concatenate(planes)), what
    assert pc.judge_bf16(N, K, w, np.concatenate([h, m]))                            # a plane short


def test_judge_sees_a_wrong_element():
    job = (5, 0, 64, 32, 0, 0)
    w = pc.weights(job)
    good = pc.restate(job, w)[0].astype(np.float32)
    assert not pc.judge(job, w, good)
    bad = good.copy()
    i = int(np.argmax(np.abs(bad)))
    bad[i] = np.nextafter(np.nextafter(bad[i], np.float32(np.inf)), np.float32(np.inf))        # two places off: beyond one rounding
    assert pc.judge(job, w, bad)
    bad = good.copy()
    bad[5] = np.nan
    assert pc.judge(job, w, bad)
    job0 = (0, 1, 12, 20, 0, 0)
    w0 = pc.weights(job0)
    good0 = pc.restate(job0, w0)[0].astype(np.float32)
    assert not pc.judge(job0, w0, good0)
    good0[[3, 4]] = good0[[4, 3]]
    assert pc.judge(job0, w0, good0)
