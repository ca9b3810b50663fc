"""-m gpu: what the fifteen workgroup-era metric and post-processing entry points read and write, through the C ABI on hostile
buffers (tests/contract_cases.py: the table, the arenas, the checker; tests/test_contract_reference.py tests those on the CPU).

For every case of an entry point: three launches on fresh arenas whose workspace is pre-filled with all-zero bits, with all-one
bits and with exactly what the previous, different case left in its workspace; after each one every arena is copied back and
`check` must find nothing (guards and gaps intact, inputs intact, every element of a written set written and right by the rule
of the entry point's own GPU test, nothing written outside one, status words as expected), and the outputs of the three must
be bit-identical.  Then one call the library must refuse (the workspace one byte short; S = 0 for the entry points without a
workspace) has to return an error and leave every arena, the workspace included, bit-intact.

A launch that returns an error, or a device error at the synchronisation behind it, ends the module: no later test of this
file starts anything on the device.  A finding of the checker is a failed assertion, not a fault: every stray access the
arenas can catch lands inside an allocation of the test's own."""
import ctypes

import numpy as np
import pytest
import torch

import contract_cases as cc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_SIGNED = {1: np.uint8, 4: np.int32, 8: np.int64}            # torch.from_numpy takes these everywhere
_stop = []                                                   # why nothing further may be launched


def _upload(arenas):
    return {f: torch.from_numpy(a.bits.view(_SIGNED[a.bits.dtype.itemsize])).to(DEV) for f, a in arenas.items()}


def _download(arenas, dev):
    return {f: a.copy(dev[f].cpu().numpy()) for f, a in arenas.items()}


def _launch(call, ws_fill=0, refuse=False):
    """One call on fresh arenas -> (return code, arenas before, arenas after)."""
    from anoddpm_amd import _lib
    L = _lib.lib()
    if _stop:
        pytest.fail(f"not started: {_stop[0]}")
    before = cc.build_arenas(call, cc.workspace_bytes(call, L), ws_fill)
    dev = _upload(before)
    a = cc.fill_struct(call, before, {f: t.data_ptr() for f, t in dev.items()}, ws_short=1 if refuse and "workspace" in before else 0)
    if refuse and "workspace" not in before:
        a.S = 0
    try:
        with torch.cuda.device(DEV):
            code = getattr(L, "anoddpm_" + call["entry"])(ctypes.byref(a), _lib.current_stream())
            torch.cuda.synchronize()
        after = _download(before, dev)
    except Exception as e:                                   # a device error: nothing of this module runs after it
        _stop.append(f"{call['entry']} {call['id']}: {e}")
        raise
    if code != 0 and not refuse:
        _stop.append(f"{call['entry']} {call['id']}: error code {code}: {L.anoddpm_last_error()}")
        pytest.fail(_stop[0])
    return code, before, after


@pytest.mark.parametrize("entry", cc.ENTRY_POINTS)
def test_entry_point_keeps_its_contract_on_hostile_buffers(entry):
    from anoddpm_amd import _lib
    calls = cc.cases(entry)
    left = b""
    if cc.has_workspace(entry):                              # the first case gets what the last one leaves
        _, _, after = _launch(calls[-1])
        left = after["workspace"].get().tobytes()
    problems = []
    for call in calls:
        expected = cc.expected_of(call)
        fills = (0, 0xff, left) if cc.has_workspace(entry) else (0, 0)
        first = None
        for i, fill in enumerate(fills):
            _, before, after = _launch(call, fill)
            found = cc.check(call, before, after, expected, reference=first)
            if first is not None:                            # everything but the values, which the first launch answered for
                found += [f for f in cc.check(call, before, after, expected) if f[0] not in ("wrong_value", "status")]
            problems += [(call["id"], f"launch {i}") + f for f in found]
            first = after if first is None else first
            mine = after
        if cc.has_workspace(entry):
            left = mine["workspace"].get().tobytes()
        code, before, after = _launch(call, 0xff, refuse=True)
        assert code != 0 and _lib.lib().anoddpm_last_error(), (call["id"], "a call that must be refused was accepted")
        if cc.has_workspace(entry):
            assert cc.TABLE[entry]["too_small"] in _lib.lib().anoddpm_last_error(), call["id"]
        touched = [f for f in before if not np.array_equal(before[f].bits, after[f].bits)]
        assert not touched, (call["id"], "a refused call wrote to", touched)
    for p in problems[:40]:
        print(p)
    assert not problems, f"{len(problems)} finding(s) in {len({p[0] for p in problems})} of {len(calls)} cases; the first: {problems[0]}"
