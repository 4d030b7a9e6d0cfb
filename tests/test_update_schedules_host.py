"""CPU: the queue schedules of tests/update_schedule_cases.py through the host double of the
device calls (host_double: fp64 through square-root weights, one split per accumulator), and
what test_gpu_update_schedules.py relies on: the table covers every knob value, and every sum is
exact in fp32 in any order."""
import numpy as np
import pytest

import host_double
import update_schedule_cases as S


def test_table_covers_the_knobs():
    T = S.SCHEDULES
    assert len(T) >= 24
    assert {s.pattern for s in T} == set(S.PATTERNS) and {s.net for s in T} == set(S.NETS)
    assert {s.defer_batches for s in T} == set(S.DEFER_BATCHES)
    assert {s.launch_first for s in T} == set(S.LAUNCH_FIRST)
    for knob in ("defer_reduce", "merge_launches", "double_buffer"):
        assert {getattr(s, knob) for s in T} == {True, False}, knob
    assert {s.read_mid is None for s in T} == {True, False}
    small = [s for s in T if s.defer_bytes < 2 * S.update_bytes(s.net, max(s.sizes))]
    assert small and len(small) < len(T)
    for s in T:
        assert set(s.sizes) <= {64, 32, 16}
    long = [s for s in T if s.pattern == "70 updates"]
    assert long and all(len(s.sizes) == 70 and s.launch_first == s.defer_batches == 128 and s.defer_reduce for s in long)
    # the deferred queue with merged launches, short batches and a cached third pass all occur together
    assert any(s.defer_reduce and s.merge_launches and s.launch_first >= 16 and len(set(s.sizes)) > 1 for s in T)


@pytest.mark.parametrize("s", S.SCHEDULES, ids=S.IDS)
def test_sums_are_exact(s):
    for p in range(S.PASSES):
        assert 0 < S.bound(s, p) < 2 ** 24
        for F in S.reference(s, p):
            assert np.array_equal(F.astype(np.float32).astype(np.float64), F) and np.array_equal(F, F.T)
    assert not np.array_equal(S.reference(s, 0)[0], S.reference(s, 1)[0])


@pytest.mark.parametrize("s", S.SCHEDULES, ids=S.IDS)
def test_schedule_through_the_double(monkeypatch, s):
    import torch
    from bnn_kfac_amd.curvatures import KFAC
    host_double.install(monkeypatch)
    host_double.UPDATES.clear()
    slow, per_pass, nseg = [], [], []
    orig = KFAC._remember
    monkeypatch.setattr(KFAC, "_remember", lambda self, *a, **k: (slow.append(1), orig(self, *a, **k))[1])

    def compare(what, got, want):
        np.testing.assert_allclose(got.numpy(), want, rtol=1e-6, err_msg=what)

    def after_pass(kfac, p):
        per_pass.append(len(slow))
        nseg.append(max(max(u) for u in host_double.UPDATES))
        host_double.UPDATES.clear()

    S.run(s, torch.device("cpu"), compare, after_pass)
    if s.defer_reduce:
        # the third pass runs on cached templates alone
        assert per_pass[2] == per_pass[1], per_pass
    if s.pattern == "70 updates":
        assert nseg == [70] * 3  # one flush past KSEG batch bases, from Python
    elif not s.defer_reduce:
        assert nseg == [1] * 3
