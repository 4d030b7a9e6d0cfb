"""GPU: the conv factor kernels against an int64 reference, bit for bit, over the cases of
tests/conv_factor_cases.py (test_conv_factor_cases_host.py proves on the host that the data is
exact in every summation order, what the sweep covers, and that each planted mistake of the model
shows on the cases named for it).

Raw C ABI.  Per case: the profile slot of the routed family counted exactly the expected launches
and no other factor family launched; the WHOLE F buffer equals the expectation (the n x n region,
and NaN in the ldF padding and around F); the input buffers are bitwise what was uploaded.  Images
lie sB > C H W apart in NaN, so a read outside an image is a NaN in F."""
import numpy as np
import pytest
import torch

import conv_factor_cases as C

pytestmark = pytest.mark.gpu


def _report(case, got, want):
    """Why `got` (the whole F buffer) is not `want`: the first wrong entry of the region, or the
    first touched float outside it."""
    n, ld = case.n, case.ldF
    at = C.F_OFF + np.arange(n)[:, None] * ld + np.arange(n)[None, :]
    g, w = got[at].astype(np.float64), want[at]
    bad = np.argwhere(~(g == w))
    head = f"{case.id} ({case.layout}, family {case.family}, n = {n}, alpha {case.alpha}, beta {case.beta})"
    if len(bad):
        i, j = (int(v) for v in bad[0])
        blocks = sorted({(int(a) // 32, int(b) // 32) for a, b in bad})
        nan = bool(np.isnan(g[i, j]))
        return (f"{head}: F[{i}][{j}] (32 x 32 block ({i // 32}, {j // 32})) got {g[i, j]!r} want {w[i, j]!r}"
                f"{' -- NaN: a read outside an image' if nan else ''}; {len(bad)} entries in {len(blocks)} "
                f"blocks differ, first blocks {blocks[:8]}; NaN entries {int(np.isnan(g).sum())}")
    outside = np.ones(got.size, dtype=bool)
    outside[at] = False
    k = int(np.flatnonzero(outside & ~np.isnan(got))[0])
    return f"{head}: float {k - C.F_OFF} from F[0][0] (row {(k - C.F_OFF) // ld}, column {(k - C.F_OFF) % ld}) " \
           f"is outside the n x n region and was written: {got[k]!r}"


def _run(N, dev, case):
    """Runs the case; returns None or what is wrong."""
    host = C.inputs(case)
    bufs = [torch.from_numpy(b).to(dev) for b in host]
    F = torch.from_numpy(C.f_buffer(case)).to(dev)
    ptrs = [b.data_ptr() + 4 * case.guard for b in bufs]
    F_ptr = F.data_ptr() + 4 * C.F_OFF
    assert len({p % 16 for p in ptrs}) == 1
    keep = []
    N.profile_reset()
    N.profile_enable(True)
    try:
        if case.steps:
            j0, _ = C.job(N, case, ptrs, F_ptr, case.steps[0], 1)
            (splits, nbytes), = N.factor_accum_plan([j0])
            assert splits == case.splits
            acc = torch.full((nbytes // 4,), float("nan"), device=dev)
            for m, _, acc_beta in C.updates(case):
                j, _ = C.job(N, case, ptrs, F_ptr, m, 1)
                j.acc, j.acc_splits, j.acc_beta = acc.data_ptr(), splits, acc_beta
                N.factor_update([j], dev)
            j.alpha = 1.0  # (the partials carry alpha)
            N.factor_flush([j], dev)
        else:
            j, table = C.job(N, case, ptrs, F_ptr)
            keep.append(table)
            N.factor_update([j], dev)
        torch.cuda.synchronize()
    finally:
        N.profile_enable(False)
    counts = {name: N.profile_read(slot)[1] for slot, name in N.PROF_FACTOR_KERNELS.items()}
    want_counts = {name: 0 for name in counts}
    want_counts[N.PROF_FACTOR_KERNELS[{v: k for k, v in C.FAMILY.items()}[case.family]]] = C.launches(case)
    if counts != want_counts:
        return f"{case.id}: launches {counts}, expected {want_counts}"
    got, want = F.cpu().numpy(), C.expected(case)
    if not np.array_equal(got.astype(np.float64), want, equal_nan=True):
        return _report(case, got, want)
    for s, (b, h) in enumerate(zip(bufs, host)):
        if not np.array_equal(b.view(torch.int32).cpu().numpy(), h.view(np.int32)):
            return f"{case.id}: input buffer {s} changed"
    return None


def _run_all(dev, cases):
    from bnn_kfac_amd import _native as N
    assert cases
    failed = [msg for msg in (_run(N, dev, c) for c in cases) if msg]
    assert not failed, f"{len(failed)} of {len(cases)} cases:\n" + "\n".join(failed[:12])


@pytest.mark.parametrize("family", C.PATCH_FAMILIES)
def test_patch_sweep_exact(hip_device, family):
    cases = [c for c in C.patch_sweep()[0] if c.family == family]
    assert len(cases) >= C.FLOORS[family]
    if family == "conv_x3f":
        # conv_x3f_geom memoizes a shape's geometry and refreshes B / bseg alone: each case
        # again at B = 5, exact whether the search or the memo served it
        again = C.route([C.with_batch(c, 5) for c in cases])
        assert all(c.family == family for c in again)
        cases = [c for pair in zip(cases, again) for c in pair]
    _run_all(hip_device, cases)


@pytest.mark.parametrize("family", ("channel_small", "channel_x3", "conv", "tiles"))
def test_channel_sweep_exact(hip_device, family):
    _run_all(hip_device, [c for c in C.channel_sweep() if c.family == family])


FIXED = [(mode, name) for mode in ("large", "multi", "deferred") for name, *_ in C.LARGE] + [("multi", "tiles")]


@pytest.mark.parametrize("mode,name", FIXED)
def test_large_shapes_exact(hip_device, mode, name):
    """Tasks of two and three images (immediate), a task across the boundary of two batches in
    separate allocations (multi), tasks without an image that must leave their slab alone (deferred)."""
    case, = [c for c in C.fixed()[mode] if c.id == f"{mode}[{name}]"]
    _run_all(hip_device, [case])
