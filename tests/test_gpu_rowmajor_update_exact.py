"""GPU: kfac_factor_update's row-major path against an int64-exact reference, bit for bit, over
the cases of tests/rowmajor_update_cases.py (test_rowmajor_update_cases_host.py proves on the host
that every sum is exact in any order, that the routes and launch counts follow from
kfac_factor_route and the model of update_group, and that each planted mistake shows on the cases
named for it).

Raw C ABI, one call per case (deferred cases: one call and one kfac_factor_flush) into a
workspace of exactly kfac_factor_workspace_bytes bytes between two guards.  After one
synchronize: every profile slot counted exactly the modelled launches; the WHOLE F buffer equals
the expectation (every job's n x n region, NaN in the ldF padding and around every F); the input
buffer is bitwise what was uploaded; the workspace guards are intact."""
import ctypes

import numpy as np
import pytest
import torch

import rowmajor_update_cases as C

pytestmark = pytest.mark.gpu

CASES = C.all_cases()
WS_GUARD = 256


def _report(c, got, want):
    """Why `got` (the whole F buffer) is not `want`: per job the first wrong entry of its
    region, or the first touched float outside every region."""
    inside = np.zeros(got.size, dtype=bool)
    for i in C.factors(c):
        j, at = c.jobs[i], C.region(c, i)
        inside[at] = True
        g, w = got[at].astype(np.float64), want[at]
        bad = np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))
        if len(bad):
            r, k = (int(v) for v in bad[0])
            blocks = sorted({(int(a) // 32, int(b) // 32) for a, b in bad})
            nan = bool(np.isnan(g[r, k]))
            batches = f"{len(j.batches)} x {j.rows}" + (f", the last {j.last}" if j.last else "")
            return (f"{c.id}: job {i} (n = {j.n}, cols {j.cols}, ld {j.ld}, batches {batches}, alpha {j.alpha}, "
                    f"beta {j.beta}): F[{r}][{k}] (32 x 32 block ({r // 32}, {k // 32})) got {g[r, k]!r} want "
                    f"{w[r, k]!r}{' -- NaN: a read outside a batch, or an entry never written' if nan else ''}; "
                    f"{len(bad)} entries in {len(blocks)} blocks differ, first blocks {blocks[:8]}; "
                    f"NaN entries {int(np.isnan(g).sum())}")
    k = int(np.flatnonzero(~inside & ~np.isnan(got))[0])
    return f"{c.id}: float {k} of the F buffer lies outside every n x n region and was written: {got[k]!r}"


def _call(N, dev, c, short=0):
    """Uploads the case and makes its call(s); returns what the checks need."""
    L = N.lib()
    Xd = torch.tensor(C.inputs(c), device=dev)
    Fd = torch.tensor(C.f_buffer(c), device=dev)
    acc, accs = None, {}
    if c.deferred:
        accs = {f: torch.full((C.acc_floats(c, f),), float("nan"), device=dev) for f in C.factors(c)}
        acc = {f: (t.data_ptr(), C.slab_stride(c, f)) for f, t in accs.items()}
    jobs, keep = C.make_jobs(N, c, Xd.data_ptr(), Fd.data_ptr(), acc=acc)
    arr = N.as_array(N.FactorJob, jobs)
    need = L.kfac_factor_workspace_bytes(arr, len(jobs))
    assert need == C.workspace_bytes(c), (c.id, need)
    ws = torch.full((WS_GUARD + need + WS_GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    ws[WS_GUARD:WS_GUARD + need] = 0xFF
    assert (ws.data_ptr() + WS_GUARD) % 256 == 0
    stream = N.stream_handle(dev)
    torch.cuda.synchronize()
    N.profile_reset()
    N.profile_enable(True)
    try:
        rc = L.kfac_factor_update(arr, len(jobs), ctypes.c_void_p(ws.data_ptr() + WS_GUARD), need - short, stream)
        if rc == N.KFAC_OK and c.deferred:
            fl = C.flush_jobs(N, c, Fd.data_ptr(), acc)
            rc = L.kfac_factor_flush(N.as_array(N.FactorJob, fl), len(fl), stream)
        torch.cuda.synchronize()
    finally:
        N.profile_enable(False)
    counts = {slot: N.profile_read(slot)[1] for slot in list(N.PROF_FACTOR_KERNELS) + [C.REDUCE]}
    return NS(rc=rc, counts=counts, F=Fd.cpu().numpy(), X=Xd.cpu().numpy(), ws=ws.cpu().numpy(), need=need, keep=keep)


class NS:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _names(N, counts):
    names = dict(N.PROF_FACTOR_KERNELS)
    names[C.REDUCE] = "kfac_factor_reduce"
    return {names[k]: v for k, v in counts.items() if v}


def _check(N, c, r):
    assert r.rc == N.KFAC_OK, f"{c.id}: the call returned {r.rc}"
    want_counts = C.launch_counts(c)
    assert r.counts == want_counts, f"{c.id}: launches {_names(N, r.counts)}, expected {_names(N, want_counts)}"
    want = C.expected(c)
    if not np.array_equal(r.F.astype(np.float64), want, equal_nan=True):
        pytest.fail(_report(c, r.F, want))
    assert np.array_equal(r.X.view(np.int32), C.inputs(c).view(np.int32)), f"{c.id}: the input buffer changed"
    g = r.ws
    assert (g[:WS_GUARD] == 0xA5).all() and (g[WS_GUARD + r.need:] == 0xA5).all(), \
        f"{c.id}: a workspace guard was written (workspace of {r.need} bytes)"


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_update_exact(hip_device, c):
    from bnn_kfac_amd import _native as N
    _check(N, c, _call(N, hip_device, c))


SHORT = ("glds[n132,rows2048]", "mixed[glds+staged]", "x3ragged[immediate]", "syrk3[2049,40]")


@pytest.mark.parametrize("cid", SHORT)
def test_workspace_one_byte_short(hip_device, cid):
    """KFAC_EWORKSPACE, nothing launched: F, the workspace and the inputs are what was uploaded."""
    from bnn_kfac_amd import _native as N
    c = C.get(cid)
    assert not c.deferred and len(C.plan(c)) == 1
    r = _call(N, hip_device, c, short=1)
    assert r.need > 0 and r.rc == N.KFAC_EWORKSPACE
    assert not any(r.counts.values()), _names(N, r.counts)
    assert np.array_equal(r.F.view(np.int32), C.f_buffer(c).view(np.int32))
    assert np.array_equal(r.X.view(np.int32), C.inputs(c).view(np.int32))
    assert (r.ws[:WS_GUARD] == 0xA5).all() and (r.ws[WS_GUARD + r.need:] == 0xA5).all()
    assert (r.ws[WS_GUARD:WS_GUARD + r.need] == 0xFF).all()


def test_rounds_are_deterministic(hip_device):
    """The 70 / 3 / 1 rounds case twice: bit-identical."""
    from bnn_kfac_amd import _native as N
    c = C.get("rounds[70/3/1,beta1]")
    a, b = _call(N, hip_device, c), _call(N, hip_device, c)
    _check(N, c, a)
    assert np.array_equal(a.F.view(np.int32), b.F.view(np.int32))
