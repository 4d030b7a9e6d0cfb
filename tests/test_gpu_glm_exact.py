"""GPU: kfac_kron_cov, kfac_kron_cov_outer, kfac_kron_cov_sweep and kfac_kron_cov_outer_sweep
on the integer cases of glm_exact_cases.py, through the raw C entry points.

Every operand of a case and its `cov` sit in ONE NaN-filled buffer; the workspace is a buffer
of its own, [256 guard bytes 0xA5 | exactly *_workspace_bytes of 0xFF (every float a NaN) |
256 guard bytes], and the call gets the interior pointer and the query's answer as its size.
After the call the WHOLE flat buffer must equal `want`: `cov` the int64 reference (the cases'
partial sums stay below 2^24, test_glm_exact_cases_host.py, so fp32 is exact in any order), the
inputs, their padding and the gaps untouched, NaN matching NaN.  Both guards must be
unchanged (the call stays inside what the query asks for) and `cov` holds no NaN (the call
reads no workspace it has not written).  The workspace interior is the only region not
compared.  One call of eight mixed jobs per route, plain and accumulated onto an integer
prefill, and one call per route with a workspace one byte short."""
import numpy as np
import pytest
import torch

import glm_exact_cases as E

pytestmark = pytest.mark.gpu


def _N():
    from bnn_kfac_amd import _native as N
    return N


def _guarded(dev, need):
    ws = torch.empty(need + 2 * E.GUARD, dtype=torch.uint8, device=dev)
    ws.fill_(0xA5)
    ws[E.GUARD:E.GUARD + need].fill_(0xFF)
    assert (ws.data_ptr() + E.GUARD) % 256 == 0
    return ws


def _run(dev, cid, short=0):
    """(status, flat buffer after the call, workspace after the call, the query's answer)."""
    N = _N()
    c = E.case(cid)
    buf = torch.from_numpy(np.array(c.flat)).to(dev)
    assert buf.data_ptr() % 16 == 0  # (the cases' alignment is relative to the buffer)
    jobs = E.native_jobs(N, c, buf.data_ptr())
    need = E.workspace_bytes(N, c, jobs)
    assert need > 0
    ws = _guarded(dev, need)
    rc = E.call(N, c, jobs, buf.data_ptr(), ws.data_ptr() + E.GUARD, need - short, N.stream_handle(dev))
    torch.cuda.synchronize(dev)
    return rc, buf.cpu().numpy(), ws.cpu().numpy(), need


def _check(dev, cid):
    N = _N()
    c = E.case(cid)
    rc, got, ws, need = _run(dev, cid)
    assert rc == N.KFAC_OK, rc
    expect = E.want(c)
    bad = E.differing(got, expect)
    assert E.same(got, expect), (f"{len(bad)} elements differ; first at element {bad[0]} ({E.region_of(c, bad[0])}; "
                                 f"cov at {c.cov.off}, shape {c.cov_shape}): got {got[bad[0]]!r}, "
                                 f"want {expect[bad[0]]!r}")
    assert not np.isnan(got[c.cov.off:c.cov.end]).any()
    assert (ws[:E.GUARD] == 0xA5).all() and (ws[E.GUARD + need:] == 0xA5).all(), \
        f"the call wrote outside its {need} workspace bytes"


@pytest.mark.parametrize("cid", E.SINGLE_IDS["dense"])
def test_kron_cov_whole_buffer(hip_device, cid):
    _check(hip_device, cid)


@pytest.mark.parametrize("cid", E.SINGLE_IDS["outer"])
def test_kron_cov_outer_whole_buffer(hip_device, cid):
    _check(hip_device, cid)


@pytest.mark.parametrize("cid", E.SINGLE_IDS["sweep"])
def test_kron_cov_sweep_whole_buffer(hip_device, cid):
    _check(hip_device, cid)


@pytest.mark.parametrize("cid", E.SINGLE_IDS["outer_sweep"])
def test_kron_cov_outer_sweep_whole_buffer(hip_device, cid):
    _check(hip_device, cid)


@pytest.mark.parametrize("cid", [cid for r in E.ROUTES for cid in E.JOBS8_IDS[r]])
def test_eight_mixed_jobs_whole_buffer(hip_device, cid):
    """cov = the int64 sum over the eight jobs, plain and accumulated onto an integer prefill:
    cov_find_job, the per-job carve-up of the workspace and the job-order sum."""
    c = E.case(cid)
    assert len(c.jobs) == 8 and len({(j.nA, j.nG) for j in c.jobs}) >= 5
    _check(hip_device, cid)


@pytest.mark.parametrize("route", E.ROUTES)
def test_workspace_one_byte_short(hip_device, route):
    """KFAC_EWORKSPACE before any launch: neither the workspace nor cov changes."""
    N = _N()
    cid = E.JOBS8_IDS[route][1]  # (accumulate: cov holds numbers that must stay)
    c = E.case(cid)
    rc, got, ws, need = _run(hip_device, cid, short=1)
    assert rc == N.KFAC_EWORKSPACE, rc
    assert E.same(got, c.flat)
    assert (ws[E.GUARD:E.GUARD + need] == 0xFF).all() and (ws[:E.GUARD] == 0xA5).all() and \
        (ws[E.GUARD + need:] == 0xA5).all()
