"""GPU: the eigensolver on factor-shaped spectra (eig_cases.py), with strided operands, in a
mixed group, and under its two launch knobs.  Every bound is one of eig_cases' derived ones."""
import numpy as np
import pytest
import torch

import eig_cases as E

pytestmark = pytest.mark.gpu


def _solve(mats, dev, vectors=True, pad_f=0, pad_v=0):
    """One kfac_syev call through the raw ABI.  Every operand lives in a NaN-filled buffer
    (F with `pad_f`, evecs with `pad_v` extra columns).  Returns [(ev, V, V's padding)], info."""
    from bnn_kfac_amd import _native as N
    jobs, bufs = [], []
    for F in mats:
        n = F.shape[0]
        fb = torch.full((n, n + pad_f), float("nan"), dtype=torch.float32, device=dev)
        fb[:, :n] = torch.tensor(F)  # (a copy: the shared cases are read-only)
        ev = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
        vb = torch.full((n, n + pad_v), float("nan"), dtype=torch.float32, device=dev) if vectors else None
        j = N.EigJob()
        j.F, j.ldF, j.n = fb.data_ptr(), n + pad_f, n
        j.evals, j.evecs, j.ldv = ev.data_ptr(), N.ptr(vb), n + pad_v
        jobs.append(j)
        bufs.append((fb, ev, vb))
    info = N.syev(jobs, dev).cpu().numpy()
    out = []
    for F, (_, ev, vb) in zip(mats, bufs):
        n = F.shape[0]
        vb = vb.cpu().numpy() if vectors else None
        out.append((ev.cpu().numpy(), np.ascontiguousarray(vb[:, :n]) if vectors else None,
                    vb[:, n:] if vectors else None))
    return out, info


def _check_case(name, n, dev):
    F = E.matrix(name, n)
    ((ev, V, _),), info = _solve([F], dev)
    want = E.lapack(name, n)[0]
    f = E.figures(F, ev, V, want)
    print(f"{name}-{n}: info {info[0]} ev {f['ev']:.2e} orth {f['orth']:.2e} res {f['res']:.2e}")
    E.check(F, ev, V, want, info[0])
    return ev, V


@pytest.mark.parametrize("name,n", E.CASES, ids=E.CASE_IDS)
def test_spectrum(hip_device, name, n):
    ev, _ = _check_case(name, n, hip_device)
    if n > E.LARGE:  # the vectors call's eigenvalues are the values-only call's
        ((ev2, _, _),), info = _solve([E.matrix(name, n)], hip_device, vectors=False)
        assert info[0] == 0
        np.testing.assert_array_equal(ev, ev2)


@pytest.mark.parametrize("n", [33, 129])
def test_strided_operands(hip_device, n):
    """ldF = n + 3, ldv = n + 5: the same bits as the contiguous call, padding untouched."""
    F = E.matrix("kfac_A", n)
    ((ev0, V0, _),), info0 = _solve([F], hip_device)
    ((ev1, V1, pad),), info1 = _solve([F], hip_device, pad_f=3, pad_v=5)
    assert info0[0] == 0 and info1[0] == 0
    E.check(F, ev0, V0, E.lapack("kfac_A", n)[0])
    np.testing.assert_array_equal(ev1, ev0)
    np.testing.assert_array_equal(V1, V0)
    assert pad.shape == (n, 5) and np.isnan(pad).all()


def _check_group_against_solo(sizes, seed, dev):
    mats = [E.factor_like(n, seed + i) for i, n in enumerate(sizes)]
    group, info = _solve(mats, dev)
    assert not info.any(), info
    for F, (ev, V, _) in zip(mats, group):
        ((ev1, V1, _),), info1 = _solve([F], dev)
        E.check(F, ev1, V1, np.linalg.eigvalsh(F.astype(np.float64)), info1[0])
        np.testing.assert_array_equal(ev, ev1)
        np.testing.assert_array_equal(V, V1)


def test_mixed_group(hip_device):
    """Nine small jobs interleaved with three large ones.  Every large job closes the pending
    small group, so the Jacobi launches are {40}, {7, 128}, {1, 2, 64, 33, 12} and {5}, each
    followed (but the last) by a large job in the same workspace.  Every job's output equals
    its solo solve bit for bit."""
    assert [len(g) for g in E.jacobi_groups(E.MIXED_SIZES)] == [1, 2, 5, 1]
    _check_group_against_solo(E.MIXED_SIZES, 1000, hip_device)


def test_full_jacobi_groups(hip_device):
    """Jacobi launches of 8, 8, 2, 8, 1 and 1 jobs in one call: two full groups back to back
    (the workspace pointer starts over between them), a large job in the workspace they used,
    a full group of the largest matrices right after it, another large job.  Bit for bit the
    solo solves."""
    assert [len(g) for g in E.jacobi_groups(E.FULL_SIZES)] == [8, 8, 2, 8, 1, 1]
    _check_group_against_solo(E.FULL_SIZES, 2000, hip_device)


KNOB_CASES = (("kfac_A", 192), ("chain_straddle", 192), ("glued_wilkinson_rot", 147))
KNOB_DEFAULTS = {"KFAC_EIG_RB": 4, "KFAC_EIG_G": 0}
_knob_default = {}  # (case, n) -> (ev, V) of the default launch, solved once


@pytest.mark.parametrize("knob,value", [("KFAC_EIG_RB", 8), ("KFAC_EIG_G", 2), ("KFAC_EIG_G", 64),
                                        ("KFAC_EIG_G", 256)])
@pytest.mark.parametrize("name,n", KNOB_CASES, ids=[f"{c}-{n}" for c, n in KNOB_CASES])
def test_knobs(hip_device, name, n, knob, value):
    """Eight rows per batch; 2 workgroups (many rows each), 64, and 256 (more workgroups
    than rows: the surplus own no row and only take part in the exchange).  The bounds hold,
    and the bits are the default launch's: a row's dot product is split over the threads of
    its owner by column and summed by a fixed tree, the scalars c and sigma are summed from
    the gathered values by the same tree in every workgroup, so neither the owner of a row
    nor the batch it is read in enters any sum.  (A kernel that re-partitions those sums by
    workgroup or batch would have to drop the two equality lines, not the bounds.)"""
    from bnn_kfac_amd import _native as N
    before = {k: N.get_knob(k) for k in ("KFAC_EIG_RB", "KFAC_EIG_G")}
    try:
        for k, v in KNOB_DEFAULTS.items():  # (whatever the environment set at load)
            N.set_knob(k, v)
        if (name, n) not in _knob_default:
            _knob_default[name, n] = _check_case(name, n, hip_device)
        ev0, V0 = _knob_default[name, n]
        N.set_knob(knob, value)
        assert N.get_knob(knob) == value
        ev, V = _check_case(name, n, hip_device)
    finally:
        for k, v in before.items():
            N.set_knob(k, v)
    assert {k: N.get_knob(k) for k in before} == before
    np.testing.assert_array_equal(ev, ev0)
    np.testing.assert_array_equal(V, V0)
