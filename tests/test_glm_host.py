"""CPU: the host side of the GLM predictive (variance.posterior_jacobian /
probit_predictive) and the C ABI of kfac_kron_cov (struct layout, argument validation
before any launch, workspace query).  No GPU calls."""
import ctypes

import numpy as np
import pytest
import torch

from abi_layout import c_layout


def _loop_reference(dW, db):
    """M[a][g] = dW[g][a] (a < wcols), M[nA-1][g] = db[g], flattened a*nG + g."""
    nG = dW.shape[0]
    w = dW.reshape(nG, -1)
    wcols = w.shape[1]
    nA = wcols + (1 if db is not None else 0)
    out = np.zeros(nA * nG, dtype=np.float64)
    for g in range(nG):
        for a in range(wcols):
            out[a * nG + g] = w[g, a]
        if db is not None:
            out[(nA - 1) * nG + g] = db[g]
    return out


@pytest.mark.parametrize("wshape,bias", [((7, 12), True), ((7, 12), False), ((6, 3, 3, 3), True)])
def test_posterior_jacobian_matches_loop(wshape, bias):
    from bnn_kfac_amd.variance import posterior_jacobian
    rng = np.random.default_rng(0)
    lead = (2, 3)
    dW = rng.standard_normal(lead + wshape)
    db = rng.standard_normal(lead + wshape[:1]) if bias else None
    got = posterior_jacobian(torch.from_numpy(dW), torch.from_numpy(db) if bias else None,
                             batch_dims=2).numpy()
    nA = int(np.prod(wshape[1:])) + int(bias)
    assert got.shape == lead + (nA * wshape[0],)
    for i in range(lead[0]):
        for j in range(lead[1]):
            want = _loop_reference(dW[i, j], db[i, j] if bias else None)
            np.testing.assert_array_equal(got[i, j], want)
    # one layer's gradient, no leading dimensions (batch_dims derived from db / 0)
    one = posterior_jacobian(torch.from_numpy(dW[0, 0]), torch.from_numpy(db[0, 0]) if bias else None)
    np.testing.assert_array_equal(one.numpy(), got[0, 0])


def test_probit_predictive_properties():
    from bnn_kfac_amd.variance import probit_predictive
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(9, 10, generator=g) * 3
    R = torch.randn(9, 10, 10, generator=g)
    cov = R @ R.mT
    p0 = probit_predictive(logits, torch.zeros_like(cov))
    torch.testing.assert_close(p0, torch.softmax(logits, dim=1), rtol=0, atol=0)
    p1 = probit_predictive(logits, cov)
    p4 = probit_predictive(logits, 4 * cov)
    for p in (p0, p1, p4):
        torch.testing.assert_close(p.sum(dim=1), torch.ones(9), rtol=0, atol=1e-6)
    # scaling cov up lowers every row's maximum probability.  Checked with one variance
    # per row: it divides the whole row by one factor > 1 (a temperature), which provably
    # flattens the row; unequal variances can reorder the logits, so no such law holds.
    var = torch.rand(9, generator=g) + 0.5
    iso = torch.diag_embed(var.unsqueeze(1).expand(9, 10))
    q1, q4 = probit_predictive(logits, iso), probit_predictive(logits, 4 * iso)
    assert bool((q1.max(dim=1).values < p0.max(dim=1).values).all())
    assert bool((q4.max(dim=1).values < q1.max(dim=1).values).all())


def test_cov_struct_layout(tmp_path):
    from bnn_kfac_amd import _native as N
    got = c_layout(tmp_path, "kfac_cov_job", ("K1", "K2", "lower2"))
    assert got == [ctypes.sizeof(N.CovJob), N.CovJob.K1.offset, N.CovJob.K2.offset,
                   N.CovJob.lower2.offset]


def _valid_job(N, nA=5, nG=3):
    # (pointers are never dereferenced on the host: validation happens before any launch)
    return N.CovJob(1 << 12, nA * nG, nA, nG, 1 << 13, nA, 1 << 14, nG, 1, 1)


def test_kron_cov_validates_before_any_launch():
    from bnn_kfac_amd import _native as N
    lib = N.lib()
    arr = N.as_array(N.CovJob, [_valid_job(N)])
    out = 1 << 15
    assert lib.kfac_kron_cov(arr, 0, 2, 3, 0, out, None, 0, None) == N.KFAC_EINVAL
    assert lib.kfac_kron_cov(arr, 9, 2, 3, 0, out, None, 0, None) == N.KFAC_EINVAL
    assert lib.kfac_kron_cov(arr, 1, 2, 0, 0, out, None, 0, None) == N.KFAC_EINVAL
    assert lib.kfac_kron_cov(arr, 1, 2, 33, 0, out, None, 0, None) == N.KFAC_EINVAL
    assert lib.kfac_kron_cov(None, 1, 2, 3, 0, out, None, 0, None) == N.KFAC_EINVAL
    assert lib.kfac_kron_cov(arr, 1, 2, 3, 0, None, None, 0, None) == N.KFAC_EINVAL
    for field, value in (("J", None), ("K1", None), ("K2", None), ("ldJ", 14), ("ld1", 4), ("ld2", 2)):
        bad = _valid_job(N)
        setattr(bad, field, value)
        assert lib.kfac_kron_cov(N.as_array(N.CovJob, [bad]), 1, 2, 3, 0, out, None, 0,
                                 None) == N.KFAC_EINVAL, field
    # more than 2^31 tasks
    assert lib.kfac_kron_cov(arr, 1, 1 << 30, 32, 0, out, None, 0, None) == N.KFAC_EINVAL
    # a valid job with no workspace
    assert lib.kfac_kron_cov(arr, 1, 2, 3, 0, out, None, 0, None) == N.KFAC_EWORKSPACE
    need = lib.kfac_kron_cov_workspace_bytes(arr, 1, 2, 3)
    assert lib.kfac_kron_cov(arr, 1, 2, 3, 0, out, 1 << 16, need - 1, None) == N.KFAC_EWORKSPACE


def test_kron_cov_workspace_grows_with_nb():
    from bnn_kfac_amd import _native as N
    lib = N.lib()
    for nA, nG in ((785, 128), (20, 130)):
        arr = N.as_array(N.CovJob, [_valid_job(N, nA, nG)])
        sizes = [lib.kfac_kron_cov_workspace_bytes(arr, 1, nb, 10) for nb in (1, 2, 8, 64)]
        assert sizes == sorted(set(sizes))
        assert sizes[0] >= 10 * nA * nG * 4  # at least T for every row
    assert lib.kfac_kron_cov_workspace_bytes(arr, 0, 4, 10) == 0
