"""Test double for kfac_inf_cov / kfac_inf_cov_outer (and the two device calls
inf_covariance_factors makes) so the HOST logic of the INF GLM predictive -- job descriptors,
strides, chunking, folding, the wiring of Linear and Conv2d layers -- can be tested on a
CPU-only machine.  It reads the same ctypes job descriptors the C ABI receives and applies the
header's formula in numpy fp64 to the host memory they point at.  Never used by the product
path."""
import numpy as np

from host_double import _view, fake_invert

CALLS = []  # per fake call: (name, njobs, nb, accumulate)


def _matrix(ptr, rows, cols, ld):
    assert ld >= cols
    return np.stack([_view(ptr + 4 * r * ld, cols) for r in range(rows)]).astype(np.float64)


def _operands(j, nA):
    r = j.ra * j.rg
    UA = _matrix(j.UA, nA, j.ra, j.ldA).reshape(nA, j.ra)
    UG = _matrix(j.UG, j.nG, j.rg, j.ldG).reshape(j.nG, j.rg)
    assert j.ldW >= nA * j.nG and j.ldF >= r
    W = _view(j.W, nA * j.nG).astype(np.float64).reshape(nA, j.nG)
    F = _matrix(j.F, r, r, j.ldF).reshape(r, r)
    return UA, UG, W, F


def _block(M, UA, UG, W, F):
    """M (nb, nc, nA, nG) fp64 -> (nb, nc, nc)."""
    nb, nc = M.shape[:2]
    t = np.einsum("ip,bcig,gq->bcpq", UA, M * W, UG).reshape(nb, nc, -1)
    y = t @ F.T
    return np.einsum("ig,bcig,bdig->bcd", W, M, M) - np.einsum("bcr,bdr->bcd", y, y)


def _finish(out, total, accumulate):
    res = total + (out.numpy().astype(np.float64) if accumulate else 0.0)
    out.copy_(out.new_tensor(res.astype(np.float32)))


def fake_inf_cov(jobs, nb, nc, out, accumulate=False):
    assert 0 < len(jobs) <= 8 and tuple(out.shape) == (nb, nc, nc)
    CALLS.append(("inf_cov", len(jobs), nb, bool(accumulate)))
    total = 0.0
    for j in jobs:
        J = _matrix(j.J, nb * nc, j.nA * j.nG, j.ldJ).reshape(nb, nc, j.nA, j.nG)
        total = total + _block(J, *_operands(j, j.nA))
    _finish(out, total, accumulate)


def fake_inf_cov_outer(jobs, nb, nc, out, accumulate=False):
    assert 0 < len(jobs) <= 8 and tuple(out.shape) == (nb, nc, nc)
    CALLS.append(("inf_cov_outer", len(jobs), nb, bool(accumulate)))
    total = 0.0
    for j in jobs:
        nA = j.cols + j.has_ones
        a = _matrix(j.a, nb, j.cols, j.lda).reshape(nb, j.cols)
        abar = np.concatenate([a, np.ones((nb, 1))], axis=1) if j.has_ones else a
        D = _matrix(j.D, nb * nc, j.nG, j.ldD).reshape(nb, nc, j.nG)
        total = total + _block(np.einsum("bi,bcg->bcig", abar, D), *_operands(j, nA))
    _finish(out, total, accumulate)


def fake_workspace_bytes(jobs, nb, nc):
    """Linear in nb, as the device's answer nearly is: 1024 bytes per job and sample."""
    return 1024 * len(jobs) * nb


def fake_kron_gram(UA, UG, c, sigma):
    """kfac_kron_gram: diag(sigma) V^T V diag(sigma), V = c * kron(UA, UG), fp64 inside."""
    U = np.kron(UA.double().numpy(), UG.double().numpy()) * c.double().numpy().reshape(-1, 1)
    s = sigma.double().numpy()
    return UA.new_tensor((s[:, None] * (U.T @ U) * s[None, :]).astype(np.float32))


def install(monkeypatch):
    from bnn_kfac_amd import _native as N
    from bnn_kfac_amd import variance
    CALLS.clear()
    monkeypatch.setattr(N, "require_device", lambda t, what, owner=None: None)
    monkeypatch.setattr(N, "inf_cov", fake_inf_cov)
    monkeypatch.setattr(N, "inf_cov_outer", fake_inf_cov_outer)
    monkeypatch.setattr(N, "inf_cov_workspace_bytes", fake_workspace_bytes)
    monkeypatch.setattr(N, "inf_cov_outer_workspace_bytes", fake_workspace_bytes)
    monkeypatch.setattr(N, "kron_gram", fake_kron_gram)
    monkeypatch.setattr(N, "invert", fake_invert)
    # (Conv2d rows from torch: the device kernel that forms them is not under test here)
    monkeypatch.setattr(variance, "_conv_rows", variance.conv_jacobian_rows)
