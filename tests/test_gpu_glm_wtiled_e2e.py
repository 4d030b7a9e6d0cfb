"""GPU: variance.glm_predictive_efb, glm_predictive_efb_sweep and glm_predictive_sweep end to end
on nets with 40 outputs (the class-tiled weighted route: kron_covariance_*_tiled), both
`jacobians` routes, chunk = 2, against the fp64 CPU recompute of the existing end-to-end tests
(glm_sweep_cases.fp64_rows / fp64_cov, the EFB formula of test_gpu_glm_full.py), and against
invert + the single-damping call.  Every factor edge is <= 128 (the Jacobi eigensolver).

End to end: 1e-4 * max|cov[b]| per sample; the sweep slice against invert + glm_predictive_efb:
2e-5; the KFAC sweep slice against invert + glm_predictive (class-tiled itself): 1e-4."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

import glm_sweep_cases as S
from test_gpu_glm_full import _per_sample

pytestmark = pytest.mark.gpu

N_TEST = 5
NC = 40
GRID = [(1e-3, 200.0), (0.04, 200.0), (1.0, 1.0)]
NETS = {"mlp40": (lambda: nn.Sequential(nn.Linear(20, 24), nn.Tanh(), nn.Linear(24, NC)), (20,)),
        "conv40": (lambda: nn.Sequential(nn.Conv2d(1, 3, 3), nn.ReLU(), nn.Flatten(), nn.Linear(3 * 6 * 6, NC)),
                   (1, 8, 8))}


@pytest.fixture
def deterministic_convolutions():
    """(test_gpu_glm_factored.py: torch's vmapped Conv2d weight gradient picks its MIOpen solver
    per call; comparisons of two dense-route calls run in torch's deterministic mode.)"""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = before


def _fit(dev, net, in_shape):
    """test_gpu_glm_full._fit_efb's procedure, keeping the KFAC object: KFAC factors from two
    batches, then EFB on their eigenbases from three."""
    from bnn_kfac_amd.curvatures import EFB, KFAC
    net64 = copy.deepcopy(net).double()  # (before KFAC hooks the modules)
    net = net.to(dev)
    kfac = KFAC(net)

    def backward():
        x = torch.rand(32, *in_shape, device=dev)
        net.zero_grad()
        nn.functional.cross_entropy(net(x), torch.randint(0, NC, (32,), device=dev)).backward()

    for _ in range(2):
        backward()
        kfac.update(batch_size=32)
    factors = {m: [F.clone() for F in v] for m, v in kfac.state.items()}
    efb = EFB(net, factors)
    for _ in range(3):
        backward()
        efb.update(batch_size=32)
    return net, net64, kfac, efb


def _sandwich(M, A, G):
    """A^T M G for every row M (n, nc, nA, nG), one matrix product per side."""
    return np.einsum("bcig,gh->bcih", np.einsum("ai,bcag->bcig", A, M), G)


def _fp64_cov(rows, factors64, points):
    """glm_sweep_cases.fp64_cov's formula, contracted side by side: its single four-operand
    einsum visits nc^2 nA^2 nG^2 terms per sample, minutes at 40 outputs."""
    cov = 0.0
    for M, (A, G), (n, s) in zip(rows, factors64, points):
        SA = np.linalg.inv(np.sqrt(s) * A + np.sqrt(n) * np.eye(A.shape[0]))
        SG = np.linalg.inv(np.sqrt(s) * G + np.sqrt(n) * np.eye(G.shape[0]))
        cov = cov + np.einsum("bcag,bdag->bcd", M, _sandwich(M, SA, SG))
    return cov


@pytest.fixture(scope="module", params=list(NETS))
def fitted(request, hip_device):
    make, in_shape = NETS[request.param]
    torch.manual_seed(0)
    net, net64, kfac, efb = _fit(hip_device, make(), in_shape)
    x = torch.rand(N_TEST, *in_shape, device=hip_device)
    layers = [m for m in list(net.modules())[1:] if m in kfac.state]
    layers64 = [m for m in list(net64.modules())[1:] if isinstance(m, (nn.Linear, nn.Conv2d))]
    assert len(layers) == len(layers64) == 2
    for layer in layers:
        assert all(F.shape[0] <= 128 for F in kfac.state[layer])
    logits64, rows = S.fp64_rows(net64, layers64, x.cpu())
    bases = [tuple(v.double().cpu().numpy() for v in efb.eigvecs[layer]) for layer in layers]
    Ys = [_sandwich(M, VA, VG) for M, (VA, VG) in zip(rows, bases)]            # once for the grid
    want_efb = []
    for n, s in GRID:
        cov = 0.0
        for layer, Y in zip(layers, Ys):
            Wl = 1.0 / (s * efb.state[layer].double().cpu().numpy().T + n)   # (nA, nG)
            cov = cov + np.einsum("ih,bcih,bdih->bcd", Wl, Y, Y)
        want_efb.append(cov)
    grid = S.grid_for(len(layers))
    factors64 = [tuple(F.double().cpu().numpy() for F in kfac.state[layer]) for layer in layers]
    want_kfac = [_fp64_cov(rows, factors64, [S.point_of(p, i) for i in range(len(layers))]) for p in grid]
    # the staged contraction is glm_sweep_cases.fp64_cov: one sample, two outputs
    points = [S.point_of(grid[0], i) for i in range(len(layers))]
    np.testing.assert_allclose(want_kfac[0][:1, :2, :2], S.fp64_cov([M[:1, :2] for M in rows], factors64, points),
                               rtol=1e-10)
    return dict(name=request.param, net=net, kfac=kfac, efb=efb, x=x, logits64=logits64, want_efb=want_efb,
                grid=grid, want_kfac=want_kfac)


def _logits_ok(fitted, logits):
    with torch.no_grad():
        direct = fitted["net"](fitted["x"]).cpu().numpy()
    assert logits.shape == (N_TEST, NC)
    np.testing.assert_allclose(logits.cpu().numpy(), direct, rtol=1e-6, atol=1e-6 * np.abs(direct).max())
    np.testing.assert_allclose(logits.cpu().numpy(), fitted["logits64"], rtol=1e-4,
                               atol=1e-5 * np.abs(fitted["logits64"]).max())


@pytest.mark.parametrize("route", ["dense", "factored"])
def test_glm_predictive_efb_above_32_outputs(fitted, deterministic_convolutions, route):
    from bnn_kfac_amd.variance import glm_predictive_efb, glm_predictive_efb_sweep
    efb, x, want, name = fitted["efb"], fitted["x"], fitted["want_efb"], fitted["name"]
    sweep = glm_predictive_efb_sweep(efb, x, GRID, chunk=2, jacobians=route)      # needs no invert
    efb.invert(0.04, 200.0)
    logits, cov = glm_predictive_efb(efb, x, chunk=2, jacobians=route)
    assert cov.shape == (N_TEST, NC, NC) and cov.dtype == torch.float32
    assert sweep.shape == (len(GRID), N_TEST, NC, NC) and sweep.dtype == torch.float32
    _logits_ok(fitted, logits)
    _per_sample(cov.cpu().numpy(), want[1], 1e-4, f"{name} {route} glm_predictive_efb against fp64:")
    for t, point in enumerate(GRID):
        _per_sample(sweep[t].cpu().numpy(), want[t], 1e-4, f"{name} {route} sweep {point} against fp64:")
    _per_sample(sweep[1].cpu().numpy(), cov.cpu().numpy(), 2e-5,
                f"{name} {route} sweep against invert + glm_predictive_efb:")
    assert torch.equal(cov, cov.mT) and torch.equal(sweep, sweep.mT)


@pytest.mark.parametrize("route", ["dense", "factored"])
def test_glm_predictive_sweep_above_32_outputs(fitted, deterministic_convolutions, route):
    from bnn_kfac_amd.variance import glm_predictive, glm_predictive_sweep
    kfac, x, want, grid, name = fitted["kfac"], fitted["x"], fitted["want_kfac"], fitted["grid"], fitted["name"]
    logits, cov = glm_predictive_sweep(kfac, x, grid, chunk=2, jacobians=route)
    assert cov.shape == (len(grid), N_TEST, NC, NC) and cov.dtype == torch.float32
    _logits_ok(fitted, logits)
    assert torch.equal(cov, cov.mT)
    for t, point in enumerate(grid):
        _per_sample(cov[t].cpu().numpy(), want[t], 1e-4, f"{name} {route} {point} against fp64:")
        kfac.invert(*point)                           # the existing path, class-tiled itself
        _, old = glm_predictive(kfac, x, chunk=2, jacobians=route)
        _per_sample(cov[t].cpu().numpy(), old.cpu().numpy(), 1e-4,
                    f"{name} {route} {point} against invert + glm_predictive:")
