"""GPU: the factored GLM predictive on conv nets, with the Conv2d rows formed on the device
(kfac_cov_conv_rows through variance.conv_jacobian_rows_device).

glm_predictive(jacobians="factored") per sample and with joint=True, and
glm_predictive_sweep(jacobians="factored"), on a BaseNet_750-shaped net and on a net whose
first conv has stride 2, padding 1 and no bias: against the fp64 CPU recompute at the
project's end-to-end tolerance (rtol 1e-4, atol 1e-5 * max, as test_gpu_glm_factored.py) and
against the dense route.  A counting wrapper shows which rows served each Conv2d layer at the
three call sites; a net with a dilation-2 conv takes the torch rows for that layer and still
matches.  Chunks of 2 and of 64 samples give the same bits: end to end on BaseNet_750, and on
both nets with one capture handed out in slices (torch's own backward is not batch-size
invariant on the stride-2 net; see test_chunks_of_one_capture_do_not_change_a_bit)."""
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

import glm_sweep_cases as C
from test_gpu_glm import _categorical_loss, _fp64_glm

pytestmark = pytest.mark.gpu

N_TEST = 3                # chunks of 2: a full one and a ragged one
NCHUNK = -(-N_TEST // 2)
GRID = [(0.04, 200.0), (1.0, 200.0), ([0.04, 0.08, 0.12], [200.0, 100.0, 50.0])]


def _stride2_net():
    return nn.Sequential(nn.Conv2d(2, 4, 3, stride=2, padding=1, bias=False), nn.ReLU(), nn.Conv2d(4, 3, 3),
                         nn.ReLU(), nn.Flatten(), nn.Linear(27, 5))


def _dilated_net():
    return nn.Sequential(nn.Conv2d(1, 3, 3, dilation=2), nn.ReLU(), nn.Conv2d(3, 4, 3, padding=1), nn.ReLU(),
                         nn.Flatten(), nn.Linear(100, 4))


def _nets():
    from models_for_tests import BaseNet750
    return {"basenet750": (BaseNet750, (1, 28, 28)), "stride2-nobias": (_stride2_net, (2, 9, 9))}


@pytest.fixture
def deterministic_convolutions():
    """torch's convolution backward picks its MIOpen solver per call and batch size; the
    bitwise comparisons here are about this project's code, so they run in torch's
    deterministic mode (as test_gpu_glm_factored.py)."""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = before


@pytest.fixture(scope="module")
def fitted(hip_device):
    """name -> fitted net, KFAC (inverted at (0.04, 200)), test inputs and the fp64 references,
    computed once: per-sample and joint covariance from the inverted factors, the sweep's from
    the factors themselves."""
    cache = {}

    def get(name):
        if name not in cache:
            make, shape = _nets()[name]
            torch.manual_seed(0)
            net, net64, kfac = C.fit(hip_device, make(), lambda n: torch.rand(n, *shape, device=hip_device),
                                     _categorical_loss)
            kfac.invert(0.04, 200)
            x = torch.rand(N_TEST, *shape, device=hip_device)
            layers = [m for m in list(net.modules())[1:] if m in kfac.state]
            layers64 = [m for m in list(net64.modules())[1:] if isinstance(m, (nn.Linear, nn.Conv2d))]
            assert len(layers) == len(layers64) == 3
            inv64 = [tuple(t.double().cpu().numpy() for t in kfac.inv_state[l]) for l in layers]
            logits64, cov64 = _fp64_glm(net64, layers64, inv64, x.cpu())
            _, rows = C.fp64_rows(net64, layers64, x.cpu())
            joint64 = 0.0
            for M, (LA, LG) in zip(rows, inv64):
                T = np.einsum("ai,bcag,gh->bcih", LA, M, LG).reshape(M.shape[0] * M.shape[1], -1)
                joint64 = joint64 + T @ T.T
            state64 = [tuple(F_.double().cpu().numpy() for F_ in kfac.state[l]) for l in layers]
            sweep64 = [C.fp64_cov(rows, state64, [C.point_of(p, i) for i in range(3)]) for p in GRID]
            cache[name] = types.SimpleNamespace(net=net, kfac=kfac, x=x, layers=layers, logits64=logits64,
                                                cov64=cov64, joint64=joint64, sweep64=sweep64)
        return cache[name]

    return get


def _close(what, got, want):
    """The project's end-to-end tolerance; the worst |err| / max|want| printed first."""
    print(what, "max err / max|want| =", float(np.abs(got - want).max() / np.abs(want).max()))
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5 * np.abs(want).max())


@pytest.fixture
def counted(monkeypatch):
    """Counts the calls of the two row builders at the route's call sites."""
    from bnn_kfac_amd import variance as V
    calls = {"device": [], "torch": []}
    device, host = V.conv_jacobian_rows_device, V.conv_jacobian_rows

    def on_device(layer, a, D):
        calls["device"].append(layer)
        return device(layer, a, D)

    def on_host(layer, a, D):
        calls["torch"].append(layer)
        return host(layer, a, D)

    monkeypatch.setattr(V, "conv_jacobian_rows_device", on_device)
    monkeypatch.setattr(V, "conv_jacobian_rows", on_host)
    return calls


def _convs(layers):
    return [l for l in layers if isinstance(l, nn.Conv2d)]


@pytest.mark.parametrize("name", ["basenet750", "stride2-nobias"])
def test_per_sample_factored(hip_device, fitted, counted, name):
    from bnn_kfac_amd.variance import glm_predictive
    f = fitted(name)
    logits, cov = glm_predictive(f.kfac, f.x, chunk=2, jacobians="factored")
    # every chunk: both conv layers on the device, none from torch
    assert counted["device"] == _convs(f.layers) * NCHUNK and counted["torch"] == []
    nc = f.logits64.shape[1]
    assert logits.shape == (N_TEST, nc) and cov.shape == (N_TEST, nc, nc) and cov.dtype == torch.float32
    assert torch.equal(cov, cov.mT)
    _close(f"{name} logits", logits.cpu().numpy(), f.logits64)
    for b in range(N_TEST):
        _close(f"{name} per-sample, sample {b}, against fp64:", cov[b].cpu().numpy(), f.cov64[b])
    dense = glm_predictive(f.kfac, f.x, chunk=2, jacobians="dense")[1]
    assert len(counted["device"]) == 2 * NCHUNK  # (the dense route forms no rows here)
    for b in range(N_TEST):
        _close(f"{name} per-sample, sample {b}, against the dense route:", cov[b].cpu().numpy(),
               dense[b].cpu().numpy())


@pytest.mark.parametrize("name", ["basenet750", "stride2-nobias"])
def test_joint_factored(hip_device, fitted, counted, name):
    from bnn_kfac_amd.variance import glm_predictive, marginal_blocks
    f = fitted(name)
    logits, cov = glm_predictive(f.kfac, f.x, chunk=2, jacobians="factored", joint=True)
    assert counted["device"] == _convs(f.layers) * NCHUNK and counted["torch"] == []
    nc = f.logits64.shape[1]
    R = N_TEST * nc
    assert cov.shape == (N_TEST, nc, N_TEST, nc)
    flat = cov.reshape(R, R)
    assert torch.equal(flat, flat.T)
    _close(f"{name} joint against fp64:", flat.cpu().numpy(), f.joint64)
    dense = glm_predictive(f.kfac, f.x, chunk=2, jacobians="dense", joint=True)[1]
    _close(f"{name} joint against the dense route:", flat.cpu().numpy(), dense.reshape(R, R).cpu().numpy())
    blocks = marginal_blocks(cov).cpu().numpy()
    for b in range(N_TEST):
        _close(f"{name} joint diagonal block {b} against fp64:", blocks[b], f.cov64[b])


@pytest.mark.parametrize("name", ["basenet750", "stride2-nobias"])
def test_sweep_factored(hip_device, fitted, counted, name):
    from bnn_kfac_amd.variance import glm_predictive_sweep
    f = fitted(name)
    logits, cov = glm_predictive_sweep(f.kfac, f.x, GRID, chunk=2, jacobians="factored")
    assert counted["device"] == _convs(f.layers) * NCHUNK and counted["torch"] == []
    nc = f.logits64.shape[1]
    assert cov.shape == (len(GRID), N_TEST, nc, nc)
    dense = glm_predictive_sweep(f.kfac, f.x, GRID, chunk=2, jacobians="dense")[1]
    for t, point in enumerate(GRID):
        for b in range(N_TEST):
            _close(f"{name} sweep {point}, sample {b}, against fp64:", cov[t, b].cpu().numpy(), f.sweep64[t][b])
            _close(f"{name} sweep {point}, sample {b}, against the dense route:", cov[t, b].cpu().numpy(),
                   dense[t, b].cpu().numpy())


def _both_chunkings(f):
    from bnn_kfac_amd.variance import glm_predictive, glm_predictive_sweep
    for chunk in (2, 64):
        yield (glm_predictive(f.kfac, f.x, chunk=chunk, jacobians="factored"),
               glm_predictive_sweep(f.kfac, f.x, GRID, chunk=chunk, jacobians="factored"))


def test_chunks_do_not_change_a_bit(hip_device, fitted, deterministic_convolutions):
    """chunk=2 against chunk=64, end to end, on BaseNet_750."""
    (small, small_sweep), (large, large_sweep) = _both_chunkings(fitted("basenet750"))
    assert torch.equal(small[0], large[0]) and torch.equal(small[1], large[1])
    assert torch.equal(small_sweep[0], large_sweep[0]) and torch.equal(small_sweep[1], large_sweep[1])


@pytest.mark.parametrize("name", ["basenet750", "stride2-nobias"])
def test_chunks_of_one_capture_do_not_change_a_bit(hip_device, fitted, monkeypatch, name):
    """The same with the captures taken once and handed out in slices, so that everything
    after torch's backward is compared: the device rows on batch views, the covariance calls,
    the concatenation.  (End to end the stride-2 net does not repeat: torch's backward-data of
    its second conv gives the first conv's D differing by 1.3e-7 of its maximum between a batch
    of 2 and a batch of 5, in deterministic mode too; on equal captures the rows are equal.)"""
    from bnn_kfac_amd import variance as V
    f = fitted(name)
    logits, io = V.layer_io_jacobians(f.net, f.layers, f.x)
    served = []

    def slices(model, layers, xc):
        b0 = (xc.data_ptr() - f.x.data_ptr()) // (f.x.element_size() * f.x[0].numel())
        n = xc.shape[0]
        assert torch.equal(xc, f.x[b0:b0 + n])
        served.append((b0, n))
        return logits[b0:b0 + n], [(a[b0:b0 + n], D[b0:b0 + n]) for a, D in io]

    monkeypatch.setattr(V, "layer_io_jacobians", slices)
    (small, small_sweep), (large, large_sweep) = _both_chunkings(f)
    chunks = [(b0, min(2, N_TEST - b0)) for b0 in range(0, N_TEST, 2)]
    assert served == chunks * 2 + [(0, N_TEST)] * 2
    assert torch.equal(small[0], large[0]) and torch.equal(small[1], large[1])
    assert torch.equal(small_sweep[0], large_sweep[0]) and torch.equal(small_sweep[1], large_sweep[1])


# ------------------------------------------------------------------ an uncovered layer
def _lower(gen, n, dev):
    L = torch.tril(torch.randn(n, n, generator=gen) / n ** 0.5)
    L.diagonal().abs_().add_(0.5)
    return L.to(dev)


def _orthogonal(gen, n, dev):
    return torch.linalg.qr(torch.randn(n, n, generator=gen))[0].contiguous().to(dev)


@pytest.fixture(scope="module")
def dilated(hip_device):
    """A net whose first conv has dilation 2, with hand-made posterior factors (KFAC's factor
    pass is not what is tested here): an object with the attributes the predictive reads."""
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(1)
    net = _dilated_net()
    net64 = _dilated_net().double()
    net64.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
    net = net.to(hip_device)
    layers = [net[0], net[2], net[5]]
    sizes = [(10, 3), (28, 4), (101, 4)]
    inv = {l: (_lower(gen, nA, hip_device), _lower(gen, nG, hip_device)) for l, (nA, nG) in zip(layers, sizes)}
    eig = {l: ((torch.rand(nA, generator=gen).double().add(0.1).to(hip_device), _orthogonal(gen, nA, hip_device)),
               (torch.rand(nG, generator=gen).double().add(0.1).to(hip_device), _orthogonal(gen, nG, hip_device)))
           for l, (nA, nG) in zip(layers, sizes)}
    kfac = types.SimpleNamespace(model=net, state={l: None for l in layers}, inv_state=inv, eig_state=eig)
    x = torch.rand(N_TEST, 1, 9, 9, generator=gen).to(hip_device)
    layers64 = [net64[0], net64[2], net64[5]]
    inv64 = [tuple(t.double().cpu().numpy() for t in inv[l]) for l in layers]
    logits64, cov64 = _fp64_glm(net64, layers64, inv64, x.cpu())
    return types.SimpleNamespace(net=net, kfac=kfac, x=x, layers=layers, logits64=logits64, cov64=cov64)


def test_dilated_conv_takes_the_torch_rows(hip_device, dilated, counted):
    from bnn_kfac_amd.variance import glm_predictive, glm_predictive_sweep
    f = dilated
    conv1, conv2 = f.layers[0], f.layers[1]
    logits, cov = glm_predictive(f.kfac, f.x, chunk=2, jacobians="factored")
    assert counted["torch"] == [conv1] * NCHUNK and counted["device"] == [conv2] * NCHUNK
    _close("dilated logits", logits.cpu().numpy(), f.logits64)
    for b in range(N_TEST):
        _close(f"dilated per-sample, sample {b}, against fp64:", cov[b].cpu().numpy(), f.cov64[b])
    dense = glm_predictive(f.kfac, f.x, chunk=2, jacobians="dense")[1]
    _close("dilated per-sample against the dense route:", cov.cpu().numpy(), dense.cpu().numpy())
    joint = glm_predictive(f.kfac, f.x, chunk=2, jacobians="factored", joint=True)[1]
    assert counted["torch"] == [conv1] * (2 * NCHUNK) and counted["device"] == [conv2] * (2 * NCHUNK)
    dense = glm_predictive(f.kfac, f.x, chunk=2, jacobians="dense", joint=True)[1]
    _close("dilated joint against the dense route:", joint.cpu().numpy(), dense.cpu().numpy())
    grid = GRID[:2]
    sweep = glm_predictive_sweep(f.kfac, f.x, grid, chunk=2, jacobians="factored")[1]
    assert counted["torch"] == [conv1] * (3 * NCHUNK) and counted["device"] == [conv2] * (3 * NCHUNK)
    dense = glm_predictive_sweep(f.kfac, f.x, grid, chunk=2, jacobians="dense")[1]
    for t in range(len(grid)):
        _close(f"dilated sweep {grid[t]} against the dense route:", sweep[t].cpu().numpy(), dense[t].cpu().numpy())
