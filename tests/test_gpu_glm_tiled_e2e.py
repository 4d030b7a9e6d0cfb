"""GPU: variance.glm_predictive end to end on nets with more than 32 outputs (the class-tiled
route: kron_covariance_tiled / kron_covariance_outer_tiled) against an fp64 CPU recompute
built as test_gpu_glm.py builds it, the dense and factored routes against each other, the
dense route's bitwise tie to joint=True, sample chunks, probit_predictive on the result; and
a 10-output net that must still take the capped kernels.

End-to-end tolerance (test_gpu_glm.py): rtol 1e-4, atol 1e-5 * max|want| per sample; two fp32
evaluations of one quantity: rtol 1e-4, atol 1e-5 * max."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

N_TEST = 5


def _fp64_glm(net64, layers64, factors, x):
    """Per-sample logit Jacobians by autograd on the fp64 CPU copy, M built by hand in the
    posterior's order, cov = sum_l (L_A^T M L_G)(L_A^T M L_G)^T."""
    logits, covs = [], []
    for b in range(x.shape[0]):
        out = net64(x[b:b + 1].double())[0]
        nc = out.shape[0]
        cov = np.zeros((nc, nc))
        rows = [[None] * nc for _ in layers64]
        for c in range(nc):
            net64.zero_grad()
            out[c].backward(retain_graph=True)
            for li, layer in enumerate(layers64):
                dW = layer.weight.grad.numpy()
                nG = dW.shape[0]
                M = dW.reshape(nG, -1).T  # M[a][g] = dW[g][a]
                if layer.bias is not None:
                    M = np.concatenate([M, layer.bias.grad.numpy()[None, :]], axis=0)  # M[nA-1][g] = db[g]
                rows[li][c] = M.copy()
        for li, (LA, LG) in enumerate(factors):
            T = np.stack([(LA.T @ M @ LG).ravel() for M in rows[li]])
            cov += T @ T.T
        logits.append(out.detach().numpy())
        covs.append(cov)
    return np.stack(logits), np.stack(covs)


def _categorical_loss(out):
    y = torch.distributions.Categorical(logits=out.detach()).sample()
    return torch.nn.functional.cross_entropy(out, y)


def _fit(dev, net, make_x):
    from bnn_kfac_amd.curvatures import KFAC
    net64 = copy.deepcopy(net).double()  # (before KFAC hooks the modules)
    net = net.to(dev)
    kfac = KFAC(net)
    for _ in range(3):
        out = net(make_x(64))
        net.zero_grad()
        _categorical_loss(out).backward()
        kfac.update(64)
    kfac.invert(0.04, 200)
    return net, net64, kfac


NETS = {
    "mlp40": (lambda: nn.Sequential(nn.Linear(20, 16), nn.Tanh(), nn.Linear(16, 40)), (20,), 40),
    "mlp40_no_bias": (lambda: nn.Sequential(nn.Linear(20, 16, bias=False), nn.Tanh(),
                                            nn.Linear(16, 40, bias=False)), (20,), 40),
    "conv70": (lambda: nn.Sequential(nn.Conv2d(1, 4, 3), nn.ReLU(), nn.Flatten(), nn.Linear(4 * 6 * 6, 70)),
               (1, 8, 8), 70),
}


@pytest.fixture(scope="module")
def deterministic_convolutions():
    """(test_gpu_glm_factored's finding: torch's vmapped Conv2d weight gradient picks its
    MIOpen solver per call; the bitwise comparisons here are about this project's code, so
    they run in torch's deterministic mode.)"""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = before


@pytest.fixture(scope="module", params=list(NETS))
def fitted(request, hip_device, deterministic_convolutions):
    """One KFAC pass + invert per net; every glm_predictive result the tests compare and the
    fp64 reference, computed once."""
    from bnn_kfac_amd.variance import glm_predictive
    make, xshape, nc = NETS[request.param]
    torch.manual_seed(0)
    make_x = lambda n: torch.randn(n, *xshape, device=hip_device)  # noqa: E731
    net, net64, kfac = _fit(hip_device, make(), make_x)
    x = make_x(N_TEST)
    layers = [m for m in list(net.modules())[1:] if m in kfac.state]
    layers64 = [m for m in list(net64.modules())[1:] if isinstance(m, (nn.Linear, nn.Conv2d))]
    assert len(layers) == len(layers64) == 2
    factors = [tuple(t.double().cpu().numpy() for t in kfac.inv_state[l]) for l in layers]
    want_logits, want_cov = _fp64_glm(net64, layers64, factors, x.cpu())
    with torch.no_grad():
        direct = net(x)
    res = {"name": request.param, "nc": nc, "kfac": kfac, "x": x, "direct": direct.cpu().numpy(),
           "want": (want_logits, want_cov)}
    for route in ("dense", "factored"):
        res[route] = glm_predictive(kfac, x, chunk=2, jacobians=route)
        res[route + "_whole"] = glm_predictive(kfac, x, chunk=N_TEST + 3, jacobians=route)
    res["default"] = glm_predictive(kfac, x, chunk=2)
    res["joint"] = glm_predictive(kfac, x, chunk=2, jacobians="dense", joint=True)
    return res


@pytest.mark.parametrize("route", ["dense", "factored"])
def test_glm_predictive_matches_fp64(fitted, route):
    logits, cov = (t.cpu().numpy() for t in fitted[route])
    want_logits, want_cov = fitted["want"]
    nc = fitted["nc"]
    assert nc > 32 and logits.shape == (N_TEST, nc) and cov.shape == (N_TEST, nc, nc)
    assert cov.shape == want_cov.shape
    np.testing.assert_allclose(logits, fitted["direct"], rtol=1e-6, atol=1e-6 * np.abs(fitted["direct"]).max())
    np.testing.assert_allclose(logits, want_logits, rtol=1e-4, atol=1e-5 * np.abs(want_logits).max())
    for b in range(N_TEST):
        print(fitted["name"], route, "sample", b, "max err / max|want| =",
              float(np.abs(cov[b] - want_cov[b]).max() / np.abs(want_cov[b]).max()))
    for b in range(N_TEST):
        np.testing.assert_allclose(cov[b], want_cov[b], rtol=1e-4, atol=1e-5 * np.abs(want_cov[b]).max())


def test_blocks_symmetric_and_default_route_is_dense(fitted):
    for route in ("dense", "factored"):
        cov = fitted[route][1]
        assert torch.equal(cov, cov.mT)
        assert bool((torch.diagonal(cov, dim1=1, dim2=2) >= 0).all())
    assert torch.equal(fitted["default"][0], fitted["dense"][0])
    assert torch.equal(fitted["default"][1], fitted["dense"][1])


def test_dense_and_factored_routes_agree(fitted):
    dense, factored = fitted["dense"][1].cpu().numpy(), fitted["factored"][1].cpu().numpy()
    print(fitted["name"], "max diff / max =", float(np.abs(factored - dense).max() / np.abs(dense).max()))
    np.testing.assert_allclose(factored, dense, rtol=1e-4, atol=1e-5 * np.abs(dense).max())


def test_dense_route_is_the_joint_results_diagonal_blocks_bitwise(fitted):
    from bnn_kfac_amd.variance import marginal_blocks
    logits, cov = fitted["joint"]
    nc = fitted["nc"]
    assert cov.shape == (N_TEST, nc, N_TEST, nc)
    assert torch.equal(logits, fitted["dense"][0])
    marg = marginal_blocks(cov)
    print(fitted["name"], "max |tiled - joint diagonal| =", float((fitted["dense"][1] - marg).abs().max()))
    assert torch.equal(fitted["dense"][1], marg)


@pytest.mark.parametrize("route", ["dense", "factored"])
def test_sample_chunks_do_not_change_a_bit(fitted, route):
    (logits, cov), (logits_w, cov_w) = fitted[route], fitted[route + "_whole"]
    print(fitted["name"], route, "max |chunked - whole|: logits", float((logits - logits_w).abs().max()),
          "cov", float((cov - cov_w).abs().max()))
    assert torch.equal(logits, logits_w)
    assert torch.equal(cov, cov_w)


def test_probit_predictive_runs_on_the_result(fitted):
    from bnn_kfac_amd.variance import probit_predictive
    for route in ("dense", "factored"):
        logits, cov = (t.cpu() for t in fitted[route])
        p = probit_predictive(logits, cov)
        assert p.shape == (N_TEST, fitted["nc"]) and bool(torch.isfinite(p).all()) and bool((p >= 0).all())
        torch.testing.assert_close(p.sum(dim=1), torch.ones(N_TEST), rtol=0, atol=1e-6)


# ------------------------------------------------------------------ unchanged behaviour
def test_ten_outputs_still_take_the_capped_kernels(hip_device, monkeypatch):
    """A chunk with nc <= 32 goes through kron_covariance / kron_covariance_outer as before:
    glm_predictive's result is those calls' on the same Jacobians or captures, bitwise, and
    the tiled functions are never entered."""
    from bnn_kfac_amd import variance

    def never(*args, **kwargs):
        raise AssertionError("a 10-output chunk reached a class-tiled call")

    torch.manual_seed(0)
    make_x = lambda n: torch.randn(n, 12, device=hip_device)  # noqa: E731
    net, _, kfac = _fit(hip_device, nn.Sequential(nn.Linear(12, 7), nn.Tanh(), nn.Linear(7, 10)), make_x)
    x = make_x(4)
    layers = [m for m in list(net.modules())[1:] if m in kfac.state]
    inv = kfac.inv_state
    monkeypatch.setattr(variance, "kron_covariance_tiled", never)
    monkeypatch.setattr(variance, "kron_covariance_outer_tiled", never)
    logits, cov = variance.glm_predictive(kfac, x, chunk=2)
    flogits, fcov = variance.glm_predictive(kfac, x, chunk=2, jacobians="factored")
    assert cov.shape == (4, 10, 10)
    for c0 in range(0, 4, 2):
        f, Js = variance.output_jacobians(net, layers, x[c0:c0 + 2])
        want = variance.kron_covariance([(J, *inv[l]) for l, J in zip(layers, Js)], lower=True)
        assert torch.equal(logits[c0:c0 + 2], f) and torch.equal(cov[c0:c0 + 2], want)
        f, io = variance.layer_io_jacobians(net, layers, x[c0:c0 + 2])
        want = variance.kron_covariance_outer([(a, D, *inv[l]) for l, (a, D) in zip(layers, io)], lower=True)
        assert torch.equal(flogits[c0:c0 + 2], f) and torch.equal(fcov[c0:c0 + 2], want)
