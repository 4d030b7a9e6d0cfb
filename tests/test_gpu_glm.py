"""GPU: the GLM predictive -- kfac_kron_cov (variance.kron_covariance) against fp64
T = K1^T M K2, cov = T T^T written here in numpy, and variance.glm_predictive end to
end against an fp64 CPU copy of the network with hand-built posterior-order Jacobians.

Kernel tolerance: rtol 1e-5, atol 1e-5 * max|ref| (a plain fp32 evaluation of the same
formula on these shapes errs by at most 1.7e-6 * max).  End to end: rtol 1e-4,
atol 1e-5 * max|want| per sample (the project's Jacobian check; fp32 vs fp64 of the
whole chain on BaseNet_750 differs by 1.6e-7 * max)."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

SHAPES = [(5, 3, 1, 1), (27, 6, 4, 3), (129, 10, 3, 10), (70, 65, 2, 5), (64, 64, 1, 32),
          (33, 31, 2, 32), (20, 130, 2, 3), (785, 128, 2, 10)]


def _ref_term(J, K1, K2):
    """fp64 T = K1^T M K2 per row, then T T^T per sample."""
    nb, nc = J.shape[:2]
    nA, nG = K1.shape[0], K2.shape[0]
    T = K1.T @ J.astype(np.float64).reshape(nb, nc, nA, nG) @ K2
    Tf = T.reshape(nb, nc, nA * nG)
    return Tf @ Tf.transpose(0, 2, 1)


@functools.lru_cache(maxsize=None)
def _case(nA, nG, nb, nc, lower=True, seed=0):
    """(J, K1, K2) fp32 numpy and the fp64 reference, computed once per shape."""
    rng = np.random.default_rng(seed + 1000 * nA + nG)
    scale = 0.1 if nA * nG > 50000 else 1.0
    K1 = (rng.standard_normal((nA, nA)) * scale).astype(np.float32)
    K2 = (rng.standard_normal((nG, nG)) * scale).astype(np.float32)
    if lower:
        K1, K2 = np.tril(K1), np.tril(K2)
    J = rng.standard_normal((nb, nc, nA * nG)).astype(np.float32)
    ref = _ref_term(J, K1.astype(np.float64), K2.astype(np.float64))
    for a in (J, K1, K2, ref):
        a.setflags(write=False)
    return J, K1, K2, ref


def _dev(dev, *arrays):
    return [torch.from_numpy(np.array(a)).to(dev) for a in arrays]  # (a copy: the cached case stays read-only)


def _check(got, ref):
    print("max err / max|ref| =", float(np.abs(got - ref).max() / np.abs(ref).max()))
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kron_covariance_matches_fp64(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance
    J, K1, K2, ref = _case(*shape)
    Jd, K1d, K2d = _dev(hip_device, J, K1, K2)
    got = kron_covariance([(Jd, K1d, K2d)], lower=True)
    assert got.shape == (shape[2], shape[3], shape[3]) and got.dtype == torch.float32
    _check(got.cpu().numpy(), ref)


@pytest.mark.parametrize("shape", [(27, 6, 4, 3), (70, 65, 2, 5)], ids=lambda s: "x".join(map(str, s)))
def test_kron_covariance_dense_factors(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance
    J, K1, K2, ref = _case(*shape, lower=False)
    assert np.abs(np.triu(K1, 1)).max() > 0
    Jd, K1d, K2d = _dev(hip_device, J, K1, K2)
    _check(kron_covariance([(Jd, K1d, K2d)], lower=False).cpu().numpy(), ref)


def test_nine_terms_fold_in_groups_of_eight(hip_device):
    from bnn_kfac_amd.variance import kron_covariance
    shapes = [(5, 3), (27, 6), (9, 10), (70, 65), (12, 4), (20, 130), (33, 31), (8, 8), (64, 64)]
    terms, ref = [], 0.0
    for nA, nG in shapes:
        J, K1, K2, r = _case(nA, nG, 3, 4)
        terms.append(tuple(_dev(hip_device, J, K1, K2)))
        ref = ref + r
    _check(kron_covariance(terms, lower=True).cpu().numpy(), ref)


def test_blocks_bitwise_symmetric_and_repeatable(hip_device):
    from bnn_kfac_amd.variance import kron_covariance
    for shape in ((27, 6, 4, 3), (33, 31, 2, 32), (20, 130, 2, 3)):
        terms = [tuple(_dev(hip_device, *_case(*shape)[:3]))]
        a = kron_covariance(terms)
        b = kron_covariance(terms)
        assert torch.equal(a, a.mT)
        assert bool((torch.diagonal(a, dim1=1, dim2=2) >= 0).all())
        assert torch.equal(a, b)


def test_strided_jacobian_rows(hip_device):
    from bnn_kfac_amd.variance import kron_covariance
    J, K1, K2, ref = _case(70, 65, 2, 5)
    Jd, K1d, K2d = _dev(hip_device, J, K1, K2)
    wide = torch.full((2, 5, 70 * 65 + 7), float("nan"), device=hip_device)
    wide[:, :, :70 * 65] = Jd
    Js = wide[:, :, :70 * 65]
    assert Js.stride(1) == 70 * 65 + 7
    got = kron_covariance([(Js, K1d, K2d)])
    _check(got.cpu().numpy(), ref)
    assert torch.equal(got, kron_covariance([(Jd, K1d, K2d)]))


def test_sample_chunks_do_not_change_a_bit(hip_device):
    from bnn_kfac_amd import _native as N
    from bnn_kfac_amd.variance import kron_covariance
    shapes = [(27, 6), (20, 130)]
    terms = [tuple(_dev(hip_device, *_case(nA, nG, 4, 3)[:3])) for nA, nG in shapes]
    jobs = [N.CovJob(1, nA * nG, nA, nG, 1, nA, 1, nG, 1, 1) for nA, nG in shapes]
    one, two = (N.kron_cov_workspace_bytes(jobs, n, 3) for n in (1, 2))
    assert one < two  # a budget of `one` forces chunks of one sample: four chunks
    whole = kron_covariance(terms)
    assert torch.equal(kron_covariance(terms, max_workspace_bytes=one), whole)
    with pytest.raises(ValueError):
        kron_covariance(terms, max_workspace_bytes=one - 1)


@pytest.mark.parametrize("shape", [(27, 6, 4, 3), (70, 65, 2, 5)], ids=lambda s: "x".join(map(str, s)))
def test_diagonal_matches_kron_quadform(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance, kron_quadform
    J, K1, K2, _ = _case(*shape)
    Jd, K1d, K2d = _dev(hip_device, J, K1, K2)
    cov = kron_covariance([(Jd, K1d, K2d)]).cpu().numpy()
    S1, S2 = _dev(hip_device, (K1.astype(np.float64) @ K1.T).astype(np.float32),
                  (K2.astype(np.float64) @ K2.T).astype(np.float32))
    for c in range(shape[3]):
        want = kron_quadform([(Jd[:, c], S1, S2)], lower=False, abs_sum=False).cpu().numpy()
        np.testing.assert_allclose(cov[:, c, c], want, rtol=1e-4, atol=1e-4 * np.abs(want).max())


def test_more_than_32_outputs_raise(hip_device):
    from bnn_kfac_amd.variance import kron_covariance
    J = torch.zeros(2, 33, 15, device=hip_device)
    K1, K2 = torch.eye(5, device=hip_device), torch.eye(3, device=hip_device)
    with pytest.raises(ValueError):
        kron_covariance([(J, K1, K2)])


# ------------------------------------------------------------------ end to end
def _fp64_glm(net64, layers64, factors, x):
    """Per-sample logit Jacobians by autograd on the fp64 CPU copy, M built by hand in
    the posterior's order, cov = sum_l (L_A^T M L_G)(L_A^T M L_G)^T."""
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


def _fit_and_predict(dev, net, make_x, loss_of, n_test, chunk):
    from bnn_kfac_amd.curvatures import KFAC
    from bnn_kfac_amd.variance import glm_predictive
    net64 = copy.deepcopy(net).double()  # (before KFAC hooks the modules)
    net = net.to(dev)
    kfac = KFAC(net)

    def step():
        xb = make_x(64)
        out = net(xb)
        net.zero_grad()
        loss_of(out).backward()
        kfac.update(64)

    for _ in range(3):
        step()
    kfac.invert(0.04, 200)
    x = make_x(n_test)
    logits, cov = glm_predictive(kfac, x, chunk=chunk)
    layers = [m for m in list(net.modules())[1:] if m in kfac.state]
    layers64 = [m for m in list(net64.modules())[1:] if isinstance(m, (nn.Linear, nn.Conv2d))]
    assert len(layers) == len(layers64)
    factors = [tuple(t.double().cpu().numpy() for t in kfac.inv_state[l]) for l in layers]
    want_logits, want_cov = _fp64_glm(net64, layers64, factors, x.cpu())
    with torch.no_grad():
        direct = net(x).cpu().numpy()
    # hooks intact: another forward/backward + update still moves the factors
    before = kfac.state[layers[0]][0].clone()
    step()
    torch.cuda.synchronize()
    assert not torch.equal(before, kfac.state[layers[0]][0])
    return logits.cpu().numpy(), cov.cpu().numpy(), want_logits, want_cov, direct


def _check_glm(res):
    logits, cov, want_logits, want_cov, direct = res
    assert cov.shape == want_cov.shape and logits.shape == want_logits.shape
    # rtol 1e-6 as stated; logits cross zero, so the same 1e-6 of the largest one is the floor
    np.testing.assert_allclose(logits, direct, rtol=1e-6, atol=1e-6 * np.abs(direct).max())
    np.testing.assert_allclose(logits, want_logits, rtol=1e-4, atol=1e-5 * np.abs(want_logits).max())
    for b in range(cov.shape[0]):
        print("sample", b, "max err / max|want| =",
              float(np.abs(cov[b] - want_cov[b]).max() / np.abs(want_cov[b]).max()))
        np.testing.assert_allclose(cov[b], want_cov[b], rtol=1e-4, atol=1e-5 * np.abs(want_cov[b]).max())


def _categorical_loss(out):
    y = torch.distributions.Categorical(logits=out.detach()).sample()
    return torch.nn.functional.cross_entropy(out, y)


@pytest.fixture(scope="module")
def basenet750_glm(hip_device):
    from models_for_tests import BaseNet750
    torch.manual_seed(0)
    return _fit_and_predict(hip_device, BaseNet750(),
                            lambda n: torch.rand(n, 1, 28, 28, device=hip_device),
                            _categorical_loss, n_test=5, chunk=2)


def test_glm_predictive_basenet750(basenet750_glm):
    assert basenet750_glm[1].shape == (5, 10, 10)
    _check_glm(basenet750_glm)


def test_glm_predictive_layer_without_bias(hip_device):
    torch.manual_seed(0)
    net = nn.Sequential(nn.Linear(12, 7, bias=False), nn.Tanh(), nn.Linear(7, 3))
    _check_glm(_fit_and_predict(hip_device, net, lambda n: torch.randn(n, 12, device=hip_device),
                                _categorical_loss, n_test=5, chunk=2))


def test_glm_predictive_regression_variance(hip_device):
    torch.manual_seed(0)
    net = nn.Sequential(nn.Linear(4, 8), nn.Tanh(), nn.Linear(8, 1))
    res = _fit_and_predict(hip_device, net, lambda n: torch.randn(n, 4, device=hip_device),
                           lambda out: ((out - torch.randn_like(out)) ** 2).mean(), n_test=6, chunk=4)
    assert res[1].shape == (6, 1, 1) and (res[1][:, 0, 0] > 0).all()
    _check_glm(res)


def test_probit_of_glm_predictive(hip_device, basenet750_glm):
    """Rows sum to 1, and the arg-max is that of the logits.  The probit approximation
    divides logit c by sqrt(1 + pi/8 cov[c, c]) > 0, which keeps signs but, with unequal
    variances, not the order of same-signed logits (the untrained BaseNet_750's top two
    logits are 0.1320 and 0.1295: their order is the variances' to decide).  So the
    arg-max is asserted where it is a law: a decisive classifier whose top logit is
    positive and whose other logits are negative."""
    from bnn_kfac_amd.variance import probit_predictive
    p = probit_predictive(torch.from_numpy(basenet750_glm[0]), torch.from_numpy(basenet750_glm[1]))
    torch.testing.assert_close(p.sum(dim=1), torch.ones(5), rtol=0, atol=1e-6)

    torch.manual_seed(0)
    net = nn.Sequential(nn.Linear(4, 3))
    with torch.no_grad():
        net[0].weight.copy_(4 * torch.eye(3, 4) - 2)
        net[0].bias.zero_()

    def make_x(n):  # class k: e_k plus a little noise -> logit k near +2, the others near -2
        return torch.eye(4, device=hip_device)[torch.arange(n) % 3] + 0.1 * torch.rand(n, 4, device=hip_device)

    res = _fit_and_predict(hip_device, net, make_x, _categorical_loss, n_test=6, chunk=4)
    _check_glm(res)
    logits, cov = torch.from_numpy(res[0]), torch.from_numpy(res[1])
    top = logits.argmax(dim=1)
    assert torch.equal(top, torch.arange(6) % 3)
    assert bool((logits.sort(dim=1).values[:, -2] < 0).all()) and bool((logits.max(dim=1).values > 0).all())
    p = probit_predictive(logits, cov)
    torch.testing.assert_close(p.sum(dim=1), torch.ones(6), rtol=0, atol=1e-6)
    assert torch.equal(p.argmax(dim=1), top)
    assert bool((p.max(dim=1).values < torch.softmax(logits, dim=1).max(dim=1).values).all())
