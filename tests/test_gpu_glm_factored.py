"""GPU: the factored GLM predictive -- kfac_kron_cov_outer (variance.kron_covariance_outer)
against fp64 s = ||K1^T abar||^2, V = Delta K2, cov = s V V^T written here in numpy,
against the dense kernel on hand-built outer-product rows, and
variance.glm_predictive(jacobians="factored") end to end against the fp64 CPU recompute
of test_gpu_glm.

Kernel tolerance: the dense kernel's, rtol 1e-5, atol 1e-5 * max|ref| (a plain fp32 numpy
evaluation of the same formula is within 4.6e-7 * max on all eight shapes).  Against the
dense kernel and end to end: rtol 1e-4, atol 1e-5 * max (two fp32 evaluations of one
quantity: the project's end-to-end tolerance)."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

from test_gpu_glm import _categorical_loss, _fp64_glm

pytestmark = pytest.mark.gpu

# (cols, has_ones, nG, nb, nc)
SHAPES = [(4, 1, 3, 1, 1),
          (63, 1, 10, 3, 10),      # nA = 64: the ones column ends a tile
          (64, 1, 10, 5, 3),       # nA = 65: the ones column alone in the second tile
          (128, 0, 65, 2, 5),
          (130, 1, 130, 70, 2),    # nb crosses a sample tile
          (20, 1, 31, 2, 32),      # nc at its cap
          (784, 1, 128, 64, 10),
          (4096, 1, 4096, 8, 10)]  # C5's layer: the dense route cannot run it
IDS = lambda s: "x".join(map(str, s))  # noqa: E731


def _ref_term(a, ones, D, K1, K2):
    abar = np.concatenate([a, np.ones((a.shape[0], 1))], axis=1) if ones else a
    s = ((abar @ K1) ** 2).sum(axis=1)
    V = D @ K2
    return s[:, None, None] * (V @ V.transpose(0, 2, 1))


@functools.lru_cache(maxsize=None)
def _case(cols, ones, nG, nb, nc, lower=True, seed=0):
    """(a, D, K1, K2) fp32 numpy and the fp64 reference, computed once per shape."""
    rng = np.random.default_rng(seed + 1000 * cols + nG)
    nA = cols + ones
    K1 = (rng.standard_normal((nA, nA)) / np.sqrt(nA)).astype(np.float32)
    K2 = (rng.standard_normal((nG, nG)) / np.sqrt(nG)).astype(np.float32)
    if lower:
        K1, K2 = np.tril(K1), np.tril(K2)
    a = rng.standard_normal((nb, cols)).astype(np.float32)
    D = rng.standard_normal((nb, nc, nG)).astype(np.float32)
    ref = _ref_term(a.astype(np.float64), ones, D.astype(np.float64), K1.astype(np.float64),
                    K2.astype(np.float64))
    for t in (a, D, K1, K2, ref):
        t.setflags(write=False)
    return a, D, K1, K2, ref


def _dev(dev, *arrays):
    return [torch.from_numpy(np.array(t)).to(dev) for t in arrays]  # (a copy: the cached case stays read-only)


def _check(got, ref):
    print("max err / max|ref| =", float(np.abs(got - ref).max() / np.abs(ref).max()))
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_kron_covariance_outer_matches_fp64(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance_outer
    a, D, K1, K2, ref = _case(*shape)
    got = kron_covariance_outer([tuple(_dev(hip_device, a, D, K1, K2))], lower=True)
    assert got.shape == (shape[3], shape[4], shape[4]) and got.dtype == torch.float32
    _check(got.cpu().numpy(), ref)


@pytest.mark.parametrize("shape", [(63, 1, 10, 3, 10), (128, 0, 65, 2, 5)], ids=IDS)
def test_dense_factors(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance_outer
    a, D, K1, K2, ref = _case(*shape, lower=False)
    assert np.abs(np.triu(K1, 1)).max() > 0 and np.abs(np.triu(K2, 1)).max() > 0
    _check(kron_covariance_outer([tuple(_dev(hip_device, a, D, K1, K2))], lower=False).cpu().numpy(), ref)


def test_strided_inputs(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_outer
    cols, ones, nG, nb, nc = shape = (130, 1, 130, 70, 2)
    a, D, K1, K2, ref = _case(*shape)
    ad, Dd, K1d, K2d = _dev(hip_device, a, D, K1, K2)
    wide_a = torch.full((nb, cols + 7), float("nan"), device=hip_device)
    wide_a[:, :cols] = ad
    wide_D = torch.full((nb, nc, nG + 5), float("nan"), device=hip_device)
    wide_D[:, :, :nG] = Dd
    a_s, D_s = wide_a[:, :cols], wide_D[:, :, :nG]
    assert a_s.stride(0) == cols + 7 and D_s.stride(1) == nG + 5
    plain = kron_covariance_outer([(ad, Dd, K1d, K2d)])
    _check(plain.cpu().numpy(), ref)
    assert torch.equal(kron_covariance_outer([(a_s, Dd, K1d, K2d)]), plain)
    assert torch.equal(kron_covariance_outer([(ad, D_s, K1d, K2d)]), plain)
    assert torch.equal(kron_covariance_outer([(a_s, D_s, K1d, K2d)]), plain)


def test_blocks_bitwise_symmetric_and_repeatable(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_outer
    for shape in ((63, 1, 10, 3, 10), (20, 1, 31, 2, 32), (130, 1, 130, 70, 2)):
        terms = [tuple(_dev(hip_device, *_case(*shape)[:4]))]
        one = kron_covariance_outer(terms)
        two = kron_covariance_outer(terms)
        assert torch.equal(one, one.mT)
        assert bool((torch.diagonal(one, dim1=1, dim2=2) >= 0).all())
        assert torch.equal(one, two)


def test_sample_chunks_do_not_change_a_bit(hip_device):
    from bnn_kfac_amd import _native as N
    from bnn_kfac_amd.variance import kron_covariance_outer
    shapes = [(128, 0, 65), (130, 1, 130)]
    terms = [tuple(_dev(hip_device, *_case(c, o, g, 4, 5)[:4])) for c, o, g in shapes]
    jobs = [N.CovOuterJob(1, c, c, o, 1, g, g, 0, 1, c + o, 1, g, 1, 1) for c, o, g in shapes]
    one, two = (N.kron_cov_outer_workspace_bytes(jobs, n, 5) for n in (1, 2))
    assert 0 < one < two  # a budget of `one` forces chunks of one sample: four chunks
    whole = kron_covariance_outer(terms)
    assert torch.equal(kron_covariance_outer(terms, max_workspace_bytes=one), whole)
    with pytest.raises(ValueError):
        kron_covariance_outer(terms, max_workspace_bytes=one - 1)


def test_nine_terms_fold_in_groups_of_eight(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_outer
    shapes = [(4, 1, 3), (63, 1, 10), (9, 0, 10), (70, 1, 65), (12, 1, 4), (20, 1, 130), (33, 0, 31),
              (8, 1, 8), (64, 1, 64)]
    terms, ref = [], 0.0
    for cols, ones, nG in shapes:
        *arrays, r = _case(cols, ones, nG, 3, 4)
        terms.append(tuple(_dev(hip_device, *arrays)))
        ref = ref + r
    _check(kron_covariance_outer(terms, lower=True).cpu().numpy(), ref)


@pytest.mark.parametrize("shape", [(63, 1, 10, 3, 10), (130, 1, 130, 2, 5)], ids=IDS)
def test_agrees_with_dense_kernel(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance, kron_covariance_outer
    a, D, K1, K2, _ = _case(*shape)
    ad, Dd, K1d, K2d = _dev(hip_device, a, D, K1, K2)
    nb, nc = shape[3], shape[4]
    abar = torch.cat([ad, torch.ones(nb, 1, device=hip_device)], dim=1)
    J = torch.einsum("ba,bcg->bcag", abar, Dd).reshape(nb, nc, -1)
    want = kron_covariance([(J, K1d, K2d)]).cpu().numpy()
    got = kron_covariance_outer([(ad, Dd, K1d, K2d)]).cpu().numpy()
    print("max diff / max =", float(np.abs(got - want).max() / np.abs(want).max()))
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5 * np.abs(want).max())


def test_shape_mismatches_raise(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_outer
    a, D = torch.zeros(2, 5, device=hip_device), torch.zeros(2, 3, 4, device=hip_device)
    K2 = torch.eye(4, device=hip_device)
    for nA in (4, 7):
        with pytest.raises(ValueError):
            kron_covariance_outer([(a, D, torch.eye(nA, device=hip_device), K2)])
    with pytest.raises(ValueError):
        kron_covariance_outer([(a[:1], D, torch.eye(6, device=hip_device), K2)])
    with pytest.raises(ValueError):
        kron_covariance_outer([(a, torch.zeros(2, 33, 4, device=hip_device), torch.eye(6, device=hip_device), K2)])


# ------------------------------------------------------------------ end to end
def _fit(dev, net, make_x, loss_of):
    from bnn_kfac_amd.curvatures import KFAC
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
    return net, net64, kfac, step


def _check_factored(dev, net, make_x, loss_of, n_test, chunk):
    from bnn_kfac_amd.variance import glm_predictive
    net, net64, kfac, step = _fit(dev, net, make_x, loss_of)
    x = make_x(n_test)
    logits, cov = glm_predictive(kfac, x, chunk=chunk, jacobians="factored")
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
    logits, cov = logits.cpu().numpy(), cov.cpu().numpy()
    assert cov.shape == want_cov.shape and logits.shape == want_logits.shape
    np.testing.assert_allclose(logits, direct, rtol=1e-6, atol=1e-6 * np.abs(direct).max())
    np.testing.assert_allclose(logits, want_logits, rtol=1e-4, atol=1e-5 * np.abs(want_logits).max())
    for b in range(cov.shape[0]):
        print("sample", b, "max err / max|want| =",
              float(np.abs(cov[b] - want_cov[b]).max() / np.abs(want_cov[b]).max()))
        np.testing.assert_allclose(cov[b], want_cov[b], rtol=1e-4, atol=1e-5 * np.abs(want_cov[b]).max())
    return cov


def test_factored_basenet750(hip_device):
    from models_for_tests import BaseNet750
    torch.manual_seed(0)
    cov = _check_factored(hip_device, BaseNet750(), lambda n: torch.rand(n, 1, 28, 28, device=hip_device),
                          _categorical_loss, n_test=5, chunk=2)
    assert cov.shape == (5, 10, 10)


def test_factored_layer_without_bias(hip_device):
    torch.manual_seed(0)
    net = nn.Sequential(nn.Linear(12, 7, bias=False), nn.Tanh(), nn.Linear(7, 3))
    _check_factored(hip_device, net, lambda n: torch.randn(n, 12, device=hip_device), _categorical_loss,
                    n_test=5, chunk=2)


def test_factored_regression_variance(hip_device):
    torch.manual_seed(0)
    net = nn.Sequential(nn.Linear(4, 8), nn.Tanh(), nn.Linear(8, 1))
    cov = _check_factored(hip_device, net, lambda n: torch.randn(n, 4, device=hip_device),
                          lambda out: ((out - torch.randn_like(out)) ** 2).mean(), n_test=6, chunk=4)
    assert cov.shape == (6, 1, 1) and (cov[:, 0, 0] > 0).all()


def test_factored_relu_inplace_after_linear(hip_device):
    torch.manual_seed(0)
    net = nn.Sequential(nn.Linear(9, 6), nn.ReLU(inplace=True), nn.Linear(6, 4))
    _check_factored(hip_device, net, lambda n: torch.randn(n, 9, device=hip_device), _categorical_loss,
                    n_test=5, chunk=3)


@pytest.fixture
def deterministic_convolutions():
    """torch's vmapped Conv2d weight gradient picks its MIOpen solver per call: on a
    one-sample chunk conv1's dense Jacobian differed between two calls by 6e-8 of its
    maximum (output_jacobians alone, kron_covariance on fixed rows is repeatable).  The
    bitwise comparison below is about this project's code, so it runs in torch's
    deterministic mode and on two-sample chunks, which repeat in either mode."""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = before


def test_unknown_route_raises_and_default_is_unchanged(hip_device, deterministic_convolutions):
    from bnn_kfac_amd.variance import glm_predictive, kron_covariance, output_jacobians
    from models_for_tests import BaseNet750
    torch.manual_seed(0)
    net, _, kfac, _ = _fit(hip_device, BaseNet750(), lambda n: torch.rand(n, 1, 28, 28, device=hip_device),
                           _categorical_loss)
    x = torch.rand(4, 1, 28, 28, device=hip_device)
    with pytest.raises(ValueError):
        glm_predictive(kfac, x, jacobians="nope")
    logits, cov = glm_predictive(kfac, x, chunk=2)
    logits2, cov2 = glm_predictive(kfac, x, chunk=2, jacobians="dense")
    assert torch.equal(logits, logits2) and torch.equal(cov, cov2)
    layers = [m for m in list(net.modules())[1:] if m in kfac.state]
    for c0 in range(0, 4, 2):  # the dense route, spelled out per chunk
        f, Js = output_jacobians(net, layers, x[c0:c0 + 2])
        want = kron_covariance([(J, *kfac.inv_state[l]) for l, J in zip(layers, Js)], lower=True)
        assert torch.equal(logits[c0:c0 + 2], f) and torch.equal(cov[c0:c0 + 2], want)
