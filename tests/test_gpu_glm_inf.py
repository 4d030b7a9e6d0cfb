"""GPU: the GLM predictive under the INF posterior -- kfac_inf_cov and kfac_inf_cov_outer
(variance.kron_covariance_inf / kron_covariance_outer_inf) against fp64 numpy on the same fp32
inputs, against each other, their bitwise guarantees, one integer-exact case per route, and
variance.glm_predictive_inf / inf_log_det end to end against an fp64 host J P^-1 J^T built from
`inf.state`.

Tolerance (glm_inf_cases.SCALE, from the fp32 stage chain measured on the CPU): rtol = SCALE,
atol = SCALE * max|first term|, for the two device routes against each other too."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

import glm_inf_cases as C
import glm_sweep_cases as S
from models_for_tests import BaseNet750, mlp

pytestmark = pytest.mark.gpu

IDS = lambda s: "x".join(map(str, s))  # noqa: E731
OUTER3 = [(63, 1, 10, 5, 3, 3, 10), (130, 1, 130, 33, 9, 70, 2), (300, 0, 257, 3, 2, 3, 4)]
DENSE3 = [(64, 10, 8, 4, 3, 10), (33, 65, 5, 7, 2, 5), (26, 5, 26, 5, 3, 32)]


def _dev(dev, *arrays):
    return [torch.from_numpy(np.array(t)).to(dev) for t in arrays]  # (a copy: the cached case stays read-only)


def _check(got, ref, top, scale=C.SCALE):
    """rtol = scale, atol = scale * max|first term|."""
    assert got.shape == ref.shape
    print("max err / max|first term| =", float(np.abs(got - ref).max() / top), "of", scale)
    np.testing.assert_allclose(got, ref, rtol=scale, atol=scale * top)


def _outer_terms(dev, shape):
    *inputs, ref, top = C.outer_case(*shape)
    return [tuple(_dev(dev, *inputs))], ref, top


def _dense_terms(dev, shape):
    *inputs, ref, top = C.dense_case(*shape)
    return [tuple(_dev(dev, *inputs))], ref, top


def _routes():
    from bnn_kfac_amd.variance import kron_covariance_inf, kron_covariance_outer_inf
    return {"outer": (kron_covariance_outer_inf, _outer_terms, OUTER3),
            "dense": (kron_covariance_inf, _dense_terms, DENSE3)}


# ------------------------------------------------------------------ 1: against fp64
@pytest.mark.parametrize("shape", C.OUTER_SHAPES, ids=IDS)
def test_outer_inf_matches_fp64(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance_outer_inf
    terms, ref, top = _outer_terms(hip_device, shape)
    got = kron_covariance_outer_inf(terms)
    assert got.shape == (shape[5], shape[6], shape[6]) and got.dtype == torch.float32
    _check(got.cpu().numpy(), ref, top)


@pytest.mark.parametrize("shape", C.DENSE_SHAPES, ids=IDS)
def test_dense_inf_matches_fp64(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance_inf
    terms, ref, top = _dense_terms(hip_device, shape)
    got = kron_covariance_inf(terms)
    assert got.shape == (shape[4], shape[5], shape[5]) and got.dtype == torch.float32
    _check(got.cpu().numpy(), ref, top)


# ------------------------------------------------------------------ 2: the two routes
@pytest.mark.parametrize("shape", C.OUTER_SHAPES, ids=IDS)
def test_outer_route_agrees_with_dense_route_on_materialised_rows(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance_inf, kron_covariance_outer_inf
    a, D, UA, UG, W, F, ref, top = C.outer_case(*shape)
    ad, Dd, UAd, UGd, Wd, Fd, Jd = _dev(hip_device, a, D, UA, UG, W, F, C.rows_of(a, shape[1], D))
    outer = kron_covariance_outer_inf([(ad, Dd, UAd, UGd, Wd, Fd)])
    dense = kron_covariance_inf([(Jd, UAd, UGd, Wd, Fd)])
    _check(outer.cpu().numpy(), dense.cpu().numpy().astype(np.float64), top)
    _check(dense.cpu().numpy(), ref, top)


# ------------------------------------------------------------------ 3: bitwise properties
@pytest.mark.parametrize("route", ["outer", "dense"])
def test_repeatable_and_bitwise_symmetric(hip_device, route):
    fn, make, shapes = _routes()[route]
    for shape in shapes:
        terms, _, _ = make(hip_device, shape)
        once = fn(terms)
        assert torch.equal(once, fn(terms)), shape
        assert torch.equal(once, once.mT), shape


def _job_bytes(route, shape, n):
    from bnn_kfac_amd import _native as N
    if route == "outer":
        cols, ones, nG, ra, rg, nb, nc = shape
        nA = cols + ones
        job = N.InfCovOuterJob(1, cols, cols, ones, 1, nG, nG, 0, 1, ra, ra, 1, rg, rg, 1, nA * nG, 1, ra * rg)
        return N.inf_cov_outer_workspace_bytes([job], n, nc)
    nA, nG, ra, rg, nb, nc = shape
    job = N.InfCovJob(1, nA * nG, nA, nG, 1, ra, ra, 1, rg, rg, 1, nA * nG, 1, ra * rg)
    return N.inf_cov_workspace_bytes([job], n, nc)


@pytest.mark.parametrize("route", ["outer", "dense"])
def test_one_sample_chunks_do_not_change_a_bit(hip_device, route):
    fn, make, shapes = _routes()[route]
    for shape in shapes:
        terms, _, _ = make(hip_device, shape)
        one, two = _job_bytes(route, shape, 1), _job_bytes(route, shape, 2)
        assert 0 < one < two  # a budget of `one` forces chunks of one sample
        assert torch.equal(fn(terms, max_workspace_bytes=one), fn(terms)), shape
        with pytest.raises(ValueError):
            fn(terms, max_workspace_bytes=one - 1)


def test_outer_sample_block_unchanged_by_other_samples(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_outer_inf
    (a, D, *ops), = _outer_terms(hip_device, (130, 1, 130, 33, 9, 70, 2))[0]
    whole = kron_covariance_outer_inf([(a, D, *ops)])
    assert whole.shape[0] == 70
    assert torch.equal(kron_covariance_outer_inf([(a[:3], D[:3], *ops)]), whole[:3])
    assert torch.equal(kron_covariance_outer_inf([(a[66:], D[66:], *ops)]), whole[66:])


def test_dense_sample_block_unchanged_by_other_samples(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_inf
    (J, *ops), = _dense_terms(hip_device, (64, 10, 8, 4, 3, 10))[0]
    whole = kron_covariance_inf([(J, *ops)])
    assert torch.equal(kron_covariance_inf([(J[-1:], *ops)])[0], whole[-1])
    assert torch.equal(kron_covariance_inf([(J[:2], *ops)]), whole[:2])


def test_nine_terms_fold_in_groups_of_eight(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_inf, kron_covariance_outer_inf
    shapes = [(4, 1, 3, 2, 1), (63, 1, 10, 5, 3), (9, 0, 10, 9, 2), (70, 1, 65, 3, 33), (12, 1, 4, 4, 4),
              (20, 1, 130, 7, 2), (33, 0, 31, 1, 31), (8, 1, 8, 2, 2), (64, 1, 64, 6, 6)]
    terms, ref, top = [], 0.0, 0.0
    for dims in shapes:
        *inputs, r, t = C.outer_case(*dims, 3, 4)
        terms.append(tuple(_dev(hip_device, *inputs)))
        ref, top = ref + r, top + t
    _check(kron_covariance_outer_inf(terms).cpu().numpy(), ref, top)
    dshapes = [(5, 3, 2, 2), (64, 10, 8, 4), (9, 10, 9, 2), (33, 65, 5, 7), (12, 4, 4, 4), (20, 13, 7, 2),
               (70, 1, 9, 1), (8, 8, 2, 2), (26, 5, 26, 5)]
    terms, ref, top = [], 0.0, 0.0
    for dims in dshapes:
        *inputs, r, t = C.dense_case(*dims, 3, 4)
        terms.append(tuple(_dev(hip_device, *inputs)))
        ref, top = ref + r, top + t
    _check(kron_covariance_inf(terms).cpu().numpy(), ref, top)


def _padded_rows(t, dev, pad=3):
    """The same values with row stride n + pad, from a base an odd number of floats in."""
    n = t.shape[-1]
    lead = t.shape[:-1]
    buf = torch.full((int(np.prod(lead)) * (n + pad) + 1,), float("nan"), device=dev)
    view = buf[1:].view(*lead, n + pad)[..., :n]
    view.copy_(t)
    assert view.data_ptr() == buf.data_ptr() + 4 and view.stride(-2) == n + pad
    return view


@pytest.mark.parametrize("shape", OUTER3, ids=IDS)
def test_outer_strided_inputs_bit_equal(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance_outer_inf
    (a, D, UA, UG, W, F), = _outer_terms(hip_device, shape)[0]
    plain = kron_covariance_outer_inf([(a, D, UA, UG, W, F)])
    wide = torch.full((a.shape[0], a.shape[1] + 7), float("nan"), device=hip_device)
    wide[:, 2:2 + a.shape[1]] = a
    a_slice = wide[:, 2:2 + a.shape[1]]       # a column slice of a wider tensor: not copied
    Dp, UAp, UGp, Fp = (_padded_rows(t, hip_device) for t in (D, UA, UG, F))
    for terms in ((a_slice, D, UA, UG, W, F), (a, Dp, UA, UG, W, F), (a, D, UAp, UG, W, F),
                  (a_slice, Dp, UAp, UGp, W, Fp)):
        assert torch.equal(kron_covariance_outer_inf([terms]), plain)


@pytest.mark.parametrize("shape", DENSE3, ids=IDS)
def test_dense_strided_inputs_bit_equal(hip_device, shape):
    from bnn_kfac_amd.variance import _cov_rows, kron_covariance_inf
    (J, UA, UG, W, F), = _dense_terms(hip_device, shape)[0]
    plain = kron_covariance_inf([(J, UA, UG, W, F)])
    Jp, UAp, UGp, Fp = (_padded_rows(t, hip_device) for t in (J, UA, UG, F))
    assert _cov_rows(Jp, J.shape[2])[1] == J.shape[2] + 3      # a padded row stride: not copied
    for terms in ((Jp, UA, UG, W, F), (J, UAp, UG, W, F), (Jp, UAp, UGp, W, Fp)):
        assert torch.equal(kron_covariance_inf([terms]), plain)


def test_accumulate_adds(hip_device):
    from bnn_kfac_amd import _native as N
    a, D, UA, UG, W, F, ref, top = C.outer_case(63, 1, 10, 5, 3, 3, 10)
    ad, Dd, UAd, UGd, Wd, Fd = _dev(hip_device, a, D, UA, UG, W, F)
    job = N.InfCovOuterJob(ad.data_ptr(), 63, 63, 1, Dd.data_ptr(), 10, 10, 0, UAd.data_ptr(), 5, 5,
                           UGd.data_ptr(), 3, 3, Wd.data_ptr(), 640, Fd.data_ptr(), 15)
    base = torch.from_numpy(np.array(ref)).float().to(hip_device) * 0.5
    base = (base + base.mT) / 2
    out = base.clone()
    N.inf_cov_outer([job], 3, 10, out, accumulate=True)
    _check(out.cpu().numpy(), ref + base.cpu().numpy().astype(np.float64), top)
    N.inf_cov_outer([job], 3, 10, out, accumulate=False)
    _check(out.cpu().numpy(), ref, top)

    J, UA, UG, W, F, ref, top = C.dense_case(64, 10, 8, 4, 3, 10)
    Jd, UAd, UGd, Wd, Fd = _dev(hip_device, J, UA, UG, W, F)
    job = N.InfCovJob(Jd.data_ptr(), 640, 64, 10, UAd.data_ptr(), 8, 8, UGd.data_ptr(), 4, 4, Wd.data_ptr(), 640,
                      Fd.data_ptr(), 32)
    base = torch.from_numpy(np.array(ref)).float().to(hip_device) * 0.5
    base = (base + base.mT) / 2
    out = base.clone()
    N.inf_cov([job], 3, 10, out, accumulate=True)
    _check(out.cpu().numpy(), ref + base.cpu().numpy().astype(np.float64), top)
    N.inf_cov([job], 3, 10, out, accumulate=False)
    _check(out.cpu().numpy(), ref, top)


# ------------------------------------------------------------------ 4: integer-exact
def test_outer_inf_integer_exact(hip_device):
    """Small-integer inputs: every term any stage accumulates sums (in absolute value) below
    2^24, so every order of fp32 summation is exact and the whole buffer must equal int64's."""
    from bnn_kfac_amd.variance import kron_covariance_outer_inf
    *inputs, want, bound = C.int_outer_case()
    assert 0 < bound <= C.EXACT and np.abs(want).max() > 0
    got = kron_covariance_outer_inf([tuple(_dev(hip_device, *inputs))])
    assert torch.equal(got.cpu(), torch.from_numpy(want.astype(np.float32)))


def test_dense_inf_integer_exact(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_inf
    *inputs, want, bound = C.int_dense_case()
    assert 0 < bound <= C.EXACT and np.abs(want).max() > 0
    got = kron_covariance_inf([tuple(_dev(hip_device, *inputs))])
    assert torch.equal(got.cpu(), torch.from_numpy(want.astype(np.float32)))


# ------------------------------------------------------------------ 5: end to end
# Damping of the end-to-end check.  inf_covariance_factors takes vtv = sigma U^T diag(w) U sigma
# from kfac_kron_gram in fp32, so the low-rank term carries a relative error of about
# eps32 * ||vtv|| (B B^T = I + vtv has its smallest eigenvalue >= 1).  For that to stay inside
# SCALE = 1e-5 next to the kernels' own 1.5e-6, ||vtv|| must stay below about 100: the fixtures
# compute ||vtv||_2 in fp64 on the host and assert it is below VTV_MAX with this damping.
ADD, MULTIPLY = 1.0, 100.0
VTV_MAX = 50.0


def _fit_inf(dev, net, in_shape, classes, batch, rank=6):
    """KFAC factors, EFB on their eigenbases (test_gpu_efb.py's procedure), INF.update(rank).
    Returns (net on dev, its fp64 CPU copy, inf).  `batch`: enough samples for full-rank factors
    (the eigenvector solve of a 785 x 785 factor of rank 64 takes minutes)."""
    from bnn_kfac_amd.curvatures import EFB, INF, KFAC
    net64 = copy.deepcopy(net).double()  # (before KFAC hooks the modules)
    net = net.to(dev)
    kfac = KFAC(net)

    def backward():
        x = torch.rand(batch, *in_shape, device=dev)
        net.zero_grad()
        nn.functional.cross_entropy(net(x), torch.randint(0, classes, (batch,), device=dev)).backward()

    for _ in range(2):
        backward()
        kfac.update(batch_size=batch)
    factors = {m: [F.clone() for F in v] for m, v in kfac.state.items()}
    efb = EFB(net, factors)
    for _ in range(3):
        backward()
        efb.update(batch_size=batch)
    inf = INF(net, efb.diags, factors, efb.state)
    inf.update(rank=rank)
    return net, net64, inf


def _host_reference(inf, layers, rows, dense_limit=600):
    """(cov fp64 (n, nc, nc), max|first term|, log det P, its tolerance) from inf.state: P
    inverted densely where nA*nG <= dense_limit, through the fp64 Woodbury factors
    (test_glm_inf_host.py checks them against the dense inverse) where P would not fit.
    log det (I + vtv) moves by tr((I + vtv)^-1 dvtv) <= r ||dvtv|| for an error dvtv of the
    fp32 Gram, ||dvtv|| a few eps32 ||vtv||, and the fp32 diagonal of B^-1 adds 2 r eps32:
    tolerance 4 r eps32 (1 + ||vtv||) per layer."""
    cov, first_sum, logdet, logdet_atol = 0.0, 0.0, 0.0, 0.0
    for layer, M in zip(layers, rows):
        UA, UG, lam, corr = (t.double().cpu().numpy() for t in inf.state[layer])
        nA, nG = UA.shape[0], UG.shape[0]
        n, nc = M.shape[:2]
        J = M.reshape(n, nc, nA * nG)
        W, F = C.woodbury_factors(UA, UG, lam, corr, MULTIPLY, ADD)
        vtv = C.woodbury_gram(UA, UG, lam, corr, MULTIPLY, ADD)[2]
        assert np.linalg.norm(vtv, 2) <= VTV_MAX, np.linalg.norm(vtv, 2)
        logdet_atol += 4 * len(lam) * 2.0 ** -24 * (1 + np.linalg.norm(vtv, 2))
        first, second = C.dense_terms(J, nA, nG, UA, UG, W, F)
        if nA * nG <= dense_limit:
            U = np.kron(UA, UG)
            P = MULTIPLY * (U @ np.diag(lam) @ U.T + np.diag(np.maximum(corr, 0.0))) + ADD * np.eye(nA * nG)
            cov = cov + np.einsum("bck,kl,bdl->bcd", J, np.linalg.inv(P), J)
            logdet += np.linalg.slogdet(P)[1]
        else:
            cov = cov + first - second
            logdet += -np.log(W).sum() + np.linalg.slogdet(np.eye(len(lam)) + vtv)[1]
        first_sum = first_sum + first
        print(layer.__class__.__name__, (nA, nG), "rank", UA.shape[1], "x", UG.shape[1], "||vtv|| =",
              float(np.linalg.norm(vtv, 2)), "max|second| / max|first| =",
              float(np.abs(second).max() / np.abs(first).max()))
    return cov, float(np.abs(first_sum).max()), logdet, logdet_atol


@pytest.fixture(scope="module", params=["mlp", "conv"])
def fitted(request, hip_device):
    torch.manual_seed(0)
    if request.param == "mlp":
        net, in_shape, batch = mlp(), (784,), 512
        pick = lambda m: [m[0], m[2]]  # noqa: E731
    else:
        net, in_shape, batch = BaseNet750(), (1, 28, 28), 32
        pick = lambda m: [m.conv1, m.conv2, m.fc1]  # noqa: E731
    net, net64, inf = _fit_inf(hip_device, net, in_shape, 10, batch)
    x = torch.rand(4, *in_shape, device=hip_device)
    layers = pick(net)
    assert list(inf.state) == layers
    logits64, rows = S.fp64_rows(net64, pick(net64), x.cpu())
    return (net, inf, x, layers, logits64) + _host_reference(inf, layers, rows)


@pytest.mark.parametrize("route", ["dense", "factored"])
def test_glm_predictive_inf_end_to_end(hip_device, fitted, route):
    from bnn_kfac_amd.variance import glm_predictive_inf
    net, inf, x, layers, logits64, want, top, _, _ = fitted
    before = {m: tuple(t.clone() for t in v) for m, v in inf.state.items()}
    # (two chunks of one size: every new batch size costs the vmapped convolutions a solver search)
    logits, cov = glm_predictive_inf(inf, x, ADD, MULTIPLY, chunk=2, jacobians=route)   # needs no invert
    assert not inf.inv_state
    for m, v in inf.state.items():
        assert all(torch.equal(t, b) for t, b in zip(v, before[m]))
    assert logits.shape == (4, 10) and cov.shape == (4, 10, 10) and cov.dtype == torch.float32
    with torch.no_grad():
        direct = net(x).cpu().numpy()
    np.testing.assert_allclose(logits.cpu().numpy(), direct, rtol=1e-6, atol=1e-6 * np.abs(direct).max())
    np.testing.assert_allclose(logits.cpu().numpy(), logits64, rtol=1e-4, atol=1e-5 * np.abs(logits64).max())
    assert torch.equal(cov, cov.mT)
    _check(cov.cpu().numpy(), want, top)


def test_inf_log_det_on_the_device_state(hip_device, fitted):
    from bnn_kfac_amd.variance import inf_log_det
    _, inf, _, _, _, _, _, want, atol = fitted
    got = inf_log_det(inf, ADD, MULTIPLY)
    assert got.dim() == 0 and got.dtype == torch.float64 and got.device.type == "cuda"
    print("log det", float(got), "host", want, "diff", float(got) - want, "atol", atol)
    np.testing.assert_allclose(float(got), want, rtol=1e-12, atol=atol)
