"""GPU: the joint GLM predictive -- kfac_kron_cov_joint / kfac_kron_cov_outer_joint
(variance.kron_covariance_joint / kron_covariance_outer_joint) against fp64 numpy on the
same fp32 inputs, integer-exact on small-integer inputs, their bitwise guarantees
(symmetry, repeatability, strides, subsets of the samples), their agreement with the
per-sample calls and with each other, and variance.glm_predictive(joint=True) end to end
against an fp64 CPU recompute.

Kernel tolerance: the project's, rtol 1e-5, atol 1e-5 * max|ref|.  Two fp32 evaluations of
one quantity (per-sample call, factored against dense, end to end): rtol 1e-4, atol 1e-5 * max;
end to end per block (b, b') the maximum is the Cauchy-Schwarz scale
sqrt(max|want[b,:,b,:]| * max|want[b',:,b',:]|) of that block."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import glm_joint_cases as C
import glm_sweep_cases as S

pytestmark = pytest.mark.gpu

# (nA, nG, nb, nc)
DENSE = [(3, 2, 1, 1),          # R = 1
         (5, 4, 3, 10),         # R = 30 < 32
         (5, 4, 7, 10),         # R = 70: a partial second tile, one off-diagonal tile
         (9, 7, 13, 5),         # R = 65: one row alone in tile 1
         (65, 33, 2, 3),        # K = 2145: two segments, ragged last
         (130, 33, 3, 2),       # K = 4290: three segments
         (20, 31, 5, 33),       # nc > 32, R = 165: three tiles
         (6, 5, 1, 40),         # one sample, nc = 40
         (785, 128, 8, 10)]     # the MLP layer
# (cols, has_ones, nG, nb, nc)
OUTER = [(4, 1, 3, 1, 1),       # R = 1
         (63, 1, 10, 7, 10),    # nA = 64, R = 70
         (64, 1, 10, 13, 5),    # nA = 65, R = 65
         (128, 0, 65, 2, 33),   # no bias, nc > 32
         (130, 1, 130, 70, 2),  # nb = 70: S crosses a tile, R = 140
         (20, 1, 2100, 3, 4),   # W over two segments
         (4096, 1, 4096, 8, 10)]  # C5's layer
IDS = lambda s: "x".join(map(str, s))  # noqa: E731


def _dev(dev, *arrays):
    return [torch.from_numpy(np.array(t)).to(dev) for t in arrays]  # (a copy: the cached case stays read-only)


def _flat(cov):
    R = cov.shape[0] * cov.shape[1]
    assert cov.is_contiguous()
    return cov.view(R, R)


def _check(got, ref):
    print("max err / max|ref| =", float(np.abs(got - ref).max() / np.abs(ref).max()))
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())


# ------------------------------------------------------------------ against fp64
@pytest.mark.parametrize("shape", DENSE, ids=IDS)
def test_joint_matches_fp64(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance_joint
    nA, nG, nb, nc = shape
    J, K1, K2, ref = C.dense_case(*shape)
    got = kron_covariance_joint([tuple(_dev(hip_device, J, K1, K2))], lower=True)
    assert got.shape == (nb, nc, nb, nc) and got.dtype == torch.float32
    _check(_flat(got).cpu().numpy(), ref)


@pytest.mark.parametrize("shape", OUTER, ids=IDS)
def test_outer_joint_matches_fp64(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance_outer_joint
    cols, ones, nG, nb, nc = shape
    a, D, K1, K2, ref = C.outer_case(*shape)
    got = kron_covariance_outer_joint([tuple(_dev(hip_device, a, D, K1, K2))], lower=True)
    assert got.shape == (nb, nc, nb, nc) and got.dtype == torch.float32
    _check(_flat(got).cpu().numpy(), ref)


@pytest.mark.parametrize("shape", [(5, 4, 7, 10), (65, 33, 2, 3)], ids=IDS)
def test_joint_dense_factors(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance_joint
    J, K1, K2, ref = C.dense_case(*shape, lower=False)
    assert np.abs(np.triu(K1, 1)).max() > 0 and np.abs(np.triu(K2, 1)).max() > 0
    _check(_flat(kron_covariance_joint([tuple(_dev(hip_device, J, K1, K2))], lower=False)).cpu().numpy(), ref)


@pytest.mark.parametrize("shape", [(63, 1, 10, 7, 10), (128, 0, 65, 2, 33)], ids=IDS)
def test_outer_joint_dense_factors(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance_outer_joint
    a, D, K1, K2, ref = C.outer_case(*shape, lower=False)
    assert np.abs(np.triu(K1, 1)).max() > 0 and np.abs(np.triu(K2, 1)).max() > 0
    got = kron_covariance_outer_joint([tuple(_dev(hip_device, a, D, K1, K2))], lower=False)
    _check(_flat(got).cpu().numpy(), ref)


# ------------------------------------------------------------------ integer-exact
LIMIT = 1 << 24


@pytest.mark.parametrize("lower", [True, False], ids=["lower", "dense"])
def test_joint_integer_exact(hip_device, lower):
    """Small-integer inputs: every product and partial sum is an integer below 2^24, so fp32
    is exact and the result must have the int64 reference's bits.  A transposed tile or a
    wrong mirror cannot pass."""
    from bnn_kfac_amd.variance import kron_covariance_joint
    nA, nG, nb, nc = 5, 4, 7, 10
    rng = np.random.default_rng(7)
    J, K1, K2 = C.small_ints(rng, nb, nc, nA * nG), C.small_ints(rng, nA, nA), C.small_ints(rng, nG, nG)
    if lower:
        K1, K2 = np.tril(K1), np.tril(K2)
    M = J.reshape(-1, nA, nG)
    bound_U = np.abs(K1).T @ np.abs(M)
    bound_T = (bound_U @ np.abs(K2)).reshape(nb * nc, -1)
    assert bound_U.max() < LIMIT and bound_T.max() < LIMIT and (bound_T @ bound_T.T).max() < LIMIT
    want = C.dense_joint_ref(J, nA, nG, K1, K2)
    assert want.dtype == np.int64 and np.abs(want).max() < LIMIT and not np.array_equal(want, np.diag(np.diag(want)))
    got = kron_covariance_joint([tuple(_dev(hip_device, *(t.astype(np.float32) for t in (J, K1, K2))))],
                                lower=lower)
    assert torch.equal(_flat(got).cpu(), torch.from_numpy(want.astype(np.float32)))


@pytest.mark.parametrize("lower", [True, False], ids=["lower", "dense"])
def test_outer_joint_integer_exact(hip_device, lower):
    """The factored route on small integers: a wrong b(r) cannot pass."""
    from bnn_kfac_amd.variance import kron_covariance_outer_joint
    cols, ones, nG, nb, nc = 4, 1, 3, 7, 10
    rng = np.random.default_rng(11)
    a, D = C.small_ints(rng, nb, cols), C.small_ints(rng, nb, nc, nG)
    K1, K2 = C.small_ints(rng, cols + ones, cols + ones), C.small_ints(rng, nG, nG)
    if lower:
        K1, K2 = np.tril(K1), np.tril(K2)
    bU, bV = C.outer_uv(np.abs(a), ones, np.abs(D), np.abs(K1), np.abs(K2))
    bS, bW = bU @ bU.T, bV @ bV.T
    assert max(bU.max(), bV.max(), bS.max(), bW.max()) < LIMIT
    assert (np.kron(bS, np.ones((nc, nc), dtype=np.int64)) * bW).max() < LIMIT
    want = C.outer_joint_ref(a, ones, D, K1, K2)
    assert want.dtype == np.int64 and np.abs(want).max() < LIMIT
    got = kron_covariance_outer_joint(
        [tuple(_dev(hip_device, *(t.astype(np.float32) for t in (a, D, K1, K2))))], lower=lower)
    assert torch.equal(_flat(got).cpu(), torch.from_numpy(want.astype(np.float32)))


# ------------------------------------------------------------------ bitwise guarantees
def test_joint_symmetric_repeatable_nonnegative(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_joint
    for shape in ((5, 4, 7, 10), (65, 33, 2, 3), (20, 31, 5, 33)):
        terms = [tuple(_dev(hip_device, *C.dense_case(*shape)[:3]))]
        one, two = _flat(kron_covariance_joint(terms)), _flat(kron_covariance_joint(terms))
        assert torch.equal(one, one.T)
        assert torch.equal(one, two)
        assert bool((torch.diagonal(one) >= 0).all())


def test_outer_joint_symmetric_repeatable_nonnegative(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_outer_joint
    for shape in ((63, 1, 10, 7, 10), (130, 1, 130, 70, 2), (20, 1, 2100, 3, 4)):
        terms = [tuple(_dev(hip_device, *C.outer_case(*shape)[:4]))]
        one, two = _flat(kron_covariance_outer_joint(terms)), _flat(kron_covariance_outer_joint(terms))
        assert torch.equal(one, one.T)
        assert torch.equal(one, two)
        assert bool((torch.diagonal(one) >= 0).all())


def _padded(t, extra, dev):
    """t's values in a NaN-filled tensor `extra` wider in the last dimension, as a view."""
    wide = torch.full(tuple(t.shape[:-1]) + (t.shape[-1] + extra,), float("nan"), device=dev)
    wide[..., :t.shape[-1]] = t
    return wide[..., :t.shape[-1]]


def test_joint_strides(hip_device):
    from bnn_kfac_amd import _native as N
    from bnn_kfac_amd import variance
    nA, nG, nb, nc = shape = (5, 4, 7, 10)
    R = nb * nc
    Jd, K1d, K2d = _dev(hip_device, *C.dense_case(*shape)[:3])
    plain = _flat(variance.kron_covariance_joint([(Jd, K1d, K2d)]))
    J_s = _padded(Jd, 5, hip_device)
    assert J_s.stride(1) == nA * nG + 5
    assert torch.equal(_flat(variance.kron_covariance_joint([(J_s, K1d, K2d)])), plain)
    assert torch.equal(_flat(variance.kron_covariance_joint(
        [(Jd, _padded(K1d, 3, hip_device), _padded(K2d, 2, hip_device))])), plain)
    keep, jobs, _, _ = variance._cov_jobs([(J_s, K1d, K2d)], True, "test")
    wide = torch.full((R, R + 3), float("nan"), device=hip_device)
    N.kron_cov_joint([N.CovJob(*j) for j in jobs], nb, nc, wide[:, :R])
    assert torch.equal(wide[:, :R], plain) and bool(torch.isnan(wide[:, R:]).all())


def test_outer_joint_strides(hip_device):
    from bnn_kfac_amd import _native as N
    from bnn_kfac_amd import variance
    cols, ones, nG, nb, nc = shape = (63, 1, 10, 7, 10)
    R = nb * nc
    ad, Dd, K1d, K2d = _dev(hip_device, *C.outer_case(*shape)[:4])
    plain = _flat(variance.kron_covariance_outer_joint([(ad, Dd, K1d, K2d)]))
    a_s, D_s = _padded(ad, 7, hip_device), _padded(Dd, 5, hip_device)
    assert a_s.stride(0) == cols + 7 and D_s.stride(1) == nG + 5
    assert torch.equal(_flat(variance.kron_covariance_outer_joint([(a_s, Dd, K1d, K2d)])), plain)
    assert torch.equal(_flat(variance.kron_covariance_outer_joint([(ad, D_s, K1d, K2d)])), plain)
    keep, jobs, _, _ = variance._cov_outer_jobs([(a_s, D_s, K1d, K2d)], True, "test")
    wide = torch.full((R, R + 3), float("nan"), device=hip_device)
    N.kron_cov_outer_joint([N.CovOuterJob(*j) for j in jobs], nb, nc, wide[:, :R])
    assert torch.equal(wide[:, :R], plain) and bool(torch.isnan(wide[:, R:]).all())


SUBSET = [1, 3, 6]


def test_joint_subset_of_the_samples_has_the_same_bits(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_joint
    Jd, K1d, K2d = _dev(hip_device, *C.dense_case(5, 4, 7, 10)[:3])
    whole = kron_covariance_joint([(Jd, K1d, K2d)])
    part = kron_covariance_joint([(Jd[SUBSET].contiguous(), K1d, K2d)])
    assert part.shape == (3, 10, 3, 10)
    assert torch.equal(part, whole[SUBSET][:, :, SUBSET])


def test_outer_joint_subset_of_the_samples_has_the_same_bits(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_outer_joint
    ad, Dd, K1d, K2d = _dev(hip_device, *C.outer_case(63, 1, 10, 7, 10)[:4])
    whole = kron_covariance_outer_joint([(ad, Dd, K1d, K2d)])
    part = kron_covariance_outer_joint([(ad[SUBSET].contiguous(), Dd[SUBSET].contiguous(), K1d, K2d)])
    assert part.shape == (3, 10, 3, 10)
    assert torch.equal(part, whole[SUBSET][:, :, SUBSET])


# ------------------------------------------------------------------ agreement
def _close(got, want):
    print("max diff / max =", float(np.abs(got - want).max() / np.abs(want).max()))
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5 * np.abs(want).max())


@pytest.mark.parametrize("shape", [s for s in DENSE if s[3] <= 32], ids=IDS)
def test_joint_diagonal_blocks_are_the_per_sample_call(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance, kron_covariance_joint, marginal_blocks
    terms = [tuple(_dev(hip_device, *C.dense_case(*shape)[:3]))]
    _close(marginal_blocks(kron_covariance_joint(terms)).cpu().numpy(), kron_covariance(terms).cpu().numpy())


@pytest.mark.parametrize("shape", [s for s in OUTER if s[4] <= 32], ids=IDS)
def test_outer_joint_diagonal_blocks_are_the_per_sample_call(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance_outer, kron_covariance_outer_joint, marginal_blocks
    terms = [tuple(_dev(hip_device, *C.outer_case(*shape)[:4]))]
    _close(marginal_blocks(kron_covariance_outer_joint(terms)).cpu().numpy(),
           kron_covariance_outer(terms).cpu().numpy())


@pytest.mark.parametrize("shape", [(63, 1, 10, 7, 10), (128, 0, 65, 2, 33)], ids=IDS)
def test_factored_agrees_with_dense_on_outer_rows(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance_joint, kron_covariance_outer_joint
    a, D, K1, K2, _ = C.outer_case(*shape)
    ad, Dd, K1d, K2d, Jd = _dev(hip_device, a, D, K1, K2, C.outer_rows(a, shape[1], D))
    _close(kron_covariance_outer_joint([(ad, Dd, K1d, K2d)]).cpu().numpy(),
           kron_covariance_joint([(Jd, K1d, K2d)]).cpu().numpy())


# ------------------------------------------------------------------ folding and errors
def test_joint_nine_terms_fold_in_groups_of_eight(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_joint
    shapes = [(3, 2), (5, 4), (9, 7), (65, 33), (12, 4), (20, 31), (33, 3), (8, 8), (6, 5)]
    terms, ref = [], 0.0
    for nA, nG in shapes:
        *arrays, r = C.dense_case(nA, nG, 3, 4)
        terms.append(tuple(_dev(hip_device, *arrays)))
        ref = ref + r
    _check(_flat(kron_covariance_joint(terms, lower=True)).cpu().numpy(), ref)


def test_outer_joint_nine_terms_fold_in_groups_of_eight(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_outer_joint
    shapes = [(4, 1, 3), (63, 1, 10), (9, 0, 10), (70, 1, 65), (12, 1, 4), (20, 1, 130), (33, 0, 31),
              (8, 1, 8), (64, 1, 64)]
    terms, ref = [], 0.0
    for cols, ones, nG in shapes:
        *arrays, r = C.outer_case(cols, ones, nG, 3, 4)
        terms.append(tuple(_dev(hip_device, *arrays)))
        ref = ref + r
    _check(_flat(kron_covariance_outer_joint(terms, lower=True)).cpu().numpy(), ref)


def test_shape_mismatches_raise(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_joint, kron_covariance_outer_joint
    eye = lambda n: torch.eye(n, device=hip_device)  # noqa: E731
    J = torch.zeros(2, 3, 20, device=hip_device)
    with pytest.raises(ValueError):
        kron_covariance_joint([])
    with pytest.raises(ValueError):
        kron_covariance_joint([(J, eye(5), eye(3))])           # 20 columns, kron needs 15
    with pytest.raises(ValueError):
        kron_covariance_joint([(J, eye(5), torch.zeros(4, 3, device=hip_device))])
    with pytest.raises(ValueError):
        kron_covariance_joint([(J, eye(5), eye(4)), (J[:1], eye(5), eye(4))])
    a, D = torch.zeros(2, 5, device=hip_device), torch.zeros(2, 3, 4, device=hip_device)
    with pytest.raises(ValueError):
        kron_covariance_outer_joint([])
    for nA in (4, 7):
        with pytest.raises(ValueError):
            kron_covariance_outer_joint([(a, D, eye(nA), eye(4))])
    with pytest.raises(ValueError):
        kron_covariance_outer_joint([(a[:1], D, eye(6), eye(4))])


def test_workspace_one_byte_short_raises(hip_device):
    from bnn_kfac_amd import _native as N
    from bnn_kfac_amd import variance
    dense = [tuple(_dev(hip_device, *C.dense_case(65, 33, 2, 3)[:3]))]
    need = N.kron_cov_joint_workspace_bytes(
        [N.CovJob(*j) for j in variance._cov_jobs(dense, True, "test")[1]], 2, 3)
    assert need > 0
    variance.kron_covariance_joint(dense, max_workspace_bytes=need)
    with pytest.raises(ValueError, match=str(need)):
        variance.kron_covariance_joint(dense, max_workspace_bytes=need - 1)
    outer = [tuple(_dev(hip_device, *C.outer_case(63, 1, 10, 7, 10)[:4]))]
    need = N.kron_cov_outer_joint_workspace_bytes(
        [N.CovOuterJob(*j) for j in variance._cov_outer_jobs(outer, True, "test")[1]], 7, 10)
    assert need > 0
    variance.kron_covariance_outer_joint(outer, max_workspace_bytes=need)
    with pytest.raises(ValueError, match=str(need)):
        variance.kron_covariance_outer_joint(outer, max_workspace_bytes=need - 1)


# ------------------------------------------------------------------ end to end
@pytest.fixture
def deterministic_convolutions():
    """(test_gpu_glm_factored's finding: torch's vmapped Conv2d weight gradient picks its
    MIOpen solver per call; the bitwise comparison of two glm_predictive calls is about this
    project's code, so it runs in torch's deterministic mode.)"""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = before


def _make_x(dev, xshape):
    if len(xshape) == 3:
        return lambda n: torch.rand(n, *xshape, device=dev)
    return lambda n: torch.randn(n, *xshape, device=dev)


@pytest.mark.parametrize("name", ["no_bias", "regression", "relu_inplace", "basenet750"])
def test_glm_predictive_joint(hip_device, deterministic_convolutions, name):
    from bnn_kfac_amd.variance import glm_predictive, marginal_blocks
    make, xshape, loss_of = S.small_nets()[name]
    torch.manual_seed(0)
    make_x = _make_x(hip_device, xshape)
    net, net64, kfac = S.fit(hip_device, make(), make_x, loss_of)
    kfac.invert(0.04, 200)
    n = 5
    x = make_x(n)
    layers = [m for m in list(net.modules())[1:] if m in kfac.state]
    layers64 = [m for m in list(net64.modules())[1:] if isinstance(m, (nn.Linear, nn.Conv2d))]
    assert len(layers) == len(layers64)
    want_logits, rows = S.fp64_rows(net64, layers64, x.cpu())
    want = 0.0
    for layer, M in zip(layers, rows):
        LA, LG = (t.double().cpu().numpy() for t in kfac.inv_state[layer])
        want = want + np.einsum("bcag,ai,gh,dfih->bcdf", M, LA @ LA.T, LG @ LG.T, M, optimize=True)
    nc = want.shape[1]
    scale = np.array([np.abs(want[b, :, b, :]).max() for b in range(n)])
    with torch.no_grad():
        direct = net(x).cpu().numpy()
    per_sample = glm_predictive(kfac, x, chunk=2, joint=False)
    default = glm_predictive(kfac, x, chunk=2)
    assert torch.equal(default[0], per_sample[0]) and torch.equal(default[1], per_sample[1])
    for route in ("dense", "factored"):
        logits, cov = glm_predictive(kfac, x, chunk=2, jacobians=route, joint=True)
        assert logits.shape == (n, nc) and cov.shape == (n, nc, n, nc)
        flat = _flat(cov)
        assert torch.equal(flat, flat.T)
        logits, cov = logits.cpu().numpy(), cov.cpu().numpy()
        np.testing.assert_allclose(logits, direct, rtol=1e-6, atol=1e-6 * np.abs(direct).max())
        np.testing.assert_allclose(logits, want_logits, rtol=1e-4, atol=1e-5 * np.abs(want_logits).max())
        worst = 0.0
        for b in range(n):
            for b2 in range(n):
                s = np.sqrt(scale[b] * scale[b2])
                worst = max(worst, float(np.abs(cov[b, :, b2, :] - want[b, :, b2, :]).max() / s))
        print(name, route, "max over blocks of max err / Cauchy-Schwarz scale =", worst)
        for b in range(n):
            for b2 in range(n):
                np.testing.assert_allclose(cov[b, :, b2, :], want[b, :, b2, :], rtol=1e-4,
                                           atol=1e-5 * np.sqrt(scale[b] * scale[b2]))
        marg = marginal_blocks(torch.from_numpy(cov)).numpy()
        ref = glm_predictive(kfac, x, chunk=2, jacobians=route)[1].cpu().numpy()
        np.testing.assert_allclose(marg, ref, rtol=1e-4, atol=1e-5 * np.abs(ref).max())
    # hooks intact: another forward/backward + update still moves the factors
    before = kfac.state[layers[0]][0].clone()
    out = net(make_x(64))
    net.zero_grad()
    loss_of(out).backward()
    kfac.update(64)
    torch.cuda.synchronize()
    assert not torch.equal(before, kfac.state[layers[0]][0])
