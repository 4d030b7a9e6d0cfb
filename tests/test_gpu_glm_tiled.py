"""GPU: the class-tiled per-sample GLM covariance -- kfac_kron_cov_tiled /
kfac_kron_cov_outer_tiled (variance.kron_covariance_tiled / kron_covariance_outer_tiled) above
the 32-output cap of kfac_kron_cov / kfac_kron_cov_outer: against fp64 numpy on the same fp32
inputs, integer-exact on small-integer inputs, their bitwise guarantees (symmetry,
repeatability, sample chunks, strides), the dense route's bitwise tie to the joint call's
diagonal blocks, the outer route against the dense one on the rows it never forms, and both
against the capped calls at nc <= 32.  (glm_predictive end to end: test_gpu_glm_tiled_e2e.py.)

Tolerances are the project's (test_gpu_glm.py, test_gpu_glm_joint.py): against fp64 numpy
rtol 1e-5, atol 1e-5 * max|ref|; between two fp32 evaluations of one quantity rtol 1e-4,
atol 1e-5 * max."""
import numpy as np
import pytest
import torch

import glm_joint_cases as C
from glm_exact_cases import sparse_signs as _sparse_signs

pytestmark = pytest.mark.gpu

# (nA, nG, nb, nc)
DENSE = [(5, 4, 3, 33),         # one tile, one row in the second quadrant
         (6, 5, 1, 40),         # one sample
         (5, 4, 2, 64),         # one full tile
         (9, 7, 3, 65),         # one row alone in tile 1, three tile pairs
         (20, 31, 2, 130),      # three tiles, six pairs
         (65, 33, 2, 40),       # K = 2145: two segments, ragged last
         (257, 100, 2, 100),    # a 256 -> 100 head
         (33, 31, 2, 32),       # nc <= 32 through the tiled call
         (27, 6, 4, 3)]
# (cols, has_ones, nG, nb, nc)
OUTER = [(4, 1, 3, 1, 33),      # minimal case above the cap
         (63, 1, 10, 3, 64),    # one full class tile
         (64, 1, 40, 5, 65),    # one row alone in tile 1
         (128, 0, 65, 2, 130),  # no bias
         (20, 1, 2100, 2, 40),  # nG over two segments
         (130, 1, 130, 70, 33),  # nb crosses a row-norm sample tile
         (256, 1, 100, 4, 100),  # a 256 -> 100 head
         (512, 1, 1000, 2, 1000)]  # an ImageNet-sized head
IDS = lambda s: "x".join(map(str, s))  # noqa: E731


def _dev(dev, *arrays):
    return [torch.from_numpy(np.array(t)).to(dev) for t in arrays]  # (a copy: the cached case stays read-only)


def _blocks(ref, nb, nc):
    """The per-sample blocks (nb, nc, nc) of a joint reference (nb*nc, nb*nc)."""
    r4 = ref.reshape(nb, nc, nb, nc)
    return np.stack([r4[b, :, b, :] for b in range(nb)])


def _check(got, ref):
    print("max err / max|ref| =", float(np.abs(got - ref).max() / np.abs(ref).max()))
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())


def _close(got, want):
    print("max diff / max =", float(np.abs(got - want).max() / np.abs(want).max()))
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5 * np.abs(want).max())


# ------------------------------------------------------------------ against fp64
@pytest.mark.parametrize("shape", DENSE, ids=IDS)
def test_tiled_matches_fp64(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance_tiled
    nA, nG, nb, nc = shape
    J, K1, K2, ref = C.dense_case(*shape)
    got = kron_covariance_tiled([tuple(_dev(hip_device, J, K1, K2))], lower=True)
    assert got.shape == (nb, nc, nc) and got.dtype == torch.float32 and got.is_contiguous()
    _check(got.cpu().numpy(), _blocks(ref, nb, nc))


@pytest.mark.parametrize("shape", OUTER, ids=IDS)
def test_outer_tiled_matches_fp64(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance_outer_tiled
    cols, ones, nG, nb, nc = shape
    a, D, K1, K2, ref = C.outer_case(*shape)
    got = kron_covariance_outer_tiled([tuple(_dev(hip_device, a, D, K1, K2))], lower=True)
    assert got.shape == (nb, nc, nc) and got.dtype == torch.float32 and got.is_contiguous()
    _check(got.cpu().numpy(), _blocks(ref, nb, nc))


@pytest.mark.parametrize("shape", [(9, 7, 3, 65), (65, 33, 2, 40)], ids=IDS)
def test_tiled_dense_factors(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance_tiled
    J, K1, K2, ref = C.dense_case(*shape, lower=False)
    assert np.abs(np.triu(K1, 1)).max() > 0 and np.abs(np.triu(K2, 1)).max() > 0
    got = kron_covariance_tiled([tuple(_dev(hip_device, J, K1, K2))], lower=False)
    _check(got.cpu().numpy(), _blocks(ref, shape[2], shape[3]))


@pytest.mark.parametrize("shape", [(64, 1, 40, 5, 65), (128, 0, 65, 2, 130)], ids=IDS)
def test_outer_tiled_dense_factors(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance_outer_tiled
    a, D, K1, K2, ref = C.outer_case(*shape, lower=False)
    assert np.abs(np.triu(K1, 1)).max() > 0 and np.abs(np.triu(K2, 1)).max() > 0
    got = kron_covariance_outer_tiled([tuple(_dev(hip_device, a, D, K1, K2))], lower=False)
    _check(got.cpu().numpy(), _blocks(ref, shape[3], shape[4]))


# ------------------------------------------------------------------ integer-exact
LIMIT = 1 << 24


def _int_dense_ref(J, nA, nG, K1, K2):
    nb, nc = J.shape[:2]
    return _blocks(C.dense_joint_ref(J, nA, nG, K1, K2), nb, nc)


@pytest.mark.parametrize("lower", [True, False], ids=["lower", "dense"])
@pytest.mark.parametrize("case", ["nc65", "two_segments"])
def test_tiled_integer_exact(hip_device, case, lower):
    """Small-integer inputs: every product and partial sum is an integer below 2^24 (asserted
    here on the CPU), so fp32 is exact and the result must have the int64 reference's bits.  A
    transposed tile, a wrong mirror or a wrong sample offset cannot pass.  nc65: three tile
    pairs; two_segments: K = 2145 with at most three +-1 per factor column and J in {-1, 0, 1},
    so |T| <= 9 and a Gram entry is at most 81 K < 2^24."""
    from bnn_kfac_amd.variance import kron_covariance_tiled
    rng = np.random.default_rng(7)
    if case == "nc65":
        nA, nG, nb, nc = 5, 4, 3, 65
        J, K1, K2 = C.small_ints(rng, nb, nc, nA * nG), C.small_ints(rng, nA, nA), C.small_ints(rng, nG, nG)
        if lower:
            K1, K2 = np.tril(K1), np.tril(K2)
    else:
        nA, nG, nb, nc = 65, 33, 2, 40
        J = rng.integers(-1, 2, size=(nb, nc, nA * nG)).astype(np.int64)
        K1, K2 = _sparse_signs(rng, nA, lower), _sparse_signs(rng, nG, lower)
        assert nA * nG > 2048 and 81 * nA * nG < LIMIT
    if not lower:
        assert np.abs(np.triu(K1, 1)).max() > 0 and np.abs(np.triu(K2, 1)).max() > 0
    M = J.reshape(-1, nA, nG)
    bound_U = np.abs(K1).T @ np.abs(M)
    bound_T = (bound_U @ np.abs(K2)).reshape(nb, nc, -1)
    assert bound_U.max() < LIMIT and bound_T.max() < LIMIT
    assert (bound_T @ bound_T.transpose(0, 2, 1)).max() < LIMIT
    want = _int_dense_ref(J, nA, nG, K1, K2)
    assert want.dtype == np.int64 and np.abs(want).max() < LIMIT
    assert all(not np.array_equal(w, np.diag(np.diag(w))) for w in want)
    assert not np.array_equal(want[0], want[1])
    got = kron_covariance_tiled([tuple(_dev(hip_device, *(t.astype(np.float32) for t in (J, K1, K2))))],
                                lower=lower)
    assert torch.equal(got.cpu(), torch.from_numpy(want.astype(np.float32)))


@pytest.mark.parametrize("lower", [True, False], ids=["lower", "dense"])
def test_outer_tiled_integer_exact(hip_device, lower):
    """The factored route on small integers at nc = 65: s_j[b] and every Gram entry are exact
    integers, their product is formed in fp64 and stays below 2^24."""
    from bnn_kfac_amd.variance import kron_covariance_outer_tiled
    cols, ones, nG, nb, nc = 4, 1, 3, 3, 65
    rng = np.random.default_rng(11)
    a, D = C.small_ints(rng, nb, cols), C.small_ints(rng, nb, nc, nG)
    K1, K2 = C.small_ints(rng, cols + ones, cols + ones), C.small_ints(rng, nG, nG)
    if lower:
        K1, K2 = np.tril(K1), np.tril(K2)
    bU, bV = C.outer_uv(np.abs(a), ones, np.abs(D), np.abs(K1), np.abs(K2))
    bS, bW = bU @ bU.T, bV @ bV.T
    assert max(bU.max(), bV.max(), bS.max(), bW.max()) < LIMIT
    assert (np.kron(bS, np.ones((nc, nc), dtype=np.int64)) * bW).max() < LIMIT
    want = _blocks(C.outer_joint_ref(a, ones, D, K1, K2), nb, nc)
    assert want.dtype == np.int64 and np.abs(want).max() < LIMIT
    assert all(np.abs(w).max() > 0 for w in want) and not np.array_equal(want[0], want[1])
    got = kron_covariance_outer_tiled(
        [tuple(_dev(hip_device, *(t.astype(np.float32) for t in (a, D, K1, K2))))], lower=lower)
    assert torch.equal(got.cpu(), torch.from_numpy(want.astype(np.float32)))


# ------------------------------------------------------------------ bitwise guarantees
def test_tiled_symmetric_repeatable_nonnegative(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_tiled
    for shape in ((5, 4, 3, 33), (9, 7, 3, 65), (20, 31, 2, 130), (65, 33, 2, 40)):
        terms = [tuple(_dev(hip_device, *C.dense_case(*shape)[:3]))]
        a, b = kron_covariance_tiled(terms), kron_covariance_tiled(terms)
        assert torch.equal(a, a.mT)
        assert torch.equal(a, b)
        assert bool((torch.diagonal(a, dim1=1, dim2=2) >= 0).all())


def test_outer_tiled_symmetric_repeatable_nonnegative(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_outer_tiled
    for shape in ((64, 1, 40, 5, 65), (128, 0, 65, 2, 130), (20, 1, 2100, 2, 40), (130, 1, 130, 70, 33)):
        terms = [tuple(_dev(hip_device, *C.outer_case(*shape)[:4]))]
        a, b = kron_covariance_outer_tiled(terms), kron_covariance_outer_tiled(terms)
        assert torch.equal(a, a.mT)
        assert torch.equal(a, b)
        assert bool((torch.diagonal(a, dim1=1, dim2=2) >= 0).all())


def test_tiled_sample_chunks_do_not_change_a_bit(hip_device):
    from bnn_kfac_amd import _native as N
    from bnn_kfac_amd import variance
    shapes = [(9, 7), (65, 33)]
    nb, nc = 3, 65
    terms = [tuple(_dev(hip_device, *C.dense_case(nA, nG, nb, nc)[:3])) for nA, nG in shapes]
    jobs = [N.CovJob(*j) for j in variance._cov_jobs(terms, True, "test")[1]]
    one, two = (N.kron_cov_tiled_workspace_bytes(jobs, n, nc) for n in (1, 2))
    assert 0 < one < two  # a budget of `one` forces chunks of one sample: three chunks
    whole = variance.kron_covariance_tiled(terms)
    assert torch.equal(variance.kron_covariance_tiled(terms, max_workspace_bytes=one), whole)
    with pytest.raises(ValueError, match=str(one)):
        variance.kron_covariance_tiled(terms, max_workspace_bytes=one - 1)


def test_outer_tiled_sample_chunks_do_not_change_a_bit(hip_device):
    from bnn_kfac_amd import _native as N
    from bnn_kfac_amd import variance
    shapes = [(128, 0, 65), (130, 1, 130)]
    nb, nc = 4, 65
    terms = [tuple(_dev(hip_device, *C.outer_case(c, o, g, nb, nc)[:4])) for c, o, g in shapes]
    jobs = [N.CovOuterJob(*j) for j in variance._cov_outer_jobs(terms, True, "test")[1]]
    one, two = (N.kron_cov_outer_tiled_workspace_bytes(jobs, n, nc) for n in (1, 2))
    assert 0 < one < two  # a budget of `one` forces chunks of one sample: four chunks
    whole = variance.kron_covariance_outer_tiled(terms)
    assert torch.equal(variance.kron_covariance_outer_tiled(terms, max_workspace_bytes=one), whole)
    with pytest.raises(ValueError, match=str(one)):
        variance.kron_covariance_outer_tiled(terms, max_workspace_bytes=one - 1)


def test_tiled_nine_terms_fold_in_groups_of_eight(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_tiled
    shapes = [(3, 2), (5, 4), (9, 7), (65, 33), (12, 4), (20, 31), (33, 3), (8, 8), (6, 5)]
    nb, nc = 3, 33
    terms, ref = [], 0.0
    for nA, nG in shapes:
        *arrays, r = C.dense_case(nA, nG, nb, nc)
        terms.append(tuple(_dev(hip_device, *arrays)))
        ref = ref + _blocks(r, nb, nc)
    _check(kron_covariance_tiled(terms, lower=True).cpu().numpy(), ref)


def test_outer_tiled_nine_terms_fold_in_groups_of_eight(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_outer_tiled
    shapes = [(4, 1, 3), (63, 1, 10), (9, 0, 10), (70, 1, 65), (12, 1, 4), (20, 1, 130), (33, 0, 31),
              (8, 1, 8), (64, 1, 64)]
    nb, nc = 3, 33
    terms, ref = [], 0.0
    for cols, ones, nG in shapes:
        *arrays, r = C.outer_case(cols, ones, nG, nb, nc)
        terms.append(tuple(_dev(hip_device, *arrays)))
        ref = ref + _blocks(r, nb, nc)
    _check(kron_covariance_outer_tiled(terms, lower=True).cpu().numpy(), ref)


def _padded(t, extra, dev):
    """t's values in a NaN-filled tensor `extra` wider in the last dimension, as a view."""
    wide = torch.full(tuple(t.shape[:-1]) + (t.shape[-1] + extra,), float("nan"), device=dev)
    wide[..., :t.shape[-1]] = t
    return wide[..., :t.shape[-1]]


def test_tiled_strides(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_tiled
    nA, nG, nb, nc = shape = (9, 7, 3, 65)
    Jd, K1d, K2d = _dev(hip_device, *C.dense_case(*shape)[:3])
    plain = kron_covariance_tiled([(Jd, K1d, K2d)])
    J_s = _padded(Jd, 5, hip_device)
    assert J_s.stride(1) == nA * nG + 5
    assert torch.equal(kron_covariance_tiled([(J_s, K1d, K2d)]), plain)
    assert torch.equal(kron_covariance_tiled([(Jd, _padded(K1d, 3, hip_device), _padded(K2d, 2, hip_device))]),
                       plain)


def test_outer_tiled_strides(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_outer_tiled
    cols, ones, nG, nb, nc = shape = (64, 1, 40, 5, 65)
    ad, Dd, K1d, K2d = _dev(hip_device, *C.outer_case(*shape)[:4])
    plain = kron_covariance_outer_tiled([(ad, Dd, K1d, K2d)])
    a_s, D_s = _padded(ad, 7, hip_device), _padded(Dd, 5, hip_device)
    assert a_s.stride(0) == cols + 7 and D_s.stride(1) == nG + 5
    assert torch.equal(kron_covariance_outer_tiled([(a_s, Dd, K1d, K2d)]), plain)
    assert torch.equal(kron_covariance_outer_tiled([(ad, D_s, K1d, K2d)]), plain)
    assert torch.equal(kron_covariance_outer_tiled([(a_s, D_s, K1d, K2d)]), plain)


def test_native_calls_refuse_a_wrong_output(hip_device):
    from bnn_kfac_amd import _native as N
    from bnn_kfac_amd import variance
    terms = [tuple(_dev(hip_device, *C.dense_case(5, 4, 3, 33)[:3]))]
    keep, jobs, nb, nc = variance._cov_jobs(terms, True, "test")
    arr = [N.CovJob(*j) for j in jobs]
    with pytest.raises(ValueError):
        N.kron_cov_tiled(arr, nb, nc, torch.empty(nb, nc, nc + 1, device=hip_device)[:, :, :nc])
    with pytest.raises(ValueError):
        N.kron_cov_tiled(arr, nb, nc, torch.empty(nb - 1, nc, nc, device=hip_device))
    with pytest.raises(TypeError):
        N.kron_cov_tiled(arr, nb, nc, torch.empty(nb, nc, nc, device=hip_device, dtype=torch.float64))


def test_mismatched_terms_raise(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_outer_tiled, kron_covariance_tiled
    eye = lambda n: torch.eye(n, device=hip_device)  # noqa: E731
    J = torch.zeros(2, 40, 20, device=hip_device)
    with pytest.raises(ValueError):
        kron_covariance_tiled([(J, eye(5), eye(4)), (J[:1], eye(5), eye(4))])
    with pytest.raises(ValueError):
        kron_covariance_tiled([(J, eye(5), eye(4)), (J[:, :39], eye(5), eye(4))])
    a, D = torch.zeros(2, 5, device=hip_device), torch.zeros(2, 40, 4, device=hip_device)
    with pytest.raises(ValueError):
        kron_covariance_outer_tiled([(a, D, eye(6), eye(4)), (a, D[:, :39], eye(6), eye(4))])


# ------------------------------------------------------------------ the ties
@pytest.mark.parametrize("shape", [s for s in DENSE if s[3] > 32], ids=IDS)
def test_tiled_is_the_joint_calls_diagonal_blocks_bitwise(hip_device, shape):
    """One Gram body, one segmentation, one reduce order: block b of the tiled call has the
    bits of block (b, b) of the joint call."""
    from bnn_kfac_amd.variance import kron_covariance_joint, kron_covariance_tiled, marginal_blocks
    terms = [tuple(_dev(hip_device, *C.dense_case(*shape)[:3]))]
    assert torch.equal(kron_covariance_tiled(terms), marginal_blocks(kron_covariance_joint(terms)))


def test_tiled_two_jobs_accumulated_is_the_joint_calls_diagonal_blocks_bitwise(hip_device):
    """The same with two jobs in a call and a second, accumulated group (nine terms)."""
    from bnn_kfac_amd.variance import kron_covariance_joint, kron_covariance_tiled, marginal_blocks
    shapes = [(3, 2), (5, 4), (9, 7), (65, 33), (12, 4), (20, 31), (33, 3), (8, 8), (6, 5)]
    terms = [tuple(_dev(hip_device, *C.dense_case(nA, nG, 3, 33)[:3])) for nA, nG in shapes]
    assert torch.equal(kron_covariance_tiled(terms), marginal_blocks(kron_covariance_joint(terms)))


@pytest.mark.parametrize("shape", [(4, 1, 3, 1, 33), (63, 1, 10, 3, 64), (64, 1, 40, 5, 65),
                                   (128, 0, 65, 2, 130)], ids=IDS)
def test_outer_tiled_agrees_with_dense_tiled_on_outer_rows(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance_outer_tiled, kron_covariance_tiled
    a, D, K1, K2, _ = C.outer_case(*shape)
    ad, Dd, K1d, K2d, Jd = _dev(hip_device, a, D, K1, K2, C.outer_rows(a, shape[1], D))
    _close(kron_covariance_outer_tiled([(ad, Dd, K1d, K2d)]).cpu().numpy(),
           kron_covariance_tiled([(Jd, K1d, K2d)]).cpu().numpy())


@pytest.mark.parametrize("shape", [(33, 31, 2, 32), (27, 6, 4, 3)], ids=IDS)
def test_tiled_agrees_with_the_capped_call(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance, kron_covariance_tiled
    terms = [tuple(_dev(hip_device, *C.dense_case(*shape)[:3]))]
    _close(kron_covariance_tiled(terms).cpu().numpy(), kron_covariance(terms).cpu().numpy())


@pytest.mark.parametrize("shape", [(63, 1, 10, 7, 10), (64, 1, 40, 3, 32), (130, 1, 130, 70, 2)], ids=IDS)
def test_outer_tiled_agrees_with_the_capped_call(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance_outer, kron_covariance_outer_tiled
    terms = [tuple(_dev(hip_device, *C.outer_case(*shape)[:4]))]
    _close(kron_covariance_outer_tiled(terms).cpu().numpy(), kron_covariance_outer(terms).cpu().numpy())
