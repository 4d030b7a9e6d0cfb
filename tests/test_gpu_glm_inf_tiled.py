"""GPU: the GLM predictive under the INF posterior above 32 outputs -- kfac_inf_cov_tiled and
kfac_inf_cov_outer_tiled (variance.kron_covariance_inf_tiled / kron_covariance_outer_inf_tiled)
against fp64 numpy on the same fp32 inputs, against each other, against the capped calls at
nc <= 32, their bitwise guarantees (the F = 0 identity with kron_covariance_full_tiled among
them), and whole-buffer integer-exact cases.

Tolerance (glm_inf_tiled_cases.SCALE, from the fp32 stage chain measured on the CPU):
rtol = SCALE, atol = SCALE * max|first term|, for two device routes against each other too."""
import numpy as np
import pytest
import torch

import glm_inf_cases as C
import glm_inf_tiled_cases as T
from test_gpu_glm_inf import IDS, _dev, _padded_rows

pytestmark = pytest.mark.gpu

# shapes with more than one sample, for the chunking tests
OUTER_NB = [s for s in T.OUTER_SHAPES if s[5] > 1]
DENSE_NB = [s for s in T.DENSE_SHAPES if s[4] > 1]


def _check(got, ref, top):
    """rtol = SCALE, atol = SCALE * max|first term|."""
    assert got.shape == ref.shape
    print("max err / max|first term| =", float(np.abs(got - ref).max() / top), "of", T.SCALE)
    np.testing.assert_allclose(got, ref, rtol=T.SCALE, atol=T.SCALE * top)


def _outer_terms(dev, shape):
    *inputs, ref, top = C.outer_case(*shape)
    return [tuple(_dev(dev, *inputs))], ref, top


def _dense_terms(dev, shape):
    *inputs, ref, top = C.dense_case(*shape)
    return [tuple(_dev(dev, *inputs))], ref, top


def _routes():
    from bnn_kfac_amd.variance import kron_covariance_inf_tiled, kron_covariance_outer_inf_tiled
    return {"outer": (kron_covariance_outer_inf_tiled, _outer_terms, T.OUTER_SHAPES, OUTER_NB),
            "dense": (kron_covariance_inf_tiled, _dense_terms, T.DENSE_SHAPES, DENSE_NB)}


# ------------------------------------------------------------------ 1: against fp64
@pytest.mark.parametrize("shape", T.OUTER_SHAPES, ids=IDS)
def test_outer_inf_tiled_matches_fp64(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance_outer_inf_tiled
    terms, ref, top = _outer_terms(hip_device, shape)
    got = kron_covariance_outer_inf_tiled(terms)
    assert got.shape == (shape[5], shape[6], shape[6]) and got.dtype == torch.float32
    _check(got.cpu().numpy(), ref, top)


@pytest.mark.parametrize("shape", T.DENSE_SHAPES, ids=IDS)
def test_dense_inf_tiled_matches_fp64(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance_inf_tiled
    terms, ref, top = _dense_terms(hip_device, shape)
    got = kron_covariance_inf_tiled(terms)
    assert got.shape == (shape[4], shape[5], shape[5]) and got.dtype == torch.float32
    _check(got.cpu().numpy(), ref, top)


# ------------------------------------------------------------------ 2: the two routes
@pytest.mark.parametrize("shape", T.OUTER_SHAPES, ids=IDS)
def test_outer_route_agrees_with_dense_route_on_materialised_rows(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance_inf_tiled, kron_covariance_outer_inf_tiled
    a, D, UA, UG, W, F, ref, top = C.outer_case(*shape)
    ad, Dd, UAd, UGd, Wd, Fd, Jd = _dev(hip_device, a, D, UA, UG, W, F, C.rows_of(a, shape[1], D))
    outer = kron_covariance_outer_inf_tiled([(ad, Dd, UAd, UGd, Wd, Fd)])
    dense = kron_covariance_inf_tiled([(Jd, UAd, UGd, Wd, Fd)])
    _check(outer.cpu().numpy(), dense.cpu().numpy().astype(np.float64), top)
    _check(dense.cpu().numpy(), ref, top)


# ------------------------------------------------------------------ 3: against the capped calls
@pytest.mark.parametrize("shape", T.CAPPED_OUTER, ids=IDS)
def test_outer_tiled_agrees_with_the_capped_call_up_to_32_outputs(hip_device, shape):
    """nc <= 32 is one tile pair; the segmentation differs (2048 against 256): fp32 rounding."""
    from bnn_kfac_amd.variance import kron_covariance_outer_inf, kron_covariance_outer_inf_tiled
    terms, ref, top = _outer_terms(hip_device, shape)
    tiled = kron_covariance_outer_inf_tiled(terms)
    _check(tiled.cpu().numpy(), kron_covariance_outer_inf(terms).cpu().numpy().astype(np.float64), top)
    _check(tiled.cpu().numpy(), ref, top)
    assert torch.equal(tiled, tiled.mT)


@pytest.mark.parametrize("shape", T.CAPPED_DENSE, ids=IDS)
def test_dense_tiled_agrees_with_the_capped_call_up_to_32_outputs(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance_inf, kron_covariance_inf_tiled
    terms, ref, top = _dense_terms(hip_device, shape)
    tiled = kron_covariance_inf_tiled(terms)
    _check(tiled.cpu().numpy(), kron_covariance_inf(terms).cpu().numpy().astype(np.float64), top)
    _check(tiled.cpu().numpy(), ref, top)
    assert torch.equal(tiled, tiled.mT)


# ------------------------------------------------------------------ 4: bitwise properties
@pytest.mark.parametrize("route", ["outer", "dense"])
def test_repeatable_and_bitwise_symmetric(hip_device, route):
    fn, make, shapes, _ = _routes()[route]
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
        return N.inf_cov_outer_tiled_workspace_bytes([job], n, nc)
    nA, nG, ra, rg, nb, nc = shape
    job = N.InfCovJob(1, nA * nG, nA, nG, 1, ra, ra, 1, rg, rg, 1, nA * nG, 1, ra * rg)
    return N.inf_cov_tiled_workspace_bytes([job], n, nc)


@pytest.mark.parametrize("route", ["outer", "dense"])
def test_one_sample_chunks_do_not_change_a_bit(hip_device, route):
    fn, make, _, shapes = _routes()[route]
    assert len(shapes) >= 3
    for shape in shapes:
        terms, _, _ = make(hip_device, shape)
        one, two = _job_bytes(route, shape, 1), _job_bytes(route, shape, 2)
        assert 0 < one < two  # a budget of `one` forces chunks of one sample
        assert torch.equal(fn(terms, max_workspace_bytes=one), fn(terms)), shape
        with pytest.raises(ValueError):
            fn(terms, max_workspace_bytes=one - 1)


def test_outer_sample_block_unchanged_by_other_samples(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_outer_inf_tiled
    (a, D, *ops), = _outer_terms(hip_device, (63, 1, 10, 5, 3, 3, 65))[0]
    whole = kron_covariance_outer_inf_tiled([(a, D, *ops)])
    assert whole.shape[0] == 3
    assert torch.equal(kron_covariance_outer_inf_tiled([(a[:1], D[:1], *ops)]), whole[:1])
    assert torch.equal(kron_covariance_outer_inf_tiled([(a[1:], D[1:], *ops)]), whole[1:])
    assert torch.equal(kron_covariance_outer_inf_tiled([(a[[2, 0]], D[[2, 0]], *ops)]), whole[[2, 0]])


def test_dense_sample_block_unchanged_by_other_samples(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_inf_tiled
    (J, *ops), = _dense_terms(hip_device, (33, 65, 5, 7, 2, 100))[0]
    whole = kron_covariance_inf_tiled([(J, *ops)])
    assert torch.equal(kron_covariance_inf_tiled([(J[-1:], *ops)])[0], whole[-1])
    assert torch.equal(kron_covariance_inf_tiled([(J[:1], *ops)]), whole[:1])
    assert torch.equal(kron_covariance_inf_tiled([(J[[1, 0]], *ops)]), whole[[1, 0]])


@pytest.mark.parametrize("shape", [T.OUTER_SHAPES[1], T.OUTER_SHAPES[3], T.OUTER_SHAPES[4]], ids=IDS)
def test_outer_strided_inputs_bit_equal(hip_device, shape):
    """NaN-padded strides of a, D, UA, UG and F: term 1 reads D at its own leading dimension."""
    from bnn_kfac_amd.variance import _cov_rows, kron_covariance_outer_inf_tiled
    (a, D, UA, UG, W, F), = _outer_terms(hip_device, shape)[0]
    plain = kron_covariance_outer_inf_tiled([(a, D, UA, UG, W, F)])
    wide = torch.full((a.shape[0], a.shape[1] + 7), float("nan"), device=hip_device)
    wide[:, 2:2 + a.shape[1]] = a
    a_slice = wide[:, 2:2 + a.shape[1]]       # a column slice of a wider tensor: not copied
    Dp, UAp, UGp, Fp = (_padded_rows(t, hip_device) for t in (D, UA, UG, F))
    assert _cov_rows(Dp, D.shape[2])[1] == D.shape[2] + 3      # a padded row stride: not copied
    for terms in ((a_slice, D, UA, UG, W, F), (a, Dp, UA, UG, W, F), (a, D, UAp, UG, W, F),
                  (a_slice, Dp, UAp, UGp, W, Fp)):
        assert torch.equal(kron_covariance_outer_inf_tiled([terms]), plain)


@pytest.mark.parametrize("shape", [T.DENSE_SHAPES[1], T.DENSE_SHAPES[2], T.DENSE_SHAPES[3]], ids=IDS)
def test_dense_strided_inputs_bit_equal(hip_device, shape):
    """NaN-padded strides of J, UA, UG and F: term 1 reads J at its own leading dimension."""
    from bnn_kfac_amd.variance import _cov_rows, kron_covariance_inf_tiled
    (J, UA, UG, W, F), = _dense_terms(hip_device, shape)[0]
    plain = kron_covariance_inf_tiled([(J, UA, UG, W, F)])
    Jp, UAp, UGp, Fp = (_padded_rows(t, hip_device) for t in (J, UA, UG, F))
    assert _cov_rows(Jp, J.shape[2])[1] == J.shape[2] + 3      # a padded row stride: not copied
    for terms in ((Jp, UA, UG, W, F), (J, UAp, UG, W, F), (Jp, UAp, UGp, W, Fp)):
        assert torch.equal(kron_covariance_inf_tiled([terms]), plain)


@pytest.mark.parametrize("shape", [T.DENSE_SHAPES[0], T.DENSE_SHAPES[2], T.DENSE_SHAPES[3]], ids=IDS)
def test_zero_F_gives_the_bits_of_the_weighted_tiled_call(hip_device, shape):
    """F = 0: the second term is exactly 0 and the first is kfac_kron_cov_full_tiled's tile body,
    segmentation and reduce order on the same rows (VA, VG identities: x * 1 is exact)."""
    from bnn_kfac_amd.variance import kron_covariance_full_tiled, kron_covariance_inf_tiled
    (J, UA, UG, W, F), = _dense_terms(hip_device, shape)[0]
    nA, nG = shape[0], shape[1]
    got = kron_covariance_inf_tiled([(J, UA, UG, W, torch.zeros_like(F))])
    eye = lambda n: torch.eye(n, device=hip_device)  # noqa: E731
    want = kron_covariance_full_tiled([(J, eye(nA), eye(nG), W)])
    assert want.shape == (1,) + tuple(got.shape) and float(want.abs().max()) > 0
    assert torch.equal(got, want[0])
    # and F matters: the real F moves the result
    assert not torch.equal(got, kron_covariance_inf_tiled([(J, UA, UG, W, F)]))


def test_nine_terms_fold_in_groups_of_eight(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_inf_tiled, kron_covariance_outer_inf_tiled
    shapes = [(4, 1, 3, 2, 1), (63, 1, 10, 5, 3), (9, 0, 10, 9, 2), (70, 1, 65, 3, 33), (12, 1, 4, 4, 4),
              (20, 1, 130, 7, 2), (33, 0, 31, 1, 31), (8, 1, 8, 2, 2), (64, 1, 64, 6, 6)]
    terms, ref, top = [], 0.0, 0.0
    for dims in shapes:
        *inputs, r, t = C.outer_case(*dims, 2, 33)
        terms.append(tuple(_dev(hip_device, *inputs)))
        ref, top = ref + r, top + t
    got = kron_covariance_outer_inf_tiled(terms)
    _check(got.cpu().numpy(), ref, top)
    assert torch.equal(got, got.mT)
    dshapes = [(5, 3, 2, 2), (64, 10, 8, 4), (9, 10, 9, 2), (33, 65, 5, 7), (12, 4, 4, 4), (20, 13, 7, 2),
               (70, 1, 9, 1), (8, 8, 2, 2), (26, 5, 26, 5)]
    terms, ref, top = [], 0.0, 0.0
    for dims in dshapes:
        *inputs, r, t = C.dense_case(*dims, 2, 33)
        terms.append(tuple(_dev(hip_device, *inputs)))
        ref, top = ref + r, top + t
    got = kron_covariance_inf_tiled(terms)
    _check(got.cpu().numpy(), ref, top)
    assert torch.equal(got, got.mT)


def test_accumulate_adds(hip_device):
    from bnn_kfac_amd import _native as N
    a, D, UA, UG, W, F, ref, top = C.outer_case(63, 1, 10, 5, 3, 3, 65)
    ad, Dd, UAd, UGd, Wd, Fd = _dev(hip_device, a, D, UA, UG, W, F)
    job = N.InfCovOuterJob(ad.data_ptr(), 63, 63, 1, Dd.data_ptr(), 10, 10, 0, UAd.data_ptr(), 5, 5,
                           UGd.data_ptr(), 3, 3, Wd.data_ptr(), 640, Fd.data_ptr(), 15)
    base = torch.from_numpy(np.array(ref)).float().to(hip_device) * 0.5
    base = (base + base.mT) / 2
    out = base.clone()
    N.inf_cov_outer_tiled([job], 3, 65, out, accumulate=True)
    _check(out.cpu().numpy(), ref + base.cpu().numpy().astype(np.float64), top)
    N.inf_cov_outer_tiled([job], 3, 65, out, accumulate=False)
    _check(out.cpu().numpy(), ref, top)
    with pytest.raises(ValueError):        # the tiled calls write contiguous blocks
        N.inf_cov_outer_tiled([job], 3, 65, torch.empty(3, 65, 66, device=hip_device)[:, :, :65])

    J, UA, UG, W, F, ref, top = C.dense_case(64, 10, 8, 4, 2, 65)
    Jd, UAd, UGd, Wd, Fd = _dev(hip_device, J, UA, UG, W, F)
    job = N.InfCovJob(Jd.data_ptr(), 640, 64, 10, UAd.data_ptr(), 8, 8, UGd.data_ptr(), 4, 4, Wd.data_ptr(), 640,
                      Fd.data_ptr(), 32)
    base = torch.from_numpy(np.array(ref)).float().to(hip_device) * 0.5
    base = (base + base.mT) / 2
    out = base.clone()
    N.inf_cov_tiled([job], 2, 65, out, accumulate=True)
    _check(out.cpu().numpy(), ref + base.cpu().numpy().astype(np.float64), top)
    N.inf_cov_tiled([job], 2, 65, out, accumulate=False)
    _check(out.cpu().numpy(), ref, top)


# ------------------------------------------------------------------ 5: integer-exact
@pytest.mark.parametrize("kw", T.INT_OUTER, ids=lambda kw: f"nb{kw['nb']}nc{kw['nc']}")
def test_outer_inf_tiled_integer_exact(hip_device, kw):
    """Small-integer inputs: every term any stage accumulates sums (in absolute value) below
    2^24, so every order of fp32 summation is exact and the whole buffer must equal int64's."""
    from bnn_kfac_amd.variance import kron_covariance_outer_inf_tiled
    *inputs, want, bound = C.int_outer_case(**kw)
    assert 0 < bound <= C.EXACT and np.abs(want).max() > 0
    got = kron_covariance_outer_inf_tiled([tuple(_dev(hip_device, *inputs))])
    assert torch.equal(got.cpu(), torch.from_numpy(want.astype(np.float32)))


@pytest.mark.parametrize("kw", T.INT_DENSE, ids=lambda kw: f"nb{kw['nb']}nc{kw['nc']}")
def test_dense_inf_tiled_integer_exact(hip_device, kw):
    """K = 33 * 65 = 2145 crosses a Gram segment: the segment sum is exact too."""
    from bnn_kfac_amd.variance import kron_covariance_inf_tiled
    *inputs, want, bound = C.int_dense_case(**kw)
    assert inputs[0].shape[2] > 2048 and 0 < bound <= 67123 and np.abs(want).max() > 0
    got = kron_covariance_inf_tiled([tuple(_dev(hip_device, *inputs))])
    assert torch.equal(got.cpu(), torch.from_numpy(want.astype(np.float32)))
