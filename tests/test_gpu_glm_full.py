"""GPU: the GLM predictive with per-entry eigenbasis weights -- kfac_kron_cov_full and
kfac_kron_cov_outer_full (variance.kron_covariance_full / kron_covariance_outer_full) against
fp64 numpy on the same fp32 inputs, against the rank-one sweep calls, against each other,
their bitwise guarantees, one integer-exact case per route, and variance.glm_predictive_efb /
glm_predictive_efb_sweep end to end against an fp64 CPU recompute and against EFB.sample.

Kernel tolerance (test_gpu_glm_sweep.py's): rtol 1e-5, atol 1e-5 * max|ref[t]| per grid point;
test_glm_full_host.py shows a plain fp32 evaluation stays within a third of it.  Two fp32
device routes on one quantity: 2e-5 * max.  End to end: 1e-4 * max|cov[b]| per sample."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

import glm_full_cases as C
import glm_sweep_cases as S

pytestmark = pytest.mark.gpu

IDS = lambda s: "x".join(map(str, s))  # noqa: E731
OUTER3 = [(63, 1, 10, 3, 10), (130, 1, 130, 70, 2), (300, 0, 257, 3, 4)]
DENSE3 = [(64, 10, 3, 10), (33, 65, 2, 5), (26, 5, 3, 32)]


def _dev(dev, *arrays):
    return [torch.from_numpy(np.array(t)).to(dev) for t in arrays]  # (a copy: the cached case stays read-only)


def _check(got, ref, rtol=1e-5, scale=1e-5):
    """Per grid point: rtol, atol = scale * max|ref[t]|."""
    assert got.shape == ref.shape
    worst = max(float(np.abs(got[t] - ref[t]).max() / np.abs(ref[t]).max()) for t in range(ref.shape[0]))
    print("max err / max|ref| =", worst)
    for t in range(ref.shape[0]):
        np.testing.assert_allclose(got[t], ref[t], rtol=rtol, atol=scale * np.abs(ref[t]).max())


def _close(got, want, scale=2e-5):
    """Two fp32 device routes: atol = scale * max|want[t]| per grid point."""
    got, want = got.cpu().numpy(), want.cpu().numpy()
    assert got.shape == want.shape
    for t in range(want.shape[0]):
        print("max diff / max =", float(np.abs(got[t] - want[t]).max() / np.abs(want[t]).max()))
        np.testing.assert_allclose(got[t], want[t], rtol=0, atol=scale * np.abs(want[t]).max())


def _outer_terms(dev, shape, nt, rows=None):
    a, D, VA, VG, W, ref = C.outer_case(*shape)
    rows = slice(0, nt) if rows is None else rows
    return [tuple(_dev(dev, a, D, VA, VG, W[rows]))], ref[rows]


def _dense_terms(dev, shape, nt, rows=None):
    J, VA, VG, W, ref = C.dense_case(*shape)
    rows = slice(0, nt) if rows is None else rows
    return [tuple(_dev(dev, J, VA, VG, W[rows]))], ref[rows]


def _routes():
    from bnn_kfac_amd.variance import kron_covariance_full, kron_covariance_outer_full
    return {"outer": (kron_covariance_outer_full, _outer_terms, OUTER3),
            "dense": (kron_covariance_full, _dense_terms, DENSE3)}


# ------------------------------------------------------------------ 1: against fp64
@pytest.mark.parametrize("nt", C.NTS)
@pytest.mark.parametrize("shape", C.OUTER_SHAPES, ids=IDS)
def test_outer_full_matches_fp64(hip_device, shape, nt):
    from bnn_kfac_amd.variance import kron_covariance_outer_full
    terms, ref = _outer_terms(hip_device, shape, nt)
    got = kron_covariance_outer_full(terms)
    assert got.shape == (nt, shape[3], shape[4], shape[4]) and got.dtype == torch.float32
    _check(got.cpu().numpy(), ref)


@pytest.mark.parametrize("nt", C.NTS)
@pytest.mark.parametrize("shape", C.DENSE_SHAPES, ids=IDS)
def test_dense_full_matches_fp64(hip_device, shape, nt):
    from bnn_kfac_amd.variance import kron_covariance_full
    terms, ref = _dense_terms(hip_device, shape, nt)
    got = kron_covariance_full(terms)
    assert got.shape == (nt, shape[2], shape[3], shape[3]) and got.dtype == torch.float32
    _check(got.cpu().numpy(), ref)


def test_a_single_weight_matrix_may_be_two_dimensional(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_full, kron_covariance_outer_full
    (a, D, VA, VG, W), = _outer_terms(hip_device, (63, 1, 10, 3, 10), 1)[0]
    assert torch.equal(kron_covariance_outer_full([(a, D, VA, VG, W[0])]), kron_covariance_outer_full([(a, D, VA, VG, W)]))
    (J, VA, VG, W), = _dense_terms(hip_device, (64, 10, 3, 10), 1)[0]
    assert torch.equal(kron_covariance_full([(J, VA, VG, W[0])]), kron_covariance_full([(J, VA, VG, W)]))


# ------------------------------------------------------------------ 2: rank-one weights
@pytest.mark.parametrize("shape", [(63, 1, 10, 3, 10), (64, 1, 10, 5, 3), (130, 1, 130, 70, 2)], ids=IDS)
def test_outer_rank_one_weights_agree_with_the_sweep(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance_outer_full, kron_covariance_outer_sweep
    a, D, VA, VG, wA, wG = _dev(hip_device, *S.outer_case(*shape)[:6])
    wA, wG = wA[:5], wG[:5]
    W = wA[:, :, None] * wG[:, None, :]
    _close(kron_covariance_outer_full([(a, D, VA, VG, W)]), kron_covariance_outer_sweep([(a, D, VA, VG, wA, wG)]))


@pytest.mark.parametrize("shape", [(64, 10, 3, 10), (33, 65, 2, 5), (70, 1, 2, 3)], ids=IDS)
def test_dense_rank_one_weights_agree_with_the_sweep(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance_full, kron_covariance_sweep
    J, VA, VG, wA, wG = _dev(hip_device, *S.dense_case(*shape)[:5])
    wA, wG = wA[:5], wG[:5]
    W = wA[:, :, None] * wG[:, None, :]
    _close(kron_covariance_full([(J, VA, VG, W)]), kron_covariance_sweep([(J, VA, VG, wA, wG)]))


# ------------------------------------------------------------------ 3: the two routes
@pytest.mark.parametrize("shape", C.OUTER_SHAPES, ids=IDS)
def test_outer_route_agrees_with_dense_route_on_materialised_rows(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance_full, kron_covariance_outer_full
    a, D, VA, VG, W, ref = C.outer_case(*shape)
    ad, Dd, VAd, VGd, Wd, Jd = _dev(hip_device, a, D, VA, VG, W[:5], C.rows_of(a, shape[1], D))
    outer = kron_covariance_outer_full([(ad, Dd, VAd, VGd, Wd)])
    dense = kron_covariance_full([(Jd, VAd, VGd, Wd)])
    _close(outer, dense)
    _check(dense.cpu().numpy(), ref[:5])


# ------------------------------------------------------------------ 4: bitwise properties
@pytest.mark.parametrize("route", ["outer", "dense"])
def test_slices_repeatable_symmetric(hip_device, route):
    """Two calls give the same bits; every block is bitwise symmetric with a non-negative
    diagonal; slice t of an nt = 5 call has the bits of the nt = 1 call with W[t]."""
    fn, make, shapes = _routes()[route]
    for shape in shapes:
        terms, _ = make(hip_device, shape, 5)
        five = fn(terms)
        assert torch.equal(five, fn(terms))
        assert torch.equal(five, five.mT)
        assert bool((torch.diagonal(five, dim1=2, dim2=3) >= 0).all())
        for t in range(5):
            alone, _ = make(hip_device, shape, 1, rows=slice(t, t + 1))
            assert torch.equal(fn(alone)[0], five[t]), (shape, t)


def _job_bytes(route, shape, n, nt):
    from bnn_kfac_amd import _native as N
    if route == "outer":
        cols, ones, nG, nb, nc = shape
        nA = cols + ones
        job = N.CovOuterFullJob(1, cols, cols, ones, 1, nG, nG, 0, 1, nA, 1, nG, 1, nA * nG)
        return N.kron_cov_outer_full_workspace_bytes([job], n, nc, nt)
    nA, nG, nb, nc = shape
    return N.kron_cov_full_workspace_bytes([N.CovFullJob(1, nA * nG, nA, nG, 1, nA, 1, nG, 1, nA * nG)], n, nc, nt)


@pytest.mark.parametrize("route", ["outer", "dense"])
def test_one_sample_chunks_do_not_change_a_bit(hip_device, route):
    fn, make, shapes = _routes()[route]
    for shape in shapes:
        terms, _ = make(hip_device, shape, 5)
        one, two = _job_bytes(route, shape, 1, 5), _job_bytes(route, shape, 2, 5)
        assert 0 < one < two  # a budget of `one` forces chunks of one sample
        assert torch.equal(fn(terms, max_workspace_bytes=one), fn(terms)), shape
        with pytest.raises(ValueError):
            fn(terms, max_workspace_bytes=one - 1)


@pytest.mark.parametrize("route", ["outer", "dense"])
def test_65_grid_points_go_through_two_calls(hip_device, route):
    fn, make, _ = _routes()[route]
    shape = C.OUTER_SHAPES[0] if route == "outer" else C.DENSE_SHAPES[0]
    order = np.concatenate([np.arange(64), [5]])
    terms, ref = make(hip_device, shape, 65, rows=order)
    got = fn(terms)
    assert got.shape[0] == 65
    _check(got.cpu().numpy(), ref)
    for t in range(65):
        alone, _ = make(hip_device, shape, 1, rows=slice(order[t], order[t] + 1))
        assert torch.equal(fn(alone)[0], got[t]), t


def test_outer_sample_block_unchanged_by_other_samples(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_outer_full
    (a, D, VA, VG, W), = _outer_terms(hip_device, (130, 1, 130, 70, 2), 5)[0]
    whole = kron_covariance_outer_full([(a, D, VA, VG, W)])
    assert whole.shape[1] == 70
    assert torch.equal(kron_covariance_outer_full([(a[:3], D[:3], VA, VG, W)]), whole[:, :3])
    assert torch.equal(kron_covariance_outer_full([(a[66:], D[66:], VA, VG, W)]), whole[:, 66:])


def test_dense_sample_block_unchanged_by_other_samples(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_full
    (J, VA, VG, W), = _dense_terms(hip_device, (64, 10, 3, 10), 5)[0]
    whole = kron_covariance_full([(J, VA, VG, W)])
    assert torch.equal(kron_covariance_full([(J[-1:], VA, VG, W)])[:, 0], whole[:, -1])


def test_nine_terms_fold_in_groups_of_eight(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_full, kron_covariance_outer_full
    nt = 3
    shapes = [(4, 1, 3), (63, 1, 10), (9, 0, 10), (70, 1, 65), (12, 1, 4), (20, 1, 130), (33, 0, 31),
              (8, 1, 8), (64, 1, 64)]
    terms, ref = [], 0.0
    for cols, ones, nG in shapes:
        a, D, VA, VG, W, r = C.outer_case(cols, ones, nG, 3, 4)
        terms.append(tuple(_dev(hip_device, a, D, VA, VG, W[:nt])))
        ref = ref + r[:nt]
    _check(kron_covariance_outer_full(terms).cpu().numpy(), ref)
    dshapes = [(5, 3), (64, 10), (9, 10), (33, 65), (12, 4), (20, 13), (70, 1), (8, 8), (26, 5)]
    terms, ref = [], 0.0
    for nA, nG in dshapes:
        J, VA, VG, W, r = C.dense_case(nA, nG, 3, 4)
        terms.append(tuple(_dev(hip_device, J, VA, VG, W[:nt])))
        ref = ref + r[:nt]
    _check(kron_covariance_full(terms).cpu().numpy(), ref)


def _padded_rows(t, dev, pad=3):
    """The same values with row stride n + pad, from a base an odd number of floats in."""
    n = t.shape[-1]
    lead = t.shape[:-1]
    buf = torch.full((int(np.prod(lead)) * (n + pad) + 1,), float("nan"), device=dev)
    view = buf[1:].view(*lead, n + pad)[..., :n]
    view.copy_(t)
    assert view.data_ptr() == buf.data_ptr() + 4 and view.stride(-2) == n + pad
    return view


def _padded_matrices(W, dev, pad=3):
    """W (nt, nA, nG) with its matrices contiguous blocks nA*nG + pad floats apart."""
    nt, nA, nG = W.shape
    buf = torch.full((nt, nA * nG + pad), float("nan"), device=dev)
    view = buf[:, :nA * nG].view(nt, nA, nG)
    view.copy_(W)
    assert view.stride() == (nA * nG + pad, nG, 1) and view.data_ptr() == buf.data_ptr()
    return view


@pytest.mark.parametrize("shape", OUTER3, ids=IDS)
def test_outer_strided_inputs_bit_equal(hip_device, shape):
    from bnn_kfac_amd.variance import _full_weights, kron_covariance_outer_full
    (a, D, VA, VG, W), = _outer_terms(hip_device, shape, 5)[0]
    plain = kron_covariance_outer_full([(a, D, VA, VG, W)])
    wide = torch.full((a.shape[0], a.shape[1] + 7), float("nan"), device=hip_device)
    wide[:, 2:2 + a.shape[1]] = a
    a_slice = wide[:, 2:2 + a.shape[1]]       # a column slice of a wider tensor: not copied
    Wp = _padded_matrices(W, hip_device)
    assert _full_weights(Wp)[1] == W.shape[1] * W.shape[2] + 3  # ... nor is W: ldW > nA*nG
    for terms in ((a_slice, D, VA, VG, W), (a, D, VA, VG, Wp), (a, _padded_rows(D, hip_device), VA, VG, W),
                  (a_slice, _padded_rows(D, hip_device), _padded_rows(VA, hip_device), _padded_rows(VG, hip_device), Wp)):
        assert torch.equal(kron_covariance_outer_full([terms]), plain)


@pytest.mark.parametrize("shape", DENSE3, ids=IDS)
def test_dense_strided_inputs_bit_equal(hip_device, shape):
    from bnn_kfac_amd.variance import _cov_rows, kron_covariance_full
    (J, VA, VG, W), = _dense_terms(hip_device, shape, 5)[0]
    plain = kron_covariance_full([(J, VA, VG, W)])
    Jp, Wp = _padded_rows(J, hip_device), _padded_matrices(W, hip_device)
    assert _cov_rows(Jp, J.shape[2])[1] == J.shape[2] + 3      # a padded row stride: not copied
    for terms in ((Jp, VA, VG, W), (J, VA, VG, Wp),
                  (Jp, _padded_rows(VA, hip_device), _padded_rows(VG, hip_device), Wp)):
        assert torch.equal(kron_covariance_full([terms]), plain)


def test_accumulate_adds(hip_device):
    from bnn_kfac_amd import _native as N
    nt = 3
    a, D, VA, VG, W, ref = C.outer_case(63, 1, 10, 3, 10)
    ad, Dd, VAd, VGd, Wd = _dev(hip_device, a, D, VA, VG, W[:nt])
    job = N.CovOuterFullJob(ad.data_ptr(), 63, 63, 1, Dd.data_ptr(), 10, 10, 0, VAd.data_ptr(), 64,
                            VGd.data_ptr(), 10, Wd.data_ptr(), 640)
    base = torch.from_numpy(np.array(ref[:nt])).float().to(hip_device) * 0.5
    base = (base + base.mT) / 2
    out = base.clone()
    N.kron_cov_outer_full([job], 3, 10, nt, out, accumulate=True)
    _check(out.cpu().numpy(), ref[:nt] + base.cpu().numpy().astype(np.float64))
    N.kron_cov_outer_full([job], 3, 10, nt, out, accumulate=False)
    _check(out.cpu().numpy(), ref[:nt])

    J, VA, VG, W, ref = C.dense_case(64, 10, 3, 10)
    Jd, VAd, VGd, Wd = _dev(hip_device, J, VA, VG, W[:nt])
    job = N.CovFullJob(Jd.data_ptr(), 640, 64, 10, VAd.data_ptr(), 64, VGd.data_ptr(), 10, Wd.data_ptr(), 640)
    base = torch.from_numpy(np.array(ref[:nt])).float().to(hip_device) * 0.5
    base = (base + base.mT) / 2
    out = base.clone()
    N.kron_cov_full([job], 3, 10, nt, out, accumulate=True)
    _check(out.cpu().numpy(), ref[:nt] + base.cpu().numpy().astype(np.float64))


# ------------------------------------------------------------------ 5: integer-exact
def test_outer_full_integer_exact(hip_device):
    """Small-integer inputs: every term any stage accumulates sums (in absolute value) below
    2^24, so every order of fp32 summation is exact and the whole buffer must equal int64's."""
    from bnn_kfac_amd.variance import kron_covariance_outer_full
    a, D, VA, VG, W, want, bound = C.int_outer_case()
    assert 0 < bound < C.EXACT
    assert (np.abs(VA) > 0).sum(0).max() <= 3 and (np.abs(VG) > 0).sum(0).max() <= 3
    assert set(np.unique(W)) == {0.0, 1.0, 2.0} and not np.array_equal(W[0, :10, :10], W[0, :10, :10].T)
    got = kron_covariance_outer_full([tuple(_dev(hip_device, a, D, VA, VG, W))])
    assert np.abs(want).max() > 0
    assert torch.equal(got.cpu(), torch.from_numpy(want.astype(np.float32)))


def test_dense_full_integer_exact(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_full
    J, VA, VG, W, want, bound = C.int_dense_case()
    assert 0 < bound < C.EXACT
    assert (np.abs(VA) > 0).sum(0).max() <= 3 and (np.abs(VG) > 0).sum(0).max() <= 3
    assert set(np.unique(W)) == {0.0, 1.0, 2.0} and not np.array_equal(W[0, :33, :33], W[0, :33, :33].T)
    got = kron_covariance_full([tuple(_dev(hip_device, J, VA, VG, W))])
    assert np.abs(want).max() > 0
    assert torch.equal(got.cpu(), torch.from_numpy(want.astype(np.float32)))


# ------------------------------------------------------------------ 6: end to end
GRID = [(1e-3, 200.0), (0.04, 200.0), (1.0, 1.0)]


@pytest.fixture
def deterministic_convolutions():
    """torch's vmapped Conv2d weight gradient picks its MIOpen solver per call (see
    test_gpu_glm_factored.py): comparisons of two dense-route calls run in torch's
    deterministic mode."""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = before


def _fit_efb(dev, net, in_shape, classes, kfac_batches, efb_batches):
    """test_gpu_efb.py's procedure: KFAC factors, then EFB on their eigenbases.  Returns
    (net on dev, its fp64 CPU copy, efb)."""
    from bnn_kfac_amd.curvatures import EFB, KFAC
    net64 = copy.deepcopy(net).double()  # (before KFAC hooks the modules)
    net = net.to(dev)
    kfac = KFAC(net)

    def backward():
        x = torch.rand(32, *in_shape, device=dev)
        net.zero_grad()
        nn.functional.cross_entropy(net(x), torch.randint(0, classes, (32,), device=dev)).backward()

    for _ in range(kfac_batches):
        backward()
        kfac.update(batch_size=32)
    factors = {m: [F.clone() for F in v] for m, v in kfac.state.items()}
    efb = EFB(net, factors)
    for _ in range(efb_batches):
        backward()
        efb.update(batch_size=32)
    return net, net64, efb


@pytest.fixture(scope="module")
def fitted(hip_device):
    torch.manual_seed(0)
    net = nn.Sequential(nn.Conv2d(1, 3, 3), nn.ReLU(), nn.Flatten(), nn.Linear(3 * 6 * 6, 5))
    net, net64, efb = _fit_efb(hip_device, net, (1, 8, 8), 5, 2, 3)
    x = torch.rand(5, 1, 8, 8, device=hip_device)
    layers = [net[0], net[3]]
    logits64, rows = S.fp64_rows(net64, [net64[0], net64[3]], x.cpu())
    want = []
    for n, s in GRID:
        cov = 0.0
        for layer, M in zip(layers, rows):
            VA, VG = (v.double().cpu().numpy() for v in efb.eigvecs[layer])
            Wl = 1.0 / (s * efb.state[layer].double().cpu().numpy().T + n)   # (nA, nG)
            Y = np.einsum("ai,bcag,gh->bcih", VA, M, VG)
            cov = cov + np.einsum("ih,bcih,bdih->bcd", Wl, Y, Y)
        want.append(cov)
    return net, efb, x, logits64, want


def _per_sample(got, want, scale, what):
    worst = max(float(np.abs(got[b] - want[b]).max() / np.abs(want[b]).max()) for b in range(want.shape[0]))
    print(what, "max err / max|cov[b]| =", worst)
    for b in range(want.shape[0]):
        np.testing.assert_allclose(got[b], want[b], rtol=0, atol=scale * np.abs(want[b]).max())


@pytest.mark.parametrize("route", ["dense", "factored"])
def test_glm_predictive_efb_end_to_end(hip_device, fitted, deterministic_convolutions, route):
    from bnn_kfac_amd.variance import glm_predictive_efb, glm_predictive_efb_sweep
    net, efb, x, logits64, want = fitted
    efb._inv_state.clear()
    with pytest.raises(AssertionError):
        glm_predictive_efb(efb, x)                     # inv_state must be filled
    sweep = glm_predictive_efb_sweep(efb, x, GRID, chunk=2, jacobians=route)   # needs no invert
    assert not efb.inv_state
    efb.invert(0.04, 200.0)
    logits, cov = glm_predictive_efb(efb, x, chunk=2, jacobians=route)
    assert logits.shape == (5, 5) and cov.shape == (5, 5, 5) and cov.dtype == torch.float32
    assert sweep.shape == (len(GRID), 5, 5, 5) and sweep.dtype == torch.float32
    with torch.no_grad():
        direct = net(x).cpu().numpy()
    np.testing.assert_allclose(logits.cpu().numpy(), direct, rtol=1e-6, atol=1e-6 * np.abs(direct).max())
    np.testing.assert_allclose(logits.cpu().numpy(), logits64, rtol=1e-4, atol=1e-5 * np.abs(logits64).max())
    _per_sample(cov.cpu().numpy(), want[1], 1e-4, f"{route} glm_predictive_efb against fp64:")
    for t, point in enumerate(GRID):
        _per_sample(sweep[t].cpu().numpy(), want[t], 1e-4, f"{route} sweep {point} against fp64:")
    _per_sample(sweep[1].cpu().numpy(), cov.cpu().numpy(), 2e-5, f"{route} sweep against invert + glm_predictive_efb:")
    assert torch.equal(cov, cov.mT)
    # a weight budget of one grid point at a time gives the same covariance
    small = glm_predictive_efb_sweep(efb, x, GRID, chunk=2, jacobians=route, max_weight_bytes=1)
    _close(small, sweep)
    # per-layer lists, and a subset of the layers
    lists = glm_predictive_efb_sweep(efb, x, [([0.04, 0.04], [200.0, 200.0])], jacobians=route)
    _close(lists, sweep[1:2])
    parts = [glm_predictive_efb_sweep(efb, x, GRID, layers=[layer], jacobians=route) for layer in (net[0], net[3])]
    _close(parts[0] + parts[1], sweep)
    with pytest.raises(ValueError):
        glm_predictive_efb(efb, x, jacobians="nope")
    with pytest.raises(ValueError):
        glm_predictive_efb_sweep(efb, x, [])


def test_efb_log_det_sweep_on_the_device_state(hip_device, fitted):
    from bnn_kfac_amd.variance import efb_log_det_sweep
    net, efb, x, _, _ = fitted
    got = efb_log_det_sweep(efb, GRID)
    assert got.shape == (len(GRID),) and got.dtype == torch.float64 and got.device.type == "cuda"
    for t, (n, s) in enumerate(GRID):
        want = sum(float(np.log(s * lam.double().cpu().numpy() + n).sum()) for lam in efb.state.values())
        np.testing.assert_allclose(float(got[t]), want, rtol=1e-12)


# ------------------------------------------------------------------ 7: EFB.sample's covariance
def _unit_randn(monkeypatch, k):
    def fake(*size, device=None, dtype=None, **kwargs):
        z = torch.zeros(*size, device=device, dtype=dtype)
        z.view(-1)[k] = 1
        return z
    monkeypatch.setattr(torch, "randn", fake)


@pytest.mark.parametrize("name", ["linear", "conv"])
@pytest.mark.parametrize("route", ["dense", "factored"])
def test_covariance_is_that_of_efb_sample(hip_device, monkeypatch, name, route):
    """Z = the k-th unit matrix makes EFB.sample return the k-th column of the posterior's
    square root; summing the outer products of J vec(S_k^T) over all nA*nG of them is the
    predictive covariance of the sampler itself."""
    from bnn_kfac_amd.variance import glm_predictive_efb, output_jacobians
    torch.manual_seed(0)
    if name == "linear":
        net, in_shape, classes, count = nn.Sequential(nn.Linear(4, 3)), (4,), 3, 15
    else:
        net, in_shape, classes, count = nn.Sequential(nn.Conv2d(1, 2, 2), nn.Flatten()), (1, 3, 3), 8, 10
    net, _, efb = _fit_efb(hip_device, net, in_shape, classes, 1, 2)
    layer = net[0]
    efb.invert(0.04, 200.0)
    assert efb.inv_state[layer].numel() == count
    x = torch.rand(4, *in_shape, device=hip_device)
    logits, cov = glm_predictive_efb(efb, x, jacobians=route)
    _, (J,) = output_jacobians(net, [layer], x)
    J = J.double().cpu().numpy()                                   # (n, nc, nA*nG)
    want = 0.0
    for k in range(count):
        _unit_randn(monkeypatch, k)
        Sk = efb.sample(layer)                                     # (nG, nA)
        v = J @ Sk.t().double().cpu().numpy().reshape(-1)          # (n, nc)
        want = want + v[:, :, None] * v[:, None, :]
    monkeypatch.undo()
    assert cov.shape == want.shape
    _per_sample(cov.cpu().numpy(), want, 1e-4, f"{name} {route} against EFB.sample:")
