"""GPU: the GLM predictive over a damping grid -- kfac_kron_cov_sweep and
kfac_kron_cov_outer_sweep (variance.kron_covariance_sweep / kron_covariance_outer_sweep)
against fp64 numpy on the same fp32 inputs, their bitwise guarantees, their agreement with
the existing kernels given K = V diag(sqrt(w)), and variance.glm_predictive_sweep /
log_det_sweep end to end against the fp64 CPU recompute and against invert + glm_predictive.

Kernel tolerance: the covariance kernels', rtol 1e-5, atol 1e-5 * max|ref|, per grid point.
Two fp32 kernels on one quantity: 2e-5 * max.  End to end: 1e-4 * max|cov[b]| per sample
(the tolerance for predictive variances; test_glm_sweep_host.py confirms on the CPU that
the eigen route in fp32 stays two orders inside it)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import glm_sweep_cases as C

pytestmark = pytest.mark.gpu

# (cols, has_ones, nG, nb, nc)
OUTER_SHAPES = [(4, 1, 3, 1, 1),
                (63, 1, 10, 3, 10),      # nA = 64 ends a tile
                (64, 1, 10, 5, 3),       # the ones column alone in tile 2
                (20, 1, 31, 2, 32),      # nc at the cap
                (130, 1, 130, 70, 2)]    # two sample tiles, three column tiles, nG > 128
# (nA, nG, nb, nc)
DENSE_SHAPES = [(5, 3, 2, 4),
                (64, 10, 3, 10),
                (33, 65, 2, 5),          # 2145 elements: segment edges inside an a-row, nG % 4 != 0
                (70, 1, 2, 3),           # nG = 1
                (26, 5, 3, 32)]          # nc at the cap
# 5: one more than the Gram kernel's group of 4 grid points; 17: one more than the row
# norm's group of 16
NTS = [1, 3, 5, 17, 64]
IDS = lambda s: "x".join(map(str, s))  # noqa: E731


def _dev(dev, *arrays):
    return [torch.from_numpy(np.array(t)).to(dev) for t in arrays]  # (a copy: the cached case stays read-only)


def _check(got, ref, rtol=1e-5, scale=1e-5):
    """Per grid point: rtol, atol = scale * max|ref[t]|."""
    assert got.shape == ref.shape
    worst = 0.0
    for t in range(ref.shape[0]):
        worst = max(worst, float(np.abs(got[t] - ref[t]).max() / np.abs(ref[t]).max()))
    print("max err / max|ref| =", worst)
    for t in range(ref.shape[0]):
        np.testing.assert_allclose(got[t], ref[t], rtol=rtol, atol=scale * np.abs(ref[t]).max())


def _outer_terms(dev, shape, nt, rows=None):
    a, D, VA, VG, wA, wG, ref = C.outer_case(*shape)
    rows = slice(0, nt) if rows is None else rows
    return [tuple(_dev(dev, a, D, VA, VG, wA[rows], wG[rows]))], ref[rows]


def _dense_terms(dev, shape, nt, rows=None):
    J, VA, VG, wA, wG, ref = C.dense_case(*shape)
    rows = slice(0, nt) if rows is None else rows
    return [tuple(_dev(dev, J, VA, VG, wA[rows], wG[rows]))], ref[rows]


def _routes():
    from bnn_kfac_amd.variance import kron_covariance_outer_sweep, kron_covariance_sweep
    return {"outer": (kron_covariance_outer_sweep, _outer_terms, OUTER_SHAPES),
            "dense": (kron_covariance_sweep, _dense_terms, DENSE_SHAPES)}


@pytest.mark.parametrize("nt", NTS)
@pytest.mark.parametrize("shape", OUTER_SHAPES, ids=IDS)
def test_outer_sweep_matches_fp64(hip_device, shape, nt):
    from bnn_kfac_amd.variance import kron_covariance_outer_sweep
    terms, ref = _outer_terms(hip_device, shape, nt)
    got = kron_covariance_outer_sweep(terms)
    assert got.shape == (nt, shape[3], shape[4], shape[4]) and got.dtype == torch.float32
    _check(got.cpu().numpy(), ref)


@pytest.mark.parametrize("nt", NTS)
@pytest.mark.parametrize("shape", DENSE_SHAPES, ids=IDS)
def test_dense_sweep_matches_fp64(hip_device, shape, nt):
    from bnn_kfac_amd.variance import kron_covariance_sweep
    terms, ref = _dense_terms(hip_device, shape, nt)
    got = kron_covariance_sweep(terms)
    assert got.shape == (nt, shape[2], shape[3], shape[3]) and got.dtype == torch.float32
    _check(got.cpu().numpy(), ref)


@pytest.mark.parametrize("shape", OUTER_SHAPES, ids=IDS)
def test_outer_unit_weights_equal_the_plain_kernel(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance_outer, kron_covariance_outer_sweep
    terms, ref = _outer_terms(hip_device, shape, 3)
    a, D, VA, VG, wA, wG = terms[0]
    assert bool((wA[C.ONES_ROW] == 1).all()) and bool((wG[C.ONES_ROW] == 1).all())
    got = kron_covariance_outer_sweep(terms)[C.ONES_ROW].cpu().numpy()
    plain = kron_covariance_outer([(a, D, VA, VG)], lower=False).cpu().numpy()
    _check(got[None], ref[C.ONES_ROW][None])
    _check(got[None], plain[None])


@pytest.mark.parametrize("shape", DENSE_SHAPES, ids=IDS)
def test_dense_unit_weights_equal_the_plain_kernel(hip_device, shape):
    from bnn_kfac_amd.variance import kron_covariance, kron_covariance_sweep
    terms, ref = _dense_terms(hip_device, shape, 3)
    J, VA, VG, wA, wG = terms[0]
    got = kron_covariance_sweep(terms)[C.ONES_ROW].cpu().numpy()
    plain = kron_covariance([(J, VA, VG)], lower=False).cpu().numpy()
    _check(got[None], ref[C.ONES_ROW][None])
    _check(got[None], plain[None])


def _strided(t, dev):
    """The same values with row stride n + 3, from a base an odd number of floats in."""
    n = t.shape[-1]
    lead = t.shape[:-1]
    rows = int(np.prod(lead)) if lead else 1
    buf = torch.full((rows * (n + 3) + 1,), float("nan"), device=dev)
    view = buf[1:].view(*lead, n + 3)[..., :n]
    view.copy_(t)
    assert view.data_ptr() == buf.data_ptr() + 4 and (t.dim() < 2 or view.stride(-2) == n + 3)
    return view


@pytest.mark.parametrize("route", ["outer", "dense"])
def test_strided_inputs_bit_equal(hip_device, route):
    fn, make, shapes = _routes()[route]
    shape = (130, 1, 130, 70, 2) if route == "outer" else (33, 65, 2, 5)
    terms, ref = make(hip_device, shape, 5)
    plain = fn(terms)
    _check(plain.cpu().numpy(), ref)
    every = tuple(_strided(t, hip_device) for t in terms[0])
    assert torch.equal(fn([every]), plain)
    for i in range(len(terms[0])):  # each operand strided alone
        one = list(terms[0])
        one[i] = every[i]
        assert torch.equal(fn([tuple(one)]), plain), i


@pytest.mark.parametrize("route", ["outer", "dense"])
def test_slices_repeatable_symmetric(hip_device, route):
    """Slice t of an nt = 5 call has the bits of the nt = 1 call with row t's weights; two
    calls give the same bits; every block is bitwise symmetric with a non-negative diagonal."""
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
    # ... and of a 64-point call, in another group of grid points
    terms, _ = make(hip_device, shapes[1], 64)
    full = fn(terms)
    for t in (4, 21, 63):
        alone, _ = make(hip_device, shapes[1], 1, rows=slice(t, t + 1))
        assert torch.equal(fn(alone)[0], full[t]), t


@pytest.mark.parametrize("route", ["outer", "dense"])
def test_sample_block_depends_on_that_sample_only(hip_device, route):
    fn, make, shapes = _routes()[route]
    shape = (130, 1, 130, 70, 2) if route == "outer" else (64, 10, 3, 10)
    terms, _ = make(hip_device, shape, 3)
    whole = fn(terms)
    t0 = terms[0]
    last = tuple(t[-1:] if i < (2 if route == "outer" else 1) else t for i, t in enumerate(t0))
    assert torch.equal(fn([last])[:, 0], whole[:, -1])


def test_sample_chunks_do_not_change_a_bit(hip_device):
    from bnn_kfac_amd import _native as N
    from bnn_kfac_amd.variance import kron_covariance_outer_sweep, kron_covariance_sweep
    nt = 3
    shapes = [(128, 0, 65), (130, 1, 130)]
    terms = [tuple(_dev(hip_device, *(lambda c: c[:4] + (c[4][:nt], c[5][:nt]))(C.outer_case(c_, o, g, 4, 5))))
             for c_, o, g in shapes]
    jobs = [N.CovOuterSweepJob(1, c_, c_, o, 1, g, g, 0, 1, c_ + o, 1, g, 1, c_ + o, 1, g) for c_, o, g in shapes]
    one, two = (N.kron_cov_outer_sweep_workspace_bytes(jobs, n, 5, nt) for n in (1, 2))
    assert 0 < one < two  # a budget of `one` forces chunks of one sample: four chunks
    whole = kron_covariance_outer_sweep(terms)
    assert torch.equal(kron_covariance_outer_sweep(terms, max_workspace_bytes=one), whole)
    with pytest.raises(ValueError):
        kron_covariance_outer_sweep(terms, max_workspace_bytes=one - 1)

    dshapes = [(33, 65), (64, 10)]
    dterms = [tuple(_dev(hip_device, *(lambda c: c[:3] + (c[3][:nt], c[4][:nt]))(C.dense_case(a, g, 4, 5))))
              for a, g in dshapes]
    djobs = [N.CovSweepJob(1, a * g, a, g, 1, a, 1, g, 1, a, 1, g) for a, g in dshapes]
    one, two = (N.kron_cov_sweep_workspace_bytes(djobs, n, 5, nt) for n in (1, 2))
    assert 0 < one < two
    whole = kron_covariance_sweep(dterms)
    assert torch.equal(kron_covariance_sweep(dterms, max_workspace_bytes=one), whole)
    with pytest.raises(ValueError):
        kron_covariance_sweep(dterms, max_workspace_bytes=one - 1)


def test_nine_terms_fold_in_groups_of_eight(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_outer_sweep, kron_covariance_sweep
    nt = 3
    shapes = [(4, 1, 3), (63, 1, 10), (9, 0, 10), (70, 1, 65), (12, 1, 4), (20, 1, 130), (33, 0, 31),
              (8, 1, 8), (64, 1, 64)]
    terms, ref = [], 0.0
    for cols, ones, nG in shapes:
        a, D, VA, VG, wA, wG, r = C.outer_case(cols, ones, nG, 3, 4)
        terms.append(tuple(_dev(hip_device, a, D, VA, VG, wA[:nt], wG[:nt])))
        ref = ref + r[:nt]
    _check(kron_covariance_outer_sweep(terms).cpu().numpy(), ref)
    dshapes = [(5, 3), (64, 10), (9, 10), (33, 65), (12, 4), (20, 13), (70, 1), (8, 8), (26, 5)]
    terms, ref = [], 0.0
    for nA, nG in dshapes:
        J, VA, VG, wA, wG, r = C.dense_case(nA, nG, 3, 4)
        terms.append(tuple(_dev(hip_device, J, VA, VG, wA[:nt], wG[:nt])))
        ref = ref + r[:nt]
    _check(kron_covariance_sweep(terms).cpu().numpy(), ref)


def test_accumulate_adds(hip_device):
    from bnn_kfac_amd import _native as N
    nt = 3
    a, D, VA, VG, wA, wG, ref = C.outer_case(63, 1, 10, 3, 10)
    ad, Dd, VAd, VGd, wAd, wGd = _dev(hip_device, a, D, VA, VG, wA[:nt], wG[:nt])
    job = N.CovOuterSweepJob(ad.data_ptr(), 63, 63, 1, Dd.data_ptr(), 10, 10, 0, VAd.data_ptr(), 64,
                             VGd.data_ptr(), 10, wAd.data_ptr(), 64, wGd.data_ptr(), 10)
    base = torch.from_numpy(np.array(ref[:nt])).float().to(hip_device) * 0.5
    base = (base + base.mT) / 2
    out = base.clone()
    N.kron_cov_outer_sweep([job], 3, 10, nt, out, accumulate=True)
    _check(out.cpu().numpy(), ref[:nt] + base.cpu().numpy().astype(np.float64))
    N.kron_cov_outer_sweep([job], 3, 10, nt, out, accumulate=False)
    _check(out.cpu().numpy(), ref[:nt])

    J, VA, VG, wA, wG, ref = C.dense_case(64, 10, 3, 10)
    Jd, VAd, VGd, wAd, wGd = _dev(hip_device, J, VA, VG, wA[:nt], wG[:nt])
    job = N.CovSweepJob(Jd.data_ptr(), 640, 64, 10, VAd.data_ptr(), 64, VGd.data_ptr(), 10, wAd.data_ptr(), 64,
                        wGd.data_ptr(), 10)
    base = torch.from_numpy(np.array(ref[:nt])).float().to(hip_device) * 0.5
    base = (base + base.mT) / 2
    out = base.clone()
    N.kron_cov_sweep([job], 3, 10, nt, out, accumulate=True)
    _check(out.cpu().numpy(), ref[:nt] + base.cpu().numpy().astype(np.float64))


def test_more_than_64_grid_points_go_through_further_calls(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_outer_sweep, kron_covariance_sweep
    a, D, VA, VG, wA, wG, ref = C.outer_case(63, 1, 10, 3, 10)
    order = np.concatenate([np.arange(64), np.arange(6)[::-1]])  # 70 grid points
    terms = [tuple(_dev(hip_device, a, D, VA, VG, wA[order], wG[order]))]
    got = kron_covariance_outer_sweep(terms)
    _check(got.cpu().numpy(), ref[order])
    assert torch.equal(got[64:], got[:6].flip(0))
    J, VA, VG, wA, wG, ref = C.dense_case(5, 3, 2, 4)
    got = kron_covariance_sweep([tuple(_dev(hip_device, J, VA, VG, wA[order], wG[order]))],
                                max_workspace_bytes=1 << 20)
    _check(got.cpu().numpy(), ref[order])


# ------------------------------------------------- consistency with the existing kernels
GRID4 = [(0.04, 200.0), (1.0, 200.0), (1e-4, 1.0), (1e-6, 1e4)]


@pytest.mark.parametrize("shape", [(63, 1, 10, 3, 10), (130, 1, 130, 5, 2)], ids=IDS)
def test_outer_sweep_agrees_with_plain_kernel_on_scaled_eigenvectors(hip_device, shape):
    from bnn_kfac_amd.variance import damping_weights, kron_covariance_outer, kron_covariance_outer_sweep
    cols, ones, nG, nb, nc = shape
    a, D = C.outer_case(*shape)[:2]
    lamA, VA = np.linalg.eigh(C.factor_shaped(cols + ones, ones, 1).astype(np.float64))
    lamG, VG = np.linalg.eigh(C.factor_shaped(nG, 0, 2).astype(np.float64))
    ad, Dd, VAd, VGd = _dev(hip_device, a, D, VA.astype(np.float32), VG.astype(np.float32))
    wA = damping_weights(torch.from_numpy(lamA).to(hip_device), GRID4)
    wG = damping_weights(torch.from_numpy(lamG).to(hip_device), GRID4)
    got = kron_covariance_outer_sweep([(ad, Dd, VAd, VGd, wA, wG)]).cpu().numpy()
    for t in range(len(GRID4)):
        want = kron_covariance_outer([(ad, Dd, VAd * wA[t].sqrt(), VGd * wG[t].sqrt())], lower=False).cpu().numpy()
        print(GRID4[t], "max diff / max =", float(np.abs(got[t] - want).max() / np.abs(want).max()))
        np.testing.assert_allclose(got[t], want, rtol=0, atol=2e-5 * np.abs(want).max())


@pytest.mark.parametrize("shape", [(64, 10, 3, 10), (33, 65, 2, 5)], ids=IDS)
def test_dense_sweep_agrees_with_plain_kernel_on_scaled_eigenvectors(hip_device, shape):
    from bnn_kfac_amd.variance import damping_weights, kron_covariance, kron_covariance_sweep
    nA, nG, nb, nc = shape
    J = C.dense_case(*shape)[0]
    lamA, VA = np.linalg.eigh(C.factor_shaped(nA, 1, 3).astype(np.float64))
    lamG, VG = np.linalg.eigh(C.factor_shaped(nG, 0, 4).astype(np.float64))
    Jd, VAd, VGd = _dev(hip_device, J, VA.astype(np.float32), VG.astype(np.float32))
    wA = damping_weights(torch.from_numpy(lamA).to(hip_device), GRID4)
    wG = damping_weights(torch.from_numpy(lamG).to(hip_device), GRID4)
    got = kron_covariance_sweep([(Jd, VAd, VGd, wA, wG)]).cpu().numpy()
    for t in range(len(GRID4)):
        want = kron_covariance([(Jd, VAd * wA[t].sqrt(), VGd * wG[t].sqrt())], lower=False).cpu().numpy()
        print(GRID4[t], "max diff / max =", float(np.abs(got[t] - want).max() / np.abs(want).max()))
        np.testing.assert_allclose(got[t], want, rtol=0, atol=2e-5 * np.abs(want).max())


def test_shape_mismatches_raise(hip_device):
    from bnn_kfac_amd.variance import kron_covariance_outer_sweep, kron_covariance_sweep
    dev = hip_device
    a, D = torch.zeros(2, 5, device=dev), torch.zeros(2, 3, 4, device=dev)
    VA, VG = torch.eye(6, device=dev), torch.eye(4, device=dev)
    wA, wG = torch.ones(2, 6, device=dev), torch.ones(2, 4, device=dev)
    assert kron_covariance_outer_sweep([(a, D, VA, VG, wA, wG)]).shape == (2, 2, 3, 3)
    for bad in ((a, D, torch.eye(7, device=dev), VG, torch.ones(2, 7, device=dev), wG),
                (a, D, VA, VG, wA[:, :5], wG), (a, D, VA, VG, wA, wG[:1]), (a[:1], D, VA, VG, wA, wG),
                (a, torch.zeros(2, 33, 4, device=dev), VA, VG, wA, wG)):
        with pytest.raises(ValueError):
            kron_covariance_outer_sweep([bad])
    J = torch.zeros(2, 3, 24, device=dev)
    assert kron_covariance_sweep([(J, VA, VG, wA, wG)]).shape == (2, 2, 3, 3)
    for bad in ((J[:, :, :23], VA, VG, wA, wG), (J, VA, VG, wA, wG[:, :3]), (J, VA, VG, wA[:1], wG)):
        with pytest.raises(ValueError):
            kron_covariance_sweep([bad])
    with pytest.raises(ValueError):
        kron_covariance_sweep([])


# ------------------------------------------------------------------ end to end
@pytest.fixture
def deterministic_convolutions():
    """torch's vmapped Conv2d weight gradient picks its MIOpen solver per call (see
    test_gpu_glm_factored.py): comparisons of two dense-route calls run in torch's
    deterministic mode."""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = before


@pytest.fixture(scope="module")
def fitted(hip_device):
    """name -> (net, kfac, x, layers, fp64 logits, fp64 cov per grid point, grid), fitted once."""
    cache = {}

    def get(name):
        if name not in cache:
            make, in_shape, loss_of = C.small_nets()[name]
            torch.manual_seed(0)
            rand = torch.rand if name == "basenet750" else torch.randn
            net, net64, kfac = C.fit(hip_device, make(), lambda n: rand(n, *in_shape, device=hip_device), loss_of)
            x = rand(5, *in_shape, device=hip_device)
            layers = [m for m in list(net.modules())[1:] if m in kfac.state]
            layers64 = [m for m in list(net64.modules())[1:] if isinstance(m, (nn.Linear, nn.Conv2d))]
            assert len(layers) == len(layers64) == len(kfac.state)
            grid = C.grid_for(len(layers))
            factors64 = [tuple(F_.double().cpu().numpy() for F_ in kfac.state[l]) for l in layers]
            logits64, rows = C.fp64_rows(net64, layers64, x.cpu())
            want = [C.fp64_cov(rows, factors64, [C.point_of(p, i) for i in range(len(layers))]) for p in grid]
            cache[name] = (net, kfac, x, layers, logits64, want, grid)
        return cache[name]

    return get


@pytest.mark.parametrize("route", ["dense", "factored"])
@pytest.mark.parametrize("name", ["no_bias", "regression", "relu_inplace", "basenet750"])
def test_glm_predictive_sweep_end_to_end(hip_device, fitted, deterministic_convolutions, name, route):
    from bnn_kfac_amd.variance import glm_predictive, glm_predictive_sweep, log_det_sweep
    net, kfac, x, layers, logits64, want, grid = fitted(name)
    logits, cov = glm_predictive_sweep(kfac, x, grid, chunk=2, jacobians=route)
    assert kfac.eig_state and list(kfac.eig_state) == list(kfac.state)
    nc = logits64.shape[1]
    assert logits.shape == (5, nc) and cov.shape == (len(grid), 5, nc, nc) and cov.dtype == torch.float32
    with torch.no_grad():
        direct = net(x).cpu().numpy()
    np.testing.assert_allclose(logits.cpu().numpy(), direct, rtol=1e-6, atol=1e-6 * np.abs(direct).max())
    np.testing.assert_allclose(logits.cpu().numpy(), logits64, rtol=1e-4, atol=1e-5 * np.abs(logits64).max())
    cov = cov.cpu().numpy()
    logdet = log_det_sweep(kfac, grid).cpu().numpy()
    assert torch.equal(log_det_sweep(kfac.eig_state, grid), log_det_sweep(kfac, grid))
    for t, point in enumerate(grid):
        worst = max(float(np.abs(cov[t, b] - want[t][b]).max() / np.abs(want[t][b]).max()) for b in range(5))
        print(name, route, point, "against fp64: max err / max|cov[b]| =", worst)
        for b in range(5):
            np.testing.assert_allclose(cov[t, b], want[t][b], rtol=0, atol=1e-4 * np.abs(want[t][b]).max())
        # the existing path: an inversion and a predictive per grid point
        kfac.invert(*point)
        _, old = glm_predictive(kfac, x, chunk=2, jacobians=route)
        old = old.cpu().numpy()
        worst = max(float(np.abs(cov[t, b] - old[b]).max() / np.abs(old[b]).max()) for b in range(5))
        print(name, route, point, "against invert + glm_predictive: max diff / max =", worst)
        for b in range(5):
            np.testing.assert_allclose(cov[t, b], old[b], rtol=0, atol=1e-4 * np.abs(old[b]).max())
        from_chol = 0.0
        for layer in layers:
            LA, LG = kfac.inv_state[layer]
            from_chol += -2.0 * (LG.shape[0] * float(torch.diagonal(LA).double().log().sum()) +
                                 LA.shape[0] * float(torch.diagonal(LG).double().log().sum()))
        print(name, point, "log det", logdet[t], "from invert", from_chol)
        np.testing.assert_allclose(logdet[t], from_chol, rtol=1e-5)


def test_sweep_uses_the_cached_eigenpairs_and_update_drops_them(hip_device, fitted):
    from bnn_kfac_amd.variance import glm_predictive_sweep
    net, kfac, x, layers, _, _, grid = fitted("no_bias")
    eig = kfac.eigh()
    assert kfac.eigh() is eig
    one = glm_predictive_sweep(kfac, x, grid[:1], jacobians="factored")[1]
    assert kfac.eig_state is eig
    # layers=...: a subset, and the grid's per-layer lists still index the state's entries
    sub = glm_predictive_sweep(kfac, x, grid, layers=layers[1:], jacobians="factored")[1]
    rest = glm_predictive_sweep(kfac, x, grid, layers=layers[:1], jacobians="factored")[1]
    both = glm_predictive_sweep(kfac, x, grid, jacobians="factored")[1]
    np.testing.assert_allclose((sub + rest).cpu().numpy(), both.cpu().numpy(), rtol=1e-5)
    assert torch.equal(both[:1], one)
    out = net(torch.randn(64, 12, device=hip_device))
    net.zero_grad()
    C.categorical_loss(out).backward()
    kfac.update(64)
    assert kfac.eig_state == {}
    with pytest.raises(ValueError):
        glm_predictive_sweep(kfac, x, grid, jacobians="nope")
    with pytest.raises(ValueError):
        glm_predictive_sweep(kfac, x, [])
