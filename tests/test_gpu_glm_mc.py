"""GPU: the Monte-Carlo GLM predictive -- kfac_glm_draws / kfac_glm_draws_outer
(variance.kron_draws / kron_draws_outer) and kfac_softmax_mc against fp64 numpy on the same fp32
inputs, integer-exact on small-integer inputs, their bitwise guarantees (repeatability, subsets
of the samples and of the draws, chunks), the covariance identity on one-hot draws, factored
against dense, the existing samplers on models that are linear in their weights, and
variance.glm_predictive_mc end to end against an fp64 CPU recompute.

Every raw-call case runs with pitches above the widths (lda = cols + 3, ldD = nG + 5,
ldJ = K + 7, ldZ = nA*nG + 3, ldF = R + 5), NaN in the padding, and F's pad columns are checked
to be NaN afterwards.

Kernel tolerance: the project's, rtol 1e-5, atol 1e-5 * max|ref|.  Two fp32 evaluations of one
quantity, or an end-to-end check: rtol 1e-4, atol 1e-5 * max|ref|.  kfac_softmax_mc is fp64
inside: it meets the first on psum / ns and hsum / ns."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import glm_mc_cases as C
import glm_sweep_cases as S

pytestmark = pytest.mark.gpu


def _dev(dev, *arrays):
    return [torch.from_numpy(np.array(t)).to(dev) for t in arrays]  # (a copy: the cached case stays read-only)


def _padded(t, extra):
    """t's values in a NaN-filled tensor `extra` wider in the last dimension, as a view."""
    wide = torch.full(tuple(t.shape[:-1]) + (t.shape[-1] + extra,), float("nan"), device=t.device)
    wide[..., :t.shape[-1]] = t
    return wide[..., :t.shape[-1]]


def _z_view(Z):
    """Z (ns, nA, nG) as a view whose draws are nA*nG + 3 apart, NaN between them."""
    ns, nA, nG = Z.shape
    return _padded(Z.reshape(ns, nA * nG), 3).view(ns, nA, nG)


def _raw(dev, route, terms, nb, nc, prefill=None):
    """The raw call on padded operands: terms [(a, D, K1, K2, Z, lower)] (outer) or
    [(J, K1, K2, Z, lower)] (rows) of device tensors; returns F (ns, nb*nc)."""
    from bnn_kfac_amd import _native as N
    from bnn_kfac_amd import variance as V
    jobs, keep = [], []
    for *ops, Z, lower in terms:
        z, ldz = V._draw_z(_z_view(Z), Z.shape[1], Z.shape[2], None, 0)
        ns = Z.shape[0]
        assert ns == 1 or ldz == Z.shape[1] * Z.shape[2] + 3
        if route == "outer":
            a, D, K1, K2 = ops
            k, j, _, _ = V._cov_outer_jobs([(_padded(a, 3), _padded(D, 5), K1, K2)], lower, "test")
            assert (nb == 1 or j[0][1] == a.shape[1] + 3) and (nb * nc == 1 or j[0][5] == D.shape[2] + 5)
            jobs.append(N.DrawOuterJob(N.CovOuterJob(*j[0]), z.data_ptr(), ldz))
        else:
            J, K1, K2 = ops
            k, j, _, _ = V._cov_jobs([(_padded(J, 7), K1, K2)], lower, "test")
            assert nb * nc == 1 or j[0][1] == J.shape[2] + 7
            jobs.append(N.DrawJob(N.CovJob(*j[0]), z.data_ptr(), ldz))
        keep.extend([k, z])
    R = nb * nc
    wide = torch.full((ns, R + 5), float("nan"), device=dev)
    if prefill is not None:
        wide[:, :R] = prefill
    call = N.glm_draws_outer if route == "outer" else N.glm_draws
    call(jobs, nb, nc, ns, wide[:, :R], accumulate=prefill is not None)
    torch.cuda.synchronize()
    assert bool(torch.isnan(wide[:, R:]).all()), "the pad columns of F were written"
    return wide[:, :R].clone()


def _check(got, ref):
    print("max err / max|ref| =", float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)))
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())


def _close(got, want):
    print("max diff / max =", float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)))
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5 * np.abs(want).max())


# ------------------------------------------------------------------ against fp64
@pytest.mark.parametrize("shape", C.OUTER, ids=C.IDS)
def test_outer_draws_match_fp64(hip_device, shape):
    cols, ones, nG, nb, nc, ns = shape
    *arrays, ref = C.outer_case(*shape)
    got = _raw(hip_device, "outer", [(*_dev(hip_device, *arrays), True)], nb, nc)
    _check(got.cpu().numpy(), ref.reshape(ns, nb * nc))


@pytest.mark.parametrize("shape", C.DENSE, ids=C.IDS)
def test_draws_match_fp64(hip_device, shape):
    nA, nG, nb, nc, ns = shape
    *arrays, ref = C.dense_case(*shape)
    got = _raw(hip_device, "rows", [(*_dev(hip_device, *arrays), True)], nb, nc)
    _check(got.cpu().numpy(), ref.reshape(ns, nb * nc))


@pytest.mark.parametrize("shape", [(63, 1, 10, 3, 10, 2), (20, 0, 130, 3, 33, 5)], ids=C.IDS)
def test_outer_draws_dense_factors(hip_device, shape):
    *arrays, ref = C.outer_case(*shape, lower=False)
    assert np.abs(np.triu(arrays[2], 1)).max() > 0 and np.abs(np.triu(arrays[3], 1)).max() > 0
    got = _raw(hip_device, "outer", [(*_dev(hip_device, *arrays), False)], shape[3], shape[4])
    _check(got.cpu().numpy(), ref.reshape(shape[5], -1))


@pytest.mark.parametrize("shape", [(5, 4, 3, 10, 3), (65, 33, 2, 3, 2)], ids=C.IDS)
def test_draws_dense_factors(hip_device, shape):
    *arrays, ref = C.dense_case(*shape, lower=False)
    assert np.abs(np.triu(arrays[1], 1)).max() > 0 and np.abs(np.triu(arrays[2], 1)).max() > 0
    got = _raw(hip_device, "rows", [(*_dev(hip_device, *arrays), False)], shape[2], shape[3])
    _check(got.cpu().numpy(), ref.reshape(shape[4], -1))


# ------------------------------------------------------------------ integer-exact
@pytest.mark.parametrize("route", ["outer", "rows"])
@pytest.mark.parametrize("name", list(C.INT_CASES))
def test_draws_integer_exact(hip_device, name, route):
    """Small-integer inputs (test_glm_mc_host.py shows every partial sum stays below 2^24): the
    result has the int64 reference's bits, through the job sum and the accumulate prefill."""
    c = C.int_case(name)
    assert C.int_bound(c, route) < C.LIMIT
    terms = []
    for j in c.jobs:
        f = lambda t: t.astype(np.float32)  # noqa: E731
        if route == "outer":
            terms.append((*_dev(hip_device, f(j.a), f(j.D), f(j.K1), f(j.K2), f(j.Z)), j.lower))
        else:
            terms.append((*_dev(hip_device, f(C.outer_rows(j.a, j.ones, j.D)), f(j.K1), f(j.K2), f(j.Z)), j.lower))
    prefill = None
    if c.accumulate:
        prefill = torch.from_numpy(c.prefill.astype(np.float32)).to(hip_device).view(c.ns, -1)
    got = _raw(hip_device, route, terms, c.nb, c.nc, prefill)
    want = torch.from_numpy(C.int_reference(c, route).astype(np.float32)).view(c.ns, -1)
    assert torch.equal(got.cpu(), want)


# ------------------------------------------------------------------ bitwise guarantees
SUBSET = [1, 3, 66]


def test_outer_draws_bitwise_guarantees(hip_device):
    from bnn_kfac_amd import _native as N
    from bnn_kfac_amd import variance as V
    cols, ones, nG, nb, nc, ns = shape = (20, 1, 65, 70, 3, 6)
    a, D, K1, K2, Z = _dev(hip_device, *C.outer_case(*shape)[:5])
    whole = V.kron_draws_outer([(a, D, K1, K2)], [Z])
    assert whole.shape == (ns, nb, nc) and whole.dtype == torch.float32
    assert torch.equal(whole, V.kron_draws_outer([(a, D, K1, K2)], [Z]))
    part = V.kron_draws_outer([(a[SUBSET].contiguous(), D[SUBSET].contiguous(), K1, K2)], [Z])
    assert torch.equal(part, whole[:, SUBSET])
    assert torch.equal(V.kron_draws_outer([(a, D, K1, K2)], [Z[1:4]]), whole[1:4])
    halves = [V.kron_draws_outer([(a, D, K1, K2)], [Z[s0:s0 + 3]]) for s0 in (0, 3)]
    assert torch.equal(torch.cat(halves), whole)
    # a budget one byte short of the whole call's scratch: the draws are cut, no bit changes
    _, jobs, _, _ = V._cov_outer_jobs([(a, D, K1, K2)], True, "test")
    need = N.glm_draws_outer_workspace_bytes(
        [N.DrawOuterJob(N.CovOuterJob(*jobs[0]), Z.data_ptr(), Z.stride(0))], nb, nc, ns)
    assert need > 0
    assert torch.equal(V.kron_draws_outer([(a, D, K1, K2)], [Z], max_workspace_bytes=need - 1), whole)
    with pytest.raises(ValueError, match="workspace bytes"):
        V.kron_draws_outer([(a, D, K1, K2)], [Z], max_workspace_bytes=16)


def test_draws_bitwise_guarantees(hip_device):
    from bnn_kfac_amd import variance as V
    nA, nG, nb, nc, ns = shape = (65, 33, 13, 5, 6)
    J, K1, K2, Z = _dev(hip_device, *C.dense_case(*shape)[:4])
    whole = V.kron_draws([(J, K1, K2)], [Z])
    assert whole.shape == (ns, nb, nc) and whole.dtype == torch.float32
    assert torch.equal(whole, V.kron_draws([(J, K1, K2)], [Z]))
    subset = [1, 3, 12]
    assert torch.equal(V.kron_draws([(J[subset].contiguous(), K1, K2)], [Z]), whole[:, subset])
    assert torch.equal(V.kron_draws([(J, K1, K2)], [Z[1:4]]), whole[1:4])
    halves = [V.kron_draws([(J, K1, K2)], [Z[s0:s0 + 3]]) for s0 in (0, 3)]
    assert torch.equal(torch.cat(halves), whole)


# ------------------------------------------------------------------ identities
def test_one_hot_draws_give_the_joint_covariance(hip_device):
    """Z = all nA*nG one-hot draws: F = T^T, so F^T F is the joint covariance of the same
    terms (deterministic: two fp32 evaluations of one quantity)."""
    from bnn_kfac_amd import variance as V
    cols, ones, nG, nb, nc = 4, 1, 4, 7, 10
    nA = cols + ones
    Z = torch.eye(nA * nG, device=hip_device).view(nA * nG, nA, nG)
    a, D, K1, K2 = _dev(hip_device, *C.outer_case(cols, ones, nG, nb, nc, 1)[:4])
    F = V.kron_draws_outer([(a, D, K1, K2)], [Z]).view(nA * nG, -1).double().cpu().numpy()
    cov = V.kron_covariance_outer_joint([(a, D, K1, K2)]).view(nb * nc, nb * nc).cpu().numpy()
    _close(F.T @ F, cov.astype(np.float64))
    J, K1, K2 = _dev(hip_device, *C.dense_case(nA, nG, nb, nc, 1)[:3])
    F = V.kron_draws([(J, K1, K2)], [Z]).view(nA * nG, -1).double().cpu().numpy()
    cov = V.kron_covariance_joint([(J, K1, K2)]).view(nb * nc, nb * nc).cpu().numpy()
    _close(F.T @ F, cov.astype(np.float64))


@pytest.mark.parametrize("shape", [(63, 1, 10, 3, 10, 2), (20, 0, 130, 3, 33, 5)], ids=C.IDS)
def test_factored_agrees_with_dense_on_rank_one_rows(hip_device, shape):
    from bnn_kfac_amd import variance as V
    a, D, K1, K2, Z, _ = C.outer_case(*shape)
    ad, Dd, K1d, K2d, Zd, Jd = _dev(hip_device, a, D, K1, K2, Z, C.outer_rows(a, shape[1], D))
    _close(V.kron_draws_outer([(ad, Dd, K1d, K2d)], [Zd]).cpu().numpy(),
           V.kron_draws([(Jd, K1d, K2d)], [Zd]).cpu().numpy())


def test_nine_terms_fold_in_groups_of_eight(hip_device):
    from bnn_kfac_amd import variance as V
    shapes = [(4, 1, 3), (63, 1, 10), (9, 0, 10), (70, 1, 65), (12, 1, 4), (20, 1, 130), (33, 0, 31),
              (8, 1, 8), (64, 1, 64)]
    outer, dense, zs, ref = [], [], [], 0.0
    for cols, ones, nG in shapes:
        a, D, K1, K2, Z, r = C.outer_case(cols, ones, nG, 3, 4, 2)
        ad, Dd, K1d, K2d, Zd, Jd = _dev(hip_device, a, D, K1, K2, Z, C.outer_rows(a, ones, D))
        outer.append((ad, Dd, K1d, K2d))
        dense.append((Jd, K1d, K2d))
        zs.append(Zd)
        ref = ref + r
    _check(V.kron_draws_outer(outer, zs).cpu().numpy(), ref)
    _check(V.kron_draws(dense, zs).cpu().numpy(), ref)


def test_shape_mismatches_raise(hip_device):
    from bnn_kfac_amd import variance as V
    eye = lambda n: torch.eye(n, device=hip_device)  # noqa: E731
    J = torch.zeros(2, 3, 20, device=hip_device)
    z = torch.zeros(4, 5, 4, device=hip_device)
    with pytest.raises(ValueError):
        V.kron_draws([], [])
    with pytest.raises(ValueError):
        V.kron_draws([(J, eye(5), eye(4))], [])
    with pytest.raises(ValueError):
        V.kron_draws([(J, eye(5), eye(4))], [z[:, :, :3]])
    with pytest.raises(ValueError):
        V.kron_draws([(J, eye(5), eye(4)), (J, eye(5), eye(4))], [z, z[:2]])
    a, D = torch.zeros(2, 4, device=hip_device), torch.zeros(2, 3, 4, device=hip_device)
    with pytest.raises(ValueError):
        V.kron_draws_outer([(a, D, eye(5), eye(4))], [z.view(4, 4, 5)])
    with pytest.raises(N_error()):
        V.kron_draws_outer([(a, D, eye(5), eye(4))], [z.cpu()])


def N_error():
    from bnn_kfac_amd import _native as N
    return N.NativeError


# ------------------------------------------------------------------ softmax statistics
def _softmax_raw(dev, mean, F, chunks=1):
    """kfac_softmax_mc on padded operands (ldm = nc + 3, ldF = nb*nc + 5, NaN in the padding),
    the draws in `chunks` calls; returns the four finished statistics as numpy."""
    from bnn_kfac_amd import _native as N
    from bnn_kfac_amd import variance as V
    ns, nb, nc = F.shape
    md, Fd = _dev(dev, mean, F)
    md = _padded(md, 3)
    Fd = _padded(Fd.reshape(ns, nb * nc), 5).view(ns, nb, nc)
    psum = torch.full((nb, nc), float("nan"), dtype=torch.float64, device=dev)
    hsum = torch.full((nb,), float("nan"), dtype=torch.float64, device=dev)
    step = -(-ns // chunks)
    for i, s0 in enumerate(range(0, ns, step)):
        N.softmax_mc(md, Fd[s0:s0 + step], psum, hsum, accumulate=i > 0)
    return psum, hsum, [t.cpu().numpy() for t in V._softmax_mc_finish(psum, hsum, ns)]


@pytest.mark.parametrize("shape", C.SOFTMAX + [(5, 4, 10, 80.0)], ids=C.IDS)
def test_softmax_mc_matches_fp64(hip_device, shape):
    mean, F, *refs = C.softmax_case(*shape)
    ns = shape[0]
    psum, hsum, got = _softmax_raw(hip_device, mean, F)
    for g, r, what in zip(got, refs, ("probs", "expected_entropy", "entropy", "mutual_information")):
        assert g.dtype == np.float32 and g.shape == r.shape and np.isfinite(g).all(), what
        print(what, end=": ")
        _check(g, r)
    _check((psum / ns).cpu().numpy(), refs[0])
    _check((hsum / ns).cpu().numpy(), refs[1])
    np.testing.assert_allclose(got[0].sum(axis=1), 1.0, rtol=0, atol=1e-6)
    assert (got[3] >= 0).all()
    if ns > 1:  # the draws in two calls: the running sums go on, no bit changes
        psum2, hsum2, _ = _softmax_raw(hip_device, mean, F, chunks=2)
        assert torch.equal(psum, psum2) and torch.equal(hsum, hsum2)


def test_softmax_mc_stats_wrapper(hip_device):
    from bnn_kfac_amd import variance as V
    mean, F, *refs = C.softmax_case(7, 5, 10)
    got = V.softmax_mc_stats(*_dev(hip_device, mean, F))
    for g, r in zip(got, refs):
        _check(g.cpu().numpy(), r)


# ------------------------------------------------------------------ the existing samplers
def _inject(monkeypatch, draws):
    """torch.randn returns `draws` in order (as test_gpu_golden_r02 injects the reference's)."""
    queue = list(draws)

    def randn(*shape, **kw):
        z = queue.pop(0)
        assert tuple(z.shape) == tuple(shape)
        return z.clone()
    monkeypatch.setattr(torch, "randn", randn)


def _linear_in_weights(name, dev):
    if name == "linear":
        return nn.Sequential(nn.Linear(12, 5)), lambda n: torch.randn(n, 12, device=dev)
    return nn.Sequential(nn.Conv2d(2, 3, 3), nn.Flatten()), lambda n: torch.randn(n, 2, 6, 6, device=dev)


def _forward64(layer, x):
    """The one-layer model in fp64 from the layer's current fp32 weights."""
    w, b, x = layer.weight.detach().double(), layer.bias.detach().double(), x.double()
    if isinstance(layer, nn.Linear):
        return x @ w.T + b
    return torch.nn.functional.conv2d(x, w, b).flatten(1)


@pytest.mark.parametrize("name", ["linear", "conv"])
def test_draw_is_what_sample_and_replace_does(hip_device, monkeypatch, name):
    """One z through KFAC.sample_and_replace() and a forward pass, and through
    glm_predictive_mc: the model is linear in its weights, so the two agree (orders, the bias
    row and z's shape end to end)."""
    from bnn_kfac_amd.variance import glm_predictive_mc
    torch.manual_seed(0)
    net, make_x = _linear_in_weights(name, hip_device)
    net, _, kfac = S.fit(hip_device, net, make_x, S.categorical_loss)
    kfac.invert(0.04, 200.0)
    layer = net[0]
    x = make_x(5)
    nA, nG = (t.shape[0] for t in kfac.inv_state[layer])
    z = torch.randn(nA, nG, device=hip_device)
    mean = _forward64(layer, x)
    with monkeypatch.context() as m:
        _inject(m, [z])
        kfac.sample_and_replace()
    want = (_forward64(layer, x) - mean).cpu().numpy()
    net.load_state_dict(kfac.model_state)
    assert np.abs(want).max() > 0
    for route in ("factored", "dense"):
        res = glm_predictive_mc(kfac, x, n_draws=1, z=[z[None]], jacobians=route, return_draws=True)
        assert res.draws.shape == (1, 5, want.shape[1])
        print(name, route, end=": ")
        _close(res.draws[0].cpu().numpy(), want)
        np.testing.assert_allclose(res.logits.cpu().numpy(), mean.cpu().numpy(), rtol=1e-4,
                                   atol=1e-5 * float(mean.abs().max()))


def test_draw_is_what_efb_sample_does(hip_device, monkeypatch):
    from bnn_kfac_amd.curvatures import EFB
    from bnn_kfac_amd.variance import glm_predictive_mc
    torch.manual_seed(0)
    net, make_x = _linear_in_weights("linear", hip_device)
    net, _, kfac = S.fit(hip_device, net, make_x, S.categorical_loss)
    layer = net[0]
    efb = EFB(net, {layer: [t.clone() for t in kfac.state[layer]]})
    for _ in range(2):
        out = net(make_x(64))
        net.zero_grad()
        S.categorical_loss(out).backward()
        efb.update(64)
    efb.invert(0.04, 200.0)
    x = make_x(5)
    z = torch.randn(13, 5, device=hip_device)
    with monkeypatch.context() as m:
        _inject(m, [z])
        sample = efb.sample(layer).double()  # (nG, nA): the perturbation of [W | b]
    want = (x.double() @ sample[:, :12].T + sample[:, 12]).cpu().numpy()
    assert np.abs(want).max() > 0
    for route in ("factored", "dense"):
        res = glm_predictive_mc(efb, x, n_draws=1, z=[z[None]], jacobians=route, return_draws=True)
        print("efb", route, end=": ")
        _close(res.draws[0].cpu().numpy(), want)


# ------------------------------------------------------------------ end to end
def _e2e_nets():
    from models_for_tests import BaseNet750, mlp
    return {"mlp": (mlp, (784,)), "basenet750": (BaseNet750, (1, 28, 28))}


@pytest.fixture(scope="module")
def e2e(hip_device):
    """name -> (kfac, x, layers, z, fp64 logits, fp64 draws (S, N, nc)): the reference once."""
    cache = {}

    def get(name):
        if name in cache:
            return cache[name]
        make, xshape = _e2e_nets()[name]
        torch.manual_seed(0)
        make_x = (lambda n: torch.rand(n, *xshape, device=hip_device)) if len(xshape) == 3 else \
            (lambda n: torch.randn(n, *xshape, device=hip_device))
        net, net64, kfac = S.fit(hip_device, make(), make_x, S.categorical_loss)
        kfac.invert(0.04, 200.0)
        x = make_x(5)
        layers = [m for m in list(net.modules())[1:] if m in kfac.state]
        layers64 = [m for m in list(net64.modules())[1:] if isinstance(m, (nn.Linear, nn.Conv2d))]
        assert len(layers) == len(layers64)
        g = torch.Generator(device=hip_device).manual_seed(5)
        z = [torch.randn(3, *(t.shape[0] for t in kfac.inv_state[layer]), generator=g, device=hip_device)
             for layer in layers]
        logits, rows = S.fp64_rows(net64, layers64, x.cpu())
        draws = 0.0
        for layer, M, zl in zip(layers, rows, z):
            LA, LG = (t.double().cpu().numpy() for t in kfac.inv_state[layer])
            Sl = np.matmul(np.matmul(LA, zl.double().cpu().numpy()), LG.T)  # the weight draws K1 Z K2^T
            draws = draws + np.einsum("bcag,sag->sbc", M, Sl)
        cache[name] = (kfac, x, layers, z, logits, draws)
        return cache[name]
    return get


@pytest.fixture
def deterministic_convolutions():
    """(test_gpu_glm_factored's finding: torch's vmapped Conv2d gradients pick their MIOpen
    solver per call; the bitwise comparison of two glm_predictive_mc calls is about this
    project's code, so it runs in torch's deterministic mode.)"""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = before


@pytest.mark.parametrize("route", ["factored", "dense"])
@pytest.mark.parametrize("name", ["mlp", "basenet750"])
def test_glm_predictive_mc_end_to_end(hip_device, deterministic_convolutions, e2e, name, route):
    from bnn_kfac_amd.variance import glm_predictive_mc
    kfac, x, layers, z, logits, draws = e2e(name)
    probs, expected, entropy, mi = C.softmax_ref(logits, draws)
    res = glm_predictive_mc(kfac, x, n_draws=3, chunk=2, jacobians=route, z=z, return_draws=True)
    assert res.draws.shape == draws.shape and res.probs.shape == probs.shape
    got = {"logits": res.logits, "draws": res.draws, "probs": res.probs, "entropy": res.entropy,
           "expected_entropy": res.expected_entropy, "mutual_information": res.mutual_information}
    want = {"logits": logits, "draws": draws, "probs": probs, "entropy": entropy,
            "expected_entropy": expected, "mutual_information": mi}
    for key in got:
        g, w = got[key].cpu().numpy(), want[key]
        print(name, route, key, "max diff / max =", float(np.abs(g - w).max() / np.abs(w).max()))
    for key in got:
        np.testing.assert_allclose(got[key].cpu().numpy(), want[key], rtol=1e-4,
                                   atol=1e-5 * np.abs(want[key]).max(), err_msg=key)
    # without the draws tensor: the same statistics, bit for bit; draws in two chunks as well
    lean = glm_predictive_mc(kfac, x, n_draws=3, chunk=2, jacobians=route, z=z)
    assert lean.draws is None
    per_draw = 4 * sum(zl[0].numel() for zl in z)
    cut = glm_predictive_mc(kfac, x, n_draws=3, chunk=2, jacobians=route, z=z, max_draw_bytes=2 * per_draw,
                            return_draws=True)
    assert torch.equal(cut.draws, res.draws)
    for other in (lean, cut):
        for a, b in zip(other[:5], res[:5]):
            assert torch.equal(a, b)


def test_glm_predictive_mc_properties(hip_device, e2e):
    from bnn_kfac_amd.variance import glm_predictive_mc
    kfac, x, layers, z, logits, _ = e2e("mlp")
    shapes = [tuple(zl.shape[1:]) for zl in z]
    g1 = torch.Generator(device=hip_device).manual_seed(9)
    drawn = glm_predictive_mc(kfac, x, n_draws=4, chunk=2, generator=g1, return_draws=True)
    assert drawn.draws.shape == (4, 5, 10)
    np.testing.assert_allclose(drawn.probs.sum(dim=1).cpu().numpy(), 1.0, rtol=0, atol=1e-6)
    assert bool((drawn.mutual_information >= 0).all()) and bool((drawn.mutual_information > 0).any())
    # the documented order of the draws: per draw chunk, the layers in `layers` order
    g2 = torch.Generator(device=hip_device).manual_seed(9)
    same = [torch.randn(4, *s, generator=g2, device=hip_device) for s in shapes]
    assert torch.equal(glm_predictive_mc(kfac, x, n_draws=4, chunk=2, z=same, return_draws=True).draws,
                       drawn.draws)
    # z = 0: every draw is the mean, so probs = softmax(logits) and nothing is epistemic
    # (fp64 sums of identical terms: what is left is a few fp64 roundings)
    zero = glm_predictive_mc(kfac, x, n_draws=3, chunk=2, z=[torch.zeros(3, *s, device=hip_device) for s in shapes],
                             return_draws=True)
    assert not bool(zero.draws.any())
    soft = torch.softmax(zero.logits.double(), dim=1).cpu().numpy()
    _check(zero.probs.cpu().numpy(), soft)
    assert float(zero.mutual_information.abs().max()) <= 1e-12
    with pytest.raises(ValueError):
        glm_predictive_mc(kfac, x, n_draws=3, z=same)  # four draws given
    with pytest.raises(ValueError):
        glm_predictive_mc(kfac, x, n_draws=3, jacobians="nope")


def test_glm_predictive_mc_regression(hip_device):
    """nc = 1: the draws are the output; the statistics are the degenerate ones, not special-cased."""
    from bnn_kfac_amd.variance import glm_predictive, glm_predictive_mc
    make, xshape, loss_of = S.small_nets()["regression"]
    torch.manual_seed(0)
    make_x = lambda n: torch.randn(n, *xshape, device=hip_device)  # noqa: E731
    net, _, kfac = S.fit(hip_device, make(), make_x, loss_of)
    kfac.invert(0.04, 200.0)
    x = make_x(5)
    res = glm_predictive_mc(kfac, x, n_draws=4, generator=torch.Generator(device=hip_device).manual_seed(1),
                            return_draws=True)
    assert res.draws.shape == (4, 5, 1) and bool(res.draws.abs().max() > 0)
    assert torch.equal(res.probs, torch.ones(5, 1, device=hip_device))
    for t in (res.entropy, res.expected_entropy, res.mutual_information):
        assert not bool(t.any())
    assert torch.equal(res.logits, glm_predictive(kfac, x, jacobians="factored")[0])
