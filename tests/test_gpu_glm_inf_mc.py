"""GPU: the Monte-Carlo GLM predictive under the INF posterior -- kfac_inf_draws /
kfac_inf_draws_outer (variance.kron_draws_inf / kron_draws_outer_inf) against fp64 numpy on the
same fp32 inputs, integer-exact on small-integer inputs, their bitwise guarantees (repeatability,
subsets of the samples and of the draws, chunks, the F = 0 identity with kfac_glm_draws_outer),
the covariance identity on one-hot draws, factored against dense, a draw against an actual weight
sample (inf_posterior_sample written into the model), and variance.glm_predictive_mc under an INF
end to end against an fp64 CPU recompute from inf.state.

Every raw-call case runs with pitches above the widths (lda = cols + 3, ldD = nG + 5,
ldJ = K + 7, ldZ = nA*nG + 3, ldE = r + 2, ldF = R + 5), NaN in the padding, and F's pad columns
are checked to be NaN afterwards.

Kernel tolerance (glm_inf_mc_cases): rtol = SCALE, atol = SCALE * max(max|first|, max|second|),
SCALE from the fp32 stage chain measured on the CPU.  Two fp32 evaluations of one quantity, or an
end-to-end check: test_gpu_glm_mc.py's, rtol 1e-4, atol 1e-5 * max|ref|."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

import glm_inf_cases as P
import glm_inf_mc_cases as C
import glm_mc_cases as MC
import glm_sweep_cases as S

pytestmark = pytest.mark.gpu

ADD, MULTIPLY = 1.0, 100.0   # test_gpu_glm_inf.py's damping of the end-to-end checks


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
    """The raw call on padded operands: terms [(a, D, UA, UG, W, F, C, Binv, Z, E)] (outer) or
    [(J, UA, UG, W, F, C, Binv, Z, E)] (rows) of device tensors; returns F (ns, nb*nc)."""
    from bnn_kfac_amd import _native as N
    from bnn_kfac_amd import variance as V
    full, zl, el = [], [], []
    for *ops, Z, E in terms:
        if route == "outer":
            a, D, *rest = ops
            full.append((_padded(a, 3), _padded(D, 5), *rest))
        else:
            J, *rest = ops
            full.append((_padded(J, 7), *rest))
        zl.append(_z_view(Z))
        el.append(_padded(E, 2))
    ns, R = terms[0][-2].shape[0], nb * nc
    cov_terms, zs = V._inf_draw_operands(full, zl, el, "test")
    if route == "outer":
        keep, jobs, _, _ = V._inf_outer_jobs(cov_terms, "test", None)
        structs = [N.InfDrawOuterJob(N.InfCovOuterJob(*j), *V._inf_draw_at(z, 0)) for j, z in zip(jobs, zs)]
        for j, t in zip(jobs, terms):
            assert (nb == 1 or j[1] == t[0].shape[1] + 3) and (R == 1 or j[5] == t[1].shape[2] + 5)
    else:
        keep, jobs, _, _ = V._inf_dense_jobs(cov_terms, "test", None)
        structs = [N.InfDrawJob(N.InfCovJob(*j), *V._inf_draw_at(z, 0)) for j, z in zip(jobs, zs)]
        for j, t in zip(jobs, terms):
            assert R == 1 or j[1] == t[0].shape[2] + 7
    for z, t in zip(zs, terms):
        Z, E = t[-2], t[-1]
        assert ns == 1 or (z[1] == Z.shape[1] * Z.shape[2] + 3 and z[3] == E.shape[1] + 2)
    wide = torch.full((ns, R + 5), float("nan"), device=dev)
    if prefill is not None:
        wide[:, :R] = prefill
    call = N.inf_draws_outer if route == "outer" else N.inf_draws
    call(structs, nb, nc, ns, wide[:, :R], accumulate=prefill is not None)
    torch.cuda.synchronize()
    assert bool(torch.isnan(wide[:, R:]).all()), "the pad columns of F were written"
    return wide[:, :R].clone()


def _check(got, ref, top):
    print("max err / max(max|first|, max|second|) =", float(np.abs(got - ref).max() / top), "SCALE", C.SCALE)
    np.testing.assert_allclose(got, ref, rtol=C.SCALE, atol=C.SCALE * top)


def _close(got, want):
    print("max diff / max =", float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)))
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5 * np.abs(want).max())


# ------------------------------------------------------------------ against fp64
@pytest.mark.parametrize("shape", C.OUTER_SHAPES, ids=C.IDS)
def test_outer_inf_draws_match_fp64(hip_device, shape):
    cols, ones, nG, ra, rg, nb, nc, ns = shape
    *arrays, ref, top = C.outer_case(*shape)
    got = _raw(hip_device, "outer", [tuple(_dev(hip_device, *arrays))], nb, nc)
    _check(got.cpu().numpy(), ref.reshape(ns, nb * nc), top)


@pytest.mark.parametrize("shape", C.DENSE_SHAPES, ids=C.IDS)
def test_inf_draws_match_fp64(hip_device, shape):
    nA, nG, ra, rg, nb, nc, ns = shape
    *arrays, ref, top = C.dense_case(*shape)
    got = _raw(hip_device, "rows", [tuple(_dev(hip_device, *arrays))], nb, nc)
    _check(got.cpu().numpy(), ref.reshape(ns, nb * nc), top)


# ------------------------------------------------------------------ integer-exact
@pytest.mark.parametrize("route", ["outer", "rows"])
@pytest.mark.parametrize("name", list(C.INT_CASES))
def test_inf_draws_integer_exact(hip_device, name, route):
    """Small-integer inputs (int_bound: every partial sum of every stage stays below 2^24): the
    result has the int64 reference's bits, through the job sum and the accumulate prefill."""
    c = C.int_case(name)
    kind = "outer" if route == "outer" else "dense"
    assert 0 < C.int_bound(c, kind) < C.EXACT
    f = lambda t: t.astype(np.float32)  # noqa: E731
    terms = []
    for j in c.jobs:
        head = (f(j.a), f(j.D)) if route == "outer" else (f(C.int_rows(j)),)
        terms.append(tuple(_dev(hip_device, *head, f(j.UA), f(j.UG), f(j.W), f(j.F), f(j.C), f(j.Binv), f(j.Z),
                                f(j.E))))
    prefill = None
    if c.accumulate:
        prefill = torch.from_numpy(c.prefill.astype(np.float32)).to(hip_device).view(c.ns, -1)
    got = _raw(hip_device, route, terms, c.nb, c.nc, prefill)
    want = torch.from_numpy(C.int_reference(c, kind).astype(np.float32)).view(c.ns, -1)
    assert bool(want.abs().max() > 0)
    assert torch.equal(got.cpu(), want)


# ------------------------------------------------------------------ bitwise guarantees
SUBSET = [1, 3, 66]


def test_outer_inf_draws_bitwise_guarantees(hip_device):
    from bnn_kfac_amd import _native as N
    from bnn_kfac_amd import variance as V
    cols, ones, nG, ra, rg, nb, nc, ns = shape = (20, 1, 65, 7, 9, 70, 3, 6)
    a, D, UA, UG, W, F, Cc, Binv, Z, E = _dev(hip_device, *C.outer_case(*shape)[:10])
    term = (a, D, UA, UG, W, F, Cc, Binv)
    whole = V.kron_draws_outer_inf([term], [Z], [E])
    assert whole.shape == (ns, nb, nc) and whole.dtype == torch.float32
    assert torch.equal(whole, V.kron_draws_outer_inf([term], [Z], [E]))
    part = V.kron_draws_outer_inf([(a[SUBSET].contiguous(), D[SUBSET].contiguous(), *term[2:])], [Z], [E])
    assert torch.equal(part, whole[:, SUBSET])
    assert torch.equal(V.kron_draws_outer_inf([term], [Z[1:4]], [E[1:4]]), whole[1:4])
    halves = [V.kron_draws_outer_inf([term], [Z[s0:s0 + 3]], [E[s0:s0 + 3]]) for s0 in (0, 3)]
    assert torch.equal(torch.cat(halves), whole)
    # a budget one byte short of the whole call's scratch: the draws are cut, no bit changes
    cov_terms, zs = V._inf_draw_operands([term], [Z], [E], "test")
    _, jobs, _, _ = V._inf_outer_jobs(cov_terms, "test", None)
    need = N.inf_draws_outer_workspace_bytes(
        [N.InfDrawOuterJob(N.InfCovOuterJob(*jobs[0]), *V._inf_draw_at(zs[0], 0))], nb, nc, ns)
    assert need > 0
    assert torch.equal(V.kron_draws_outer_inf([term], [Z], [E], max_workspace_bytes=need - 1), whole)
    with pytest.raises(ValueError, match="workspace bytes"):
        V.kron_draws_outer_inf([term], [Z], [E], max_workspace_bytes=16)


def test_inf_draws_bitwise_guarantees(hip_device):
    from bnn_kfac_amd import _native as N
    from bnn_kfac_amd import variance as V
    nA, nG, ra, rg, nb, nc, ns = shape = (65, 33, 5, 7, 13, 5, 6)
    J, UA, UG, W, F, Cc, Binv, Z, E = _dev(hip_device, *C.dense_case(*shape)[:9])
    term = (J, UA, UG, W, F, Cc, Binv)
    whole = V.kron_draws_inf([term], [Z], [E])
    assert whole.shape == (ns, nb, nc) and whole.dtype == torch.float32
    assert torch.equal(whole, V.kron_draws_inf([term], [Z], [E]))
    subset = [1, 3, 12]
    assert torch.equal(V.kron_draws_inf([(J[subset].contiguous(), *term[1:])], [Z], [E]), whole[:, subset])
    assert torch.equal(V.kron_draws_inf([term], [Z[1:4]], [E[1:4]]), whole[1:4])
    halves = [V.kron_draws_inf([term], [Z[s0:s0 + 3]], [E[s0:s0 + 3]]) for s0 in (0, 3)]
    assert torch.equal(torch.cat(halves), whole)
    cov_terms, zs = V._inf_draw_operands([term], [Z], [E], "test")
    _, jobs, _, _ = V._inf_dense_jobs(cov_terms, "test", None)
    need = N.inf_draws_workspace_bytes([N.InfDrawJob(N.InfCovJob(*jobs[0]), *V._inf_draw_at(zs[0], 0))], nb, nc, ns)
    assert need > 0
    assert torch.equal(V.kron_draws_inf([term], [Z], [E], max_workspace_bytes=need - 1), whole)


def test_zero_low_rank_part_gives_the_bits_of_kron_draws_outer(hip_device):
    """F = 0 and Binv = 0: the second term is exactly 0 and the first is kfac_glm_draws_outer's
    on the same a, Delta with identity K1, K2 and Z pre-multiplied by C in fp32 (one tile body,
    g-tile cut and reduce order; x * 1 and s - 0 are exact)."""
    from bnn_kfac_amd import variance as V
    shape = (20, 1, 65, 7, 9, 2, 3, 2)
    a, D, UA, UG, W, F, Cc, Binv, Z, E = _dev(hip_device, *C.outer_case(*shape)[:10])
    got = V.kron_draws_outer_inf([(a, D, UA, UG, W, torch.zeros_like(F), Cc, torch.zeros_like(Binv))], [Z], [E])
    eye = lambda n: torch.eye(n, device=hip_device)  # noqa: E731
    want = V.kron_draws_outer([(a, D, eye(21), eye(65))], [Cc * Z])
    assert bool(want.abs().max() > 0)
    assert torch.equal(got, want)


def test_nine_terms_fold_in_groups_of_eight(hip_device):
    from bnn_kfac_amd import variance as V
    shapes = [(4, 1, 3, 2, 2), (63, 1, 10, 5, 3), (9, 0, 10, 3, 3), (70, 1, 65, 4, 2), (12, 1, 4, 2, 3),
              (20, 1, 130, 3, 2), (33, 0, 31, 5, 7), (8, 1, 8, 8, 1), (64, 1, 64, 2, 2)]
    outer, dense, zs, es, ref, top = [], [], [], [], 0.0, 0.0
    for cols, ones, nG, ra, rg in shapes:
        a, D, *ops, Z, E, r, t = C.outer_case(cols, ones, nG, ra, rg, 3, 4, 2)
        ad, Dd, Jd, Zd, Ed, *opsd = _dev(hip_device, a, D, P.rows_of(a, ones, D), Z, E, *ops)
        outer.append((ad, Dd, *opsd))
        dense.append((Jd, *opsd))
        zs.append(Zd)
        es.append(Ed)
        ref, top = ref + r, top + t
    _check(V.kron_draws_outer_inf(outer, zs, es).cpu().numpy(), ref, top)
    _check(V.kron_draws_inf(dense, zs, es).cpu().numpy(), ref, top)


# ------------------------------------------------------------------ identities
def test_one_hot_draws_give_the_joint_covariance(hip_device):
    """[Z; E] = the identity over the nA*nG + r coordinates of a consistent posterior: F is
    J A, so F^T F = J P^-1 J^T over all sample pairs (deterministic)."""
    from bnn_kfac_amd import variance as V
    nA, nG, ra, rg, s, n = 6, 4, 3, 2, 3.0, 0.25
    nb, nc, r, K = 5, 4, ra * rg, nA * nG
    UA, UG, lam, corr, Pm = P.posterior(nA, nG, ra, rg, s, n)
    W, F = P.woodbury_factors(UA, UG, lam, corr, s, n)
    Binv = np.linalg.inv(np.linalg.cholesky(np.eye(r) + P.woodbury_gram(UA, UG, lam, corr, s, n)[2]))
    rng = np.random.default_rng(3)
    a = rng.standard_normal((nb, nA - 1)).astype(np.float32)
    D = rng.standard_normal((nb, nc, nG)).astype(np.float32)
    J = P.rows_of(a, 1, D)
    f = lambda t: np.ascontiguousarray(t, dtype=np.float32)  # noqa: E731
    ops = _dev(hip_device, f(UA), f(UG), f(W), f(F), f(np.sqrt(W)), f(Binv))
    ad, Dd, Jd = _dev(hip_device, a, D, J)
    eye = torch.eye(K + r, device=hip_device)
    Z, E = eye[:, :K].reshape(K + r, nA, nG).contiguous(), eye[:, K:].contiguous()
    J64 = J.astype(np.float64).reshape(nb * nc, K)
    want = J64 @ np.linalg.inv(Pm) @ J64.T
    blocks = np.stack([want[b * nc:(b + 1) * nc, b * nc:(b + 1) * nc] for b in range(nb)])
    for draws, cov in ((V.kron_draws_outer_inf([(ad, Dd, *ops)], [Z], [E]),
                        V.kron_covariance_outer_inf([(ad, Dd, *ops[:4])])),
                       (V.kron_draws_inf([(Jd, *ops)], [Z], [E]), V.kron_covariance_inf([(Jd, *ops[:4])]))):
        Fd = draws.view(K + r, nb * nc).double().cpu().numpy()
        joint = Fd.T @ Fd
        _close(joint, want)                                   # every sample pair: the joint consistency
        got = np.stack([joint[b * nc:(b + 1) * nc, b * nc:(b + 1) * nc] for b in range(nb)])
        _close(got, cov.double().cpu().numpy())               # the covariance calls, on the same inputs
        _close(cov.double().cpu().numpy(), blocks)
    # teeth: without the eps rows the covariance lacks a term
    assert np.abs(Fd[:K].T @ Fd[:K] - want).max() > 1e-3 * np.abs(want).max()


@pytest.mark.parametrize("shape", [(63, 1, 10, 5, 3, 3, 10, 2), (20, 0, 130, 3, 2, 3, 33, 5)], ids=C.IDS)
def test_factored_agrees_with_dense_on_rank_one_rows(hip_device, shape):
    """Two fp32 evaluations, each within SCALE * top of the fp64 value: they differ by at most
    twice that."""
    from bnn_kfac_amd import variance as V
    a, D, *ops, Z, E, _, top = C.outer_case(*shape)
    ad, Dd, Jd, Zd, Ed, *opsd = _dev(hip_device, a, D, P.rows_of(a, shape[1], D), Z, E, *ops)
    outer = V.kron_draws_outer_inf([(ad, Dd, *opsd)], [Zd], [Ed]).cpu().numpy()
    dense = V.kron_draws_inf([(Jd, *opsd)], [Zd], [Ed]).cpu().numpy()
    print("max diff / top =", float(np.abs(outer - dense).max() / top))
    np.testing.assert_allclose(outer, dense, rtol=2 * C.SCALE, atol=2 * C.SCALE * top)


# ------------------------------------------------------------------ a draw is a weight sample
def _fit_inf(dev, net, make_x, loss_of, rank, batch=64):
    """test_gpu_glm_inf.py's fit for any loss: KFAC factors, EFB on their eigenbases,
    INF.update(rank).  Returns (net on dev, its fp64 CPU copy, inf)."""
    from bnn_kfac_amd.curvatures import EFB, INF, KFAC
    net64 = copy.deepcopy(net).double()  # (before KFAC hooks the modules)
    net = net.to(dev)
    kfac = KFAC(net)

    def backward():
        out = net(make_x(batch))
        net.zero_grad()
        loss_of(out).backward()

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


def _linear_in_weights(name, dev):
    if name == "linear":
        return nn.Sequential(nn.Linear(12, 5)), lambda n: torch.randn(n, 12, device=dev)
    return nn.Sequential(nn.Conv2d(2, 3, 3), nn.Flatten()), lambda n: torch.randn(n, 2, 6, 6, device=dev)


@pytest.mark.parametrize("name", ["linear", "conv"])
def test_draw_is_a_weight_sample(hip_device, name):
    """inf_posterior_sample's weights written into the (fp64) model, and the same (z, e) through
    glm_predictive_mc: the model is linear in its weights, so the forward difference is the draw
    (orders, the bias row, the sign of the low-rank part and e's place end to end)."""
    from bnn_kfac_amd.variance import glm_predictive_mc, inf_draw_factors, inf_posterior_sample
    torch.manual_seed(0)
    net, make_x = _linear_in_weights(name, hip_device)
    net, net64, inf = _fit_inf(hip_device, net, make_x, S.categorical_loss, rank=6)
    layer, layer64 = net[0], net64[0]
    x = make_x(5)
    UA, UG, _, _ = inf.state[layer]
    (nA, ra), (nG, rg) = UA.shape, UG.shape
    g = torch.Generator(device=hip_device).manual_seed(3)
    z = torch.randn(2, nA, nG, generator=g, device=hip_device)
    e = torch.randn(2, ra * rg, generator=g, device=hip_device)
    factors = inf_draw_factors(inf, ADD, MULTIPLY)[layer]
    sample = inf_posterior_sample(*(t.double().cpu() for t in factors), z.double().cpu(), e.double().cpu())
    assert sample.shape == (2, nA, nG)
    x64 = x.double().cpu()
    with torch.no_grad():
        base = net64(x64)
        want = []
        weight, bias = layer64.weight.clone(), layer64.bias.clone()
        for s in range(2):
            layer64.weight.copy_(weight + sample[s, :nA - 1].t().reshape(weight.shape))
            layer64.bias.copy_(bias + sample[s, nA - 1])
            want.append((net64(x64) - base).numpy())
        layer64.weight.copy_(weight)
        layer64.bias.copy_(bias)
    want = np.stack(want)
    assert np.abs(want).max() > 0
    before = {m: tuple(t.clone() for t in v) for m, v in inf.state.items()}
    for route in ("factored", "dense"):
        res = glm_predictive_mc(inf, x, n_draws=2, z=[(z, e)], jacobians=route, return_draws=True, add=ADD,
                                multiply=MULTIPLY)
        assert res.draws.shape == want.shape and not inf.inv_state
        print(name, route, end=": ")
        _close(res.draws.cpu().numpy(), want)
        np.testing.assert_allclose(res.logits.cpu().numpy(), base.numpy(), rtol=1e-4,
                                   atol=1e-5 * float(base.abs().max()))
    for m, v in inf.state.items():
        assert all(torch.equal(t, b) for t, b in zip(v, before[m]))


# ------------------------------------------------------------------ end to end
def _e2e_nets():
    from models_for_tests import BaseNet750, mlp
    return {"mlp": (mlp, (784,), 512, lambda m: [m[0], m[2]]),
            "basenet750": (BaseNet750, (1, 28, 28), 32, lambda m: [m.conv1, m.conv2, m.fc1])}


@pytest.fixture(scope="module")
def e2e(hip_device):
    """name -> (inf, x, layers, z pairs, fp64 logits, fp64 draws (S, N, nc)): the fit of
    test_gpu_glm_inf.py (KFAC -> EFB -> INF.update(rank=6)) and the reference, once."""
    from test_gpu_glm_inf import _fit_inf as fit_inf
    cache = {}

    def get(name):
        if name in cache:
            return cache[name]
        make, in_shape, batch, pick = _e2e_nets()[name]
        torch.manual_seed(0)
        net, net64, inf = fit_inf(hip_device, make(), in_shape, 10, batch)
        x = torch.rand(5, *in_shape, device=hip_device)
        layers = pick(net)
        assert list(inf.state) == layers
        g = torch.Generator(device=hip_device).manual_seed(5)
        z = []
        for layer in layers:
            UA, UG = inf.state[layer][:2]
            zl = torch.randn(3, UA.shape[0], UG.shape[0], generator=g, device=hip_device)
            z.append((zl, torch.randn(3, UA.shape[1] * UG.shape[1], generator=g, device=hip_device)))
        logits, rows = S.fp64_rows(net64, pick(net64), x.cpu())
        draws = 0.0
        for layer, M, (zl, el) in zip(layers, rows, z):
            UA, UG, lam, corr = (t.double().cpu().numpy() for t in inf.state[layer])
            nA, nG = UA.shape[0], UG.shape[0]
            W, F = P.woodbury_factors(UA, UG, lam, corr, MULTIPLY, ADD)
            vtv = P.woodbury_gram(UA, UG, lam, corr, MULTIPLY, ADD)[2]
            Binv = np.linalg.inv(np.linalg.cholesky(np.eye(len(lam)) + vtv))
            first, sg, se = C.dense_parts(M.reshape(M.shape[0], M.shape[1], nA * nG), nA, nG, UA, UG, W, F,
                                          np.sqrt(W), Binv, zl.double().cpu().numpy(), el.double().cpu().numpy())
            print(name, layer.__class__.__name__, (nA, nG), "||vtv|| =", float(np.linalg.norm(vtv, 2)),
                  "max|first| =", float(np.abs(first).max()), "max|second| =", float(np.abs(sg + se).max()))
            draws = draws + first - sg - se
        cache[name] = (inf, x, layers, z, logits, draws)
        return cache[name]
    return get


@pytest.fixture
def deterministic_convolutions():
    """(test_gpu_glm_mc.py's: the bitwise comparison of two glm_predictive_mc calls is about this
    project's code, so it runs in torch's deterministic mode.)"""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = before


@pytest.mark.parametrize("route", ["factored", "dense"])
@pytest.mark.parametrize("name", ["mlp", "basenet750"])
def test_glm_predictive_mc_inf_end_to_end(hip_device, deterministic_convolutions, e2e, name, route):
    from bnn_kfac_amd.variance import glm_predictive_mc
    inf, x, layers, z, logits, draws = e2e(name)
    probs, expected, entropy, mi = MC.softmax_ref(logits, draws)
    kw = dict(n_draws=3, chunk=2, jacobians=route, z=z, add=ADD, multiply=MULTIPLY)
    res = glm_predictive_mc(inf, x, return_draws=True, **kw)   # needs no invert
    assert not inf.inv_state
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
    lean = glm_predictive_mc(inf, x, **kw)
    assert lean.draws is None
    per_draw = 4 * sum(zl[0].numel() + el[0].numel() for zl, el in z)
    cut = glm_predictive_mc(inf, x, max_draw_bytes=2 * per_draw, return_draws=True, **kw)
    assert torch.equal(cut.draws, res.draws)
    for other in (lean, cut):
        for a, b in zip(other[:5], res[:5]):
            assert torch.equal(a, b)


def test_glm_predictive_mc_inf_draws_its_own_z(hip_device, e2e):
    """The documented order of the random numbers: per draw chunk, the layers in order, Z then E."""
    from bnn_kfac_amd.variance import glm_predictive_mc
    inf, x, layers, z, _, _ = e2e("mlp")
    g1 = torch.Generator(device=hip_device).manual_seed(9)
    drawn = glm_predictive_mc(inf, x, n_draws=4, chunk=5, generator=g1, return_draws=True, add=ADD,
                              multiply=MULTIPLY)
    assert drawn.draws.shape == (4, 5, 10)
    np.testing.assert_allclose(drawn.probs.sum(dim=1).cpu().numpy(), 1.0, rtol=0, atol=1e-6)
    assert bool((drawn.mutual_information >= 0).all()) and bool((drawn.mutual_information > 0).any())
    g2 = torch.Generator(device=hip_device).manual_seed(9)
    same = []
    for zl, el in z:
        zz = torch.randn(4, *zl.shape[1:], generator=g2, device=hip_device)
        same.append((zz, torch.randn(4, el.shape[1], generator=g2, device=hip_device)))
    again = glm_predictive_mc(inf, x, n_draws=4, chunk=5, z=same, return_draws=True, add=ADD, multiply=MULTIPLY)
    assert torch.equal(again.draws, drawn.draws)
    with pytest.raises(ValueError):
        glm_predictive_mc(inf, x, n_draws=3, z=same, add=ADD, multiply=MULTIPLY)  # four draws given


def test_glm_predictive_mc_inf_regression(hip_device):
    """nc = 1: the draws are the output; the statistics are the degenerate ones."""
    from bnn_kfac_amd.variance import glm_predictive_inf, glm_predictive_mc
    make, xshape, loss_of = S.small_nets()["regression"]
    torch.manual_seed(0)
    make_x = lambda n: torch.randn(n, *xshape, device=hip_device)  # noqa: E731
    net, _, inf = _fit_inf(hip_device, make(), make_x, loss_of, rank=4)
    x = make_x(5)
    res = glm_predictive_mc(inf, x, n_draws=4, generator=torch.Generator(device=hip_device).manual_seed(1),
                            return_draws=True, add=ADD, multiply=MULTIPLY)
    assert res.draws.shape == (4, 5, 1) and bool(res.draws.abs().max() > 0)
    assert bool(torch.isfinite(res.draws).all())
    assert torch.equal(res.probs, torch.ones(5, 1, device=hip_device))
    for t in (res.entropy, res.expected_entropy, res.mutual_information):
        assert not bool(t.any())
    assert torch.equal(res.logits, glm_predictive_inf(inf, x, ADD, MULTIPLY, jacobians="factored")[0])


def test_kfac_and_efb_keep_their_bits_with_the_new_keywords(hip_device):
    from bnn_kfac_amd.curvatures import EFB
    from bnn_kfac_amd.variance import glm_predictive_mc
    torch.manual_seed(0)
    make_x = lambda n: torch.randn(n, 12, device=hip_device)  # noqa: E731
    net, _, kfac = S.fit(hip_device, nn.Sequential(nn.Linear(12, 5)), make_x, S.categorical_loss)
    layer = net[0]
    efb = EFB(net, {layer: [t.clone() for t in kfac.state[layer]]})
    for _ in range(2):
        out = net(make_x(64))
        net.zero_grad()
        S.categorical_loss(out).backward()
        efb.update(64)
    kfac.invert(0.04, 200.0)
    efb.invert(0.04, 200.0)
    x = make_x(5)
    z = [torch.randn(3, 13, 5, device=hip_device)]
    for curv in (kfac, efb):
        for route in ("factored", "dense"):
            plain = glm_predictive_mc(curv, x, n_draws=3, z=z, jacobians=route, return_draws=True)
            keyed = glm_predictive_mc(curv, x, n_draws=3, z=z, jacobians=route, return_draws=True, add=0.,
                                      multiply=1.)
            other = glm_predictive_mc(curv, x, n_draws=3, z=z, jacobians=route, return_draws=True, add=7.,
                                      multiply=3.)   # (INF's arguments: not read here)
            for a, b, c in zip(plain, keyed, other):
                assert torch.equal(a, b) and torch.equal(a, c)
