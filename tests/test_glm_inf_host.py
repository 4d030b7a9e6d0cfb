"""CPU: the host side of the INF GLM predictive -- the cases file's references against
J P^-1 J^T with a dense fp64 inverse, the recorded fp32-chain error behind the GPU tolerance,
the ValueErrors that fire before any device call, and, through a numpy double of the two device
calls (host_double_inf.py), the wiring of glm_predictive_inf, inf_covariance_factors and
inf_log_det."""
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

import glm_inf_cases as C
import host_double_inf


# ------------------------------------------------------------------ the references
@pytest.mark.parametrize("nA,nG,ra,rg", [(6, 4, 3, 2), (5, 3, 5, 3), (7, 1, 2, 1), (4, 5, 1, 4)])
def test_reference_formulas_equal_the_dense_inverse(nA, nG, ra, rg):
    """The formulas the cases are built from, on a consistent (U, Lambda, D, s, n): both equal
    J P^-1 J^T with P inverted densely in fp64."""
    s, n = 3.0, 0.25
    UA, UG, lam, corr, P = C.posterior(nA, nG, ra, rg, s, n)
    assert (corr < 0).any()                       # the clip at 0 is exercised
    W, F = C.woodbury_factors(UA, UG, lam, corr, s, n)
    rng = np.random.default_rng(nA)
    nb, nc = 3, 4
    J = rng.standard_normal((nb, nc, nA * nG))
    want = np.einsum("bck,kl,bdl->bcd", J, np.linalg.inv(P), J)
    first, second = C.dense_terms(J, nA, nG, UA, UG, W, F)
    np.testing.assert_allclose(first - second, want, rtol=1e-11, atol=1e-12 * np.abs(want).max())
    # a Linear layer's rows abar delta^T, never formed by the factored formula
    a, D = rng.standard_normal((nb, nA - 1)), rng.standard_normal((nb, nc, nG))
    rows = np.einsum("bi,bcg->bcig", np.concatenate([a, np.ones((nb, 1))], axis=1), D).reshape(nb, nc, -1)
    want = np.einsum("bck,kl,bdl->bcd", rows, np.linalg.inv(P), rows)
    first, second = C.outer_terms(a, 1, D, UA, UG, W, F)
    np.testing.assert_allclose(first - second, want, rtol=1e-11, atol=1e-12 * np.abs(want).max())


def test_case_references_are_the_formulas_on_the_case_inputs():
    for shape in C.OUTER_SHAPES[:4]:
        a, D, UA, UG, W, F, ref, top = C.outer_case(*shape)
        assert ref.shape == (shape[5], shape[6], shape[6]) and not ref.flags.writeable
        assert UA.shape == (shape[0] + shape[1], shape[3]) and UG.shape == (shape[2], shape[4])
        assert F.shape == (shape[3] * shape[4],) * 2 and np.array_equal(F, np.tril(F))
        assert float(W[0].max()) == float(np.float32(1e-2)) and float(W[-1].min()) == float(np.float32(1e2))
        first, second = C.dense_terms(C.rows_of(a, shape[1], D), shape[0] + shape[1], shape[2], UA, UG, W, F)
        # (rows_of rounds each product to fp32: 6e-8 relative per entry)
        np.testing.assert_allclose(first - second, ref, rtol=0, atol=1e-6 * top)
        assert top <= 10 * np.abs(ref).max()
    for shape in C.DENSE_SHAPES:
        J, UA, UG, W, F, ref, top = C.dense_case(*shape)
        assert ref.shape == (shape[4], shape[5], shape[5]) and top <= 10 * np.abs(ref).max()


def test_recorded_fp32_chain_error_and_scale():
    """The GPU tolerance's record: the stage chain in numpy fp32 on every shape."""
    worst = C.fp32_chain_error()
    print("fp32 chain: worst err / max|first term| =", worst, "recorded", C.MEASURED_FP32_CHAIN)
    assert worst <= 2 * C.MEASURED_FP32_CHAIN          # (BLAS summation orders differ by machine)
    assert C.SCALE == max(1e-5, 4 * C.MEASURED_FP32_CHAIN) and 4 * worst <= C.SCALE


def test_integer_cases_stay_exact_in_fp32():
    for case in (C.int_outer_case(), C.int_dense_case()):
        *inputs, want, bound = case
        assert 0 < bound <= C.EXACT and np.abs(want).max() > 0 and want.dtype == np.int64
        for t in inputs:
            assert np.array_equal(t, np.round(t)) and np.abs(t).max() <= 3
        UA, UG, W, F = inputs[-4:]
        assert set(np.unique(W)) == {1.0, 2.0, 3.0} and not np.array_equal(W[:3, :3], W[:3, :3].T)
        assert (np.abs(UA) > 0).sum(0).max() <= 3 and (np.abs(UG) > 0).sum(0).max() <= 3
        assert (np.abs(F) > 0).sum(1).max() <= 3


# ------------------------------------------------------------------ argument errors
def test_value_errors_fire_before_any_device_call():
    """Shapes are judged on the host: CPU tensors never reach the device requirement."""
    from bnn_kfac_amd.variance import kron_covariance_inf, kron_covariance_outer_inf
    nA, nG, ra, rg, nb, nc = 6, 4, 3, 2, 2, 3
    r = ra * rg
    J, a, D = torch.zeros(nb, nc, nA * nG), torch.zeros(nb, nA - 1), torch.zeros(nb, nc, nG)
    UA, UG, W, F = torch.ones(nA, ra), torch.ones(nG, rg), torch.ones(nA, nG), torch.eye(r)
    bad = [dict(W=torch.ones(nG, nA)), dict(W=torch.ones(nA * nG)), dict(W=torch.ones(1, nA, nG)),
           dict(F=torch.eye(r + 1)), dict(F=torch.ones(r)), dict(F=torch.ones(r, r - 1)),
           dict(UA=torch.ones(nA)), dict(UG=torch.ones(nG, 0)), dict(UA=torch.ones(nA + 2, ra))]
    for change in bad:
        ops = {**dict(UA=UA, UG=UG, W=W, F=F), **change}
        with pytest.raises(ValueError):
            kron_covariance_inf([(J, ops["UA"], ops["UG"], ops["W"], ops["F"])])
        with pytest.raises(ValueError):
            kron_covariance_outer_inf([(a, D, ops["UA"], ops["UG"], ops["W"], ops["F"])])
    with pytest.raises(ValueError, match="at most 32"):
        kron_covariance_inf([(torch.zeros(nb, 33, nA * nG), UA, UG, W, F)])
    with pytest.raises(ValueError, match="at most 32"):
        kron_covariance_outer_inf([(a, torch.zeros(nb, 33, nG), UA, UG, W, F)])
    with pytest.raises(ValueError, match="no terms"):
        kron_covariance_inf([])
    with pytest.raises(ValueError, match="no terms"):
        kron_covariance_outer_inf([])
    with pytest.raises(ValueError):
        kron_covariance_inf([(J[:, :, :-1], UA, UG, W, F)])
    with pytest.raises(ValueError, match="same"):
        kron_covariance_inf([(J, UA, UG, W, F), (J[:1], UA, UG, W, F)])
    with pytest.raises(ValueError):
        kron_covariance_outer_inf([(a[:1], D, UA, UG, W, F)])
    with pytest.raises(ValueError):
        kron_covariance_outer_inf([(a[:, :-2], D, UA, UG, W, F)])
    with pytest.raises(ValueError):
        kron_covariance_outer_inf([(torch.zeros(nb, 2, nA - 1), D, UA, UG, W, F)])
    # valid shapes on the CPU get as far as the device requirement, and no further
    from bnn_kfac_amd._native import NativeError
    with pytest.raises(NativeError):
        kron_covariance_inf([(J, UA, UG, W, F)])
    with pytest.raises(NativeError):
        kron_covariance_outer_inf([(a, D, UA, UG, W, F)])
    from bnn_kfac_amd.variance import glm_predictive_inf
    with pytest.raises(ValueError, match="jacobians"):
        glm_predictive_inf(types.SimpleNamespace(state={}, model=nn.Linear(2, 2)), torch.zeros(1, 2),
                           jacobians="nope")


# ------------------------------------------------------------------ through the double
def _state(layer_dims, seed=0):
    """INF.update's state entries (U_A, U_G, Lambda, D) in fp32 for [(nA, nG, ra, rg)]."""
    out = []
    for k, (nA, nG, ra, rg) in enumerate(layer_dims):
        UA, UG, lam, corr, _ = C.posterior(nA, nG, ra, rg, 1.0, 1.0, seed=seed + k)
        out.append(tuple(torch.from_numpy(t.astype(np.float32)) for t in (UA, UG, lam, corr)))
    return out


def _dense_precision(entry, s, n):
    UA, UG, lam, corr = (t.double().numpy() for t in entry)
    U = np.kron(UA, UG)
    return s * (U @ np.diag(lam) @ U.T + np.diag(np.maximum(corr, 0.0))) + n * np.eye(U.shape[0])


@pytest.fixture
def conv_net():
    torch.manual_seed(0)
    net = nn.Sequential(nn.Conv2d(1, 2, 3), nn.ReLU(), nn.Flatten(), nn.Linear(2 * 4 * 4, 3))
    layers = [net[0], net[3]]
    entries = _state([(10, 2, 4, 2), (33, 3, 5, 2)])
    inf = types.SimpleNamespace(model=net, state=dict(zip(layers, entries)))
    return net, layers, inf, torch.rand(5, 1, 6, 6)


@pytest.mark.parametrize("route", ["dense", "factored"])
def test_glm_predictive_inf_wires_linear_and_conv_layers(monkeypatch, conv_net, route):
    from bnn_kfac_amd.variance import glm_predictive_inf, output_jacobians
    host_double_inf.install(monkeypatch)
    net, layers, inf, x = conv_net
    add, multiply = [0.5, 0.25], [2.0, 3.0]
    logits, cov = glm_predictive_inf(inf, x, add, multiply, chunk=2, jacobians=route)
    assert logits.shape == (5, 3) and cov.shape == (5, 3, 3) and cov.dtype == torch.float32
    with torch.no_grad():
        np.testing.assert_allclose(logits.numpy(), net(x).numpy(), rtol=1e-5, atol=1e-6)
    _, Js = output_jacobians(net, layers, x)
    want = 0.0
    for k, (layer, J) in enumerate(zip(layers, Js)):
        Pinv = np.linalg.inv(_dense_precision(inf.state[layer], multiply[k], add[k]))
        Jn = J.double().numpy()
        want = want + np.einsum("bck,kl,bdl->bcd", Jn, Pinv, Jn)
    # (W and F reach the calls in fp32; vtv is rounded to fp32 on the way)
    np.testing.assert_allclose(cov.numpy(), want, rtol=0, atol=1e-5 * np.abs(want).max())
    names = [c[0] for c in host_double_inf.CALLS]
    if route == "dense":
        assert names == ["inf_cov"] * 3 and all(c[1] == 2 for c in host_double_inf.CALLS)
    else:  # per chunk: the Linear layer through the outer call, the Conv2d rows through the dense one
        assert names == ["inf_cov_outer", "inf_cov"] * 3 and all(c[1] == 1 for c in host_double_inf.CALLS)
    assert [c[2] for c in host_double_inf.CALLS[::len(names) // 3]] == [2, 2, 1]
    # one layer at a time adds up; scalars are per-layer lists of equal entries
    parts = [glm_predictive_inf(inf, x, add, multiply, layers=[layer], jacobians=route)[1] for layer in layers]
    np.testing.assert_allclose((parts[0] + parts[1]).numpy(), cov.numpy(), rtol=0, atol=1e-6 * np.abs(want).max())
    same = glm_predictive_inf(inf, x, 0.5, 2.0, jacobians=route)[1]
    lists = glm_predictive_inf(inf, x, [0.5, 0.5], [2.0, 2.0], jacobians=route)[1]
    assert torch.equal(same, lists)


def test_jobs_fold_in_groups_of_eight_and_samples_chunk(monkeypatch):
    from bnn_kfac_amd.variance import kron_covariance_inf, kron_covariance_outer_inf
    host_double_inf.install(monkeypatch)
    t = lambda *arrays: tuple(torch.from_numpy(np.array(v)) for v in arrays)  # noqa: E731
    J, UA, UG, W, F, ref, top = C.dense_case(5, 3, 2, 2, 2, 4)
    got = kron_covariance_inf([t(J, UA, UG, W, F)] * 9)
    assert host_double_inf.CALLS == [("inf_cov", 8, 2, False), ("inf_cov", 1, 2, True)]
    np.testing.assert_allclose(got.numpy(), 9 * ref, rtol=0, atol=1e-5 * 9 * top)
    a, D, UA, UG, W, F, ref, top = C.outer_case(63, 1, 10, 5, 3, 3, 10)
    host_double_inf.CALLS.clear()
    terms = [t(a, D, UA, UG, W, F)]
    got = kron_covariance_outer_inf(terms, max_workspace_bytes=1024)   # the double: 1024 per sample
    assert host_double_inf.CALLS == [("inf_cov_outer", 1, 1, False)] * 3
    np.testing.assert_allclose(got.numpy(), ref, rtol=0, atol=1e-5 * top)
    with pytest.raises(ValueError, match="workspace"):
        kron_covariance_outer_inf(terms, max_workspace_bytes=1023)
    # strided operands go through without a copy and give the same numbers
    wide = torch.zeros(3, 70)
    wide[:, 2:65] = terms[0][0]
    UAp = torch.zeros(64, 9)[:, :5]
    UAp.copy_(terms[0][2])
    again = kron_covariance_outer_inf([(wide[:, 2:65], terms[0][1], UAp, *terms[0][3:])])
    assert torch.equal(again, kron_covariance_outer_inf(terms))
    # an expanded tensor (row stride 0 < its width) is copied, not handed over with a wrong ld
    row = terms[0][3][:1]                               # (1, rg)
    UGx = row.expand(10, 3)
    assert UGx.stride() == (0, 1)
    expanded = kron_covariance_outer_inf([(*terms[0][:3], UGx, *terms[0][4:])])
    assert torch.equal(expanded, kron_covariance_outer_inf([(*terms[0][:3], UGx.contiguous(), *terms[0][4:])]))


def test_inf_covariance_factors_reads_the_state_and_leaves_it(monkeypatch):
    from bnn_kfac_amd.variance import inf_covariance_factors
    host_double_inf.install(monkeypatch)
    entries = _state([(6, 4, 3, 2), (5, 3, 5, 3)])
    inf = types.SimpleNamespace(state={"l0": entries[0], "l1": entries[1]}, model=None)
    before = {k: tuple(t.clone() for t in v) for k, v in inf.state.items()}
    assert any(bool((v[3] < 0).any()) for v in before.values())
    add, multiply = [0.25, 1.5], [3.0, 0.5]
    got = inf_covariance_factors(inf, add, multiply)
    assert list(got) == ["l0", "l1"]
    for k, name in enumerate(got):
        UA, UG, W, F = got[name]
        ua, ug, lam, corr = (t.double().numpy() for t in before[name])
        Wn, Fn = C.woodbury_factors(ua, ug, lam, corr, multiply[k], add[k])
        assert W.dtype == F.dtype == torch.float32 and W.shape == Wn.shape and F.shape == Fn.shape
        assert W.is_contiguous() and F.is_contiguous()
        # W: fp64 arithmetic on the fp32 state, one rounding to fp32
        assert np.array_equal(W.numpy(), Wn.astype(np.float32))
        np.testing.assert_allclose(F.numpy(), Fn, rtol=0, atol=1e-5 * np.abs(Fn).max())
        assert torch.equal(UA, before[name][0]) and torch.equal(UG, before[name][1])
        for t, b in zip(inf.state[name], before[name]):
            assert torch.equal(t, b)               # the negative corrections are still there
    only = inf_covariance_factors(inf, add, multiply, layers=["l1"])
    assert list(only) == ["l1"] and torch.equal(only["l1"][3], got["l1"][3])  # its own damping: index 1
    with pytest.raises(np.linalg.LinAlgError):     # a clipped correction and no additive damping
        inf_covariance_factors(inf, 0.0, 1.0)
    with pytest.raises(np.linalg.LinAlgError):
        inf_covariance_factors(inf, -1.0, 0.1)
    with pytest.raises(AssertionError):
        inf_covariance_factors(types.SimpleNamespace(state={}, model=None), 1.0, 1.0)


def test_closed_form_is_exact_where_the_ported_sampler_is_not(monkeypatch):
    """INF.sampler / pre_sampler (the reference's, ported literally) are linear in the draw X:
    sample = A X, so the sampler's covariance is A A^T.  On a 6 x 4 layer with ra = 3, rg = 2 it
    is NOT P^-1 (the INF section: the reshape of an i*nG + g vector as (nG, nA),
    and a Cholesky factor where a symmetric root is needed), while the closed form is P^-1 to
    rounding.  INF.sample is left as the parity-tested port; this records the difference."""
    from bnn_kfac_amd.curvatures import INF
    host_double_inf.install(monkeypatch)
    nA, nG, ra, rg, s, n = 6, 4, 3, 2, 3.0, 0.25
    UA, UG, lam, corr, P = C.posterior(nA, nG, ra, rg, s, n)
    Pinv = np.linalg.inv(P)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))  # noqa: E731
    c = np.sqrt(1.0 / (s * np.maximum(corr, 0.0) + n))
    pre = INF.pre_sampler(t(UA), t(UG), t(np.sqrt(s * lam)), t(c))
    columns = []
    for k in range(nA * nG):
        def unit(size, device=None, dtype=None, k=k):
            z = torch.zeros(size, dtype=dtype)
            z[k] = 1
            return z
        monkeypatch.setattr(torch, "randn", unit)
        columns.append(INF.sampler(t(UA), t(UG), t(c), pre).double().numpy())
    A = np.stack(columns, axis=1)
    off = np.abs(A @ A.T - Pinv).max() / np.abs(Pinv).max()
    W, F = C.woodbury_factors(UA, UG, lam, corr, s, n)
    first, second = C.dense_terms(np.eye(nA * nG)[None], nA, nG, UA, UG, W, F)
    exact = np.abs(first - second - Pinv).max() / np.abs(Pinv).max()
    print("sampler covariance off by", off, "x max|P^-1|; closed form off by", exact)
    assert off > 1.0 and exact < 1e-14


def test_inf_log_det_equals_the_dense_slogdet(monkeypatch):
    from bnn_kfac_amd.variance import inf_log_det
    host_double_inf.install(monkeypatch)
    entries = _state([(6, 4, 3, 2), (5, 3, 5, 3), (7, 1, 2, 1)])
    inf = types.SimpleNamespace(state=dict(enumerate(entries)), model=None)
    for add, multiply in ((0.25, 3.0), ([0.25, 1.5, 1e-3], [3.0, 0.5, 200.0])):
        got = inf_log_det(inf, add, multiply)
        assert got.dim() == 0 and got.dtype == torch.float64
        want = 0.0
        for k, entry in enumerate(entries):
            n, s = (add[k], multiply[k]) if isinstance(add, list) else (add, multiply)
            sign, logdet = np.linalg.slogdet(_dense_precision(entry, s, n))
            assert sign > 0
            want += logdet
        np.testing.assert_allclose(float(got), want, rtol=1e-6)
