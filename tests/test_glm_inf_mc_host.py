"""CPU: the host side of the INF Monte-Carlo GLM predictive -- the mathematics of the exact draw
(inf_posterior_sample's linear map A satisfies A A^T = P^-1; the factored and the rows-given logit
formulas equal J vec(x)), its teeth, the caps and integer bounds of every generator of
glm_inf_mc_cases, the recorded fp32 chain error behind the GPU tolerance, the layout of
kfac_inf_draw_job / kfac_inf_draw_outer_job against the header, argument validation before any
launch, and glm_predictive_mc's argument errors under an INF.  No GPU calls."""
import ctypes

import numpy as np
import pytest
import torch

import glm_inf_cases as P
import glm_inf_mc_cases as C
from abi_layout import c_layout

OUT, WS = 1 << 16, 1 << 17  # (pointers are never dereferenced: validation precedes any launch)
POSTERIORS = [(6, 4, 3, 2, 3.0, 0.25), (5, 3, 2, 3, 1.0, 1.0), (4, 7, 4, 1, 0.5, 2.0), (3, 3, 3, 3, 10.0, 0.1)]


def _consistent(nA, nG, ra, rg, s, n):
    """(UA, UG, W, F, C, Binv) fp64 of a consistent posterior and its dense precision P."""
    UA, UG, lam, corr, Pm = P.posterior(nA, nG, ra, rg, s, n)
    w, sigma, vtv = P.woodbury_gram(UA, UG, lam, corr, s, n)
    Binv = np.linalg.inv(np.linalg.cholesky(np.eye(len(lam)) + vtv))
    W = w.reshape(nA, nG)
    return (UA, UG, W, Binv * sigma[None, :], np.sqrt(W), Binv), Pm


def _torch_map(ops, nA, nG, r):
    """The linear map of bnn_kfac_amd.variance.inf_posterior_sample: column k of A is the draw
    from the k-th unit vector of [vec(Z); eps]."""
    from bnn_kfac_amd.variance import inf_posterior_sample
    n = nA * nG
    eye = torch.eye(n + r, dtype=torch.float64)
    x = inf_posterior_sample(*(torch.from_numpy(np.ascontiguousarray(t)) for t in ops),
                             eye[:, :n].reshape(n + r, nA, nG), eye[:, n:].contiguous())
    assert x.shape == (n + r, nA, nG) and x.dtype == torch.float64
    return x.reshape(n + r, n).t().numpy()


@pytest.mark.parametrize("post", POSTERIORS, ids=C.IDS)
def test_draw_has_the_posterior_covariance(post):
    nA, nG, ra, rg, s, n = post
    ops, Pm = _consistent(*post)
    cov = np.linalg.inv(Pm)
    A = _torch_map(ops, nA, nG, ra * rg)
    np.testing.assert_allclose(A, C.sample_linear_map(*ops), rtol=0, atol=1e-13 * np.abs(A).max())
    err = np.abs(A @ A.T - cov).max() / np.abs(cov).max()
    print(post, "|A A^T - P^-1| / max|P^-1| =", err)
    assert err <= 1e-12
    # teeth: without the eps part the covariance lacks a term; w for c is another distribution
    no_eps = A[:, :nA * nG]
    assert np.abs(no_eps @ no_eps.T - cov).max() / np.abs(cov).max() > 1e-3
    UA, UG, W, F, Cc, Binv = ops
    wrong = C.sample_linear_map(UA, UG, W, F, W, Binv)
    assert np.abs(wrong @ wrong.T - cov).max() / np.abs(cov).max() > 1e-3


@pytest.mark.parametrize("post", POSTERIORS, ids=C.IDS)
def test_logit_formulas_equal_the_jacobian_times_the_weight_draw(post):
    from bnn_kfac_amd.variance import inf_posterior_sample
    nA, nG, ra, rg, s, n = post
    ops, _ = _consistent(*post)
    rng = np.random.default_rng(5)
    nb, nc, ns = 3, 4, 5
    a = rng.standard_normal((nb, nA - 1))
    D = rng.standard_normal((nb, nc, nG))
    Z, E = rng.standard_normal((ns, nA, nG)), rng.standard_normal((ns, ra * rg))
    x = inf_posterior_sample(*(torch.from_numpy(np.ascontiguousarray(t)) for t in ops), torch.from_numpy(Z),
                             torch.from_numpy(E)).numpy()
    J = np.einsum("bi,bcg->bcig", C.abar_of(a, 1), D).reshape(nb, nc, nA * nG)
    want = np.einsum("bck,sk->sbc", J, x.reshape(ns, -1))
    first, sg, se = C.outer_parts(a, 1, D, *ops, Z, E)
    np.testing.assert_allclose(first - sg - se, want, rtol=0, atol=1e-12 * np.abs(want).max())
    first, sg, se = C.dense_parts(J, nA, nG, *ops, Z, E)
    np.testing.assert_allclose(first - sg - se, want, rtol=0, atol=1e-12 * np.abs(want).max())
    # teeth: the eps term is part of the logit draw
    assert np.abs(first - sg - want).max() > 1e-3 * np.abs(want).max()
    # dense rows that are not rank one
    J = rng.standard_normal((nb, nc, nA * nG))
    want = np.einsum("bck,sk->sbc", J, x.reshape(ns, -1))
    first, sg, se = C.dense_parts(J, nA, nG, *ops, Z, E)
    np.testing.assert_allclose(first - sg - se, want, rtol=0, atol=1e-12 * np.abs(want).max())


def test_every_generator_keeps_its_cap():
    for shape in C.OUTER_SHAPES:
        *inputs, ref, top = C.outer_case(*shape)
        assert ref.shape == (shape[7], shape[5], shape[6]) and 0 < top <= 10 * np.abs(ref).max()
        a, D, UA, UG, W, F, Cc, Binv, Z, E = inputs
        assert all(t.dtype == np.float32 for t in inputs)
        np.testing.assert_array_equal(Cc, np.sqrt(W.astype(np.float64)).astype(np.float32))
        d = lambda *ts: [t.astype(np.float64) for t in ts]  # noqa: E731
        first, sg, se = C.outer_parts(*d(a), shape[1], *d(D, UA, UG, W, F, Cc, Binv, Z, E))
        # the scaling: each half of the second term is a quarter of the first (fp32 rounding of F, Binv)
        np.testing.assert_allclose([np.abs(sg).max(), np.abs(se).max()], 0.25 * np.abs(first).max(), rtol=1e-5)
    for shape in C.DENSE_SHAPES:
        *inputs, ref, top = C.dense_case(*shape)
        assert ref.shape == (shape[6], shape[4], shape[5]) and 0 < top <= 10 * np.abs(ref).max()


def test_recorded_fp32_chain_error_and_scale():
    """The GPU tolerance's record: the stage chain in numpy fp32 on every shape."""
    worst, where = C.fp32_chain_error()
    print("fp32 chain: worst err / max(max|first|, max|second|) =", worst, "at", where, "recorded",
          C.MEASURED_FP32_CHAIN)
    assert worst <= 2 * C.MEASURED_FP32_CHAIN          # (BLAS summation orders differ by machine)
    assert C.SCALE == max(1e-5, 4 * C.MEASURED_FP32_CHAIN) and 4 * worst <= C.SCALE


@pytest.mark.parametrize("name", list(C.INT_CASES))
def test_integer_cases_stay_below_2_to_24(name):
    c = C.int_case(name)
    for j in c.jobs:
        for t in (j.a, j.D, j.Z, j.E, j.UA, j.UG, j.F, j.Binv):
            assert t.dtype == np.int64 and np.abs(t).max() <= 1
        assert set(np.unique(j.C)) <= {1, 2, 3} and np.array_equal(j.W, j.C * j.C)
    outer, dense = C.int_reference(c, "outer"), C.int_reference(c, "dense")
    assert outer.dtype == np.int64 and np.array_equal(outer, dense) and np.abs(outer).max() > 0
    for route in ("outer", "dense"):
        assert 0 < C.int_bound(c, route) < C.EXACT
    # the second term takes part in every case
    first_only = sum(np.einsum("sbg,bcg->sbc", np.matmul(C.abar_of(j.a, j.ones), j.C * j.Z), j.D) for j in c.jobs)
    assert not np.array_equal(first_only + (c.prefill if c.accumulate else 0), outer)


# ------------------------------------------------------------------ the C ABI
TAIL =("C", "Binv", "ldB", "Z", "ldZ", "E", "ldE")


@pytest.mark.parametrize("cname,pyname,rows", [("kfac_inf_draw_job", "InfDrawJob", "InfCovJob"),
                                               ("kfac_inf_draw_outer_job", "InfDrawOuterJob", "InfCovOuterJob")])
def test_inf_draw_struct_layout_matches_header(tmp_path, cname, pyname, rows):
    from bnn_kfac_amd import _native as N
    S = getattr(N, pyname)
    fields = ("rows",) + TAIL
    got = c_layout(tmp_path, cname, fields)
    assert [f for f, _ in S._fields_] == list(fields)
    assert got == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in fields]
    assert S.rows.offset == 0 and S.C.offset == ctypes.sizeof(getattr(N, rows))
    assert dict(S._fields_)["rows"] is getattr(N, rows)


def _dense_job(N, nA=5, nG=3, ra=2, rg=2):
    r = ra * rg
    rows = N.InfCovJob(1 << 12, nA * nG, nA, nG, 1 << 13, ra, ra, 1 << 14, rg, rg, 1 << 15, nA * nG, 1 << 16, r)
    return N.InfDrawJob(rows, 1 << 17, 1 << 18, r, 1 << 19, nA * nG, 1 << 20, r)


def _outer_job(N, cols=4, has_ones=1, nG=3, ra=2, rg=2):
    nA, r = cols + has_ones, ra * rg
    rows = N.InfCovOuterJob(1 << 12, cols, cols, has_ones, 1 << 13, nG, nG, 0, 1 << 14, ra, ra, 1 << 15, rg, rg,
                            1 << 16, nA * nG, 1 << 17, r)
    return N.InfDrawOuterJob(rows, 1 << 18, 1 << 19, r, 1 << 20, nA * nG, 1 << 21, r)


ROUTES = [("kfac_inf_draws", "InfDrawJob", _dense_job,
           (("J", None), ("UA", None), ("UG", None), ("W", None), ("F", None), ("ldJ", 14), ("ldA", 1), ("ldG", 1),
            ("ldW", 14), ("ldF", 3), ("nA", 0), ("nG", -1), ("ra", 0), ("rg", -2))),
          ("kfac_inf_draws_outer", "InfDrawOuterJob", _outer_job,
           (("a", None), ("D", None), ("UA", None), ("UG", None), ("W", None), ("F", None), ("lda", 3), ("ldD", 2),
            ("ldA", 1), ("ldG", 1), ("ldW", 14), ("ldF", 3), ("cols", 0), ("nG", 0), ("ra", 0), ("rg", -2)))]


@pytest.mark.parametrize("symbol,pyname,make,bad_rows", ROUTES, ids=["dense", "outer"])
def test_inf_draw_calls_validate_before_any_launch(symbol, pyname, make, bad_rows):
    from bnn_kfac_amd import _native as N
    lib = N.lib()
    call, query, S = getattr(lib, symbol), getattr(lib, symbol + "_workspace_bytes"), getattr(N, pyname)
    arr = N.as_array(S, [make(N)])
    nb, nc, ns = 2, 3, 4
    R = nb * nc
    for njobs in (0, 9, -1):
        assert call(arr, njobs, nb, nc, ns, 0, OUT, R, None, 0, None) == N.KFAC_EINVAL
        assert query(arr, njobs, nb, nc, ns) == 0
    assert call(N.as_array(S, [make(N)] * 9), 9, nb, nc, ns, 0, OUT, R, None, 0, None) == N.KFAC_EINVAL
    for bad in ((0, 3, 4), (-4, 3, 4), (2, 0, 4), (2, -1, 4), (2, 3, 0), (2, 3, -5)):
        assert call(arr, 1, *bad, 0, OUT, R, None, 0, None) == N.KFAC_EINVAL
        assert query(arr, 1, *bad) == 0
    assert call(None, 1, nb, nc, ns, 0, OUT, R, None, 0, None) == N.KFAC_EINVAL
    assert query(None, 1, nb, nc, ns) == 0
    assert call(arr, 1, nb, nc, ns, 0, None, R, None, 0, None) == N.KFAC_EINVAL   # F
    assert call(arr, 1, nb, nc, ns, 0, OUT, R - 1, None, 0, None) == N.KFAC_EINVAL  # ldF < R
    for field, value in bad_rows:
        bad = make(N)
        setattr(bad.rows, field, value)
        assert call(N.as_array(S, [bad]), 1, nb, nc, ns, 0, OUT, R, None, 0, None) == N.KFAC_EINVAL, field
        # ... even with a workspace that would do: EINVAL comes first
        assert call(N.as_array(S, [bad]), 1, nb, nc, ns, 0, OUT, R, WS, 1 << 30, None) == N.KFAC_EINVAL, field
    for field, value in (("C", None), ("Binv", None), ("Z", None), ("E", None), ("ldB", 3), ("ldZ", 14), ("ldE", 3)):
        bad = make(N)
        setattr(bad, field, value)
        assert call(N.as_array(S, [bad]), 1, nb, nc, ns, 0, OUT, R, None, 0, None) == N.KFAC_EINVAL, field
    bad = make(N)
    bad.ldE = 3  # the second job of two is validated too
    assert call(N.as_array(S, [make(N), bad]), 2, nb, nc, ns, 0, OUT, R, None, 0, None) == N.KFAC_EINVAL
    # R, ns or a task count beyond 31 bits: refused, not wrapped
    for big in ((1 << 30, 32, 1), ((1 << 31) // 10, 10, 1), (2, 3, 1 << 31), (1 << 20, 1 << 10, 1 << 20)):
        assert call(arr, 1, *big, 0, OUT, big[0] * big[1], WS, 1 << 62, None) == N.KFAC_EINVAL
    # a valid call without a workspace, and with one a byte short
    assert call(arr, 1, nb, nc, ns, 0, OUT, R, None, 0, None) == N.KFAC_EWORKSPACE
    assert call(arr, 1, nb, nc, ns, 1, OUT, R + 5, None, 0, None) == N.KFAC_EWORKSPACE
    need = query(arr, 1, nb, nc, ns)
    assert need > 0
    assert call(arr, 1, nb, nc, ns, 0, OUT, R, None, need, None) == N.KFAC_EWORKSPACE
    assert call(arr, 1, nb, nc, ns, 0, OUT, R, WS, need - 1, None) == N.KFAC_EWORKSPACE
    wide = make(N)
    wide.ldB, wide.ldZ, wide.ldE, wide.rows.ldF = 4 + 1, 15 + 3, 4 + 2, 4 + 3  # wider pitches are allowed
    assert call(N.as_array(S, [wide]), 1, nb, nc, ns, 0, OUT, R, None, 0, None) == N.KFAC_EWORKSPACE
    # no cap on nc or ns: accepted as far as the workspace check
    for wide_nc, many in ((33, 4), (1000, 1), (3, 1000)):
        assert query(arr, 1, 2, wide_nc, many) > 0
        assert call(arr, 1, 2, wide_nc, many, 0, OUT, 2 * wide_nc, None, 0, None) == N.KFAC_EWORKSPACE
    # the workspace grows with the samples, the classes and the draws; two jobs add up
    assert query(arr, 1, 2, 3, 4) < query(arr, 1, 70, 3, 4) < query(arr, 1, 70, 30, 4) < query(arr, 1, 70, 30, 70)
    assert query(N.as_array(S, [make(N), make(N)]), 2, nb, nc, ns) == 2 * need
    wrapper = getattr(N, symbol[len("kfac_"):] + "_workspace_bytes")
    assert wrapper([make(N)], nb, nc, ns) == need
    assert callable(getattr(N, symbol[len("kfac_"):])) and symbol in N.SIGNATURES


def test_native_wrappers_refuse_cpu_outputs():
    from bnn_kfac_amd import _native as N
    for call, make in ((N.inf_draws, _dense_job), (N.inf_draws_outer, _outer_job)):
        with pytest.raises(N.NativeError):       # no CPU fallback
            call([make(N)], 2, 3, 4, torch.zeros(4, 6))
        with pytest.raises(ValueError):
            call([make(N)], 2, 3, 4, torch.zeros(4, 5))


# ------------------------------------------------------------------ the Python interface
def _cpu_inf(ra=2, rg=2):
    """An INF with a state on the CPU: enough for every check that precedes the device."""
    from bnn_kfac_amd.curvatures import INF
    net = torch.nn.Sequential(torch.nn.Linear(4, 3))
    inf = INF.__new__(INF)
    inf.model = net
    inf._state = {net[0]: (torch.randn(5, ra), torch.randn(3, rg), torch.rand(ra * rg), torch.rand(15))}
    inf._inv_state = {}
    return inf


def test_glm_predictive_mc_argument_errors_under_inf():
    from bnn_kfac_amd.variance import glm_predictive_mc
    inf = _cpu_inf()
    x = torch.randn(2, 4)
    with pytest.raises(ValueError, match="jacobians must be"):
        glm_predictive_mc(inf, x, n_draws=3, jacobians="sparse")
    with pytest.raises(ValueError, match="n_draws"):
        glm_predictive_mc(inf, x, n_draws=0)
    good = (torch.zeros(3, 5, 3), torch.zeros(3, 4))
    for z in ([], [good, good], [good[0]], [(good[0],)], [(torch.zeros(3, 3, 5), good[1])],
              [(good[0], torch.zeros(3, 5))], [(torch.zeros(2, 5, 3), good[1])], [(good[0], torch.zeros(2, 4))],
              [(good[1], good[0])]):
        with pytest.raises(ValueError, match="draw pairs|expected a pair"):
            glm_predictive_mc(inf, x, n_draws=3, z=z)
    # a well-formed call gets as far as the device: no CPU fallback
    from bnn_kfac_amd import _native as N
    with pytest.raises(N.NativeError):
        glm_predictive_mc(inf, x, n_draws=3, z=[good])


def test_kron_draws_inf_shape_errors_precede_the_device():
    from bnn_kfac_amd.variance import kron_draws_inf, kron_draws_outer_inf
    UA, UG, W, F, Cc, Binv = (torch.zeros(5, 2), torch.zeros(3, 2), torch.zeros(5, 3), torch.zeros(4, 4),
                              torch.zeros(5, 3), torch.zeros(4, 4))
    J, a, D = torch.zeros(2, 3, 15), torch.zeros(2, 4), torch.zeros(2, 3, 3)
    z, e = torch.zeros(4, 5, 3), torch.zeros(4, 4)
    for bad in (dict(Cc=torch.zeros(3, 5)), dict(Binv=torch.zeros(4, 3)), dict(e=torch.zeros(4, 5)),
                dict(e=torch.zeros(3, 4)), dict(z=torch.zeros(4, 3, 5))):
        v = dict(Cc=Cc, Binv=Binv, z=z, e=e)
        v.update(bad)
        with pytest.raises(ValueError):
            kron_draws_inf([(J, UA, UG, W, F, v["Cc"], v["Binv"])], [v["z"]], [v["e"]])
        with pytest.raises(ValueError):
            kron_draws_outer_inf([(a, D, UA, UG, W, F, v["Cc"], v["Binv"])], [v["z"]], [v["e"]])
    with pytest.raises(ValueError):
        kron_draws_inf([(J, UA, UG, W, F, Cc, Binv)], [z, z], [e])
    with pytest.raises(ValueError):
        kron_draws_inf([], [], [])
