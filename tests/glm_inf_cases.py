"""Inputs and fp64 references shared by the INF GLM-predictive tests (test_gpu_glm_inf.py,
test_glm_inf_host.py), in the style of glm_full_cases.py: every reference is numpy fp64
computed from the same fp32 inputs the device gets, once per shape (lru_cache, arrays
read-only).

    cov[b, c, c'] = sum_{i,g} W[i, g] M[b, c][i, g] M[b, c'][i, g] - < F t[b, c], F t[b, c'] > ,
    t[b, c][p*rg + q] = sum_{i,g} UA[i, p] W[i, g] M[b, c][i, g] UG[g, q] .

UA / UG are leading columns of orthogonal matrices; W is 10^U(-2, 2) per entry with row i = 0 at
1e-2 and row i = nA - 1 at 1e2, so a transposed or shifted index cannot pass; F is a random
lower-triangular matrix times a diagonal, scaled so the second term is about half the first
(the generators assert max|first term| <= 10 max|ref|: the cancellation is capped)."""
import functools

import numpy as np

from glm_full_cases import EXACT, _sparse_basis, _ternary, rows_of  # noqa: F401  (rows_of: re-exported)
from glm_sweep_cases import _freeze, _orthogonal

# (cols, has_ones, nG, ra, rg, nb, nc)
OUTER_SHAPES = [(4, 1, 3, 2, 1, 1, 1),
                (63, 1, 10, 5, 3, 3, 10),       # nA = 64 ends a tile
                (64, 1, 10, 64, 1, 5, 3),       # the ones column alone in a tile; ra a full tile; rg = 1
                (20, 1, 31, 7, 31, 2, 32),      # nc at the cap; rg = nG
                (130, 1, 130, 33, 9, 70, 2),    # two sample tiles; r = 297 crosses a Gram segment
                (300, 0, 257, 3, 2, 3, 4),      # no bias; nG crosses a Gram segment
                (69, 1, 70, 2, 66, 2, 3)]       # rg > 64: a second q tile of the t launch
# (nA, nG, ra, rg, nb, nc)
DENSE_SHAPES = [(5, 3, 2, 2, 2, 4),
                (64, 10, 8, 4, 3, 10),
                (33, 65, 5, 7, 2, 5),
                (70, 1, 9, 1, 2, 3),
                (26, 5, 26, 5, 3, 32),
                (70, 70, 65, 2, 2, 3),          # ra > 64: a second p tile of the X launch
                (70, 70, 2, 66, 2, 3)]          # rg > 64: a second q tile of the t launch

# Tolerance of the GPU tests: rtol = SCALE, atol = SCALE * max|first term|.  The second term
# goes through four chained fp32 GEMMs (H or X, t, y, the Gram), so the 1e-5 of
# test_gpu_glm_full._check is not assumed to carry over: fp32_chain_error below runs the stage
# chain in numpy fp32 on the CPU for every shape above; its worst error / max|first term| is
# MEASURED_FP32_CHAIN (test_glm_inf_host.py re-measures it and checks this record), and
# SCALE = max(1e-5, 4 x that).  Never derived from the device's output.
MEASURED_FP32_CHAIN = 3.8e-7  # worst case: outer (300, 0, 257, 3, 2, 3, 4), 3.73e-7
SCALE = max(1e-5, 4 * MEASURED_FP32_CHAIN)  # = 1e-5: four times the measured error is 1.5e-6


def _weights(rng, nA, nG):
    W = (10.0 ** rng.uniform(-2.0, 2.0, size=(nA, nG))).astype(np.float32)
    W[0, :] = np.float32(1e-2)
    W[-1, :] = np.float32(1e2)
    return W


def dense_terms(J, nA, nG, UA, UG, W, F):
    """(first, second) terms in fp64, each (nb, nc, nc); the reference is first - second."""
    J, UA, UG, W, F = (np.asarray(t, dtype=np.float64) for t in (J, UA, UG, W, F))
    nb, nc = J.shape[:2]
    M = J.reshape(nb, nc, nA, nG)
    first = np.einsum("ig,bcig,bdig->bcd", W, M, M)
    t = np.einsum("ip,bcig,gq->bcpq", UA, M * W, UG, optimize=True).reshape(nb, nc, -1)
    y = t @ F.T
    return first, np.einsum("bcr,bdr->bcd", y, y)


def outer_terms(a, ones, D, UA, UG, W, F):
    """The factored formula in fp64 (no row is formed): (first, second)."""
    a, D, UA, UG, W, F = (np.asarray(t, dtype=np.float64) for t in (a, D, UA, UG, W, F))
    abar = np.concatenate([a, np.ones((a.shape[0], 1))], axis=1) if ones else a
    rho = (abar * abar) @ W                                        # (nb, nG)
    H = np.einsum("ip,bi,ig->bpg", UA, abar, W)                    # (nb, ra, nG)
    t = np.einsum("bpg,bcg,gq->bcpq", H, D, UG).reshape(D.shape[0], D.shape[1], -1)
    y = t @ F.T
    return np.einsum("bcg,bg,bdg->bcd", D, rho, D), np.einsum("bcr,bdr->bcd", y, y)


def _factor(rng, r, first, second_of):
    """F = tril(randn) diag(10^U(-1, 1)), scaled so max|second term| = max|first term| / 2."""
    F0 = np.tril(rng.standard_normal((r, r))) * 10.0 ** rng.uniform(-1.0, 1.0, size=(1, r))
    alpha = np.sqrt(0.5 * np.abs(first).max() / np.abs(second_of(F0)).max())
    return (alpha * F0).astype(np.float32)


def _capped(first, second):
    ref = first - second
    assert np.abs(first).max() <= 10.0 * np.abs(ref).max(), (np.abs(first).max(), np.abs(ref).max())
    return ref


@functools.lru_cache(maxsize=None)
def outer_case(cols, ones, nG, ra, rg, nb, nc, seed=0):
    """(a, D, UA, UG, W, F) fp32, the fp64 reference (nb, nc, nc) and max|first term|."""
    rng = np.random.default_rng(seed + 1000 * cols + nG)
    nA = cols + ones
    a = rng.standard_normal((nb, cols)).astype(np.float32)
    D = rng.standard_normal((nb, nc, nG)).astype(np.float32)
    UA = np.ascontiguousarray(_orthogonal(rng, nA)[:, :ra])
    UG = np.ascontiguousarray(_orthogonal(rng, nG)[:, :rg])
    W = _weights(rng, nA, nG)
    F = _factor(rng, ra * rg, outer_terms(a, ones, D, UA, UG, W, np.eye(ra * rg))[0],
                lambda F0: outer_terms(a, ones, D, UA, UG, W, F0)[1])
    first, second = outer_terms(a, ones, D, UA, UG, W, F)
    return _freeze(a, D, UA, UG, W, F, _capped(first, second)) + (float(np.abs(first).max()),)


@functools.lru_cache(maxsize=None)
def dense_case(nA, nG, ra, rg, nb, nc, seed=0):
    """(J, UA, UG, W, F) fp32, the fp64 reference (nb, nc, nc) and max|first term|."""
    rng = np.random.default_rng(seed + 1000 * nA + nG)
    J = rng.standard_normal((nb, nc, nA * nG)).astype(np.float32)
    UA = np.ascontiguousarray(_orthogonal(rng, nA)[:, :ra])
    UG = np.ascontiguousarray(_orthogonal(rng, nG)[:, :rg])
    W = _weights(rng, nA, nG)
    F = _factor(rng, ra * rg, dense_terms(J, nA, nG, UA, UG, W, np.eye(ra * rg))[0],
                lambda F0: dense_terms(J, nA, nG, UA, UG, W, F0)[1])
    first, second = dense_terms(J, nA, nG, UA, UG, W, F)
    return _freeze(J, UA, UG, W, F, _capped(first, second)) + (float(np.abs(first).max()),)


# ------------------------------------------------------------------ the fp32 stage chain on the CPU
def _f32(*arrays):
    return [np.asarray(t, dtype=np.float32) for t in arrays]


def fp32_outer(a, ones, D, UA, UG, W, F):
    """kfac_inf_cov_outer's stages with every GEMM in numpy fp32 (the two Grams' difference in
    fp64, as the reduce forms it)."""
    a, D, UA, UG, W, F = _f32(a, D, UA, UG, W, F)
    abar = np.concatenate([a, np.ones((a.shape[0], 1), np.float32)], axis=1) if ones else a
    rho = (abar * abar) @ W
    H = np.einsum("bip,ig->bpg", abar[:, :, None] * UA[None], W, optimize=True).astype(np.float32)
    t = np.einsum("bcpg,gq->bcpq", H[:, None] * D[:, :, None, :], UG, optimize=True).astype(np.float32)
    y = t.reshape(D.shape[0], D.shape[1], -1) @ F.T
    first = np.einsum("bcg,bdg->bcd", D * rho[:, None, :], D, optimize=True).astype(np.float32)
    second = np.einsum("bcr,bdr->bcd", y, y, optimize=True).astype(np.float32)
    assert rho.dtype == H.dtype == t.dtype == y.dtype == np.float32
    return first.astype(np.float64) - second.astype(np.float64)


def fp32_dense(J, nA, nG, UA, UG, W, F):
    """kfac_inf_cov's stages with every GEMM in numpy fp32."""
    J, UA, UG, W, F = _f32(J, UA, UG, W, F)
    nb, nc = J.shape[:2]
    M = J.reshape(nb, nc, nA, nG)
    MW = M * W
    X = np.einsum("ip,bcig->bcpg", UA, MW, optimize=True).astype(np.float32)
    t = np.einsum("bcpg,gq->bcpq", X, UG, optimize=True).astype(np.float32)
    y = t.reshape(nb, nc, -1) @ F.T
    first = np.einsum("bcig,bdig->bcd", MW, M, optimize=True).astype(np.float32)
    second = np.einsum("bcr,bdr->bcd", y, y, optimize=True).astype(np.float32)
    assert X.dtype == t.dtype == y.dtype == np.float32
    return first.astype(np.float64) - second.astype(np.float64)


def fp32_chain_error():
    """Worst |fp32 chain - fp64 reference| / max|first term| over every shape above."""
    worst = 0.0
    for shape in OUTER_SHAPES:
        a, D, UA, UG, W, F, ref, top = outer_case(*shape)
        worst = max(worst, float(np.abs(fp32_outer(a, shape[1], D, UA, UG, W, F) - ref).max() / top))
    for shape in DENSE_SHAPES:
        J, UA, UG, W, F, ref, top = dense_case(*shape)
        worst = max(worst, float(np.abs(fp32_dense(J, shape[0], shape[1], UA, UG, W, F) - ref).max() / top))
    return worst


# ------------------------------------------------------------------ a consistent posterior
def posterior(nA, nG, ra, rg, s, n, seed=0):
    """(UA, UG, lam (ra*rg,), corr (nA*nG,) with some negative entries) fp64 and the dense
    precision P = s (U diag(lam) U^T + diag(max(corr, 0))) + n I, U = kron(UA, UG)."""
    rng = np.random.default_rng(seed + 31 * nA + nG)
    UA = np.linalg.qr(rng.standard_normal((nA, nA)))[0][:, :ra]
    UG = np.linalg.qr(rng.standard_normal((nG, nG)))[0][:, :rg]
    lam = rng.uniform(0.1, 3.0, size=ra * rg)
    corr = rng.uniform(-0.2, 1.0, size=nA * nG)
    U = np.kron(UA, UG)
    P = s * (U @ np.diag(lam) @ U.T + np.diag(np.maximum(corr, 0.0))) + n * np.eye(nA * nG)
    return UA, UG, lam, corr, P


def woodbury_gram(UA, UG, lam, corr, s, n):
    """(w (nA*nG,), sigma (r,), vtv = sigma U^T diag(w) U sigma (r, r)) fp64."""
    w = 1.0 / (s * np.maximum(corr, 0.0) + n)
    sigma = np.sqrt(s * lam)
    U = np.kron(UA, UG)
    return w, sigma, sigma[:, None] * (U.T @ (w[:, None] * U)) * sigma[None, :]


def woodbury_factors(UA, UG, lam, corr, s, n):
    """(W (nA, nG), F (r, r)) fp64 of the posterior above."""
    w, sigma, vtv = woodbury_gram(UA, UG, lam, corr, s, n)
    B = np.linalg.cholesky(np.eye(len(lam)) + vtv)
    return w.reshape(UA.shape[0], UG.shape[0]), np.linalg.inv(B) * sigma[None, :]


# ------------------------------------------------------------------ integer-exact cases
def _int_weights(rng, nA, nG):
    """{1, 2, 3}, asymmetric in (i, g): row i = 0 all 3, column g = 0 of the other rows all 1."""
    W = rng.integers(1, 4, size=(nA, nG)).astype(np.int64)
    W[1:, 0] = 1
    W[0, :] = 3
    return W


def _int_operands(rng, nA, nG, ra, rg):
    UA, UG = _sparse_basis(rng, nA)[:, :ra], _sparse_basis(rng, nG)[:, :rg]
    F = _sparse_basis(rng, ra * rg).T     # at most three non-zeros per row
    return np.ascontiguousarray(UA), np.ascontiguousarray(UG), _int_weights(rng, nA, nG), np.ascontiguousarray(F)


@functools.lru_cache(maxsize=None)
def int_outer_case(cols=64, ones=1, nG=10, ra=5, rg=3, nb=5, nc=3):
    """(a, D, UA, UG, W, F) fp32 holding small integers, the int64 result, and the largest sum
    of absolute values any stage accumulates (the same formulas on |inputs|, the two terms
    added)."""
    rng = np.random.default_rng(7)
    nA = cols + ones
    a, D = _ternary(rng, (nb, cols)), _ternary(rng, (nb, nc, nG))
    UA, UG, W, F = _int_operands(rng, nA, nG, ra, rg)
    abar = np.concatenate([a, np.ones((nb, 1), np.int64)], axis=1) if ones else a

    def run(abar, D, UA, UG, F):
        rho = (abar * abar) @ W
        H = np.einsum("ip,bi,ig->bpg", UA, abar, W)
        t = np.einsum("bpg,bcg,gq->bcpq", H, D, UG).reshape(nb, nc, -1)
        y = t @ F.T
        return (rho, H, t, y), np.einsum("bcg,bg,bdg->bcd", D, rho, D), np.einsum("bcr,bdr->bcd", y, y)

    _, first, second = run(abar, D, UA, UG, F)
    stages, f1, f2 = run(np.abs(abar), np.abs(D), np.abs(UA), np.abs(UG), np.abs(F))
    bound = max(int((f1 + f2).max()), *(int(s.max()) for s in stages))
    assert 0 < bound <= EXACT, bound      # every partial is an fp32 integer
    f = lambda t: t.astype(np.float32)  # noqa: E731
    return _freeze(f(a), f(D), f(UA), f(UG), f(W), f(F), first - second) + (bound,)


@functools.lru_cache(maxsize=None)
def int_dense_case(nA=33, nG=65, ra=5, rg=7, nb=2, nc=5):
    """(J, UA, UG, W, F) fp32 holding small integers, the int64 result, and the bound as above."""
    rng = np.random.default_rng(11)
    J = _ternary(rng, (nb, nc, nA, nG))
    UA, UG, W, F = _int_operands(rng, nA, nG, ra, rg)

    def run(J, UA, UG, F):
        X = np.einsum("ip,bcig->bcpg", UA, J * W)
        t = np.einsum("bcpg,gq->bcpq", X, UG).reshape(nb, nc, -1)
        y = t @ F.T
        return (X, t, y), np.einsum("ig,bcig,bdig->bcd", W, J, J), np.einsum("bcr,bdr->bcd", y, y)

    _, first, second = run(J, UA, UG, F)
    stages, f1, f2 = run(np.abs(J), np.abs(UA), np.abs(UG), np.abs(F))
    bound = max(int((f1 + f2).max()), *(int(s.max()) for s in stages))
    assert 0 < bound <= EXACT, bound      # every partial is an fp32 integer
    f = lambda t: t.astype(np.float32)  # noqa: E731
    return _freeze(f(J.reshape(nb, nc, nA * nG)), f(UA), f(UG), f(W), f(F), first - second) + (bound,)
