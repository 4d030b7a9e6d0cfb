"""Inputs and fp64 references shared by the INF Monte-Carlo GLM predictive tests
(test_glm_inf_mc_host.py, test_gpu_glm_inf_mc.py), in the style of glm_inf_cases.py and
glm_mc_cases.py: a plain helper module, no GPU, no torch device; every reference is numpy fp64
(int64 on the integer cases) written from the formulas of include/kfac_hip.h, never from the
kernels, computed from the same fp32 inputs the device gets, once per shape (lru_cache, arrays
read-only).

    F[s][b, c] = first - second ,
    first  = < M[b, c] o C , Z_s >                      (outer: abar_b^T (C o Z_s) delta_{b,c})
    second = < y[b, c] , q_s > ,  y = F t (glm_inf_cases' t) ,
    q_s    = F vec(UA^T (C o Z_s) UG) + Binv eps_s .

UA / UG / W as glm_inf_cases builds them, C = sqrt(W) in fp64 rounded to fp32.  F is scaled so
that max|<y, F g>| = max|first| / 4, then Binv (random lower-triangular) so that
max|<y, Binv eps>| = max|first| / 4: max|second| <= max|first| / 2, so the cancellation cap
max(max|first|, max|second|) <= 10 max|ref|, asserted in every generator, holds with room."""
import functools
import zlib
from types import SimpleNamespace as NS

import numpy as np

from glm_full_cases import EXACT, _sparse_basis, _ternary
from glm_inf_cases import _weights
from glm_sweep_cases import _freeze, _orthogonal

F32, F64 = np.float32, np.float64

# (cols, has_ones, nG, ra, rg, nb, nc, ns)
OUTER_SHAPES = [(1, 0, 1, 1, 1, 1, 1, 1),          # smallest possible
                (63, 1, 10, 5, 3, 3, 10, 2),       # nA = 64 ends a tile
                (64, 1, 5, 64, 1, 2, 3, 3),        # the ones column alone in the second K step; ra a full tile
                (20, 1, 65, 7, 9, 2, 3, 2),        # one column alone in g-tile 1
                (12, 1, 6, 2, 3, 65, 2, 2),        # the samples cross a 64-tile
                (20, 0, 130, 3, 2, 3, 33, 5),      # no bias, nc > 32, three g-tiles
                (69, 1, 70, 33, 66, 2, 3, 2),      # r = 2178 crosses a segment of the second term; rg > 64
                (130, 1, 130, 33, 9, 3, 2, 65),    # the draws cross a 64-tile
                (784, 1, 128, 10, 10, 8, 10, 4)]   # the MLP layer
# (nA, nG, ra, rg, nb, nc, ns)
DENSE_SHAPES = [(1, 1, 1, 1, 1, 1, 1),             # smallest possible
                (5, 4, 2, 2, 3, 10, 3),            # a small mixed shape
                (9, 7, 3, 2, 13, 5, 2),            # R = 65
                (65, 33, 5, 7, 2, 3, 2),           # K = 2145
                (20, 31, 4, 5, 5, 33, 65),         # the draws cross a 64-tile, nc > 32
                (70, 70, 65, 2, 2, 3, 2)]          # ra > 64
IDS = lambda s: "x".join(map(str, s))  # noqa: E731

# Tolerance of the GPU tests: rtol = SCALE, atol = SCALE * max(max|first|, max|second|).
# fp32_chain_error below runs the stage chain (h | x, t, y, g, q, both partial sums, the fp64
# difference) in numpy fp32 on the CPU for every shape above; its worst error over
# max(max|first|, max|second|) is MEASURED_FP32_CHAIN (test_glm_inf_mc_host.py re-measures it and
# checks this record), and SCALE = max(1e-5, 4 x that), the factor 4 the project's margin for
# another accumulation order.  Never derived from the device's output.
MEASURED_FP32_CHAIN = 5.1e-7  # worst case: dense (70, 70, 65, 2, 2, 3, 2), 5.02e-7
SCALE = max(1e-5, 4 * MEASURED_FP32_CHAIN)  # = 1e-5: four times the measured error is 2.0e-6


def abar_of(a, ones):
    return np.concatenate([a, np.ones((a.shape[0], 1), dtype=a.dtype)], axis=1) if ones else a


def sample_linear_map(UA, UG, W, F, C, Binv):
    """A (nA*nG, nA*nG + r) with vec(x) = A [vec(Z); eps] for the draw of kfac_hip.h, in the
    dtype of the inputs; `A A^T = P^-1` is the claim."""
    U = np.kron(UA, UG)
    n, r = U.shape
    w, c = W.reshape(-1), C.reshape(-1)
    Qz = F @ U.T * c[None, :]                       # q = Qz vec(Z) + Binv eps
    low = w[:, None] * (U @ F.T)                    # w o U F^T
    return np.concatenate([np.diag(c) - low @ Qz, -low @ Binv], axis=1)


def _q(UA, UG, F, C, Binv, Z, E):
    """(F g, Binv eps), each (ns, r)."""
    g = np.einsum("ip,sig,gq->spq", UA, C * Z, UG, optimize=True).reshape(Z.shape[0], -1)
    return g @ F.T, E @ Binv.T


def outer_parts(a, ones, D, UA, UG, W, F, C, Binv, Z, E):
    """The factored formula in the dtype of the inputs (no row is formed): (first, <y, F g>,
    <y, Binv eps>), each (ns, nb, nc)."""
    abar = abar_of(a, ones)
    first = np.einsum("sbg,bcg->sbc", np.matmul(abar, C * Z), D)
    H = np.einsum("ip,bi,ig->bpg", UA, abar, W)
    t = np.einsum("bpg,bcg,gq->bcpq", H, D, UG, optimize=True).reshape(D.shape[0], D.shape[1], -1)
    y = t @ F.T
    qg, qe = _q(UA, UG, F, C, Binv, Z, E)
    return first, np.einsum("bcr,sr->sbc", y, qg), np.einsum("bcr,sr->sbc", y, qe)


def dense_parts(J, nA, nG, UA, UG, W, F, C, Binv, Z, E):
    """The rows-given formula: (first, <y, F g>, <y, Binv eps>), each (ns, nb, nc)."""
    nb, nc = J.shape[:2]
    M = J.reshape(nb, nc, nA, nG)
    first = np.einsum("bcig,sig->sbc", M, C * Z, optimize=True)
    t = np.einsum("ip,bcig,gq->bcpq", UA, M * W, UG, optimize=True).reshape(nb, nc, -1)
    y = t @ F.T
    qg, qe = _q(UA, UG, F, C, Binv, Z, E)
    return first, np.einsum("bcr,sr->sbc", y, qg), np.einsum("bcr,sr->sbc", y, qe)


def _operands(rng, nA, nG, ra, rg):
    UA = np.ascontiguousarray(_orthogonal(rng, nA)[:, :ra])
    UG = np.ascontiguousarray(_orthogonal(rng, nG)[:, :rg])
    W = _weights(rng, nA, nG)
    C = np.sqrt(W.astype(F64)).astype(F32)
    return UA, UG, W, C


def _scaled(rng, r, parts_of):
    """(F, Binv) fp32: F = alpha tril(randn) diag(10^U(-1, 1)) with max|<y, F g>| = max|first| / 4,
    then Binv = beta tril(randn) with max|<y, Binv eps>| = max|first| / 4."""
    F0 = np.tril(rng.standard_normal((r, r))) * 10.0 ** rng.uniform(-1.0, 1.0, size=(1, r))
    B0 = np.tril(rng.standard_normal((r, r)))
    first, sg, _ = parts_of(F0, B0)
    F = np.sqrt(0.25 * np.abs(first).max() / np.abs(sg).max()) * F0      # <y, F g> is quadratic in F
    _, _, se = parts_of(F, B0)
    Binv = 0.25 * np.abs(first).max() / np.abs(se).max() * B0            # <y, Binv eps> is linear in Binv
    return F.astype(F32), Binv.astype(F32)


def _capped(first, sg, se):
    """(ref, max(max|first|, max|second|)) with the cancellation cap asserted."""
    second = sg + se
    ref = first - second
    top = max(float(np.abs(first).max()), float(np.abs(second).max()))
    assert top <= 10.0 * np.abs(ref).max(), (top, np.abs(ref).max())
    return ref, top


@functools.lru_cache(maxsize=None)
def outer_case(cols, ones, nG, ra, rg, nb, nc, ns, seed=0):
    """(a, D, UA, UG, W, F, C, Binv, Z, E) fp32, the fp64 reference (ns, nb, nc) and
    max(max|first|, max|second|)."""
    rng = np.random.default_rng(seed + 1000 * cols + nG + 7)
    nA = cols + ones
    a = rng.standard_normal((nb, cols)).astype(F32)
    D = rng.standard_normal((nb, nc, nG)).astype(F32)
    UA, UG, W, C = _operands(rng, nA, nG, ra, rg)
    Z = rng.standard_normal((ns, nA, nG)).astype(F32)
    E = rng.standard_normal((ns, ra * rg)).astype(F32)
    d = lambda *ts: [t.astype(F64) for t in ts]  # noqa: E731
    F, Binv = _scaled(rng, ra * rg, lambda F0, B0: outer_parts(*d(a), ones, *d(D, UA, UG, W, F0, C, B0, Z, E)))
    ref, top = _capped(*outer_parts(*d(a), ones, *d(D, UA, UG, W, F, C, Binv, Z, E)))
    return _freeze(a, D, UA, UG, W, F, C, Binv, Z, E, ref) + (top,)


@functools.lru_cache(maxsize=None)
def dense_case(nA, nG, ra, rg, nb, nc, ns, seed=0):
    """(J, UA, UG, W, F, C, Binv, Z, E) fp32, the fp64 reference (ns, nb, nc) and
    max(max|first|, max|second|)."""
    rng = np.random.default_rng(seed + 1000 * nA + nG + 11)
    J = rng.standard_normal((nb, nc, nA * nG)).astype(F32)
    UA, UG, W, C = _operands(rng, nA, nG, ra, rg)
    Z = rng.standard_normal((ns, nA, nG)).astype(F32)
    E = rng.standard_normal((ns, ra * rg)).astype(F32)
    d = lambda *ts: [t.astype(F64) for t in ts]  # noqa: E731
    F, Binv = _scaled(rng, ra * rg,
                      lambda F0, B0: dense_parts(*d(J), nA, nG, *d(UA, UG, W, F0, C, B0, Z, E)))
    ref, top = _capped(*dense_parts(*d(J), nA, nG, *d(UA, UG, W, F, C, Binv, Z, E)))
    return _freeze(J, UA, UG, W, F, C, Binv, Z, E, ref) + (top,)


# ------------------------------------------------------------------ the fp32 stage chain on the CPU
def _f32(*arrays):
    return [np.asarray(t, dtype=F32) for t in arrays]


def _fp32_q(UA, UG, F, C, Binv, Z, E):
    """x, t, y of the draws' projection and q = G + E Binv^T, every GEMM in numpy fp32."""
    CZ = C * Z
    X = np.einsum("ip,sig->spg", UA, CZ, optimize=True).astype(F32)
    g = np.einsum("spg,gq->spq", X, UG, optimize=True).astype(F32).reshape(Z.shape[0], -1)
    q = g @ F.T + E @ Binv.T
    assert CZ.dtype == X.dtype == g.dtype == q.dtype == F32
    return CZ, q


def fp32_outer(a, ones, D, UA, UG, W, F, C, Binv, Z, E):
    """kfac_inf_draws_outer's stages with every GEMM in numpy fp32 (the difference of the two
    terms in fp64, as the reduce forms it)."""
    a, D, UA, UG, W, F, C, Binv, Z, E = _f32(a, D, UA, UG, W, F, C, Binv, Z, E)
    abar = abar_of(a, ones)
    H = np.einsum("bip,ig->bpg", abar[:, :, None] * UA[None], W, optimize=True).astype(F32)
    t = np.einsum("bcpg,gq->bcpq", H[:, None] * D[:, :, None, :], UG, optimize=True).astype(F32)
    y = t.reshape(D.shape[0], D.shape[1], -1) @ F.T
    CZ, q = _fp32_q(UA, UG, F, C, Binv, Z, E)
    Wt = np.matmul(abar, CZ)                                                  # (ns, nb, nG)
    first = np.einsum("sbg,bcg->sbc", Wt, D, optimize=True).astype(F32)
    second = np.einsum("bcr,sr->sbc", y, q, optimize=True).astype(F32)
    assert H.dtype == t.dtype == y.dtype == Wt.dtype == F32
    return first.astype(F64) - second.astype(F64)


def fp32_dense(J, nA, nG, UA, UG, W, F, C, Binv, Z, E):
    """kfac_inf_draws' stages with every GEMM in numpy fp32."""
    J, UA, UG, W, F, C, Binv, Z, E = _f32(J, UA, UG, W, F, C, Binv, Z, E)
    nb, nc = J.shape[:2]
    M = J.reshape(nb, nc, nA, nG)
    X = np.einsum("ip,bcig->bcpg", UA, M * W, optimize=True).astype(F32)
    t = np.einsum("bcpg,gq->bcpq", X, UG, optimize=True).astype(F32)
    y = t.reshape(nb, nc, -1) @ F.T
    CZ, q = _fp32_q(UA, UG, F, C, Binv, Z, E)
    first = np.einsum("bck,sk->sbc", (M * C).reshape(nb, nc, -1), Z.reshape(Z.shape[0], -1),
                      optimize=True).astype(F32)
    second = np.einsum("bcr,sr->sbc", y, q, optimize=True).astype(F32)
    assert X.dtype == t.dtype == y.dtype == F32
    return first.astype(F64) - second.astype(F64)


def fp32_chain_error():
    """(worst |fp32 chain - fp64 reference| / max(max|first|, max|second|), its shape) over every
    shape above."""
    worst, where = 0.0, None
    for shape in OUTER_SHAPES:
        *inputs, ref, top = outer_case(*shape)
        err = float(np.abs(fp32_outer(inputs[0], shape[1], *inputs[1:]) - ref).max() / top)
        if err > worst:
            worst, where = err, ("outer", shape)
    for shape in DENSE_SHAPES:
        *inputs, ref, top = dense_case(*shape)
        err = float(np.abs(fp32_dense(inputs[0], shape[0], shape[1], *inputs[1:]) - ref).max() / top)
        if err > worst:
            worst, where = err, ("dense", shape)
    return worst, where


# ------------------------------------------------------------------ integer-exact cases
# name -> ([(cols, has_ones, nG, ra, rg) per job], nb, nc, ns, accumulate); every case runs on
# both draw calls (the rows-given call gets the rank-one rows abar delta^T of the same a, D)
INT_CASES = {
    "two-jobs": ([(63, 1, 10, 5, 3), (20, 0, 130, 3, 2)], 3, 4, 3, False),
    "accumulate": ([(64, 1, 5, 4, 2), (12, 1, 6, 2, 3)], 2, 3, 3, True),
    "ns65-nc33": ([(19, 1, 31, 3, 2)], 5, 33, 65, False),
    "nG2049": ([(3, 1, 2049, 2, 3)], 2, 2, 1, False),
}


@functools.lru_cache(maxsize=None)
def int_case(name):
    """The case's jobs (int64 a, D, UA, UG, W, F, C, Binv, Z, E per job: a, D, Z, E ternary,
    UA, UG, F, Binv with at most three +-1 per column / row, C in {1, 2, 3}, W = C^2) and its
    prefill (accumulate) or None."""
    shapes, nb, nc, ns, accumulate = INT_CASES[name]
    c = NS(name=name, nb=nb, nc=nc, ns=ns, accumulate=accumulate, jobs=[])
    for index, (cols, ones, nG, ra, rg) in enumerate(shapes):
        rng = np.random.default_rng(zlib.crc32(repr(("glm_inf_mc", name, index)).encode()))
        nA, r = cols + ones, ra * rg
        j = NS(cols=cols, ones=ones, nA=nA, nG=nG, ra=ra, rg=rg)
        j.a, j.D = _ternary(rng, (nb, cols)), _ternary(rng, (nb, nc, nG))
        j.UA = np.ascontiguousarray(_sparse_basis(rng, nA)[:, :ra])
        j.UG = np.ascontiguousarray(_sparse_basis(rng, nG)[:, :rg])
        j.F = np.ascontiguousarray(_sparse_basis(rng, r).T)
        j.Binv = np.ascontiguousarray(_sparse_basis(rng, r).T)
        j.C = rng.integers(1, 4, size=(nA, nG)).astype(np.int64)
        j.C[0, :] = 3            # asymmetric in (i, g): a transposed index cannot pass
        j.C[1:, 0] = 1
        j.W = j.C * j.C
        j.Z, j.E = _ternary(rng, (ns, nA, nG)), _ternary(rng, (ns, r))
        j.Z[:, -1, -1] = rng.choice([-1, 1], size=ns)  # the last element of a draw is never 0
        c.jobs.append(j)
    rng = np.random.default_rng(zlib.crc32(repr(("glm_inf_mc prefill", name)).encode()))
    c.prefill = rng.integers(-3, 4, size=(ns, nb, nc)).astype(np.int64) if accumulate else None
    return c


def int_rows(j):
    """Job j's rank-one rows abar delta^T: (nb, nc, nA*nG) int64."""
    return np.einsum("bi,bcg->bcig", abar_of(j.a, j.ones), j.D).reshape(j.D.shape[0], j.D.shape[1], -1)


def _int_eval(c, route, ab):
    """(F int64 (ns, nb, nc), the largest magnitude any stage holds) by `route`'s stages; `ab`:
    on the absolute values of every operand, the two terms added."""
    cast = np.abs if ab else (lambda t: t)
    peak, total = 0, 0
    for j in c.jobs:
        a, D, UA, UG, W, F, C, Binv, Z, E = (cast(t) for t in (j.a, j.D, j.UA, j.UG, j.W, j.F, j.C, j.Binv,
                                                                j.Z, j.E))
        abar = abar_of(a, j.ones)
        CZ = C * Z
        X = np.einsum("ip,sig->spg", UA, CZ)
        g = np.einsum("spg,gq->spq", X, UG).reshape(c.ns, -1)
        G, EB = g @ F.T, E @ Binv.T
        q = G + EB
        if route == "outer":
            HR = np.einsum("bip,ig->bpg", np.concatenate([abar[:, :, None] * UA[None], (abar * abar)[:, :, None]],
                                                         axis=2), W)
            t = np.einsum("bpg,bcg,gq->bcpq", HR[:, :j.ra], D, UG).reshape(c.nb, c.nc, -1)
            Wt = np.matmul(abar, CZ)
            first = np.einsum("sbg,bcg->sbc", Wt, D)
            seen = [HR, Wt]
        else:
            M = np.einsum("bi,bcg->bcig", abar, D)
            Xr = np.einsum("ip,bcig->bcpg", UA, M * W)
            t = np.einsum("bcpg,gq->bcpq", Xr, UG).reshape(c.nb, c.nc, -1)
            first = np.einsum("bcig,sig->sbc", M, CZ)
            seen = [Xr]
        y = t @ F.T
        second = np.einsum("bcr,sr->sbc", y, q)
        total = total + (first + second if ab else first - second)
        seen += [CZ, X, g, G, EB, q, t, y, first, second, total]
        peak = max([peak] + [int(np.abs(s).max()) for s in seen])
    if c.accumulate:
        total = total + cast(c.prefill)
        peak = max(peak, int(np.abs(total).max()))
    return total, peak


def int_reference(c, route):
    return _int_eval(c, route, False)[0]


def int_bound(c, route):
    """The largest magnitude any partial sum of any stage can reach, in any order: asserted below
    2^24, so fp32 is exact throughout and the device result has the reference's bits."""
    bound = _int_eval(c, route, True)[1]
    assert 0 < bound < EXACT, (c.name, route, bound)
    return bound
