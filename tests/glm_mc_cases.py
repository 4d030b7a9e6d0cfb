"""Inputs and references shared by the Monte-Carlo GLM predictive tests (test_glm_mc_host.py,
test_gpu_glm_mc.py): a plain helper module, no GPU, no torch device.

References are numpy fp64 (or int64 on the integer cases) written from the formulas of
include/kfac_hip.h, never from the kernels:
  rows given   F[s][r] = < K1^T M_r K2 , Z_s >_F,  M_r = J[r] viewed (nA, nG), index a*nG + g
  factored     F[s][(b, c)] = u_b^T Z_s v_{b,c},  U = [a | 1] K1,  V = D K2
  softmax      psum[b][c] = sum_s softmax(mean[b] + F[s][b])[c],  hsum[b] = sum_s H(.) in nats
Random cases are fp32 inputs with their fp64 reference, once per shape (lru_cache, read-only).

Integer cases.  K1 and K2 hold at most three +-1 per column (`sparse_signs`), a and D rows at
most eight +-1, Z is in {-1, 0, 1}; the rows-given call gets the rank-one rows abar delta^T of
the same a and D.  Then |U| <= 3, |V| <= 3 and |F| <= 9 nA nG per job, every intermediate is an
integer, and `int_bound` -- ONE evaluation of the chain on absolute values, with the prefill of
an accumulate case -- is the largest magnitude any partial sum in any order can reach.  Below
2^24 fp32 is exact in every order and so are the fp64 reduces and the final cast: the device
result must have the bits of the int64 reference."""
import functools
import zlib
from types import SimpleNamespace as NS

import numpy as np

F32 = np.float32
LIMIT = 1 << 24

# (cols, has_ones, nG, nb, nc, ns)
OUTER = [(1, 0, 1, 1, 1, 1),          # smallest possible
         (63, 1, 10, 3, 10, 2),       # nA = 64 exactly
         (64, 1, 5, 2, 3, 3),         # the ones entry alone in the second K step
         (20, 1, 65, 2, 3, 2),        # one column alone in g-tile 1
         (12, 1, 6, 65, 2, 2),        # samples cross the 64-sample tile
         (20, 0, 130, 3, 33, 5),      # no bias, nc > 32, three g-tiles
         (20, 1, 2049, 2, 2, 1),      # one element past a 2048 boundary
         (784, 1, 128, 8, 10, 4),     # the MLP layer
         (4096, 1, 4096, 8, 10, 2)]   # C5's layer; Z is 134 MB
# (nA, nG, nb, nc, ns)
DENSE = [(1, 1, 1, 1, 1),             # smallest possible
         (5, 4, 3, 10, 3),            # a small mixed shape
         (9, 7, 13, 5, 2),            # R = 65
         (65, 33, 2, 3, 2),           # K = 2145, two segments
         (20, 31, 5, 33, 65),         # draws cross a 64-tile, nc > 32
         (785, 128, 8, 10, 4)]        # the MLP layer
# (ns, nb, nc)
SOFTMAX = [(1, 1, 1), (3, 2, 2), (7, 5, 10), (2, 3, 33), (5, 2, 257), (65, 3, 10), (4, 2, 1000)]
IDS = lambda s: "x".join(map(str, s))  # noqa: E731

# integer cases: name -> ([(cols, has_ones, nG, lower) per job], nb, nc, ns, accumulate); every
# case runs on both draw calls.  9 nA nG stays far below 2^24 (the widest: 21 * 2049 * 9 = 387261)
INT_CASES = {
    "1x0x1": ([(1, 0, 1, True)], 1, 1, 1, False),
    "63x1x10": ([(63, 1, 10, True)], 3, 10, 2, False),
    "64x1x5-dense": ([(64, 1, 5, False)], 2, 3, 3, False),
    "20x1x65": ([(20, 1, 65, True)], 2, 3, 2, False),
    "12x1x6-nb65": ([(12, 1, 6, False)], 65, 2, 2, False),
    "20x0x130-nc33": ([(20, 0, 130, True)], 3, 33, 5, False),
    "20x1x2049": ([(20, 1, 2049, True)], 2, 2, 1, False),
    "19x1x31-ns65": ([(19, 1, 31, False)], 5, 33, 65, False),
    "two-jobs": ([(63, 1, 10, True), (20, 0, 130, False)], 3, 4, 3, False),
    "accumulate": ([(64, 1, 5, True), (12, 1, 6, False)], 2, 3, 3, True),
}


def _freeze(*arrays):
    for t in arrays:
        t.setflags(write=False)
    return arrays


def abar_of(a, ones):
    return np.concatenate([a, np.ones((a.shape[0], 1), dtype=a.dtype)], axis=1) if ones else a


def outer_rows(a, ones, D):
    """The rank-one Jacobian rows abar delta^T: (nb, nc, nA*nG), index a*nG + g."""
    return np.einsum("ba,bcg->bcag", abar_of(a, ones), D).reshape(D.shape[0], D.shape[1], -1)


def rows_ref(J, nA, nG, K1, K2, Z):
    """F (ns, nb, nc) = < M_r , K1 Z_s K2^T >_F (= < K1^T M_r K2 , Z_s >_F, with the weight
    draw formed instead of the projected rows) in the dtype of the inputs; Z (ns, nA, nG)."""
    nb, nc = J.shape[:2]
    S = np.matmul(np.matmul(K1, Z), K2.T)
    return np.einsum("rag,sag->sr", J.reshape(-1, nA, nG), S).reshape(Z.shape[0], nb, nc)


def outer_ref(a, ones, D, K1, K2, Z):
    """F (ns, nb, nc) = u_b^T Z_s v_{b,c} in the dtype of the inputs."""
    U = abar_of(a, ones) @ K1
    V = D @ K2
    W = np.matmul(U, Z)  # (ns, nb, nG)
    return np.einsum("sbg,bcg->sbc", W, V)


def softmax_ref(mean, F):
    """(probs, expected_entropy, entropy, mutual_information) in fp64 from mean (nb, nc) and
    F (ns, nb, nc): log-sum-exp after subtracting the row maximum."""
    y = mean.astype(np.float64)[None] + F.astype(np.float64)
    y = y - y.max(axis=2, keepdims=True)
    e = np.exp(y)
    se = e.sum(axis=2, keepdims=True)
    p = e / se
    H = np.log(se[..., 0]) - (p * y).sum(axis=2)
    probs = p.mean(axis=0)
    expected = H.mean(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        entropy = -np.where(probs > 0, probs * np.log(probs), 0.0).sum(axis=1)
    return probs, expected, entropy, np.maximum(entropy - expected, 0.0)


def _factors(rng, nA, nG, lower):
    K1 = rng.standard_normal((nA, nA), dtype=F32) / F32(np.sqrt(nA))
    K2 = rng.standard_normal((nG, nG), dtype=F32) / F32(np.sqrt(nG))
    return (np.tril(K1), np.tril(K2)) if lower else (K1, K2)


@functools.lru_cache(maxsize=None)
def outer_case(cols, ones, nG, nb, nc, ns, lower=True):
    """(a, D (nb, nc, nG), K1, K2, Z (ns, nA, nG)) fp32 and the fp64 reference (ns, nb, nc)."""
    rng = np.random.default_rng(7 + 1000 * cols + nG + (0 if lower else 1 << 20))
    nA = cols + ones
    K1, K2 = _factors(rng, nA, nG, lower)
    a = rng.standard_normal((nb, cols), dtype=F32)
    D = rng.standard_normal((nb, nc, nG), dtype=F32)
    Z = rng.standard_normal((ns, nA, nG), dtype=F32)
    d = np.float64
    ref = outer_ref(a.astype(d), ones, D.astype(d), K1.astype(d), K2.astype(d), Z)
    return _freeze(a, D, K1, K2, Z, ref)


@functools.lru_cache(maxsize=None)
def dense_case(nA, nG, nb, nc, ns, lower=True):
    """(J (nb, nc, nA*nG), K1, K2, Z (ns, nA, nG)) fp32 and the fp64 reference (ns, nb, nc)."""
    rng = np.random.default_rng(11 + 1000 * nA + nG + (0 if lower else 1 << 20))
    K1, K2 = _factors(rng, nA, nG, lower)
    J = rng.standard_normal((nb, nc, nA * nG), dtype=F32)
    Z = rng.standard_normal((ns, nA, nG), dtype=F32)
    d = np.float64
    ref = rows_ref(J.astype(d), nA, nG, K1.astype(d), K2.astype(d), Z.astype(d))
    return _freeze(J, K1, K2, Z, ref)


@functools.lru_cache(maxsize=None)
def softmax_case(ns, nb, nc, scale=1.0):
    """(mean (nb, nc), F (ns, nb, nc)) fp32 and softmax_ref's four fp64 results.  scale = 80:
    every entry is +-80, so mean + F is in {-160, 0, 160}."""
    rng = np.random.default_rng(13 + 100 * ns + 10 * nb + nc)
    if scale == 1.0:
        mean = (3 * rng.standard_normal((nb, nc))).astype(F32)
        F = rng.standard_normal((ns, nb, nc)).astype(F32)
    else:
        mean = (scale * rng.choice([-1.0, 1.0], size=(nb, nc))).astype(F32)
        F = (scale * rng.choice([-1.0, 1.0], size=(ns, nb, nc))).astype(F32)
    return _freeze(mean, F) + softmax_ref(mean, F)


# ------------------------------------------------------------------ integer cases
def sparse_signs(rng, n, lower):
    """n x n with at most three +-1 per column (on and below the diagonal if lower)."""
    K = np.zeros((n, n), dtype=np.int64)
    for c in range(n):
        first = c if lower else 0
        rows = rng.choice(np.arange(first, n), size=min(3, n - first), replace=False)
        K[rows, c] = rng.choice([-1, 1], size=rows.size)
    return K


def _sparse_rows(rng, rows, width):
    """(rows, width) int64, every row exactly min(8, width) entries of +-1."""
    out = np.zeros((rows, width), dtype=np.int64)
    for r in range(rows):
        pos = rng.choice(width, size=min(8, width), replace=False)
        out[r, pos] = rng.choice([-1, 1], size=pos.size)
    return out


@functools.lru_cache(maxsize=None)
def int_case(name):
    """The case's jobs (int64 a, D, K1, K2, Z per job), its prefill (accumulate) or None."""
    shapes, nb, nc, ns, accumulate = INT_CASES[name]
    c = NS(name=name, nb=nb, nc=nc, ns=ns, accumulate=accumulate, jobs=[])
    for index, (cols, ones, nG, lower) in enumerate(shapes):
        rng = np.random.default_rng(zlib.crc32(repr(("glm_mc", name, index)).encode()))
        nA = cols + ones
        j = NS(cols=cols, ones=ones, nA=nA, nG=nG, lower=lower)
        j.K1, j.K2 = sparse_signs(rng, nA, lower), sparse_signs(rng, nG, lower)
        j.a = _sparse_rows(rng, nb, cols)
        j.D = _sparse_rows(rng, nb * nc, nG).reshape(nb, nc, nG)
        j.Z = rng.integers(-1, 2, size=(ns, nA, nG)).astype(np.int64)
        j.Z[:, -1, -1] = rng.choice([-1, 1], size=ns)  # the last element of a draw is never 0
        c.jobs.append(j)
    rng = np.random.default_rng(zlib.crc32(repr(("glm_mc prefill", name)).encode()))
    c.prefill = rng.integers(-3, 4, size=(ns, nb, nc)).astype(np.int64) if accumulate else None
    return c


def _int_eval(c, route, ab):
    """(F int64 (ns, nb, nc), the largest magnitude seen) by `route`'s formula; `ab`: on the
    absolute values of every operand."""
    cast = np.abs if ab else (lambda t: t)
    peak, total = 0, 0
    for j in c.jobs:
        a, D, K1, K2, Z = (cast(t) for t in (j.a, j.D, j.K1, j.K2, j.Z))
        if route == "outer":
            U, V = abar_of(a, j.ones) @ K1, D @ K2
            W = np.matmul(U, Z)
            F = np.einsum("sbg,bcg->sbc", W, V)
            seen = (U, V, W, F)
        else:
            M = outer_rows(a, j.ones, D).reshape(-1, j.nA, j.nG)
            U = K1.T @ M
            T = U @ K2
            F = np.einsum("rag,sag->sr", T, Z).reshape(c.ns, c.nb, c.nc)
            seen = (U, T, F)
        total = total + F
        peak = max([peak, int(np.abs(total).max())] + [int(np.abs(t).max()) for t in seen])
    if c.accumulate:
        total = total + cast(c.prefill)
        peak = max(peak, int(np.abs(total).max()))
    return total, peak


def int_reference(c, route):
    return _int_eval(c, route, False)[0]


def int_bound(c, route):
    return _int_eval(c, route, True)[1]
