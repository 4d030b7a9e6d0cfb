"""Inputs and fp64 references shared by the per-entry-weight tests (test_gpu_glm_full.py,
test_glm_full_host.py), in the style of glm_sweep_cases.py: every reference is numpy fp64
computed from the same fp32 inputs the device gets, once per shape (lru_cache, arrays
read-only).  W[t] is 10^U(-3, 3) per entry with row i = 0 at 1e-3 and row i = nA - 1 at 1e3:
with that spread a transposed or shifted index cannot pass."""
import functools

import numpy as np

from glm_sweep_cases import _freeze, _orthogonal

NT_MAX = 64

# (cols, has_ones, nG, nb, nc)
OUTER_SHAPES = [(4, 1, 3, 1, 1),
                (63, 1, 10, 3, 10),      # nA = 64 ends a tile
                (64, 1, 10, 5, 3),       # the ones column alone in a tile
                (20, 1, 31, 2, 32),      # nc at the cap
                (130, 1, 130, 70, 2),    # two sample tiles, three i tiles
                (300, 0, 257, 3, 4)]     # nG crosses one 256-long Gram segment, no bias
# (nA, nG, nb, nc)
DENSE_SHAPES = [(5, 3, 2, 4),
                (64, 10, 3, 10),         # a full tile
                (33, 65, 2, 5),          # segment edges inside an i-row, nG % 4 != 0
                (70, 1, 2, 3),           # nG = 1
                (26, 5, 3, 32)]          # nc at the cap
NTS = [1, 5, 64]                         # 5: one more than the Gram's group of four


def _weights(rng, nA, nG):
    W = (10.0 ** rng.uniform(-3.0, 3.0, size=(NT_MAX, nA, nG))).astype(np.float32)
    W[:, 0, :] = np.float32(1e-3)
    W[:, -1, :] = np.float32(1e3)
    return W


def outer_ref(a, ones, D, VA, VG, W):
    a, D, VA, VG, W = (t.astype(np.float64) for t in (a, D, VA, VG, W))
    abar = np.concatenate([a, np.ones((a.shape[0], 1))], axis=1) if ones else a
    r = np.einsum("bi,tig->tbg", (abar @ VA) ** 2, W)
    Q = D @ VG                                         # (nb, nc, nG)
    return np.einsum("bcg,tbg,bdg->tbcd", Q, r, Q)


def dense_ref(J, nA, nG, VA, VG, W):
    J, VA, VG, W = (t.astype(np.float64) for t in (J, VA, VG, W))
    nb, nc = J.shape[:2]
    Y = np.einsum("ai,bcag,gh->bcih", VA, J.reshape(nb, nc, nA, nG), VG)
    return np.einsum("tih,bcih,bdih->tbcd", W, Y, Y)


@functools.lru_cache(maxsize=None)
def outer_case(cols, ones, nG, nb, nc, seed=0):
    """(a, D, VA, VG, W) fp32 and the fp64 reference (NT_MAX, nb, nc, nc)."""
    rng = np.random.default_rng(seed + 1000 * cols + nG)
    nA = cols + ones
    a = rng.standard_normal((nb, cols)).astype(np.float32)
    D = rng.standard_normal((nb, nc, nG)).astype(np.float32)
    VA, VG = _orthogonal(rng, nA), _orthogonal(rng, nG)
    W = _weights(rng, nA, nG)
    return _freeze(a, D, VA, VG, W, outer_ref(a, ones, D, VA, VG, W))


@functools.lru_cache(maxsize=None)
def dense_case(nA, nG, nb, nc, seed=0):
    """(J, VA, VG, W) fp32 and the fp64 reference (NT_MAX, nb, nc, nc)."""
    rng = np.random.default_rng(seed + 1000 * nA + nG)
    J = rng.standard_normal((nb, nc, nA * nG)).astype(np.float32)
    VA, VG = _orthogonal(rng, nA), _orthogonal(rng, nG)
    W = _weights(rng, nA, nG)
    return _freeze(J, VA, VG, W, dense_ref(J, nA, nG, VA, VG, W))


def rows_of(a, ones, D):
    """A Linear layer's materialised rows outer([a | 1], delta): (nb, nc, nA*nG) fp32 (exact:
    one product per entry)."""
    abar = np.concatenate([a, np.ones((a.shape[0], 1), np.float32)], axis=1) if ones else a
    return np.einsum("bi,bcg->bcig", abar, D).reshape(D.shape[0], D.shape[1], -1).astype(np.float32)


# ------------------------------------------------------------------ integer-exact cases
EXACT = 1 << 24  # every integer of magnitude <= 2^24 is an fp32 number


def _ternary(rng, shape):
    return rng.integers(-1, 2, size=shape).astype(np.int64)


def _sparse_basis(rng, n):
    """n x n, entries in {-1, 0, 1}, at most three non-zeros per column."""
    V = np.zeros((n, n), np.int64)
    for col in range(n):
        rows = rng.choice(n, size=min(3, n), replace=False)
        V[rows, col] = rng.choice([-1, 1], size=len(rows))
    return V


def _int_weights(rng, nt, nA, nG):
    """{0, 1, 2}, asymmetric in (i, g): row i = 0 all 2, column g = 0 of the other rows all 0."""
    W = rng.integers(0, 3, size=(nt, nA, nG)).astype(np.int64)
    W[:, 1:, 0] = 0
    W[:, 0, :] = 2
    return W


@functools.lru_cache(maxsize=None)
def int_outer_case(cols=64, ones=1, nG=10, nb=5, nc=3, nt=5):
    """(a, D, VA, VG, W) fp32 holding small integers, the int64 result, and the largest sum of
    absolute values of the terms any stage accumulates (the same formula on |inputs|)."""
    rng = np.random.default_rng(7)
    nA = cols + ones
    a, D = _ternary(rng, (nb, cols)), _ternary(rng, (nb, nc, nG))
    VA, VG, W = _sparse_basis(rng, nA), _sparse_basis(rng, nG), _int_weights(rng, nt, nA, nG)
    abar = np.concatenate([a, np.ones((nb, 1), np.int64)], axis=1) if ones else a

    def run(abar, D, VA, VG):
        p = abar @ VA
        r = np.einsum("bi,tig->tbg", p * p, W)
        Q = D @ VG
        return (p, r, Q), np.einsum("bcg,tbg,bdg->tbcd", Q, r, Q)

    _, want = run(abar, D, VA, VG)
    stages, top = run(np.abs(abar), np.abs(D), np.abs(VA), np.abs(VG))
    bound = max(int(top.max()), *(int(s.max()) for s in stages))
    f = lambda t: t.astype(np.float32)  # noqa: E731
    return _freeze(f(a), f(D), f(VA), f(VG), f(W), want) + (bound,)


@functools.lru_cache(maxsize=None)
def int_dense_case(nA=33, nG=65, nb=2, nc=5, nt=5):
    """(J, VA, VG, W) fp32 holding small integers, the int64 result, and the bound as above."""
    rng = np.random.default_rng(11)
    J = _ternary(rng, (nb, nc, nA, nG))
    VA, VG, W = _sparse_basis(rng, nA), _sparse_basis(rng, nG), _int_weights(rng, nt, nA, nG)

    def run(J, VA, VG):
        U = np.einsum("ai,bcag->bcig", VA, J)
        Y = np.einsum("bcig,gh->bcih", U, VG)
        return (U, Y), np.einsum("tih,bcih,bdih->tbcd", W, Y, Y)

    _, want = run(J, VA, VG)
    stages, top = run(np.abs(J), np.abs(VA), np.abs(VG))
    bound = max(int(top.max()), *(int(s.max()) for s in stages))
    f = lambda t: t.astype(np.float32)  # noqa: E731
    return _freeze(f(J.reshape(nb, nc, nA * nG)), f(VA), f(VG), f(W), want) + (bound,)
