"""Inputs and fp64 references shared by the joint-covariance tests (test_gpu_glm_joint.py,
test_glm_joint_host.py).  Every reference is numpy fp64 computed from the same fp32 inputs
the device gets, once per shape (lru_cache, arrays read-only)."""
import functools

import numpy as np


def dense_rows_T(J, nA, nG, K1, K2):
    """T (R, nA*nG): row r = vec(K1^T M_r K2), M_r = J[r] viewed (nA, nG)."""
    M = J.reshape(-1, nA, nG)
    return ((K1.T @ M) @ K2).reshape(M.shape[0], -1)


def dense_joint_ref(J, nA, nG, K1, K2):
    """cov (R, R) = T T^T in the dtype of the inputs."""
    T = dense_rows_T(J, nA, nG, K1, K2)
    return T @ T.T


def outer_uv(a, ones, D, K1, K2):
    """U = [a | 1] K1 (nb, nA) and V = D K2 (nb*nc, nG)."""
    abar = np.concatenate([a, np.ones((a.shape[0], 1), dtype=a.dtype)], axis=1) if ones else a
    return abar @ K1, D.reshape(-1, D.shape[-1]) @ K2


def outer_joint_ref(a, ones, D, K1, K2):
    """cov (R, R) = (U U^T expanded over the classes) * (V V^T)."""
    nc = D.shape[1]
    U, V = outer_uv(a, ones, D, K1, K2)
    return np.kron(U @ U.T, np.ones((nc, nc), dtype=U.dtype)) * (V @ V.T)


def outer_rows(a, ones, D):
    """The Jacobian rows the factored route never forms: (nb, nc, nA*nG), M = abar delta^T."""
    abar = np.concatenate([a, np.ones((a.shape[0], 1), dtype=a.dtype)], axis=1) if ones else a
    return np.einsum("ba,bcg->bcag", abar, D).reshape(D.shape[0], D.shape[1], -1)


def _factors(rng, nA, nG, lower):
    K1 = (rng.standard_normal((nA, nA)) / np.sqrt(nA)).astype(np.float32)
    K2 = (rng.standard_normal((nG, nG)) / np.sqrt(nG)).astype(np.float32)
    return (np.tril(K1), np.tril(K2)) if lower else (K1, K2)


def _freeze(*arrays):
    for t in arrays:
        t.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def dense_case(nA, nG, nb, nc, lower=True, seed=0):
    """(J (nb, nc, nA*nG), K1, K2) fp32 and the fp64 reference (nb*nc, nb*nc)."""
    rng = np.random.default_rng(seed + 1000 * nA + nG)
    K1, K2 = _factors(rng, nA, nG, lower)
    J = rng.standard_normal((nb, nc, nA * nG)).astype(np.float32)
    ref = dense_joint_ref(J.astype(np.float64), nA, nG, K1.astype(np.float64), K2.astype(np.float64))
    return _freeze(J, K1, K2, ref)


@functools.lru_cache(maxsize=None)
def outer_case(cols, ones, nG, nb, nc, lower=True, seed=0):
    """(a (nb, cols), D (nb, nc, nG), K1, K2) fp32 and the fp64 reference (nb*nc, nb*nc)."""
    rng = np.random.default_rng(seed + 1000 * cols + nG)
    K1, K2 = _factors(rng, cols + ones, nG, lower)
    a = rng.standard_normal((nb, cols)).astype(np.float32)
    D = rng.standard_normal((nb, nc, nG)).astype(np.float32)
    ref = outer_joint_ref(a.astype(np.float64), ones, D.astype(np.float64), K1.astype(np.float64),
                          K2.astype(np.float64))
    return _freeze(a, D, K1, K2, ref)


def small_ints(rng, *shape):
    """Integers from {-2..2}."""
    return rng.integers(-2, 3, size=shape).astype(np.int64)
