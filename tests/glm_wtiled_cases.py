"""Shapes, tolerances and the host emulation shared by the class-tiled weighted covariance tests
(test_gpu_glm_wtiled.py, test_glm_wtiled_host.py).  The inputs and fp64 references are those of
glm_full_cases.py (per-entry weights) and glm_sweep_cases.py (rank-one weights), which take any
nc.

The emulation runs the device's stage chain in SEQUENTIAL fp32 on the host -- every projection
element one k-ordered fma chain, every Gram element one k-ordered fma chain per 2048-long
segment, the segments (and the outer sweep's scale) in fp64 -- for the two shapes whose chains
are long: numpy's own fp32 sums are pairwise and would flatter them."""
import functools

import numpy as np

import glm_full_cases as C
import glm_sweep_cases as S

JSEG = 2048
TILE = 64

# (cols, has_ones, nG, nb, nc)
OUTER_SHAPES = [(4, 1, 3, 1, 33),
                (63, 1, 10, 3, 64),       # one full tile
                (64, 1, 40, 5, 65),       # one row past a tile: three tile pairs
                (128, 0, 65, 2, 130),     # six tile pairs, no bias
                (20, 1, 2100, 2, 40),     # nG over two JSEG segments
                (130, 1, 130, 70, 33)]    # two sample tiles
# (nA, nG, nb, nc)
DENSE_SHAPES = [(5, 3, 2, 33),
                (9, 7, 3, 65),
                (33, 65, 2, 40),          # K = 2145: two segments
                (20, 31, 2, 130),
                (26, 5, 3, 32)]           # under the cap through the tiled call
NTS = [1, 5]
LONG_OUTER, LONG_DENSE = (20, 1, 2100, 2, 40), (33, 65, 2, 40)

# atol = SCALE * max|ref[t]| per grid point, rtol 1e-5: the project's kernel tolerance.  The
# sequential-fp32 emulation of the two long-K shapes (emulated_errors, nt = 5) gives, against
# fp64: dense K = 2145 2.2e-6 (per-entry) and 2.1e-6 (rank one), below a quarter of 1e-5; outer
# nG = 2100 1.4e-6 (per-entry) and 3.5e-6 (rank one), above it.  So that one shape takes
# max(1e-5, 4 x worst emulated) = 1.4e-5; test_glm_wtiled_host.py holds the emulation to a
# quarter of each bound.  Neither number comes from a device result.
SCALE = 1e-5
SCALE_LONG_OUTER = 1.4e-5


def scale_for(shape):
    return SCALE_LONG_OUTER if tuple(shape) == LONG_OUTER else SCALE


def _fma_chain(A, B):
    """A (m, K) @ B (K, n) with every element one k-ordered fp32 fma chain from 0 (the product
    of two fp32 numbers is exact in fp64; the sum is rounded to fp32 once per step)."""
    A, B = A.astype(np.float64), B.astype(np.float64)
    acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
    for k in range(A.shape[1]):
        acc = (acc.astype(np.float64) + A[:, k:k + 1] * B[k:k + 1, :]).astype(np.float32)
    return acc


def _wgram(X, w):
    """X (nc, K) fp32, w (K,) fp32: sum over JSEG segments (fp64, in order) of the fp32 chains
    part[r][r'] = sum_k X[r][k] * fl(w[k] * X[r'][k])."""
    total = np.zeros((X.shape[0], X.shape[0]), np.float64)
    B = (w[None, :] * X).astype(np.float32)
    for k0 in range(0, X.shape[1], JSEG):
        total += _fma_chain(X[:, k0:k0 + JSEG], B[:, k0:k0 + JSEG].T).astype(np.float64)
    return total


def _project_dense(J, nA, nG, VA, VG):
    """Y[b, c] = VA^T M VG in the device's two stages: U = VA^T M over a, then U VG over g."""
    nb, nc = J.shape[:2]
    M = J.reshape(nb * nc, nA, nG)
    U = _fma_chain(VA.T.copy(), M.transpose(1, 0, 2).reshape(nA, -1))          # (i, (r, g))
    U = U.reshape(nA, nb * nc, nG).transpose(1, 0, 2).reshape(-1, nG)          # ((r, i), g)
    return _fma_chain(U, VG).reshape(nb, nc, nA * nG)


def _abar(a, ones):
    return np.concatenate([a, np.ones((a.shape[0], 1), np.float32)], axis=1) if ones else a


def emulate_dense(J, nA, nG, VA, VG, weights):
    """weights (nt, nA*nG) fp32 -> (nt, nb, nc, nc) fp64 as the device sums it."""
    Y = _project_dense(J, nA, nG, VA, VG)
    return np.stack([np.stack([_wgram(Y[b], w) for b in range(Y.shape[0])]) for w in weights])


def emulate_outer_full(a, ones, D, VA, VG, W):
    nb, nc, nG = D.shape
    p = _fma_chain(_abar(a, ones), VA)
    p2 = (p * p).astype(np.float32)
    Q = _fma_chain(D.reshape(-1, nG), VG).reshape(nb, nc, nG)
    out = []
    for Wt in W:
        R = _fma_chain(p2, Wt)                                                 # (nb, nG)
        out.append(np.stack([_wgram(Q[b], R[b]) for b in range(nb)]))
    return np.stack(out)


def emulate_outer_sweep(a, ones, D, VA, VG, wA, wG):
    """kfac_cov_rownorm_w sums a 64-column tile's 64 weighted squares in a tree of its own; its
    sums are short (nA terms), so they are taken in fp64 here: the long chains are the Gram's."""
    nb, nc, nG = D.shape
    p = _fma_chain(_abar(a, ones), VA)
    p2 = (p * p).astype(np.float32).astype(np.float64)
    Q = _fma_chain(D.reshape(-1, nG), VG).reshape(nb, nc, nG)
    out = []
    for t in range(wA.shape[0]):
        s = p2 @ wA[t].astype(np.float64)
        out.append(np.stack([s[b] * _wgram(Q[b], wG[t]) for b in range(nb)]))
    return np.stack(out)


def rel_err(got, ref):
    """max over grid points of max|got[t] - ref[t]| / max|ref[t]|."""
    return max(float(np.abs(got[t] - ref[t]).max() / np.abs(ref[t]).max()) for t in range(ref.shape[0]))


@functools.lru_cache(maxsize=None)
def emulated_errors(nt=5):
    """{call: rel_err of the sequential-fp32 emulation against the fp64 reference} on the two
    long-K shapes, both weight families."""
    out = {}
    J, VA, VG, W, ref = C.dense_case(*LONG_DENSE)
    nA, nG = LONG_DENSE[:2]
    out["full"] = rel_err(emulate_dense(J, nA, nG, VA, VG, W[:nt].reshape(nt, -1)), ref[:nt])
    J, VA, VG, wA, wG, ref = S.dense_case(*LONG_DENSE)
    w = (wA[:nt, :, None] * wG[:nt, None, :]).astype(np.float32).reshape(nt, -1)
    out["sweep"] = rel_err(emulate_dense(J, nA, nG, VA, VG, w), ref[:nt])
    a, D, VA, VG, W, ref = C.outer_case(*LONG_OUTER)
    out["outer_full"] = rel_err(emulate_outer_full(a, LONG_OUTER[1], D, VA, VG, W[:nt]), ref[:nt])
    a, D, VA, VG, wA, wG, ref = S.outer_case(*LONG_OUTER)
    out["outer_sweep"] = rel_err(emulate_outer_sweep(a, LONG_OUTER[1], D, VA, VG, wA[:nt], wG[:nt]), ref[:nt])
    return out


# ------------------------------------------------------------------ integer rank-one weights
def int_rank_one(nt, nA, nG, seed=3):
    """(wA (nt, nA), wG (nt, nG)) int64 in {0, 1, 2}, asymmetric: wA[:, 0] = 2, wG[:, 0] = 0."""
    rng = np.random.default_rng(seed)
    wA = rng.integers(0, 3, size=(nt, nA)).astype(np.int64)
    wG = rng.integers(0, 3, size=(nt, nG)).astype(np.int64)
    wA[:, 0] = 2
    wG[:, 0] = 0
    wG[:, -1] = 2
    return wA, wG
