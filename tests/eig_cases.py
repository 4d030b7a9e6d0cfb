"""Factor-shaped spectra for the eigensolver (a plain helper module, like x3_exact).

The eigensolver (bnn_kfac_amd/csrc/eig.hip) takes two routes: a two-sided Jacobi in LDS for
n <= 128, and for n > 128 a Householder tridiagonalisation, Sturm multisection, inverse
iteration per cluster (two eigenvalues closer than 1e-7 ||T||_1 form a cluster, only a
cluster is re-orthogonalised) and the back-transform.  Random dense matrices have
well-separated spectra and no zero Householder sub-column, so they reach neither the
cluster rule nor the `tau == 0` and split-tridiagonal paths.  The matrices built here do:

  kfac_A          X^T X / 48 (fp32) of 48 uniform rows, a seeded quarter of the columns
                  exactly zero, a ones column appended: rank <= 48, a cluster of
                  rounding-level eigenvalues, exactly zero rows and columns.
  kfac_A_dn/_up   the same matrix scaled by 2^-60 / 2^+60 (exact scalings).
  kfac_G          g^T g / 48 (fp32), rows of g = softmax(z) - onehot(y): the ones vector
                  is a null vector.
  chain_below / chain_straddle / chain_above
                  Q diag(1 + g i) Q^T with g = 3e-8, 1.5e-7, 1e-6.  ||F||_2 <= ||T||_1 <=
                  3 ||F||_2, so against the rule's 1e-7 ||T||_1 the first is one cluster
                  of n for certain, the last has no cluster for certain, and the middle
                  one lies in the band between, where ||T||_1 decides.  (F is close to I
                  here, so ||T||_1 is close to ||F||_2 and eig.hip as it stands leaves the
                  middle one unclustered too: its 1.4e-7 gaps get no re-orthogonalisation.
                  No case sits on the threshold itself.)
  twin_blocks     blockdiag(B, B) (n odd: plus a 1 x 1 block 0.5): exact double
                  eigenvalues, and the tridiagonal splits.
  glued_wilkinson_raw / glued_wilkinson_perm / glued_wilkinson_rot
                  n / 21 copies of Wilkinson's W21+ (diagonal |i - 10|, off-diagonal 1)
                  glued by 1e-6: the tridiagonal itself (every reflector trivial, every
                  tau zero), a seeded symmetric permutation of it, and Q G Q^T.
  graded          Q diag(10^(-12 i / n)) Q^T.
  cI              3 I.
  diag_repeated   a diagonal of three distinct values in a seeded shuffled order.
  zeros           the zero matrix.
  rank1           q0 q0^T.

Q is a seeded random orthogonal matrix.  Every builder is deterministic (numpy, seeded by
case name and size), returns an exactly symmetric fp32 matrix, and is cached read-only.

The checks judge a solver's output (`ev` fp64 ascending, `V` fp32, column j the vector of
ev[j]) in fp64 on the host against numpy's eigvalsh of the same fp32 matrix.  `scale` is
the largest |eigenvalue| (1 for the zero matrix).  The bounds:

  EV_BOUND   max |ev - eigvalsh(F)| <= 1e-11 scale: the suite's absolute eigenvalue bound
             (test_gpu_eig_variance.py); no relative term, a rounding-level cluster has
             no relative accuracy.
  ORTH_BOUND max |V^T V - I| <= 2^-23.  Rounding a unit fp64 vector to fp32 moves it by at
             most 2^-25 in norm, which changes a dot product or a squared norm by at most
             2^-24; the fp64 algorithm's own loss (~2e-9 by eig.hip's argument) is far
             below that.  2^-23 leaves a factor two.
  RES_BOUND  max |F V - V diag(ev)| <= 2^-23 scale.  The same rounding moves an entry of
             F v by at most 2^-25 ||F|| and of lambda v by 2^-25 |lambda|: 2^-24 scale, and
             again a factor two.

test_eig_cases_host.py asserts that LAPACK's fp64 eigh rounded to fp32 meets all of them
on every case, and that each of four planted defects misses one."""
import functools
import zlib

import numpy as np

JACOBI_SIZES = (33, 128)   # n <= 128: eig_jacobi_lds
TRIDIAG_SIZES = (129, 192)  # n > 128: eig_tridiag + eig_bisect + eig_tri_vectors + back-transform
WILK_SIZES = (126, 147)    # multiples of 21 on either side of the switch
LARGE = 128                # the last Jacobi size

EV_BOUND = 1e-11
ORTH_BOUND = 2.0 ** -23
RES_BOUND = 2.0 ** -23
SAMPLES = 48

CHAIN_GAP = {"chain_below": 3e-8, "chain_straddle": 1.5e-7, "chain_above": 1e-6}


def _rng(tag, n):
    return np.random.default_rng(zlib.crc32(f"{tag}/{n}".encode()))


def _orth(tag, n):
    Q, _ = np.linalg.qr(_rng(tag, n).standard_normal((n, n)))
    return Q


def _sym32(F):
    """fp64 -> fp32, exactly symmetric (the mean of F and F^T is, entry by entry)."""
    return (0.5 * (F + F.T)).astype(np.float32)


def _mirror(F):
    """An fp32 product's upper triangle mirrored: exactly symmetric, no entry re-rounded."""
    return np.triu(F) + np.triu(F, 1).T


def _spectrum(tag, n, lam):
    Q = _orth(tag, n)
    return _sym32((Q * lam) @ Q.T)


def kfac_A(n):
    rng = _rng("kfac_A", n)
    X = rng.random((SAMPLES, n - 1), dtype=np.float32)
    X[:, rng.permutation(n - 1)[:(n - 1) // 4]] = 0.0
    X = np.concatenate([X, np.ones((SAMPLES, 1), np.float32)], axis=1)
    return _mirror((X.T @ X) / np.float32(SAMPLES))


def kfac_G(n):
    rng = _rng("kfac_G", n)
    z = 2.0 * rng.standard_normal((SAMPLES, n))
    p = np.exp(z - z.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    p[np.arange(SAMPLES), rng.integers(0, n, SAMPLES)] -= 1.0
    g = p.astype(np.float32)
    return _mirror((g.T @ g) / np.float32(SAMPLES))


def _chain(name):
    return lambda n: _spectrum(name, n, 1.0 + CHAIN_GAP[name] * np.arange(n))


def twin_blocks(n):
    m = n // 2
    X = _rng("twin_blocks", n).standard_normal((m, m))
    B = (X + X.T).astype(np.float32)
    F = np.zeros((n, n), np.float32)
    F[:m, :m] = B
    F[m:2 * m, m:2 * m] = B
    if n & 1:
        F[n - 1, n - 1] = 0.5
    return F


def _wilkinson(n):
    assert n % 21 == 0
    d = np.tile(np.abs(np.arange(21) - 10.0), n // 21)
    e = np.ones(n - 1)
    e[20::21] = 1e-6
    return np.diag(d) + np.diag(e, 1) + np.diag(e, -1)


def glued_wilkinson_raw(n):
    return _wilkinson(n).astype(np.float32)


def glued_wilkinson_perm(n):
    p = _rng("glued_wilkinson_perm", n).permutation(n)
    return _wilkinson(n)[np.ix_(p, p)].astype(np.float32)


def glued_wilkinson_rot(n):
    Q = _orth("glued_wilkinson_rot", n)
    return _sym32(Q @ glued_wilkinson_raw(n).astype(np.float64) @ Q.T)


def graded(n):
    return _spectrum("graded", n, 10.0 ** (-12.0 * np.arange(n) / n))


def cI(n):
    return (3.0 * np.eye(n)).astype(np.float32)


def diag_repeated(n):
    vals = np.repeat([1.0, 2.0, 5.0], (n + 2) // 3)[:n]
    return np.diag(_rng("diag_repeated", n).permutation(vals)).astype(np.float32)


def zeros(n):
    return np.zeros((n, n), np.float32)


def rank1(n):
    q = _orth("rank1", n)[:, 0]
    return _sym32(np.outer(q, q))


def _scaled(p):
    return lambda n: (kfac_A(n) * np.float32(2.0 ** p)).astype(np.float32)


BUILDERS = {
    "kfac_A": kfac_A, "kfac_G": kfac_G,
    "chain_below": _chain("chain_below"), "chain_straddle": _chain("chain_straddle"),
    "chain_above": _chain("chain_above"),
    "twin_blocks": twin_blocks,
    "glued_wilkinson_raw": glued_wilkinson_raw, "glued_wilkinson_perm": glued_wilkinson_perm,
    "glued_wilkinson_rot": glued_wilkinson_rot,
    "graded": graded, "cI": cI, "diag_repeated": diag_repeated, "zeros": zeros, "rank1": rank1,
    "kfac_A_dn": _scaled(-60), "kfac_A_up": _scaled(60),
}


def sizes_of(name):
    return WILK_SIZES if name.startswith("glued_wilkinson_") else JACOBI_SIZES + TRIDIAG_SIZES


# (case, n), shared by the host test of the data and the GPU test of the kernels
CASES = tuple((name, n) for name in BUILDERS for n in sizes_of(name))
CASE_IDS = tuple(f"{name}-{n}" for name, n in CASES)


@functools.lru_cache(maxsize=None)
def matrix(name, n):
    F = np.ascontiguousarray(BUILDERS[name](n), dtype=np.float32)
    assert F.shape == (n, n) and np.array_equal(F, F.T)
    F.setflags(write=False)
    return F


@functools.lru_cache(maxsize=None)
def lapack(name, n):
    """numpy's fp64 eigh of the fp32 matrix: (w fp64 ascending, V fp32), read-only."""
    w, V = np.linalg.eigh(matrix(name, n).astype(np.float64))
    V = V.astype(np.float32)
    w.setflags(write=False)
    V.setflags(write=False)
    return w, V


def scale_of(want):
    s = float(np.abs(want).max())
    return s if s > 0.0 else 1.0


def figures(F, ev, V, want):
    """The measured quantities of one solve, all in fp64; `want` = eigvalsh of F in fp64."""
    F64 = np.asarray(F, dtype=np.float64)
    ev = np.asarray(ev, dtype=np.float64)
    V64 = np.asarray(V, dtype=np.float64)
    n = F64.shape[0]
    scale = scale_of(want)
    finite = bool(np.isfinite(ev).all() and np.isfinite(V64).all())
    with np.errstate(invalid="ignore", over="ignore"):
        return {
            "scale": scale,
            "finite": finite,
            "ascending": bool(np.all(np.diff(ev) >= 0)),
            "ev": float(np.abs(ev - want).max()) / scale,
            "orth": float(np.abs(V64.T @ V64 - np.eye(n)).max()),
            "res": float(np.abs(F64 @ V64 - V64 * ev).max()) / scale,
        }


def check(F, ev, V, want, info=0):
    """Every check of the module docstring; returns the figures."""
    n = F.shape[0]
    assert int(info) == 0, f"info = {int(info)}"
    assert ev.shape == (n,) and ev.dtype == np.float64
    assert V.shape == (n, n) and V.dtype == np.float32
    f = figures(F, ev, V, want)
    assert f["finite"], "NaN or inf in the output"
    assert f["ascending"], "eigenvalues not ascending"
    assert f["ev"] <= EV_BOUND, f"|ev - eigvalsh| = {f['ev']:.3e} scale > {EV_BOUND:.1e} scale"
    assert f["orth"] <= ORTH_BOUND, f"|V^T V - I| = {f['orth']:.3e} > 2^-23 = {ORTH_BOUND:.3e}"
    assert f["res"] <= RES_BOUND, f"|F V - V ev| = {f['res']:.3e} scale > 2^-23 = {RES_BOUND:.3e} scale"
    return f


def largest_cluster(w, tol):
    """The longest run of ascending eigenvalues whose consecutive gaps are all <= tol."""
    best = run = 1
    for gap in np.diff(w):
        run = run + 1 if gap <= tol else 1
        best = max(best, run)
    return best


# ------------------------------------------------------------------ kfac_syev's launches
GROUP_MAX = 8  # EMAXJ of eig.hip: Jacobi jobs per launch


def jacobi_groups(sizes):
    """The Jacobi launches of one kfac_syev call over jobs of these sizes, as lists of job
    indices (the dispatch loop of eig.hip): small jobs (n <= LARGE) collect in order, and the
    pending group is launched when it holds GROUP_MAX jobs and another small one arrives, at
    every large job (which then runs alone in the same workspace), and at the end."""
    groups, cur = [], []
    for i, n in enumerate(sizes):
        if n > LARGE:
            if cur:
                groups.append(cur)
            cur = []
            continue
        if len(cur) == GROUP_MAX:
            groups.append(cur)
            cur = []
        cur.append(i)
    if cur:
        groups.append(cur)
    return groups


def factor_like(n, seed):
    """A seeded fp32 matrix of size n: kfac_A-style for an even seed and n >= 4 (fewer samples
    than columns, a quarter of the columns zero), else random symmetric."""
    rng = np.random.default_rng(seed)
    if seed % 2 == 0 and n >= 4:
        X = rng.random((max(2, n // 3), n), dtype=np.float32)
        X[:, rng.permutation(n)[:n // 4]] = 0.0
        F = _mirror((X.T @ X) / np.float32(X.shape[0]))
    else:
        X = rng.standard_normal((n, n)).astype(np.float32)
        F = X + X.T
    return np.ascontiguousarray(F, dtype=np.float32)


# the issue's order: every large job closes the pending group, so the Jacobi launches are
# {40}, {7, 128}, {1, 2, 64, 33, 12}, {5} and no group fills
MIXED_SIZES = (40, 129, 7, 128, 160, 1, 2, 64, 33, 12, 130, 5)
# eighteen small jobs in a row (two full groups back to back, then two jobs), a large job in
# the workspace they used, eight jobs of about the largest Jacobi size (a full group after a
# large job), one more that closes it, a large job, a last small one
FULL_SIZES = (33, 5, 128, 64, 12, 1, 40, 2, 7, 100, 128, 3, 17, 90, 31, 64, 8, 20, 129,
              128, 127, 120, 128, 96, 128, 110, 128, 50, 130, 6)
