"""Matrices, fp64 oracle and rounding-derived bounds for the fp64 inversion (a plain helper
module, like eig_cases).

The kernels (bnn_kfac_amd/csrc/invert*.hip, invert_tiles.inc) compute, in fp64 with one
rounding to fp32 at the end,

    R = scale (F + F^T)/2 + shift I,   C = chol(P R P),   X = C^-1,
    L = P X^T P  (KFAC_OUT_INV_CHOL),  Y = L L^T = R^-1  (KFAC_OUT_INVERSE),

P the exchange (flip) matrix.  `oracle` follows the same route in numpy: LAPACK's fp64
Cholesky of the flipped matrix, then a triangular solve (scipy's when it imports, a forward
substitution otherwise).  It is NOT cholesky(inv(R)): the explicit inverse loses cond(R)
units of fp64 rounding before the second factorisation, and from cond(R) = 1e6 on that
restatement itself misses the bound below (by 13 to 1e5 units of 2^-24), while the
triangular route stays under two units up to cond 1e12.  That is why test_gpu_invert.py,
which compares with cholesky(inv(R)), could not be tighter than rtol 1e-4.

Bounds (elementwise; Lh / Yh the fp32 output taken to fp64, U = 2^-24):

  KFAC_OUT_INV_CHOL   |Lh^T R Lh - I| <= 2 U (1 + 2^-10) B + 4 (n + 1) 2^-53 G
      B = |Lh|^T |R| |Lh|: each of the two L factors is off by at most U relative (the
      output's one rounding); (1 + 2^-10) absorbs the second-order term and the use of Lh
      for L in B.  G = P (M M^T) P, M = |X| |C| from the oracle's own factors: the fp64
      Cholesky and triangular inversion (Higham, Accuracy and Stability of Numerical
      Algorithms, Thm 10.3 and 8.5).  Where B and G are 0 (off-block entries of a
      block-diagonal R) the residual must be exactly 0.  The strict upper triangle must be
      exactly 0 and the diagonal > 0: with the residual bound that makes Lh THE Cholesky
      factor of R^-1 (P X^T alone, the flip applied to rows only, has a zero residual too).
  KFAC_OUT_INVERSE    |R Yh - I| <= 2 U |R| |Yh|, Yh bitwise symmetric.
      One rounding gives U; the other factor of two is headroom for the fp64 part, which
      for the inverse has no condition-free elementwise bound, so the cases run with this
      kind keep cond(R) <= 1e6 and test_inv_cases_host.py shows the oracle within half the
      bound on each.

  forward (inverse-Cholesky, the cases with cond(R) <= 1e6)
      |Lh - L| <= U |L| + 4 n^2 2^-53 kF ||L||_F,  kF = ||R||_F ||R^-1||_F >= cond_2(R).
      The residual bounds cannot see a relative perturbation of R itself below U (F + F^T or
      the damping formed in fp32): |Lh^T dR Lh| <= U B by the argument that gives the bound.
      The forward error can.  To first order L(R + dR) - L = -L low(L^T dR L) (low: the
      lower triangle with half the diagonal), so ||dL||_F <= ||L||_2 ||R^-1||_2 ||dR||_F
      <= cond_2(R) eps ||L||_2 for ||dR||_F <= eps ||R||_2.  The fp64 Cholesky's backward
      error is |dA| <= (n + 1) 2^-53 |C||C|^T with || |C||C|^T ||_F <= tr(A) <= n ||A||_2
      (Higham Thm 10.3), the triangular inversion's residual is of the same form (Thm 8.5):
      eps <= 2 n (n + 1) 2^-53, taken as 4 n^2 2^-53 for the oracle's own like error.  The
      allowance is a norm and grows with n^2 and cond(R), so this check has its teeth at
      small n: F + F^T formed in fp32 (modelled in test_inv_cases_host.py) is 96 times over
      it on spd_1e2_skew-33 and 19 times on spd_1e5_skew-65, and inside it at n = 193.

Cases (fp32, deterministic, seeded by name and size; each carries its (scale, shift)):

  spd_1e2 / spd_1e5 / spd_1e8   Q diag(lambda) Q^T, lambda log-spaced over [1e-2 / cond, 1],
                  shift 1 / cond (added in fp64 by the kernel: it sets the floor, the fp32
                  rounding of F moves the small eigenvalues by more than 1e-8).  1e8 runs
                  with the inverse-Cholesky kind only.
  spd_1e2_skew / spd_1e5_skew   the same plus a random antisymmetric part, rounded entry by
                  entry: F + F^T is not representable in fp32.
  kfac_A_bench / kfac_A_1e-4 / kfac_A_1e-3
                  X^T X / r, X >= 0, r = max(1, n / 8) rows, a quarter of the columns
                  exactly zero; at the bench's damping (sqrt 200, sqrt 0.04) and with
                  scale 1 and shift 1e-4, 1e-3.
  kfac_G          g^T g / 48, rows of g = softmax(z) - onehot(y): the ones vector is a null
                  vector; shift 1e-3.
  cI              3 I.
  graded_diag     diag(10^-6 .. 10^6) + 1e-7 off the diagonal (cond 1e12; inverse-Cholesky).
  block_diag      two SPD blocks whose edge is no multiple of 16.
  zeros           the zero matrix, shift 0.5.
  scaled_up / scaled_dn   spd_1e2 and its shift times 2^40 / 2^-40 (exact scalings).
  nonsym_grid     F = S + K, entries on a 2^-10 grid, K antisymmetric: S = (F + F^T)/2 is
                  itself fp32 (`sym_part`), and a run on F must equal a run on S bit for bit.

Planted non-positive pivots: `planted(n, p)` is fp32(P R' P), R' = Lam D Lam^T with Lam unit
lower (entries uniform in +-1/sqrt(n)), D uniform in [0.5, 2] but D[p] = -1 (scale 1, shift
0), so the first non-positive pivot of chol(P R P) is p; `zero_pivot(n, i0)` is an integer
diagonally dominant matrix with row and column i0 zeroed (pivot n - i0 is exactly 0).
`first_bad_pivot` is the plain fp64 elimination that gives the expected index."""
import functools
import zlib
from collections import namedtuple

import numpy as np

try:
    from scipy.linalg import solve_triangular as _solve_triangular
except Exception:  # scipy is optional
    _solve_triangular = None

U = 2.0 ** -24
CHOL_ROUND = 2.0 ** -23 * (1 + 2.0 ** -10)
INV_ROUND = 2.0 ** -23
# the oracle rounded to fp32, in units of the whole bound: the inverse-Cholesky bound is sharp
# (a diagonal entry's residual IS its rounding error), the inverse keeps a factor two
ORACLE_MARGIN_CHOL = 1.0
ORACLE_MARGIN_INV = 0.5
FP64_FRACTION = 1e-3       # fp64 term / rounding term, at most

CHOL, INVERSE = "chol", "inverse"

NB_MERGED, NB_BLOCKED = 32, 64
# merged path (32-tiles, 16-wide diagonal blocks, tasks 2w-1 and 2w paired): T = 1..7, 48
MERGED_SIZES = (1, 15, 16, 17, 31, 32, 33, 64, 65, 96, 97, 161, 193, 1536)
MERGED_SMALL = MERGED_SIZES[:-1]
MERGED_LARGE = MERGED_SIZES[-1]
# blocked path (64-tiles, PANEL_BLOCK = 6): companions of one n = 1537 job, T = 1, 2, 3,
# 6, 7, 12, 13: the edges of the tile, of a panel block and of the first look-ahead split
BLOCKED_N = 1537
BLOCKED_CALLS = ((1, 16, 17, 63, 64, 65), (129, 384, 385, 768, 769))
BLOCKED_COMPANIONS = BLOCKED_CALLS[0] + BLOCKED_CALLS[1]

PLANTED_MERGED = ((1, 1), (17, 16), (17, 17), (33, 32), (33, 33), (40, 1), (65, 64), (65, 65),
                  (100, 49), (129, 97), (200, 129))
PLANTED_BLOCKED = ((1537, 1537), (1537, 1))
ZERO_PIVOTS = ((40, 5), (65, 0), (70, 69), (97, 32))  # (n, i0): info = n - i0


def _rng(tag, n):
    return np.random.default_rng(zlib.crc32(f"{tag}/{n}".encode()))


def _orth(tag, n):
    Q, _ = np.linalg.qr(_rng(tag, n).standard_normal((n, n)))
    return Q


def flip(A):
    return A[::-1, ::-1]


# ------------------------------------------------------------------------ builders
def _spd64(tag, n, cond):
    lam = np.logspace(-2 - np.log10(cond), 0, n) if n > 1 else np.ones(1)
    Q = _orth(tag, n)
    S = (Q * lam) @ Q.T
    return (S + S.T) / 2


def _spd(cond):
    def build(n):
        return _spd64(f"spd{cond:g}", n, cond).astype(np.float32), 1.0, 1.0 / cond
    return build


def _spd_skew(cond):
    def build(n):
        S = _spd64(f"spd{cond:g}", n, cond)
        K = np.tril(_rng("skew", n).standard_normal((n, n)), -1) * (0.1 / np.sqrt(n))
        return (S + K - K.T).astype(np.float32), 1.0, 1.0 / cond
    return build


def _kfac_A64(n):
    rng = _rng("kfac_A", n)
    r = max(1, n // 8)
    X = rng.uniform(0.0, 2.0 / np.sqrt(n), (r, n)).astype(np.float32)
    X[:, rng.permutation(n)[:(n - 1) // 4]] = 0.0
    X = X.astype(np.float64)
    return X.T @ X / r


def _kfac_A(scale, shift):
    def build(n):
        return _kfac_A64(n).astype(np.float32), scale, shift
    return build


def _kfac_G(n):
    rng = _rng("kfac_G", n)
    z = rng.standard_normal((48, n)) * 2.0
    g = np.exp(z - z.max(axis=1, keepdims=True))
    g /= g.sum(axis=1, keepdims=True)
    g[np.arange(48), rng.integers(0, n, 48)] -= 1.0
    g = g.astype(np.float32).astype(np.float64)
    return (g.T @ g / 48).astype(np.float32), 1.0, 1e-3


def _cI(n):
    return (3.0 * np.eye(n)).astype(np.float32), 1.0, 0.0


def _graded_diag(n):
    F = np.full((n, n), 1e-7)
    F[np.diag_indices(n)] = np.logspace(-6, 6, n) if n > 1 else 1.0
    return F.astype(np.float32), 1.0, 0.0


def block_edge(n):
    """Size of the first block of block_diag(n): no multiple of 16 (for n > 2), so the edge
    falls inside a tile and inside a 16-wide diagonal block, on either side of the flip."""
    n1 = n // 2
    while n > 2 and (n1 % 16 == 0 or (n - n1) % 16 == 0):
        n1 += 1
    return n1


def _block_diag(n):
    n1 = block_edge(n)
    F = np.zeros((n, n))
    if n1:
        F[:n1, :n1] = _spd64("blockA", n1, 1e2)
    F[n1:, n1:] = 2.0 * _spd64("blockB", n - n1, 1e3)
    return F.astype(np.float32), 1.0, 1e-2


def _zeros(n):
    return np.zeros((n, n), np.float32), 7.0, 0.5


def _scaled(p):
    def build(n):
        F, scale, shift = _spd(1e2)(n)
        return (F.astype(np.float64) * 2.0 ** p).astype(np.float32), scale, shift * 2.0 ** p
    return build


def _nonsym_grid(n):
    rng = _rng("nonsym_grid", n)
    Q = _orth("nonsym_grid_q", n)
    S = (Q * np.linspace(0.0, 1.0, n)) @ Q.T
    S = np.round((S + S.T) / 2 * 1024) / 1024
    K = np.tril(np.round(rng.uniform(-0.5, 0.5, (n, n)) * 1024) / 1024, -1)
    # eigenvalues of the gridded S are within sqrt(n) 2^-10 of [0, 1]: shift 0.1 keeps R SPD
    return (S + K - K.T).astype(np.float32), 1.0, 0.1


Case = namedtuple("Case", "build kinds family")
BUILDERS = {
    "spd_1e2": Case(_spd(1e2), (CHOL, INVERSE), "spd"),
    "spd_1e5": Case(_spd(1e5), (CHOL, INVERSE), "spd"),
    "spd_1e8": Case(_spd(1e8), (CHOL,), "spd"),
    "spd_1e2_skew": Case(_spd_skew(1e2), (CHOL, INVERSE), "spd"),
    "spd_1e5_skew": Case(_spd_skew(1e5), (CHOL, INVERSE), "spd"),
    "kfac_A_bench": Case(_kfac_A(200 ** 0.5, 0.04 ** 0.5), (CHOL, INVERSE), "kfac_A"),
    "kfac_A_1e-4": Case(_kfac_A(1.0, 1e-4), (CHOL, INVERSE), "kfac_A"),
    "kfac_A_1e-3": Case(_kfac_A(1.0, 1e-3), (CHOL, INVERSE), "kfac_A"),
    "kfac_G": Case(_kfac_G, (CHOL, INVERSE), "kfac_G"),
    "cI": Case(_cI, (CHOL, INVERSE), "cI"),
    "graded_diag": Case(_graded_diag, (CHOL,), "graded_diag"),
    "block_diag": Case(_block_diag, (CHOL, INVERSE), "block_diag"),
    "zeros": Case(_zeros, (CHOL, INVERSE), "zeros"),
    "scaled_up": Case(_scaled(40), (CHOL, INVERSE), "scaled"),
    "scaled_dn": Case(_scaled(-40), (CHOL, INVERSE), "scaled"),
    "nonsym_grid": Case(_nonsym_grid, (CHOL, INVERSE), "nonsym"),
}
NAMES = tuple(BUILDERS)
FAMILIES = tuple(dict.fromkeys(c.family for c in BUILDERS.values()))
INVERSE_COND_LIMIT = 1e6


def kinds_of(name):
    return BUILDERS[name].kinds


def family_of(name):
    return BUILDERS[name].family


@functools.lru_cache(maxsize=None)
def _problem_small(name, n):
    F, scale, shift = BUILDERS[name].build(n)
    assert F.dtype == np.float32 and F.shape == (n, n)
    F.flags.writeable = False
    return F, float(scale), float(shift)


@functools.lru_cache(maxsize=4)
def _problem_large(name, n):
    return _problem_small.__wrapped__(name, n)


def problem(name, n):
    """(F fp32 read-only, scale, shift) of a case; cached."""
    return (_problem_small if n <= 800 else _problem_large)(name, n)


def sym_part(F):
    """(F + F^T)/2 as fp32; asserts that it is exact."""
    S = (F.astype(np.float64) + F.astype(np.float64).T) / 2
    S32 = S.astype(np.float32)
    assert np.array_equal(S32.astype(np.float64), S)
    return S32


# ------------------------------------------------------------------------ oracle
def damped(F, scale, shift):
    """R = scale (F + F^T)/2 + shift I in fp64."""
    F = np.asarray(F, dtype=np.float64)
    R = scale * (0.5 * (F + F.T))
    R[np.diag_indices_from(R)] += shift
    return R


def tri_inv(C):
    """Inverse of a lower triangular fp64 matrix by a triangular solve."""
    n = C.shape[0]
    if _solve_triangular is not None:
        return np.tril(_solve_triangular(C, np.eye(n), lower=True))
    X = np.zeros((n, n))
    for i in range(n):  # forward substitution, row by row
        X[i, :i] = -(C[i, :i] @ X[:i, :i]) / C[i, i]
        X[i, i] = 1.0 / C[i, i]
    return X


Oracle = namedtuple("Oracle", "R L Y G")


def oracle_of(F, scale, shift):
    """The kernel's own route in fp64: R, L = P X^T P, Y = L L^T, and G = P (M M^T) P with
    M = |X| |C| for the bound's fp64 term."""
    R = damped(F, scale, shift)
    C = np.linalg.cholesky(flip(R))
    X = tri_inv(C)
    L = np.ascontiguousarray(flip(X.T))
    M = np.abs(X) @ np.abs(C)
    return Oracle(R, L, L @ L.T, np.ascontiguousarray(flip(M @ M.T)))


@functools.lru_cache(maxsize=None)
def _oracle_small(name, n):
    return oracle_of(*problem(name, n))


@functools.lru_cache(maxsize=2)
def _oracle_large(name, n):
    return oracle_of(*problem(name, n))


def oracle(name, n):
    return (_oracle_small if n <= 800 else _oracle_large)(name, n)


# ------------------------------------------------------------------------ checks
def figures_chol(R, G, Lh):
    """Figures of an inverse-Cholesky output against its bound (nothing asserted)."""
    n = R.shape[0]
    L = np.asarray(Lh, dtype=np.float64)
    aL = np.abs(L)
    res = np.abs(L.T @ R @ L - np.eye(n))
    t1 = CHOL_ROUND * (aL.T @ np.abs(R) @ aL)
    t2 = 4 * (n + 1) * 2.0 ** -53 * G
    bound = t1 + t2
    pos = bound > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = float(np.max(res[pos] / bound[pos])) if pos.any() else 0.0
        frac = float(np.max(t2[t1 > 0] / t1[t1 > 0])) if (t1 > 0).any() else 0.0
    return {"ratio": ratio, "fp64_fraction": frac,
            "zero_exact": not res[~pos].any(),           # bound 0: residual exactly 0
            "fp64_inside": not t2[~(t1 > 0)].any(),      # no fp64 term where B is 0
            "upper_zero": not np.triu(np.asarray(Lh), 1).any(),
            "diag_positive": bool((np.diagonal(L) > 0).all())}


def check_chol(R, G, Lh, limit=1.0, tag=""):
    f = figures_chol(R, G, Lh)
    assert f["upper_zero"], f"{tag}: the strict upper triangle is not exactly 0"
    assert f["diag_positive"], f"{tag}: a diagonal entry is not > 0"
    assert f["ratio"] <= limit, f"{tag}: residual {f['ratio']:.3g} of the bound (limit {limit})"
    assert f["zero_exact"], f"{tag}: residual not exactly 0 where the bound is 0"
    return f


def figures_inverse(R, Yh):
    n = R.shape[0]
    Y = np.asarray(Yh, dtype=np.float64)
    res = np.abs(R @ Y - np.eye(n))
    bound = INV_ROUND * (np.abs(R) @ np.abs(Y))
    pos = bound > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = float(np.max(res[pos] / bound[pos])) if pos.any() else 0.0
    return {"ratio": ratio, "zero_exact": not res[~pos].any(),
            "symmetric": bool(np.array_equal(np.asarray(Yh), np.asarray(Yh).T))}


def check_inverse(R, Yh, limit=1.0, tag=""):
    f = figures_inverse(R, Yh)
    assert f["symmetric"], f"{tag}: the inverse is not bitwise symmetric"
    assert f["ratio"] <= limit, f"{tag}: residual {f['ratio']:.3g} of the bound (limit {limit})"
    assert f["zero_exact"], f"{tag}: residual not exactly 0 where the bound is 0"
    return f


def figures_forward(o, Lh):
    """Forward error of an inverse-Cholesky output against the oracle `o`, in units of
    U |L| + 4 n^2 2^-53 kF ||L||_F (module docstring)."""
    n = o.R.shape[0]
    tau = 4.0 * n * n * 2.0 ** -53 * np.linalg.norm(o.R) * np.linalg.norm(o.Y) * np.linalg.norm(o.L)
    with np.errstate(invalid="ignore"):
        ratio = float(np.max(np.abs(np.asarray(Lh, dtype=np.float64) - o.L) / (U * np.abs(o.L) + tau)))
    return {"forward": ratio, "fp64_allowance": tau / (U * float(np.abs(o.L).max()))}


def check_forward(o, Lh, tag=""):
    f = figures_forward(o, Lh)
    assert f["forward"] <= 1.0, f"{tag}: forward error {f['forward']:.3g} of its bound"
    return f


def check_output(name, n, kind, out, limit=1.0):
    """Check a device (or model) output of case (name, n); returns the figures."""
    o = oracle(name, n)
    tag = f"{name}-{n}-{kind}"
    if kind == CHOL:
        f = check_chol(o.R, o.G, out, limit, tag)
        if INVERSE in kinds_of(name):  # cond(R) <= 1e6
            f.update(check_forward(o, out, tag))
        return f
    return check_inverse(o.R, out, limit, tag)


# ------------------------------------------------------------------------ planted pivots
@functools.lru_cache(maxsize=None)
def planted(n, p):
    """fp32 F (scale 1, shift 0) whose flipped matrix P F P has its first non-positive
    pivot at p (1-based)."""
    rng = _rng(f"planted{p}", n)
    Lam = np.tril(rng.uniform(-1.0, 1.0, (n, n)) / np.sqrt(n), -1) + np.eye(n)
    D = rng.uniform(0.5, 2.0, n)
    D[p - 1] = -1.0
    Rp = (Lam * D) @ Lam.T
    F = np.ascontiguousarray(flip((Rp + Rp.T) / 2)).astype(np.float32)
    F.flags.writeable = False
    return F


@functools.lru_cache(maxsize=None)
def zero_pivot(n, i0):
    """Integer, diagonally dominant, row and column i0 (0-based) zeroed: with scale 1 and
    shift 0, pivot n - i0 of P F P is exactly 0 and every pivot before it is positive."""
    K = np.tril(_rng(f"zero{i0}", n).integers(-1, 2, (n, n)), -1).astype(np.float64)
    F = K + K.T + (n + 1) * np.eye(n)
    F[i0, :] = 0.0
    F[:, i0] = 0.0
    F = F.astype(np.float32)
    F.flags.writeable = False
    return F


def first_bad_pivot(A, block=64):
    """Plain fp64 elimination (A = Lam D Lam^T, no pivoting, no square roots) of a symmetric
    matrix: (1-based index of the first pivot that is not > 0, or 0; the smallest pivot
    before it).  The trailing matrix takes a block of eliminated columns in one product."""
    A = np.array(A, dtype=np.float64)
    n = A.shape[0]
    d = np.empty(n)
    for b0 in range(0, n, block):
        b1 = min(n, b0 + block)
        for k in range(b0, b1):
            d[k] = A[k, k]
            if not d[k] > 0:
                return k + 1, (float(d[:k].min()) if k else np.inf)
            l = A[k + 1:, k] / d[k]
            A[k + 1:, k + 1:b1] -= np.outer(l, A[k, k + 1:b1])
            A[k + 1:, k] = l
        if b1 < n:
            Lp = A[b1:, b0:b1]
            A[b1:, b1:] -= (Lp * d[b0:b1]) @ Lp.T
    return 0, float(d.min())


def expected_info(F, scale=1.0, shift=0.0):
    """The index the header promises: the first non-positive pivot of P R P, 1-based."""
    return first_bad_pivot(flip(damped(F, scale, shift)))[0]


def reported_index(p, nb, defect=None):
    """What check_pivots reports for a first bad pivot p with tile edge nb: tile d, lane c,
    d nb + ffs(ballot); `defect`: "off_by_one" (the 0-based lane) or "no_nb" (d + ffs)."""
    d, c = divmod(p - 1, nb)
    if defect == "off_by_one":
        return d * nb + c
    if defect == "no_nb":
        return d + c + 1
    return d * nb + c + 1
