"""The inversion cases of inv_cases.py are what they claim, the fp64 oracle rounded to fp32
meets the bounds the device is held to, and the bounds have teeth (CPU only: numpy stands in
for the kernels)."""
import numpy as np
import pytest

import inv_cases as C

ALL_SIZES = tuple(dict.fromkeys(C.MERGED_SIZES + C.BLOCKED_COMPANIONS))


def _rounded(name, n, kind):
    o = C.oracle(name, n)
    return (o.L if kind == C.CHOL else o.Y).astype(np.float32)


@pytest.mark.parametrize("name", C.NAMES)
def test_oracle_meets_bounds(name):
    """The oracle rounded once to fp32 is within every bound, on every case at every size of
    either path.  Inverse-Cholesky: within the whole bound, which is sharp by construction
    (at n = 1 the residual is the output's rounding error itself, and a diagonal of a
    thousand entries samples it up to 0.99 of the bound on graded_diag; 0.95 on spd_1e8,
    below 0.9 elsewhere), and the fp64 term is at most 1e-3 of the rounding term, so it
    cannot hide an fp32-level defect.  Full inverse: within half the bound, cond(R) <= 1e6."""
    worst = {C.CHOL: (0.0, ""), C.INVERSE: (0.0, "")}
    frac = allow = 0.0
    for n in ALL_SIZES:
        o = C.oracle(name, n)
        f = C.check_chol(o.R, o.G, _rounded(name, n, C.CHOL), C.ORACLE_MARGIN_CHOL, f"{name}-{n}")
        assert f["fp64_inside"] and f["fp64_fraction"] <= C.FP64_FRACTION, (name, n, f)
        worst[C.CHOL] = max(worst[C.CHOL], (f["ratio"], f"{name}-{n}"))
        frac = max(frac, f["fp64_fraction"])
        if C.INVERSE in C.kinds_of(name):
            w = np.linalg.eigvalsh(o.R)
            assert w[0] > 0 and w[-1] / w[0] <= C.INVERSE_COND_LIMIT, (name, n, w[-1] / w[0])
            g = C.check_inverse(o.R, _rounded(name, n, C.INVERSE), C.ORACLE_MARGIN_INV, f"{name}-{n}")
            worst[C.INVERSE] = max(worst[C.INVERSE], (g["ratio"], f"{name}-{n}"))
            h = C.check_forward(o, _rounded(name, n, C.CHOL), f"{name}-{n}")  # (rounding alone: <= 1)
            allow = max(allow, h["fp64_allowance"])
    print(f"INV-HOST {C.family_of(name)}: chol {worst[C.CHOL]} inverse {worst[C.INVERSE]} fp64 fraction {frac:.2e} "
          f"forward allowance {allow:.2e} of 2^-24 max|L|")


@pytest.mark.parametrize("kind", [C.CHOL, C.INVERSE])
def test_oracle_blocked_job(kind):
    """The n = 1537 job every blocked group is built around."""
    f = C.check_output("spd_1e2", C.BLOCKED_N, kind, _rounded("spd_1e2", C.BLOCKED_N, kind),
                       C.ORACLE_MARGIN_CHOL if kind == C.CHOL else C.ORACLE_MARGIN_INV)
    print(f"INV-HOST spd_1e2-{C.BLOCKED_N}-{kind}: {f['ratio']:.3f}")


def test_case_table():
    assert C.MERGED_LARGE == 48 * C.NB_MERGED and C.BLOCKED_N == C.MERGED_LARGE + 1
    assert [-(-n // C.NB_MERGED) for n in C.MERGED_SMALL] == [1, 1, 1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7]
    assert [-(-n // C.NB_BLOCKED) for n in C.BLOCKED_COMPANIONS] == [1, 1, 1, 1, 1, 2, 3, 6, 7, 12, 13]
    assert all(len(c) <= 7 for c in C.BLOCKED_CALLS)
    F, scale, shift = C.problem("kfac_A_1e-4", 97)
    assert F is C.problem("kfac_A_1e-4", 97)[0] and not F.flags.writeable
    assert np.array_equal(F, C.BUILDERS["kfac_A_1e-4"].build(97)[0])
    for name in C.NAMES:  # every F but the two non-symmetric ones is exactly symmetric
        F = C.problem(name, 65)[0]
        assert np.array_equal(F, F.T) == (name not in ("spd_1e2_skew", "spd_1e5_skew", "nonsym_grid")), name


@pytest.mark.parametrize("n", [17, 97, 385])
def test_case_structure(n):
    A = C.problem("kfac_A_1e-4", n)[0].astype(np.float64)
    zero = np.flatnonzero(~A.any(axis=1))
    assert len(zero) == (n - 1) // 4 and not A[:, zero].any() and (A >= 0).all()
    s = np.linalg.svd(A, compute_uv=False)
    r = max(1, n // 8)
    assert s[r - 1] > 1e-4 * s[0] and (r == n or s[r] < 1e-6 * s[0])  # rank r << n
    G = C.problem("kfac_G", n)[0].astype(np.float64)
    assert np.abs(G @ np.ones(n)).max() <= n * 2.0 ** -20 * np.abs(G).max()  # null vector
    n1 = C.block_edge(n)
    Bd = C.problem("block_diag", n)[0]
    assert n1 % 16 and (n - n1) % 16 and not Bd[:n1, n1:].any() and not Bd[n1:, :n1].any()
    o = C.oracle("block_diag", n)
    assert not o.G[:n1, n1:].any() and not o.L[n1:, :n1].any()  # bound exactly 0 off the blocks
    base = C.problem("spd_1e2", n)
    for tag, p in (("scaled_up", 40), ("scaled_dn", -40)):
        F, scale, shift = C.problem(tag, n)
        assert np.array_equal(F.astype(np.float64), base[0].astype(np.float64) * 2.0 ** p)
        assert shift == base[2] * 2.0 ** p and scale == base[1]
    F = C.problem("nonsym_grid", n)[0]
    S = C.sym_part(F)
    assert not np.array_equal(F, F.T) and np.array_equal(S, S.T)
    assert np.array_equal(F.astype(np.float64) * 1024, np.round(F.astype(np.float64) * 1024))
    K = C.problem("spd_1e5_skew", n)[0].astype(np.float64)
    assert ((K + K.T).astype(np.float32).astype(np.float64) != K + K.T).any()  # F + F^T is not fp32


def test_oracle_is_not_cholesky_of_inverse():
    """cholesky(inv(R)), the restatement the rtol = 1e-4 tests compare with, misses the bound
    the triangular route meets."""
    o = C.oracle("spd_1e8", 193)
    alt = np.linalg.cholesky(np.linalg.inv(o.R)).astype(np.float32)
    assert C.figures_chol(o.R, o.G, alt)["ratio"] > 2.0
    assert C.figures_chol(o.R, o.G, o.L.astype(np.float32))["ratio"] <= 1.0


def test_forward_substitution_fallback(monkeypatch):
    """Without scipy the oracle's triangular solve is a plain forward substitution: it meets
    the same bound."""
    monkeypatch.setattr(C, "_solve_triangular", None)
    for name, n in (("spd_1e8", 97), ("graded_diag", 65), ("kfac_A_1e-4", 33)):
        o = C.oracle_of(*C.problem(name, n))
        C.check_chol(o.R, o.G, o.L.astype(np.float32), tag=f"{name}-{n}")
        assert not np.triu(o.L, 1).any()


# ------------------------------------------------------------------------ planted pivots
@pytest.mark.parametrize("n,p", C.PLANTED_MERGED + C.PLANTED_BLOCKED)
def test_planted_pivot_is_found(n, p):
    """The plain elimination finds the first non-positive pivot of P R P at p, and every
    pivot before it is at least 0.1 (fp64 summation order cannot move the index)."""
    F = C.planted(n, p)
    assert np.array_equal(F, F.T)
    got, smallest = C.first_bad_pivot(C.flip(C.damped(F, 1.0, 0.0)))
    assert got == p and smallest >= 0.1, (got, smallest)


@pytest.mark.parametrize("n,i0", C.ZERO_PIVOTS)
def test_zero_pivot_is_found(n, i0):
    F = C.zero_pivot(n, i0)
    assert np.array_equal(F, np.round(F)) and np.array_equal(F, F.T)
    got, smallest = C.first_bad_pivot(C.flip(C.damped(F, 1.0, 0.0)))
    assert got == n - i0 == C.expected_info(F) and smallest >= 1.0
    assert C.expected_info(np.zeros((n, n), np.float32)) == 1
    assert C.expected_info(np.zeros((n, n), np.float32), 1.0, 0.5) == 0


def test_first_bad_pivot_matches_unblocked():
    F = C.planted(200, 129)
    A = C.flip(C.damped(F, 1.0, 0.0))
    assert C.first_bad_pivot(A, block=1)[0] == C.first_bad_pivot(A, block=64)[0] == 129
    assert C.first_bad_pivot(C.oracle("spd_1e5", 97).R)[0] == 0


@pytest.mark.parametrize("nb,cases", [(C.NB_MERGED, C.PLANTED_MERGED),
                                      (C.NB_BLOCKED, C.PLANTED_MERGED + C.PLANTED_BLOCKED)])
@pytest.mark.parametrize("defect", ["off_by_one", "no_nb"])
def test_pivot_index_defects_are_caught(nb, cases, defect):
    """A lane index reported 0-based, or a tile index without `* NB`, misreports at least one
    planted case on either path; the formula as written reports p."""
    assert all(C.reported_index(p, nb) == p for _, p in cases)
    assert any(C.reported_index(p, nb, defect) != p for _, p in cases)


# ------------------------------------------------------------------------ teeth
def _model(F, scale, shift, defect):
    """The kernel's route with one defect planted; returns the fp32 inverse-Cholesky output."""
    n = F.shape[0]
    if defect == "all_fp32":  # the whole computation in fp32
        R = np.float32(scale) * ((F + F.T) * np.float32(0.5)) + np.float32(shift) * np.eye(n, dtype=np.float32)
        Cf = np.linalg.cholesky(C.flip(R))
        assert Cf.dtype == np.float32
        return np.ascontiguousarray(C.flip(np.tril(np.linalg.inv(Cf)).T))
    R = C.damped(F, scale, shift)
    if defect == "sum_fp32":  # F + F^T formed in fp32
        R = scale * (np.float32(0.5) * (F + F.T)).astype(np.float64)
        R[np.diag_indices(n)] += shift
    elif defect == "damping_fp32":  # scale * sym rounded to fp32, the shift added in fp32
        R = (scale * (0.5 * (F.astype(np.float64) + F.T))).astype(np.float32)
        R[np.diag_indices(n)] += np.float32(shift)
        R = R.astype(np.float64)
    elif defect == "lower_triangle_only":  # no symmetrisation: the lower triangle mirrored
        Fl = np.tril(F).astype(np.float64)
        R = scale * (Fl + np.tril(Fl, -1).T)
        R[np.diag_indices(n)] += shift
    elif defect == "tile_update_skipped":
        # R'[1][1] -= C[1][0] C[1][0]^T left out: every later step sees P R P plus that term
        Rp = C.flip(R).copy()
        Cc = np.linalg.cholesky(Rp)
        e = min(n, 64)
        Rp[32:e, 32:e] += Cc[32:e, :32] @ Cc[32:e, :32].T
        R = C.flip(Rp)
    X = C.tri_inv(np.linalg.cholesky(C.flip(R)))
    if defect == "rows_only_flip":
        return np.ascontiguousarray(X.T[::-1, :]).astype(np.float32)
    L = np.ascontiguousarray(C.flip(X.T)).astype(np.float32)
    if defect == "tile_transposed":  # a strictly lower 32 x 32 output tile transposed in place
        m = min(n, 64) - 32
        L[32:32 + m, :m] = L[32:32 + m, :m].T.copy()
    return L


TEETH = {
    "all_fp32": (("kfac_G", 193), ("nonsym_grid", 193), ("graded_diag", 65)),
    "sum_fp32": (("spd_1e2_skew", 33), ("spd_1e5_skew", 65)),
    "damping_fp32": (("spd_1e8", 97), ("block_diag", 97), ("kfac_A_1e-4", 33), ("kfac_A_bench", 193)),
    "lower_triangle_only": (("spd_1e5_skew", 65), ("nonsym_grid", 97)),
    "tile_update_skipped": (("spd_1e2", 65), ("kfac_A_bench", 97)),
    "tile_transposed": (("spd_1e5", 65), ("kfac_G", 97)),
    "rows_only_flip": (("spd_1e2", 33), ("cI", 65)),
}


@pytest.mark.parametrize("defect", TEETH)
def test_defect_misses_the_bound(defect):
    """Each modelled defect fails the inverse-Cholesky check on at least one named case (a
    matrix the defect makes indefinite counts: the kernel would report a pivot)."""
    caught = []
    for name, n in TEETH[defect]:
        F, scale, shift = C.problem(name, n)
        try:
            out = _model(F, scale, shift, defect)
        except np.linalg.LinAlgError:
            caught.append((name, n, "not positive definite"))
            continue
        try:
            C.check_output(name, n, C.CHOL, out)
        except AssertionError as e:
            caught.append((name, n, str(e)))
    print(f"INV-TEETH {defect}: {caught}")
    assert caught, f"{defect} passes on every one of {TEETH[defect]}"
    # and the same route without the defect passes on all of them
    for name, n in TEETH[defect]:
        C.check_output(name, n, C.CHOL, _model(*C.problem(name, n), None))
