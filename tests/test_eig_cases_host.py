"""The eigensolver cases of eig_cases.py are what they claim, and its checks have teeth
(CPU only: numpy's fp64 eigh stands in for the solver)."""
import numpy as np
import pytest

import eig_cases as E

# cases whose spectrum has no gap wide enough for a swapped pair of columns to show in the
# residual (one eigenvalue, or a chain of total width n g <= 2e-4)
NO_WIDE_GAP = ("cI", "zeros", "chain_below", "chain_straddle", "chain_above")


@pytest.mark.parametrize("name,n", E.CASES, ids=E.CASE_IDS)
def test_reference_passes(name, n):
    """LAPACK in fp64, V rounded to fp32, meets every bound the device is held to."""
    F = E.matrix(name, n)
    w, V = E.lapack(name, n)
    f = E.check(F, w.copy(), V, w)
    print(f"{name}-{n}: orth {f['orth']:.2e} res {f['res']:.2e} scale")


def test_case_table():
    assert len(set(E.CASES)) == len(E.CASES)
    for name, n in E.CASES:
        assert (n <= E.LARGE) == (n in E.JACOBI_SIZES or n == E.WILK_SIZES[0])
    for name in E.BUILDERS:
        ns = E.sizes_of(name)
        assert any(n <= E.LARGE for n in ns) and any(n > E.LARGE for n in ns)  # both routes
    # every call returns the same read-only array
    F = E.matrix("kfac_A", 33)
    assert F is E.matrix("kfac_A", 33) and not F.flags.writeable
    assert np.array_equal(F, E.BUILDERS["kfac_A"](33))


@pytest.mark.parametrize("n", E.JACOBI_SIZES + E.TRIDIAG_SIZES)
def test_kfac_A_structure(n):
    F = E.matrix("kfac_A", n)
    zero_rows = np.flatnonzero(~F.any(axis=1))
    assert len(zero_rows) == (n - 1) // 4
    assert not F[:, zero_rows].any()
    rank = min(E.SAMPLES, n - len(zero_rows))
    s = np.linalg.svd(F.astype(np.float64), compute_uv=False)
    assert s[rank - 1] > 1e-4 * s[0] and np.all(s[rank:] < 1e-6 * s[0])
    # a cluster of n - rank eigenvalues at rounding level
    w, _ = E.lapack("kfac_A", n)
    assert E.largest_cluster(w, 1e-7 * s[0]) >= n - rank
    for tag, p in (("kfac_A_dn", -60), ("kfac_A_up", 60)):  # exact scalings
        assert np.array_equal(E.matrix(tag, n).astype(np.float64), F.astype(np.float64) * 2.0 ** p)


@pytest.mark.parametrize("n", E.JACOBI_SIZES + E.TRIDIAG_SIZES)
def test_kfac_G_null_vector(n):
    """Rows of g sum to zero up to their fp32 rounding (<= n 2^-25 each), so
    |F 1| <= n 2^-25 max|g| plus the fp32 product's own rounding: far below n 2^-20 |F|max,
    where a matrix without the null vector has |F 1| of the order of its eigenvalues."""
    F = E.matrix("kfac_G", n).astype(np.float64)
    w, _ = E.lapack("kfac_G", n)
    assert np.abs(F @ np.ones(n)).max() <= n * 2.0 ** -20 * np.abs(F).max()
    assert abs(w[0]) <= 1e-6 * w[-1] and w[-1] > 0


@pytest.mark.parametrize("n", E.JACOBI_SIZES + E.TRIDIAG_SIZES)
def test_chain_gaps(n):
    """Against the cluster rule 1e-7 ||T||_1 with ||F|| <= ||T||_1 <= 3 ||F||: every gap of
    chain_below is inside it whatever ||T||_1 is, every gap of chain_above outside it, and
    chain_straddle's gaps lie in the band between."""
    for name in ("chain_below", "chain_straddle", "chain_above"):
        w, _ = E.lapack(name, n)
        gaps, norm = np.diff(w), np.abs(w).max()
        print(f"{name}-{n}: gaps {gaps.min() / norm:.3e} .. {gaps.max() / norm:.3e} ||F||")
        if name == "chain_below":
            assert np.all(gaps < 1e-7 * norm)
        elif name == "chain_above":
            assert np.all(gaps > 3e-7 * norm)
        else:
            assert np.all((gaps > 1e-7 * norm) & (gaps < 3e-7 * norm))


@pytest.mark.parametrize("n", E.JACOBI_SIZES + E.TRIDIAG_SIZES)
def test_twin_blocks_double_eigenvalues(n):
    F = E.matrix("twin_blocks", n)
    m = n // 2
    assert np.array_equal(F[:m, :m], F[m:2 * m, m:2 * m])
    assert not F[:m, m:].any() and not F[2 * m:, :2 * m].any()
    wB = np.linalg.eigvalsh(F[:m, :m].astype(np.float64))
    both = np.sort(np.concatenate([wB, wB, [0.5]] if n & 1 else [wB, wB]))
    w, _ = E.lapack("twin_blocks", n)
    np.testing.assert_allclose(w, both, rtol=0, atol=1e-13 * np.abs(w).max())


@pytest.mark.parametrize("n", E.WILK_SIZES)
def test_wilkinson_forms(n):
    G = E.matrix("glued_wilkinson_raw", n)
    assert not np.triu(G, 2).any()  # tridiagonal: every Householder sub-column is zero
    assert np.count_nonzero(np.diag(G, 1) == np.float32(1e-6)) == n // 21 - 1
    w = E.lapack("glued_wilkinson_raw", n)[0]
    np.testing.assert_allclose(E.lapack("glued_wilkinson_perm", n)[0], w, rtol=0, atol=1e-13 * w[-1])
    np.testing.assert_allclose(E.lapack("glued_wilkinson_rot", n)[0], w, rtol=0, atol=1e-5 * w[-1])
    # the glued copies' top eigenvalues: one cluster of 2 n / 21
    assert E.largest_cluster(w, 1e-7 * w[-1]) >= 2 * (n // 21)


# ------------------------------------------------------------------ the checks have teeth
def _fails(F, ev, V, want):
    with pytest.raises(AssertionError):
        E.check(F, ev, V, want)


@pytest.mark.parametrize("name,n", E.CASES, ids=E.CASE_IDS)
def test_mixed_pair_fails(name, n):
    """The two vectors of the closest pair mixed by an angle of 1e-6, not re-orthogonalised."""
    F = E.matrix(name, n)
    w, V = E.lapack(name, n)
    a = int(np.argmin(np.diff(w)))
    V = V.copy()
    V[:, a] = V[:, a] + np.float32(1e-6) * V[:, a + 1]
    _fails(F, w.copy(), V, w)


@pytest.mark.parametrize("name,n", [c for c in E.CASES if c[0] not in NO_WIDE_GAP],
                         ids=[i for c, i in zip(E.CASES, E.CASE_IDS) if c[0] not in NO_WIDE_GAP])
def test_swapped_columns_fail(name, n):
    F = E.matrix(name, n)
    w, V = E.lapack(name, n)
    V = V.copy()
    V[:, [0, n - 1]] = V[:, [n - 1, 0]]
    _fails(F, w.copy(), V, w)


@pytest.mark.parametrize("name,n", E.CASES, ids=E.CASE_IDS)
def test_duplicated_column_fails(name, n):
    F = E.matrix(name, n)
    w, V = E.lapack(name, n)
    V = V.copy()
    V[:, n // 2] = V[:, n // 2 - 1]
    _fails(F, w.copy(), V, w)


@pytest.mark.parametrize("name,n", E.CASES, ids=E.CASE_IDS)
def test_moved_eigenvalue_fails(name, n):
    F = E.matrix(name, n)
    w, V = E.lapack(name, n)
    for k in (0, n // 2, n - 1):
        ev = w.copy()
        ev[k] += 1e-9 * E.scale_of(w)
        _fails(F, ev, V, w)


def test_other_defects_fail():
    F = E.matrix("kfac_A", 129)
    w, V = E.lapack("kfac_A", 129)
    with pytest.raises(AssertionError):
        E.check(F, w.copy(), V, w, info=-1)
    bad = V.copy()
    bad[5, 7] = np.nan
    _fails(F, w.copy(), bad, w)
    _fails(F, w[::-1].copy(), V[:, ::-1].copy(), w)


# ------------------------------------------------------------------ groups and workspace
def test_jacobi_groups_of_the_mixed_orders():
    assert E.jacobi_groups(E.MIXED_SIZES) == [[0], [2, 3], [5, 6, 7, 8, 9], [11]]
    g = E.jacobi_groups(E.FULL_SIZES)
    assert [len(x) for x in g] == [8, 8, 2, 8, 1, 1]
    assert g[0] == list(range(8)) and g[1] == list(range(8, 16))  # two full groups in a row
    assert E.FULL_SIZES[18] > E.LARGE and g[3] == list(range(19, 27))  # a full one after a large job


def _eig_jobs(sizes, vectors):
    from bnn_kfac_amd import _native as N
    jobs = []
    for n, v in zip(sizes, vectors):
        j = N.EigJob()
        j.F, j.ldF, j.n, j.evals, j.evecs, j.ldv = 1, n, n, 1, (1 if v else 0), n
        jobs.append(j)
    return N.as_array(N.EigJob, jobs), len(jobs)


@pytest.mark.parametrize("order", ["mixed", "full", "tiny_large_eight", "eight_large_eight"])
def test_eig_workspace_covers_every_launch(order):
    """kfac_eig_workspace_bytes (a host query, no GPU) is the largest need of any launch of
    the call: a Jacobi group's n x n fp64 eigenvector matrices (256-byte aligned each), or a
    large job's own plan.  `tiny_large_eight`: five 1 x 1 jobs, a values-only large job, eight
    128 x 128 jobs -- a full group that starts right after a large job."""
    from bnn_kfac_amd import _native as N
    L = N.lib()
    sizes, vectors = {
        "mixed": (E.MIXED_SIZES, None),
        "full": (E.FULL_SIZES, None),
        "tiny_large_eight": ((1,) * 5 + (129,) + (128,) * 8, (1,) * 5 + (0,) + (1,) * 8),
        "eight_large_eight": ((128,) * 8 + (129,) + (128,) * 8, (1,) * 8 + (0,) + (1,) * 8),
    }[order]
    vectors = vectors or (1,) * len(sizes)
    align = lambda b: (b + 255) // 256 * 256  # noqa: E731
    need = max(sum(align(sizes[i] ** 2 * 8) for i in g) for g in E.jacobi_groups(sizes))
    for n, v in zip(sizes, vectors):
        if n > E.LARGE:
            need = max(need, L.kfac_eig_workspace_bytes(*_eig_jobs([n], [v])))
    assert L.kfac_eig_workspace_bytes(*_eig_jobs(sizes, vectors)) == need
