"""CPU: the host side of the Monte-Carlo GLM predictive -- the layout of kfac_draw_job /
kfac_draw_outer_job against the header, argument validation of kfac_glm_draws /
kfac_glm_draws_outer / kfac_softmax_mc before any launch, the workspace queries, the two
reference formulas of glm_mc_cases against each other, and the int64 bound of every integer
case the GPU test compares bit for bit.  No GPU calls."""
import ctypes

import numpy as np
import pytest
import torch

import glm_mc_cases as C
from abi_layout import c_layout

OUT, WS = 1 << 16, 1 << 17  # (pointers are never dereferenced: validation precedes any launch)


def _dense_job(N, nA=5, nG=3):
    return N.DrawJob(N.CovJob(1 << 12, nA * nG, nA, nG, 1 << 13, nA, 1 << 14, nG, 1, 1), 1 << 18, nA * nG)


def _outer_job(N, cols=4, has_ones=1, nG=3):
    return N.DrawOuterJob(N.CovOuterJob(1 << 12, cols, cols, has_ones, 1 << 13, nG, nG, 0, 1 << 14,
                                        cols + has_ones, 1 << 15, nG, 1, 1), 1 << 18, (cols + has_ones) * nG)


def test_draw_struct_layout(tmp_path):
    from bnn_kfac_amd import _native as N
    got = (c_layout(tmp_path, "kfac_draw_job", ("rows", "Z", "ldZ")) +
           c_layout(tmp_path, "kfac_draw_outer_job", ("rows", "Z", "ldZ")))
    assert got == [ctypes.sizeof(N.DrawJob), N.DrawJob.rows.offset, N.DrawJob.Z.offset, N.DrawJob.ldZ.offset,
                   ctypes.sizeof(N.DrawOuterJob), N.DrawOuterJob.rows.offset, N.DrawOuterJob.Z.offset,
                   N.DrawOuterJob.ldZ.offset]
    assert N.DrawJob.Z.offset == ctypes.sizeof(N.CovJob)
    assert N.DrawOuterJob.Z.offset == ctypes.sizeof(N.CovOuterJob)


def _routes(N):
    lib = N.lib()
    return [(lib.kfac_glm_draws, lib.kfac_glm_draws_workspace_bytes, N.DrawJob, _dense_job,
             (("J", None), ("K1", None), ("K2", None), ("ldJ", 14), ("ld1", 4), ("ld2", 2), ("nA", 0),
              ("nG", -1)), 15),
            (lib.kfac_glm_draws_outer, lib.kfac_glm_draws_outer_workspace_bytes, N.DrawOuterJob, _outer_job,
             (("a", None), ("D", None), ("K1", None), ("K2", None), ("lda", 3), ("ldD", 2), ("ld1", 4),
              ("ld2", 2), ("cols", 0), ("nG", -2)), 15)]


@pytest.mark.parametrize("route", [0, 1], ids=["dense", "factored"])
def test_draw_calls_validate_before_any_launch(route):
    from bnn_kfac_amd import _native as N
    call, query, struct, make, bad_fields, K = _routes(N)[route]
    arr = N.as_array(struct, [make(N)])
    nb, nc, ns = 2, 3, 4
    R = nb * nc
    for njobs in (0, 9, -1):
        assert call(arr, njobs, nb, nc, ns, 0, OUT, R, None, 0, None) == N.KFAC_EINVAL
        assert query(arr, njobs, nb, nc, ns) == 0
    for bad in ((0, 3, 4), (-4, 3, 4), (2, 0, 4), (2, -1, 4), (2, 3, 0), (2, 3, -5)):
        assert call(arr, 1, *bad, 0, OUT, R, None, 0, None) == N.KFAC_EINVAL
        assert query(arr, 1, *bad) == 0
    assert call(None, 1, nb, nc, ns, 0, OUT, R, None, 0, None) == N.KFAC_EINVAL
    assert call(arr, 1, nb, nc, ns, 0, None, R, None, 0, None) == N.KFAC_EINVAL   # F
    assert call(arr, 1, nb, nc, ns, 0, OUT, R - 1, None, 0, None) == N.KFAC_EINVAL  # ldF < R
    for field, value in bad_fields:
        bad = make(N)
        setattr(bad.rows, field, value)
        assert call(N.as_array(struct, [bad]), 1, nb, nc, ns, 0, OUT, R, None, 0, None) == N.KFAC_EINVAL, field
    for field, value in (("Z", None), ("ldZ", K - 1)):
        bad = make(N)
        setattr(bad, field, value)
        assert call(N.as_array(struct, [bad]), 1, nb, nc, ns, 0, OUT, R, None, 0, None) == N.KFAC_EINVAL, field
    # the second job of two is validated too
    bad = make(N)
    bad.ldZ = K - 1
    assert call(N.as_array(struct, [make(N), bad]), 2, nb, nc, ns, 0, OUT, R, None, 0, None) == N.KFAC_EINVAL
    # R, ns or a task count beyond 31 bits
    for big in ((1 << 30, 32, 1), ((1 << 31) // 10, 10, 1), (2, 3, 1 << 31), (1 << 20, 1 << 10, 1 << 20)):
        assert call(arr, 1, *big, 0, OUT, big[0] * big[1], None, 0, None) == N.KFAC_EINVAL
    # a valid call without a workspace, and with one a byte short
    assert call(arr, 1, nb, nc, ns, 0, OUT, R, None, 0, None) == N.KFAC_EWORKSPACE
    assert call(arr, 1, nb, nc, ns, 1, OUT, R + 5, None, 0, None) == N.KFAC_EWORKSPACE
    need = query(arr, 1, nb, nc, ns)
    assert need > 0
    assert call(arr, 1, nb, nc, ns, 0, OUT, R, WS, need - 1, None) == N.KFAC_EWORKSPACE
    # no cap on nc or ns: accepted as far as the workspace check
    for wide_nc, many in ((33, 4), (1000, 1), (3, 1000)):
        assert query(arr, 1, 2, wide_nc, many) > 0
        assert call(arr, 1, 2, wide_nc, many, 0, OUT, 2 * wide_nc, None, 0, None) == N.KFAC_EWORKSPACE


def test_outer_draws_without_ones_column():
    from bnn_kfac_amd import _native as N
    lib = N.lib()
    plain = _outer_job(N, has_ones=0)
    assert plain.rows.ld1 == 4 and plain.ldZ == 12
    assert lib.kfac_glm_draws_outer(N.as_array(N.DrawOuterJob, [plain]), 1, 2, 3, 1, 0, OUT, 6, None, 0,
                                    None) == N.KFAC_EWORKSPACE
    short = _outer_job(N)
    short.ldZ = 12  # nA = 5 with the ones column: a draw is 15 elements
    assert lib.kfac_glm_draws_outer(N.as_array(N.DrawOuterJob, [short]), 1, 2, 3, 1, 0, OUT, 6, None, 0,
                                    None) == N.KFAC_EINVAL


def test_softmax_mc_validates_before_any_launch():
    from bnn_kfac_amd import _native as N
    call = N.lib().kfac_softmax_mc
    ns, nb, nc = 3, 2, 5
    good = dict(mean=OUT, ldm=nc, F=OUT, ldF=nb * nc, ns=ns, nb=nb, nc=nc, acc=0, psum=OUT, hsum=OUT)

    def run(**change):
        a = dict(good, **change)
        return call(a["mean"], a["ldm"], a["F"], a["ldF"], a["ns"], a["nb"], a["nc"], a["acc"], a["psum"],
                    a["hsum"], None)

    for change in (dict(mean=None), dict(F=None), dict(psum=None), dict(hsum=None), dict(ldm=nc - 1),
                   dict(ldF=nb * nc - 1), dict(ns=0), dict(ns=-1), dict(nb=0), dict(nb=-2), dict(nc=0),
                   dict(nc=-1), dict(nb=1 << 30, nc=4, ldF=1 << 32), dict(ns=1 << 31)):
        assert run(**change) == N.KFAC_EINVAL, change


def test_draw_workspace_queries_are_monotone():
    from bnn_kfac_amd import _native as N
    lib = N.lib()
    for query, arr in ((lib.kfac_glm_draws_workspace_bytes, N.as_array(N.DrawJob, [_dense_job(N, 65, 33)])),
                       (lib.kfac_glm_draws_outer_workspace_bytes,
                        N.as_array(N.DrawOuterJob, [_outer_job(N, 784, 1, 128)]))):
        by_nb = [query(arr, 1, nb, 10, 4) for nb in (1, 2, 8, 64, 65, 200)]
        assert by_nb == sorted(by_nb) and len(set(by_nb)) == len(by_nb) and by_nb[0] > 0
        by_ns = [query(arr, 1, 8, 10, ns) for ns in (1, 2, 64, 65, 129, 1000)]
        assert by_ns == sorted(by_ns) and by_ns[0] > 0 and by_ns[-1] > by_ns[0]
    # two jobs need the sum of their scratch
    both = N.as_array(N.DrawJob, [_dense_job(N, 785, 128), _dense_job(N, 65, 33)])
    one, two = (N.as_array(N.DrawJob, [_dense_job(N, *s)]) for s in ((785, 128), (65, 33)))
    q = lib.kfac_glm_draws_workspace_bytes
    assert q(both, 2, 8, 10, 4) == q(one, 1, 8, 10, 4) + q(two, 1, 8, 10, 4)
    # the factored route holds no Jacobian-row-sized scratch: C5's layer at nb = 64, 8 draws
    wide = N.as_array(N.DrawOuterJob, [_outer_job(N, 4096, 1, 4096)])
    assert lib.kfac_glm_draws_outer_workspace_bytes(wide, 1, 64, 10, 8) < 1 << 27


def test_native_wrappers_exist_and_refuse_bad_outputs():
    from bnn_kfac_amd import _native as N
    for name in ("glm_draws", "glm_draws_workspace_bytes", "glm_draws_outer", "glm_draws_outer_workspace_bytes",
                 "softmax_mc"):
        assert callable(getattr(N, name))
    assert N.glm_draws_workspace_bytes([_dense_job(N)], 2, 3, 4) == N.lib().kfac_glm_draws_workspace_bytes(
        N.as_array(N.DrawJob, [_dense_job(N)]), 1, 2, 3, 4)
    for call, job in ((N.glm_draws, _dense_job(N)), (N.glm_draws_outer, _outer_job(N))):
        for out in (torch.zeros(4, 5), torch.zeros(3, 6), torch.zeros(6, 4).T, torch.zeros(4, 12)[:, ::2],
                    torch.zeros(24)):
            with pytest.raises(ValueError, match="unit column stride"):
                call([job], 2, 3, 4, out)
        with pytest.raises(N.NativeError):  # a well-shaped output that is not on the device
            call([job], 2, 3, 4, torch.zeros(4, 9)[:, :6])


# ------------------------------------------------------------------ the formulas
@pytest.mark.parametrize("shape", [(4, 1, 3, 7, 10, 3), (6, 0, 5, 3, 4, 2), (9, 1, 2, 1, 5, 4)])
def test_factored_formula_equals_row_formula_on_rank_one_rows(shape):
    cols, ones, nG, nb, nc, ns = shape
    rng = np.random.default_rng(3)
    nA = cols + ones
    a, D = rng.standard_normal((nb, cols)), rng.standard_normal((nb, nc, nG))
    K1, K2 = np.tril(rng.standard_normal((nA, nA))), np.tril(rng.standard_normal((nG, nG)))
    Z = rng.standard_normal((ns, nA, nG))
    rows = C.rows_ref(C.outer_rows(a, ones, D), nA, nG, K1, K2, Z)
    factored = C.outer_ref(a, ones, D, K1, K2, Z)
    assert rows.shape == factored.shape == (ns, nb, nc)
    np.testing.assert_allclose(factored, rows, rtol=1e-12, atol=1e-12 * np.abs(rows).max())
    # and the projected form < K1^T M_r K2 , Z_s >_F, one entry at a time
    M = C.outer_rows(a, ones, D).reshape(nb, nc, nA, nG)
    for s, b, c in ((0, 0, 0), (ns - 1, nb - 1, nc - 1), (ns // 2, 0, nc // 2)):
        want = ((K1.T @ M[b, c] @ K2) * Z[s]).sum()
        np.testing.assert_allclose(rows[s, b, c], want, rtol=1e-12, atol=1e-12 * np.abs(rows).max())


def test_softmax_reference_properties():
    mean, F, probs, expected, entropy, mi = C.softmax_case(7, 5, 10)
    np.testing.assert_allclose(probs.sum(axis=1), 1.0, rtol=1e-14)
    assert (mi >= 0).all() and (entropy <= np.log(10) + 1e-12).all()
    # one draw: the mean probabilities are that draw's, so no mutual information
    _, _, p1, e1, h1, m1 = C.softmax_case(1, 1, 1)
    assert p1.shape == (1, 1) and p1[0, 0] == 1.0 and e1[0] == 0.0 and h1[0] == 0.0 and m1[0] == 0.0
    # +-80: finite everywhere
    for t in C.softmax_case(5, 4, 10, scale=80.0)[2:]:
        assert np.isfinite(t).all()


@pytest.mark.parametrize("name", list(C.INT_CASES))
def test_integer_cases_stay_below_2_to_24(name):
    c = C.int_case(name)
    per_job = sum(9 * j.nA * j.nG for j in c.jobs) + (3 if c.accumulate else 0)
    assert per_job < C.LIMIT
    for j in c.jobs:
        assert np.abs(j.K1).sum(axis=0).max() <= 3 and np.abs(j.K2).sum(axis=0).max() <= 3
        assert np.abs(j.a).sum(axis=1).max() <= 8 and np.abs(j.D).sum(axis=2).max() <= 8
        assert set(np.unique(j.Z)) <= {-1, 0, 1}
        if j.lower:
            assert not np.triu(j.K1, 1).any() and not np.triu(j.K2, 1).any()
        elif j.nA > 3:
            assert np.triu(j.K1, 1).any()
    refs = {}
    for route in ("outer", "rows"):
        bound = C.int_bound(c, route)
        print(name, route, "bound", bound, "of", per_job)
        assert 0 < bound <= per_job and bound < C.LIMIT
        refs[route] = C.int_reference(c, route)
        assert refs[route].dtype == np.int64 and refs[route].shape == (c.ns, c.nb, c.nc)
        assert np.abs(refs[route]).max() <= bound
    np.testing.assert_array_equal(refs["outer"], refs["rows"])
    if c.nb * c.nc * c.ns > 1:
        assert np.unique(refs["outer"]).size > 1
