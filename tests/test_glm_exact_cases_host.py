"""CPU: the integer cases of glm_exact_cases.py are exact (every partial sum below 2^24), not
degenerate (a reference that is not diagonal and differs between samples and between grid
points), laid out in disjoint regions, and able to see the mistakes a kernel could make: for
each name in MISTAKES the mistaken int64 result differs from the true one on every case listed
for it here.  The workspace check of the four calls returns before any launch (dummy integers
stand in for device pointers: nothing is dereferenced on the host)."""
import numpy as np
import pytest

import glm_exact_cases as E

# mistake -> the cases that must see it (a case that cannot is a failure, not a skip)
SEES = {
    "K1_transposed": ["dense-27x6x4x3-lower", "dense-27x6x4x3-dense", "dense-65x33x2x31-lower",
                      "outer-63x1x10x3x10-lower", "outer-64x1x5x2x3-dense", "sweep-27x6x3x10x64",
                      "outer_sweep-130x1x10x70x2x5"],
    "K2_transposed": ["dense-27x6x4x3-lower", "dense-27x6x4x3-dense", "dense-65x33x2x31-lower",
                      "outer-63x1x10x3x10-lower", "outer-64x1x5x2x3-dense", "sweep-27x6x3x10x64",
                      "outer_sweep-130x1x10x70x2x5"],
    "flatten_ga": ["dense-5x3x2x1-lower", "dense-27x6x4x3-dense", "dense-65x33x2x31-lower", "dense-65x33x2x31-dense",
                   "sweep-3x86x1x32x4", "sweep-65x33x2x31x17"],
    "drop_last": ["dense-64x32x1x32-ldJ=K-lower", "dense-64x32x1x32-ldJ=K-dense", "dense-683x3x2x2-lower",
                  "dense-683x3x2x2-dense", "dense-65x33x2x31-lower", "dense-65x33x2x31-dense",
                  "outer-20x1x2048x2x32-lower", "outer-20x1x2048x2x32-dense", "outer-20x1x2049x2x3-lower",
                  "outer-20x1x2049x2x3-dense", "sweep-16x16x2x3x1", "sweep-257x1x2x2x5", "sweep-3x86x1x32x4",
                  "outer_sweep-63x1x256x2x3x16", "outer_sweep-64x1x257x3x2x17"],
    # GSEG for the plain calls, WSEG for the sweeps
    "drop_segment2_first": ["dense-683x3x2x2-lower", "dense-683x3x2x2-dense", "dense-65x33x2x31-lower",
                            "dense-65x33x2x31-dense", "outer-20x1x2049x2x3-lower", "outer-20x1x2049x2x3-dense",
                            "sweep-257x1x2x2x5", "sweep-3x86x1x32x4", "sweep-65x33x2x31x17",
                            "outer_sweep-64x1x257x3x2x17"],
    "ones_omitted": ["outer-63x1x10x3x10-lower", "outer-63x1x10x3x10-dense", "outer-64x1x5x2x3-lower",
                     "outer-64x1x5x2x3-dense", "outer_sweep-63x1x256x2x3x16", "outer_sweep-64x1x257x3x2x17"],
    "ones_from_a": ["outer-63x1x10x3x10-lower", "outer-63x1x10x3x10-dense", "outer-64x1x5x2x3-lower",
                    "outer-64x1x5x2x3-dense", "outer_sweep-63x1x256x2x3x16", "outer_sweep-64x1x257x3x2x17"],
    "sample_offset_32": ["dense-27x6x4x3-lower", "dense-65x33x2x31-lower", "outer-63x1x10x3x10-lower",
                         "outer-12x1x6x65x2-lower", "sweep-27x6x3x10x64", "outer_sweep-130x1x10x70x2x5"],
    "mirror_upper": ["dense-64x32x1x32-ldJ=K-lower", "dense-64x32x1x32-ldJ=K-dense", "outer-20x1x2048x2x32-lower",
                     "sweep-3x86x1x32x4", "outer_sweep-63x1x256x2x3x16"],
    "accumulate_ignored": ["dense-jobs8-acc", "outer-jobs8-acc", "sweep-jobs8-acc", "outer_sweep-jobs8-acc"],
    "rank1_swapped": ["sweep-16x16x2x3x1", "sweep-3x86x1x32x4", "sweep-27x6x3x10x64", "sweep-65x33x2x31x17"],
    "tau_next": ["sweep-257x1x2x2x5", "sweep-27x6x3x10x64", "outer_sweep-63x1x256x2x3x16",
                 "outer_sweep-64x1x257x3x2x17"],
    "rownorm_next_tile": ["outer_sweep-64x1x257x3x2x17", "outer_sweep-130x1x10x70x2x5"],
    "scale_next_sample": ["outer-63x1x10x3x10-lower", "outer-12x1x6x65x2-lower", "outer-130x1x130x70x2-lower",
                          "outer_sweep-64x1x257x3x2x17", "outer_sweep-130x1x10x70x2x5"],
}


def test_ids_and_tables():
    assert len(set(E.IDS)) == len(E.IDS) == 2 * (len(E.DENSE) + len(E.OUTER)) + len(E.SWEEP) + len(E.OUTER_SWEEP) + 8
    assert sorted(sum(E.ROUTE_IDS.values(), [])) == sorted(E.IDS)
    for route in E.ROUTES:
        assert len(E.JOBS8_IDS[route]) == 2 and all(len(E.SPECS[cid].jobs) == 8 for cid in E.JOBS8_IDS[route])
        assert [E.SPECS[cid].accumulate for cid in E.JOBS8_IDS[route]] == [False, True]
    assert set(SEES) == set(E.MISTAKES) and all(set(v) <= set(E.IDS) and v for v in SEES.values())
    # the shapes the cases are there for
    K = lambda cid: E.SPECS[cid].jobs[0].nA * E.SPECS[cid].jobs[0].nG  # noqa: E731
    assert K("dense-64x32x1x32-ldJ=K-lower") == E.GSEG == E.SPECS["dense-64x32x1x32-ldJ=K-lower"].jobs[0].ldJ
    assert K("dense-683x3x2x2-lower") == E.GSEG + 1 and K("dense-65x33x2x31-lower") == 2145
    assert (K("sweep-16x16x2x3x1"), K("sweep-257x1x2x2x5"), K("sweep-3x86x1x32x4")) == (E.WSEG, E.WSEG + 1, E.WSEG + 2)
    assert E.SPECS["sweep-257x1x2x2x5"].nt == E.WTG + 1 and E.SPECS["outer_sweep-63x1x256x2x3x16"].nt == E.RNTG
    assert E.SPECS["outer-63x1x10x3x10-lower"].jobs[0].nA == E.TILE
    assert E.SPECS["outer-64x1x5x2x3-lower"].jobs[0].nA == E.TILE + 1
    # the two pitch / alignment paths of Panel<KFAC_ROWBATCH>: ldJ % 4 and the base
    for tag, ldJ4, skew in (("ldJ=K+4", 0, ()), ("ldJ=K+6", 2, ()), ("ldJ=K+4,Jskew", 0, ("J",))):
        j = E.SPECS[f"dense-20x8x3x5-{tag}-lower"].jobs[0]
        assert j.nG % 4 == 0 and j.ldJ % 4 == ldJ4 and j.ldJ > j.nA * j.nG and j.skew == skew
    j = E.SPECS["dense-20x8x3x5-ld=n+4,Kskew-lower"].jobs[0]
    assert (j.ld1, j.ld2, j.skew) == (j.nA + 4, j.nG + 4, ("K1", "K2"))


@pytest.mark.parametrize("cid", E.IDS)
def test_case_is_exact_and_not_degenerate(cid):
    c = E.case(cid)
    ref, b = E.reference(c), E.bound(c)
    print(f"{cid}: bound {b}, max|ref| {int(np.abs(ref).max())}")
    assert 0 < b < E.LIMIT
    assert ref.dtype == np.int64 and ref.shape == c.cov_shape and 0 < np.abs(ref).max() <= b
    assert np.array_equal(ref, np.swapaxes(ref, -1, -2))
    blocks = ref.reshape(-1, c.nb, c.nc, c.nc)
    if c.nc > 1:  # not diagonal, at every grid point
        assert all(np.abs(t - t * np.eye(c.nc, dtype=np.int64)).max() > 0 for t in blocks)
    if c.nb > 1:  # differs between two samples
        assert all(not np.array_equal(t[0], t[1]) for t in blocks)
    for s in range(c.nt):  # differs between any two grid points
        for t in range(s):
            assert not np.array_equal(blocks[s], blocks[t]), (s, t)


@pytest.mark.parametrize("cid", E.IDS)
def test_data_is_what_the_bound_assumes(cid):
    c = E.case(cid)
    for j, d in zip(c.jobs, c.data):
        for K in (d.K1, d.K2):
            assert set(np.unique(K)) <= {-1, 0, 1} and (np.abs(K).sum(axis=0) <= 3).all() and K[-1].any()
            if j.lower:
                assert not np.triu(K, 1).any()
            elif K.shape[0] > 1:
                assert np.triu(K, 1).any()
        if c.outer:
            for rows in (d.a, d.D.reshape(-1, j.nG)):
                n = np.abs(rows).sum(axis=1)
                assert set(np.unique(rows)) <= {-1, 0, 1} and (n >= 1).all() and (n <= 8).all()
        else:
            assert set(np.unique(d.J)) <= {-1, 0, 1} and d.J.shape == (c.nb, c.nc, j.nA * j.nG)
            assert j.nA * j.nG < 9 or len(np.unique(d.J)) == 3
        if c.sweep:
            for w in (d.wA, d.wG):
                assert w.min() >= 0 and w.max() <= 3
                assert w.shape[1] == 1 or ((w == 0).any(axis=1).all() and (w == 3).any(axis=1).all())
    if c.sweep:  # every grid point's weights are its own
        every = np.concatenate([w for d in c.data for w in (d.wA, d.wG)], axis=1)
        assert len({r.tobytes() for r in every}) == c.nt


@pytest.mark.parametrize("cid", E.IDS)
def test_layout_regions_are_disjoint(cid):
    c = E.case(cid)
    end = 0
    for r in c.regions:
        assert r.off >= end + E.GAP and r.ld >= r.cols and r.end == r.off + r.rows * r.ld
        skewed = r.job >= 0 and r.op in c.jobs[r.job].skew
        assert r.off % 4 == (1 if skewed else 0)  # 16-byte aligned in the buffer, or one float past
        end = r.end
    assert c.size == end + E.GAP and c.flat.shape == (c.size,) and c.flat.dtype == np.float32
    assert c.regions[-1] is c.cov and c.cov.cols == int(np.prod(c.cov_shape))
    # every element that is not an operand's (or an accumulate prefill's) is NaN, the rest is not
    data = sum(r.rows * r.cols for r in c.regions[:-1]) + (c.cov.cols if c.accumulate else 0)
    assert int((~np.isnan(c.flat)).sum()) == data
    want = E.want(c)
    assert int(np.isnan(want).sum()) == c.size - data - (0 if c.accumulate else c.cov.cols)
    assert np.array_equal(want[c.cov.off:c.cov.end], E.reference(c).reshape(-1).astype(np.float32))
    assert E.region_of(c, c.cov.off).startswith("cov") and E.region_of(c, 0) == "a gap between regions"
    # default pitches, unless the case names another
    j = c.jobs[-1]
    if len(c.jobs) > 1:
        assert (j.ldJ, j.ld1, j.ld2, j.lda, j.ldD, j.ldwA, j.ldwG) == \
            (j.nA * j.nG + 7, j.nA + 3, j.nG + 1, j.cols + 3, j.nG + 5, j.nA + 3, j.nG + 2)


@pytest.mark.parametrize("mistake", list(E.MISTAKES))
def test_cases_see_the_mistake(mistake):
    for cid in SEES[mistake]:
        c = E.case(cid)
        wrong = E.reference(c, mistake)
        assert wrong.shape == c.cov_shape
        n = int((wrong != E.reference(c)).sum())
        print(f"{mistake} on {cid}: {n} of {wrong.size} elements differ")
        assert n > 0, (mistake, cid)


def test_reference_is_the_sweep_helpers_formula():
    """The int64 chain against glm_sweep_cases.dense_ref / outer_ref in fp64 (exact on this data)."""
    import glm_sweep_cases as S
    for cid in ("sweep-27x6x3x10x64", "sweep-3x86x1x32x4"):
        c = E.case(cid)
        j, d = c.jobs[0], c.data[0]
        got = S.dense_ref(d.J, j.nA, j.nG, d.K1, d.K2, d.wA, d.wG)
        np.testing.assert_array_equal(got, E.reference(c).astype(np.float64))
    for cid in ("outer_sweep-63x1x256x2x3x16", "outer_sweep-130x1x10x70x2x5"):
        c = E.case(cid)
        j, d = c.jobs[0], c.data[0]
        got = S.outer_ref(d.a, j.ones, d.D, d.K1, d.K2, d.wA, d.wG)
        np.testing.assert_array_equal(got, E.reference(c).astype(np.float64))


@pytest.mark.parametrize("route", E.ROUTES)
def test_short_workspace_returns_before_any_launch(route):
    from bnn_kfac_amd import _native as N
    for cid in (E.SINGLE_IDS[route][1], E.JOBS8_IDS[route][0]):
        c = E.case(cid)
        base, ws = 1 << 30, 1 << 40  # never dereferenced
        jobs = E.native_jobs(N, c, base)
        need = E.workspace_bytes(N, c, jobs)
        assert need > 0 and need % 256 == 0
        assert E.call(N, c, jobs, base, ws, need - 1, None) == N.KFAC_EWORKSPACE
        assert E.call(N, c, jobs, base, None, need, None) == N.KFAC_EWORKSPACE
