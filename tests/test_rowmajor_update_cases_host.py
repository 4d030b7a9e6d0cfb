"""CPU: the row-major update cases of tests/rowmajor_update_cases.py (no GPU calls).

What test_gpu_rowmajor_update_exact.py relies on is proved here from the data, the router and
the planner (host-only calls of the library): every sum is an exact fp32 number, no reference is
trivial, the asserted routes and launch counts follow from kfac_factor_route and the model of
update_group, the ragged task kinds exist where claimed, the walk of the plan reproduces the
reference, and every planted mistake changes the result on every case its predicate names -- so
a library making that mistake fails the GPU test on those cases."""
import numpy as np
import pytest

import rowmajor_update_cases as C

CASES = C.all_cases()
IDS = [c.id for c in CASES]


def _N():
    from bnn_kfac_amd import _native as N
    return N


def test_constants_match_the_library():
    N = _N()
    assert {k: v for k, v in C.FAMILY.items()} == {
        N.PROF_FACTOR_TILES: "tiles", N.PROF_FACTOR_SYRK3: "syrk3", N.PROF_FACTOR_X3: "tiles_x3",
        N.PROF_FACTOR_CHANNEL_SMALL: "channel_small", N.PROF_FACTOR_CHANNEL_X3: "channel_x3",
        N.PROF_FACTOR_CONV: "conv"}
    assert C.REDUCE == N.PROF_FACTOR_REDUCE
    import os
    import re
    src = open(os.path.join(os.path.dirname(N.__file__), "csrc", "factor_common.h")).read()
    assert int(re.search(r"constexpr int MAXJ = (\d+);", src).group(1)) == C.MAXJ
    assert int(re.search(r"constexpr int KSEG = (\d+);", src).group(1)) == C.KSEG


def test_the_blocks_are_all_there():
    blocks = {}
    for c in CASES:
        blocks[c.block] = blocks.get(c.block, 0) + 1
    assert blocks == {"staged": 15, "glds": 20, "mixed": 6, "x3ragged": 5, "split": 6, "rounds": 9,
                      "many": 4, "syrk3": 13}, blocks
    for c in CASES:
        for j in c.jobs:
            assert j.rows <= 2048
            if j.n >= 2000:
                assert sum(j.batches) <= 96


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_bound_reference_and_walk(c):
    """0 < bound < 2^24; no reference is diagonal, two jobs of a call differ; the walk of the
    plan gives the reference."""
    assert 0 < C.bound(c) < 2 ** 24
    ref = C.reference(c)
    mats = list(ref.values())
    for R in mats:
        assert np.isfinite(R).all() and np.array_equal(R, R.T)
        if len(R) > 1:
            assert np.count_nonzero(R - np.diag(np.diag(R))) > 0
    for a in range(len(mats)):
        for b in range(a):
            m = min(len(mats[a]), len(mats[b]))
            assert not np.array_equal(mats[a][:m, :m], mats[b][:m, :m])
    got = C.walk(c)
    for i, R in ref.items():
        assert np.array_equal(got[i], R), (c.id, i)
    # the expectation is fp32-representable as computed
    want = C.expected(c)
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want, equal_nan=True)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_routes_and_launch_counts(c):
    N = _N()
    launches = C.plan(c)
    fams = []
    for L in launches:
        if L.family not in fams:
            fams.append(L.family)
    assert tuple(fams) == tuple(c.want["families"]), (fams, c.want)
    if "launches" in c.want:
        assert len(launches) == c.want["launches"]
    for L in launches:  # a launch stays within the kernel arguments
        assert len(L.subs) <= C.MAXJ and sum(C._nseg(sj) for sj in L.subs) <= C.KSEG
        assert L.family == "tiles_x3" or not any(sj.last for sj in L.subs)
    if "min_splits" in c.want:
        assert N.factor_accum_plan(launches[0].jobs)[0][0] >= c.want["min_splits"]
    counts = C.launch_counts(c)
    assert sum(v for k, v in counts.items() if k != C.REDUCE) == len(launches)
    # the first route of the call, as kfac_factor_route reports it per job of the caller's array
    jobs, keep = C.make_jobs(N, c, C.BASE, C.BASE << 2)
    first = {}
    for L in launches:
        for sj in L.subs:
            first.setdefault(sj.i, L.family)
    assert [C.FAMILY[f] for f in N.factor_route(jobs)] == [first[i] for i in range(len(c.jobs))]


def test_specific_routes():
    """What the issue's cases claim about their routes, from the plan."""
    # a 257-order factor on the fp32 kernel: one job of n > 32 without 16-byte rows beside it
    c = C.get("mixed[257 beside 70 columns]")
    assert [L.family for L in C.plan(c)] == ["tiles"] and c.jobs[0].n == 257
    # later rounds hold the narrow job alone and route to another family
    c = C.get("rounds[70/3/1,beta0]")
    assert [(L.family, [sj.i for sj in L.subs], [len(sj.batches) for sj in L.subs]) for L in C.plan(c)] == \
        [("tiles_x3", [0, 1, 2], [32, 3, 1]), ("tiles", [0], [32]), ("tiles", [0], [6])]
    # one job of 65 batches: rounds of 64 and 1, the second a single-batch job
    c = C.get("rounds[65 batches,beta0]")
    assert [[len(sj.batches) for sj in L.subs] for L in C.plan(c)] == [[64], [1]]
    assert [[len(sj.batches) for sj in L.subs] for L in C.plan(C.get("rounds[4 jobs x 17,beta1]"))] == [[16] * 4, [1] * 4]
    # a ragged group past KSEG bases: the tail split off, then rounds
    c = C.get("split[x3, 65 batches]")
    assert [[len(sj.batches) for sj in L.subs] for L in C.plan(c)] == [[16] * 4] * 4 + [[1] * 4]
    assert [float(sj.alpha / c.jobs[sj.i].alpha) for sj in C.plan(c)[-1].subs] == [4.0] * 4
    # nseg = 2: the head collapses to a single-batch job
    c = C.get("split[fp32 nseg 2]")
    assert [[len(sj.batches) for sj in L.subs] for L in C.plan(c)] == [[1, 1], [1, 1]]
    # ragged on kfac_factor_syrk3: two launches
    c = C.get("syrk3[2049,32+32+8]")
    assert [(L.family, [sj.rows for sj in L.subs]) for L in C.plan(c)] == [("syrk3", [32]), ("syrk3", [8])]
    # more than MAXJ jobs: the groups route differently, conv jobs alone and last
    c = C.get("many[33]")
    assert [(L.family, len(L.subs)) for L in C.plan(c)] == \
        [("tiles_x3", 16), ("tiles", 16), ("tiles", 1), ("channel_small", 1), ("channel_small", 1)]
    assert [c.jobs[i].layout for i in (0, 9)] == ["channel", "channel"]
    assert C.launch_counts(C.get("many[33]/deferred"))[C.REDUCE] == 3
    assert C.launch_counts(C.get("many[17]/deferred"))[C.REDUCE] == 2


def test_ragged_task_kinds():
    """The four kinds of K-split around the ragged batch exist where claimed: sps = 2, so the
    ragged batch is stage 4 of 5, and chunk = ceil(5 / splits)."""
    c = C.get("x3ragged[deferred]")
    L, = C.plan(c)
    assert L.family == "tiles_x3"
    kinds = {sj.i: C.task_kinds(c, sj, c.jobs[sj.i].splits) for sj in L.subs}
    assert kinds[0] == {"crossing"}                    # splits 2: [0, 3) [3, 5)
    assert kinds[1] == {"ends", "starts"}              # splits 3: [0, 2) [2, 4) [4, 5)
    assert kinds[2] == {"ends", "starts", "empty"}     # splits 4: ... [5, 5)
    assert kinds[3] == {"ends", "starts"}              # splits 5: one stage each
    assert set().union(*kinds.values()) == set(c.want["kinds"])
    assert C.task_ranges(5, 4) == [(0, 2), (2, 4), (4, 5), (5, 5)]


def test_workspace_is_the_maximum_over_the_groups():
    N = _N()
    for c in CASES:
        if c.block in ("many", "mixed"):
            jobs, keep = C.make_jobs(N, c, C.BASE, C.BASE << 2)
            got = N.lib().kfac_factor_workspace_bytes(N.as_array(N.FactorJob, jobs), len(jobs))
            assert got == C.workspace_bytes(c), c.id
            assert (got == 0) == c.deferred


@pytest.mark.parametrize("mistake", list(C.MISTAKES))
def test_planted_mistakes_show(mistake):
    named = [c for c in CASES if C.MISTAKES[mistake](c)]
    assert named, mistake
    for c in named:
        got, ref = C.reference(c, mistake), C.reference(c)
        assert any(not np.array_equal(got[i], ref[i], equal_nan=True) for i in ref), (mistake, c.id)
