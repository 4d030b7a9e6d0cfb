"""The integer cases of posterior_cases.py are exact, agree with the fp64 oracle and tell
every planted mistake apart; and the argument checks of the five entry points return before
any launch (CPU only: dummy integers stand in for device pointers)."""
import numpy as np
import pytest

import posterior_cases as P
from oracle import kfac_oracle as O

EXACT = 2.0 ** 24

ARENA_FAMILIES = [(kind,) + P.FAMILIES[kind] for kind in ("sample", "efb", "gram")]
ARENA_CASES = [pytest.param(c, ref, model, id=f"{kind}-{c.id}")
               for kind, cases, ref, model, _, _ in ARENA_FAMILIES for c in cases()]
TRI_OPS = ("pack", "unpack_sym", "unpack_lower")


def _ids(cases):
    return [c.id for c in cases]


# ------------------------------------------------------------------ 1. exactness
@pytest.mark.parametrize("kind,cases,bounds", [(k, c, b) for k, c, _, _, b, _ in ARENA_FAMILIES],
                         ids=["sample", "efb", "gram"])
def test_fp32_intermediates_are_exact(kind, cases, bounds):
    """|A| |B| bounds every partial sum of A B: below 2^24 every fp32 product and sum the
    kernel forms is an exact integer, in any order."""
    for c in cases():
        b = bounds(c)
        print(f"{kind}-{c.id}: " + " ".join(f"{k} {v:.0f}" for k, v in b.items()))
        assert all(v < EXACT for v in b.values()), (c.id, b)


def test_quadform_intermediates_are_exact():
    for c in P.quad_cases():
        b = P.quad_bounds(c)
        print(f"quad-{c.id}: P {b['P']:.0f} Q {b['Q']:.0f} sum {b['sum']:.3g}")
        assert b["P"] < EXACT and b["Q"] < EXACT and b["sum"] < 2.0 ** 53, (c.id, b)


def test_tri_values_are_exact():
    for op in TRI_OPS:
        c = P.tri_case(op)
        assert c.total < EXACT and np.nanmax(np.abs(c.arena.array())) < EXACT


# ---------------------------------------------------------------- data rules
def _all_jobs(cases):
    return [j for c in cases for j in c.jobs]


def _lower_ok(L):
    return not np.triu(L, 1).any() and np.all(np.abs(np.diag(L)) == 1)


def _full_ok(F):
    n = len(F)
    return n <= P.TILE or (F[:P.TILE, P.TILE:].any() and F[P.TILE:, :P.TILE].any())


def _pitches_ok(pairs):
    """(ld, n) pairs of one kernel: every ld > n, one ld no multiple of 4, one a multiple of 4
    whose n is not."""
    return (all(ld > n for ld, n in pairs) and any(ld % 4 for ld, _ in pairs)
            and any(ld % 4 == 0 and n % 4 for ld, n in pairs))


def test_data_rules():
    sj, qj, ej, gj = (_all_jobs(f()) for f in (P.sample_cases, P.quad_cases, P.efb_cases, P.gram_cases))
    tj = P.tri_case("pack").jobs
    edges = {e for j in sj + qj + ej for e in (j.nA, j.nG)} | {j.n for j in tj} | {e for j in gj
                                                                                   for e in (j.nA, j.nG)}
    assert edges <= set(P.SHAPES) and max(edges) <= 200
    for j in sj:
        assert all((_full_ok if j.dense else _lower_ok)(L) for L in (j.LA, j.LG))
        assert np.abs(j.LA).max() <= 1 and np.abs(j.z).max() <= 2
    for j in qj:
        assert (_lower_ok if j.lower1 else _full_ok)(j.K1) and (_lower_ok if j.lower2 else _full_ok)(j.K2)
        assert np.abs(j.K1).max() <= 1 and np.abs(j.K2).max() <= 1 and np.abs(j.J).max() <= 2
    for j in ej:
        assert max(np.abs(j.VA).max(), np.abs(j.VG).max()) <= 1 and all(np.abs(g).max() <= 2 for g in j.grads)
        assert len({j.ldA, j.ldG, j.ld_grad, j.ld_state, j.ld_diag}) == 5
    for j in gj:
        assert set(np.unique(j.c)) <= {1, 2, 3} and set(np.unique(j.sigma)) <= set(P.SIGMAS)
        assert max(np.abs(j.UA).max(), np.abs(j.UG).max()) <= 1
    assert {j.la ** 2 for j in gj} | {j.lg ** 2 for j in gj} == {64, 81, 9, 144}
    assert _pitches_ok([p for j in sj for p in ((j.ldA, j.nA), (j.ldG, j.nG), (j.ldW, j.wcols))])
    assert _pitches_ok([p for j in qj for p in ((j.ld1, j.nA), (j.ld2, j.nG), (j.ldJ, j.nA * j.nG))])
    assert _pitches_ok([p for j in ej for p in ((j.ldA, j.nA), (j.ldG, j.nG), (j.ld_grad, j.nA),
                                                (j.ld_state, j.nA), (j.ld_diag, j.nA))])
    assert _pitches_ok([p for j in gj for p in ((j.ldA, j.la), (j.ldG, j.lg), (j.ldo, j.la * j.lg))])
    assert _pitches_ok([(j.ldF, j.n) for j in tj])
    for j in tj:  # different above and below the diagonal
        assert np.all(np.triu(j.F, 1)[np.triu_indices(j.n, 1)] < 0) and np.all(j.F[np.tril_indices(j.n)] > 0)


def test_case_table():
    """The shapes, groups and paths the cases are there for."""
    s = {c.id: c for c in P.sample_cases()}
    for nA, nG in P.LOWER_SHAPES:
        for kind in ("full", "bias", "nobias"):
            c = s[f"lower-{nA}x{nG}-{kind}"]
            j, = c.jobs
            assert (j.nA, j.nG, j.dense, c.accumulate) == (nA, nG, 0, 0)
            assert j.wcols == (nA if kind == "full" else nA - 1) and (j.oB is not None) == (kind == "bias")
    assert {(c.jobs[0].nA, c.jobs[0].nG) for c in s.values() if c.id.startswith("dense")} == set(P.DENSE_SHAPES)
    assert all(c.covers & {"dense1", "dense2"} for c in s.values() if c.id.startswith("dense"))
    assert s["loader-65x68-odd-offsets"].jobs[0].oZ % 2 == 1 and s["loader-65x68-aligned"].jobs[0].oZ % 4 == 0
    g8, g9 = s["group8"], s["group9-chunks"]
    tiles = [-(-j.nA // P.TILE) * -(-j.nG // P.TILE) for j in g8.jobs]
    assert len(g8.jobs) == 8 and tiles == [6, 2, 4, 1, 3, 2, 6, 1] and {j.dense for j in g8.jobs} == {0, 1}
    assert len(g9.jobs) == 9 and g9.accumulate and any(c.accumulate and c.jobs[0].b0 is not None
                                                        for c in s.values())
    q = {c.id: c for c in P.quad_cases()}
    for nA, nG in P.QUAD_SHAPES:
        for l1 in (0, 1):
            for l2 in (0, 1):
                c = q[f"flags{l1}{l2}-{nA}x{nG}"]
                j, = c.jobs
                assert (j.nA, j.nG, j.lower1, j.lower2, c.nb, j.ldJ) == (nA, nG, l1, l2, 3, nA * nG + 5)
    for cid in ("group8-abs", "group8-signed"):
        assert len(q[cid].jobs) == 8 and {j.oV is None for j in q[cid].jobs} == {True, False}
    assert (q["group8-abs"].abs_sum, q["group8-signed"].abs_sum) == (1, 0)
    assert all(len(q[cid].jobs) == 9 and q[cid].via == "wrapper" for cid in ("fold9-lower-abs",
                                                                            "fold9-full-signed"))
    assert any(c.nb == 1 for c in q.values())
    e = {c.id: c for c in P.efb_cases()}
    assert len(e["group8"].jobs) == 8 and len(e["group9-chunks"].jobs) == 9
    assert not e["65x65-nodiag"].jobs[0].has_diag
    assert [len(c.jobs) for c in P.gram_cases()] == [1, 1, 1, 3]
    t = P.tri_case("pack")
    assert len(t.jobs) == 20 > P.TRI_CHUNK and [j.n for j in t.jobs[:5]] == list(P.TRI_SIZES)
    offs = [j.offset for j in t.jobs]
    assert offs != sorted(offs) and offs[P.TRI_CHUNK:] != sorted(offs[P.TRI_CHUNK:])
    spans = sorted((j.offset, j.offset + j.n * (j.n + 1) // 2) for j in t.jobs)  # a gap-free tiling
    assert spans[0][0] == 0 and spans[-1][1] == t.total
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))


def test_group_rows_have_terms_of_both_signs():
    """abs_sum can only show where one row's terms differ in sign."""
    for c in P.quad_cases():
        if len(c.jobs) > 1:
            v, _ = P.quad_reference(c)
            for i in range(0, len(v) - 1, 8):  # every call of the fold that has several jobs
                assert np.any((v[i:i + 8] > 0).any(axis=0) & (v[i:i + 8] < 0).any(axis=0)), c.id


# ---------------------------------------------------- 2. references and the oracle
@pytest.mark.parametrize("case,ref,model", ARENA_CASES)
def test_model_is_the_reference(case, ref, model):
    want = ref(case)
    assert P.same(model(case), want), P.first_difference(case.arena, model(case), want)
    assert P.first_difference(case.arena, want, want) is None


@pytest.mark.parametrize("case", P.quad_cases(), ids=_ids(P.quad_cases()))
def test_quad_model_is_the_reference(case):
    (v, out), (v0, out0) = P.quad_model(case), P.quad_reference(case)
    assert P.same(v, v0) and P.same(out, out0)
    assert np.isfinite(v0).all() and v0.dtype == out0.dtype == np.float32


@pytest.mark.parametrize("op", TRI_OPS)
def test_tri_model_is_the_reference(op):
    c = P.tri_case(op)
    assert P.same(P.tri_model(c), P.tri_reference(c))


def _region(flat, off, rows, cols, ld):
    return flat[P.idx(off, rows, cols, ld)].astype(np.float64)


@pytest.mark.parametrize("case", [c for c in P.sample_cases() if not c.accumulate],
                         ids=_ids([c for c in P.sample_cases() if not c.accumulate]))
def test_sample_reference_vs_oracle(case):
    flat = P.sample_reference(case)
    for j in case.jobs:
        want = O.sample(j.LA, j.LG, j.z)  # (nG, nA), fp64
        np.testing.assert_array_equal(_region(flat, j.oW, j.nG, j.wcols, j.ldW), want[:, :j.wcols])
        if j.oB is not None:
            np.testing.assert_array_equal(flat[j.oB:j.oB + j.nG], want[:, -1])


def test_sample_accumulate_vs_oracle_replace():
    for case in (c for c in P.sample_cases() if c.accumulate):
        flat = P.sample_reference(case)
        for j in case.jobs:
            S = O.sample(j.LA, j.LG, j.z)
            if j.wcols == j.nA:
                W, b = O.replace(S, j.W0[:, :j.wcols])
            else:  # (a NULL bias drops the last column: a zero stands in for it)
                W, b = O.replace(S, j.W0[:, :j.wcols], j.b0 if j.b0 is not None else np.zeros(j.nG))
            np.testing.assert_array_equal(_region(flat, j.oW, j.nG, j.wcols, j.ldW), W)
            if j.b0 is not None:
                np.testing.assert_array_equal(flat[j.oB:j.oB + j.nG], b)


def test_quad_reference_vs_oracle():
    dense = 0
    for case in P.quad_cases():
        v, _ = P.quad_reference(case)
        for j, vj in zip(case.jobs, v):
            np.testing.assert_array_equal(vj, O.kron_quadform(j.J, j.K1, j.K2).astype(np.float32))
            if j.nA * j.nG <= 2200 and case.id.startswith(("group8-abs", "fold9-lower")):
                np.testing.assert_array_equal(vj, O.kron_quadform_dense(j.J, j.K1, j.K2).astype(np.float32))
                dense += 1
    assert dense >= 4


@pytest.mark.parametrize("case", P.efb_cases()[:4], ids=_ids(P.efb_cases()[:4]))
def test_efb_reference_vs_oracle(case):
    """fp64 lambdas of the two batches: the fp32 reference is within the three roundings
    (two squares, one sum) of them, and the squares alone are their exact roundings."""
    flat = P.efb_reference(case)
    for j in case.jobs:
        lam = [O.efb_lambdas(g, j.VA, j.VG) for g in j.grads]
        got = _region(flat, j.oS, j.nG, j.nA, j.ld_state)
        l32 = [x.astype(np.float32) for x in lam]
        np.testing.assert_array_equal(got, (l32[0] + l32[1]).astype(np.float64))
        assert np.all(np.abs(got - (lam[0] + lam[1])) <= 3 * 2.0 ** -24 * (lam[0] + lam[1]))
        if j.has_diag:
            want = sum(g.astype(np.float64) ** 2 * P.EFB_SCALE for g in j.grads)
            np.testing.assert_array_equal(_region(flat, j.oD, j.nG, j.nA, j.ld_diag), want)


@pytest.mark.parametrize("case", P.gram_cases()[:3], ids=_ids(P.gram_cases()[:3]))
def test_gram_reference_vs_explicit_kron(case):
    flat = P.gram_reference(case)
    for j in case.jobs:
        Vs = j.c.reshape(-1, 1).astype(np.float64) * O.kron(j.UA, j.UG) @ np.diag(j.sigma)
        got = _region(flat, j.oOut, j.la * j.lg, j.la * j.lg, j.ldo)
        np.testing.assert_array_equal(got, Vs.T @ Vs)
        np.testing.assert_array_equal(got, got.T)


# --------------------------------------------------------------- 3. discrimination
@pytest.mark.parametrize("case,ref,model", ARENA_CASES)
def test_mistakes_show(case, ref, model):
    want = ref(case)
    assert case.covers
    for m in sorted(case.covers):
        assert not P.same(model(case, m), want), f"{case.id} cannot tell `{m}` apart"


@pytest.mark.parametrize("case", P.quad_cases(), ids=_ids(P.quad_cases()))
def test_quad_mistakes_show(case):
    v0, out0 = P.quad_reference(case)
    for m in sorted(case.covers):
        v, out = P.quad_model(case, m)
        assert not (P.same(v, v0) and P.same(out, out0)), f"{case.id} cannot tell `{m}` apart"
        if m in ("abs_ignored", "abs_always"):
            assert P.same(v, v0)  # only the sum over the jobs shows it


@pytest.mark.parametrize("op", TRI_OPS)
def test_tri_mistakes_show(op):
    c = P.tri_case(op)
    want = P.tri_reference(c)
    for m in sorted(c.covers):
        assert not P.same(P.tri_model(c, m), want), f"tri {op} cannot tell `{m}` apart"


def test_every_mistake_has_a_case():
    for kind, cases, _, _, _, mistakes in ARENA_FAMILIES:
        covered = set().union(*(c.covers for c in cases()))
        assert covered == set(mistakes), (kind, covered ^ set(mistakes))
    assert set().union(*(c.covers for c in P.quad_cases())) == set(P.QUAD_MISTAKES)
    assert set().union(*(P.tri_case(op).covers for op in TRI_OPS)) == set(P.TRI_MISTAKES)
    # the two holes the suite had: `dense` on the G side, and a clear flag across a tile boundary
    assert sum("dense2" in c.covers for c in P.sample_cases()) >= 2
    for flag in ("lower1_forced", "lower2_forced"):
        assert sum(flag in c.covers for c in P.quad_cases() if len(c.jobs) == 1) >= 4


# --------------------------------------------------------------- 4. argument checks
BIG = 1 << 40  # workspace bytes no valid job here needs
WS, OUT = 1 << 20, 1 << 21  # never dereferenced: every call below returns before any launch


def _N():
    from bnn_kfac_amd import _native as N
    N.lib()
    return N


def _sample_job(N, **kw):
    j = N.SampleJob(1 << 12, 5, 1 << 13, 3, 1 << 14, 5, 3, 1 << 15, 5, 1 << 16, 5, 0)
    for k, v in kw.items():
        setattr(j, k, v)
    return j


def _quad_job(N, **kw):
    j = N.QuadJob(1 << 12, 15, 5, 3, 1 << 13, 5, 1 << 14, 3, 1, 1, 1 << 15)
    for k, v in kw.items():
        setattr(j, k, v)
    return j


def _efb_job(N, **kw):
    j = N.EfbJob(1 << 12, 5, 1 << 13, 3, 1 << 14, 5, 1 << 15, 5, 1 << 16, 5, 5, 3, 0, 32.0)
    for k, v in kw.items():
        setattr(j, k, v)
    return j


def _gram_job(N, **kw):
    j = N.GramJob(1 << 12, 2, 1 << 13, 3, 1 << 14, 1 << 15, 1 << 16, 6, 5, 4, 2, 3)
    for k, v in kw.items():
        setattr(j, k, v)
    return j


def _tri_job(N, **kw):
    j = N.TriJob(1 << 12, 5, 5, 0, 0)
    for k, v in kw.items():
        setattr(j, k, v)
    return j


SAMPLE_BAD = [("LA", None), ("LG", None), ("Z", None), ("W", None), ("nA", 0), ("nA", -1), ("nG", 0),
              ("nG", -1), ("ldA", 4), ("ldG", 2), ("wcols", -1), ("wcols", 6), ("wcols", 3), ("ldW", 4)]
QUAD_BAD = [("J", None), ("K1", None), ("K2", None), ("nA", 0), ("nA", -1), ("nG", 0), ("nG", -1),
            ("ld1", 4), ("ld2", 2), ("ldJ", 14)]
EFB_BAD = [("VA", None), ("VG", None), ("grad", None), ("state", None), ("nA", 0), ("nA", -1), ("nG", 0),
           ("nG", -1), ("ldA", 4), ("ldG", 2), ("ld_grad", 4), ("ld_state", 4), ("ld_diag", 4)]
GRAM_BAD = [("UA", None), ("UG", None), ("c", None), ("sigma", None), ("out", None), ("nA", 0), ("nA", -1),
            ("nG", 0), ("nG", -1), ("la", 0), ("la", -1), ("lg", 0), ("lg", -1), ("ldA", 1), ("ldG", 2),
            ("ldo", 5)]
TRI_BAD = [("F", None), ("n", -1), ("ldF", 4), ("offset", -1)]


def _grouped_checks(N, ctype, make, bad, call, short):
    """`call(arr, njobs, ws, ws_bytes)`.  njobs of 0 and 9, NULL jobs, every single-field
    violation alone and as the second job, then the workspace."""
    ok = N.as_array(ctype, [make(N)] * 9)
    assert call(ok, 0, WS, BIG) == N.KFAC_EINVAL
    assert call(ok, 9, WS, BIG) == N.KFAC_EINVAL
    assert call(None, 1, WS, BIG) == N.KFAC_EINVAL
    for field, value in bad:
        j = make(N, **{field: value})
        assert call(N.as_array(ctype, [j]), 1, WS, BIG) == N.KFAC_EINVAL, (field, value)
        assert call(N.as_array(ctype, [make(N), j]), 2, WS, BIG) == N.KFAC_EINVAL, (field, value, "second")
    need = short(ok)
    assert need > 0
    assert call(ok, 1, None, BIG) == N.KFAC_EWORKSPACE
    assert call(ok, 1, WS, need - 1) == N.KFAC_EWORKSPACE
    assert call(ok, 1, None, 0) == N.KFAC_EWORKSPACE


def test_sample_argument_checks():
    N = _N()
    lib = N.lib()
    _grouped_checks(N, N.SampleJob, _sample_job, SAMPLE_BAD,
                    lambda arr, n, ws, b: lib.kfac_sample(arr, n, 0, ws, b, None),
                    lambda arr: lib.kfac_sample_workspace_bytes(arr, 1))


def test_quadform_argument_checks():
    N = _N()
    lib = N.lib()
    call = lambda arr, n, ws, b, nb=2, out=OUT: lib.kfac_kron_quadform(arr, n, nb, 1, out, ws, b, None)
    _grouped_checks(N, N.QuadJob, _quad_job, QUAD_BAD, call,
                    lambda arr: lib.kfac_quadform_workspace_bytes(arr, 1, 2))
    ok = N.as_array(N.QuadJob, [_quad_job(N)])
    assert call(ok, 1, WS, BIG, nb=0) == N.KFAC_EINVAL
    assert call(ok, 1, WS, BIG, out=None) == N.KFAC_EINVAL
    assert call(ok, 1, WS, BIG, nb=1 << 31) == N.KFAC_EINVAL  # 2^31 tasks
    # the NULL workspace with a byte count that would do: refused since this suite
    assert call(ok, 1, None, BIG) == N.KFAC_EWORKSPACE
    assert call(ok, 1, None, lib.kfac_quadform_workspace_bytes(ok, 1, 2)) == N.KFAC_EWORKSPACE


def test_efb_argument_checks():
    N = _N()
    lib = N.lib()
    call = lambda arr, n, ws, b: lib.kfac_efb_update(arr, n, ws, b, None)
    _grouped_checks(N, N.EfbJob, _efb_job, EFB_BAD, call, lambda arr: lib.kfac_efb_workspace_bytes(arr, 1))
    # ld_diag is only looked at with a diag: that job is valid, so it stops at the workspace
    free = N.as_array(N.EfbJob, [_efb_job(N, diag=None, ld_diag=0)])
    assert call(free, 1, None, BIG) == N.KFAC_EWORKSPACE


def test_gram_argument_checks():
    N = _N()
    lib = N.lib()
    call = lambda arr, n, ws, b: lib.kfac_kron_gram(arr, n, ws, b, None)
    _grouped_checks(N, N.GramJob, _gram_job, GRAM_BAD, call, lambda arr: lib.kfac_gram_workspace_bytes(arr, 1))
    for field in ("la", "lg"):  # la^2 / lg^2 index an int: refused from 2^30 on
        wide = _gram_job(N, **{field: 1 << 15, "ldA": 1 << 15, "ldG": 1 << 15, "ldo": 1 << 17})
        assert call(N.as_array(N.GramJob, [wide]), 1, WS, 1 << 62) == N.KFAC_EINVAL, field


def test_tri_argument_checks():
    N = _N()
    lib = N.lib()
    pack = lambda arr, n, packed=OUT: lib.kfac_tri_pack(arr, n, packed, None)
    unpack = lambda arr, n, packed=OUT, mode=N.TRI_LOWER: lib.kfac_tri_unpack(arr, n, packed, mode, None)
    ok = N.as_array(N.TriJob, [_tri_job(N)])
    for call in (pack, unpack):
        assert call(ok, -1) == N.KFAC_EINVAL
        assert call(None, 1) == N.KFAC_EINVAL
        assert call(ok, 1, packed=None) == N.KFAC_EINVAL
        for field, value in TRI_BAD:
            j = _tri_job(N, **{field: value})
            assert call(N.as_array(N.TriJob, [j]), 1) == N.KFAC_EINVAL, (field, value)
            assert call(N.as_array(N.TriJob, [_tri_job(N, n=0), j]), 2) == N.KFAC_EINVAL, (field, value)
        # nothing to move: no launch, no error
        assert call(ok, 0) == N.KFAC_OK
        assert call(N.as_array(N.TriJob, [_tri_job(N, n=0)]), 1) == N.KFAC_OK
    for mode in (-1, 2):
        assert unpack(ok, 1, mode=mode) == N.KFAC_EINVAL
