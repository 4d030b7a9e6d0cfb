"""GPU: the class-tiled weighted covariance calls -- kfac_kron_cov_full_tiled,
kfac_kron_cov_outer_full_tiled, kfac_kron_cov_sweep_tiled, kfac_kron_cov_outer_sweep_tiled
(variance.kron_covariance_*_tiled) -- above 32 outputs: against fp64 numpy on the same fp32
inputs (glm_full_cases / glm_sweep_cases, which take any nc), integer-exact against int64, the
bitwise guarantees (repeatable, symmetric, per sample, per grid point, the tie to
kron_covariance_tiled at weights 1), and against the capped siblings, each other and the dense
route.

Kernel tolerance: rtol 1e-5, atol = scale * max|ref[t]| per grid point, scale 1e-5 except the
nG = 2100 outer shape (glm_wtiled_cases.scale_for: 1.4e-5, four times its sequential-fp32 host
emulation).  Two fp32 device routes on one quantity: 2e-5 * max (test_gpu_glm_full._close)."""
import numpy as np
import pytest
import torch

import glm_full_cases as C
import glm_sweep_cases as S
import glm_wtiled_cases as T
from test_gpu_glm_full import IDS, _check, _close, _dev, _padded_matrices, _padded_rows

pytestmark = pytest.mark.gpu

CALLS = ["full", "outer_full", "sweep", "outer_sweep"]


def _fn(call):
    from bnn_kfac_amd import variance as V
    return {"full": V.kron_covariance_full_tiled, "outer_full": V.kron_covariance_outer_full_tiled,
            "sweep": V.kron_covariance_sweep_tiled, "outer_sweep": V.kron_covariance_outer_sweep_tiled}[call]


def _capped(call):
    from bnn_kfac_amd import variance as V
    return {"full": V.kron_covariance_full, "outer_full": V.kron_covariance_outer_full,
            "sweep": V.kron_covariance_sweep, "outer_sweep": V.kron_covariance_outer_sweep}[call]


def _case(call, shape):
    """(operands without weights, weight arrays (NT_MAX leading), fp64 reference)."""
    if call == "full":
        J, VA, VG, W, ref = C.dense_case(*shape)
        return (J, VA, VG), (W,), ref
    if call == "outer_full":
        a, D, VA, VG, W, ref = C.outer_case(*shape)
        return (a, D, VA, VG), (W,), ref
    if call == "sweep":
        J, VA, VG, wA, wG, ref = S.dense_case(*shape)
        return (J, VA, VG), (wA, wG), ref
    a, D, VA, VG, wA, wG, ref = S.outer_case(*shape)
    return (a, D, VA, VG), (wA, wG), ref


def _terms(dev, call, shape, rows):
    """([term], ref[rows]) with grid points `rows` (a slice or an index array)."""
    ops, ws, ref = _case(call, shape)
    return [tuple(_dev(dev, *ops, *(w[rows] for w in ws)))], ref[rows]


def _shapes(call):
    return T.OUTER_SHAPES if call.startswith("outer") else T.DENSE_SHAPES


ALL = [(call, shape) for call in CALLS for shape in _shapes(call)]
ALL_IDS = [f"{call}-{IDS(shape)}" for call, shape in ALL]
# per call: the smallest shape, one with several tile pairs, and the two-segment one
SOME = [(call, shape) for call in CALLS for shape in (_shapes(call)[0], _shapes(call)[2 if "outer" in call else 1],
                                                      T.LONG_OUTER if "outer" in call else T.LONG_DENSE)]
SOME_IDS = [f"{call}-{IDS(shape)}" for call, shape in SOME]


# ------------------------------------------------------------------ against fp64
@pytest.mark.parametrize("nt", T.NTS)
@pytest.mark.parametrize("call,shape", ALL, ids=ALL_IDS)
def test_matches_fp64(hip_device, call, shape, nt):
    terms, ref = _terms(hip_device, call, shape, slice(0, nt))
    got = _fn(call)(terms)
    nb, nc = shape[-2:]
    assert got.shape == (nt, nb, nc, nc) and got.dtype == torch.float32
    _check(got.cpu().numpy(), ref, scale=T.scale_for(shape))


# ------------------------------------------------------------------ integer-exact
INT_DENSE = [dict(nA=33, nG=65, nb=2, nc=40, nt=5), dict(nA=5, nG=4, nb=3, nc=65, nt=5)]
INT_OUTER = [dict(cols=64, ones=1, nG=10, nb=3, nc=65, nt=5), dict(cols=20, ones=1, nG=2100, nb=2, nc=40, nt=2)]
INT_IDS = lambda k: "x".join(str(v) for v in k.values())  # noqa: E731


def _exact(got, want):
    assert np.abs(want).max() > 0
    assert torch.equal(got.cpu(), torch.from_numpy(want.astype(np.float32)))


@pytest.mark.parametrize("kw", INT_DENSE, ids=INT_IDS)
def test_dense_integer_exact(hip_device, kw):
    """Small-integer inputs: every term any stage accumulates sums (in absolute value) below
    2^24, so every order of fp32 summation is exact and the whole buffer equals int64's."""
    J, VA, VG, W, want, bound = C.int_dense_case(**kw)
    print("bound", bound)
    assert 0 < bound < C.EXACT
    if kw["nc"] == 40:
        assert bound == 93181
    _exact(_fn("full")([tuple(_dev(hip_device, J, VA, VG, W))]), want)
    # rank one: integer wA, wG in {0, 1, 2}; |terms| <= 4 |Y|^2 summed, bounded as above
    nA, nG, nb, nc, nt = kw["nA"], kw["nG"], kw["nb"], kw["nc"], kw["nt"]
    wA, wG = T.int_rank_one(nt, nA, nG)
    Ji, VAi, VGi = (np.rint(t).astype(np.int64) for t in (J, VA, VG))
    Y = np.einsum("ai,bcag,gh->bcih", VAi, Ji.reshape(nb, nc, nA, nG), VGi)
    want1 = np.einsum("ti,th,bcih,bdih->tbcd", wA, wG, Y, Y)
    bound1 = int(np.einsum("ti,th,bcih,bdih->tbcd", wA, wG, np.abs(Y), np.abs(Y)).max())
    print("rank-one bound", bound1)
    assert 0 < bound1 < C.EXACT and set(np.unique(wA)) | set(np.unique(wG)) == {0, 1, 2}
    f = lambda t: t.astype(np.float32)  # noqa: E731
    _exact(_fn("sweep")([tuple(_dev(hip_device, J, VA, VG, f(wA), f(wG)))]), want1)


@pytest.mark.parametrize("kw", INT_OUTER, ids=INT_IDS)
def test_outer_integer_exact(hip_device, kw):
    a, D, VA, VG, W, want, bound = C.int_outer_case(**kw)
    print("bound", bound)
    assert 0 < bound < C.EXACT
    if kw["nG"] == 2100:
        assert bound == 1221826
    _exact(_fn("outer_full")([tuple(_dev(hip_device, a, D, VA, VG, W))]), want)
    nA, nG, nb, nt = kw["cols"] + kw["ones"], kw["nG"], kw["nb"], kw["nt"]
    wA, wG = T.int_rank_one(nt, nA, nG)
    ai, Di, VAi, VGi = (np.rint(t).astype(np.int64) for t in (a, D, VA, VG))
    abar = np.concatenate([ai, np.ones((nb, 1), np.int64)], axis=1) if kw["ones"] else ai

    def run(abar, Dm, VAm, VGm):
        p = abar @ VAm
        s = (p * p) @ wA.T                                  # (nb, nt)
        Q = Dm @ VGm
        gram = np.einsum("bcg,tg,bdg->tbcd", Q, wG, Q)
        return (p, s, Q, gram), s.T[:, :, None, None] * gram

    _, want1 = run(abar, Di, VAi, VGi)
    stages, top = run(np.abs(abar), np.abs(Di), np.abs(VAi), np.abs(VGi))
    bound1 = max(int(top.max()), *(int(s.max()) for s in stages))
    print("rank-one bound", bound1)
    assert 0 < bound1 < C.EXACT
    f = lambda t: t.astype(np.float32)  # noqa: E731
    _exact(_fn("outer_sweep")([tuple(_dev(hip_device, a, D, VA, VG, f(wA), f(wG)))]), want1)


# ------------------------------------------------------------------ 1, 3: bits
@pytest.mark.parametrize("call,shape", SOME, ids=SOME_IDS)
def test_repeatable_symmetric_and_slices_stand_alone(hip_device, call, shape):
    """Two calls give the same bits; every block is bitwise symmetric with a non-negative
    diagonal; slice t of an nt = 5 call has the bits of the nt = 1 call with grid point t."""
    fn = _fn(call)
    terms, _ = _terms(hip_device, call, shape, slice(0, 5))
    five = fn(terms)
    assert torch.equal(five, fn(terms))
    assert torch.equal(five, five.mT)
    assert bool((torch.diagonal(five, dim1=2, dim2=3) >= 0).all())
    for t in range(5):
        alone, _ = _terms(hip_device, call, shape, slice(t, t + 1))
        assert torch.equal(fn(alone)[0], five[t]), t


@pytest.mark.parametrize("call", CALLS)
def test_64_grid_points_on_the_smallest_shape(hip_device, call):
    fn, shape = _fn(call), _shapes(call)[0]
    terms, ref = _terms(hip_device, call, shape, slice(0, 64))
    got = fn(terms)
    assert got.shape[0] == 64
    _check(got.cpu().numpy(), ref, scale=T.scale_for(shape))
    for t in (0, 1, 37, 63):
        alone, _ = _terms(hip_device, call, shape, slice(t, t + 1))
        assert torch.equal(fn(alone)[0], got[t]), t
    # 65 grid points go through two device calls
    order = np.concatenate([np.arange(64), [5]])
    terms, _ = _terms(hip_device, call, shape, order)
    more = fn(terms)
    assert torch.equal(more[:64], got) and torch.equal(more[64], got[5])


# ------------------------------------------------------------------ 2: per sample
def _job_bytes(call, shape, n, nt):
    from bnn_kfac_amd import _native as N
    if call.startswith("outer"):
        cols, ones, nG, nb, nc = shape
        nA = cols + ones
        if call == "outer_full":
            job = N.CovOuterFullJob(1, cols, cols, ones, 1, nG, nG, 0, 1, nA, 1, nG, 1, nA * nG)
            return N.kron_cov_outer_full_tiled_workspace_bytes([job], n, nc, nt)
        job = N.CovOuterSweepJob(1, cols, cols, ones, 1, nG, nG, 0, 1, nA, 1, nG, 1, nA, 1, nG)
        return N.kron_cov_outer_sweep_tiled_workspace_bytes([job], n, nc, nt)
    nA, nG, nb, nc = shape
    if call == "full":
        return N.kron_cov_full_tiled_workspace_bytes([N.CovFullJob(1, nA * nG, nA, nG, 1, nA, 1, nG, 1, nA * nG)],
                                                     n, nc, nt)
    return N.kron_cov_sweep_tiled_workspace_bytes([N.CovSweepJob(1, nA * nG, nA, nG, 1, nA, 1, nG, 1, nA, 1, nG)],
                                                  n, nc, nt)


@pytest.mark.parametrize("call,shape", SOME, ids=SOME_IDS)
def test_one_sample_chunks_do_not_change_a_bit(hip_device, call, shape):
    fn = _fn(call)
    terms, _ = _terms(hip_device, call, shape, slice(0, 5))
    whole = fn(terms)
    if shape[-2] > 1:
        one, two = _job_bytes(call, shape, 1, 5), _job_bytes(call, shape, 2, 5)
        assert 0 < one < two  # a budget of `one` forces chunks of one sample
        assert torch.equal(fn(terms, max_workspace_bytes=one), whole)
    else:
        one = _job_bytes(call, shape, 1, 5)
    with pytest.raises(ValueError):
        fn(terms, max_workspace_bytes=one - 1)   # the workspace-too-small error


@pytest.mark.parametrize("call", CALLS)
def test_sample_block_unchanged_by_other_samples(hip_device, call):
    fn = _fn(call)
    shape = (130, 1, 130, 70, 33) if call.startswith("outer") else (9, 7, 3, 65)
    (term,), _ = _terms(hip_device, call, shape, slice(0, 2))
    whole = fn([term])
    nlead = 2 if call.startswith("outer") else 1          # a, D / J carry the samples
    for rows in (slice(0, 1), slice(shape[-2] - 2, shape[-2])):
        part = tuple(t[rows] if i < nlead else t for i, t in enumerate(term))
        assert torch.equal(fn([part]), whole[:, rows])


# ------------------------------------------------------------------ 4: the dense-route tie
@pytest.mark.parametrize("shape", T.DENSE_SHAPES, ids=IDS)
def test_unit_weights_give_the_bits_of_kron_covariance_tiled(hip_device, shape):
    """w = 1 is exact, and the segmentation, the chain order and the reduce order are those of
    kfac_kron_cov_tiled: one tile implementation."""
    from bnn_kfac_amd.variance import kron_covariance_tiled
    nA, nG = shape[:2]
    J, VA, VG = _dev(hip_device, *C.dense_case(*shape)[:3])
    want = kron_covariance_tiled([(J, VA, VG)], lower=False)
    ones = torch.ones(3, nA, nG, device=hip_device)
    full = _fn("full")([(J, VA, VG, ones)])
    sweep = _fn("sweep")([(J, VA, VG, ones[:, :, 0].contiguous(), ones[:, 0, :].contiguous())])
    for t in range(3):
        assert torch.equal(full[t], want), t
        assert torch.equal(sweep[t], want), t


# ------------------------------------------------------------------ 5: the capped siblings
CAPPED = [("full", (26, 5, 3, 32)), ("full", (33, 65, 2, 5)), ("sweep", (26, 5, 3, 32)), ("sweep", (33, 65, 2, 5)),
          ("outer_full", (20, 1, 31, 2, 32)), ("outer_full", (130, 1, 130, 70, 2)),
          ("outer_sweep", (20, 1, 31, 2, 32)), ("outer_sweep", (130, 1, 130, 70, 2))]


@pytest.mark.parametrize("call,shape", CAPPED, ids=[f"{c}-{IDS(s)}" for c, s in CAPPED])
def test_agrees_with_the_capped_sibling_up_to_32_outputs(hip_device, call, shape):
    terms, _ = _terms(hip_device, call, shape, slice(0, 5))
    _close(_fn(call)(terms), _capped(call)(terms))


# ------------------------------------------------------------------ 6: rank-one weights
@pytest.mark.parametrize("shape", [(9, 7, 3, 65), (33, 65, 2, 40)], ids=IDS)
def test_dense_rank_one_weights_agree_with_the_sweep(hip_device, shape):
    J, VA, VG, wA, wG = _dev(hip_device, *S.dense_case(*shape)[:5])
    wA, wG = wA[:5], wG[:5]
    W = wA[:, :, None] * wG[:, None, :]
    _close(_fn("full")([(J, VA, VG, W)]), _fn("sweep")([(J, VA, VG, wA, wG)]))


@pytest.mark.parametrize("shape", [(64, 1, 40, 5, 65), (20, 1, 2100, 2, 40), (130, 1, 130, 70, 33)], ids=IDS)
def test_outer_rank_one_weights_agree_with_the_sweep(hip_device, shape):
    a, D, VA, VG, wA, wG = _dev(hip_device, *S.outer_case(*shape)[:6])
    wA, wG = wA[:5], wG[:5]
    W = wA[:, :, None] * wG[:, None, :]
    _close(_fn("outer_full")([(a, D, VA, VG, W)]), _fn("outer_sweep")([(a, D, VA, VG, wA, wG)]))


# ------------------------------------------------------------------ 7: the two routes
@pytest.mark.parametrize("shape", [(4, 1, 3, 1, 33), (63, 1, 10, 3, 64), (64, 1, 40, 5, 65)], ids=IDS)
def test_outer_route_agrees_with_dense_route_on_materialised_rows(hip_device, shape):
    a, D, VA, VG, W, ref = C.outer_case(*shape)
    ad, Dd, VAd, VGd, Wd, Jd = _dev(hip_device, a, D, VA, VG, W[:5], C.rows_of(a, shape[1], D))
    dense = _fn("full")([(Jd, VAd, VGd, Wd)])
    _close(_fn("outer_full")([(ad, Dd, VAd, VGd, Wd)]), dense)
    _check(dense.cpu().numpy(), ref[:5])
    a, D, VA, VG, wA, wG, ref = S.outer_case(*shape)
    ad, Dd, VAd, VGd, wAd, wGd = _dev(hip_device, a, D, VA, VG, wA[:5], wG[:5])
    dense = _fn("sweep")([(Jd, VAd, VGd, wAd, wGd)])     # (the same a, D: the case modules share seeds)
    assert np.array_equal(a, C.outer_case(*shape)[0]) and np.array_equal(D, C.outer_case(*shape)[1])
    _close(_fn("outer_sweep")([(ad, Dd, VAd, VGd, wAd, wGd)]), dense)
    _check(dense.cpu().numpy(), ref[:5])


# ------------------------------------------------------------------ jobs, strides, accumulate
def test_nine_terms_fold_in_groups_of_eight(hip_device):
    nt, nb, nc = 3, 2, 40
    oshapes = [(4, 1, 3), (63, 1, 10), (9, 0, 10), (70, 1, 65), (12, 1, 4), (20, 1, 130), (33, 0, 31),
               (8, 1, 8), (64, 1, 64)]
    dshapes = [(5, 3), (64, 10), (9, 10), (33, 65), (12, 4), (20, 13), (70, 1), (8, 8), (26, 5)]
    for call, shapes in (("outer_full", oshapes), ("outer_sweep", oshapes), ("full", dshapes), ("sweep", dshapes)):
        terms, ref = [], 0.0
        for shape in shapes:
            (term,), r = _terms(hip_device, call, (*shape, nb, nc), slice(0, nt))
            terms.append(term)
            ref = ref + r
        got = _fn(call)(terms)
        _check(got.cpu().numpy(), ref)
        # 8 + 1: the ninth term is accumulated onto the first eight's sum
        first, last = _fn(call)(terms[:8]), _fn(call)(terms[8:])
        _close(got, first + last, scale=1e-6)


def test_accumulate_adds_through_the_c_call(hip_device):
    from bnn_kfac_amd import _native as N
    nt = 3
    a, D, VA, VG, W, ref = C.outer_case(63, 1, 10, 3, 64)
    ad, Dd, VAd, VGd, Wd = _dev(hip_device, a, D, VA, VG, W[:nt])
    job = N.CovOuterFullJob(ad.data_ptr(), 63, 63, 1, Dd.data_ptr(), 10, 10, 0, VAd.data_ptr(), 64,
                            VGd.data_ptr(), 10, Wd.data_ptr(), 640)
    base = torch.from_numpy(np.array(ref[:nt])).float().to(hip_device) * 0.5
    base = (base + base.mT) / 2
    out = base.clone()
    N.kron_cov_outer_full_tiled([job], 3, 64, nt, out, accumulate=True)
    _check(out.cpu().numpy(), ref[:nt] + base.cpu().numpy().astype(np.float64))
    N.kron_cov_outer_full_tiled([job], 3, 64, nt, out, accumulate=False)
    _check(out.cpu().numpy(), ref[:nt])


@pytest.mark.parametrize("shape", [(64, 1, 40, 5, 65)], ids=IDS)
def test_outer_strided_inputs_bit_equal(hip_device, shape):
    (a, D, VA, VG, W), = _terms(hip_device, "outer_full", shape, slice(0, 5))[0]
    plain = _fn("outer_full")([(a, D, VA, VG, W)])
    wide = torch.full((a.shape[0], a.shape[1] + 7), float("nan"), device=hip_device)
    wide[:, 2:2 + a.shape[1]] = a
    a_slice = wide[:, 2:2 + a.shape[1]]
    Dp, Wp = _padded_rows(D, hip_device), _padded_matrices(W, hip_device)
    for terms in ((a_slice, D, VA, VG, W), (a, D, VA, VG, Wp), (a, Dp, VA, VG, W),
                  (a_slice, Dp, _padded_rows(VA, hip_device), _padded_rows(VG, hip_device), Wp)):
        assert torch.equal(_fn("outer_full")([terms]), plain)
    (a, D, VA, VG, wA, wG), = _terms(hip_device, "outer_sweep", shape, slice(0, 5))[0]
    plain = _fn("outer_sweep")([(a, D, VA, VG, wA, wG)])
    wAp, wGp = _padded_rows(wA, hip_device), _padded_rows(wG, hip_device)   # weights with a row stride
    assert wAp.stride(0) == wA.shape[1] + 3
    for terms in ((a_slice, Dp, VA, VG, wA, wG), (a, D, VA, VG, wAp, wGp),
                  (a_slice, Dp, _padded_rows(VA, hip_device), _padded_rows(VG, hip_device), wAp, wGp)):
        assert torch.equal(_fn("outer_sweep")([terms]), plain)


@pytest.mark.parametrize("shape", [(9, 7, 3, 65), (33, 65, 2, 40)], ids=IDS)
def test_dense_strided_inputs_bit_equal(hip_device, shape):
    from bnn_kfac_amd.variance import _cov_rows
    (J, VA, VG, W), = _terms(hip_device, "full", shape, slice(0, 5))[0]
    plain = _fn("full")([(J, VA, VG, W)])
    Jp, Wp = _padded_rows(J, hip_device), _padded_matrices(W, hip_device)
    assert _cov_rows(Jp, J.shape[2])[1] == J.shape[2] + 3      # a padded row stride: not copied
    for terms in ((Jp, VA, VG, W), (J, VA, VG, Wp),
                  (Jp, _padded_rows(VA, hip_device), _padded_rows(VG, hip_device), Wp)):
        assert torch.equal(_fn("full")([terms]), plain)
    (J, VA, VG, wA, wG), = _terms(hip_device, "sweep", shape, slice(0, 5))[0]
    plain = _fn("sweep")([(J, VA, VG, wA, wG)])
    wAp, wGp = _padded_rows(wA, hip_device), _padded_rows(wG, hip_device)
    for terms in ((Jp, VA, VG, wA, wG), (J, VA, VG, wAp, wGp),
                  (Jp, _padded_rows(VA, hip_device), _padded_rows(VG, hip_device), wAp, wGp)):
        assert torch.equal(_fn("sweep")([terms]), plain)
