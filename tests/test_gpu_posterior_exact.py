"""GPU: kfac_sample, kfac_kron_quadform, kfac_efb_update, kfac_kron_gram and kfac_tri_pack /
kfac_tri_unpack on the integer cases of posterior_cases.py, through the raw job structs.
Every operand of a case lives in one NaN-filled device buffer; after the call the WHOLE
buffer must equal the reference's: the written region the exact integers, everything else
(padding columns, columns at or beyond wcols, gaps between J rows, the inputs) its prefill.
Every comparison is an equality."""
import numpy as np
import pytest
import torch

import posterior_cases as P

pytestmark = pytest.mark.gpu


def _ids(cases):
    return [c.id for c in cases]


def _upload(case, dev):
    flat = torch.from_numpy(case.arena.array()).to(dev)
    assert flat.data_ptr() % 16 == 0
    return flat, (lambda off: None if off is None else flat.data_ptr() + 4 * off)


def _check(case, flat, want):
    torch.cuda.synchronize()
    got = flat.cpu().numpy()
    diff = P.first_difference(case.arena, got, want)
    assert diff is None, f"{case.kind} {case.id}: {diff}"
    assert np.array_equal(got, want, equal_nan=True)


# ---------------------------------------------------------------------------- sample
@pytest.mark.parametrize("case", P.sample_cases(), ids=_ids(P.sample_cases()))
def test_sample(hip_device, case):
    """<= 8 jobs: one kfac_sample call; group9-chunks: two calls sharing the workspace."""
    from bnn_kfac_amd import _native as N
    flat, p = _upload(case, hip_device)
    jobs = [N.SampleJob(p(j.oLA), j.ldA, p(j.oLG), j.ldG, p(j.oZ), j.nA, j.nG, p(j.oW), j.ldW, p(j.oB),
                        j.wcols, j.dense) for j in case.jobs]
    if case.id.startswith("loader"):  # z is contiguous; its base decides the float4 path
        assert all((p(j.oZ) % 16 != 0) == case.odd and p(j.oZ) % 4 == 0 for j in case.jobs)
    N.sample(jobs, hip_device, bool(case.accumulate))
    _check(case, flat, P.sample_reference(case))


# -------------------------------------------------------------------------- quadform
RAW_QUAD = [c for c in P.quad_cases() if c.via == "raw"]
FOLD_QUAD = [c for c in P.quad_cases() if c.via == "wrapper"]


@pytest.mark.parametrize("case", RAW_QUAD, ids=_ids(RAW_QUAD))
def test_quadform(hip_device, case):
    """v[j][b] = (float) of the exact integer, out[b] = (float) of their (absolute) sum."""
    from bnn_kfac_amd import _native as N
    flat, p = _upload(case, hip_device)
    jobs = [N.QuadJob(p(j.oJ), j.ldJ, j.nA, j.nG, p(j.o1), j.ld1, p(j.o2), j.ld2, j.lower1, j.lower2,
                      p(j.oV)) for j in case.jobs]
    out = torch.as_strided(flat, (case.nb,), (1,), case.oOut)
    N.kron_quadform(jobs, case.nb, bool(case.abs_sum), out)
    v, total = P.quad_reference(case)
    _check(case, flat, P.quad_expected(case, v, total))


@pytest.mark.parametrize("case", FOLD_QUAD, ids=_ids(FOLD_QUAD))
def test_quadform_fold_over_nine_terms(hip_device, case):
    """variance.kron_quadform with nine strided terms: two calls, `acc += part` in fp32."""
    from bnn_kfac_amd import variance
    flat, _ = _upload(case, hip_device)
    terms = [(torch.as_strided(flat, (case.nb, j.nA * j.nG), (j.ldJ, 1), j.oJ),
              torch.as_strided(flat, (j.nA, j.nA), (j.ld1, 1), j.o1),
              torch.as_strided(flat, (j.nG, j.nG), (j.ld2, 1), j.o2)) for j in case.jobs]
    lower = bool(case.jobs[0].lower1)
    assert all(j.lower1 == j.lower2 == int(lower) for j in case.jobs)
    out, v = variance.kron_quadform(terms, lower=lower, abs_sum=bool(case.abs_sum), per_term=True)
    want_v, want_out = P.quad_reference(case)
    got_v, got_out = v.cpu().numpy(), out.cpu().numpy()
    for t, (g, w) in enumerate(zip(got_v, want_v)):
        assert np.array_equal(g, w), f"{case.id}: term {t} ({case.jobs[t].nA} x {case.jobs[t].nG}): got {g}, want {w}"
    assert np.array_equal(got_out, want_out), f"{case.id}: out got {got_out}, want {want_out}"
    _check(case, flat, case.arena.array())  # the inputs are as they were


# ------------------------------------------------------------------------------- EFB
@pytest.mark.parametrize("case", P.efb_cases(), ids=_ids(P.efb_cases()))
def test_efb_update(hip_device, case):
    """Two batches (accumulate 0 onto NaN, then 1); nine jobs run as two calls."""
    from bnn_kfac_amd import _native as N
    flat, p = _upload(case, hip_device)
    for i in range(2):
        jobs = [N.EfbJob(p(j.oVA), j.ldA, p(j.oVG), j.ldG, p(j.oGr[i]), j.ld_grad, p(j.oS), j.ld_state,
                         p(j.oD), j.ld_diag if j.has_diag else 0, j.nA, j.nG, int(i > 0), P.EFB_SCALE)
                for j in case.jobs]
        N.efb_update(jobs, hip_device)
    _check(case, flat, P.efb_reference(case))


# ------------------------------------------------------------------------------ Gram
@pytest.mark.parametrize("case", P.gram_cases(), ids=_ids(P.gram_cases()))
def test_kron_gram(hip_device, case):
    """Raw GramJobs, built as N.kron_gram builds its one; with power-of-two sigma the output
    is the exact integer sum, scaled exactly, and exactly symmetric."""
    from bnn_kfac_amd import _native as N
    flat, p = _upload(case, hip_device)
    jobs = [N.GramJob(p(j.oUA), j.ldA, p(j.oUG), j.ldG, p(j.oC), p(j.oSig), p(j.oOut), j.ldo, j.nA, j.nG,
                      j.la, j.lg) for j in case.jobs]
    L = N.lib()
    arr = N.as_array(N.GramJob, jobs)
    ws = N.workspace.get(hip_device, L.kfac_gram_workspace_bytes(arr, len(jobs)))
    N.check(L.kfac_kron_gram(arr, len(jobs), N.ptr(ws), ws.numel(), N.stream_handle(hip_device)),
            "kfac_kron_gram")
    _check(case, flat, P.gram_reference(case))
    got = flat.cpu().numpy()
    for j in case.jobs:
        G = got[P.idx(j.oOut, j.la * j.lg, j.la * j.lg, j.ldo)]
        assert np.array_equal(G, G.T)


# -------------------------------------------------------------------------- tri-pack
@pytest.mark.parametrize("op", ["pack", "unpack_sym", "unpack_lower"])
def test_tri_pack_unpack(hip_device, op):
    """Twenty strided factors in one call (chunks of 16 and 4), offsets in a permuted order."""
    from bnn_kfac_amd import _native as N
    case = P.tri_case(op)
    flat, p = _upload(case, hip_device)
    jobs = [N.TriJob(p(j.oF), j.ldF, j.n, 0, j.offset) for j in case.jobs]
    packed = torch.as_strided(flat, (case.total,), (1,), case.oP)
    if op == "pack":
        N.tri_pack(jobs, packed)
    else:
        N.tri_unpack(jobs, packed, case.mode)
    _check(case, flat, P.tri_reference(case))
