"""GPU: the bf16x3 factor kernels against the six-term sum, bit for bit, on inputs whose hi,
mid and lo parts are all non-zero (tests/x3_exact.py; test_x3_exact_data.py proves on the
host that the data is exact in every summation order and that every one of the six products
shows in every 32 x 32 block).  The integer-exact tests (test_gpu_x3_cliques.py,
test_mfma_layout_asymmetric, test_x3_*_exact) bind the geometry through hi hi alone; a lost,
doubled or mis-paired mid mid, hi lo or lo hi product stays inside their random-data
tolerance and fails here by a multiple of 2^-18.

Raw C ABI, F = 1.0 X^T X + 0.0 F onto a NaN-filled F, the family asserted by its profile
slot: kfac_factor_tiles_x3 (one launch group of P = 9 with a one-column last panel, P = 10,
the Steiner table and a narrow job; three seeds, three batches, the deferred accumulators),
kfac_factor_syrk3 (n = 2048 and 2053), kfac_factor_conv_x3 / _x3s / _x3f (two shapes each,
the live patch against the top-left padding, in the last image's bottom-right corner and in
the interior) and kfac_factor_channel_x3."""
import numpy as np
import pytest
import torch

import x3_exact as X

pytestmark = pytest.mark.gpu


def _slot(N, family):
    return {"tiles_x3": N.PROF_FACTOR_X3, "syrk3": N.PROF_FACTOR_SYRK3, "conv_x3": N.PROF_FACTOR_CONV_X3,
            "conv_x3s": N.PROF_FACTOR_CONV_X3S, "conv_x3f": N.PROF_FACTOR_CONV_X3F,
            "channel_x3": N.PROF_FACTOR_CHANNEL_X3}[family]


def _device_job(N, dev, job, keep):
    """The kfac_factor_job of a host job and its NaN-filled output."""
    bufs = [torch.from_numpy(np.ascontiguousarray(b)).to(dev) for b in job.batches]
    keep += bufs
    if job.layout == "rowmajor":
        op = N.rowmajor_operand(bufs[0], job.ones)
    elif job.layout == "channel":
        op = N.channel_operand(bufs[0])
    else:
        k, s, p = job.conv
        op = N.patch_operand(bufs[0], k, p, s, job.ones)
    F = torch.full((job.n, job.n), float("nan"), device=dev)
    fj = N.factor_job(op, F, 1.0, 0.0)
    if len(bufs) > 1:
        table = N.segment_table([b.data_ptr() for b in bufs])
        keep.append(table)
        fj.seg_ptrs, fj.nseg = N.table_ptr(table), len(bufs)
    return fj, F


def _check(job, F, gid):
    got = F.cpu().numpy()
    want = job.want.astype(np.float32)
    if np.array_equal(got, want):
        return
    err = np.abs(got.astype(np.float64) - job.want) / X.U18
    err[np.isnan(err)] = np.inf
    i, j = np.unravel_index(np.argmax(err), err.shape)
    bad = sorted({(int(a) // 32, int(b) // 32) for a, b in np.argwhere(err > 0)})
    np.testing.assert_array_equal(
        got, want, err_msg=f"{gid} job {job.name}, n = {job.n}: worst error {err[i, j]:.6g} x 2^-18 at ({i}, {j}), "
                           f"32 x 32 block ({i // 32}, {j // 32}); {len(bad)} blocks differ, first {bad[:12]}")


@pytest.mark.parametrize("gid", X.GROUP_IDS)
def test_x3_term_exact(hip_device, gid):
    from bnn_kfac_amd import _native as N
    group = X.GROUPS[X.GROUP_IDS.index(gid)]
    keep, jobs, outs = [], [], []
    for job in group.jobs:
        fj, F = _device_job(N, hip_device, job, keep)
        jobs.append(fj)
        outs.append(F)
    N.profile_reset()
    N.profile_enable(True)
    try:
        if group.mode == "deferred":
            flush = []
            for fj, (splits, nbytes) in zip(jobs, N.factor_accum_plan(jobs)):
                acc = torch.empty(nbytes, dtype=torch.uint8, device=hip_device)
                keep.append(acc)
                fj.acc, fj.acc_splits, fj.acc_beta = acc.data_ptr(), splits, 0.0
                flush.append(N.FactorJob.from_buffer_copy(fj))
            N.factor_update(jobs, hip_device)
            N.factor_flush(flush, hip_device)
        else:
            N.factor_update(jobs, hip_device)
        torch.cuda.synchronize()
    finally:
        N.profile_enable(False)
    launches = {f: N.profile_read(_slot(N, f))[1] for f in ("tiles_x3", "syrk3", "conv_x3", "conv_x3s", "conv_x3f",
                                                             "channel_x3")}
    assert launches.pop(group.family) == 1 and not any(launches.values()), (group.family, launches)
    assert N.profile_read(N.PROF_FACTOR_TILES)[1] == 0 and N.profile_read(N.PROF_FACTOR_CONV)[1] == 0
    for job, F in zip(group.jobs, outs):
        _check(job, F, gid)
