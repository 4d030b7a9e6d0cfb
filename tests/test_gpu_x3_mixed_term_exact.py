"""GPU: kfac_factor_tiles_x3's mixed units (S3D3, P1D2) against the six-term sum, bit for bit,
on the term-exact data of tests/x3_exact.py (values +-{1, 1 + 2^-9, 1 + 2^-9 + 2^-18}, 16 live
K-rows; test_x3_exact_data.py proves the data's properties on the host for any column count).

Factor orders 129 (128 + ones) and 160: P = 5, a K4, an S3D3 and a P1D2 each, so every block
of the two new kinds -- the three hub blocks and the six diagonal ones -- is held to all six
products; a lost, doubled or mis-paired mid mid, hi lo or lo hi term fails by a multiple of
2^-18.  A 256-column job rides along: a group routes to kfac_factor_tiles_x3 only when its
largest factor has n >= 256.  One batch (three seeds), three batches, and the deferred
accumulators; the family asserted by its profile slot."""
import numpy as np
import pytest
import torch

import x3_exact as X
from test_gpu_x3_term_exact import _check, _device_job

pytestmark = pytest.mark.gpu

SIZES = [(128, True), (160, False), (256, False)]  # (cols, ones)
MODES = {"seed0": (10, 96, 1, False), "seed1": (11, 96, 1, False), "seed2": (12, 96, 1, False),
         "nseg3": (13, 64, 3, False), "deferred": (14, 96, 1, True)}  # seed, rows, batches, deferred


@pytest.mark.parametrize("mode", list(MODES))
def test_x3_mixed_term_exact(hip_device, mode):
    from bnn_kfac_amd import _native as N
    seed, rows, nseg, deferred = MODES[mode]
    rng = np.random.default_rng(seed)
    host = [X._rowmajor_job(rng, cols, ones, rows, nseg) for cols, ones in SIZES]
    keep, jobs, outs = [], [], []
    for job in host:
        fj, F = _device_job(N, hip_device, job, keep)
        jobs.append(fj)
        outs.append(F)
    N.profile_reset()
    N.profile_enable(True)
    try:
        if deferred:
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
    assert N.profile_read(N.PROF_FACTOR_X3)[1] == 1  # one kfac_factor_tiles_x3 launch
    assert N.profile_read(N.PROF_FACTOR_TILES)[1] == 0 and N.profile_read(N.PROF_FACTOR_SYRK3)[1] == 0
    for job, F in zip(host, outs):
        _check(job, F, mode)
