"""The factor planner and kernel routing, pinned from the host side (no GPU calls).

kfac_factor_accum_plan and kfac_factor_workspace_bytes run the same routing and K-split
planner as kfac_factor_update without touching a device, so the operands here carry fake
non-null pointers.  EXPECTED was recorded with the library as it stood before the routing
was gathered into one place (factor.hip's route_group) and the kernels were split into one
file per family: (splits per job, accumulator bytes per job, workspace bytes of the call).
A change of any figure is a change of which kernel a job gets or of how it is split.
"""
import pytest

BASE = 0x10000  # fake operand pointer, 16-byte aligned
F_PTR = 0x20000


def _job(N, op, n):
    job = N.FactorJob()
    job.x, job.alpha, job.beta, job.F, job.ldF = op, 1.0, 0.0, F_PTR, n
    return job


def _rowmajor(N, rows, cols, ones, ptr=BASE, bases=None, last_rows=0):
    op = N.Operand(ptr, N.ROWMAJOR, cols, rows, int(ones), last_rows, cols)
    job = _job(N, op, cols + int(ones))
    keep = None
    if bases:
        keep = N.segment_table(bases)
        job.x.ptr, job.seg_ptrs, job.nseg = bases[0], N.table_ptr(keep), len(bases)
    return job, keep


def _patch(N, B, C, H, W, k, s=(1, 1), p=(0, 0), bias=True):
    op = N.Operand()
    Ho, Wo = (H + 2 * p[0] - k[0]) // s[0] + 1, (W + 2 * p[1] - k[1]) // s[1] + 1
    op.ptr, op.layout = BASE, N.PATCH
    op.C, op.H, op.W, op.kh, op.kw, op.sh, op.sw, op.ph, op.pw, op.Ho, op.Wo = \
        C, H, W, k[0], k[1], s[0], s[1], p[0], p[1], Ho, Wo
    op.L, op.sB, op.rows, op.cols, op.has_ones = Ho * Wo, C * H * W, B * Ho * Wo, C * k[0] * k[1], int(bias)
    return _job(N, op, op.cols + int(bias)), None


def _channel(N, B, n, L, ones=False, bases=None):
    op = N.Operand()
    op.ptr, op.layout, op.cols, op.L, op.sB, op.rows, op.has_ones = BASE, N.CHANNEL, n, L, n * L, B * L, int(ones)
    job = _job(N, op, n + int(ones))
    keep = None
    if bases:
        keep = N.segment_table(bases)
        job.x.ptr, job.seg_ptrs, job.nseg = bases[0], N.table_ptr(keep), len(bases)
    return job, keep


def _bases(n, step=1 << 24):
    return [BASE + i * step for i in range(n)]


# name -> builder of [(job, keepalive)]
CASES = {
    # the MNIST MLP (C2) row-major group: one batch, and 15 queued batches with a ragged last one
    "c2": lambda N: [_rowmajor(N, 4096, c, o) for c, o in ((784, 1), (128, 1), (129, 0), (10, 0))],
    "c2_nseg15_ragged": lambda N: [_rowmajor(N, 4096, c, o, bases=_bases(15), last_rows=2656)
                                   for c, o in ((784, 1), (128, 1), (129, 0), (10, 0))],
    # the wide MLP (C5) group
    "c5": lambda N: [_rowmajor(N, 4096, c, o) for c, o in
                     ((784, 1), (4096, 0), (4096, 1), (4096, 0), (4096, 1), (10, 0))],
    "narrow_only": lambda N: [_rowmajor(N, 4096, c, o) for c, o in ((10, 0), (31, 1), (32, 0), (5, 1))],
    # a misaligned operand pointer: off the LDS-DMA path
    "rowmajor_misaligned": lambda N: [_rowmajor(N, 4096, 784, 1, ptr=BASE + 4)],
    # LeNet-5 at B = 1,024
    "lenet_conv1_A": lambda N: [_patch(N, 1024, 1, 28, 28, (5, 5), p=(2, 2))],
    "lenet_conv2_A": lambda N: [_patch(N, 1024, 6, 14, 14, (5, 5))],
    "lenet_conv1_G": lambda N: [_channel(N, 1024, 6, 784)],
    "lenet_conv2_G": lambda N: [_channel(N, 1024, 16, 100)],
    "lenet_all": lambda N: [_patch(N, 1024, 1, 28, 28, (5, 5), p=(2, 2)), _channel(N, 1024, 6, 784),
                            _patch(N, 1024, 6, 14, 14, (5, 5)), _channel(N, 1024, 16, 100),
                            _rowmajor(N, 1024, 400, 1), _rowmajor(N, 1024, 120, 0)],
    # one operand per remaining route (test_gpu_factors.test_conv_shapes_vs_oracle's specs)
    "conv_x3_51": lambda N: [_patch(N, 4, 2, 32, 32, (5, 5), p=(2, 2))],
    "conv_x3_stride2": lambda N: [_patch(N, 5, 4, 15, 15, (3, 3), s=(2, 2), p=(1, 1), bias=False)],
    "conv_x3_33": lambda N: [_patch(N, 3, 1, 20, 20, (4, 8))],
    "conv_x3_181": lambda N: [_patch(N, 2, 20, 10, 10, (3, 3))],
    "conv_fp32_n10": lambda N: [_patch(N, 4, 1, 10, 10, (3, 3), p=(1, 1))],
    "conv_fp32_n224": lambda N: [_patch(N, 2, 14, 9, 9, (4, 4), bias=False)],
    "conv_x3s_odd_groups": lambda N: [_patch(N, 2, 2, 5, 5, (3, 3))],
    "conv_col_stride3": lambda N: [_patch(N, 3, 3, 12, 17, (3, 3), s=(1, 3), p=(0, 1), bias=False)],
    "conv_image_too_large": lambda N: [_patch(N, 2, 3, 40, 40, (3, 3), p=(1, 1))],
    # the same routes at 4,096 images, where the planner's resident-workgroup count per
    # family (not the image count) sets the split
    "conv_x3_51_b4096": lambda N: [_patch(N, 4096, 2, 32, 32, (5, 5), p=(2, 2))],
    "conv_fp32_n10_b4096": lambda N: [_patch(N, 4096, 1, 10, 10, (3, 3), p=(1, 1))],
    "conv_fp32_n224_b4096": lambda N: [_patch(N, 4096, 14, 9, 9, (4, 4), bias=False)],
    "conv_col_stride3_b4096": lambda N: [_patch(N, 4096, 3, 12, 17, (3, 3), s=(1, 3), p=(0, 1), bias=False)],
    "conv_image_too_large_b64": lambda N: [_patch(N, 64, 3, 40, 40, (3, 3), p=(1, 1))],
    "channel_small_b16384": lambda N: [_channel(N, 16384, 6, 784)],
    "channel_L_not_x4": lambda N: [_channel(N, 2, 3, 9)],
    "channel_with_ones": lambda N: [_channel(N, 64, 6, 36, ones=True)],
    # multi-batch CHANNEL jobs: every base aligned, and one base 4 bytes off
    "channel_multibatch": lambda N: [_channel(N, 1024, 6, 784, bases=_bases(3))],
    "channel_multibatch_misaligned": lambda N: [
        _channel(N, 1024, 6, 784, bases=[BASE, BASE + (1 << 24) + 4, BASE + (2 << 24)])],
}

EXPECTED = {
    "c2": ([9, 9, 9, 9], [13418496, 884736, 884736, 147456], 15335424),
    "c2_nseg15_ragged": ([19, 19, 19, 19], [28327936, 1867776, 1867776, 311296], 32374784),
    "c5": ([3, 3, 3, 3, 3, 3], [4472832, 102236160, 105431040, 102236160, 105431040, 49152], 419856384),
    "narrow_only": ([16, 16, 16, 16], [262144, 262144, 262144, 262144], 1048576),
    "rowmajor_misaligned": ([11], [16400384], 16400384),
    "lenet_conv1_A": ([256], [4194304], 4194304),
    "lenet_conv2_A": ([256], [25165824], 25165824),
    "lenet_conv1_G": ([512], [8388608], 8388608),
    "lenet_conv2_G": ([1024], [16777216], 16777216),
    "lenet_all": ([256, 512, 256, 1024, 4, 4], [4194304, 8388608, 25165824, 16777216, 1835008, 196608], 25165824),
    "conv_x3_51": ([4], [65536], 65536),
    "conv_x3_stride2": ([5], [81920], 81920),
    "conv_x3_33": ([3], [49152], 49152),
    "conv_x3_181": ([2], [196608], 196608),
    "conv_fp32_n10": ([4], [65536], 65536),
    "conv_fp32_n224": ([2], [327680], 327680),
    "conv_x3s_odd_groups": ([2], [32768], 32768),
    "conv_col_stride3": ([3], [49152], 49152),
    "conv_image_too_large": ([13], [212992], 212992),
    "conv_x3_51_b4096": ([256], [4194304], 4194304),
    "conv_fp32_n10_b4096": ([1024], [16777216], 16777216),
    "conv_fp32_n224_b4096": ([256], [41943040], 41943040),
    "conv_col_stride3_b4096": ([1024], [16777216], 16777216),
    "conv_image_too_large_b64": ([400], [6553600], 6553600),
    "channel_small_b16384": ([1024], [16777216], 16777216),
    "channel_L_not_x4": ([1], [16384], 16384),
    "channel_with_ones": ([9], [147456], 147456),
    "channel_multibatch": ([512], [8388608], 8388608),
    "channel_multibatch_misaligned": ([1018], [16678912], 16678912),
}


# the kernel family (kfac_prof_id) each job's launch group is first routed to
# (kfac_factor_route): 0 tiles, 4 syrk3, 5 tiles_x3, 6 conv, 7 channel_small, 9 conv_x3,
# 10 conv_x3s, 11 conv_x3f, 12 channel_x3
ROUTES = {
    "c2": [0, 0, 0, 0],
    "c5": [4, 4, 4, 4, 4, 4],
    "lenet_all": [10, 7, 11, 12, 5, 5],
    "conv_x3_51": [9],
    "conv_fp32_n10": [6],
    "conv_fp32_n224": [6],
    "conv_x3s_odd_groups": [6],
    "conv_col_stride3": [6],
    "conv_image_too_large": [0],
    "channel_L_not_x4": [0],
    "channel_with_ones": [0],
    "channel_multibatch": [7],
    "channel_multibatch_misaligned": [0],
}


def measure(N, name):
    built = CASES[name](N)  # (the keepalives hold the host base tables until the calls return)
    jobs = [b[0] for b in built]
    arr = N.as_array(N.FactorJob, jobs)
    plan = N.factor_accum_plan(jobs)
    ws = N.lib().kfac_factor_workspace_bytes(arr, len(jobs))
    return [int(s) for s, _ in plan], [int(b) for _, b in plan], int(ws)


@pytest.mark.parametrize("name", list(CASES))
def test_plan_and_workspace_unchanged(name):
    from bnn_kfac_amd import _native as N
    splits, nbytes, ws = measure(N, name)
    print(name, splits, nbytes, ws)
    assert (splits, nbytes, ws) == EXPECTED[name]


@pytest.mark.parametrize("name", list(ROUTES))
def test_route_unchanged(name):
    from bnn_kfac_amd import _native as N
    built = CASES[name](N)
    assert N.factor_route([b[0] for b in built]) == ROUTES[name]
