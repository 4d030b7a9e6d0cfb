"""GPU: kfac_factor_tiles_x3's panel-clique units through kfac_factor_update, the family
asserted by its profile slot.

Factor orders 257, 320, 785, 1000 and 2045 -- P = 9, 10, 25, 32 and 64 panels of 32 columns:
a last panel of one column that is the ones column (257), the ones column inside a wider last
panel (785, 2045), the Steiner table (25) and the largest table (64).  (The kernel takes
operands with 16-byte rows only, cols % 4 == 0, so P = 64 is cols 2044 + ones = 2045: no
n = 2047 reaches it, with or without a ones column.)

Shapes: 96 rows in one batch; three batches of 64 rows whose ragged last batch has 40;
ld > cols; alpha != 1 with beta = 1 onto a non-zero F; once through the deferred
accumulators and the side reduce.

Small-integer inputs (|x| <= 8) make every fp32 partial sum exact, so the factor must equal
the integer reference bit for bit, in both triangles.  The ragged batch enters weighed
rows / last_rows = 1.6 (its own per-batch mean): its integer rows are multiples of 5, so
that weight gives integers too (1.6 x 25 m = 40 m, 1.6 x 5 m = 8 m against the ones column, 1.6 x 40 =
64 for the ones' own sum), the kernel's 0.625 rescale of the earlier batches is a division by 8
of a multiple of 5, and a product with float32(1.6) = 1.6 (1 + 1.5e-8) rounds to the integer
below 2^23.  The same shapes with U[0, 1) and N(0, 1) inputs are held against fp64 at
|err| <= 1e-5 max|F|.  (Integers bind the geometry through hi hi alone; test_gpu_x3_term_exact.py
binds the mid and lo products.)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [(256, True), (320, False), (784, True), (1000, False), (2044, True)]  # (cols, ones)
SHAPES = ["one_batch", "ragged", "ld", "alpha_beta", "deferred"]
KINDS = ["int", "uniform", "normal"]


def _draw(rng, kind, rows, cols, step=1):
    if kind == "int":
        lim = 8 // step
        return (rng.integers(-lim, lim + 1, size=(rows, cols)) * step).astype(np.float32)
    if kind == "uniform":
        return rng.random((rows, cols), dtype=np.float32)
    return rng.standard_normal((rows, cols)).astype(np.float32)


def _gram(x, ones):
    xo = np.concatenate([x, np.ones((x.shape[0], 1), np.float32)], 1) if ones else x
    xo = xo.astype(np.float64)
    return xo.T @ xo  # (integers: every sum far below 2^53, exact)


class Case:
    """One factor job of a shape, its device buffers and its fp64 reference."""

    def __init__(self, N, dev, rng, shape, kind, cols, ones):
        n = cols + ones
        self.n, self.keep = n, []
        alpha, beta = 1.0, 0.0
        F0 = np.full((n, n), np.nan, np.float32)
        if shape == "ragged":
            rows, last = 64, 40
            xs = [_draw(rng, kind, rows, cols), _draw(rng, kind, rows, cols), _draw(rng, kind, last, cols, step=5)]
            bufs = []
            for x in xs:
                b = torch.full((rows, cols), float("nan"), device=dev)  # (rows past last_rows: never read)
                b[:x.shape[0]].copy_(torch.from_numpy(x))
                bufs.append(b)
            table = N.segment_table([b.data_ptr() for b in bufs])
            self.keep += bufs + [table]
            op = N.rowmajor_operand(bufs[0], ones)
            op.last_rows = last
            g8 = _gram(xs[2], ones) * 8.0
            if kind == "int":
                assert np.all(np.mod(g8, 5.0) == 0.0)
            want = _gram(xs[0], ones) + _gram(xs[1], ones) + g8 / 5.0
        else:
            x = _draw(rng, kind, 96, cols)
            ld = cols + 4 if shape == "ld" else cols
            buf = torch.full((96, ld), float("nan"), device=dev)
            xd = buf[:, :cols]
            xd.copy_(torch.from_numpy(x))
            self.keep.append(buf)
            op = N.rowmajor_operand(xd, ones)
            assert op.ld == ld
            want = _gram(x, ones)
        if shape == "alpha_beta":
            alpha, beta = 0.5, 1.0
            F0 = rng.integers(-4, 5, size=(n, n)).astype(np.float32)
            F0 = F0 + F0.T
            want = F0.astype(np.float64) + 0.5 * want
        self.want = want
        self.F = torch.from_numpy(F0.copy()).to(dev)
        self.job = N.factor_job(op, self.F, alpha, beta)
        if shape == "ragged":
            self.job.seg_ptrs, self.job.nseg = N.table_ptr(table), 3

    def check(self, kind):
        got = self.F.cpu().numpy()
        if kind == "int":
            assert np.abs(self.want).max() < 2 ** 23
            np.testing.assert_array_equal(got, self.want.astype(np.float32), err_msg=f"n = {self.n}")
        else:
            bound = 1e-5 * np.abs(self.want).max()
            err = np.abs(got.astype(np.float64) - self.want).max()
            assert err <= bound, f"n = {self.n}: max error {err:.3e} > {bound:.3e}"


def _run(N, dev, cases, deferred):
    jobs = [c.job for c in cases]
    N.profile_reset()
    N.profile_enable(True)
    try:
        if deferred:
            accs, flush = [], []
            for job, (splits, nbytes) in zip(jobs, N.factor_accum_plan(jobs)):
                acc = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                accs.append(acc)
                job.acc, job.acc_splits, job.acc_beta = acc.data_ptr(), splits, 0.0
                f = N.FactorJob.from_buffer_copy(job)
                f.seg_ptrs, f.nseg = None, 0
                flush.append(f)
            N.factor_update(jobs, dev)
            N.factor_flush(flush, dev)
        else:
            N.factor_update(jobs, dev)
        torch.cuda.synchronize()
    finally:
        N.profile_enable(False)
    assert N.profile_read(N.PROF_FACTOR_X3)[1] == 1  # one kfac_factor_tiles_x3 launch
    assert N.profile_read(N.PROF_FACTOR_TILES)[1] == 0 and N.profile_read(N.PROF_FACTOR_SYRK3)[1] == 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_clique_units_grouped(hip_device, shape, kind):
    """The five factor orders as the jobs of one launch (five unit tables side by side)."""
    from bnn_kfac_amd import _native as N
    rng = np.random.default_rng(SHAPES.index(shape) * 10 + KINDS.index(kind))
    cases = [Case(N, hip_device, rng, shape, kind, cols, ones) for cols, ones in SIZES]
    _run(N, hip_device, cases, shape == "deferred")
    for c in cases:
        c.check(kind)


@pytest.mark.parametrize("cols,ones", SIZES)
@pytest.mark.parametrize("shape", SHAPES)
def test_clique_units_single_exact(hip_device, shape, cols, ones):
    """Each factor order as a launch of its own (its table at entry 0), exact on integers."""
    from bnn_kfac_amd import _native as N
    rng = np.random.default_rng(cols + SHAPES.index(shape))
    case = Case(N, hip_device, rng, shape, "int", cols, ones)
    _run(N, hip_device, [case], shape == "deferred")
    case.check("int")


@pytest.mark.parametrize("shape", ["ragged", "deferred"])
def test_clique_units_deterministic(hip_device, shape):
    """Two runs of one call are bit-identical (the two waves' hand-off and the reduce)."""
    from bnn_kfac_amd import _native as N
    outs = []
    for _ in range(2):
        rng = np.random.default_rng(99)
        cases = [Case(N, hip_device, rng, shape, "normal", cols, ones) for cols, ones in SIZES]
        _run(N, hip_device, cases, shape == "deferred")
        outs.append([c.F.cpu().numpy() for c in cases])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
