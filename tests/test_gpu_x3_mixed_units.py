"""GPU: kfac_factor_tiles_x3's mixed units (S3D3, P1D2) and its launch-wide split-major task
order through kfac_factor_update, the family asserted by its profile slot.  The method is
test_gpu_x3_cliques.py's (its Case and its launch helper are used as they are): small-integer
inputs, |x| <= 8, make every fp32 partial sum exact, so the factor equals the integer
reference bit for bit in both triangles; U[0, 1) and N(0, 1) inputs are held against fp64 at
|err| <= 1e-5 max|F|.

Factor orders: 129 (128 + ones: P = 5, the last panel the ones column alone), 133 (132 + ones:
the ones column inside a wider last panel), 160 (P = 5 without ones), 168 and 200 (P = 6 and
7, whatever mixed units the table forms there).  A group routes to kfac_factor_tiles_x3 only
when its largest factor has n >= 256, so every launch carries a 256-column job as well (P = 8,
whose table has mixed units too).  Shapes: those of test_gpu_x3_cliques.py.

The order: the MNIST MLP group (784 + ones, 128, 128 + ones, 10) over two batches of 1,024
rows plans 8 K-splits for every job -- one per XCD in the launch-wide order; over 1,024 +
1,024 + a ragged 600 rows, 11 (83 stages, 8 per split); with the jobs' accumulator splits
set to 8 and 4 by hand the split counts differ and the launch keeps the per-job order.  The
ragged batch's weight 1,024 / 600 is no dyadic number, so the reference of that case is the kernels' arithmetic
written out: the integer sums (exact) of each split's two waves -- wave w takes rows 16 w ..
16 w + 15 of every 32-row stage -- those of the ragged batch's splits times
float32(1,024 / 600), rounded once to fp32 (the ragged batch starts on a split boundary --
asserted -- so no task rescales its sums mid-way), the two waves added, then
kfac_factor_reduce's fixed order: part p = splits p, p + 4, ... summed in turn, parts
0 .. 3 added in turn."""
import numpy as np
import pytest
import torch

from test_gpu_x3_cliques import KINDS, SHAPES, Case, _draw, _gram, _run

pytestmark = pytest.mark.gpu

SIZES = [(128, True), (132, True), (160, False), (168, False), (200, False)]  # (cols, ones)
CARRIER = (256, False)
MLP = [(784, True), (128, False), (128, True), (10, False)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_mixed_units_grouped(hip_device, shape, kind):
    """The five factor orders and the carrier as the jobs of one launch."""
    from bnn_kfac_amd import _native as N
    rng = np.random.default_rng(1000 + SHAPES.index(shape) * 10 + KINDS.index(kind))
    cases = [Case(N, hip_device, rng, shape, kind, cols, ones) for cols, ones in SIZES + [CARRIER]]
    _run(N, hip_device, cases, shape == "deferred")
    for c in cases:
        c.check(kind)


@pytest.mark.parametrize("cols,ones", SIZES)
@pytest.mark.parametrize("shape", SHAPES)
def test_mixed_units_single_exact(hip_device, shape, cols, ones):
    """Each factor order with the carrier alone (its table second in the launch's), exact."""
    from bnn_kfac_amd import _native as N
    rng = np.random.default_rng(2000 + cols + SHAPES.index(shape))
    cases = [Case(N, hip_device, rng, shape, "int", c, o) for c, o in (CARRIER, (cols, ones))]
    _run(N, hip_device, cases, shape == "deferred")
    for c in cases:
        c.check("int")


@pytest.mark.parametrize("shape", ["ragged", "deferred"])
def test_mixed_units_deterministic(hip_device, shape):
    from bnn_kfac_amd import _native as N
    outs = []
    for _ in range(2):
        rng = np.random.default_rng(2999)
        cases = [Case(N, hip_device, rng, shape, "normal", cols, ones) for cols, ones in SIZES + [CARRIER]]
        _run(N, hip_device, cases, shape == "deferred")
        outs.append([c.F.cpu().numpy() for c in cases])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------ the task order
class MlpJob:
    """One job of the MLP group over batches of 1,024 rows (the last one `last` rows)."""

    def __init__(self, N, dev, rng, kind, cols, ones, nbatch, last):
        rows = 1024
        self.ones, self.n = ones, cols + ones
        self.xs = [_draw(rng, kind, rows if b < nbatch - 1 else last, cols) for b in range(nbatch)]
        self.bufs = []
        for x in self.xs:
            b = torch.full((rows, cols), float("nan"), device=dev)  # (rows past `last`: never read)
            b[:x.shape[0]].copy_(torch.from_numpy(x))
            self.bufs.append(b)
        self.table = N.segment_table([b.data_ptr() for b in self.bufs])
        op = N.rowmajor_operand(self.bufs[0], ones)
        if last != rows:
            op.last_rows = last
        self.F = torch.full((self.n, self.n), float("nan"), device=dev)
        self.job = N.factor_job(op, self.F, 1.0, 0.0)
        self.job.seg_ptrs, self.job.nseg = N.table_ptr(self.table), nbatch

    def want_plain(self):
        return sum(_gram(x, self.ones) for x in self.xs)

    def want_ragged(self, splits):
        """The kernels' arithmetic on integer inputs (module docstring), in fp32."""
        rows, last = 1024, self.xs[-1].shape[0]
        nst = 32 * (len(self.xs) - 1) + -(-last // 32)  # (the ragged batch: its own stages only)
        chunk = -(-nst // splits)
        rstage = 32 * (len(self.xs) - 1)
        assert rstage % chunk == 0, "the ragged batch starts on a split boundary"
        x = np.concatenate([np.concatenate([x, np.zeros((rows - x.shape[0], x.shape[1]), np.float32)]) for x in self.xs])
        valid = np.concatenate([np.arange(rows) < x.shape[0] for x in self.xs])
        rw = np.float32(np.float64(rows) / np.float64(last))
        half = (np.arange(len(x)) % 32) // 16  # the wave that takes a row (16-row halves of a stage)
        parts = []
        for s in range(splits):
            r0, r1 = min(s * chunk, nst) * 32, min((s + 1) * chunk, nst) * 32
            waves = []
            for w in range(2):
                xs = x[r0:r1][valid[r0:r1] & (half[r0:r1] == w)]
                g = _gram(xs, self.ones) if len(xs) else np.zeros((self.n, self.n))
                assert np.abs(g).max() < 2 ** 23
                if s * chunk >= rstage:
                    g = g * np.float64(rw)  # (24 x 24 bits: exact in fp64, rounded once below)
                waves.append(g.astype(np.float32))
            parts.append(waves[0] + waves[1])
        psum = []
        for p in range(4):
            acc = np.zeros((self.n, self.n), np.float32)
            for s in range(p, splits, 4):
                acc = acc + parts[s]
            psum.append(acc)
        return ((psum[0] + psum[1]) + psum[2]) + psum[3]


def _launch(N, dev, jobs, acc_splits=None):
    N.profile_reset()
    N.profile_enable(True)
    keep = []
    try:
        if acc_splits:
            flush = []
            for j, (splits, nbytes), mine in zip(jobs, N.factor_accum_plan([m.job for m in jobs]), acc_splits):
                assert nbytes % splits == 0  # (the plan's bytes are linear in the splits)
                acc = torch.empty(nbytes // splits * mine, dtype=torch.uint8, device=dev)
                keep.append(acc)
                j.job.acc, j.job.acc_splits, j.job.acc_beta = acc.data_ptr(), mine, 0.0
                f = N.FactorJob.from_buffer_copy(j.job)
                f.seg_ptrs, f.nseg = None, 0
                flush.append(f)
            N.factor_update([m.job for m in jobs], dev)
            N.factor_flush(flush, dev)
        else:
            N.factor_update([m.job for m in jobs], dev)
        torch.cuda.synchronize()
    finally:
        N.profile_enable(False)
    assert N.profile_read(N.PROF_FACTOR_X3)[1] == 1  # one kfac_factor_tiles_x3 launch
    assert N.profile_read(N.PROF_FACTOR_TILES)[1] == 0 and N.profile_read(N.PROF_FACTOR_SYRK3)[1] == 0


def _mlp(N, dev, seed, kind, nbatch, last):
    rng = np.random.default_rng(seed)
    return [MlpJob(N, dev, rng, kind, cols, ones, nbatch, last) for cols, ones in MLP]


def _splits(N, jobs):
    return [int(s) for s, _ in N.factor_accum_plan([m.job for m in jobs])]


def test_order_one_split_per_xcd(hip_device):
    """Two batches of 1,024 rows: 8 K-splits, 63 x 8 workgroups, XCD x the whole split x."""
    from bnn_kfac_amd import _native as N
    jobs = _mlp(N, hip_device, 3001, "int", 2, 1024)
    assert _splits(N, jobs) == [8] * 4
    _launch(N, hip_device, jobs)
    for m in jobs:
        np.testing.assert_array_equal(m.F.cpu().numpy(), m.want_plain().astype(np.float32), err_msg=f"n = {m.n}")


def test_order_ragged(hip_device):
    from bnn_kfac_amd import _native as N
    jobs = _mlp(N, hip_device, 3002, "int", 3, 600)
    splits = _splits(N, jobs)  # (uniform: the launch-wide order, 63 x 11 workgroups)
    assert splits == [11] * 4  # 64 + 19 stages, 8 per split
    _launch(N, hip_device, jobs)
    for m in jobs:
        np.testing.assert_array_equal(m.F.cpu().numpy(), m.want_ragged(11), err_msg=f"n = {m.n}")


def test_order_fallback_per_job(hip_device):
    """Accumulator splits 8 and 4 by hand: the split counts differ, the per-job order runs."""
    from bnn_kfac_amd import _native as N
    jobs = _mlp(N, hip_device, 3003, "int", 2, 1024)
    _launch(N, hip_device, jobs, acc_splits=[8, 4, 8, 4])
    for m in jobs:
        np.testing.assert_array_equal(m.F.cpu().numpy(), m.want_plain().astype(np.float32), err_msg=f"n = {m.n}")


def test_order_uniform_accumulators(hip_device):
    """The callers' accumulator splits all 8: the launch-wide order on the deferred path."""
    from bnn_kfac_amd import _native as N
    jobs = _mlp(N, hip_device, 3004, "int", 2, 1024)
    _launch(N, hip_device, jobs, acc_splits=[8, 8, 8, 8])
    for m in jobs:
        np.testing.assert_array_equal(m.F.cpu().numpy(), m.want_plain().astype(np.float32), err_msg=f"n = {m.n}")


@pytest.mark.parametrize("kind", ["uniform", "normal"])
@pytest.mark.parametrize("nbatch,last", [(2, 1024), (3, 600)])
def test_order_vs_fp64(hip_device, kind, nbatch, last):
    from bnn_kfac_amd import _native as N
    jobs = _mlp(N, hip_device, 3005 + nbatch, kind, nbatch, last)
    _launch(N, hip_device, jobs)
    for m in jobs:
        want = m.want_plain()
        if last != 1024:  # the ragged batch enters with its own per-batch mean's weight
            want = want + _gram(m.xs[-1], m.ones) * (1024.0 / last - 1.0)
        err = np.abs(m.F.cpu().numpy().astype(np.float64) - want).max()
        assert err <= 1e-5 * np.abs(want).max(), f"n = {m.n}: max error {err:.3e}"


def test_order_deterministic(hip_device):
    from bnn_kfac_amd import _native as N
    outs = []
    for _ in range(2):
        jobs = _mlp(N, hip_device, 3009, "normal", 3, 600)
        _launch(N, hip_device, jobs)
        outs.append([m.F.cpu().numpy() for m in jobs])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
