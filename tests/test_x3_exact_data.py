"""Host: the term-exact inputs of tests/x3_exact.py are exact and sensitive, for every job
of every case test_gpu_x3_term_exact.py launches (the same table).

(a) mid is non-zero in more than 10 % of the live elements and lo in more than 5 %;
(b) the six-term factor round-trips through float32, and sum_K |x_i| |x_j| < 64 for every
    entry -- but ones x ones, the row count: an integer sum of hi hi = 1 terms below 2^24;
(c) an fp32 accumulation of the six terms, one K-row and term at a time in a shuffled
    order, equals the factor bit for bit;
(d) removing any one of the six terms changes at least one entry of EVERY 32 x 32 block of
    the factor, both triangles.  Two exemptions, both structural: a panel that holds the
    ones column alone (n = 257) has no mid or lo part to give, so the terms that take mid
    or lo from that panel are identically zero in its blocks for any input; and a job the
    launch computes on the fp32 MFMA (n <= 32 in a row-major group) carries no lo parts
    (x3_exact's docstring), so (a)'s lo share and (d)'s hi lo / lo hi do not apply to it."""
import numpy as np
import pytest

import x3_exact as X

JOBS = [(g.id, i) for g in X.GROUPS for i in range(g.njobs)]


def _job(gid, i):
    return X.GROUPS[X.GROUP_IDS.index(gid)].jobs[i]


def _block_counts(mask):
    starts = np.arange(0, mask.shape[0], 32)
    return np.add.reduceat(np.add.reduceat(mask.astype(np.int64), starts, 0), starts, 1)


@pytest.mark.parametrize("gid,i", JOBS, ids=[f"{g}-{i}" for g, i in JOBS])
def test_x3_exact_data(gid, i):
    job = _job(gid, i)
    h, m, l = job.parts
    x = h + m + l
    n, cols = job.n, job.n - job.ones
    F = job.want

    # (a) all three parts are there
    live = x[:, :cols] != 0
    assert live.sum() > 0
    assert (m[:, :cols] != 0).sum() > 0.10 * live.sum()
    if not job.fp32:
        assert (l[:, :cols] != 0).sum() > 0.05 * live.sum()
    else:
        assert not l.any()

    # (b) on the fp32 grid, every partial sum below 2^6
    assert np.array_equal(F.astype(np.float32).astype(np.float64), F)
    assert np.array_equal(np.mod(F, X.U18), np.zeros_like(F))
    bound = np.abs(x).T @ np.abs(x)
    if job.ones:
        assert bound[-1, -1] == x.shape[0] < 2 ** 24 and F[-1, -1] == x.shape[0]
        bound[-1, -1] = 0.0
    assert bound.max() < 64.0
    live_rows = live.any(1).sum() if job.layout != "patch" else live.sum(0).max()
    assert live_rows <= X.R  # (PATCH: live rows of any one im2col column)

    # (c) exact in a shuffled sequential fp32 sum
    got = X.sequential_fp32(job.parts, np.random.default_rng(n))
    np.testing.assert_array_equal(got, F.astype(np.float32))

    # (d) every term shows in every block
    nb = (n + 31) // 32
    lone_ones = np.zeros(nb, bool)  # panels that hold nothing but the ones column
    if job.ones and cols % 32 == 0:
        lone_ones[-1] = True
    for name, p, q in X.TERMS:
        if job.fp32 and 2 in (p, q):
            continue
        hit = _block_counts((job.parts[p].T @ job.parts[q]) != 0) > 0
        exempt = np.zeros((nb, nb), bool)
        if p != 0:
            exempt[lone_ones, :] = True
        if q != 0:
            exempt[:, lone_ones] = True
        missing = np.argwhere(~hit & ~exempt)
        assert missing.size == 0, f"term {name} leaves blocks {missing.tolist()} unchanged"
