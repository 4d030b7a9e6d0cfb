"""kfac_factor_tiles_x3's mixed units and its launch-wide task order, from the host (no GPU).

The table of P panels may take the pairs its cliques leave single together with diagonal
blocks: an S3D3 unit (a, b, c, h) owns the blocks (h, a), (h, b), (h, c) and the diagonal
blocks of a, b, c; a P1D2 unit (a, b) owns (b, a), (a, a) and (b, b).  P = 5 -- the MNIST
MLP's 129 -- is then three units where cliques and diagonal units alone took seven, the MLP
group has 63 units per K-split instead of 67, and the planner's one round of 1,024 slots
holds 16 splits instead of 15.  With every job at the same split count the launch is ordered
split-major across all jobs (kfac_x3_task_decode returns what the kernel computes for a
workgroup): every (job, unit, split) exactly once, and where 8 divides the split count every
XCD -- workgroup index mod 8 -- holds whole splits.

PARENT is the unit count per P of the tables before the mixed kinds (cliques and diagonal
units only), P = 2 .. 64."""
import ctypes

import numpy as np
import pytest

from test_factor_plan import _bases, _rowmajor
from test_x3_unit_table import unit_table

PARENT = [2, 2, 2, 7, 10, 13, 14, 16, 19, 16, 16, 17,
          34, 38, 39, 46, 50, 57, 65, 76, 77, 86, 97,
          57, 110, 119, 127, 132, 140, 146, 158, 163, 173, 181, 191, 200, 209,
          220, 227, 243, 255, 275, 284, 299, 310, 326, 343, 356, 376, 389,
          411, 426, 440, 459, 474, 495, 511, 530, 550, 571, 583, 604, 625]
assert len(PARENT) == 63

MLP = ((784, 1), (128, 0), (128, 1), (10, 0))  # (cols, ones): factor orders 785, 128, 129, 10


def test_p5_is_three_units():
    """A K4, the star of panel 4 with three diagonal blocks, the last pair with its two."""
    assert unit_table(5).tolist() == [[0, 1, 2, 3, 0b111111, 0],
                                      [0, 1, 2, 4, 0b110100, 0b0111],
                                      [3, 4, -1, -1, 0b000001, 0b0011]]


@pytest.mark.parametrize("P", range(2, 65))
def test_no_more_units_than_cliques_alone(P):
    n = len(unit_table(P))
    assert n <= PARENT[P - 2]
    if P in (4, 13, 25):
        assert n == PARENT[P - 2]


@pytest.mark.parametrize("P", range(2, 65))
def test_unit_shapes_and_order(P):
    """Every unit is one of the six kinds, the longest kinds first: K4 and S3D3, diagonal
    units, K3, P1D2, K2."""
    kinds = {(4, 63, 0): 0, (4, 0b110100, 0b0111): 0, (3, 0b001011, 0): 2, (2, 1, 0b0011): 3, (2, 1, 0): 4}
    rank = []
    for *panels, pmask, dmask in unit_table(P).tolist():
        np_ = sum(p >= 0 for p in panels)
        if pmask == 0:
            assert dmask == (1 << np_) - 1 and 1 <= np_ <= 4
            rank.append(1)
        else:
            rank.append(kinds[(np_, pmask, dmask)])
    assert rank == sorted(rank)


def _mlp_group(N, shape):
    if shape == "c2":  # 60,000 images at batch 4,096: 15 queued batches, the last one ragged
        return [_rowmajor(N, 4096, c, o, bases=_bases(15), last_rows=2656) for c, o in MLP]
    if shape == "c4_shard":
        return [_rowmajor(N, 8192, c, o, bases=_bases(8, step=1 << 25)) for c, o in MLP]
    return [_rowmajor(N, 4096, c, o) for c, o in MLP]


@pytest.mark.parametrize("shape", ["c2", "c4_shard", "one_batch"])
def test_mlp_group_takes_16_splits(shape):
    from bnn_kfac_amd import _native as N
    built = _mlp_group(N, shape)  # (the keepalives hold the base tables until the calls return)
    jobs = [b[0] for b in built]
    assert N.factor_route(jobs) == [N.PROF_FACTOR_X3] * 4
    assert [int(s) for s, _ in N.factor_accum_plan(jobs)] == [16] * 4


def _decode_all(N, units, splits):
    fn = N.lib().kfac_x3_task_decode
    u = (ctypes.c_int32 * len(units))(*units)
    blocks = sum(units) * splits
    out = np.full((blocks, 4), -7, dtype=np.int32)
    for b in range(blocks):
        row = out[b].ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        assert fn(u, len(units), splits, blocks, b, row) == N.KFAC_OK
    return out


@pytest.mark.parametrize("units,splits", [((57, 2, 3, 1), 16), ((57, 2, 3, 1), 8), ((57, 2, 3, 1), 15),
                                          ((57, 2, 3, 1), 1), ((17, 2), 4), ((3,), 5)])
def test_task_decode(units, splits):
    from bnn_kfac_amd import _native as N
    t = _decode_all(N, units, splits)
    blocks = len(t)
    assert t[:, 0].tolist() == [b % 8 for b in range(blocks)]
    want = {(j, u, s) for j, n in enumerate(units) for u in range(n) for s in range(splits)}
    got = [tuple(r) for r in t[:, 1:].tolist()]
    assert len(got) == len(want) and set(got) == want, "every (job, unit, split) exactly once"
    if splits % 8 == 0:
        per = splits // 8
        assert ((t[:, 3] >= t[:, 0] * per) & (t[:, 3] < (t[:, 0] + 1) * per)).all()
        # and every XCD the same mix: each unit of each job `per` times
        for x in range(8):
            mine = t[t[:, 0] == x]
            assert sorted(map(tuple, mine[:, 1:3].tolist())) == sorted(
                (j, u) for j, n in enumerate(units) for u in range(n) for _ in range(per))


def test_task_decode_arguments():
    from bnn_kfac_amd import _native as N
    fn = N.lib().kfac_x3_task_decode
    u = (ctypes.c_int32 * 2)(17, 2)
    out = (ctypes.c_int32 * 4)()
    assert fn(u, 2, 4, 76, 0, out) == N.KFAC_OK
    for args in ((None, 2, 4, 76, 0, out), (u, 2, 4, 76, 0, None), (u, 0, 4, 76, 0, out), (u, 17, 4, 76, 0, out),
                 (u, 2, 0, 76, 0, out), (u, 2, 4, 75, 0, out), (u, 2, 4, 76, 76, out), (u, 2, 4, 76, -1, out)):
        assert fn(*args) == N.KFAC_EINVAL
