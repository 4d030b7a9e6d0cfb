"""kfac_factor_tiles_x3's panel-clique unit tables (no GPU): for every P the table is an
exact partition of the factor's lower triangle of 32 x 32 blocks -- every panel pair in
exactly one unit, every diagonal block in exactly one -- and deterministic; P = 25 (the
MNIST MLP's 785) is a Steiner system S(2, 4, 25)."""
import ctypes

import numpy as np
import pytest

PAIRS = ((1, 0), (2, 0), (3, 0), (2, 1), (3, 1), (3, 2))  # mask bit -> (row slot, column slot)


def unit_table(P):
    from bnn_kfac_amd import _native as N
    fn = N.lib().kfac_x3_unit_table
    n = fn(P, None, 0)
    out = np.full((n, 6), -7, dtype=np.int32)
    assert fn(P, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n) == n
    return out


@pytest.mark.parametrize("P", range(2, 65))
def test_exact_partition(P):
    t = unit_table(P)
    assert len(t) > 0
    pair = np.zeros((P, P), dtype=np.int64)
    diag = np.zeros(P, dtype=np.int64)
    for *panels, pmask, dmask in t.tolist():
        used = [p for p in panels if p >= 0]
        assert panels[:len(used)] == used, "unused slots come last"
        assert all(0 <= p < P for p in used)
        assert used == sorted(set(used)), "panels ascend, none twice"
        assert 0 <= pmask < 64 and 0 <= dmask < 16
        for bit, (i, j) in enumerate(PAIRS):
            if pmask >> bit & 1:
                assert i < len(used)
                pair[used[i], used[j]] += 1
        for s in range(4):
            if dmask >> s & 1:
                assert s < len(used)
                diag[used[s]] += 1
    want = np.tril(np.ones((P, P), dtype=np.int64), -1)
    np.testing.assert_array_equal(pair, want)
    np.testing.assert_array_equal(diag, np.ones(P, dtype=np.int64))


@pytest.mark.parametrize("P", [2, 4, 9, 25, 32, 64])
def test_deterministic(P):
    np.testing.assert_array_equal(unit_table(P), unit_table(P))


def test_out_of_range():
    from bnn_kfac_amd import _native as N
    fn = N.lib().kfac_x3_unit_table
    for P in (-1, 0, 1, 65, 1000):
        assert fn(P, None, 0) == 0


def test_p25_is_steiner():
    """50 four-panel units own the 300 off-diagonal blocks: 200 fragment splits per
    32-row stage (the 64 x 64 tile units took 300)."""
    t = unit_table(25)
    off = t[t[:, 4] != 0]
    assert len(off) == 50
    assert (off[:, :4] >= 0).all() and (off[:, 4] == 63).all() and (off[:, 5] == 0).all()
    assert int((off[:, :4] >= 0).sum()) <= 200
    assert sum(bin(m).count("1") for m in off[:, 4].tolist()) == 300
