"""CPU: the C ABI of the class-tiled weighted covariance calls (kfac_kron_cov_full_tiled,
kfac_kron_cov_outer_full_tiled, kfac_kron_cov_sweep_tiled, kfac_kron_cov_outer_sweep_tiled) --
argument validation before any launch, no class cap, and the workspace queries against the
layout the header documents.  No GPU calls (pointers are never dereferenced on the host)."""
import pytest


def _full(N, nA=5, nG=3):
    return N.CovFullJob(1 << 12, nA * nG, nA, nG, 1 << 13, nA, 1 << 14, nG, 1 << 15, nA * nG)


def _outer_full(N, cols=4, has_ones=1, nG=3):
    nA = cols + has_ones
    return N.CovOuterFullJob(1 << 12, cols, cols, has_ones, 1 << 13, nG, nG, 0, 1 << 14, nA, 1 << 15, nG,
                             1 << 16, nA * nG)


def _sweep(N, nA=5, nG=3):
    return N.CovSweepJob(1 << 12, nA * nG, nA, nG, 1 << 13, nA, 1 << 14, nG, 1 << 15, nA, 1 << 16, nG)


def _outer_sweep(N, cols=4, has_ones=1, nG=3):
    nA = cols + has_ones
    return N.CovOuterSweepJob(1 << 12, cols, cols, has_ones, 1 << 13, nG, nG, 0, 1 << 14, nA, 1 << 15, nG,
                              1 << 16, nA, 1 << 17, nG)


DENSE_BAD = (("J", None), ("VA", None), ("VG", None), ("ldJ", 14), ("ldA", 4), ("ldG", 2), ("nA", 0), ("nG", -1))
OUTER_BAD = (("a", None), ("D", None), ("VA", None), ("VG", None), ("lda", 3), ("ldD", 2), ("ldA", 4),
             ("ldG", 2), ("cols", 0), ("nG", 0))
# (symbol, capped sibling, struct, valid job, bad fields)
CASES = [("kfac_kron_cov_full_tiled", "kfac_kron_cov_full", "CovFullJob", _full,
          DENSE_BAD + (("W", None), ("ldW", 14))),
         ("kfac_kron_cov_outer_full_tiled", "kfac_kron_cov_outer_full", "CovOuterFullJob", _outer_full,
          OUTER_BAD + (("W", None), ("ldW", 14))),
         ("kfac_kron_cov_sweep_tiled", "kfac_kron_cov_sweep", "CovSweepJob", _sweep,
          DENSE_BAD + (("wA", None), ("wG", None), ("ldwA", 4), ("ldwG", 2))),
         ("kfac_kron_cov_outer_sweep_tiled", "kfac_kron_cov_outer_sweep", "CovOuterSweepJob", _outer_sweep,
          OUTER_BAD + (("wA", None), ("wG", None), ("ldwA", 4), ("ldwG", 2)))]
CASE_IDS = ["full", "outer_full", "sweep", "outer_sweep"]


@pytest.mark.parametrize("symbol,capped,pyname,make,bad_fields", CASES, ids=CASE_IDS)
def test_validates_before_any_launch(symbol, capped, pyname, make, bad_fields):
    from bnn_kfac_amd import _native as N
    lib = N.lib()
    call, query = getattr(lib, symbol), getattr(lib, symbol + "_workspace_bytes")
    S = getattr(N, pyname)
    arr = N.as_array(S, [make(N)])
    out = 1 << 20
    # (jobs, njobs, nb, nc, nt, accumulate, cov, workspace, bytes, stream)
    for njobs, nb, nc, nt in ((0, 2, 3, 2), (9, 2, 3, 2), (-1, 2, 3, 2), (1, 0, 3, 2), (1, -4, 3, 2),
                              (1, 2, 0, 2), (1, 2, -1, 2), (1, 2, 40, 0), (1, 2, 40, 65), (1, 2, 40, -1)):
        assert call(arr, njobs, nb, nc, nt, 0, out, None, 0, None) == N.KFAC_EINVAL, (njobs, nb, nc, nt)
        assert query(arr, njobs, nb, nc, nt) == 0, (njobs, nb, nc, nt)
    nine = N.as_array(S, [make(N)] * 9)
    assert query(nine, 9, 2, 40, 2) == 0
    assert call(nine, 9, 2, 40, 2, 0, out, None, 0, None) == N.KFAC_EINVAL
    assert call(None, 1, 2, 40, 2, 0, out, None, 0, None) == N.KFAC_EINVAL
    assert call(arr, 1, 2, 40, 2, 0, None, None, 0, None) == N.KFAC_EINVAL
    assert query(None, 1, 2, 40, 2) == 0
    for field, value in bad_fields:
        bad = make(N)
        setattr(bad, field, value)
        assert call(N.as_array(S, [bad]), 1, 2, 40, 2, 0, out, None, 0, None) == N.KFAC_EINVAL, field
        # the second job of two is validated too
        assert call(N.as_array(S, [make(N), bad]), 2, 2, 40, 2, 0, out, None, 0, None) == N.KFAC_EINVAL, field
    # nb*nc overflows 31 bits; nb*nc fits but the Gram launch's tasks do not
    assert call(arr, 1, 1 << 30, 32, 2, 0, out, None, 0, None) == N.KFAC_EINVAL
    assert call(arr, 1, 1 << 26, 33, 2, 0, out, None, 0, None) == N.KFAC_EINVAL
    assert call(arr, 1, 2000, 100000, 1, 0, out, None, 0, None) == N.KFAC_EINVAL
    assert query(arr, 1, 1 << 30, 32, 2) == 0


@pytest.mark.parametrize("symbol,capped,pyname,make,bad_fields", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("nc", [3, 32, 33, 65, 1000])
def test_no_class_cap_and_a_short_workspace(symbol, capped, pyname, make, bad_fields, nc):
    """Above 32 outputs the size query is positive and the call gets as far as asking for its
    workspace; the capped sibling still rejects the same arguments."""
    from bnn_kfac_amd import _native as N
    lib = N.lib()
    call, query = getattr(lib, symbol), getattr(lib, symbol + "_workspace_bytes")
    arr = N.as_array(getattr(N, pyname), [make(N)])
    need = query(arr, 1, 2, nc, 2)
    assert need > 0
    assert call(arr, 1, 2, nc, 2, 0, 1 << 20, None, 0, None) == N.KFAC_EWORKSPACE
    assert call(arr, 1, 2, nc, 2, 0, 1 << 20, 1 << 21, need - 1, None) == N.KFAC_EWORKSPACE
    assert call(arr, 1, 2, nc, 64, 0, 1 << 20, None, 0, None) == N.KFAC_EWORKSPACE   # nt = 64 is allowed
    old, old_query = getattr(lib, capped), getattr(lib, capped + "_workspace_bytes")
    assert (old_query(arr, 1, 2, nc, 2) > 0) == (nc <= 32)
    assert old(arr, 1, 2, nc, 2, 0, 1 << 20, None, 0, None) == (N.KFAC_EWORKSPACE if nc <= 32 else N.KFAC_EINVAL)


def _up(nbytes):
    return -(-nbytes // 256) * 256


def _partials(nb, nc, nt, K):
    tiles = -(-nc // 64)
    return _up(nt * nb * -(-K // 2048) * (tiles * (tiles + 1) // 2) * 64 * 64 * 4)


@pytest.mark.parametrize("nb,nc,nt", [(2, 33, 1), (3, 1000, 5), (1, 130, 64), (7, 32, 2)])
def test_workspace_bytes_follow_the_documented_layout(nb, nc, nt):
    """kfac_hip.h: per job, every part rounded up to 256 bytes."""
    from bnn_kfac_amd import _native as N
    lib = N.lib()
    rows = nb * nc
    dense = [(5, 3), (33, 65), (20, 2100)]
    want = sum(2 * _up(rows * nA * nG * 4) + _partials(nb, nc, nt, nA * nG) for nA, nG in dense)
    arr = N.as_array(N.CovFullJob, [_full(N, *s) for s in dense])
    assert lib.kfac_kron_cov_full_tiled_workspace_bytes(arr, 3, nb, nc, nt) == want
    arr = N.as_array(N.CovSweepJob, [_sweep(N, *s) for s in dense])
    assert lib.kfac_kron_cov_sweep_tiled_workspace_bytes(arr, 3, nb, nc, nt) == want
    outer = [(4, 1, 3), (128, 0, 65), (20, 1, 2100)]
    want_full = want_sweep = 0
    for cols, ones, nG in outer:
        nA = cols + ones
        V, P = _up(rows * nG * 4), _partials(nb, nc, nt, nG)
        want_full += _up(nA * nb * 4) + _up(nt * nb * nG * 4) + V + P
        want_sweep += _up(nt * -(-nA // 64) * nb * 4) + V + P
    arr = N.as_array(N.CovOuterFullJob, [_outer_full(N, *s) for s in outer])
    assert lib.kfac_kron_cov_outer_full_tiled_workspace_bytes(arr, 3, nb, nc, nt) == want_full
    arr = N.as_array(N.CovOuterSweepJob, [_outer_sweep(N, *s) for s in outer])
    assert lib.kfac_kron_cov_outer_sweep_tiled_workspace_bytes(arr, 3, nb, nc, nt) == want_sweep


def test_wrappers_exist_for_every_new_symbol():
    from bnn_kfac_amd import _native as N
    for name in ("kron_cov_full_tiled", "kron_cov_outer_full_tiled", "kron_cov_sweep_tiled",
                 "kron_cov_outer_sweep_tiled"):
        for suffix in ("", "_workspace_bytes"):
            assert callable(getattr(N, name + suffix)) and "kfac_" + name + suffix in N.SIGNATURES
