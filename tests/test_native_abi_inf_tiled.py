"""CPU: the C ABI of the class-tiled INF covariance calls (kfac_inf_cov_tiled,
kfac_inf_cov_outer_tiled) -- argument validation before any launch, no class cap, and the
workspace queries against the layout the header documents.  No GPU calls (pointers are never
dereferenced on the host)."""
import pytest

from test_native_abi_inf import CASES as CAPPED_CASES

# (symbol, capped sibling, struct, valid job, bad fields): the capped calls' own ladders
CASES = [(symbol + "_tiled", symbol, pyname, make, bad) for symbol, pyname, make, bad in CAPPED_CASES]
IDS = ["dense", "outer"]


@pytest.mark.parametrize("symbol,capped,pyname,make,bad_fields", CASES, ids=IDS)
def test_validates_before_any_launch(symbol, capped, pyname, make, bad_fields):
    from bnn_kfac_amd import _native as N
    lib = N.lib()
    call, query = getattr(lib, symbol), getattr(lib, symbol + "_workspace_bytes")
    S = getattr(N, pyname)
    arr = N.as_array(S, [make(N)])
    out = 1 << 20
    # (jobs, njobs, nb, nc, accumulate, cov, workspace, bytes, stream)
    for njobs, nb, nc in ((0, 2, 40), (9, 2, 40), (-1, 2, 40), (1, 0, 40), (1, -4, 40), (1, 2, 0), (1, 2, -1)):
        assert call(arr, njobs, nb, nc, 0, out, None, 0, None) == N.KFAC_EINVAL, (njobs, nb, nc)
        assert query(arr, njobs, nb, nc) == 0, (njobs, nb, nc)
    nine = N.as_array(S, [make(N)] * 9)
    assert query(nine, 9, 2, 40) == 0
    assert call(nine, 9, 2, 40, 0, out, None, 0, None) == N.KFAC_EINVAL
    assert call(None, 1, 2, 40, 0, out, None, 0, None) == N.KFAC_EINVAL
    assert query(None, 1, 2, 40) == 0
    assert call(arr, 1, 2, 40, 0, None, None, 0, None) == N.KFAC_EINVAL          # null cov
    assert call(arr, 1, 2, 40, 0, None, 1 << 21, 1 << 30, None) == N.KFAC_EINVAL
    for field, value in bad_fields:
        bad = make(N)
        setattr(bad, field, value)
        assert call(N.as_array(S, [bad]), 1, 2, 40, 0, out, None, 0, None) == N.KFAC_EINVAL, field
        # ... even with a workspace that would do: EINVAL comes first
        assert call(N.as_array(S, [bad]), 1, 2, 40, 0, out, 1 << 21, 1 << 30, None) == N.KFAC_EINVAL, field
        # the second job of two is validated too
        assert call(N.as_array(S, [make(N), bad]), 2, 2, 40, 0, out, None, 0, None) == N.KFAC_EINVAL, field
    # nb*nc reaches 2^31: refused, not wrapped
    assert call(arr, 1, 1 << 30, 32, 0, out, 1 << 21, 1 << 62, None) == N.KFAC_EINVAL
    assert call(arr, 1, 1 << 26, 33, 0, out, 1 << 21, 1 << 62, None) == N.KFAC_EINVAL
    assert query(arr, 1, 1 << 30, 32) == 0 and query(arr, 1, 1 << 26, 33) == 0
    # nb*nc fits, the Gram launch's tasks (nb x 2 segments x 1563*1564/2 tile pairs) do not
    assert call(arr, 1, 2000, 100000, 0, out, 1 << 21, 1 << 62, None) == N.KFAC_EINVAL
    wide = make(N)
    wide.ldW, wide.ldF, wide.ldA, wide.ldG = 15 + 3, 4 + 1, 2 + 5, 2 + 1  # wider strides are allowed
    assert call(N.as_array(S, [wide]), 1, 2, 40, 0, out, None, 0, None) == N.KFAC_EWORKSPACE


@pytest.mark.parametrize("symbol,capped,pyname,make,bad_fields", CASES, ids=IDS)
@pytest.mark.parametrize("nc", [3, 32, 33, 40, 65, 1000])
def test_no_class_cap_and_a_short_workspace(symbol, capped, pyname, make, bad_fields, nc):
    """Above 32 outputs the size query is positive and the call gets as far as asking for its
    workspace; the capped sibling still rejects the same arguments."""
    from bnn_kfac_amd import _native as N
    lib = N.lib()
    call, query = getattr(lib, symbol), getattr(lib, symbol + "_workspace_bytes")
    arr = N.as_array(getattr(N, pyname), [make(N)])
    need = query(arr, 1, 2, nc)
    assert need > 0
    assert call(arr, 1, 2, nc, 0, 1 << 20, None, 0, None) == N.KFAC_EWORKSPACE
    assert call(arr, 1, 2, nc, 0, 1 << 20, None, need, None) == N.KFAC_EWORKSPACE
    assert call(arr, 1, 2, nc, 0, 1 << 20, 1 << 21, need - 1, None) == N.KFAC_EWORKSPACE
    old, old_query = getattr(lib, capped), getattr(lib, capped + "_workspace_bytes")
    assert (old_query(arr, 1, 2, nc) > 0) == (nc <= 32)
    assert old(arr, 1, 2, nc, 0, 1 << 20, None, 0, None) == (N.KFAC_EWORKSPACE if nc <= 32 else N.KFAC_EINVAL)


def _up(nbytes):
    return -(-nbytes // 256) * 256


def _partials(nb, nc, K):
    tiles = -(-nc // 64)
    return _up(nb * -(-K // 2048) * (tiles * (tiles + 1) // 2) * 64 * 64 * 4)


@pytest.mark.parametrize("nb,nc", [(2, 33), (3, 1000), (1, 130), (7, 32)])
def test_workspace_bytes_follow_the_documented_layout(nb, nc):
    """kfac_hip.h: per job, every part rounded up to 256 bytes."""
    from bnn_kfac_amd import _native as N
    from test_native_abi_inf import _dense_job, _outer_job
    lib = N.lib()
    rows = nb * nc
    dense = [(5, 3, 2, 2), (33, 65, 5, 7), (40, 70, 33, 63)]
    want = sum(_up(rows * ra * nG * 4) + 2 * _up(rows * ra * rg * 4) + _partials(nb, nc, nA * nG) +
               _partials(nb, nc, ra * rg) for nA, nG, ra, rg in dense)
    arr = N.as_array(N.InfCovJob, [_dense_job(N, *s) for s in dense])
    assert lib.kfac_inf_cov_tiled_workspace_bytes(arr, 3, nb, nc) == want
    outer = [(4, 1, 3, 2, 2), (3, 0, 2050, 2, 2), (40, 1, 70, 33, 63)]
    want = sum(_up(nb * (ra + 1) * nG * 4) + 2 * _up(rows * ra * rg * 4) + _partials(nb, nc, nG) +
               _partials(nb, nc, ra * rg) for _, _, nG, ra, rg in outer)
    arr = N.as_array(N.InfCovOuterJob, [_outer_job(N, *s) for s in outer])
    assert lib.kfac_inf_cov_outer_tiled_workspace_bytes(arr, 3, nb, nc) == want


@pytest.mark.parametrize("symbol,capped,pyname,make,bad_fields", CASES, ids=IDS)
def test_workspace_is_monotone_in_nb_and_additive_over_jobs(symbol, capped, pyname, make, bad_fields):
    from bnn_kfac_amd import _native as N
    query = getattr(N.lib(), symbol + "_workspace_bytes")
    big = dict(nA=70, nG=65, ra=9, rg=33) if pyname == "InfCovJob" else dict(cols=130, nG=300, ra=33, rg=9)
    S = getattr(N, pyname)
    arr = N.as_array(S, [make(N, **big)])
    sizes = [query(arr, 1, nb, 40) for nb in range(1, 70)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert query(arr, 1, 4, 64) < query(arr, 1, 4, 65)
    two = N.as_array(S, [make(N, **big), make(N)])
    assert query(two, 2, 4, 40) == query(arr, 1, 4, 40) + query(N.as_array(S, [make(N)]), 1, 4, 40)
    # the wrappers' queries are the same numbers
    wrapper = getattr(N, symbol[len("kfac_"):] + "_workspace_bytes")
    assert wrapper([make(N, **big)], 4, 40) == query(arr, 1, 4, 40)


def test_the_capped_calls_keep_their_cap():
    from bnn_kfac_amd import _native as N
    from test_native_abi_inf import _dense_job, _outer_job
    lib = N.lib()
    for symbol, S, make in (("kfac_inf_cov", N.InfCovJob, _dense_job), ("kfac_inf_cov_outer", N.InfCovOuterJob,
                                                                      _outer_job)):
        arr = N.as_array(S, [make(N)])
        assert getattr(lib, symbol)(arr, 1, 2, 33, 0, 1 << 20, 1 << 21, 1 << 30, None) == N.KFAC_EINVAL
        assert getattr(lib, symbol + "_workspace_bytes")(arr, 1, 2, 33) == 0


def test_wrappers_exist_for_every_new_symbol():
    from bnn_kfac_amd import _native as N
    for name in ("inf_cov_tiled", "inf_cov_tiled_workspace_bytes", "inf_cov_outer_tiled",
                 "inf_cov_outer_tiled_workspace_bytes"):
        assert callable(getattr(N, name)) and "kfac_" + name in N.SIGNATURES
        assert hasattr(N.lib(), "kfac_" + name)
