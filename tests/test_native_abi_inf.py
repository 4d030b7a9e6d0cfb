"""CPU: the C ABI of kfac_inf_cov and kfac_inf_cov_outer -- struct layouts against the
header, the workspace queries, and argument validation before any launch.  No GPU calls
(pointers are never dereferenced on the host)."""
import ctypes

import pytest

from abi_layout import c_layout

DENSE_FIELDS = ("J", "ldJ", "nA", "nG", "UA", "ldA", "ra", "UG", "ldG", "rg", "W", "ldW", "F", "ldF")
OUTER_FIELDS = ("a", "lda", "cols", "has_ones", "D", "ldD", "nG", "reserved", "UA", "ldA", "ra", "UG", "ldG",
                "rg", "W", "ldW", "F", "ldF")


@pytest.mark.parametrize("cname,pyname,fields", [("kfac_inf_cov_job", "InfCovJob", DENSE_FIELDS),
                                                 ("kfac_inf_cov_outer_job", "InfCovOuterJob", OUTER_FIELDS)])
def test_inf_struct_layout_matches_header(tmp_path, cname, pyname, fields):
    from bnn_kfac_amd import _native as N
    S = getattr(N, pyname)
    got = c_layout(tmp_path, cname, fields)
    assert [f for f, _ in S._fields_] == list(fields)
    assert got == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in fields]
    # the outer job starts like kfac_cov_outer_sweep_job: its first eight fields
    if pyname == "InfCovOuterJob":
        assert S._fields_[:8] == N.CovOuterSweepJob._fields_[:8]


def _dense_job(N, nA=5, nG=3, ra=2, rg=2):
    return N.InfCovJob(1 << 12, nA * nG, nA, nG, 1 << 13, ra, ra, 1 << 14, rg, rg, 1 << 15, nA * nG,
                       1 << 16, ra * rg)


def _outer_job(N, cols=4, has_ones=1, nG=3, ra=2, rg=2):
    nA = cols + has_ones
    return N.InfCovOuterJob(1 << 12, cols, cols, has_ones, 1 << 13, nG, nG, 0, 1 << 14, ra, ra, 1 << 15, rg, rg,
                            1 << 16, nA * nG, 1 << 17, ra * rg)


CASES = [("kfac_inf_cov", "InfCovJob", _dense_job,
          (("J", None), ("UA", None), ("UG", None), ("W", None), ("F", None), ("ldJ", 14), ("ldA", 1), ("ldG", 1),
           ("ldW", 14), ("ldF", 3), ("nA", 0), ("nG", -1), ("ra", 0), ("rg", -2))),
         ("kfac_inf_cov_outer", "InfCovOuterJob", _outer_job,
          (("a", None), ("D", None), ("UA", None), ("UG", None), ("W", None), ("F", None), ("lda", 3), ("ldD", 2),
           ("ldA", 1), ("ldG", 1), ("ldW", 14), ("ldF", 3), ("cols", 0), ("nG", 0), ("ra", 0), ("rg", -2)))]


@pytest.mark.parametrize("symbol,pyname,make,bad_fields", CASES, ids=["dense", "outer"])
def test_inf_validates_before_any_launch(symbol, pyname, make, bad_fields):
    """test_native_abi_full.py's ladder, without the grid-point count."""
    from bnn_kfac_amd import _native as N
    lib = N.lib()
    call = getattr(lib, symbol)
    query = getattr(lib, symbol + "_workspace_bytes")
    S = getattr(N, pyname)
    arr = N.as_array(S, [make(N)])
    out = 1 << 20
    # (jobs, njobs, nb, nc, accumulate, cov, workspace, bytes, stream)
    for njobs, nb, nc in ((0, 2, 3), (9, 2, 3), (-1, 2, 3), (1, 0, 3), (1, -4, 3), (1, 2, 0), (1, 2, 33),
                          (1, 2, -1)):
        assert call(arr, njobs, nb, nc, 0, out, None, 0, None) == N.KFAC_EINVAL, (njobs, nb, nc)
        assert query(arr, njobs, nb, nc) == 0, (njobs, nb, nc)
    nine = N.as_array(S, [make(N)] * 9)
    assert query(nine, 9, 2, 3) == 0
    assert call(nine, 9, 2, 3, 0, out, None, 0, None) == N.KFAC_EINVAL
    assert call(None, 1, 2, 3, 0, out, None, 0, None) == N.KFAC_EINVAL
    assert query(None, 1, 2, 3) == 0
    assert call(arr, 1, 2, 3, 0, None, None, 0, None) == N.KFAC_EINVAL
    for field, value in bad_fields:  # null W / F, ldW < nA*nG = 15 and ldF < r = 4 among them
        bad = make(N)
        setattr(bad, field, value)
        assert call(N.as_array(S, [bad]), 1, 2, 3, 0, out, None, 0, None) == N.KFAC_EINVAL, field
        # ... even with a workspace that would do: EINVAL comes first
        assert call(N.as_array(S, [bad]), 1, 2, 3, 0, out, 1 << 21, 1 << 30, None) == N.KFAC_EINVAL, field
    bad = make(N)
    bad.F = None  # the second job of two is checked too
    assert call(N.as_array(S, [make(N), bad]), 2, 2, 3, 0, out, None, 0, None) == N.KFAC_EINVAL
    # nb * nc reaching 2^31: refused, not wrapped
    assert call(arr, 1, (1 << 31) // 3 + 1, 3, 0, out, 1 << 21, 1 << 62, None) == N.KFAC_EINVAL
    # valid arguments: the workspace is checked next, still before any launch
    need = query(arr, 1, 2, 3)
    assert need > 0
    assert call(arr, 1, 2, 3, 0, out, None, 0, None) == N.KFAC_EWORKSPACE
    assert call(arr, 1, 2, 3, 0, out, None, need, None) == N.KFAC_EWORKSPACE
    assert call(arr, 1, 2, 3, 0, out, 1 << 21, need - 1, None) == N.KFAC_EWORKSPACE
    assert call(arr, 1, 2, 32, 0, out, None, 0, None) == N.KFAC_EWORKSPACE  # nc = 32 is allowed
    wide = make(N)
    wide.ldW, wide.ldF, wide.ldA, wide.ldG = 15 + 3, 4 + 1, 2 + 5, 2 + 1  # wider strides are allowed
    assert call(N.as_array(S, [wide]), 1, 2, 3, 0, out, None, 0, None) == N.KFAC_EWORKSPACE


@pytest.mark.parametrize("symbol,pyname,make", [c[:3] for c in CASES], ids=["dense", "outer"])
def test_inf_workspace_is_monotone_in_nb(symbol, pyname, make):
    from bnn_kfac_amd import _native as N
    query = getattr(N.lib(), symbol + "_workspace_bytes")
    big = dict(nA=70, nG=65, ra=9, rg=33) if pyname == "InfCovJob" else dict(cols=130, nG=300, ra=33, rg=9)
    arr = N.as_array(getattr(N, pyname), [make(N, **big)])
    assert 0 < query(arr, 1, 4, 10) < query(arr, 1, 5, 10) < query(arr, 1, 64, 10)
    sizes = [query(arr, 1, nb, 10) for nb in range(1, 70)]
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert query(arr, 1, 4, 10) < query(arr, 1, 4, 11)
    two = N.as_array(getattr(N, pyname), [make(N, **big), make(N)])
    assert query(two, 2, 4, 10) == query(arr, 1, 4, 10) + query(N.as_array(getattr(N, pyname), [make(N)]), 1, 4, 10)
    # the wrappers' queries are the same numbers
    wrapper = getattr(N, symbol[len("kfac_"):] + "_workspace_bytes")
    assert wrapper([make(N, **big)], 4, 10) == query(arr, 1, 4, 10)


def test_wrappers_exist_for_every_new_symbol():
    from bnn_kfac_amd import _native as N
    for name in ("inf_cov", "inf_cov_workspace_bytes", "inf_cov_outer", "inf_cov_outer_workspace_bytes"):
        assert callable(getattr(N, name)) and "kfac_" + name in N.SIGNATURES
        assert hasattr(N.lib(), "kfac_" + name)
