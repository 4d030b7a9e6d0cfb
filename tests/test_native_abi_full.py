"""CPU: the C ABI of kfac_kron_cov_full and kfac_kron_cov_outer_full -- struct layouts
against the header, the workspace queries, and argument validation before any launch.
No GPU calls (pointers are never dereferenced on the host)."""
import ctypes

import pytest

from abi_layout import c_layout

DENSE_FIELDS = ("J", "ldJ", "nA", "nG", "VA", "ldA", "VG", "ldG", "W", "ldW")
OUTER_FIELDS = ("a", "lda", "cols", "has_ones", "D", "ldD", "nG", "reserved", "VA", "ldA", "VG", "ldG",
                "W", "ldW")


@pytest.mark.parametrize("cname,pyname,fields", [("kfac_cov_full_job", "CovFullJob", DENSE_FIELDS),
                                                 ("kfac_cov_outer_full_job", "CovOuterFullJob", OUTER_FIELDS)])
def test_full_struct_layout_matches_header(tmp_path, cname, pyname, fields):
    from bnn_kfac_amd import _native as N
    S = getattr(N, pyname)
    got = c_layout(tmp_path, cname, fields)
    assert [f for f, _ in S._fields_] == list(fields)
    assert got == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in fields]
    # the outer job starts like kfac_cov_outer_sweep_job: its first eight fields
    if pyname == "CovOuterFullJob":
        assert S._fields_[:8] == N.CovOuterSweepJob._fields_[:8]


def _dense_job(N, nA=5, nG=3):
    return N.CovFullJob(1 << 12, nA * nG, nA, nG, 1 << 13, nA, 1 << 14, nG, 1 << 15, nA * nG)


def _outer_job(N, cols=4, has_ones=1, nG=3):
    nA = cols + has_ones
    return N.CovOuterFullJob(1 << 12, cols, cols, has_ones, 1 << 13, nG, nG, 0, 1 << 14, nA, 1 << 15, nG,
                             1 << 16, nA * nG)


CASES = [("kfac_kron_cov_full", "CovFullJob", _dense_job,
          (("J", None), ("VA", None), ("VG", None), ("W", None), ("ldJ", 14), ("ldA", 4), ("ldG", 2),
           ("ldW", 14), ("nA", 0), ("nG", -1))),
         ("kfac_kron_cov_outer_full", "CovOuterFullJob", _outer_job,
          (("a", None), ("D", None), ("VA", None), ("VG", None), ("W", None), ("lda", 3), ("ldD", 2),
           ("ldA", 4), ("ldG", 2), ("ldW", 14), ("cols", 0), ("nG", 0)))]


@pytest.mark.parametrize("symbol,pyname,make,bad_fields", CASES, ids=["dense", "outer"])
def test_full_validates_before_any_launch(symbol, pyname, make, bad_fields):
    from bnn_kfac_amd import _native as N
    lib = N.lib()
    call = getattr(lib, symbol)
    query = getattr(lib, symbol + "_workspace_bytes")
    S = getattr(N, pyname)
    arr = N.as_array(S, [make(N)])
    out = 1 << 20
    # (jobs, njobs, nb, nc, nt, accumulate, cov, workspace, bytes, stream)
    for njobs, nb, nc, nt in ((0, 2, 3, 2), (9, 2, 3, 2), (-1, 2, 3, 2), (1, 0, 3, 2), (1, -4, 3, 2),
                              (1, 2, 0, 2), (1, 2, 33, 2), (1, 2, 3, 0), (1, 2, 3, 65), (1, 2, 3, -1)):
        assert call(arr, njobs, nb, nc, nt, 0, out, None, 0, None) == N.KFAC_EINVAL, (njobs, nb, nc, nt)
        assert query(arr, njobs, nb, nc, nt) == 0, (njobs, nb, nc, nt)
    nine = N.as_array(S, [make(N)] * 9)
    assert query(nine, 9, 2, 3, 2) == 0
    assert call(nine, 9, 2, 3, 2, 0, out, None, 0, None) == N.KFAC_EINVAL
    assert call(None, 1, 2, 3, 2, 0, out, None, 0, None) == N.KFAC_EINVAL
    assert call(arr, 1, 2, 3, 2, 0, None, None, 0, None) == N.KFAC_EINVAL
    for field, value in bad_fields:  # a null W and ldW < nA*nG = 15 among them
        bad = make(N)
        setattr(bad, field, value)
        assert call(N.as_array(S, [bad]), 1, 2, 3, 2, 0, out, None, 0, None) == N.KFAC_EINVAL, field
    bad = make(N)
    bad.W = None  # the second job of two is checked too
    assert call(N.as_array(S, [make(N), bad]), 2, 2, 3, 2, 0, out, None, 0, None) == N.KFAC_EINVAL
    # valid arguments: the workspace is checked next, still before any launch
    need = query(arr, 1, 2, 3, 2)
    assert need > 0
    assert call(arr, 1, 2, 3, 2, 0, out, None, 0, None) == N.KFAC_EWORKSPACE
    assert call(arr, 1, 2, 3, 2, 0, out, 1 << 21, need - 1, None) == N.KFAC_EWORKSPACE
    assert call(arr, 1, 2, 3, 64, 0, out, None, 0, None) == N.KFAC_EWORKSPACE  # nt = 64 is allowed
    wide = make(N)
    wide.ldW = 15 + 3  # ldW > nA*nG is allowed
    assert call(N.as_array(S, [wide]), 1, 2, 3, 2, 0, out, None, 0, None) == N.KFAC_EWORKSPACE


@pytest.mark.parametrize("symbol,pyname,make", [c[:3] for c in CASES], ids=["dense", "outer"])
def test_full_workspace_is_monotone_in_nb_and_nt(symbol, pyname, make):
    from bnn_kfac_amd import _native as N
    query = getattr(N.lib(), symbol + "_workspace_bytes")
    big = dict(nA=70, nG=65) if pyname == "CovFullJob" else dict(cols=130, nG=300)
    arr = N.as_array(getattr(N, pyname), [make(N, **big)])
    assert 0 < query(arr, 1, 4, 10, 1) < query(arr, 1, 4, 10, 2) < query(arr, 1, 4, 10, 64)
    assert query(arr, 1, 4, 10, 3) < query(arr, 1, 5, 10, 3) < query(arr, 1, 64, 10, 3)
    sizes = [query(arr, 1, nb, 10, 3) for nb in range(1, 70)]
    assert sizes == sorted(sizes)
    sizes = [query(arr, 1, 4, 10, nt) for nt in range(1, 65)]
    assert sizes == sorted(sizes)
    two = N.as_array(getattr(N, pyname), [make(N, **big), make(N)])
    assert query(two, 2, 4, 10, 3) > query(arr, 1, 4, 10, 3)


def test_wrappers_exist_for_every_new_symbol():
    from bnn_kfac_amd import _native as N
    for name in ("kron_cov_full", "kron_cov_full_workspace_bytes", "kron_cov_outer_full",
                 "kron_cov_outer_full_workspace_bytes"):
        assert callable(getattr(N, name)) and "kfac_" + name in N.SIGNATURES
