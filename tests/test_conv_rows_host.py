"""CPU: the integer cases of conv_rows_cases.py are exact and their int64 reference is
variance.conv_jacobian_rows; the ctypes struct mirrors the header; and every argument check
of kfac_cov_conv_rows returns KFAC_EINVAL before any launch, alone and as the second job
(dummy integers stand in for device pointers: nothing is dereferenced on the host)."""
import ctypes

import numpy as np
import pytest
import torch

import conv_rows_cases as R
from abi_layout import c_layout

FIELDS = ("x", "D", "ldD", "nG", "reserved", "M", "ldM")


@pytest.mark.parametrize("cid", R.IDS)
def test_partial_sums_are_exact(cid):
    c = R.case(cid)
    b = R.bound(c)
    print(f"{cid}: L {c.g.L}, largest partial sum {b}")
    assert b <= 4 * c.g.L <= 3136 < 2 ** 24
    assert np.abs(c.a).max() <= 2 and np.abs(c.D).max() <= 2
    assert np.abs(c.ref).max() <= b


def test_case_table():
    """The shapes the cases are there for."""
    g = {cid: R.case(cid).g for cid in R.IDS}
    assert (g["L1"].L, g["L1"].nA) == (1, 2)
    assert (g["lenet-conv1"].nA, g["lenet-conv1"].L, g["lenet-conv1"].nc * g["lenet-conv1"].nG) == (26, 784, 60)
    assert (g["lenet-conv2"].nA, g["lenet-conv2"].L, g["lenet-conv2"].nc * g["lenet-conv2"].nG) == (151, 100, 160)
    assert (g["nA64"].nA, g["nA64"].L, g["nA64"].nc * g["nA64"].nG) == (64, 30, 70) and g["nA64"].H != g["nA64"].W
    assert (g["nA65"].nA, g["nA65"].L, g["nA65"].nc) == (65, 4, 1)
    assert (g["stride2x1-nobias"].Ho, g["stride2x1-nobias"].Wo, g["stride2x1-nobias"].bias) == (6, 7, False)
    assert g["pad2"].ph == 2 and g["stride3-k2"].sh > g["stride3-k2"].kh
    assert (g["L33"].L, g["L65"].L, g["nb70"].nb, g["nc40"].nc) == (33, 65, 70, 40)
    for cid in R.IDS:
        c = R.case(cid)
        assert c.sB == c.g.C * c.g.H * c.g.W + 3 and c.ldD == c.g.nG * c.g.L + 5 and c.ldM == c.g.nA * c.g.nG + 7
        assert np.isnan(c.flat).sum() == np.isnan(c.want).sum() + c.ref.size


@pytest.mark.parametrize("cid", R.IDS)
def test_reference_is_conv_jacobian_rows(cid):
    """The int64 reference against the project's torch rows in fp64 (exact on this data)."""
    from bnn_kfac_amd.variance import conv_jacobian_rows
    c = R.case(cid)
    g = c.g
    layer = torch.nn.Conv2d(g.C, g.nG, (g.kh, g.kw), stride=(g.sh, g.sw), padding=(g.ph, g.pw), bias=g.bias)
    got = conv_jacobian_rows(layer, torch.from_numpy(np.array(c.a)).double(),
                             torch.from_numpy(np.array(c.D)).double())
    assert tuple(got.shape) == c.ref.shape
    np.testing.assert_array_equal(got.numpy(), c.ref.astype(np.float64))
    # and the slice-built unfold is F.unfold
    unf = torch.nn.functional.unfold(torch.from_numpy(np.array(c.a)).double(), (g.kh, g.kw),
                                     padding=(g.ph, g.pw), stride=(g.sh, g.sw))
    np.testing.assert_array_equal(unf.numpy(), R.unfold(c.a, g).astype(np.float64))


def test_struct_layout_matches_header(tmp_path):
    from bnn_kfac_amd import _native as N
    got = c_layout(tmp_path, "kfac_cov_conv_rows_job", FIELDS)
    assert [f for f, _ in N.CovConvRowsJob._fields_] == list(FIELDS)
    assert got == [ctypes.sizeof(N.CovConvRowsJob)] + [getattr(N.CovConvRowsJob, f).offset for f in FIELDS]


# ------------------------------------------------------------------ argument checks
NB, NC = 2, 3
A, D, M = 1 << 12, 1 << 16, 1 << 20  # never dereferenced: every call below returns before any launch
BASE = R.geometry((2, 4, 4, 3, 3, 1, 1, 1, 1, True, 3, NB, NC))  # Ho = Wo = 4, L = 16, cols = 18, nA = 19


def _job(N, nb=NB, x=None, **kw):
    """The valid job tests/test_gpu_conv_rows.py launches (conv_rows_cases.job), with
    fields of the operand (`x`) or of the job overwritten."""
    j = R.job(N, BASE, nb, A, D, M)
    for k, v in (x or {}).items():
        setattr(j.x, k, v)
    for k, v in kw.items():
        setattr(j, k, v)
    return j


def _bad_jobs(N):
    """(what, job) with exactly one violated requirement each."""
    bad = [("x.ptr NULL", _job(N, x={"ptr": None})), ("D NULL", _job(N, D=None)), ("M NULL", _job(N, M=None)),
           ("layout ROWMAJOR", _job(N, x={"layout": N.ROWMAJOR})), ("layout CHANNEL", _job(N, x={"layout": N.CHANNEL})),
           ("layout 7", _job(N, x={"layout": 7})),
           ("cols + 1", _job(N, x={"cols": BASE.cols + 1}, ldM=1 << 10)),
           ("cols - 1", _job(N, x={"cols": BASE.cols - 1})),
           ("L + 1", _job(N, x={"L": BASE.L + 1, "rows": NB * (BASE.L + 1)}, ldD=1 << 10)),
           ("L half", _job(N, x={"L": BASE.L // 2, "rows": NB * (BASE.L // 2)})),
           ("rows + 1", _job(N, x={"rows": NB * BASE.L + 1})),
           ("rows of another nb", _job(N, x={"rows": (NB + 1) * BASE.L})),
           ("nG 0", _job(N, nG=0)), ("nG -1", _job(N, nG=-1)),
           ("ldD short", _job(N, ldD=BASE.nG * BASE.L - 1)), ("ldD 0", _job(N, ldD=0)),
           ("ldM short", _job(N, ldM=BASE.nA * BASE.nG - 1)), ("ldM 0", _job(N, ldM=0)),
           ("ph -1", _job(N, x={"ph": -1})), ("pw -1", _job(N, x={"pw": -1}))]
    for f in ("C", "H", "W", "kh", "kw", "sh", "sw", "Ho", "Wo"):
        for v in (0, -1):
            bad.append((f"{f} {v}", _job(N, x={f: v})))
    # kh / kw at 2^15 with everything else consistent: padding that keeps the patches inside
    # the padded image, cols = C*kh*kw, ldM wide enough
    big = 1 << 15
    bad.append(("kh 2^15", _job(N, x={"kh": big, "ph": big // 2, "cols": BASE.C * big * 3}, ldM=1 << 40)))
    bad.append(("kw 2^15", _job(N, x={"kw": big, "pw": big // 2, "cols": BASE.C * 3 * big}, ldM=1 << 40)))
    # C*H*W = 2^31 with a consistent operand: Ho = Wo = 1024 for the 3x3 kernel with padding 1
    C, HW = 1 << 11, 1 << 10
    L = HW * HW
    bad.append(("C*H*W 2^31", _job(N, x={"C": C, "H": HW, "W": HW, "Ho": HW, "Wo": HW, "L": L, "rows": NB * L,
                                           "cols": C * 9, "sB": 1 << 31}, ldD=1 << 40, ldM=1 << 40)))
    # a sample stride below one image
    bad.append(("sB short", _job(N, x={"sB": BASE.C * BASE.H * BASE.W - 1})))
    # patches outside the padded image: an output size the geometry cannot give
    bad.append(("Ho too large", _job(N, x={"Ho": BASE.Ho + 1, "L": (BASE.Ho + 1) * BASE.Wo,
                                            "rows": NB * (BASE.Ho + 1) * BASE.Wo}, ldD=1 << 10)))
    return bad


def test_argument_checks_return_before_any_launch():
    from bnn_kfac_amd import _native as N
    call = N.lib().kfac_cov_conv_rows
    ok = N.as_array(N.CovConvRowsJob, [_job(N)] * 9)
    for njobs in (0, -1, 9):
        assert call(ok, njobs, NB, NC, None) == N.KFAC_EINVAL, njobs
    assert call(None, 1, NB, NC, None) == N.KFAC_EINVAL
    for nb in (0, -1):
        assert call(N.as_array(N.CovConvRowsJob, [_job(N, nb=nb)]), 1, nb, NC, None) == N.KFAC_EINVAL, nb
    for nc in (0, -1):
        assert call(ok, 1, NB, nc, None) == N.KFAC_EINVAL, nc
    for what, bad in _bad_jobs(N):
        assert call(N.as_array(N.CovConvRowsJob, [bad]), 1, NB, NC, None) == N.KFAC_EINVAL, what
        assert call(N.as_array(N.CovConvRowsJob, [_job(N), bad]), 2, NB, NC, None) == N.KFAC_EINVAL, (what, "second")


def test_task_count_of_2_31_is_refused():
    """nb = 2^30 samples of one a-tile and three column tiles (nc*nG = 192): 3 * 2^30 tasks.
    Alone, as the second job, and where only the sum over two jobs reaches 2^31."""
    from bnn_kfac_amd import _native as N
    call = N.lib().kfac_cov_conv_rows
    nb = 1 << 30
    one = _job(N, nb=nb)
    assert call(N.as_array(N.CovConvRowsJob, [one]), 1, nb, 64, None) == N.KFAC_EINVAL
    assert call(N.as_array(N.CovConvRowsJob, [one, one]), 2, nb, 64, None) == N.KFAC_EINVAL
    # nc = 3: one column tile, 2^30 tasks per job; two jobs make 2^31
    assert call(N.as_array(N.CovConvRowsJob, [one, one]), 2, nb, NC, None) == N.KFAC_EINVAL
    # nb itself at 2^31, and nc*nG at 2^31
    two31 = 1 << 31
    assert call(N.as_array(N.CovConvRowsJob, [_job(N, nb=two31)]), 1, two31, NC, None) == N.KFAC_EINVAL
    assert call(N.as_array(N.CovConvRowsJob, [_job(N)]), 1, NB, (1 << 31) // BASE.nG + 1, None) == N.KFAC_EINVAL


def test_python_surface():
    """The binding and the route helper exist, and the uncovered layers raise before the
    device is looked at."""
    from bnn_kfac_amd import _native as N
    from bnn_kfac_amd import variance as V
    assert "kfac_cov_conv_rows" in N.SIGNATURES and callable(N.cov_conv_rows)
    a, Dz = torch.zeros(2, 2, 6, 6), torch.zeros(2, 3, 2, 2, 2)
    for layer in (torch.nn.Conv2d(2, 2, 3, dilation=2), torch.nn.Conv2d(2, 2, 3, groups=2),
                  torch.nn.Conv2d(2, 2, 3, padding="same"), torch.nn.Conv2d(2, 2, 3, padding=1, padding_mode="reflect")):
        with pytest.raises(ValueError):
            V.conv_jacobian_rows_device(layer, a, Dz)
    # a covered layer on CPU tensors: no fallback
    with pytest.raises(N.NativeError):
        V.conv_jacobian_rows_device(torch.nn.Conv2d(2, 2, 3), torch.zeros(2, 2, 4, 4), torch.zeros(2, 3, 2, 2, 2))
