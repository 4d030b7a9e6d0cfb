"""CPU: the host side of the class-tiled GLM predictive -- the C ABI of kfac_kron_cov_tiled /
kfac_kron_cov_outer_tiled (argument validation before any launch, workspace query, no class
cap) and the shape errors of variance.kron_covariance_tiled / kron_covariance_outer_tiled
on CPU tensors.  No GPU calls."""
import pytest
import torch


def _dense_job(N, nA=5, nG=3):
    # (pointers are never dereferenced on the host: validation happens before any launch)
    return N.CovJob(1 << 12, nA * nG, nA, nG, 1 << 13, nA, 1 << 14, nG, 1, 1)


def _outer_job(N, cols=4, has_ones=1, nG=3):
    return N.CovOuterJob(1 << 12, cols, cols, has_ones, 1 << 13, nG, nG, 0, 1 << 14, cols + has_ones,
                         1 << 15, nG, 1, 1)


DENSE_BAD = (("J", None), ("K1", None), ("K2", None), ("ldJ", 14), ("ld1", 4), ("ld2", 2), ("nA", 0),
             ("nA", -1), ("nG", 0), ("nG", -2))
OUTER_BAD = (("a", None), ("D", None), ("K1", None), ("K2", None), ("lda", 3), ("ldD", 2), ("ld1", 4),
             ("ld2", 2), ("cols", 0), ("cols", -1), ("nG", 0), ("nG", -2))


def _routes(N):
    lib = N.lib()
    return [(lib.kfac_kron_cov_tiled, lib.kfac_kron_cov_tiled_workspace_bytes, N.CovJob, _dense_job,
             DENSE_BAD),
            (lib.kfac_kron_cov_outer_tiled, lib.kfac_kron_cov_outer_tiled_workspace_bytes, N.CovOuterJob,
             _outer_job, OUTER_BAD)]


@pytest.mark.parametrize("route", [0, 1], ids=["dense", "outer"])
def test_tiled_validates_before_any_launch(route):
    from bnn_kfac_amd import _native as N
    call, _, struct, valid, bad_fields = _routes(N)[route]
    arr = N.as_array(struct, [valid(N)])
    out = 1 << 16
    for njobs in (0, 9, -1):
        assert call(arr, njobs, 2, 3, 0, out, None, 0, None) == N.KFAC_EINVAL, njobs
    for nb in (0, -4):
        assert call(arr, 1, nb, 3, 0, out, None, 0, None) == N.KFAC_EINVAL, nb
    for nc in (0, -1):
        assert call(arr, 1, 2, nc, 0, out, None, 0, None) == N.KFAC_EINVAL, nc
    assert call(None, 1, 2, 3, 0, out, None, 0, None) == N.KFAC_EINVAL
    assert call(arr, 1, 2, 3, 0, None, None, 0, None) == N.KFAC_EINVAL
    for field, value in bad_fields:
        bad = valid(N)
        setattr(bad, field, value)
        assert call(N.as_array(struct, [bad]), 1, 2, 3, 0, out, None, 0, None) == N.KFAC_EINVAL, field
        # the second job of two is validated too
        assert call(N.as_array(struct, [valid(N), bad]), 2, 2, 3, 0, out, None, 0,
                    None) == N.KFAC_EINVAL, field
    # nb*nc overflows 31 bits
    assert call(arr, 1, 1 << 30, 32, 0, out, None, 0, None) == N.KFAC_EINVAL
    assert call(arr, 1, 1 << 26, 33, 0, out, None, 0, None) == N.KFAC_EINVAL
    # nb*nc = 2e8 fits, the tile pairs x segments x samples of the Gram launch do not:
    # 1563 class tiles are 1 222 266 pairs, times 2000 samples
    assert call(arr, 1, 2000, 100000, 0, out, None, 0, None) == N.KFAC_EINVAL
    # a valid call with no workspace, and with one a byte short
    assert call(arr, 1, 2, 3, 0, out, None, 0, None) == N.KFAC_EWORKSPACE
    assert call(arr, 1, 2, 3, 0, out, None, 1 << 30, None) == N.KFAC_EWORKSPACE


def test_outer_tiled_ld1_follows_the_ones_column():
    from bnn_kfac_amd import _native as N
    call = N.lib().kfac_kron_cov_outer_tiled
    plain = _outer_job(N, has_ones=0)
    assert plain.ld1 == 4  # nA = cols: enough without the ones column, not with it
    assert call(N.as_array(N.CovOuterJob, [plain]), 1, 2, 3, 0, 1 << 16, None, 0, None) == N.KFAC_EWORKSPACE
    plain.has_ones = 1
    assert call(N.as_array(N.CovOuterJob, [plain]), 1, 2, 3, 0, 1 << 16, None, 0, None) == N.KFAC_EINVAL


@pytest.mark.parametrize("route", [0, 1], ids=["dense", "outer"])
@pytest.mark.parametrize("nc", [3, 32, 33, 65, 1000])
def test_tiled_has_no_class_cap(route, nc):
    """What tells the new entry points from the old: above 32 outputs the size query is
    non-zero and the call gets as far as asking for its workspace."""
    from bnn_kfac_amd import _native as N
    call, size, struct, valid, _ = _routes(N)[route]
    arr = N.as_array(struct, [valid(N)])
    need = size(arr, 1, 2, nc)
    assert need > 0
    assert call(arr, 1, 2, nc, 0, 1 << 16, None, 0, None) == N.KFAC_EWORKSPACE
    assert call(arr, 1, 2, nc, 0, 1 << 16, 1 << 17, need - 1, None) == N.KFAC_EWORKSPACE
    old = (N.lib().kfac_kron_cov_outer_workspace_bytes if route else N.lib().kfac_kron_cov_workspace_bytes)
    assert (old(arr, 1, 2, nc) > 0) == (nc <= 32)


@pytest.mark.parametrize("route", [0, 1], ids=["dense", "outer"])
def test_tiled_workspace_grows_with_nb_and_holds_the_partials(route):
    from bnn_kfac_amd import _native as N
    _, size, struct, valid, _ = _routes(N)[route]
    for p, nG in ((257, 100), (20, 2100)):
        arr = N.as_array(struct, [valid(N, p, nG) if route == 0 else valid(N, p, 1, nG)])
        K = p * nG if route == 0 else nG
        for nc in (10, 100, 130):
            sizes = [size(arr, 1, nb, nc) for nb in (1, 2, 8, 64)]
            assert sizes == sorted(set(sizes))
            ntile = -(-nc // 64)
            partial = (ntile * (ntile + 1) // 2) * -(-K // 2048) * 64 * 64 * 4
            rows = nc * K * 4 * (2 if route == 0 else 1)  # U and T, or V
            assert sizes[0] >= partial + rows
            assert sizes[3] >= 64 * (partial + rows)
    assert size(arr, 0, 4, 10) == 0
    assert size(None, 1, 4, 10) == 0
    assert size(arr, 1, 0, 10) == 0
    assert size(arr, 1, 4, 0) == 0
    assert size(arr, 1, 1 << 30, 32) == 0


def test_outer_tiled_needs_no_row_sized_scratch():
    from bnn_kfac_amd import _native as N
    lib = N.lib()
    outer = N.as_array(N.CovOuterJob, [_outer_job(N, 512, 1, 1000)])
    dense = N.as_array(N.CovJob, [_dense_job(N, 513, 1000)])
    assert (100 * lib.kfac_kron_cov_outer_tiled_workspace_bytes(outer, 1, 2, 1000)
            < lib.kfac_kron_cov_tiled_workspace_bytes(dense, 1, 2, 1000))


def test_python_shape_errors_before_any_device_call():
    """CPU tensors: a shape error is a ValueError raised before anything asks for a device."""
    from bnn_kfac_amd.variance import kron_covariance_outer_tiled, kron_covariance_tiled
    eye = torch.eye
    J = torch.zeros(2, 40, 20)
    with pytest.raises(ValueError, match="no terms"):
        kron_covariance_tiled([])
    with pytest.raises(ValueError):
        kron_covariance_tiled([(J, eye(5), eye(3))])           # 20 columns, kron needs 15
    with pytest.raises(ValueError):
        kron_covariance_tiled([(J, eye(5), torch.zeros(4, 3))])  # K2 not square
    with pytest.raises(ValueError):
        kron_covariance_tiled([(J, torch.zeros(5), eye(4))])     # K1 not a matrix
    with pytest.raises(ValueError):
        kron_covariance_tiled([(torch.zeros(2, 2, 40, 20), eye(5), eye(4))])  # J not (nb, nc, K)
    a, D = torch.zeros(2, 5), torch.zeros(2, 40, 4)
    with pytest.raises(ValueError, match="no terms"):
        kron_covariance_outer_tiled([])
    for nA in (4, 7):                                            # nA must be cols or cols + 1
        with pytest.raises(ValueError):
            kron_covariance_outer_tiled([(a, D, eye(nA), eye(4))])
    with pytest.raises(ValueError):
        kron_covariance_outer_tiled([(a[:1], D, eye(6), eye(4))])  # a has 1 row, D 2 samples
    with pytest.raises(ValueError):
        kron_covariance_outer_tiled([(a, D, eye(6), eye(3))])      # D has 4 columns, K2 is 3 x 3
    with pytest.raises(ValueError):
        kron_covariance_outer_tiled([(torch.zeros(2, 5, 1), D, eye(6), eye(4))])  # a not 2-D


def test_python_has_no_class_cap_but_no_cpu_fallback():
    """40 and 1000 outputs pass the shape checks (the capped siblings raise ValueError there)
    and stop at the device requirement."""
    from bnn_kfac_amd import _native as N
    from bnn_kfac_amd.variance import (kron_covariance, kron_covariance_outer, kron_covariance_outer_tiled,
                                       kron_covariance_tiled)
    for nc in (40, 1000):
        dense = [(torch.zeros(2, nc, 20), torch.eye(5), torch.eye(4))]
        outer = [(torch.zeros(2, 5), torch.zeros(2, nc, 4), torch.eye(6), torch.eye(4))]
        with pytest.raises(ValueError, match="at most 32"):
            kron_covariance(dense)
        with pytest.raises(ValueError, match="at most 32"):
            kron_covariance_outer(outer)
        with pytest.raises(N.NativeError):
            kron_covariance_tiled(dense)
        with pytest.raises(N.NativeError):
            kron_covariance_outer_tiled(outer)


def test_glm_predictive_routes_by_the_number_of_outputs():
    from bnn_kfac_amd import variance
    assert variance.MAX_COV_CLASSES == 32
    for nc in (1, 10, 32):
        assert variance._per_sample_calls(nc) == (variance.kron_covariance, variance.kron_covariance_outer)
    for nc in (33, 100, 1000):
        assert variance._per_sample_calls(nc) == (variance.kron_covariance_tiled,
                                                  variance.kron_covariance_outer_tiled)
