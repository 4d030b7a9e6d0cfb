"""CPU: the host side of the factored GLM predictive -- the C ABI of kfac_kron_cov_outer
(struct layout, argument validation before any launch, workspace query) and
variance.layer_io_jacobians against the dense output_jacobians rows in fp64.  No GPU
calls."""
import ctypes

import pytest
import torch
import torch.nn as nn

from abi_layout import c_layout

FIELDS = ("a", "lda", "cols", "has_ones", "D", "ldD", "nG", "reserved", "K1", "ld1", "K2", "ld2",
          "lower1", "lower2")


def test_cov_outer_struct_layout(tmp_path):
    from bnn_kfac_amd import _native as N
    got = c_layout(tmp_path, "kfac_cov_outer_job", FIELDS)
    assert [f for f, _ in N.CovOuterJob._fields_] == list(FIELDS)
    assert got == [ctypes.sizeof(N.CovOuterJob)] + [getattr(N.CovOuterJob, f).offset for f in FIELDS]


def _valid_job(N, cols=4, has_ones=1, nG=3):
    # (pointers are never dereferenced on the host: validation happens before any launch)
    return N.CovOuterJob(1 << 12, cols, cols, has_ones, 1 << 13, nG, nG, 0, 1 << 14, cols + has_ones,
                         1 << 15, nG, 1, 1)


def test_kron_cov_outer_validates_before_any_launch():
    from bnn_kfac_amd import _native as N
    lib = N.lib()
    call = lib.kfac_kron_cov_outer
    arr = N.as_array(N.CovOuterJob, [_valid_job(N)])
    out = 1 << 16
    assert call(arr, 0, 2, 3, 0, out, None, 0, None) == N.KFAC_EINVAL
    assert call(arr, 9, 2, 3, 0, out, None, 0, None) == N.KFAC_EINVAL
    assert call(arr, -1, 2, 3, 0, out, None, 0, None) == N.KFAC_EINVAL
    assert call(arr, 1, 2, 0, 0, out, None, 0, None) == N.KFAC_EINVAL
    assert call(arr, 1, 2, 33, 0, out, None, 0, None) == N.KFAC_EINVAL
    assert call(arr, 1, 0, 3, 0, out, None, 0, None) == N.KFAC_EINVAL
    assert call(arr, 1, -4, 3, 0, out, None, 0, None) == N.KFAC_EINVAL
    assert call(None, 1, 2, 3, 0, out, None, 0, None) == N.KFAC_EINVAL
    assert call(arr, 1, 2, 3, 0, None, None, 0, None) == N.KFAC_EINVAL
    for field, value in (("a", None), ("D", None), ("K1", None), ("K2", None), ("lda", 3), ("ldD", 2),
                         ("ld1", 4), ("ld2", 2), ("cols", 0), ("cols", -1), ("nG", 0), ("nG", -2)):
        bad = _valid_job(N)
        setattr(bad, field, value)
        assert call(N.as_array(N.CovOuterJob, [bad]), 1, 2, 3, 0, out, None, 0, None) == N.KFAC_EINVAL, field
    # without the ones column nA = cols: ld1 = cols is enough, with it it is not
    plain = _valid_job(N, has_ones=0)
    assert plain.ld1 == 4
    assert call(N.as_array(N.CovOuterJob, [plain]), 1, 2, 3, 0, out, None, 0, None) == N.KFAC_EWORKSPACE
    # the second job of two is validated too
    bad = _valid_job(N)
    bad.ldD = 2
    assert call(N.as_array(N.CovOuterJob, [_valid_job(N), bad]), 2, 2, 3, 0, out, None, 0,
                None) == N.KFAC_EINVAL
    # more than 2^31 tasks
    assert call(arr, 1, 1 << 30, 32, 0, out, None, 0, None) == N.KFAC_EINVAL
    # a valid job with no workspace, and with one a byte short
    assert call(arr, 1, 2, 3, 0, out, None, 0, None) == N.KFAC_EWORKSPACE
    need = lib.kfac_kron_cov_outer_workspace_bytes(arr, 1, 2, 3)
    assert need > 0
    assert call(arr, 1, 2, 3, 0, out, 1 << 17, need - 1, None) == N.KFAC_EWORKSPACE


def test_kron_cov_outer_workspace():
    from bnn_kfac_amd import _native as N
    lib = N.lib()
    for cols, nG in ((784, 128), (19, 130), (4096, 4096)):
        arr = N.as_array(N.CovOuterJob, [_valid_job(N, cols, 1, nG)])
        sizes = [lib.kfac_kron_cov_outer_workspace_bytes(arr, 1, nb, 10) for nb in (1, 2, 8, 64)]
        assert sizes == sorted(set(sizes))
        assert sizes[0] >= 10 * nG * 4  # at least V for every row
    assert lib.kfac_kron_cov_outer_workspace_bytes(arr, 0, 4, 10) == 0
    # the point of the feature: no Jacobian-row-sized scratch
    outer = N.as_array(N.CovOuterJob, [_valid_job(N, 784, 1, 128)])
    dense = N.as_array(N.CovJob, [N.CovJob(1 << 12, 785 * 128, 785, 128, 1 << 13, 785, 1 << 14, 128, 1, 1)])
    assert (100 * lib.kfac_kron_cov_outer_workspace_bytes(outer, 1, 64, 10)
            < lib.kfac_kron_cov_workspace_bytes(dense, 1, 64, 10))


def _models():
    from models_for_tests import BaseNet750
    return {
        "mlp_nobias": (lambda: nn.Sequential(nn.Linear(12, 7, bias=False), nn.Tanh(), nn.Linear(7, 3)), (12,)),
        "relu_inplace": (lambda: nn.Sequential(nn.Linear(9, 6), nn.ReLU(inplace=True), nn.Linear(6, 5),
                                               nn.ReLU(inplace=True), nn.Linear(5, 4)), (9,)),
        "basenet750": (BaseNet750, (1, 28, 28)),
    }


@pytest.mark.parametrize("name", ["mlp_nobias", "relu_inplace", "basenet750"])
def test_layer_io_jacobians_match_dense_rows(name):
    from bnn_kfac_amd.variance import conv_jacobian_rows, layer_io_jacobians, output_jacobians
    make, xshape = _models()[name]
    torch.manual_seed(0)
    net = make().double()
    layers = [m for m in net.modules() if isinstance(m, (nn.Linear, nn.Conv2d))]
    x = torch.randn(4, *xshape, dtype=torch.float64)
    want_logits, Js = output_jacobians(net, layers, x)
    logits, io = layer_io_jacobians(net, layers, x)
    with torch.no_grad():
        direct = net(x)
    torch.testing.assert_close(logits, direct, rtol=1e-10, atol=0)
    torch.testing.assert_close(logits, want_logits, rtol=1e-10, atol=0)
    nc = direct.shape[1]
    assert len(io) == len(layers)
    for layer, J, (a, D) in zip(layers, Js, io):
        assert D.is_contiguous() and D.shape[:2] == (4, nc) and not D.requires_grad
        assert float(J.abs().max()) > 0
        atol = 1e-10 * float(J.abs().max())
        if isinstance(layer, nn.Linear):
            assert a.shape == (4, layer.in_features) and D.shape == (4, nc, layer.out_features)
            abar = torch.cat([a, torch.ones(4, 1, dtype=a.dtype)], dim=1) if layer.bias is not None else a
            rows = torch.einsum("ba,bcg->bcag", abar, D).reshape(4, nc, -1)
        else:
            rows = conv_jacobian_rows(layer, a, D)
        assert rows.shape == J.shape
        torch.testing.assert_close(rows, J, rtol=1e-10, atol=atol)


def test_layer_io_jacobians_restore_model_hooks():
    from bnn_kfac_amd.curvatures import KFAC
    from bnn_kfac_amd.variance import layer_io_jacobians
    torch.manual_seed(0)
    net = nn.Sequential(nn.Linear(9, 6), nn.ReLU(inplace=True), nn.Linear(6, 4))
    kfac = KFAC(net)
    layers = [net[0], net[2]]
    hooks = [(dict(m._forward_hooks), dict(m._forward_pre_hooks)) for m in layers]
    layer_io_jacobians(net, layers, torch.randn(3, 9))
    assert [(dict(m._forward_hooks), dict(m._forward_pre_hooks)) for m in layers] == hooks
    assert all(kfac.record[m] == [None, None] for m in layers)  # nothing recorded while suspended
    x = torch.randn(5, 9)
    net(x).sum().backward()
    for m in layers:
        forward, backward = kfac.record[m]
        assert forward is not None and backward is not None
        assert forward.shape[0] == 5 and backward.shape == (5, m.out_features)
    assert kfac.record[net[0]][0] is x


def test_glm_predictive_rejects_unknown_route():
    from bnn_kfac_amd.variance import glm_predictive

    class Stub:
        model = nn.Linear(2, 2)
        state = {}
        inv_state = {}

    with pytest.raises(ValueError):
        glm_predictive(Stub(), torch.zeros(1, 2), jacobians="nope")
