"""GPU: variance.glm_predictive_inf end to end on nets with 40 outputs (the class-tiled route:
kron_covariance_inf_tiled / kron_covariance_outer_inf_tiled), both `jacobians` routes,
chunk = 2, five inputs, on test_gpu_glm_wtiled_e2e.py's two nets.  INF is fitted by
test_gpu_glm_inf.py's _fit_inf, the reference is its _host_reference: J P^-1 J^T in fp64 from
`inf.state`, P inverted densely where nA*nG <= 600, through the fp64 Woodbury factors otherwise;
it asserts ||vtv||_2 <= VTV_MAX = 50 at ADD, MULTIPLY = 1.0, 100.0 in fp64 on the host.

Tolerance: glm_inf_tiled_cases.SCALE (rtol = SCALE, atol = SCALE * max|first term|)."""
import numpy as np
import pytest
import torch

import glm_inf_tiled_cases as T
import glm_sweep_cases as S
from test_gpu_glm_inf import ADD, MULTIPLY, _fit_inf, _host_reference
from test_gpu_glm_wtiled_e2e import N_TEST, NC, NETS

pytestmark = pytest.mark.gpu

BATCH = 64  # two KFAC batches: 128 samples for the 109 x 109 input factor of the conv net's head


@pytest.fixture(scope="module", params=list(NETS))
def fitted(request, hip_device):
    make, in_shape = NETS[request.param]
    torch.manual_seed(0)
    net, net64, inf = _fit_inf(hip_device, make(), in_shape, NC, BATCH)
    x = torch.rand(N_TEST, *in_shape, device=hip_device)
    layers = list(inf.state)
    layers64 = [m for m in list(net64.modules())[1:] if isinstance(m, (torch.nn.Linear, torch.nn.Conv2d))]
    assert len(layers) == len(layers64) == 2
    logits64, rows = S.fp64_rows(net64, layers64, x.cpu())
    return (net, inf, x, logits64) + _host_reference(inf, layers, rows)[:2]


@pytest.mark.parametrize("route", ["dense", "factored"])
def test_glm_predictive_inf_above_32_outputs(hip_device, fitted, route):
    from bnn_kfac_amd.variance import glm_predictive_inf
    net, inf, x, logits64, want, top = fitted
    before = {m: tuple(t.clone() for t in v) for m, v in inf.state.items()}
    logits, cov = glm_predictive_inf(inf, x, ADD, MULTIPLY, chunk=2, jacobians=route)   # needs no invert
    for m, v in inf.state.items():
        assert all(torch.equal(t, b) for t, b in zip(v, before[m]))
    assert logits.shape == (N_TEST, NC) and cov.shape == (N_TEST, NC, NC) and cov.dtype == torch.float32
    with torch.no_grad():
        direct = net(x).cpu().numpy()
    np.testing.assert_allclose(logits.cpu().numpy(), direct, rtol=1e-6, atol=1e-6 * np.abs(direct).max())
    np.testing.assert_allclose(logits.cpu().numpy(), logits64, rtol=1e-4, atol=1e-5 * np.abs(logits64).max())
    assert torch.equal(cov, cov.mT)
    got = cov.cpu().numpy()
    print("max err / max|first term| =", float(np.abs(got - want).max() / top), "of", T.SCALE)
    np.testing.assert_allclose(got, want, rtol=T.SCALE, atol=T.SCALE * top)
