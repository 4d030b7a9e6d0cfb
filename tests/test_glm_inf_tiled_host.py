"""CPU: the host side of the class-tiled INF GLM predictive -- the recorded fp32-chain error
behind the GPU tolerance on the tiled shapes, the ValueErrors that fire before any device call,
and which pair of calls _inf_chunk / glm_predictive_inf take at 32 and at 33 outputs."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import glm_inf_cases as C
import glm_inf_tiled_cases as T


def test_recorded_fp32_chain_error_and_scale():
    """The GPU tolerance's record: the stage chain in numpy fp32 on every tiled shape."""
    errors = T.fp32_chain_errors()
    for key, err in errors.items():
        print(key, "fp32 chain err / max|first term| =", err)
    worst = max(errors.values())
    print("worst", worst, "recorded", T.MEASURED_FP32_CHAIN)
    assert worst <= 2 * T.MEASURED_FP32_CHAIN          # (BLAS summation orders differ by machine)
    assert T.SCALE == max(1e-5, 4 * T.MEASURED_FP32_CHAIN) == C.SCALE and 4 * worst <= T.SCALE


def test_case_shapes_reach_their_edges():
    for shape in T.OUTER_SHAPES:
        *_, ref, top = C.outer_case(*shape)
        assert ref.shape == (shape[5], shape[6], shape[6]) and shape[6] > 32 and top <= 10 * np.abs(ref).max()
    for shape in T.DENSE_SHAPES:
        *_, ref, top = C.dense_case(*shape)
        assert ref.shape == (shape[4], shape[5], shape[5]) and shape[5] > 32 and top <= 10 * np.abs(ref).max()
    seg = 2048
    assert any(s[2] > seg for s in T.OUTER_SHAPES) and any(s[3] * s[4] > seg for s in T.OUTER_SHAPES)
    assert any(s[0] * s[1] > seg for s in T.DENSE_SHAPES) and any(s[2] * s[3] > seg for s in T.DENSE_SHAPES)
    assert {-(-s[6] // 64) for s in T.OUTER_SHAPES} == {1, 2, 3} == {-(-s[5] // 64) for s in T.DENSE_SHAPES}
    for kw in T.INT_OUTER:
        *_, want, bound = C.int_outer_case(**kw)
        assert want.shape == (kw["nb"], kw["nc"], kw["nc"]) and 0 < bound <= C.EXACT
    for kw in T.INT_DENSE:
        J, *_, want, bound = C.int_dense_case(**kw)
        assert J.shape[2] > seg and want.shape == (kw["nb"], kw["nc"], kw["nc"]) and 0 < bound <= 67123


def test_value_errors_fire_before_any_device_call():
    """test_glm_inf_host.py's list on the tiled functions: the same shape checks, no cap."""
    from bnn_kfac_amd._native import NativeError
    from bnn_kfac_amd.variance import (kron_covariance_inf, kron_covariance_inf_tiled, kron_covariance_outer_inf,
                                       kron_covariance_outer_inf_tiled)
    nA, nG, ra, rg, nb, nc = 6, 4, 3, 2, 2, 40
    r = ra * rg
    J, a, D = torch.zeros(nb, nc, nA * nG), torch.zeros(nb, nA - 1), torch.zeros(nb, nc, nG)
    UA, UG, W, F = torch.ones(nA, ra), torch.ones(nG, rg), torch.ones(nA, nG), torch.eye(r)
    bad = [dict(W=torch.ones(nG, nA)), dict(W=torch.ones(nA * nG)), dict(W=torch.ones(1, nA, nG)),
           dict(F=torch.eye(r + 1)), dict(F=torch.ones(r)), dict(F=torch.ones(r, r - 1)),
           dict(UA=torch.ones(nA)), dict(UG=torch.ones(nG, 0)), dict(UA=torch.ones(nA + 2, ra))]
    for change in bad:
        ops = {**dict(UA=UA, UG=UG, W=W, F=F), **change}
        with pytest.raises(ValueError):
            kron_covariance_inf_tiled([(J, ops["UA"], ops["UG"], ops["W"], ops["F"])])
        with pytest.raises(ValueError):
            kron_covariance_outer_inf_tiled([(a, D, ops["UA"], ops["UG"], ops["W"], ops["F"])])
    for fn in (kron_covariance_inf_tiled, kron_covariance_outer_inf_tiled):
        with pytest.raises(ValueError, match="no terms"):
            fn([])
    with pytest.raises(ValueError):
        kron_covariance_inf_tiled([(J[:, :, :-1], UA, UG, W, F)])
    with pytest.raises(ValueError, match="same"):
        kron_covariance_inf_tiled([(J, UA, UG, W, F), (J[:1], UA, UG, W, F)])
    with pytest.raises(ValueError, match="same"):
        kron_covariance_inf_tiled([(J, UA, UG, W, F), (J[:, :33], UA, UG, W, F)])
    with pytest.raises(ValueError):
        kron_covariance_outer_inf_tiled([(a[:1], D, UA, UG, W, F)])
    with pytest.raises(ValueError):
        kron_covariance_outer_inf_tiled([(a[:, :-2], D, UA, UG, W, F)])
    with pytest.raises(ValueError):
        kron_covariance_outer_inf_tiled([(torch.zeros(nb, 2, nA - 1), D, UA, UG, W, F)])
    # valid shapes with 40 outputs on the CPU get as far as the device requirement, and no further
    with pytest.raises(NativeError):
        kron_covariance_inf_tiled([(J, UA, UG, W, F)])
    with pytest.raises(NativeError):
        kron_covariance_outer_inf_tiled([(a, D, UA, UG, W, F)])
    # the capped functions keep their cap
    with pytest.raises(ValueError, match="kron_covariance_inf handles at most 32"):
        kron_covariance_inf([(J, UA, UG, W, F)])
    with pytest.raises(ValueError, match="kron_covariance_outer_inf handles at most 32"):
        kron_covariance_outer_inf([(a, D, UA, UG, W, F)])


def test_inf_calls_pick_the_pair_by_nc():
    from bnn_kfac_amd import variance as V
    for nc in (1, 10, 32):
        assert V._inf_calls(nc) == (V.kron_covariance_inf, V.kron_covariance_outer_inf)
    for nc in (33, 40, 1000):
        assert V._inf_calls(nc) == (V.kron_covariance_inf_tiled, V.kron_covariance_outer_inf_tiled)


@pytest.mark.parametrize("nc", [32, 33])
@pytest.mark.parametrize("route", ["dense", "factored"])
def test_inf_chunk_takes_the_capped_calls_up_to_32_outputs_and_the_tiled_ones_above(monkeypatch, route, nc):
    """Recording stubs in place of the four covariance functions: a Linear and a Conv2d layer,
    both `jacobians` routes, Conv2d rows through the dense call."""
    from bnn_kfac_amd import variance as V
    calls = []

    def stub(name):
        def fn(terms, max_workspace_bytes=1 << 30):
            first = terms[0]
            lead = first[0] if name.startswith("kron_covariance_inf") else first[1]
            calls.append((name, len(terms)))
            return torch.zeros(lead.shape[0], nc, nc)
        return fn

    for name in ("kron_covariance_inf", "kron_covariance_outer_inf", "kron_covariance_inf_tiled",
                 "kron_covariance_outer_inf_tiled"):
        monkeypatch.setattr(V, name, stub(name))
    monkeypatch.setattr(V, "_conv_rows", V.conv_jacobian_rows)
    torch.manual_seed(0)
    net = nn.Sequential(nn.Conv2d(1, 2, 3), nn.ReLU(), nn.Flatten(), nn.Linear(2 * 2 * 2, nc))
    layers = [net[0], net[3]]
    factors = {layer: (None, None, None, None) for layer in layers}
    f, cov = V._inf_chunk(net, layers, factors, torch.rand(3, 1, 4, 4), route)
    assert f.shape == (3, nc) and cov.shape == (3, nc, nc)
    suffix = "_tiled" if nc > 32 else ""
    if route == "dense":
        assert calls == [("kron_covariance_inf" + suffix, 2)]
    else:
        assert calls == [("kron_covariance_outer_inf" + suffix, 1), ("kron_covariance_inf" + suffix, 1)]
