"""CPU: the host side of the class-tiled weighted covariance -- the shape errors of
variance.kron_covariance_{full,outer_full,sweep,outer_sweep}_tiled on CPU tensors (before
anything asks for a device), the routing by the number of outputs, the capped functions'
unchanged errors, and the tolerance of test_gpu_glm_wtiled.py: the device's stage chain in
sequential fp32 on the host for the two long-K shapes.  No GPU calls."""
import numpy as np
import pytest
import torch

import glm_full_cases as C
import glm_sweep_cases as S
import glm_wtiled_cases as T


def test_routing_by_the_number_of_outputs():
    from bnn_kfac_amd import variance as V
    assert V.MAX_COV_CLASSES == 32
    for nc in (1, 10, 32):
        assert V._full_calls(nc) == (V.kron_covariance_full, V.kron_covariance_outer_full)
        assert V._sweep_calls(nc) == (V.kron_covariance_sweep, V.kron_covariance_outer_sweep)
    for nc in (33, 100, 1000):
        assert V._full_calls(nc) == (V.kron_covariance_full_tiled, V.kron_covariance_outer_full_tiled)
        assert V._sweep_calls(nc) == (V.kron_covariance_sweep_tiled, V.kron_covariance_outer_sweep_tiled)


def test_full_shape_errors_before_any_device_call():
    """CPU tensors: a shape error is a ValueError raised before anything asks for a device."""
    from bnn_kfac_amd.variance import kron_covariance_full_tiled, kron_covariance_outer_full_tiled
    eye = torch.eye
    J, W = torch.zeros(2, 40, 20), torch.ones(3, 5, 4)
    with pytest.raises(ValueError, match="no terms"):
        kron_covariance_full_tiled([])
    with pytest.raises(ValueError):
        kron_covariance_full_tiled([(J, eye(5), eye(3), torch.ones(3, 5, 3))])      # 20 columns, needs 15
    with pytest.raises(ValueError):
        kron_covariance_full_tiled([(J, eye(5), torch.zeros(4, 3), W)])             # VG not square
    with pytest.raises(ValueError):
        kron_covariance_full_tiled([(J, eye(5), eye(4), torch.ones(3, 4, 5))])      # W transposed
    with pytest.raises(ValueError):
        kron_covariance_full_tiled([(J, eye(5), eye(4), torch.ones(0, 5, 4))])      # no grid point
    with pytest.raises(ValueError):
        kron_covariance_full_tiled([(J, eye(5), eye(4), W), (J, eye(5), eye(4), W[:2])])   # nt differs
    with pytest.raises(ValueError):
        kron_covariance_full_tiled([(J, eye(5), eye(4), W), (J[:, :39], eye(5), eye(4), W)])  # nc differs
    a, D, Wo = torch.zeros(2, 5), torch.zeros(2, 40, 4), torch.ones(3, 6, 4)
    with pytest.raises(ValueError, match="no terms"):
        kron_covariance_outer_full_tiled([])
    for nA in (4, 7):                                                               # nA must be cols or cols + 1
        with pytest.raises(ValueError):
            kron_covariance_outer_full_tiled([(a, D, eye(nA), eye(4), torch.ones(3, nA, 4))])
    with pytest.raises(ValueError):
        kron_covariance_outer_full_tiled([(a[:1], D, eye(6), eye(4), Wo)])          # a has 1 row, D 2 samples
    with pytest.raises(ValueError):
        kron_covariance_outer_full_tiled([(a, D, eye(6), eye(3), torch.ones(3, 6, 3))])  # D has 4 columns
    with pytest.raises(ValueError):
        kron_covariance_outer_full_tiled([(torch.zeros(2, 5, 1), D, eye(6), eye(4), Wo)])  # a not 2-D
    with pytest.raises(ValueError):
        kron_covariance_outer_full_tiled([(a, D, eye(6), eye(4), Wo[:, :5])])       # W one row short


def test_no_class_cap_but_no_cpu_fallback():
    """40 and 1000 outputs pass the shape checks (the capped siblings raise ValueError there,
    as before) and stop at the device requirement."""
    from bnn_kfac_amd import _native as N
    from bnn_kfac_amd import variance as V
    for nc in (40, 1000):
        J, a, D = torch.zeros(2, nc, 20), torch.zeros(2, 5), torch.zeros(2, nc, 4)
        full = [(J, torch.eye(5), torch.eye(4), torch.ones(2, 5, 4))]
        outer_full = [(a, D, torch.eye(6), torch.eye(4), torch.ones(2, 6, 4))]
        sweep = [(J, torch.eye(5), torch.eye(4), torch.ones(2, 5), torch.ones(2, 4))]
        outer_sweep = [(a, D, torch.eye(6), torch.eye(4), torch.ones(2, 6), torch.ones(2, 4))]
        for capped, tiled, terms in ((V.kron_covariance_full, V.kron_covariance_full_tiled, full),
                                     (V.kron_covariance_outer_full, V.kron_covariance_outer_full_tiled, outer_full)):
            with pytest.raises(ValueError, match="at most 32"):
                capped(terms)
            with pytest.raises(N.NativeError):
                tiled(terms)
        # (the sweep functions ask for the device while they parse: NativeError from both)
        for tiled, terms in ((V.kron_covariance_sweep_tiled, sweep), (V.kron_covariance_outer_sweep_tiled, outer_sweep)):
            with pytest.raises(N.NativeError):
                tiled(terms)


def test_sweep_shape_errors():
    from bnn_kfac_amd.variance import kron_covariance_outer_sweep_tiled, kron_covariance_sweep_tiled
    eye = torch.eye
    with pytest.raises(ValueError, match="no terms"):
        kron_covariance_sweep_tiled([])
    with pytest.raises(ValueError, match="no terms"):
        kron_covariance_outer_sweep_tiled([])
    with pytest.raises(ValueError):
        kron_covariance_sweep_tiled([(torch.zeros(2, 40, 20), torch.zeros(5, 4), eye(4), torch.ones(2, 5),
                                      torch.ones(2, 4))])                           # VA not square
    with pytest.raises(ValueError):
        kron_covariance_outer_sweep_tiled([(torch.zeros(2, 5), torch.zeros(2, 40, 4), torch.zeros(6, 5), eye(4),
                                            torch.ones(2, 6), torch.ones(2, 4))])   # VA not square


def test_sequential_fp32_emulation_stays_within_a_quarter_of_the_bound():
    """The tolerance of the GPU tests on the two shapes with 2048-long chains: the stage chain
    emulated in sequential fp32 (glm_wtiled_cases) against the fp64 reference, nt = 5."""
    errs = T.emulated_errors()
    print(errs)
    assert set(errs) == {"full", "sweep", "outer_full", "outer_sweep"}
    for call in ("full", "sweep"):
        assert 0 < errs[call] <= T.scale_for(T.LONG_DENSE) / 4, (call, errs[call])
    for call in ("outer_full", "outer_sweep"):
        assert 0 < errs[call] <= T.scale_for(T.LONG_OUTER) / 4, (call, errs[call])
    assert T.scale_for(T.LONG_DENSE) == 1e-5 and T.scale_for(T.LONG_OUTER) == 1.4e-5
    assert all(T.scale_for(s) == 1e-5 for s in T.OUTER_SHAPES + T.DENSE_SHAPES if s != T.LONG_OUTER)


def test_emulation_is_the_reference_on_a_small_case():
    """The emulation computes the documented quantity: on a short shape it agrees with fp64."""
    J, VA, VG, W, ref = C.dense_case(5, 3, 2, 33)
    got = T.emulate_dense(J, 5, 3, VA, VG, W[:2].reshape(2, -1))
    assert T.rel_err(got, ref[:2]) < 1e-6
    a, D, VA, VG, W, ref = C.outer_case(4, 1, 3, 1, 33)
    assert T.rel_err(T.emulate_outer_full(a, 1, D, VA, VG, W[:2]), ref[:2]) < 1e-6
    a, D, VA, VG, wA, wG, ref = S.outer_case(4, 1, 3, 1, 33)
    assert T.rel_err(T.emulate_outer_sweep(a, 1, D, VA, VG, wA[:2], wG[:2]), ref[:2]) < 1e-6
    wA, wG = T.int_rank_one(3, 5, 4)
    assert set(np.unique(wA)) | set(np.unique(wG)) == {0, 1, 2}
