"""CPU: the host side of the per-entry-weight GLM predictive -- variance.efb_weights /
efb_log_det_sweep against numpy fp64, the room the kernel tolerance of
test_gpu_glm_full.py leaves over a plain fp32 evaluation, and the ValueErrors of
kron_covariance_full / kron_covariance_outer_full that fire before any device call."""
import types

import numpy as np
import pytest
import torch

import glm_full_cases as C

GRID = [(0.04, 200.0), (1.0, 200.0), (1e-4, 1.0), (1e-6, 1e4)]
KERNEL_TOL = 1e-5  # test_gpu_glm_full.py: atol = 1e-5 * max|ref[t]| per grid point


def _lam(nG, nA, seed):
    """Distinct non-negative entries, a few exact zeros (lambdas on a factor's null space)."""
    rng = np.random.default_rng(seed)
    lam = rng.permutation(np.arange(nG * nA, dtype=np.float64)).reshape(nG, nA) ** 2 * 1e-3
    return lam


def test_efb_weights_match_numpy_and_are_the_transpose():
    from bnn_kfac_amd.variance import efb_weights
    nG, nA = 3, 5
    lam = _lam(nG, nA, 0)
    assert len(set(lam.ravel())) == nG * nA
    got = efb_weights(torch.from_numpy(lam), GRID)
    assert got.shape == (len(GRID), nA, nG) and got.dtype == torch.float32 and got.is_contiguous()
    want = np.stack([1.0 / (s * lam.T + n) for n, s in GRID])
    np.testing.assert_allclose(got.numpy().astype(np.float64), want.astype(np.float32).astype(np.float64),
                               rtol=1e-12, atol=0)
    for t, (n, s) in enumerate(GRID):      # entry by entry: W[t, i, g] belongs to lam[g, i]
        for i in range(nA):
            for g in range(nG):
                assert float(got[t, i, g]) == float(np.float32(1.0 / (s * lam[g, i] + n)))
    # EFB.invert's own numbers, squared and transposed
    lam32 = torch.from_numpy(lam.astype(np.float32))
    inv = torch.reciprocal(200.0 * lam32 + 0.04).sqrt()
    np.testing.assert_allclose(efb_weights(lam32, [(0.04, 200.0)])[0].numpy(), (inv.t() ** 2).numpy(), rtol=1e-6)
    # an fp32 state is widened before the arithmetic, not after it
    want32 = np.stack([1.0 / (s * lam32.numpy().astype(np.float64).T + n) for n, s in GRID])
    np.testing.assert_allclose(efb_weights(lam32, GRID).numpy().astype(np.float64),
                               want32.astype(np.float32).astype(np.float64), rtol=1e-12, atol=0)
    with pytest.raises(ValueError):
        efb_weights(torch.ones(4), GRID)


def _fake_efb(lams):
    return types.SimpleNamespace(state={f"l{i}": torch.from_numpy(l) for i, l in enumerate(lams)})


def test_efb_log_det_sweep_matches_numpy():
    from bnn_kfac_amd.variance import efb_log_det_sweep
    lams = [_lam(3, 5, 1), _lam(4, 7, 2).astype(np.float32)]
    grid = GRID + [([0.04, 1.0], [200.0, 3.0])]  # one per-layer pair of lists
    got = efb_log_det_sweep(_fake_efb(lams), grid)
    assert got.shape == (len(grid),) and got.dtype == torch.float64
    for t, (add, mul) in enumerate(grid):
        want = 0.0
        for i, lam in enumerate(lams):
            n, s = (add[i], mul[i]) if isinstance(add, list) else (add, mul)
            want += np.log(s * lam.astype(np.float64) + n).sum()
        np.testing.assert_allclose(float(got[t]), want, rtol=1e-12)
    # log det = -sum log W: the two helpers describe one damped spectrum
    from bnn_kfac_amd.variance import efb_weights
    w = efb_weights(torch.from_numpy(lams[0]), GRID).double()
    np.testing.assert_allclose(-w.log().sum(dim=(1, 2)).numpy(),
                               efb_log_det_sweep(_fake_efb(lams[:1]), GRID).numpy(), rtol=1e-6)


def test_non_positive_damped_eigenvalue_raises():
    from bnn_kfac_amd.variance import efb_log_det_sweep, efb_weights
    lam = torch.tensor([[-0.5, 0.0, 2.0]], dtype=torch.float64)
    assert efb_weights(lam, [(1.0, 1.0)]).shape == (1, 3, 1)       # -0.5 + 1 > 0
    for grid in ([(1.0, 1.0), (0.5, 1.0)],                         # -0.5 + 0.5 = 0
                 [(0.0, 1.0)],                                     # the zero eigenvalue undamped
                 [(1.0, 4.0)]):                                    # -0.5 * 4 + 1 < 0
        with pytest.raises(np.linalg.LinAlgError):
            efb_weights(lam, grid)
        with pytest.raises(np.linalg.LinAlgError):
            efb_log_det_sweep(_fake_efb([lam.numpy()]), grid)
    with pytest.raises(np.linalg.LinAlgError):
        efb_weights(torch.tensor([[float("nan"), 1.0]]), [(1.0, 1.0)])
    assert efb_log_det_sweep(_fake_efb([lam.numpy()]), [(1.0, 1.0)]).shape == (1,)


# ------------------------------------------------------------------ the tolerance has room
def _fp32_outer(a, ones, D, VA, VG, W):
    a, D, VA, VG, W = (torch.from_numpy(np.array(t)) for t in (a, D, VA, VG, W))
    abar = torch.cat([a, torch.ones(a.shape[0], 1)], dim=1) if ones else a
    r = torch.einsum("bi,tig->tbg", (abar @ VA) ** 2, W)
    Q = D @ VG
    return torch.einsum("bcg,tbg,bdg->tbcd", Q, r, Q).numpy()


def _fp32_dense(J, nA, nG, VA, VG, W):
    J, VA, VG, W = (torch.from_numpy(np.array(t)) for t in (J, VA, VG, W))
    nb, nc = J.shape[:2]
    Y = torch.einsum("bcih,hk->bcik", torch.einsum("ai,bcag->bcig", VA, J.reshape(nb, nc, nA, nG)), VG)
    return torch.einsum("tih,bcih,bdih->tbcd", W, Y, Y).numpy()


def _worst(got, ref):
    return max(float(np.abs(got[t] - ref[t]).max() / np.abs(ref[t]).max()) for t in range(ref.shape[0]))


def test_fp32_evaluation_stays_inside_a_third_of_the_kernel_tolerance():
    """A plain fp32 torch evaluation of both formulas, on every shape of the GPU test at
    nt = 5, against the fp64 reference: at most a third of the kernel tolerance."""
    nt = 5
    assert torch.get_default_dtype() == torch.float32
    worst = {"outer": 0.0, "dense": 0.0}
    for shape in C.OUTER_SHAPES:
        a, D, VA, VG, W, ref = C.outer_case(*shape)
        got = _fp32_outer(a, shape[1], D, VA, VG, W[:nt])
        assert got.dtype == np.float32
        err = _worst(got.astype(np.float64), ref[:nt])
        print("outer", shape, "fp32 err / max|ref| =", err)
        worst["outer"] = max(worst["outer"], err)
    for shape in C.DENSE_SHAPES:
        J, VA, VG, W, ref = C.dense_case(*shape)
        got = _fp32_dense(J, shape[0], shape[1], VA, VG, W[:nt])
        assert got.dtype == np.float32
        err = _worst(got.astype(np.float64), ref[:nt])
        print("dense", shape, "fp32 err / max|ref| =", err)
        worst["dense"] = max(worst["dense"], err)
    print("worst:", worst)
    assert worst["outer"] <= KERNEL_TOL / 3 and worst["dense"] <= KERNEL_TOL / 3


# ------------------------------------------------------------------ argument errors
def test_value_errors_fire_before_any_device_call():
    """Shapes are judged on the host: CPU tensors never reach the device requirement."""
    from bnn_kfac_amd.variance import kron_covariance_full, kron_covariance_outer_full
    nA, nG, nb, nc, nt = 6, 4, 2, 3, 2
    J, a, D = torch.zeros(nb, nc, nA * nG), torch.zeros(nb, nA - 1), torch.zeros(nb, nc, nG)
    VA, VG, W = torch.eye(nA), torch.eye(nG), torch.ones(nt, nA, nG)
    bad_W = [torch.ones(nt, nG, nA), torch.ones(nt, nA, nG - 1), torch.ones(nt, nA * nG), torch.ones(nA),
             torch.ones(0, nA, nG)]
    for w in bad_W:
        with pytest.raises(ValueError):
            kron_covariance_full([(J, VA, VG, w)])
        with pytest.raises(ValueError):
            kron_covariance_outer_full([(a, D, VA, VG, w)])
    with pytest.raises(ValueError, match="at most 32"):
        kron_covariance_full([(torch.zeros(nb, 33, nA * nG), VA, VG, W)])
    with pytest.raises(ValueError, match="at most 32"):
        kron_covariance_outer_full([(a, torch.zeros(nb, 33, nG), VA, VG, W)])
    with pytest.raises(ValueError, match="same number nt"):
        kron_covariance_full([(J, VA, VG, W), (J, VA, VG, W[:1])])
    with pytest.raises(ValueError, match="same number nt"):
        kron_covariance_outer_full([(a, D, VA, VG, W), (a, D, VA, VG, W[0])])
    with pytest.raises(ValueError, match="no terms"):
        kron_covariance_full([])
    with pytest.raises(ValueError, match="no terms"):
        kron_covariance_outer_full([])
    # the siblings' other shape errors
    with pytest.raises(ValueError):
        kron_covariance_full([(J[:, :, :-1], VA, VG, W)])
    with pytest.raises(ValueError):
        kron_covariance_full([(J, VA, VG, W), (J[:1], VA, VG, W)])
    with pytest.raises(ValueError):
        kron_covariance_outer_full([(a[:1], D, VA, VG, W)])
    with pytest.raises(ValueError):
        kron_covariance_outer_full([(a[:, :-1], D, VA, VG, W)])
    with pytest.raises(ValueError):
        kron_covariance_full([(J, torch.ones(nA, nA + 1), VG, W)])
