"""CPU: the host side of the joint GLM predictive -- argument validation of
kfac_kron_cov_joint / kfac_kron_cov_outer_joint before any launch, their workspace queries,
the two formulas against each other and against the per-sample references in fp64 numpy,
variance.marginal_blocks, and glm_predictive(joint=True)'s argument errors.  No GPU calls."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import glm_joint_cases as C

OUT, WS = 1 << 16, 1 << 17  # (pointers are never dereferenced: validation precedes any launch)


def _dense_job(N, nA=5, nG=3):
    return N.CovJob(1 << 12, nA * nG, nA, nG, 1 << 13, nA, 1 << 14, nG, 1, 1)


def _outer_job(N, cols=4, has_ones=1, nG=3):
    return N.CovOuterJob(1 << 12, cols, cols, has_ones, 1 << 13, nG, nG, 0, 1 << 14, cols + has_ones,
                         1 << 15, nG, 1, 1)


def _routes(N):
    lib = N.lib()
    return [(lib.kfac_kron_cov_joint, lib.kfac_kron_cov_joint_workspace_bytes, N.CovJob, _dense_job,
             (("J", None), ("K1", None), ("K2", None), ("ldJ", 14), ("ld1", 4), ("ld2", 2), ("nA", 0),
              ("nG", -1))),
            (lib.kfac_kron_cov_outer_joint, lib.kfac_kron_cov_outer_joint_workspace_bytes, N.CovOuterJob,
             _outer_job,
             (("a", None), ("D", None), ("K1", None), ("K2", None), ("lda", 3), ("ldD", 2), ("ld1", 4),
              ("ld2", 2), ("cols", 0), ("nG", -2)))]


@pytest.mark.parametrize("route", [0, 1], ids=["dense", "factored"])
def test_joint_calls_validate_before_any_launch(route):
    from bnn_kfac_amd import _native as N
    call, query, struct, make, bad_fields = _routes(N)[route]
    arr = N.as_array(struct, [make(N)])
    nb, nc = 2, 3
    R = nb * nc
    for njobs in (0, 9, -1):
        assert call(arr, njobs, nb, nc, 0, OUT, R, None, 0, None) == N.KFAC_EINVAL
        assert query(arr, njobs, nb, nc) == 0
    for bad_nb, bad_nc in ((0, 3), (-4, 3), (2, 0), (2, -1)):
        assert call(arr, 1, bad_nb, bad_nc, 0, OUT, R, None, 0, None) == N.KFAC_EINVAL
        assert query(arr, 1, bad_nb, bad_nc) == 0
    assert call(None, 1, nb, nc, 0, OUT, R, None, 0, None) == N.KFAC_EINVAL
    assert call(arr, 1, nb, nc, 0, None, R, None, 0, None) == N.KFAC_EINVAL
    assert call(arr, 1, nb, nc, 0, OUT, R - 1, None, 0, None) == N.KFAC_EINVAL  # ldc < R
    for field, value in bad_fields:
        bad = make(N)
        setattr(bad, field, value)
        assert call(N.as_array(struct, [bad]), 1, nb, nc, 0, OUT, R, None, 0, None) == N.KFAC_EINVAL, field
    # the second job of two is validated too
    bad = make(N)
    bad.ld2 = 2
    assert call(N.as_array(struct, [make(N), bad]), 2, nb, nc, 0, OUT, R, None, 0, None) == N.KFAC_EINVAL
    # R, or the tile pairs of R x R, beyond the kernels' 32-bit indices
    for big_nb, big_nc in ((1 << 30, 32), ((1 << 31) // 10, 10), (1 << 22, 1), (1, 1 << 22)):
        assert call(arr, 1, big_nb, big_nc, 0, OUT, big_nb * big_nc, None, 0, None) == N.KFAC_EINVAL
        assert query(arr, 1, big_nb, big_nc) == 0
    # a valid call without a workspace, and with one a byte short
    assert call(arr, 1, nb, nc, 0, OUT, R, None, 0, None) == N.KFAC_EWORKSPACE
    assert call(arr, 1, nb, nc, 0, OUT, R + 3, None, 0, None) == N.KFAC_EWORKSPACE
    need = query(arr, 1, nb, nc)
    assert need > 0
    assert call(arr, 1, nb, nc, 0, OUT, R, WS, need - 1, None) == N.KFAC_EWORKSPACE
    # no cap on nc: accepted as far as the workspace check
    for wide in (33, 100):
        assert query(arr, 1, 1, wide) > 0 and query(arr, 1, 4, wide) > query(arr, 1, 1, wide)
        assert call(arr, 1, 1, wide, 0, OUT, wide, None, 0, None) == N.KFAC_EWORKSPACE
        assert call(arr, 1, 4, wide, 0, OUT, 4 * wide, WS, query(arr, 1, 4, wide) - 1,
                    None) == N.KFAC_EWORKSPACE


def test_outer_joint_without_ones_column():
    from bnn_kfac_amd import _native as N
    lib = N.lib()
    plain = _outer_job(N, has_ones=0)
    assert plain.ld1 == 4  # nA = cols: ld1 = cols is enough, with the ones column it is not
    assert lib.kfac_kron_cov_outer_joint(N.as_array(N.CovOuterJob, [plain]), 1, 2, 3, 0, OUT, 6, None, 0,
                                         None) == N.KFAC_EWORKSPACE
    short = _outer_job(N)
    short.ld1 = 4
    assert lib.kfac_kron_cov_outer_joint(N.as_array(N.CovOuterJob, [short]), 1, 2, 3, 0, OUT, 6, None, 0,
                                         None) == N.KFAC_EINVAL


def test_joint_workspace_queries():
    from bnn_kfac_amd import _native as N
    lib = N.lib()
    for nA, nG in ((785, 128), (20, 130), (65, 33)):
        arr = N.as_array(N.CovJob, [_dense_job(N, nA, nG)])
        sizes = [lib.kfac_kron_cov_joint_workspace_bytes(arr, 1, nb, 10) for nb in (1, 2, 8, 64)]
        assert sizes == sorted(set(sizes)) and sizes[0] >= 2 * 10 * nA * nG * 4  # U and T for every row
    for cols, nG in ((784, 128), (19, 130), (4096, 4096)):
        arr = N.as_array(N.CovOuterJob, [_outer_job(N, cols, 1, nG)])
        sizes = [lib.kfac_kron_cov_outer_joint_workspace_bytes(arr, 1, nb, 10) for nb in (1, 2, 8, 64)]
        assert sizes == sorted(set(sizes)) and sizes[0] >= (cols + 1 + 10 * nG) * 4  # U and V
    # two jobs need the sum of their scratch
    both = N.as_array(N.CovJob, [_dense_job(N, 785, 128), _dense_job(N, 65, 33)])
    one, two = (N.as_array(N.CovJob, [_dense_job(N, *s)]) for s in ((785, 128), (65, 33)))
    assert lib.kfac_kron_cov_joint_workspace_bytes(both, 2, 8, 10) == (
        lib.kfac_kron_cov_joint_workspace_bytes(one, 1, 8, 10) + lib.kfac_kron_cov_joint_workspace_bytes(two, 1, 8, 10))
    # the factored route holds no Jacobian-row-sized scratch
    outer = N.as_array(N.CovOuterJob, [_outer_job(N, 784, 1, 128)])
    dense = N.as_array(N.CovJob, [_dense_job(N, 785, 128)])
    assert (20 * lib.kfac_kron_cov_outer_joint_workspace_bytes(outer, 1, 64, 10)
            < lib.kfac_kron_cov_joint_workspace_bytes(dense, 1, 64, 10))
    # C5's layer at nb = 64 stays far below the default budget of the Python wrappers
    wide = N.as_array(N.CovOuterJob, [_outer_job(N, 4096, 1, 4096)])
    assert lib.kfac_kron_cov_outer_joint_workspace_bytes(wide, 1, 64, 10) < 1 << 27


def test_native_wrappers_exist():
    from bnn_kfac_amd import _native as N
    for name in ("kron_cov_joint", "kron_cov_joint_workspace_bytes", "kron_cov_outer_joint",
                 "kron_cov_outer_joint_workspace_bytes"):
        assert callable(getattr(N, name))
    assert N.kron_cov_joint_workspace_bytes([_dense_job(N)], 2, 3) == N.lib().kfac_kron_cov_joint_workspace_bytes(
        N.as_array(N.CovJob, [_dense_job(N)]), 1, 2, 3)


def test_native_wrappers_refuse_an_output_they_would_overrun():
    from bnn_kfac_amd import _native as N
    nb, nc = 2, 3
    for call, job in ((N.kron_cov_joint, _dense_job(N)), (N.kron_cov_outer_joint, _outer_job(N))):
        for out in (torch.zeros(6, 5), torch.zeros(5, 6), torch.zeros(6, 6).T,
                    torch.zeros(6, 12)[:, ::2], torch.zeros(36), torch.zeros(6, 6, 1)):
            with pytest.raises(ValueError, match="unit column stride"):
                call([job], nb, nc, out)
        with pytest.raises(N.NativeError):  # a well-shaped output that is not on the device
            call([job], nb, nc, torch.zeros(6, 9)[:, :6])


# ------------------------------------------------------------------ the formulas, fp64
@pytest.mark.parametrize("shape", [(4, 1, 3, 7, 10), (6, 0, 5, 3, 4), (9, 1, 2, 1, 5)])
def test_factored_formula_equals_dense_on_outer_rows(shape):
    cols, ones, nG, nb, nc = shape
    rng = np.random.default_rng(3)
    nA = cols + ones
    a, D = rng.standard_normal((nb, cols)), rng.standard_normal((nb, nc, nG))
    K1, K2 = np.tril(rng.standard_normal((nA, nA))), np.tril(rng.standard_normal((nG, nG)))
    dense = C.dense_joint_ref(C.outer_rows(a, ones, D), nA, nG, K1, K2)
    factored = C.outer_joint_ref(a, ones, D, K1, K2)
    assert dense.shape == factored.shape == (nb * nc, nb * nc)
    np.testing.assert_allclose(factored, dense, rtol=1e-12, atol=1e-12 * np.abs(dense).max())
    np.testing.assert_array_equal(factored, factored.T)
    # the diagonal blocks are the per-sample references
    from test_gpu_glm_factored import _ref_term
    want = _ref_term(a, ones, D, K1, K2)
    for ref in (dense, factored):
        blocks = ref.reshape(nb, nc, nb, nc)
        got = np.stack([blocks[b, :, b, :] for b in range(nb)])
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
    # and the definition: < T_r, T_r' >_F with T_r = K1^T M_r K2, one pair at a time
    M = C.outer_rows(a, ones, D).reshape(nb * nc, nA, nG)
    for r, r2 in ((0, 0), (nb * nc - 1, 0), (nc // 2, nb * nc - 1)):
        t, t2 = K1.T @ M[r] @ K2, K1.T @ M[r2] @ K2
        np.testing.assert_allclose(dense[r, r2], (t * t2).sum(), rtol=1e-12, atol=1e-12 * np.abs(dense).max())


def test_marginal_blocks():
    from bnn_kfac_amd.variance import marginal_blocks, probit_predictive
    torch.manual_seed(0)
    cov = torch.randn(5, 3, 5, 3)
    got = marginal_blocks(cov)
    assert got.shape == (5, 3, 3) and got.is_contiguous()
    for b in range(5):
        assert torch.equal(got[b], cov[b, :, b, :])
    sym = torch.randn(15, 15)
    sym = (sym @ sym.T).view(5, 3, 5, 3)
    assert probit_predictive(torch.randn(5, 3), marginal_blocks(sym)).shape == (5, 3)
    for bad in (torch.zeros(5, 3, 3), torch.zeros(5, 3, 4, 3), torch.zeros(5, 3, 5, 2)):
        with pytest.raises(ValueError):
            marginal_blocks(bad)


def test_glm_predictive_joint_argument_errors():
    from bnn_kfac_amd.variance import glm_predictive

    def stub(model, layers):
        class Stub:
            pass
        s = Stub()
        s.model, s.state, s.inv_state = model, {m: None for m in layers}, {}
        return s

    lin = nn.Linear(2, 2)
    with pytest.raises(ValueError):
        glm_predictive(stub(lin, []), torch.zeros(1, 2), jacobians="nope", joint=True)
    # the factored route: a layer that is neither Linear nor Conv2d, and a Linear layer with
    # a 3-D input, are refused while the captures are collected (before any device call)
    net = nn.Sequential(nn.Linear(3, 4), nn.LayerNorm(4), nn.Linear(4, 2))
    with pytest.raises(ValueError, match="Linear and Conv2d"):
        glm_predictive(stub(net, [net[1]]), torch.zeros(2, 3), layers=[net[1]], jacobians="factored",
                       joint=True)
    seq = nn.Sequential(nn.Linear(3, 2), nn.Flatten())
    with pytest.raises(ValueError, match="2-D Linear inputs"):
        glm_predictive(stub(seq, [seq[0]]), torch.zeros(2, 5, 3), layers=[seq[0]], jacobians="factored",
                       joint=True)
