"""CPU: the host side of the damping sweep -- the C ABI of kfac_kron_cov_sweep and
kfac_kron_cov_outer_sweep (struct layouts, argument validation before any launch,
workspace queries), variance.damping_weights / log_det_sweep against numpy, and the
lifetime of KFAC.eigh's cache.  No GPU calls."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

from abi_layout import c_layout

DENSE_FIELDS = ("J", "ldJ", "nA", "nG", "VA", "ldA", "VG", "ldG", "wA", "ldwA", "wG", "ldwG")
OUTER_FIELDS = ("a", "lda", "cols", "has_ones", "D", "ldD", "nG", "reserved", "VA", "ldA", "VG", "ldG",
                "wA", "ldwA", "wG", "ldwG")
GRID = [(0.04, 200.0), (1.0, 200.0), (1e-4, 1.0), (1e-6, 1e4)]


@pytest.mark.parametrize("cname,pyname,fields", [("kfac_cov_sweep_job", "CovSweepJob", DENSE_FIELDS),
                                                 ("kfac_cov_outer_sweep_job", "CovOuterSweepJob", OUTER_FIELDS)])
def test_sweep_struct_layout(tmp_path, cname, pyname, fields):
    from bnn_kfac_amd import _native as N
    S = getattr(N, pyname)
    got = c_layout(tmp_path, cname, fields)
    assert [f for f, _ in S._fields_] == list(fields)
    assert got == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in fields]


# (pointers are never dereferenced on the host: validation happens before any launch)
def _dense_job(N, nA=5, nG=3):
    return N.CovSweepJob(1 << 12, nA * nG, nA, nG, 1 << 13, nA, 1 << 14, nG, 1 << 15, nA, 1 << 16, nG)


def _outer_job(N, cols=4, has_ones=1, nG=3):
    nA = cols + has_ones
    return N.CovOuterSweepJob(1 << 12, cols, cols, has_ones, 1 << 13, nG, nG, 0, 1 << 14, nA, 1 << 15, nG,
                              1 << 16, nA, 1 << 17, nG)


CASES = [("kfac_kron_cov_sweep", "CovSweepJob", _dense_job,
          (("J", None), ("VA", None), ("VG", None), ("wA", None), ("wG", None), ("ldJ", 14), ("ldA", 4),
           ("ldG", 2), ("ldwA", 4), ("ldwG", 2), ("nA", 0), ("nG", -1))),
         ("kfac_kron_cov_outer_sweep", "CovOuterSweepJob", _outer_job,
          (("a", None), ("D", None), ("VA", None), ("VG", None), ("wA", None), ("wG", None), ("lda", 3),
           ("ldD", 2), ("ldA", 4), ("ldG", 2), ("ldwA", 4), ("ldwG", 2), ("cols", 0), ("nG", 0)))]


@pytest.mark.parametrize("symbol,pyname,make,bad_fields", CASES, ids=["dense", "outer"])
def test_sweep_validates_before_any_launch(symbol, pyname, make, bad_fields):
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
        assert query(arr, njobs, nb, nc, nt) == 0
    assert call(None, 1, 2, 3, 2, 0, out, None, 0, None) == N.KFAC_EINVAL
    assert call(arr, 1, 2, 3, 2, 0, None, None, 0, None) == N.KFAC_EINVAL
    for field, value in bad_fields:
        bad = make(N)
        setattr(bad, field, value)
        assert call(N.as_array(S, [bad]), 1, 2, 3, 2, 0, out, None, 0, None) == N.KFAC_EINVAL, field
    # nine jobs, and the second job of two, are refused too
    assert call(N.as_array(S, [make(N)] * 9), 9, 2, 3, 2, 0, out, None, 0, None) == N.KFAC_EINVAL
    bad = make(N)
    bad.wG = None
    assert call(N.as_array(S, [make(N), bad]), 2, 2, 3, 2, 0, out, None, 0, None) == N.KFAC_EINVAL
    # valid arguments: the workspace is checked next, still before any launch
    need = query(arr, 1, 2, 3, 2)
    assert need > 0
    assert call(arr, 1, 2, 3, 2, 0, out, None, 0, None) == N.KFAC_EWORKSPACE
    assert call(arr, 1, 2, 3, 2, 0, out, 1 << 21, need - 1, None) == N.KFAC_EWORKSPACE
    assert call(arr, 1, 2, 3, 64, 0, out, None, 0, None) == N.KFAC_EWORKSPACE  # nt = 64 is allowed


@pytest.mark.parametrize("symbol,pyname,make", [c[:3] for c in CASES], ids=["dense", "outer"])
def test_sweep_workspace_grows_with_nt_and_nb(symbol, pyname, make):
    from bnn_kfac_amd import _native as N
    query = getattr(N.lib(), symbol + "_workspace_bytes")
    big = dict(nA=70, nG=65) if pyname == "CovSweepJob" else dict(cols=130, nG=300)
    arr = N.as_array(getattr(N, pyname), [make(N, **big)])
    assert 0 < query(arr, 1, 4, 10, 1) < query(arr, 1, 4, 10, 2) < query(arr, 1, 4, 10, 64)
    assert query(arr, 1, 4, 10, 3) < query(arr, 1, 5, 10, 3) < query(arr, 1, 64, 10, 3)
    two = N.as_array(getattr(N, pyname), [make(N, **big), make(N)])
    assert query(two, 2, 4, 10, 3) > query(arr, 1, 4, 10, 3)


def _spectrum(n, seed):
    """Eigenvalues shaped like a factor's: a few large ones, a decaying tail, exact zeros."""
    rng = np.random.default_rng(seed)
    lam = np.sort(np.concatenate([np.zeros(n // 3), rng.random(n - n // 3) ** 4 * 50.0]))
    return lam


def test_damping_weights_match_numpy():
    from bnn_kfac_amd.variance import damping_weights
    lam = _spectrum(41, 0)
    got = damping_weights(torch.from_numpy(lam), GRID)
    assert got.shape == (len(GRID), 41) and got.dtype == torch.float32
    want = np.stack([1.0 / (np.sqrt(s) * lam + np.sqrt(n)) for n, s in GRID])
    np.testing.assert_allclose(got.numpy().astype(np.float64), want.astype(np.float32).astype(np.float64),
                               rtol=1e-12, atol=0)
    # an fp32 spectrum is widened before the arithmetic, not after it
    lam32 = torch.from_numpy(lam.astype(np.float32))
    want32 = np.stack([1.0 / (np.sqrt(s) * lam32.numpy().astype(np.float64) + np.sqrt(n)) for n, s in GRID])
    np.testing.assert_allclose(damping_weights(lam32, GRID).numpy().astype(np.float64),
                               want32.astype(np.float32).astype(np.float64), rtol=1e-12, atol=0)


def test_non_positive_shifted_eigenvalue_raises():
    from bnn_kfac_amd.variance import damping_weights, log_det_sweep
    lam = torch.tensor([-0.5, 0.0, 2.0], dtype=torch.float64)
    assert damping_weights(lam, [(1.0, 1.0)]).shape == (1, 3)      # -0.5 + 1 > 0
    with pytest.raises(np.linalg.LinAlgError):
        damping_weights(lam, [(1.0, 1.0), (0.25, 1.0)])            # -0.5 + 0.5 = 0
    with pytest.raises(np.linalg.LinAlgError):
        damping_weights(lam, [(0.0, 1.0)])                         # the zero eigenvalue undamped
    with pytest.raises(np.linalg.LinAlgError):
        damping_weights(torch.tensor([float("nan"), 1.0]), [(1.0, 1.0)])
    eig = {"layer": ((lam, None), (torch.tensor([1.0, 2.0], dtype=torch.float64), None))}
    assert log_det_sweep(eig, [(1.0, 1.0)]).shape == (1,)
    with pytest.raises(np.linalg.LinAlgError):
        log_det_sweep(eig, [(1.0, 1.0), (0.25, 4.0)])              # -0.5 * 2 + 0.5 < 0


def test_log_det_sweep_matches_numpy_and_slogdet():
    from bnn_kfac_amd.variance import log_det_sweep
    rng = np.random.default_rng(3)

    def spd(n):
        X = rng.standard_normal((n, max(1, n - 2)))  # rank-deficient, as a factor can be
        return X @ X.T / n

    shapes = [(5, 3), (7, 4)]
    mats = [(spd(nA), spd(nG)) for nA, nG in shapes]
    eig = {}
    for i, (A, G) in enumerate(mats):
        eig[f"l{i}"] = ((torch.from_numpy(np.linalg.eigvalsh(A)), None), (torch.from_numpy(np.linalg.eigvalsh(G)), None))
    grid = GRID + [([0.04, 1.0], [200.0, 3.0])]  # one per-layer pair of lists
    got = log_det_sweep(eig, grid)
    assert got.shape == (len(grid),) and got.dtype == torch.float64
    for t, (add, mul) in enumerate(grid):
        want = explicit = slack = 0.0
        for i, ((A, G), (nA, nG)) in enumerate(zip(mats, shapes)):
            n, s = (add[i], mul[i]) if isinstance(add, list) else (add, mul)
            RA = np.sqrt(s) * A + np.sqrt(n) * np.eye(nA)
            RG = np.sqrt(s) * G + np.sqrt(n) * np.eye(nG)
            want += nG * np.log(np.sqrt(s) * np.linalg.eigvalsh(A) + np.sqrt(n)).sum()
            want += nA * np.log(np.sqrt(s) * np.linalg.eigvalsh(G) + np.sqrt(n)).sum()
            R = np.kron(RA, RG)
            sign, logdet = np.linalg.slogdet(R)
            assert sign == 1.0
            explicit += logdet
            # slogdet's own error: an LU of R perturbs each of its n pivots by about
            # eps * cond(R) relatively (the rank-deficient factors reach cond 1e9 here)
            slack += R.shape[0] * np.finfo(np.float64).eps * np.linalg.cond(R)
        np.testing.assert_allclose(float(got[t]), want, rtol=1e-12)
        np.testing.assert_allclose(float(got[t]), explicit, rtol=1e-12, atol=slack)


def test_log_det_sweep_single_layer_5x3_against_slogdet():
    from bnn_kfac_amd.variance import log_det_sweep
    rng = np.random.default_rng(5)
    A = rng.standard_normal((5, 9)); A = A @ A.T / 9
    G = rng.standard_normal((3, 9)); G = G @ G.T / 9
    eig = {0: ((torch.from_numpy(np.linalg.eigvalsh(A)), None), (torch.from_numpy(np.linalg.eigvalsh(G)), None))}
    got = log_det_sweep(eig, GRID).numpy()
    for t, (n, s) in enumerate(GRID):
        R = np.kron(np.sqrt(s) * A + np.sqrt(n) * np.eye(5), np.sqrt(s) * G + np.sqrt(n) * np.eye(3))
        np.testing.assert_allclose(got[t], np.linalg.slogdet(R)[1], rtol=1e-12)


def test_eigh_cache_is_dropped_by_state_assignment_and_reset(monkeypatch):
    from bnn_kfac_amd import utilities
    from bnn_kfac_amd.curvatures import KFAC
    net = nn.Sequential(nn.Linear(4, 3), nn.Tanh(), nn.Linear(3, 2))
    kfac = KFAC(net)
    calls = []

    def fake_symeig(factors, eigenvectors=False, symmetrize=True):
        calls.append((len(factors), eigenvectors))
        out = []
        for F in factors:
            lam, V = torch.linalg.eigh((F.double() + F.double().T) / 2)
            out.append((lam, V.float()))
        return out

    monkeypatch.setattr(utilities, "symeig", fake_symeig)

    def state_of(scale):
        return {net[0]: [scale * torch.eye(5), scale * torch.eye(3)],
                net[2]: [scale * torch.eye(4), scale * torch.eye(2)]}

    kfac.state = state_of(1.0)
    assert kfac.eig_state == {}
    eig = kfac.eigh()
    assert calls == [(4, True)]                   # ONE grouped call over all four factors
    assert list(eig) == [net[0], net[2]] and kfac.eig_state is eig
    (lamA, VA), (lamG, VG) = eig[net[0]]
    assert lamA.dtype == torch.float64 and VA.dtype == torch.float32
    assert lamA.shape == (5,) and VA.shape == (5, 5) and lamG.shape == (3,) and VG.shape == (3, 3)
    assert kfac.eigh() is eig and len(calls) == 1  # cached
    kfac.state = state_of(2.0)                     # the state setter drops it
    assert kfac.eig_state == {}
    assert float(kfac.eigh()[net[2]][0][0][0]) == 2.0 and len(calls) == 2
    kfac.reset()                                   # so does reset
    assert kfac.eig_state == {}
    with pytest.raises(AssertionError):
        kfac.eigh()                                # (an empty state, as invert refuses it)


def test_eigh_cache_is_dropped_by_the_real_update(monkeypatch):
    """KFAC.update drops the cache before it looks at the records (here there are none: it
    raises, as it does without this feature, and the cache is gone)."""
    from bnn_kfac_amd import utilities
    from bnn_kfac_amd.curvatures import KFAC
    net = nn.Sequential(nn.Linear(4, 3))
    kfac = KFAC(net)
    monkeypatch.setattr(utilities, "symeig",
                        lambda factors, eigenvectors=False, symmetrize=True:
                        [(torch.ones(F.shape[0], dtype=torch.float64), torch.eye(F.shape[0])) for F in factors])
    kfac.state = {net[0]: [torch.eye(5), torch.eye(3)]}
    assert kfac.eigh() and kfac.eig_state
    kfac.defer_reduce = False
    with pytest.raises(AttributeError):
        kfac.update(batch_size=1)                  # no forward / backward was recorded
    assert kfac.eig_state == {}


def test_save_does_not_write_eigenpairs(tmp_path, monkeypatch):
    from bnn_kfac_amd import utilities
    from bnn_kfac_amd.curvatures import KFAC
    net = nn.Sequential(nn.Linear(4, 3))
    kfac = KFAC(net)
    monkeypatch.setattr(utilities, "symeig",
                        lambda factors, eigenvectors=False, symmetrize=True:
                        [(torch.ones(F.shape[0], dtype=torch.float64), torch.eye(F.shape[0])) for F in factors])
    kfac.state = {net[0]: [torch.eye(5), torch.eye(3)]}
    kfac.eigh()
    path = str(tmp_path / "kfac.pt")
    kfac.save(path)
    blob = torch.load(path, weights_only=True)
    assert sorted(blob) == ["inv_state", "model", "state"]
    kfac.load(path)                                # load assigns `state`: the cache goes
    assert kfac.eig_state == {}


def _hand_factors(net64, layers64, make_x, loss_of, passes=3, batch=64):
    """KFAC-shaped factors of an all-Linear net, accumulated by hand on the CPU and rounded
    to fp32 like `state`: A = sum_passes mean(abar abar^T) (rank-deficient where the batch
    or a ReLU leaves directions empty, ones column last), G = sum_passes B * mean(g g^T)."""
    factors = [None] * len(layers64)
    for _ in range(passes):
        seen = {}

        def capture(module, inputs, output):
            output.retain_grad()
            seen[module] = (inputs[0].detach(), output)

        hooks = [layer.register_forward_hook(capture) for layer in layers64]
        out = net64(make_x(batch).double())
        net64.zero_grad()
        loss_of(out).backward()
        for h in hooks:
            h.remove()
        for li, layer in enumerate(layers64):
            a, z = seen[layer]
            if layer.bias is not None:
                a = torch.cat([a, torch.ones(batch, 1, dtype=a.dtype)], dim=1)
            g = z.grad * batch
            A, G = (a.T @ a / batch).numpy(), (g.T @ g / batch).numpy()
            factors[li] = (A, G) if factors[li] is None else (factors[li][0] + A, factors[li][1] + G)
    return [(A.astype(np.float32).astype(np.float64), G.astype(np.float32).astype(np.float64))
            for A, G in factors]


@pytest.mark.parametrize("name", ["no_bias", "regression", "relu_inplace"])
def test_fp32_eigen_route_stays_inside_the_end_to_end_tolerance(name):
    """Host emulation of what test_gpu_glm_sweep.py relies on: on the small nets and the
    grid of the end-to-end test, the eigen route with V and w rounded to fp32 and fp32
    products stays within 1e-6 * max|cov[b]| of the fp64 inverse route -- two orders inside
    the 1e-4 the GPU test allows.  (In fp64 the two routes agree to 1e-10.)"""
    import glm_sweep_cases as C
    make, in_shape, loss_of = C.small_nets()[name]
    torch.manual_seed(0)
    net64 = make().double()
    layers64 = [m for m in net64.modules() if isinstance(m, nn.Linear)]
    factors = _hand_factors(net64, layers64, lambda n: torch.randn(n, *in_shape), loss_of)
    logits, rows = C.fp64_rows(net64, layers64, torch.randn(5, *in_shape))
    for point in C.grid_for(len(layers64)):
        points = [C.point_of(point, i) for i in range(len(layers64))]
        want = C.fp64_cov(rows, factors, points)
        got = C.fp32_eigen_cov(rows, factors, points).astype(np.float64)
        exact = 0.0
        for M, (A, G), (n, s) in zip(rows, factors, points):
            (lA, VA), (lG, VG) = np.linalg.eigh(A), np.linalg.eigh(G)
            Y = np.einsum("ai,bcag,gh->bcih", VA, M, VG)
            exact = exact + np.einsum("i,h,bcih,bdih->bcd", 1 / (np.sqrt(s) * lA + np.sqrt(n)),
                                      1 / (np.sqrt(s) * lG + np.sqrt(n)), Y, Y)
        for b in range(want.shape[0]):
            scale = np.abs(want[b]).max()
            print(name, point, b, "fp32 eigen route err / max =", np.abs(got[b] - want[b]).max() / scale)
            assert np.abs(exact[b] - want[b]).max() <= 1e-10 * scale
            assert np.abs(got[b] - want[b]).max() <= 1e-6 * scale
