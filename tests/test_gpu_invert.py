"""GPU parity: KFAC.invert (fp64 device potrf + trtri) vs the fp64 oracle and the goldens.

Criterion: the device result within rtol 1e-4 of the fp64
restatement cholesky(inverse(sqrt(s) F + sqrt(n) I)); against the reference's own
fp32 output only to the reference's own error (it is ~5e-3 off at cond 5e4).
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import golden
from oracle import kfac_oracle as O

pytestmark = pytest.mark.gpu


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _spd(n, rng, cond=1e4):
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    ev = np.logspace(0, np.log10(cond), n)
    return ((q * ev) @ q.T).astype(np.float32)


@pytest.mark.parametrize("n", [1, 5, 31, 32, 33, 63, 64, 65, 128, 129, 200, 785, 1536, 1537, 2000])
def test_inv_chol_sizes_vs_fp64(hip_device, n):
    from bnn_kfac_amd import _native as N
    rng = np.random.default_rng(n)
    F = _spd(n, rng)
    Ft = _t(F, hip_device)
    L = torch.empty_like(Ft)
    info = N.invert([N.invert_job(Ft, L, 200 ** 0.5, 0.04 ** 0.5)], hip_device)
    assert int(info.cpu()[0]) == 0
    ref = O.invert_factor(F, 0.04, 200)
    got = L.cpu().numpy()
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-7 * np.abs(ref).max())
    assert np.all(np.triu(got, 1) == 0)


def test_grouped_invert_and_inverse_kind(hip_device):
    from bnn_kfac_amd import _native as N
    rng = np.random.default_rng(3)
    mats = [_spd(n, rng, 1e3) for n in (10, 129, 70, 300)]
    jobs, outs = [], []
    for i, F in enumerate(mats):
        Ft = _t(F, hip_device)
        out = torch.empty_like(Ft)
        kind = N.OUT_INVERSE if i % 2 else N.OUT_INV_CHOL
        jobs.append(N.invert_job(Ft, out, 3.0, 0.5, kind))
        outs.append((Ft, out, kind))
    info = N.invert(jobs, hip_device)
    assert not info.cpu().any()
    for F, (_, out, kind) in zip(mats, outs):
        R = O.damped_factor(F, 0.25, 9.0)
        ref = np.linalg.inv(R) if kind == N.OUT_INVERSE else np.linalg.cholesky(np.linalg.inv(R))
        np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-4, atol=1e-7 * np.abs(ref).max())


def _invert_group(mats, kinds, dev):
    """One grouped call (scale 3, shift 0.5) on `dev`; returns (outs, info), synchronised."""
    from bnn_kfac_amd import _native as N
    jobs, outs = [], []
    for F, kind in zip(mats, kinds):
        Ft = _t(F, dev)
        outs.append(torch.full_like(Ft, float("nan")))
        jobs.append(N.invert_job(Ft, outs[-1], 3.0, 0.5, kind))
    info = N.invert(jobs, dev)
    torch.cuda.synchronize()
    return outs, info.cpu()


def _check_group(mats, kinds, outs, info):
    from bnn_kfac_amd import _native as N
    assert not info.any()
    for F, kind, out in zip(mats, kinds, outs):
        R = O.damped_factor(F, 0.25, 9.0)
        ref = np.linalg.inv(R) if kind == N.OUT_INVERSE else np.linalg.cholesky(np.linalg.inv(R))
        got = out.cpu().numpy()
        np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-7 * np.abs(ref).max())
        if kind == N.OUT_INV_CHOL:
            assert np.all(np.triu(got, 1) == 0)


@pytest.fixture(scope="module")
def blocked_group():
    """1537 is the smallest size on 64-tiles (T = 25: five panel blocks, four with
    look-ahead); the 70 and 200 jobs run out of tasks in the early blocks."""
    from bnn_kfac_amd import _native as N
    rng = np.random.default_rng(17)
    return ([_spd(n, rng, 1e3) for n in (1537, 70, 200)],
            [N.OUT_INV_CHOL, N.OUT_INVERSE, N.OUT_INVERSE])


def test_blocked_grouped_both_kinds(hip_device, blocked_group):
    mats, kinds = blocked_group
    outs, info = _invert_group(mats, kinds, hip_device)
    _check_group(mats, kinds, outs, info)


def test_blocked_lookahead_bit_exact(hip_device, blocked_group):
    """Each tile sums the same panels in the same order whichever part of the bulk
    update owns it: the helper-stream split changes no bit."""
    from bnn_kfac_amd import _native as N
    mats, kinds = blocked_group
    before = N.get_knob("KFAC_INV_LOOKAHEAD")
    got = {}
    try:
        for la in (0, 1):
            N.set_knob("KFAC_INV_LOOKAHEAD", la)
            outs, info = _invert_group(mats, kinds, hip_device)
            assert not info.any()
            got[la] = outs
    finally:
        N.set_knob("KFAC_INV_LOOKAHEAD", before)
    for a, b in zip(got[0], got[1]):
        assert torch.equal(a, b)


def test_merged_upper_limit_inverse_kind(hip_device):
    """n = 1536 is the largest size on 32-tiles (T = 48); a full-inverse job in the group
    keeps the steps off the graph replay and the output on inv_xtx / inv_out."""
    from bnn_kfac_amd import _native as N
    rng = np.random.default_rng(19)
    mats = [_spd(n, rng, 1e3) for n in (1536, 33)]
    kinds = [N.OUT_INVERSE, N.OUT_INV_CHOL]
    outs, info = _invert_group(mats, kinds, hip_device)
    _check_group(mats, kinds, outs, info)


def test_kfac_invert_small_golden(hip_device):
    from bnn_kfac_amd.curvatures import KFAC
    g = golden("g1_small_linear.npz")
    net = nn.Sequential(nn.Linear(20, 12), nn.ReLU(), nn.Linear(12, 5, bias=False)).to(hip_device)
    kfac = KFAC(net)
    for bi in range(3):
        kfac.record[net[0]] = [_t(g[f"b{bi}_a1"], hip_device), _t(g[f"b{bi}_g1"], hip_device)]
        kfac.record[net[2]] = [_t(g[f"b{bi}_a2"], hip_device), _t(g[f"b{bi}_g2"], hip_device)]
        kfac.update(batch_size=16)
    for tag, (add, mult) in {"s": (0.2 ** 2, 200), "t": (1, 200),
                             "l": ([0.1, 0.3], [10.0, 20.0])}.items():
        kfac.invert(add, mult)
        pairs = O.damping_pairs(add, mult, 2)
        for li, layer in enumerate([net[0], net[2]]):
            LA, LG = [t.cpu().numpy() for t in kfac.inv_state[layer]]
            A, G = [t.cpu().numpy() for t in kfac.state[layer]]
            n, s = pairs[li]
            np.testing.assert_allclose(LA, O.invert_factor(A, n, s), rtol=1e-4, atol=1e-8)
            np.testing.assert_allclose(LG, O.invert_factor(G, n, s), rtol=1e-4, atol=1e-8)
            np.testing.assert_allclose(LA, g[f"inv{tag}_LA{li}"], rtol=2e-4, atol=2e-5)
            np.testing.assert_allclose(LG, g[f"inv{tag}_LG{li}"], rtol=2e-4, atol=2e-5)


def test_kfac_invert_mlp_golden(hip_device):
    from bnn_kfac_amd.curvatures import KFAC
    g = golden("g1_mlp.npz")
    net = nn.Sequential(nn.Linear(784, 128), nn.ReLU(), nn.Linear(128, 10)).to(hip_device)
    kfac = KFAC(net)
    rng = np.random.default_rng(123)
    for B in (256, 256, 256, 96):
        a1 = rng.random((B, 784), dtype=np.float32)
        g1 = rng.standard_normal((B, 128), dtype=np.float32)
        a2 = rng.random((B, 128), dtype=np.float32)
        g2 = rng.standard_normal((B, 10), dtype=np.float32)
        kfac.record[net[0]] = [_t(a1, hip_device), _t(g1, hip_device)]
        kfac.record[net[2]] = [_t(a2, hip_device), _t(g2, hip_device)]
        kfac.update(B)
    kfac.invert(0.2 ** 2, 200)
    LA1, LG1 = [t.cpu().numpy() for t in kfac.inv_state[net[0]]]
    LA2, LG2 = [t.cpu().numpy() for t in kfac.inv_state[net[2]]]
    A1 = kfac.state[net[0]][0].cpu().numpy()
    # against fp64 truth on the device's own factor: tight
    np.testing.assert_allclose(LA1, O.invert_factor(A1, 0.04, 200), rtol=1e-4, atol=1e-7)
    # against the reference's fp32 outputs: the reference's own error band
    np.testing.assert_allclose(LG1, g["LG1"], rtol=5e-4, atol=1e-5)
    np.testing.assert_allclose(LA2, g["LA2"], rtol=5e-4, atol=1e-5)
    np.testing.assert_allclose(LG2, g["LG2"], rtol=5e-4, atol=1e-5)
    np.testing.assert_allclose(np.diag(LA1), g["LA1_diag"], rtol=1e-2, atol=1e-5)
    np.testing.assert_allclose(LA1[-8:], g["LA1_tail"], rtol=1e-2, atol=2e-3)


def test_singular_raises_linalgerror(hip_device, capsys):
    """Under the defaults invert() itself raises LinAlgError on a non-SPD factor,
    after the reference's printed message (curvatures.py:390-396), so a caller's
    `try: kfac.invert(...) except LinAlgError` catches it; the failing layer is not
    assigned; a later damped inversion runs."""
    from bnn_kfac_amd.curvatures import KFAC
    g = golden("g2_singular.npz")
    assert str(g["outcome"]) == "LinAlgError"
    net = nn.Sequential(nn.Linear(6, 4)).to(hip_device)
    kfac = KFAC(net)
    assert kfac.eager_verdict
    kfac.record[net[0]] = [_t(g["a"], hip_device), _t(g["g"], hip_device)]
    kfac.update(2)
    with pytest.raises(np.linalg.LinAlgError):
        kfac.invert(0.0, 1.0)
    assert "PyTorch Cholesky is singular. Using Numpy." in capsys.readouterr().out
    assert net[0] not in kfac.inv_state
    kfac.invert(1.0, 1.0)  # damped: positive definite, no raise
    assert net[0] in kfac.inv_state


def test_singular_deferred_verdict(hip_device):
    """eager_verdict = False (the bench's pipelined mode): the verdict is read back
    asynchronously and raises at the next inv_state read or invert()."""
    from bnn_kfac_amd.curvatures import KFAC
    g = golden("g2_singular.npz")
    net = nn.Sequential(nn.Linear(6, 4)).to(hip_device)
    kfac = KFAC(net)
    kfac.eager_verdict = False
    kfac.record[net[0]] = [_t(g["a"], hip_device), _t(g["g"], hip_device)]
    kfac.update(2)
    kfac.invert(0.0, 1.0)  # the verdict is read back asynchronously ...
    with pytest.raises(np.linalg.LinAlgError):
        _ = kfac.inv_state  # ... and settled at the next inv_state read
    assert net[0] not in kfac.inv_state
    kfac.invert(0.0, 1.0)
    torch.cuda.synchronize()  # the verdict is back before the next invert() starts ...
    with pytest.raises(np.linalg.LinAlgError):
        kfac.invert(1.0, 1.0)  # ... so that invert() reads it and raises (and does not run)
    kfac.invert(1.0, 1.0)
    assert net[0] in kfac.inv_state


def test_invert_identity_property_wide(hip_device):
    """Size-independent check at a wide-MLP-like size: L L^T R = I."""
    from bnn_kfac_amd import _native as N
    rng = np.random.default_rng(9)
    n = 1500
    X = rng.random((4096, n), dtype=np.float32)
    Xt = _t(X, hip_device)
    F = (Xt.t() @ Xt) / 4096
    L = torch.empty_like(F)
    info = N.invert([N.invert_job(F, L, 200 ** 0.5, 0.04 ** 0.5)], hip_device)
    assert int(info.cpu()[0]) == 0
    R = O.damped_factor(F.cpu().numpy(), 0.04, 200)
    Ld = L.cpu().numpy().astype(np.float64)
    E = Ld.T @ R @ Ld  # = I for the exact factor (L^T R L = I  <=>  L L^T = R^{-1})
    assert np.abs(E - np.eye(n)).max() < 1e-3


@pytest.mark.parametrize("reset", [True, False])
def test_overlapped_inversion_matches_serial(hip_device, reset):
    """invert() runs on the side stream and the next pass is queued right behind it
    (the bench's pattern, deferred verdicts: nothing read in between, so pass k+1's
    SYRK overlaps inversion k).  With reset() the passes alternate two packed buffers
    and pass k+2's flush overwrites the buffer inversion k read; without it every
    flush adds into the buffer the previous inversion is reading.  Every pass's L
    factors equal the serial path's bit for bit."""
    from bnn_kfac_amd.curvatures import KFAC
    torch.manual_seed(0)
    net = nn.Sequential(nn.Linear(784, 128), nn.ReLU(), nn.Linear(128, 10)).to(hip_device)
    g = torch.Generator(device=hip_device).manual_seed(3)
    passes = [[(torch.rand(2048, 784, device=hip_device, generator=g),
                torch.randn(2048, 128, device=hip_device, generator=g),
                torch.rand(2048, 128, device=hip_device, generator=g),
                torch.randn(2048, 10, device=hip_device, generator=g)) for _ in range(3)]
              for _ in range(3)]

    def run(overlap):
        kfac = KFAC(net)
        kfac.overlap_invert = overlap
        kfac.eager_verdict = False
        kept = []
        for batches in passes:
            if reset:
                kfac.reset()
            for a1, g1, a2, g2 in batches:
                kfac.record[net[0]] = [a1, g1]
                kfac.record[net[2]] = [a2, g2]
                kfac.update(a1.shape[0])
            kfac.invert(0.04, 200)
            kept.append(dict(kfac._inv_state))  # no settle: the next pass overlaps
        _ = kfac.inv_state
        torch.cuda.synchronize()
        return [[t.cpu().numpy() for pair in d.values() for t in pair] for d in kept]

    serial, overlapped = run(False), run(True)
    for got_pass, want_pass in zip(overlapped, serial):
        for got, want in zip(got_pass, want_pass):
            np.testing.assert_array_equal(got, want)
    # and pass 0 is right in its own terms: L^T R L = I on the oracle's damped factor
    ref = O.OracleKFAC(np.float64)
    for a1, g1, a2, g2 in passes[0]:
        ref.update_linear("l0", a1.cpu().numpy(), g1.cpu().numpy(), True)
    R = O.damped_factor(ref.state["l0"][0], 0.04, 200)
    L = serial[0][0].astype(np.float64)
    assert np.abs(L.T @ R @ L - np.eye(R.shape[0])).max() < 1e-3


def test_double_buffer_slow_inversion_race(hip_device):
    """A slow (4097-sized, throughput-bound) inversion still reading packed buffer P
    while later passes reduce into the buffers: update -> invert -> reset looped, plus
    update-after-invert without reset, pipelined (deferred verdicts).  state and
    inv_state equal the same run with double_buffer = False and no overlap."""
    from bnn_kfac_amd.curvatures import KFAC
    torch.manual_seed(0)
    net = nn.Sequential(nn.Linear(4096, 16)).to(hip_device)
    gen = torch.Generator(device=hip_device).manual_seed(7)
    batches = [(torch.rand(1024, 4096, device=hip_device, generator=gen),
                torch.randn(1024, 16, device=hip_device, generator=gen)) for _ in range(8)]
    plan = ["u", "u", "i", "r", "u", "i", "r", "u", "i", "u", "i", "r", "u", "u", "i"]

    def run(fast):
        kfac = KFAC(net)
        kfac.double_buffer = fast
        kfac.overlap_invert = fast
        kfac.eager_verdict = False
        out, k = [], 0
        for op in plan:
            if op == "u":
                kfac.record[net[0]] = list(batches[k % len(batches)])
                k += 1
                kfac.update(1024)
            elif op == "i":
                kfac.invert(0.04, 200)
                out.append(dict(kfac._inv_state))
            else:
                kfac.reset()
        st = [t.clone() for pair in kfac.state.values() for t in pair]
        _ = kfac.inv_state
        torch.cuda.synchronize()
        return ([[t.cpu().numpy() for pair in d.values() for t in pair] for d in out],
                [t.cpu().numpy() for t in st])

    want_inv, want_state = run(False)
    got_inv, got_state = run(True)
    for got_pass, want_pass in zip(got_inv, want_inv):
        for got, want in zip(got_pass, want_pass):
            np.testing.assert_array_equal(got, want)
    for got, want in zip(got_state, want_state):
        np.testing.assert_array_equal(got, want)


def test_back_to_back_throughput_bound_inversions(hip_device):
    """A factor > 24 tiles of 64 (here 1601^2) takes the single side stream: inversions
    queued back to back share its workspace, so each must be fully queued before the
    next starts (wide-MLP bench regression: spurious LinAlgError)."""
    import torch.nn as nn
    from bnn_kfac_amd.curvatures import KFAC
    torch.manual_seed(0)
    net = nn.Sequential(nn.Linear(1600, 8)).to(hip_device)
    kfac = KFAC(net)
    x = torch.rand(512, 1600, device=hip_device)
    for _ in range(4):
        net.zero_grad()
        nn.functional.cross_entropy(net(x), torch.randint(0, 8, (512,), device=hip_device)).backward()
        kfac.update(batch_size=512)
        kfac.invert(0.04, 200)
    LA, LG = kfac.inv_state[net[0]]
    A = kfac.state[net[0]][0].double()
    R = (200 ** 0.5) * A + (0.04 ** 0.5) * torch.eye(A.shape[0], device=hip_device, dtype=torch.float64)
    L = LA.double()
    err = (L.t() @ R @ L - torch.eye(A.shape[0], device=hip_device, dtype=torch.float64)).abs().max()
    assert err < 1e-3, float(err)


@pytest.mark.parametrize("where", ["invert_job", "pinned"])
def test_invert_failure_keeps_the_reduce(hip_device, monkeypatch, where):
    """invert() hands the pass's deferred reduce to the side stream (_take_reduce); a
    failure after that hand-over was prepared but before the side stream took it (an
    invert_job / allocation error, models/curvatures.py:381-392's inputs) must still
    reduce the pass on the caller's stream: `state` then equals the fp64 pass sum,
    and a retried invert() gives the same L as an undisturbed run."""
    from bnn_kfac_amd import curvatures as C
    torch.manual_seed(0)
    net = nn.Sequential(nn.Linear(784, 128), nn.ReLU(), nn.Linear(128, 10)).to(hip_device)
    g = torch.Generator(device=hip_device).manual_seed(11)
    batches = [(torch.rand(1024, 784, device=hip_device, generator=g),
                torch.randn(1024, 128, device=hip_device, generator=g),
                torch.rand(1024, 128, device=hip_device, generator=g),
                torch.randn(1024, 10, device=hip_device, generator=g)) for _ in range(3)]

    def run(fail):
        kfac = C.KFAC(net)
        kfac.eager_verdict = False
        kfac.launch_first = 16  # one launch at the flush: the reduce goes to the side stream
        kfac.reset()
        for a1, g1, a2, g2 in batches:
            kfac.record[net[0]] = [a1, g1]
            kfac.record[net[2]] = [a2, g2]
            kfac.update(a1.shape[0])
        if fail:
            with monkeypatch.context() as m:
                def boom(*a, **k):
                    raise RuntimeError("injected")
                if where == "invert_job":
                    m.setattr(C.N, "invert_job", boom)
                else:
                    m.setattr(kfac, "_pinned_host", boom)
                with pytest.raises(RuntimeError, match="injected"):
                    kfac.invert(0.04, 200)
        st = [t.cpu().numpy() for pair in kfac.state.values() for t in pair]
        kfac.invert(0.04, 200)
        inv = [t.cpu().numpy() for pair in kfac.inv_state.values() for t in pair]
        return st, inv

    st_bad, inv_bad = run(True)
    st_ok, inv_ok = run(False)
    ref = O.OracleKFAC(np.float64)
    for a1, g1, a2, g2 in batches:
        ref.update_linear("l0", a1.cpu().numpy(), g1.cpu().numpy(), True)
        ref.update_linear("l1", a2.cpu().numpy(), g2.cpu().numpy(), True)
    want = [ref.state["l0"][0], ref.state["l0"][1], ref.state["l1"][0], ref.state["l1"][1]]
    for got, w in zip(st_bad, want):
        np.testing.assert_allclose(got, w, rtol=1e-5, atol=1e-5 * np.abs(w).max())
    for a, b in zip(st_bad, st_ok):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(inv_bad, inv_ok):
        np.testing.assert_array_equal(a, b)
