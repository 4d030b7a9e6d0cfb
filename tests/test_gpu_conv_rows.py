"""GPU: kfac_cov_conv_rows -- Conv2d Jacobian rows formed on the device.

Integer cases (conv_rows_cases.py) through the raw job struct: the whole buffer is compared,
the written region `array_equal` to the int64 reference, everything else to its prefill.
Random normal data against the fp64 reference at the project's kernel tolerance (rtol 1e-5,
atol 1e-5 * max|ref|, as test_gpu_glm_factored.py).  The three guarantees of the header with
torch.equal: two calls give the same bits; a row depends on its own a_b, D[b, c] and the
shapes only (not on nb, nc, or the tile of its columns); strided operands give the bits of
contiguous ones and leave M's padding alone.  Then variance.conv_jacobian_rows_device."""
import functools

import numpy as np
import pytest
import torch

import conv_rows_cases as R

pytestmark = pytest.mark.gpu


def _N():
    from bnn_kfac_amd import _native as N
    return N


def _rows(dev, g, a, D):
    """One raw call on contiguous device tensors a (n, C, H, W), D (n, nc, nG, Ho, Wo)."""
    N = _N()
    n, nc = D.shape[0], D.shape[1]
    assert a.is_contiguous() and D.is_contiguous()
    M = torch.full((n, nc, g.nA * g.nG), float("nan"), device=dev)
    N.cov_conv_rows([R.job(N, g, n, a.data_ptr(), D.data_ptr(), M.data_ptr())], n, nc, dev)
    return M


@functools.lru_cache(maxsize=None)
def _normal(spec, seed=0):
    """(geometry, a, D) fp32 numpy and the fp64 reference, once per shape."""
    g = R.geometry(spec)
    rng = np.random.default_rng(seed + 7919 * g.cols + g.nG)
    a = rng.standard_normal((g.nb, g.C, g.H, g.W)).astype(np.float32)
    D = rng.standard_normal((g.nb, g.nc, g.nG, g.Ho, g.Wo)).astype(np.float32)
    ref = R.rows_reference(a.astype(np.float64), D.astype(np.float64), g)
    for t in (a, D, ref):
        t.setflags(write=False)
    return g, a, D, ref


def _dev(dev, *arrays):
    return [torch.from_numpy(np.array(t)).to(dev) for t in arrays]


# ------------------------------------------------------------------ integer cases
@pytest.mark.parametrize("cid", R.IDS)
def test_integer_case_whole_buffer(hip_device, cid):
    N = _N()
    c = R.case(cid)
    buf = torch.from_numpy(np.array(c.flat)).to(hip_device)
    N.cov_conv_rows([R.case_job(N, c, buf.data_ptr())], c.g.nb, c.g.nc, hip_device)
    got = buf.cpu().numpy()
    bad = np.flatnonzero(~((got == c.want) | (np.isnan(got) & np.isnan(c.want))))
    assert R.same(got, c.want), (f"{len(bad)} elements differ; first at element {bad[0]} (a at {c.oA}, D at {c.oD}, "
                                 f"M at {c.oM}, ldM {c.ldM}): got {got[bad[0]]!r}, want {c.want[bad[0]]!r}")


# ------------------------------------------------------------------ random data
@pytest.mark.parametrize("cid", ["lenet-conv1", "lenet-conv2", "nA64", "nA65"])
def test_normal_data_matches_fp64(hip_device, cid):
    g, a, D, ref = _normal(dict(R.CASES)[cid])
    got = _rows(hip_device, g, *_dev(hip_device, a, D)).cpu().numpy()
    print(cid, "max err / max|ref| =", float(np.abs(got - ref).max() / np.abs(ref).max()))
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())


# (C, H, W, kh, kw, sh, sw, ph, pw, bias, nG, nb, nc): seven samples, ten classes
SEVEN = [(6, 14, 14, 5, 5, 1, 1, 0, 0, True, 16, 7, 10),   # conv2: 3 a-tiles x 3 column tiles
         (7, 6, 5, 3, 3, 1, 1, 1, 1, True, 7, 7, 10),      # a class boundary inside a tile, a tile edge inside a class
         (1, 28, 28, 5, 5, 1, 1, 2, 2, True, 6, 7, 10)]    # conv1: 25 stages
SEVEN_IDS = ["conv2", "nA64", "conv1"]


@pytest.mark.parametrize("spec", SEVEN, ids=SEVEN_IDS)
def test_two_calls_give_identical_bits(hip_device, spec):
    g, a, D, _ = _normal(spec)
    ad, Dd = _dev(hip_device, a, D)
    one, two = _rows(hip_device, g, ad, Dd), _rows(hip_device, g, ad, Dd)
    assert not torch.isnan(one).any()
    assert torch.equal(one, two)


@pytest.mark.parametrize("spec", SEVEN, ids=SEVEN_IDS)
def test_rows_do_not_depend_on_the_call(hip_device, spec):
    """Samples [1, 3, 6] alone, and classes [2, 3, 4] alone (other column tiles, another
    position in them), have the bits of those rows of the whole call."""
    g, a, D, _ = _normal(spec)
    ad, Dd = _dev(hip_device, a, D)
    whole = _rows(hip_device, g, ad, Dd)
    some = [1, 3, 6]
    assert torch.equal(_rows(hip_device, g, ad[some].contiguous(), Dd[some].contiguous()), whole[some])
    classes = [2, 3, 4]
    assert torch.equal(_rows(hip_device, g, ad, Dd[:, classes].contiguous()), whole[:, classes])
    for c in (0, 9):  # one class per call: the columns of class 9 move from tile 2 to tile 0
        assert torch.equal(_rows(hip_device, g, ad, Dd[:, c:c + 1].contiguous()), whole[:, c:c + 1])
    assert torch.equal(_rows(hip_device, g, ad[6:7].contiguous(), Dd[6:7, 4:5].contiguous()), whole[6:7, 4:5])


@pytest.mark.parametrize("spec", SEVEN[:2], ids=SEVEN_IDS[:2])
def test_strided_operands_and_sample_chunks(hip_device, spec):
    """a, D and M with pitches above their widths, NaN between: the bits of the contiguous
    call, the padding of M untouched; then the same buffers in sample chunks of 3, 3 and 1
    (pointer offsets, as variance's per-sample chunking does)."""
    N = _N()
    dev = hip_device
    g, a, D, _ = _normal(spec)
    ad, Dd = _dev(dev, a, D)
    plain = _rows(dev, g, ad, Dd)
    n, nc, chw, K, W = g.nb, g.nc, g.C * g.H * g.W, g.nG * g.L, g.nA * g.nG
    sB, ldD, ldM = chw + 3, K + 5, W + 7
    wa = torch.full((n, sB), float("nan"), device=dev)
    wa[:, :chw] = ad.reshape(n, chw)
    wD = torch.full((n * nc, ldD), float("nan"), device=dev)
    wD[:, :K] = Dd.reshape(n * nc, K)

    def run(chunks):
        wM = torch.full((n * nc, ldM), float("nan"), device=dev)
        for b0, nb in chunks:
            j = R.job(N, g, nb, wa[b0].data_ptr(), wD[b0 * nc].data_ptr(), wM[b0 * nc].data_ptr(), sB, ldD, ldM)
            N.cov_conv_rows([j], nb, nc, dev)
        return wM

    for chunks in ([(0, n)], [(0, 3), (3, 3), (6, 1)]):
        wM = run(chunks)
        assert torch.equal(wM[:, :W].reshape(n, nc, W), plain), chunks
        assert bool(torch.isnan(wM[:, W:]).all()), chunks
    # each of the three pitches alone
    for kw in ({"sB": sB}, {"ldD": ldD}, {"ldM": ldM}):
        wM = torch.full((n * nc, ldM), float("nan"), device=dev)
        src_a = wa if "sB" in kw else ad
        src_D = wD if "ldD" in kw else Dd
        dst = wM if "ldM" in kw else torch.full((n * nc, W), float("nan"), device=dev)
        N.cov_conv_rows([R.job(N, g, n, src_a.data_ptr(), src_D.data_ptr(), dst.data_ptr(), **kw)], n, nc, dev)
        assert torch.equal(dst[:, :W].reshape(n, nc, W), plain), kw


# (C, H, W, kh, kw, sh, sw, ph, pw, bias, nG): eight layers of one call, nb = 2, nc = 3
MIXED = [(6, 14, 14, 5, 5, 1, 1, 0, 0, True, 16), (1, 1, 1, 1, 1, 1, 1, 0, 0, True, 1),
         (7, 6, 5, 3, 3, 1, 1, 1, 1, True, 7), (3, 11, 8, 3, 2, 2, 1, 1, 0, False, 5),
         (1, 9, 9, 8, 8, 1, 1, 0, 0, True, 3), (1, 28, 28, 5, 5, 1, 1, 2, 2, True, 6),
         (2, 5, 5, 3, 3, 1, 1, 2, 2, False, 30), (1, 5, 13, 1, 1, 1, 1, 0, 0, True, 2)]


def test_eight_mixed_jobs_equal_eight_calls(hip_device):
    N = _N()
    dev = hip_device
    nb, nc = 2, 3
    rng = np.random.default_rng(8)
    gs, ops, refs = [], [], []
    for spec in MIXED:
        g = R.geometry(spec + (nb, nc))
        a = rng.integers(-2, 3, size=(nb, g.C, g.H, g.W)).astype(np.int64)
        D = rng.integers(-2, 3, size=(nb, nc, g.nG, g.Ho, g.Wo)).astype(np.int64)
        gs.append(g)
        ops.append(_dev(dev, a.astype(np.float32), D.astype(np.float32)))
        refs.append(R.rows_reference(a, D, g))
    singles = [_rows(dev, g, a, D) for g, (a, D) in zip(gs, ops)]
    grouped = [torch.full_like(m, float("nan")) for m in singles]
    jobs = [R.job(N, g, nb, a.data_ptr(), D.data_ptr(), m.data_ptr()) for g, (a, D), m in zip(gs, ops, grouped)]
    N.cov_conv_rows(jobs, nb, nc, dev)
    for g, one, many, ref in zip(gs, singles, grouped, refs):
        assert torch.equal(one, many), g
        np.testing.assert_array_equal(many.cpu().numpy(), ref.astype(np.float32))
    with pytest.raises(N.NativeError):
        N.cov_conv_rows(jobs + jobs[:1], nb, nc, dev)


# ------------------------------------------------------------------ conv_jacobian_rows_device
def _layer(g, dev):
    return torch.nn.Conv2d(g.C, g.nG, (g.kh, g.kw), stride=(g.sh, g.sw), padding=(g.ph, g.pw),
                           bias=g.bias).to(dev)


@pytest.mark.parametrize("cid", ["lenet-conv1", "lenet-conv2", "nA64", "stride2x1-nobias", "pad2"])
def test_device_rows_match_torch_rows(hip_device, cid):
    from bnn_kfac_amd.variance import conv_jacobian_rows, conv_jacobian_rows_device
    g, a, D, ref = _normal(dict(R.CASES)[cid])
    ad, Dd = _dev(hip_device, a, D)
    layer = _layer(g, hip_device)
    got = conv_jacobian_rows_device(layer, ad, Dd)
    assert got.shape == (g.nb, g.nc, g.nA * g.nG) and got.dtype == torch.float32 and got.device == ad.device
    want = conv_jacobian_rows(layer.double().cpu(), torch.from_numpy(np.array(a)).double(),
                              torch.from_numpy(np.array(D)).double()).numpy()
    np.testing.assert_allclose(want, ref, rtol=0, atol=1e-12 * np.abs(ref).max())  # (two fp64 evaluations)
    print(cid, "max err / max|ref| =", float(np.abs(got.cpu().numpy() - want).max() / np.abs(want).max()))
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-5, atol=1e-5 * np.abs(want).max())
    assert torch.equal(got, _rows(hip_device, g, ad, Dd))
    same_on_gpu = conv_jacobian_rows(layer.float().to(hip_device), ad, Dd).cpu().numpy()
    np.testing.assert_allclose(got.cpu().numpy(), same_on_gpu, rtol=1e-4, atol=1e-5 * np.abs(want).max())


def test_device_rows_take_views_without_changing_a_bit(hip_device):
    from bnn_kfac_amd.variance import conv_jacobian_rows_device
    dev = hip_device
    g, a, D, _ = _normal(SEVEN[1])
    ad, Dd = _dev(dev, a, D)
    layer = _layer(g, dev)
    plain = conv_jacobian_rows_device(layer, ad, Dd)
    # a batch slice x[::2] of a larger batch
    x = torch.randn(2 * g.nb, g.C, g.H, g.W, device=dev)
    x[::2] = ad
    view = x[::2]
    assert not view.is_contiguous() and view.stride(0) == 2 * g.C * g.H * g.W
    assert torch.equal(conv_jacobian_rows_device(layer, view, Dd), plain)
    # D with padded rows, and D with a permuted (copied) inner layout
    wide = torch.full((g.nb, g.nc, g.nG * g.L + 5), float("nan"), device=dev)
    wide[:, :, :g.nG * g.L] = Dd.reshape(g.nb, g.nc, -1)
    Dv = wide[:, :, :g.nG * g.L].view(g.nb, g.nc, g.nG * g.L).unflatten(2, (g.nG, g.Ho, g.Wo))
    assert not Dv.is_contiguous()
    assert torch.equal(conv_jacobian_rows_device(layer, ad, Dv), plain)
    Dt = Dd.transpose(3, 4).contiguous().transpose(3, 4)
    assert not Dt.is_contiguous()
    assert torch.equal(conv_jacobian_rows_device(layer, ad, Dt), plain)
    # an image whose inner dimensions are not contiguous is copied
    at = ad.transpose(2, 3).contiguous().transpose(2, 3)
    assert torch.equal(conv_jacobian_rows_device(layer, at, Dd), plain)
    # no samples
    assert conv_jacobian_rows_device(layer, ad[:0], Dd[:0]).shape == (0, g.nc, g.nA * g.nG)


def test_device_rows_refuse_what_the_kernel_does_not_cover(hip_device):
    from bnn_kfac_amd.variance import conv_jacobian_rows_device
    a = torch.zeros(2, 2, 6, 6, device=hip_device)
    D = torch.zeros(2, 3, 2, 2, 2, device=hip_device)
    for layer in (torch.nn.Conv2d(2, 2, 3, dilation=2), torch.nn.Conv2d(2, 2, 3, groups=2),
                  torch.nn.Conv2d(2, 2, 3, padding="same"),
                  torch.nn.Conv2d(2, 2, 3, padding=1, padding_mode="circular")):
        with pytest.raises(ValueError):
            conv_jacobian_rows_device(layer.to(hip_device), a, D)
    with pytest.raises(ValueError):  # D of another output size
        conv_jacobian_rows_device(torch.nn.Conv2d(2, 2, 3).to(hip_device), a, D)
    with pytest.raises(TypeError):
        conv_jacobian_rows_device(torch.nn.Conv2d(2, 2, 3).to(hip_device), a.double(), D)
