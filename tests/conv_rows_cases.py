"""Integer-exact cases for kfac_cov_conv_rows (a plain helper module, like posterior_cases).

A case is (C, H, W, kh, kw, sh, sw, ph, pw, bias, nG, nb, nc): a Conv2d layer's input
a (nb, C, H, W) and its output Jacobian D (nb, nc, nG, Ho, Wo), both integers in [-2, 2].
Every partial sum of M[k][g] = sum_p patch[p][k] D[g][p] is bounded by 4 L <= 3136 < 2^24, so
the fp32 result is one exact integer whatever the order of summation and the device is
compared with `array_equal`.  The reference is an int64 unfold (written here with slices)
and an int64 einsum, rows in the posterior's order (element k*nG + g, bias row last).

Each case's operands live in ONE NaN-filled fp32 buffer with pitches above the widths
(sample stride C*H*W + 3, ldD = nG*L + 5, ldM = nA*nG + 7), so the GPU test compares the
whole buffer: the written region against the reference, everything else against its prefill."""
import functools
import zlib
from types import SimpleNamespace as NS

import numpy as np

F32 = np.float32
GAP = 8

# (id, (C, H, W, kh, kw, sh, sw, ph, pw, bias, nG, nb, nc)): what the case exercises
CASES = (
    ("L1", (1, 1, 1, 1, 1, 1, 1, 0, 0, True, 1, 1, 1)),                # L = 1, nA = 2
    ("lenet-conv1", (1, 28, 28, 5, 5, 1, 1, 2, 2, True, 6, 3, 10)),    # nA = 26, L = 784: 25 stages, the last partial; 60 columns
    ("lenet-conv2", (6, 14, 14, 5, 5, 1, 1, 0, 0, True, 16, 2, 10)),   # nA = 151: three a-tiles, 23 rows in the last; L = 100; 160 columns
    ("nA64", (7, 6, 5, 3, 3, 1, 1, 1, 1, True, 7, 2, 10)),             # ones column ends a tile, H != W, L = 30 < a stage, 70 columns
    ("nA65", (1, 9, 9, 8, 8, 1, 1, 0, 0, True, 3, 2, 1)),              # ones column alone in the second tile, nc = 1, L = 4
    ("stride2x1-nobias", (3, 11, 8, 3, 2, 2, 1, 1, 0, False, 5, 4, 3)),  # Ho = 6, Wo = 7, padding 1 x 0, no ones row
    ("pad2", (2, 5, 5, 3, 3, 1, 1, 2, 2, True, 4, 2, 2)),              # patches that are all padding
    ("stride3-k2", (1, 9, 9, 2, 2, 3, 3, 0, 0, True, 2, 2, 2)),        # stride larger than the kernel
    ("L33", (1, 1, 33, 1, 1, 1, 1, 0, 0, True, 2, 2, 2)),              # one position past a stage
    ("L65", (1, 5, 13, 1, 1, 1, 1, 0, 0, True, 2, 2, 2)),              # one position past two stages
    ("nb70", (2, 4, 4, 3, 3, 1, 1, 1, 1, True, 3, 70, 2)),             # many samples
    ("nc40", (1, 4, 4, 3, 3, 1, 1, 1, 1, True, 3, 2, 40)),             # the rows call has no class cap
)
IDS = [cid for cid, _ in CASES]


def geometry(spec):
    C, H, W, kh, kw, sh, sw, ph, pw, bias, nG, nb, nc = spec
    Ho, Wo = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
    cols = C * kh * kw
    return NS(C=C, H=H, W=W, kh=kh, kw=kw, sh=sh, sw=sw, ph=ph, pw=pw, bias=bool(bias), nG=nG, nb=nb, nc=nc,
              Ho=Ho, Wo=Wo, L=Ho * Wo, cols=cols, nA=cols + int(bool(bias)))


def unfold(a, g):
    """F.unfold(a, (kh, kw), padding=(ph, pw), stride=(sh, sw)) for any dtype: (n, cols, L),
    feature k = ch*kh*kw + ki*kw + kj, position p = oh*Wo + ow."""
    n = a.shape[0]
    ap = np.pad(a, ((0, 0), (0, 0), (g.ph, g.ph), (g.pw, g.pw)))
    out = np.empty((n, g.C, g.kh, g.kw, g.Ho, g.Wo), dtype=a.dtype)
    for ki in range(g.kh):
        for kj in range(g.kw):
            out[:, :, ki, kj] = ap[:, :, ki:ki + g.sh * (g.Ho - 1) + 1:g.sh, kj:kj + g.sw * (g.Wo - 1) + 1:g.sw]
    return out.reshape(n, g.cols, g.L)


def rows_reference(a, D, g):
    """(n, nc, nA*nG) in a's dtype (int64 or float64): M[b, c][k][g] = sum_p unfold[b][k][p]
    D[b, c][g][p], then the bias row sum_p D[b, c][g][p]."""
    n, nc = D.shape[0], D.shape[1]
    Dp = D.reshape(n, nc, g.nG, g.L)
    M = np.einsum("bkp,bcgp->bckg", unfold(a, g), Dp)
    if g.bias:
        M = np.concatenate([M, Dp.sum(-1)[:, :, None, :]], axis=2)
    return M.reshape(n, nc, g.nA * g.nG)


def _block(flat, off, rows, cols, ld):
    return off + np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]


@functools.lru_cache(maxsize=None)
def case(cid):
    """The case's data, its flat buffer and where everything sits in it (elements)."""
    g = geometry(dict(CASES)[cid])
    rng = np.random.default_rng(zlib.crc32(repr(("conv_rows", cid)).encode()))
    a = rng.integers(-2, 3, size=(g.nb, g.C, g.H, g.W)).astype(np.int64)
    D = rng.integers(-2, 3, size=(g.nb, g.nc, g.nG, g.Ho, g.Wo)).astype(np.int64)
    chw = g.C * g.H * g.W
    c = NS(id=cid, g=g, a=a, D=D, sB=chw + 3, ldD=g.nG * g.L + 5, ldM=g.nA * g.nG + 7)
    c.oA = GAP
    c.oD = c.oA + g.nb * c.sB + GAP
    c.oM = c.oD + g.nb * g.nc * c.ldD + GAP
    c.size = c.oM + g.nb * g.nc * c.ldM + GAP
    flat = np.full(c.size, np.nan, dtype=F32)
    flat[_block(flat, c.oA, g.nb, chw, c.sB)] = a.reshape(g.nb, chw)
    flat[_block(flat, c.oD, g.nb * g.nc, g.nG * g.L, c.ldD)] = D.reshape(g.nb * g.nc, g.nG * g.L)
    c.flat = flat
    c.ref = rows_reference(a, D, g)
    want = flat.copy()
    want[_block(flat, c.oM, g.nb * g.nc, g.nA * g.nG, c.ldM)] = c.ref.reshape(g.nb * g.nc, g.nA * g.nG)
    c.want = want
    for t in (a, D, flat, want, c.ref):
        t.setflags(write=False)
    return c


def bound(c):
    """The largest magnitude a partial sum of the case can reach: |patch| |D| summed over p."""
    g = c.g
    P = np.abs(unfold(c.a, g))
    if g.bias:
        P = np.concatenate([P, np.ones((g.nb, 1, g.L), dtype=np.int64)], axis=1)
    return int(np.einsum("bkp,bcgp->bckg", P, np.abs(c.D).reshape(g.nb, g.nc, g.nG, g.L)).max())


def same(a, b):
    """Equal element for element, NaN matching NaN."""
    return np.array_equal(np.asarray(a, dtype=F32), np.asarray(b, dtype=F32), equal_nan=True)


def operand(N, g, ptr, nb, sB=None):
    """The KFAC_PATCH operand of nb images of geometry g at `ptr`, as _native.patch_operand
    fills it."""
    op = N.Operand()
    op.ptr, op.layout = ptr, N.PATCH
    op.C, op.H, op.W, op.kh, op.kw, op.sh, op.sw, op.ph, op.pw, op.Ho, op.Wo = \
        g.C, g.H, g.W, g.kh, g.kw, g.sh, g.sw, g.ph, g.pw, g.Ho, g.Wo
    op.L = g.L
    op.sB = g.C * g.H * g.W if sB is None else sB
    op.rows = nb * g.L
    op.cols = g.cols
    op.has_ones = int(g.bias)
    return op


def job(N, g, nb, a_ptr, D_ptr, M_ptr, sB=None, ldD=None, ldM=None):
    """kfac_cov_conv_rows_job for nb samples of geometry g (contiguous pitches by default)."""
    return N.CovConvRowsJob(operand(N, g, a_ptr, nb, sB), D_ptr, g.nG * g.L if ldD is None else ldD, g.nG, 0,
                            M_ptr, g.nA * g.nG if ldM is None else ldM)


def case_job(N, c, base):
    """The job of case c on its flat buffer uploaded at byte address `base`."""
    return job(N, c.g, c.g.nb, base + 4 * c.oA, base + 4 * c.oD, base + 4 * c.oM, c.sB, c.ldD, c.ldM)
