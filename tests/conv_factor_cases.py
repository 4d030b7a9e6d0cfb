"""Integer-exact cases for the conv factor kernels (a plain helper module, like posterior_cases).

kfac_factor_conv (both layouts), kfac_factor_conv_x3 / _x3s / _x3f, kfac_factor_channel_small /
_channel_x3 and the PATCH / CHANNEL instances of kfac_factor_tiles, through the raw C ABI:
F = beta F + alpha X~^T X~ of an im2col (KFAC_PATCH) or channel-major (KFAC_CHANNEL) operand.

Data rules
  * every input is an integer in [-3, 3] held in fp32: its bf16x3 mid and lo parts are zero, every
    product is an integer of magnitude <= 9 and every partial sum, in any order, an integer of
    magnitude <= 9 K (K the job's rows over all its batches and updates).  9 K < 2^24 (asserted by
    the host test), alpha is 1 or 0.5 and the prefill an integer of magnitude <= 4, so F is one
    well-defined fp32 number whatever the summation order, and the device is compared with
    `array_equal`.
  * the images of a batch lie `sB` apart in ONE flat NaN-filled buffer, at least 64 NaN floats
    before the first and after the last: sB = C H W + 3 (PATCH), n L + 4 (CHANNEL on the staged
    kernels, whose float4 loads need it) or n L + 3 (CHANNEL fallback cases).  A read outside an
    image is then a NaN in F, not whatever memory happened to hold.
  * F sits at float 64 of a NaN-filled buffer with ldF = n + 3; beta = 0 writes onto the NaNs,
    beta = 1 onto a symmetric non-zero integer prefill of the n x n region.  The whole buffer is compared.

`reference`  int64 X~^T X~ from a gather written from the header's addressing formula
             (include/kfac_hip.h, "factors"), summed over the case's updates.
`expected`   the whole F buffer that reference gives.
`model_factor(case, mistake)`  what the kernels do -- a per-image offset table, image bases
             from the batch and the sample stride, tasks owning whole images, the epilogue --
             restated in numpy with one planted mistake (MISTAKES).  test_conv_factor_cases_host.py
             asserts model(None) == expected for every case and model(m) != expected for every
             case the predicate of m names.

Routing (`kfac_factor_route`) and the K-split plan (`kfac_factor_accum_plan`) are host-only calls,
so the sweep is selected, and every expectation built, without a device."""
import itertools
import zlib
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace as NS

import numpy as np

F32 = np.float32
GUARD = 64     # NaN floats before the first image and after the last
F_OFF = 64     # F's offset in its NaN-filled buffer (floats; keeps F 16-byte aligned)
BASE = 0x100000  # fake device address of a buffer (host-only calls), 16-byte aligned
# kfac_prof_id -> family
FAMILY = {0: "tiles", 6: "conv", 7: "channel_small", 9: "conv_x3", 10: "conv_x3s", 11: "conv_x3f",
          12: "channel_x3"}
PATCH_FAMILIES = ("conv", "conv_x3", "conv_x3s", "conv_x3f", "tiles")
STAGED = ("conv", "conv_x3", "conv_x3s", "conv_x3f", "channel_small", "channel_x3")  # tasks own whole images


def _rng(*tag):
    return np.random.default_rng(zlib.crc32(repr(tag).encode()))


def _native():
    from bnn_kfac_amd import _native as N
    return N


# --------------------------------------------------------------------------- cases
def patch_case(cid, B, C, H, W, k, s=(1, 1), p=(0, 0), bias=True, **kw):
    (kh, kw_), (sh, sw), (ph, pw) = k, s, p
    Ho, Wo = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw_) // sw + 1
    cols = C * kh * kw_
    c = NS(id=cid, layout="patch", C=C, H=H, W=W, kh=kh, kw=kw_, sh=sh, sw=sw, ph=ph, pw=pw, Ho=Ho, Wo=Wo,
           L=Ho * Wo, cols=cols, ones=bool(bias), n=cols + int(bool(bias)), img=C * H * W)
    c.sB = c.img + 3
    return _finish(c, B, **kw)


def channel_case(cid, B, n, L, ones=False, staged=True, **kw):
    c = NS(id=cid, layout="channel", cols=n, L=L, ones=bool(ones), n=n + int(bool(ones)), img=n * L)
    c.sB = c.img + (4 if staged else 3)
    return _finish(c, B, **kw)


def _finish(c, B, mode="sweep", alpha=1.0, beta=0.0, batches=None, steps=None, guard=GUARD, sB=None):
    """batches: images per batch (a multi-batch job: one buffer per batch); steps: images of each
    deferred update (each reads the first m images of the one batch)."""
    c.mode, c.alpha, c.beta, c.guard = mode, float(alpha), float(beta), guard
    c.batches = tuple(batches) if batches else (B,)
    c.steps = tuple(steps) if steps else None
    c.B = sum(c.batches)
    if sB is not None:
        c.sB = sB
    c.ldF = c.n + 3
    return c


def with_batch(case, B):
    """The same single-batch case at another image count (its own data)."""
    c = NS(**vars(case))
    c.id, c.batches, c.B = f"{case.id}/B{B}", (B,), B
    for k in ("family", "splits"):
        vars(c).pop(k, None)
    return c


def updates(case):
    """[(images per batch, batches, acc_beta)] of the case's kfac_factor_update calls."""
    if case.steps:
        return [(m, 1, 0.0 if u == 0 else 1.0) for u, m in enumerate(case.steps)]
    return [(case.batches[0], len(case.batches), 0.0)]


def krows(case):
    return sum(m * nb for m, nb, _ in updates(case)) * case.L


# ----------------------------------------------------------------------------- data
_INPUTS, _REF = {}, {}


def inputs(case):
    """One flat fp32 buffer per batch: NaN everywhere but the images."""
    if case.id not in _INPUTS:
        rng = _rng("x", case.id)
        bufs = []
        for Bs in case.batches:
            buf = np.full(case.guard + (Bs - 1) * case.sB + case.img + GUARD, np.nan, dtype=F32)
            at = case.guard + np.arange(Bs)[:, None] * case.sB + np.arange(case.img)[None, :]
            buf[at] = rng.integers(-3, 4, size=at.shape)
            bufs.append(buf)
        _INPUTS[case.id] = bufs
    return _INPUTS[case.id]


def f_buffer(case):
    """The NaN-filled F buffer (fp32), its n x n region prefilled with symmetric integers when
    beta = 1."""
    n, ld = case.n, case.ldF
    buf = np.full(F_OFF + n * ld + GUARD, np.nan, dtype=F32)
    if case.beta != 0.0:
        P = _rng("F", case.id).integers(1, 5, size=(n, n)) * _rng("Fs", case.id).choice([-1, 1], size=(n, n))
        P = np.tril(P) + np.tril(P, -1).T
        buf[F_OFF + np.arange(n)[:, None] * ld + np.arange(n)[None, :]] = P
    return buf


def _region(case, ld=None):
    ld = case.ldF if ld is None else ld
    return F_OFF + np.arange(case.n)[:, None] * ld + np.arange(case.n)[None, :]


# ------------------------------------------------------------------------ reference
def _ref_rows(case, buf, nimg):
    """X~ (nimg L x n) of one batch by the header's formula, element by element:
       KFAC_CHANNEL: ptr[(k/L)*sB + (k%L) + i*L]
       KFAC_PATCH  : k = b*L + oh*Wo + ow, i = c*kh*kw + ki*kw + kj -> x[b, c, oh*sh+ki-ph, ow*sw+kj-pw]
                     (0 outside the image), x[b] at ptr + b*sB."""
    c = case
    k = np.arange(nimg * c.L, dtype=np.int64)[:, None]
    i = np.arange(c.cols, dtype=np.int64)[None, :]
    ptr = c.guard
    if c.layout == "channel":
        X = buf[ptr + (k // c.L) * c.sB + (k % c.L) + i * c.L].astype(np.float64)
    else:
        b, pos = k // c.L, k % c.L
        oh, ow = pos // c.Wo, pos % c.Wo
        ch, r = i // (c.kh * c.kw), i % (c.kh * c.kw)
        ki, kj = r // c.kw, r % c.kw
        h, w = oh * c.sh + ki - c.ph, ow * c.sw + kj - c.pw
        inside = (h >= 0) & (h < c.H) & (w >= 0) & (w < c.W)
        at = ptr + b * c.sB + (ch * c.H + h) * c.W + w
        X = np.where(inside, buf[np.where(inside, at, 0)], 0.0).astype(np.float64)
    if c.ones:
        X = np.concatenate([X, np.ones((X.shape[0], 1))], axis=1)
    assert np.isfinite(X).all(), case.id
    return X


def reference(case):
    """int64 X~^T X~ over every update of the case."""
    if case.id not in _REF:
        bufs = inputs(case)
        S = np.zeros((case.n, case.n))
        for m, nb, _ in updates(case):
            for s in range(nb):
                X = _ref_rows(case, bufs[s], m)
                S += X.T @ X  # (exact in fp64: integers below 2^53)
        Si = np.rint(S).astype(np.int64)
        assert np.array_equal(Si, S)
        _REF[case.id] = Si
    return _REF[case.id]


def expected(case):
    """The whole F buffer after the case, in fp64 (NaN outside the n x n region)."""
    buf = f_buffer(case).astype(np.float64)
    at = _region(case)
    S = reference(case).astype(np.float64)
    buf[at] = case.alpha * S if case.beta == 0.0 else case.beta * buf[at] + case.alpha * S
    return buf


def images(case, s=0):
    """Batch s as a logical array: (B, C, H, W) or (B, n, L)."""
    buf = inputs(case)[s]
    Bs = case.batches[s]
    x = buf[case.guard + np.arange(Bs)[:, None] * case.sB + np.arange(case.img)[None, :]]
    return x.reshape((Bs, case.C, case.H, case.W) if case.layout == "patch" else (Bs, case.cols, case.L))


# ---------------------------------------------------------------------------- model
def _offsets(case, mistake):
    """Per position and column: the offset inside an image (-1: a zero), as the staged kernels
    tabulate it once per task."""
    c = case
    i = np.arange(c.cols)
    pos = np.arange(c.L)
    if c.layout == "channel":
        return pos[:, None] + i[None, :] * c.L
    ph, pw = (c.pw, c.ph) if mistake == "pad_swapped" else (c.ph, c.pw)
    sh, sw = (c.sw, c.sh) if mistake == "stride_swapped" else (c.sh, c.sw)
    kk = c.kh * c.kw
    ch, r = i // kk, i % kk
    kwd = c.kh if mistake == "kernel_swapped" else c.kw  # the column decode's divisor
    ki, kj = r // kwd, r % kwd
    oh, ow = pos // c.Wo, pos % c.Wo
    h = oh[:, None] * sh + ki[None, :] - ph
    w = ow[:, None] * sw + kj[None, :] - pw
    inside = (h >= 0) & (h < c.H) & (w >= 0) & (w < c.W)
    flat = (ch[None, :] * c.H + h) * c.W + w
    if mistake == "record_sB":
        # bottom / right padding addressed flat and zeroed by the record bound alone: a bound
        # of sB instead of C H W lets the three floats behind the image through
        inside |= (h >= 0) & (w >= 0) & ((h >= c.H) | (w >= c.W)) & (flat >= c.img) & (flat < c.sB)
    return np.where(inside, flat, -1)


def _task_images(case, B, bseg, splits, mistake):
    """Which of a launch's B images its tasks read: task s owns [s B / splits, (s+1) B / splits)."""
    keep = np.zeros(B, dtype=bool)
    for s in range(splits):
        b0, b1 = s * B // splits, (s + 1) * B // splits
        if mistake == "uneven_last_dropped" and b1 - b0 > B // splits:
            b1 -= 1
        if mistake == "stops_at_batch" and b1 > b0 and (b1 - 1) // bseg != b0 // bseg:
            b1 = (b0 // bseg + 1) * bseg
        keep[b0:b1] = True
    return keep


def model_factor(case, mistake=None):
    """The whole F buffer (fp64) as the kernels produce it, with one planted mistake."""
    c = case
    assert mistake is None or mistake in MISTAKES, mistake
    bufs = inputs(c)
    off = _offsets(c, mistake)
    posmask = np.ones(c.L, dtype=bool)
    if mistake == "last_row_dropped":
        posmask &= np.arange(c.L) // c.Wo != c.Ho - 1
    if mistake == "last_col_dropped":
        posmask &= np.arange(c.L) % c.Wo != c.Wo - 1
    sB = c.img if mistake == "sB_contiguous" else c.sB
    staged = c.family in STAGED
    ups = updates(c)
    S = np.zeros((c.n, c.n))
    for u, (m, nb, _) in enumerate(ups):
        B = m * nb
        keep = _task_images(c, B, m, c.splits, mistake) if staged else np.ones(B, dtype=bool)
        if mistake == "empty_task_zeroes" and staged:
            # a slab zeroed by a later update's task without an image loses this update's share
            for m2, nb2, _ in ups[u + 1:]:
                B2 = m2 * nb2
                for s in range(c.splits):
                    if s * B2 // c.splits == (s + 1) * B2 // c.splits:
                        keep[s * B // c.splits:(s + 1) * B // c.splits] = False
        for b in np.flatnonzero(keep):
            seg, bi = divmod(int(b), m)
            buf = bufs[0 if mistake == "batch_base0" else seg]
            base = c.guard + bi * sB
            X = np.where(off >= 0, buf[base + np.maximum(off, 0)], 0.0).astype(np.float64)
            if c.ones:
                one = np.ones((c.L, 1))
                if mistake == "ones_per_image":
                    one[1:] = 0.0
                X = np.concatenate([X, one], axis=1)
            X = X[posmask]
            S += X.T @ X
    alpha = c.alpha * c.alpha if mistake == "alpha_twice" else c.alpha
    beta = 0.0 if mistake == "beta_ignored" else c.beta
    buf = f_buffer(c).astype(np.float64)
    at = _region(c, c.n if mistake == "ldF_as_n" else None)
    buf[at] = alpha * S if beta == 0.0 else beta * buf[at] + alpha * S
    return buf


def _pads_past_image(c):
    """A read of the bottom or right padding lands in [C H W, sB) when addressed flat."""
    if c.layout != "patch":
        return False
    hs = {oh * c.sh + ki - c.ph for oh in range(c.Ho) for ki in range(c.kh)}
    ws = {ow * c.sw + kj - c.pw for ow in range(c.Wo) for kj in range(c.kw)}
    return any((h >= c.H or w >= c.W) and h >= 0 and w >= 0 and
               c.img <= ((c.C - 1) * c.H + h) * c.W + w < c.sB for h in hs for w in ws)


def _straddles(c):
    """A task of the multi-batch launch owns images of two batches."""
    if len(c.batches) == 1 or c.family not in STAGED:
        return False
    m = c.batches[0]
    return any((s + 1) * c.B // c.splits > s * c.B // c.splits and
               ((s + 1) * c.B // c.splits - 1) // m != (s * c.B // c.splits) // m for s in range(c.splits))


_patch = lambda c: c.layout == "patch"
# mistake -> the cases that must show it
MISTAKES = {
    "sB_contiguous": lambda c: min(m for m, _, _ in updates(c)) > 1,
    "record_sB": _pads_past_image,
    "pad_swapped": lambda c: _patch(c) and c.ph != c.pw,
    # (one output row and one column: the strides multiply nothing)
    "stride_swapped": lambda c: _patch(c) and c.sh != c.sw and (c.Ho > 1 or c.Wo > 1),
    "kernel_swapped": lambda c: _patch(c) and c.kh != c.kw,
    "last_row_dropped": _patch,
    "last_col_dropped": _patch,
    "ones_per_image": lambda c: c.ones and c.L > 1,
    "uneven_last_dropped": lambda c: c.mode == "large" and c.B % c.splits != 0,
    "empty_task_zeroes": lambda c: c.mode == "deferred",
    "batch_base0": lambda c: len(c.batches) > 1,
    "stops_at_batch": _straddles,
    "beta_ignored": lambda c: c.beta != 0.0,
    "alpha_twice": lambda c: c.alpha != 1.0,
    "ldF_as_n": lambda c: c.n > 1,
}


# ------------------------------------------------------------------- jobs and routes
def operand(N, case, ptr, nimg):
    """The kfac_operand of `nimg` images per batch, image 0 at `ptr`."""
    c = case
    op = N.Operand()
    op.ptr, op.cols, op.L, op.sB, op.rows, op.has_ones = ptr, c.cols, c.L, c.sB, nimg * c.L, int(c.ones)
    if c.layout == "patch":
        op.layout = N.PATCH
        op.C, op.H, op.W, op.kh, op.kw, op.sh, op.sw, op.ph, op.pw, op.Ho, op.Wo = \
            c.C, c.H, c.W, c.kh, c.kw, c.sh, c.sw, c.ph, c.pw, c.Ho, c.Wo
    else:
        op.layout = N.CHANNEL
    return op


def job(N, case, ptrs, F_ptr, nimg=None, nb=None):
    """(kfac_factor_job, keepalive) over `nb` batches of `nimg` images, batch s's image 0 at
    ptrs[s]; F_ptr the address of F[0][0]."""
    nimg = case.batches[0] if nimg is None else nimg
    nb = len(case.batches) if nb is None else nb
    j = N.FactorJob()
    j.x, j.alpha, j.beta, j.F, j.ldF = operand(N, case, ptrs[0], nimg), case.alpha, case.beta, F_ptr, case.ldF
    keep = None
    if nb > 1:
        keep = N.segment_table(list(ptrs[:nb]))
        j.seg_ptrs, j.nseg = N.table_ptr(keep), nb
    return j, keep


def fake_ptrs(case):
    return [BASE + (s << 26) + 4 * case.guard for s in range(len(case.batches))]


def host_job(N, case):
    """The case's first update with fake addresses (host-only calls)."""
    m, nb, _ = updates(case)[0]
    return job(N, case, fake_ptrs(case), BASE + (1 << 30) + 4 * F_OFF, m, nb)


def route(cases, plan=True):
    """Sets case.family (kfac_factor_route) and, with `plan`, case.splits (kfac_factor_accum_plan)
    of each.  Both are host-only calls that drop the GIL, so a long list goes to eight threads."""
    N = _native()

    def chunk_route(chunk):
        built = [host_job(N, c) for c in chunk]
        jobs = [b[0] for b in built]
        for c, f in zip(chunk, N.factor_route(jobs)):
            c.family = FAMILY[f]
        if plan:
            for c, (s, _) in zip(chunk, N.factor_accum_plan(jobs)):
                c.splits = int(s)

    chunks = [cases[i:i + 1024] for i in range(0, len(cases), 1024)]
    with ThreadPoolExecutor(8) as pool:
        list(pool.map(chunk_route, chunks))
    return cases


def launches(case):
    """Launches of the case's family the profile must count."""
    if case.steps:
        return len(case.steps)
    return len(case.batches) if case.family == "tiles" else 1


# ---------------------------------------------------------------------- PATCH sweep
GRID = dict(
    C=(1, 2, 3, 4, 6, 9, 20),
    HW=((5, 5), (6, 9), (7, 8), (9, 9), (10, 11), (11, 13), (12, 16), (14, 14), (15, 15), (20, 20), (27, 26),
        (28, 28), (32, 32)),
    k=((1, 1), (2, 2), (3, 3), (3, 4), (3, 5), (4, 3), (5, 5), (6, 6), (4, 8), (2, 7)),
    s=((1, 1), (2, 1), (1, 2), (2, 2), (1, 3), (3, 2)),
    p=((0, 0), (1, 1), (0, 1), (1, 2), (2, 0), (2, 2)),
    bias=(True, False))
FLOORS = {"conv": 100, "conv_x3": 100, "conv_x3s": 80, "conv_x3f": 40, "tiles": 60}


def candidates():
    out = []
    for C, (H, W), k, s, p, bias in itertools.product(*GRID.values()):
        if p[0] < k[0] and p[1] < k[1] and k[0] <= H + 2 * p[0] and k[1] <= W + 2 * p[1]:
            out.append(patch_case(f"p{len(out)}", 3, C, H, W, k, s, p, bias))
    return out


def _cdiv(a, b):
    return -(-a // b)


def family_class(c):
    """The family-specific part of a sweep key."""
    nb = _cdiv(c.n, 32)
    return {"conv_x3s": lambda: (_cdiv(c.Wo, 8), c.kw % 2 == 1),
            "conv_x3f": lambda: (nb, len({(4 - ki * c.Wo % 4) % 4 for ki in range(c.kh)})),
            "conv_x3": lambda: (_cdiv(nb * (nb + 1) // 2, 8), c.L > 256),
            "conv": lambda: (0 if c.n <= 16 else 1 if c.n <= 32 else 2, c.img > 1024),
            "tiles": lambda: min(nb, 3)}[c.family]()


def _cls(a, b, unit):
    return "none" if (a, b) == unit else "equal" if a == b else "unequal"


def sweep_key(c):
    return (_cls(c.sh, c.sw, (1, 1)), _cls(c.ph, c.pw, (0, 0)), c.kh != c.kw, c.ones, c.family, family_class(c))


_CACHE = {}


def _once(name, make):
    if name not in _CACHE:
        _CACHE[name] = make()
    return _CACHE[name]


def patch_sweep():
    """(kept cases, {family: candidates routed there}, {family: the family-specific classes of
    those candidates}): the first candidate of every key is kept."""
    def make():
        fixed()  # (routed first: see fixed())
        cands = route(candidates(), plan=False)
        routed, classes, kept, seen = {}, {}, [], set()
        for c in cands:
            routed[c.family] = routed.get(c.family, 0) + 1
            key = sweep_key(c)
            classes.setdefault(c.family, set()).add(key[-1])
            if key not in seen:
                seen.add(key)
                c.key = key
                kept.append(c)
        route(kept)
        for i, c in enumerate(kept):
            c.id = "patch[%d,%dx%d,k%dx%d,s%dx%d,p%dx%d,%s]" % (
                c.C, c.H, c.W, c.kh, c.kw, c.sh, c.sw, c.ph, c.pw, "bias" if c.ones else "nobias")
            c.alpha, c.beta = (1.0, 0.5)[i % 2], (0.0, 1.0)[i // 2 % 2]
        return kept, routed, classes
    return _once("patch", make)


# -------------------------------------------------------------------- CHANNEL sweep
CH_N = {"channel_small": (1, 2, 3, 4, 5, 6, 7, 8), "channel_x3": (9, 11, 16, 17, 31, 32),
        "conv": (33, 40, 64, 65, 96)}
CH_L = (4, 12, 16, 20, 36, 100, 196)


def channel_sweep():
    """Staged cases (B = 3 and 5, every n of CH_N at every L of CH_L the staged kernels take) and
    the fallbacks to kfac_factor_tiles, each for its own reason."""
    def make():
        grid = [(B, n, L) for B in (3, 5) for ns in CH_N.values() for n in ns for L in CH_L]
        cases = route([channel_case(f"channel[B{B},n{n},L{L}]", B, n, L) for B, n, L in grid])
        staged = [c for c in cases if c.family != "tiles"]  # (n L > 8,192: among the fallbacks below)
        fb = []
        for B in (3, 5):
            for n in (3, 6, 16, 40):
                for L in (1, 9):
                    fb.append(channel_case(f"channel[B{B},n{n},L{L},L%4]", B, n, L, staged=False))
                fb.append(channel_case(f"channel[B{B},n{n},L16,sB%4]", B, n, 16, staged=False))
            # (each of these with sB = n L + 4 too, so that the reason named is the only one)
            for st in (False, True):
                tag = "" if not st else ",sB+4"
                for n in (3, 6, 16, 40):
                    fb.append(channel_case(f"channel[B{B},n{n},L16{tag},base+1]", B, n, 16, staged=st, guard=GUARD + 1))
                for n in (6, 16):
                    fb.append(channel_case(f"channel[B{B},n{n},L16{tag},ones]", B, n, 16, ones=True, staged=st))
                fb.append(channel_case(f"channel[B{B},n96,L196{tag},large]", B, 96, 196, staged=st))
        for c in fb:
            c.fallback = c.id.rstrip("]").split(",")[-1]
        route(fb)
        out = staged + fb
        for i, c in enumerate(out):
            c.alpha, c.beta = (1.0, 0.5)[i % 2], (0.0, 1.0)[i // 2 % 2]
        return out
    return _once("channel", make)


# ------------------------------------------------- large, multi-batch, deferred cases
# (name, builder at B images, expected family): K-splits with fewer splits than images and
# B % splits != 0, so tasks own two or three images, and not all the same number
LARGE = (
    ("x3s", lambda B, **kw: patch_case("", B, 1, 12, 12, (5, 5), p=(2, 2), **kw), 259, "conv_x3s"),
    ("x3f_n101", lambda B, **kw: patch_case("", B, 4, 8, 8, (5, 5), p=(1, 1), **kw), 259, "conv_x3f"),
    ("x3", lambda B, **kw: patch_case("", B, 2, 9, 9, (5, 5), p=(2, 2), **kw), 259, "conv_x3"),
    ("fp32_n10", lambda B, **kw: patch_case("", B, 1, 6, 6, (3, 3), p=(1, 1), **kw), 1029, "conv"),
    ("fp32_n224", lambda B, **kw: patch_case("", B, 14, 9, 9, (4, 4), bias=False, **kw), 259, "conv"),
    ("small_n6", lambda B, **kw: channel_case("", B, 6, 16, **kw), 515, "channel_small"),
    ("small_n3", lambda B, **kw: channel_case("", B, 3, 16, **kw), 1030, "channel_small"),
    # (1030 = 2 x 515: every task two images; 1029 gives the family its uneven tasks)
    ("chx3_n16", lambda B, **kw: channel_case("", B, 16, 12, **kw), 1030, "channel_x3"),
    ("chx3_n16_odd", lambda B, **kw: channel_case("", B, 16, 12, **kw), 1029, "channel_x3"),
    ("chfp32_n40", lambda B, **kw: channel_case("", B, 40, 16, **kw), 1029, "conv"),
)


def fixed():
    """{mode: cases} of the large shapes: immediate ("large"), multi-batch ("multi": three
    batches in three buffers, 87 images each where B = 259 and 343 otherwise, an odd batch
    boundary a two-image task straddles; and the tiles fallback, one launch per batch) and
    deferred (updates of B, 7 and B - 1 images into an accumulator planned at B, then the flush).
    Routed before the sweep's candidates, so kfac_factor_conv_x3f's 64-entry geometry memo holds
    the x3f shape: its modes differ in B alone and are served from the memo."""
    def make():
        out = {"large": [], "multi": [], "deferred": []}
        for i, (name, make_case, B, fam) in enumerate(LARGE):
            alpha = (1.0, 0.5)[i % 2]
            per = 87 if B == 259 else 343
            for mode, kw in (("large", dict(beta=float(i // 2 % 2))),
                             ("multi", dict(batches=(per,) * 3, beta=float((i + 1) // 2 % 2), alpha=1.5 - alpha)),
                             ("deferred", dict(steps=(B, 7, B - 1), beta=1.0))):
                c = make_case(B, mode=mode, **dict(dict(alpha=alpha), **kw))
                c.id, c.want_family = f"{mode}[{name}]", fam
                out[mode].append(c)
        c = patch_case("multi[tiles]", 3, 3, 27, 26, (3, 5), s=(2, 1), p=(1, 2), mode="multi", batches=(3, 3, 3),
                       alpha=0.5, beta=1.0)
        c.want_family = "tiles"
        out["multi"].append(c)
        for cases in out.values():
            route(cases)
        return out
    return _once("fixed", make)


def all_cases():
    f = fixed()
    return patch_sweep()[0] + channel_sweep() + f["large"] + f["multi"] + f["deferred"]
