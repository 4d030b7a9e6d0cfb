"""Integer-exact cases for the row-major update path (a plain helper module, like conv_factor_cases).

kfac_factor_update is more than a launch for row-major (Linear-layer) factors: the host side
(csrc/factor.hip) cuts a call's row-major jobs into groups of MAXJ, routes each group to
kfac_factor_tiles / kfac_factor_tiles_x3 / kfac_factor_syrk3, splits a ragged multi-batch job
into a head and a tail launch (unless the group runs on tiles_x3 within KSEG batch bases), and
cuts a group of more than KSEG batch bases into rounds.  Every case here is one call (or one
call and one kfac_factor_flush) through the raw C ABI whose whole F buffers are known exactly.

Data rules
  * every input is an integer in [-3, 3] held in fp32 (one bf16 value: the bf16x3 mid and lo
    parts are zero), every alpha a power of two, every ragged job's rows / last_rows a power of
    two, beta in {0, 1, 0.5} and the prefill a symmetric integer matrix.  `bound(case)` is an
    int64 evaluation on absolute values, in units of the finest power of two that occurs; below
    2^24 (asserted by the host test) every fp32 partial sum is exact in any order, on the fp32
    and the bf16x3 kernels alike, so the device is compared with `array_equal`.
  * every batch of every job lies in its own NaN-filled slot of ONE flat buffer, GUARD NaN floats
    either side, rows `ld` >= cols apart; the rows past last_rows of a ragged batch are NaN.
  * every F sits in a NaN-filled slot of one flat buffer, ldF = n + 3, GUARD NaN floats either
    side; beta = 0 writes onto NaN, beta != 0 onto the prefill.  The whole buffer is compared.

`reference(case)`           {job: int64-exact F} from the header comment of factor.hip:
                            F = beta F0 + alpha sum_b w_b X~_b^T X~_b, w_b = rows / last_rows for
                            the ragged batch and 1 otherwise.
`plan(case)`                a Python model of launch_groups + update_group: the sub-launches of
                            the call in order, each with the family kfac_factor_route gives for
                            exactly its jobs.
`reference(case, mistake)`  the result of walking that plan, launch by launch and K-split by
                            K-split, with one planted mistake (MISTAKES); without a mistake the
                            walk reproduces the reference (asserted by the host test)."""
import zlib
from fractions import Fraction
from types import SimpleNamespace as NS

import numpy as np

F32 = np.float32
GUARD = 64        # NaN floats either side of every batch and every F
BASE = 0x10000000  # fake device address of a buffer (host-only calls), 256-byte aligned
MAXJ, KSEG, BK, TILE = 16, 64, 32, 64  # csrc/factor_common.h, kfac_common.h
FAMILY = {0: "tiles", 4: "syrk3", 5: "tiles_x3", 7: "channel_small", 12: "channel_x3", 6: "conv"}
REDUCE = 1        # KFAC_PROF_FACTOR_REDUCE


def _rng(*tag):
    return np.random.default_rng(zlib.crc32(repr(tag).encode()))


def _native():
    from bnn_kfac_amd import _native as N
    return N


def _cdiv(a, b):
    return -(-a // b)


# ----------------------------------------------------------------------------- cases
def J(cols, ones=0, pad=0, off=0, batches=(32,), alpha=1.0, beta=0.0, splits=2, into=None):
    """One job: `cols` columns (+ the ones column), rows `cols + pad` floats apart, batch s's base
    `off` (or off[s]) floats past a 16-byte boundary, `batches` rows per batch (all equal but a
    shorter last one: the ragged batch).  Deferred cases: `splits` = acc_splits; `into` = the job
    whose F and accumulator this job shares (it takes the next slab range: acc_stride)."""
    batches = tuple(batches)
    assert all(b == batches[0] for b in batches[:-1]) and batches[-1] <= batches[0]
    offs = tuple(off) if isinstance(off, (tuple, list)) else (off,) * len(batches)
    return NS(layout="rowmajor", cols=cols, ones=int(bool(ones)), n=cols + int(bool(ones)), ld=cols + pad,
              offs=offs, batches=batches, rows=batches[0],
              last=batches[-1] if len(batches) > 1 and batches[-1] < batches[0] else 0,
              alpha=float(alpha), beta=float(beta), splits=splits, into=into)


def CH(n, L, B, alpha=1.0, beta=0.0, splits=2):
    """A small channel-major (KFAC_CHANNEL) job: B images of n channels x L positions, sB = n L + 4."""
    return NS(layout="channel", cols=n, ones=0, n=n, L=L, sB=n * L + 4, ld=0, offs=(0,), batches=(B * L,),
              rows=B * L, last=0, alpha=float(alpha), beta=float(beta), splits=splits, into=None)


def ragged(j):
    return j.last > 0


def rw(j):
    return Fraction(j.rows, j.last) if ragged(j) else Fraction(1)


def case(cid, block, jobs, deferred=False, **want):
    """want: families=(...) the families the plan must use, in order of first use; launches=k."""
    c = NS(id=cid, block=block, jobs=list(jobs), deferred=deferred, want=want)
    for j in c.jobs:
        j.ldF = j.n + 3
    return c


_AB = ((1.0, 0.0), (0.5, 1.0), (2.0, 0.5), (0.25, 0.0), (1.0, 1.0), (4.0, 0.5))


def _ab(k):
    a, b = _AB[k % len(_AB)]
    return dict(alpha=a, beta=b)


def _build():
    out = []

    def add(cid, block, jobs, both=False, **want):
        out.append(case(cid, block, jobs(), **want))
        if both:
            out.append(case(cid + "/deferred", block, jobs(), deferred=True, **want))

    # fp32, register-staged (one job, not 16-byte shaped: kfac_factor_tiles' staged path)
    k = 0
    for cols, ones, off in ((33, 0, 0), (64, 1, 1), (130, 0, 0)):
        for rows in (1, 31, 33, 95):
            k += 1
            add(f"staged[n{cols + ones},rows{rows}]", "staged",
                lambda: [J(cols, ones, off=off, batches=(rows,), **_ab(k))], families=("tiles",), launches=1)
    add("staged[ld%4]", "staged", lambda: [J(36, 0, pad=1, batches=(33,), **_ab(1))], families=("tiles",))
    add("staged[base+1]", "staged", lambda: [J(36, 0, off=1, batches=(95,), **_ab(2))], families=("tiles",))
    add("staged[middle base+1]", "staged", lambda: [J(36, 1, off=(0, 1, 0), batches=(33, 33, 33), **_ab(3))],
        families=("tiles",), launches=1)
    # fp32, LDS-DMA (16-byte rows)
    for cols, ones in ((36, 0), (64, 0), (64, 1), (128, 1), (132, 0), (252, 1)):
        for rows in (1, 33, 95):
            k += 1
            add(f"glds[n{cols + ones},rows{rows}]", "glds",
                lambda: [J(cols, ones, batches=(rows,), **_ab(k))], families=("tiles",), launches=1)
    add("glds[n132,rows2048]", "glds", lambda: [J(132, 0, batches=(2048,), **_ab(0))], families=("tiles",), min_splits=2)
    add("glds[n64,ld+4]", "glds", lambda: [J(64, 0, pad=4, batches=(95,), **_ab(1))], families=("tiles",))
    # fp32, mixed launches
    add("mixed[glds+staged]", "mixed", lambda: [J(64, 1, batches=(95,), **_ab(1)), J(33, 0, batches=(95,), **_ab(2))],
        both=True, families=("tiles",), launches=1)
    add("mixed[glds+narrow direct]", "mixed", lambda: [J(64, 1, batches=(95,), **_ab(2)), J(10, 0, batches=(95,), **_ab(3))],
        both=True, families=("tiles",), launches=1)
    add("mixed[257 beside 70 columns]", "mixed", lambda: [J(256, 1, batches=(95,), **_ab(4)), J(70, 0, batches=(95,), **_ab(5))],
        both=True, families=("tiles",), launches=1)

    # tiles_x3, ragged in the kernel: 257 (256 + ones), 36, 9 (8 + ones: narrow, 16-byte) and
    # 10 (narrow, direct); 5 stages, the ragged batch is stage 4
    def x3group(b=(64, 64, 16), full=None, scale=1.0):
        js = [J(256, 1, batches=b, splits=2, **_ab(1)), J(36, 0, batches=b, splits=3, **_ab(2)),
              J(8, 1, batches=b, splits=4, **_ab(3)), J(10, 0, batches=b, splits=5, **_ab(4))]
        if full is not None:
            js[full] = J(36, 0, batches=(b[0],) * len(b), splits=3, **_ab(2))
        return js
    add("x3ragged[deferred]", "x3ragged", x3group, deferred=True, families=("tiles_x3",), launches=1,
        kinds=("crossing", "starts", "ends", "empty"))
    add("x3ragged[immediate]", "x3ragged", x3group, families=("tiles_x3",), launches=1)
    add("x3ragged[one job full]", "x3ragged", lambda: x3group(full=1), both=True, families=("tiles_x3",), launches=1)
    # one factor from two jobs of one call on slab ranges of one accumulator (acc_stride)
    add("x3ragged[two jobs, one accumulator]", "x3ragged",
        lambda: [J(256, 1, batches=(64, 64), splits=2, **_ab(1)), J(36, 0, batches=(64, 64), splits=3, **_ab(2)),
                 J(256, 1, batches=(16,), splits=1, alpha=2.0, into=0)],
        deferred=True, families=("tiles_x3",), launches=1)
    # ragged off tiles_x3: the head / tail split
    add("split[fp32 81+10]", "split", lambda: [J(81, 0, batches=(32, 32, 8), **_ab(1)), J(10, 0, batches=(32, 32, 8), **_ab(2))],
        both=True, families=("tiles",), launches=2)
    add("split[fp32 nseg 2]", "split", lambda: [J(81, 0, batches=(32, 8), **_ab(3)), J(10, 0, batches=(32, 8), **_ab(4))],
        both=True, families=("tiles",), launches=2)
    add("split[x3, 65 batches]", "split", lambda: x3group(b=(16,) * 64 + (4,)), both=True, families=("tiles_x3",), launches=5)
    # rounds
    for tag, ab in (("beta0", dict(alpha=0.5, beta=0.0)), ("beta1", dict(alpha=2.0, beta=1.0))):
        add(f"rounds[65 batches,{tag}]", "rounds", lambda: [J(256, 1, batches=(8,) * 65, **ab)],
            both=tag == "beta0", families=("tiles_x3",), launches=2)
        add(f"rounds[4 jobs x 17,{tag}]", "rounds",
            lambda: [J(256, 1, batches=(16,) * 17, **ab), J(36, 0, batches=(16,) * 17, **ab),
                     J(8, 1, batches=(8,) * 17, **ab), J(10, 0, batches=(8,) * 17, **ab)],
            both=tag == "beta0", families=("tiles_x3",), launches=2)
        add(f"rounds[70/3/1,{tag}]", "rounds",
            lambda: [J(10, 0, batches=(8,) * 70, **ab), J(256, 1, batches=(16,) * 3, **ab), J(36, 0, batches=(16,), **ab)],
            both=tag == "beta0", families=("tiles_x3", "tiles"), launches=3)

    # more than MAXJ row-major jobs, a small CHANNEL job at positions 0 and 9 of the caller's array
    def many(nrm):
        # distinct orders, 16-byte rows (so the group of the 257 routes to tiles_x3, the others to tiles)
        cols = [12 + 4 * i for i in range(nrm)]
        cols[5] = 256
        js = [J(c, int(i % 3 == 0 or c == 256), batches=(40,) if i % 2 else (24, 24), **_ab(i))
              for i, c in enumerate(cols)]
        js.insert(0, CH(6, 16, 3, **_ab(1)))
        js.insert(9, CH(3, 16, 5, **_ab(2)))
        return js
    add("many[17]", "many", lambda: many(17), both=True, families=("tiles_x3", "tiles", "channel_small"))
    add("many[33]", "many", lambda: many(33), both=True, families=("tiles_x3", "tiles", "channel_small"))
    # kfac_factor_syrk3
    for gname, group in (("2048", lambda b, k: [J(2048, 0, batches=b, **_ab(k))]),
                         ("2049", lambda b, k: [J(2048, 1, batches=b, **_ab(k))]),
                         ("2053+260+10", lambda b, k: [J(2052, 1, batches=b, **_ab(k)), J(260, 0, batches=b, **_ab(k + 1)),
                                                        J(10, 0, batches=b, **_ab(k + 2))])):
        for bi, b in enumerate(((40,), (32, 32, 32), (32, 32, 8))):
            k += 1
            add(f"syrk3[{gname},{'+'.join(map(str, b))}]", "syrk3", lambda: group(b, k),
                both=gname != "2048" and bi != 1, families=("syrk3",), launches=2 if len(b) == 3 and b[-1] < b[0] else 1)
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids)
    return out


_CASES = None


def all_cases():
    global _CASES
    if _CASES is None:
        _CASES = _build()
    return _CASES


def get(cid):
    c, = [c for c in all_cases() if c.id == cid]
    return c


# ------------------------------------------------------------------------------ data
def layout(c):
    """Float offsets of the case's buffers: c.xat[i][s] batch s of job i in the input buffer,
    c.fat[i] F[0][0] of job i in the F buffer (a job `into` another shares its F)."""
    if hasattr(c, "xat"):
        return c
    at, c.xat = 0, []
    for j in c.jobs:
        row = []
        for s, off in enumerate(j.offs):
            if j.layout == "channel":
                extent = (j.rows // j.L - 1) * j.sB + j.n * j.L
            else:
                extent = (j.rows - 1) * j.ld + j.cols
            row.append(at + GUARD + off)
            at += _cdiv(GUARD + off + extent + GUARD, 4) * 4
        c.xat.append(row)
    c.xsize = at
    at, c.fat = 0, []
    for j in c.jobs:
        if j.into is not None:
            c.fat.append(c.fat[j.into])
            continue
        c.fat.append(at + GUARD)
        at += _cdiv(GUARD + j.n * j.ldF + GUARD, 4) * 4
    c.fsize = at
    return c


def _idx(j, base, rows):
    """Flat indices of the rows x cols elements of one batch at `base`."""
    k = np.arange(rows, dtype=np.int64)[:, None]
    i = np.arange(j.cols, dtype=np.int64)[None, :]
    if j.layout == "channel":  # include/kfac_hip.h: ptr[(k / L) * sB + (k % L) + i * L]
        return base + (k // j.L) * j.sB + (k % j.L) + i * j.L
    return base + k * j.ld + i


def batch_rows(j, s):
    return j.last if ragged(j) and s == len(j.batches) - 1 else j.rows


_INPUTS = {}


def inputs(c):
    """The flat fp32 input buffer: NaN everywhere but the batches' elements."""
    if c.id not in _INPUTS:
        layout(c)
        buf = np.full(c.xsize, np.nan, dtype=F32)
        rng = _rng("x", c.id)
        for i, j in enumerate(c.jobs):
            for s in range(len(j.batches)):
                at = _idx(j, c.xat[i][s], batch_rows(j, s))
                buf[at] = rng.integers(-3, 4, size=at.shape)
        buf.setflags(write=False)
        _INPUTS[c.id] = buf
    return _INPUTS[c.id]


def region(c, i):
    j = c.jobs[i]
    return c.fat[i] + np.arange(j.n)[:, None] * j.ldF + np.arange(j.n)[None, :]


def prefill(c, i):
    """Job i's symmetric integer prefill (beta != 0), or None (beta = 0: NaN)."""
    j = c.jobs[i]
    if j.beta == 0.0:
        return None
    P = _rng("F", c.id, i).integers(1, 5, size=(j.n, j.n)) * _rng("Fs", c.id, i).choice([-1, 1], size=(j.n, j.n))
    return np.tril(P) + np.tril(P, -1).T


def f_buffer(c):
    layout(c)
    buf = np.full(c.fsize, np.nan, dtype=F32)
    for i, j in enumerate(c.jobs):
        if j.into is None and j.beta != 0.0:
            buf[region(c, i)] = prefill(c, i)
    return buf


def X(c, i, s, r0=0, r1=None, mistake=None):
    """Rows [r0, r1) of X~ of batch s of job i (fp64), the ones column included."""
    j = c.jobs[i]
    rows = batch_rows(j, s)
    r1 = rows if r1 is None else min(r1, rows)
    buf = inputs(c)
    x = buf[_idx(j, c.xat[i][s], rows)[r0:r1]].astype(np.float64)
    if j.ones:
        one = np.ones((x.shape[0], 1))
        if mistake == "ones_from_padding":  # x[:, cols]: the float behind each row
            one = buf[c.xat[i][s] + np.arange(r0, r1) * j.ld + j.cols].astype(np.float64)[:, None]
        x = np.concatenate([x, one], axis=1)
    return x


def factors(c):
    """Caller indices of the jobs that own an F."""
    return [i for i, j in enumerate(c.jobs) if j.into is None]


# ------------------------------------------------------------------------- reference
def _unit(c):
    """2^-u, the finest power of two an intermediate or a result is a multiple of."""
    u = Fraction(1)
    for j in c.jobs:
        a = Fraction(j.alpha)
        assert a.numerator == 1 or a.denominator == 1, "alpha is a power of two"
        w = rw(j)
        assert w.denominator == 1 and w.numerator & (w.numerator - 1) == 0, "rows / last_rows is a power of two"
        u = min(u, min(a, 1) * min(Fraction(j.beta) if j.beta else 1, 1) / w)
    return u


_REF = {}


def _gram(c, i, absolute=False):
    """int64 sum_b w_b X~_b^T X~_b of job i."""
    j = c.jobs[i]
    S = np.zeros((j.n, j.n), dtype=np.int64)
    for s in range(len(j.batches)):
        x = X(c, i, s)
        assert np.isfinite(x).all()
        x = np.abs(x) if absolute else x
        w = int(rw(j)) if ragged(j) and s == len(j.batches) - 1 else 1
        S += w * np.rint(x.T @ x).astype(np.int64)  # (fp64 matmul of small integers: exact)
    return S


def _combine(c, absolute):
    u = _unit(c)
    out = {}
    for i in factors(c):
        j = c.jobs[i]
        P = prefill(c, i)
        R = np.zeros((j.n, j.n), dtype=np.int64)
        if P is not None:
            R += int(Fraction(j.beta) / u) * (np.abs(P) if absolute else P)
        for k, jk in enumerate(c.jobs):
            if k == i or jk.into == i:
                R += int(Fraction(jk.alpha) / u) * _gram(c, k, absolute)
        out[i] = R
    return out, u


def bound(c):
    """The largest magnitude any partial sum or result can reach, in units of _unit(c)."""
    R, _ = _combine(c, True)
    return max(int(r.max()) for r in R.values())


def reference(c, mistake=None):
    """{job: F (n x n, fp64, exact)}; with a mistake: what walking plan(c) with it gives."""
    if mistake is not None:
        return walk(c, mistake)
    if c.id not in _REF:
        R, u = _combine(c, False)
        _REF[c.id] = {i: r.astype(np.float64) * float(u) for i, r in R.items()}
    return _REF[c.id]


def expected(c, ref=None):
    """The whole F buffer (fp64) after the case."""
    buf = f_buffer(c).astype(np.float64)
    for i, r in (reference(c) if ref is None else ref).items():
        buf[region(c, i)] = r
    return buf


# ------------------------------------------------------------------ jobs for the C ABI
def make_jobs(N, c, x_ptr, f_ptr, sub=None, acc=None):
    """The kfac_factor_job array of the call (or of the sub-jobs `sub` of one modelled launch),
    the input buffer at address x_ptr and the F buffer at f_ptr; returns (jobs, keepalive).
    acc: {factor: (address, stride)} of the deferred accumulators."""
    layout(c)
    subs = sub if sub is not None else [whole(c, i) for i in range(len(c.jobs))]
    jobs, keep = [], []
    for sj in subs:
        j = c.jobs[sj.i]
        ptrs = [x_ptr + 4 * c.xat[sj.i][s] for s in sj.batches]
        op = N.Operand()
        op.ptr, op.cols, op.rows, op.has_ones, op.last_rows = ptrs[0], j.cols, sj.rows, j.ones, sj.last
        if j.layout == "channel":
            op.layout, op.L, op.sB = N.CHANNEL, j.L, j.sB
        else:
            op.layout, op.ld = N.ROWMAJOR, j.ld
        fj = N.FactorJob()
        fj.x, fj.alpha, fj.beta, fj.F, fj.ldF = op, float(sj.alpha), 1.0 if sj.add else j.beta, f_ptr + 4 * c.fat[sj.i], j.ldF
        if len(ptrs) > 1:
            table = N.segment_table(ptrs)
            keep.append(table)
            fj.seg_ptrs, fj.nseg = N.table_ptr(table), len(ptrs)
        if c.deferred:
            f = sj.i if j.into is None else j.into
            base, stride = acc[f] if acc else (BASE << 4, slab_stride(c, f))
            fj.acc = base + 4 * TILE * TILE * slab_first(c, sj.i)
            fj.acc_splits, fj.acc_beta = j.splits, 1.0 if sj.add else 0.0
            fj.acc_stride = stride if stride != j.splits else 0
        jobs.append(fj)
    return jobs, keep


def slab_first(c, i):
    """First slab (per tile) of job i's range in its factor's accumulator."""
    f = c.jobs[i].into
    if f is None:
        return 0
    return c.jobs[f].splits + sum(jk.splits for k, jk in enumerate(c.jobs) if jk.into == f and k < i)


def slab_stride(c, f):
    return c.jobs[f].splits + sum(jk.splits for jk in c.jobs if jk.into == f)


def acc_floats(c, f):
    t = _cdiv(c.jobs[f].n, TILE)
    return t * (t + 1) // 2 * slab_stride(c, f) * TILE * TILE


def flush_jobs(N, c, f_ptr, acc):
    jobs = []
    for f in factors(c):
        j = c.jobs[f]
        fj = N.FactorJob()
        fj.x.layout, fj.x.cols, fj.x.has_ones, fj.x.ld = N.ROWMAJOR, j.cols, j.ones, j.cols
        fj.alpha, fj.beta, fj.F, fj.ldF = 1.0, j.beta, f_ptr + 4 * c.fat[f], j.ldF  # (the partials carry alpha)
        fj.acc, fj.acc_splits = acc[f][0], acc[f][1]
        jobs.append(fj)
    return jobs


# ----------------------------------------------------------------------------- model
def whole(c, i):
    j = c.jobs[i]
    return NS(i=i, batches=list(range(len(j.batches))), rows=j.rows, last=j.last, alpha=Fraction(j.alpha), add=False)


def _nseg(sj):
    return len(sj.batches) if len(sj.batches) > 1 else 0


def _route(N, c, subs):
    jobs, keep = make_jobs(N, c, BASE, BASE << 2, subs)
    fam = N.factor_route(jobs)
    assert len(set(fam)) == 1
    return FAMILY[fam[0]], jobs


def _update_group(N, c, subs, out, mistake):
    """update_group of factor.hip on the sub-jobs `subs`: appends the launches to `out`."""
    is_ragged = any(sj.last for sj in subs)
    nbases = sum(_nseg(sj) for sj in subs)
    family, jobs = _route(N, c, subs)
    if is_ragged and (family != "tiles_x3" or nbases > KSEG):
        head, tail = [], []
        for sj in subs:
            if not sj.last:
                head.append(sj)
                continue
            a = sj.alpha if mistake == "tail_alpha" else sj.alpha * sj.rows / sj.last
            tail.append(NS(i=sj.i, batches=sj.batches[-1:], rows=sj.last, last=0, alpha=a,
                           add=mistake != "tail_overwrites"))
            h = NS(i=sj.i, batches=sj.batches[:-1], rows=sj.rows, last=0, alpha=sj.alpha, add=sj.add)
            if len(h.batches) == 1 and mistake == "head_wrong_batch":
                h.batches = sj.batches[-1:]  # (the full-size read of the short batch)
                h.wrong = True
            head.append(h)
        _update_group(N, c, head, out, mistake)
        _update_group(N, c, tail, out, mistake)
        return
    multi = [sj for sj in subs if _nseg(sj)]
    if nbases <= KSEG:
        out.append(NS(family=family, subs=subs, jobs=jobs))
        return
    S = KSEG // len(multi)
    maxseg = max(_nseg(sj) for sj in multi)
    r = 0
    while r * S < maxseg:
        rnd = []
        for sj in subs:
            b = sj.batches
            if _nseg(sj):
                if r * S >= len(b):
                    if mistake != "round_spent_job_again":
                        continue
                    b = b[-1:]
                else:
                    b0 = 0 if mistake == "round_first_bases" else r * S
                    b = b[b0:b0 + min(S, len(b) - r * S)]
            elif r > 0:
                continue
            rnd.append(NS(i=sj.i, batches=b, rows=sj.rows, last=0, alpha=sj.alpha,
                          add=sj.add or (r > 0 and mistake != "round_beta0")))
        fam, rjobs = _route(N, c, rnd)
        out.append(NS(family=fam, subs=rnd, jobs=rjobs))
        r += 1


_PLANS = {}


def plan(c, mistake=None):
    """The launches of the case's kfac_factor_update call, in order: NS(family, subs, jobs)."""
    key = (c.id, mistake if mistake in HOST_MISTAKES else None)
    if key not in _PLANS:
        N = _native()
        rm = [i for i, j in enumerate(c.jobs) if j.layout == "rowmajor"]
        groups = [rm[g:g + MAXJ] for g in range(0, len(rm), MAXJ)]
        groups += [[i] for i, j in enumerate(c.jobs) if j.layout != "rowmajor"]
        out = []
        for g in groups:
            _update_group(N, c, [whole(c, i) for i in g], out, key[1])
        _PLANS[key] = out
    return _PLANS[key]


def launch_counts(c):
    """{profile slot: launches} the call (and the flush of a deferred case) must count."""
    N = _native()
    ids = {v: k for k, v in FAMILY.items()}
    counts = {slot: 0 for slot in N.PROF_FACTOR_KERNELS}
    for L in plan(c):
        counts[ids[L.family]] += 1
    counts[REDUCE] = _cdiv(len(factors(c)), MAXJ) if c.deferred else len(plan(c))
    return counts


def workspace_bytes(c):
    """What kfac_factor_workspace_bytes must return: the maximum over the launch groups."""
    N = _native()
    jobs, keep = make_jobs(N, c, BASE, BASE << 2)
    rm = [fj for fj in jobs if fj.x.layout == N.ROWMAJOR]
    groups = [rm[g:g + MAXJ] for g in range(0, len(rm), MAXJ)] + [[fj] for fj in jobs if fj.x.layout != N.ROWMAJOR]
    L = N.lib()
    return max(L.kfac_factor_workspace_bytes(N.as_array(N.FactorJob, g), len(g)) for g in groups)


def _stage_list(c, sj):
    """[(batch, first row, end row)] of a launch's job: BK-row stages, never across two batches."""
    out = []
    for s in sj.batches:
        rows = sj.last if sj.last and s == sj.batches[-1] else sj.rows
        if getattr(sj, "wrong", False):
            rows = min(rows, batch_rows(c.jobs[sj.i], s))
        out += [(s, k, min(k + BK, rows)) for k in range(0, max(rows, 1), BK)]
    return out


def task_ranges(stages, splits):
    """[(s0, s1)] of the K-splits: chunk = ceil(stages / splits); trailing splits may be empty."""
    chunk = _cdiv(stages, splits)
    return [(min(s * chunk, stages), min((s + 1) * chunk, stages)) for s in range(splits)]


def task_kinds(c, sj, splits):
    """The ragged task kinds among a job's K-splits, from the stage arithmetic."""
    sps = _cdiv(sj.rows, BK)
    stages = sps * (len(sj.batches) - 1) + _cdiv(sj.last, BK)
    rstage, kinds = sps * (len(sj.batches) - 1), set()
    for s0, s1 in task_ranges(stages, splits):
        if s0 == s1:
            kinds.add("empty")
        elif s0 < rstage < s1:
            kinds.add("crossing")
        elif s0 == rstage:
            kinds.add("starts")
        elif s1 == rstage:
            kinds.add("ends")
    return kinds


def _partials(c, sj, splits, mistake):
    """The K-splits' partial sums (fp64) of one job of one launch, as the kernels form them."""
    j = c.jobs[sj.i]
    st = _stage_list(c, sj)
    rstage = len(st) - _cdiv(sj.last, BK) if sj.last else -1
    w = float(Fraction(sj.rows, sj.last)) if sj.last else 1.0
    out = []
    for s0, s1 in task_ranges(len(st), splits):
        P = np.zeros((j.n, j.n))
        for s in range(s0, s1):
            if s == rstage and s > s0 and mistake != "rinv_skipped":
                P = P / w
            b, r0, r1 = st[s]
            x = X(c, sj.i, b, r0, r1, mistake)
            if mistake == "clamp_repeats_row" and r1 - r0 < BK and r1 > r0:
                x = np.concatenate([x, np.repeat(x[-1:], BK - (r1 - r0), axis=0)])
            P = P + x.T @ x
        if s1 > s0 and rstage >= 0:
            if s1 > rstage:
                if not (s0 == rstage and mistake == "rw_skipped_at_start"):
                    P = P * w
            elif s1 == rstage and mistake == "rw_applied_before":
                P = P * w
        out.append(P)
    return out


def _tiles(n):
    t = _cdiv(n, TILE)
    return [(ti, tj) for ti in range(t) for tj in range(ti + 1)]


def walk(c, mistake=None):
    """{job: F} from the plan's launches, K-split by K-split, with one planted mistake."""
    assert mistake is None or mistake in MISTAKES, mistake
    N = _native()
    F, acc = {}, {}
    for f in factors(c):
        n = c.jobs[f].n
        P = prefill(c, f)
        F[f] = np.full((n, n), np.nan) if P is None else P.astype(np.float64)
        if c.deferred:  # the real layout: tile, slab, 64 x 64
            acc[f] = np.full((len(_tiles(n)) * slab_stride(c, f), TILE, TILE), np.nan)
    for L in plan(c, mistake):
        if c.deferred:
            splits = [c.jobs[sj.i].splits for sj in L.subs]
        else:
            splits = [s for s, _ in N.factor_accum_plan(L.jobs)]
        for sj, sp in zip(L.subs, splits):
            j = c.jobs[sj.i]
            f = sj.i if j.into is None else j.into
            parts = _partials(c, sj, sp, mistake)
            a = float(sj.alpha)
            if not c.deferred:
                G = sum(parts)
                beta = 1.0 if sj.add else j.beta
                F[f] = a * G if beta == 0.0 else beta * F[f] + a * G
                continue
            stride, first = slab_stride(c, f), slab_first(c, sj.i)
            pad = _cdiv(j.n, TILE) * TILE
            for s, P in enumerate(parts):
                Pp = np.zeros((pad, pad))
                Pp[:j.n, :j.n] = P
                for t, (ti, tj) in enumerate(_tiles(j.n)):
                    at = t * stride + first + s
                    if mistake == "stride_as_splits":
                        at = first + t * sp + s
                    if at >= len(acc[f]):
                        continue
                    blk = a * Pp[ti * TILE:(ti + 1) * TILE, tj * TILE:(tj + 1) * TILE]
                    acc[f][at] = blk if not sj.add else acc[f][at] + blk
    if c.deferred:
        for f in factors(c):
            j = c.jobs[f]
            stride, pad = slab_stride(c, f), _cdiv(j.n, TILE) * TILE
            S = np.zeros((pad, pad))
            for t, (ti, tj) in enumerate(_tiles(j.n)):
                S[ti * TILE:(ti + 1) * TILE, tj * TILE:(tj + 1) * TILE] = acc[f][t * stride:(t + 1) * stride].sum(axis=0)
            S = np.tril(S[:j.n, :j.n])
            S = S + np.tril(S, -1).T
            F[f] = S if j.beta == 0.0 else j.beta * F[f] + S
    if mistake == "upper_not_mirrored":
        for f in factors(c):
            P = prefill(c, f)
            up = np.triu(np.ones_like(F[f], dtype=bool), 1)
            F[f][up] = np.nan if P is None else P[up]
    if mistake == "F_of_neighbour":
        rm = [i for i, j in enumerate(c.jobs) if j.layout == "rowmajor"]
        a, b = rm[MAXJ - 1], rm[MAXJ]  # either side of the first group boundary
        Fa, Fb = F[a], F[b]
        m = min(len(Fa), len(Fb))
        F[a], F[b] = Fa.copy(), Fb.copy()
        F[a][:m, :m], F[b][:m, :m] = Fb[:m, :m], Fa[:m, :m]
    return F


def _split_cases(c):
    return any(ragged(j) for j in c.jobs) and len(plan(c)) > 1 and c.block in ("split", "syrk3")


def _rounds(c):
    return c.block == "rounds" or c.id.startswith("split[x3")


def _walked(c):
    """The mistakes every case shows are walked on every case but, of the 20xx orders (4 M
    entries a walk), on the one-batch cases alone -- to keep the host test short."""
    return c.block != "syrk3" or len(c.jobs[0].batches) == 1


def _kinds(c, kind):
    """A launch of the case runs a ragged job in the kernel with a K-split of `kind`."""
    N = _native()
    for L in plan(c):
        sp = [c.jobs[sj.i].splits for sj in L.subs] if c.deferred else [s for s, _ in N.factor_accum_plan(L.jobs)]
        if any(sj.last and kind in task_kinds(c, sj, s) for sj, s in zip(L.subs, sp)):
            return True
    return False


HOST_MISTAKES = ("round_beta0", "round_first_bases", "round_spent_job_again", "tail_alpha", "tail_overwrites",
                 "head_wrong_batch")
# mistake -> the cases that must show it
MISTAKES = {
    # (a job's own beta = 1 is what a later round sets anyway)
    "round_beta0": lambda c: _rounds(c) and (c.deferred or any(j.beta != 1.0 for j in c.jobs)),
    "round_first_bases": _rounds,
    "round_spent_job_again": lambda c: _rounds(c) and len({len(j.batches) for j in c.jobs if len(j.batches) > 1}) > 1,
    "tail_alpha": _split_cases,
    "tail_overwrites": _split_cases,
    "head_wrong_batch": lambda c: _split_cases(c) and any(ragged(j) and len(j.batches) == 2 for j in c.jobs),
    "rinv_skipped": lambda c: _kinds(c, "crossing"),
    "rw_skipped_at_start": lambda c: _kinds(c, "starts"),
    "rw_applied_before": lambda c: _kinds(c, "ends"),
    "ones_from_padding": lambda c: _walked(c) and any(j.ones for j in c.jobs),
    "clamp_repeats_row": lambda c: _walked(c) and any(batch_rows(j, s) % BK for j in c.jobs if j.layout == "rowmajor"
                                                      for s in range(len(j.batches))),
    "F_of_neighbour": lambda c: c.block == "many",
    "stride_as_splits": lambda c: c.deferred and any(j.into is not None for j in c.jobs),
    "upper_not_mirrored": lambda c: _walked(c),
}
