"""Integer-exact cases for the posterior kernels (a plain helper module, like eig_cases).

kfac_sample, kfac_kron_quadform, kfac_efb_update, kfac_kron_gram and kfac_tri_pack /
kfac_tri_unpack on small-integer data.  Every fp32 product and every partial sum of such
data is an integer below 2^24 (the quadform's double sums: below 2^53), so each output is
one well-defined number whatever the order of summation, and the device is compared with
`array_equal`.  A dropped k-step, a K-range one panel short, a mis-masked edge column, a
stride read as the width or a write outside the output each change an integer.

Data rules
  * factors (L, K, V, U) in {-1, 0, 1}; z, J, grad in [-2, 2]; c in {1, 2, 3}; sigma in
    {0.5, 1, 2, 4}; every edge <= 200, from {1, 33, 63, 64, 65, 68, 70, 97, 128, 129, 130}:
    the sizes at which a tile count (64), a last k-step (32) or a float4 edge changes.
  * lower-triangular factors hold exact zeros above the diagonal and +-1 on it; full
    factors (`dense`, `lower = 0`) are non-zero in the tiles beyond the diagonal tile.
  * every operand of a case lives in ONE flat fp32 buffer (`Arena`): each matrix occupies the
    left columns of a block whose row pitch is its leading dimension; padding columns,
    the gaps between blocks and not-accumulated outputs are NaN, accumulated outputs are
    prefilled with distinct integers.  The test uploads the buffer, runs the kernel and
    compares the WHOLE buffer: the written region against the reference, everything else
    (padding, columns at or beyond wcols, gaps between J rows, the inputs) against its prefill.

Three functions per kernel:
  *_reference  the operation in int64 / float64 from the logical integer matrices.  Where
               the kernel performs one correctly-rounded fp32 operation on exact operands
               (EFB's P*P and state + l, the quadform's (float)s and (float)total, the
               `acc += part` fold over more than 8 terms) the same operation in np.float32.
  *_model      a numpy restatement of what the kernel does (tiles, K-ranges, strides, where
               it writes) reading the flat buffer, with an optional planted `mistake`.
  *_bounds     the largest magnitude any fp32 intermediate can reach (|A| |B| products, which
               bound every partial sum).
test_posterior_cases_host.py asserts model(None) == reference, and model(m) != reference for
every mistake m a case lists in `covers`."""
import functools
import zlib
from types import SimpleNamespace as NS

import numpy as np

TILE, BK, GAP = 64, 32, 8
SHAPES = (1, 33, 63, 64, 65, 68, 70, 97, 128, 129, 130)
F32 = np.float32


def _rng(*tag):
    return np.random.default_rng(zlib.crc32(repr(tag).encode()))


def ints(rng, shape, lo=-2, hi=2):
    return rng.integers(lo, hi + 1, size=shape).astype(np.int64)


def lower_factor(rng, n):
    """Entries in {-1, 0, 1}, exact zeros above the diagonal, +-1 on it."""
    L = np.tril(ints(rng, (n, n), -1, 1))
    L[np.arange(n), np.arange(n)] = rng.choice([-1, 1], size=n)
    return L


def full_factor(rng, n):
    """Entries in {-1, 0, 1} over the whole square."""
    return ints(rng, (n, n), -1, 1)


def pad(mat, ld, fill=np.nan):
    """`mat` in the left columns of a (rows, ld) block of `fill`."""
    mat = np.atleast_2d(np.asarray(mat, dtype=np.float64))
    out = np.full((mat.shape[0], ld), fill, dtype=np.float64)
    out[:, :mat.shape[1]] = mat
    return out


def int_block(rows, ld, start):
    """Distinct integers: the prefill of an accumulated output, padding included."""
    return (start + np.arange(rows * ld, dtype=np.float64)).reshape(rows, ld)


def idx(off, rows, cols, ld):
    return off + np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]


class Arena:
    """One flat fp32 buffer: named 2-D blocks, NaN gaps between them.  Blocks start at a
    multiple of 4 elements (16 bytes, the row-major loader's float4 path), or at an odd
    element with `odd`."""

    def __init__(self):
        self.blocks, self.size = [], 0

    def put(self, name, block, odd=False):
        b = np.atleast_2d(np.asarray(block, dtype=np.float64)).astype(F32)
        off = self.size + GAP
        off += -off % 4
        if odd:
            off += 1
        self.blocks.append((name, off, b))
        self.size = off + b.size
        return off

    def array(self):
        flat = np.full(self.size + GAP, np.nan, dtype=F32)
        for _, off, b in self.blocks:
            flat[off:off + b.size] = b.ravel()
        return flat

    def locate(self, i):
        """Element i of the flat buffer as `name[row, col] (tile r, c)`."""
        for name, off, b in self.blocks:
            if off <= i < off + b.size:
                r, c = divmod(int(i) - off, b.shape[1])
                return f"{name}[{r}, {c}] (64x64 tile {r // TILE}, {c // TILE}; block pitch {b.shape[1]})"
        return f"gap element {int(i)}"


def same(a, b):
    """Equal element for element, NaN matching NaN."""
    return np.array_equal(np.asarray(a, dtype=F32), np.asarray(b, dtype=F32), equal_nan=True)


def first_difference(arena, got, want):
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
    if not len(bad):
        return None
    i = bad[0]
    return f"{len(bad)} elements differ; first at {arena.locate(i)}: got {got[i]!r}, want {want[i]!r}"


def _read(flat, off, rows, cols, ld):
    return flat[idx(off, rows, cols, ld)]


def _absmax(x):
    return float(np.abs(x).max()) if np.size(x) else 0.0


# ---------------------------------------------------------------------------- sample
SAMPLE_MISTAKES = ("dense1", "dense2", "kshort1", "kshort2", "bias_dropped", "bias_to_W",
                   "acc_ignored", "ldA", "ldG", "ldW")


def _sample_job(ar, tag, nA, nG, wcols, bias, dense, acc, pads, odd=False):
    r = _rng("sample", tag, nA, nG, wcols, bias, dense, acc)
    mk = full_factor if dense else lower_factor
    j = NS(tag=tag, nA=nA, nG=nG, wcols=wcols, dense=int(dense), LA=mk(r, nA), LG=mk(r, nG),
           z=ints(r, (nA, nG)), ldA=nA + pads[0], ldG=nG + pads[1], ldW=wcols + pads[2])
    j.W0 = int_block(nG, j.ldW, 100) if acc else np.full((nG, j.ldW), np.nan)
    j.b0 = None
    if bias:
        j.b0 = 7 + 3 * np.arange(nG, dtype=np.float64) if acc else np.full(nG, np.nan)
    j.oLA = ar.put(f"{tag}.LA", pad(j.LA, j.ldA), odd)
    j.oLG = ar.put(f"{tag}.LG", pad(j.LG, j.ldG), odd)
    j.oZ = ar.put(f"{tag}.z", j.z, odd)
    j.oW = ar.put(f"{tag}.W", j.W0, odd)
    j.oB = ar.put(f"{tag}.bias", j.b0, odd) if bias else None
    return j


def _sample_covers(jobs, acc):
    c = set()
    for j in jobs:
        if j.wcols < j.nA:
            c.add("bias_to_W")
        if j.wcols == 0 and j.b0 is None:
            continue  # (nA = 1 with a NULL bias writes nothing: it only shows a stray write)
        c |= {"kshort1", "kshort2"}
        if j.dense and j.nA > TILE:
            c.add("dense1")
        if j.dense and j.nG > TILE:
            c.add("dense2")
        if j.wcols < j.nA and j.b0 is not None:
            c.add("bias_dropped")
        if j.nA > 1:
            c.add("ldA")
        if j.nG > 1:
            c.add("ldG")
            if j.wcols > 0:
                c.add("ldW")
    if acc:
        c.add("acc_ignored")
    return c


def _sample_case(cid, specs, acc=False, via="raw", odd=False):
    """specs: (nA, nG, wcols or None, bias, dense, pads) per job."""
    ar = Arena()
    jobs = [_sample_job(ar, f"{cid}.job{i}", nA, nG, nA if wcols is None else wcols, bias, dense, acc,
                        pads, odd) for i, (nA, nG, wcols, bias, dense, pads) in enumerate(specs)]
    return NS(kind="sample", id=cid, jobs=jobs, accumulate=int(acc), arena=ar, via=via, odd=odd,
              covers=_sample_covers(jobs, acc))


def _pads(nA, nG):
    """Leading-dimension paddings: n + 3 where that is a multiple of 4 (then n is not), and
    odd otherwise, so both loader paths and both kinds of pitch occur."""
    pa = 3 if (nA + 3) % 4 == 0 else 1
    pg = 3 if (nG + 3) % 4 == 0 else 5
    return (pa, pg, 7 if (nA + 7) % 4 else 5)


LOWER_SHAPES = ((64, 64), (65, 65), (129, 33), (33, 130), (1, 70), (97, 1))
DENSE_SHAPES = ((70, 130), (130, 70), (65, 65))
GROUP8 = ((130, 70, True), (1, 70, False), (65, 65, False), (33, 33, True), (129, 33, False),
          (97, 1, False), (70, 130, True), (64, 64, False))  # tiles 6 2 4 1 3 2 6 1
GROUP9 = GROUP8[:4] + ((65, 68, False), (33, 130, True), (63, 65, False), (128, 1, False),
                       (130, 70, True))


@functools.lru_cache(maxsize=None)
def sample_cases():
    cases = []
    for nA, nG in LOWER_SHAPES:
        p = _pads(nA, nG)
        cases.append(_sample_case(f"lower-{nA}x{nG}-full", [(nA, nG, None, False, False, p)]))
        cases.append(_sample_case(f"lower-{nA}x{nG}-bias", [(nA, nG, nA - 1, True, False, p)]))
        cases.append(_sample_case(f"lower-{nA}x{nG}-nobias", [(nA, nG, nA - 1, False, False, p)]))
    for nA, nG in ((65, 65), (129, 33), (33, 130)):
        cases.append(_sample_case(f"lower-{nA}x{nG}-acc", [(nA, nG, nA - 1, True, False, _pads(nA, nG))],
                                  acc=True))
    cases.append(_sample_case("lower-64x64-acc-full", [(64, 64, None, False, False, _pads(64, 64))],
                              acc=True))
    for nA, nG in DENSE_SHAPES:
        cases.append(_sample_case(f"dense-{nA}x{nG}", [(nA, nG, nA - 1, True, True, _pads(nA, nG))]))
    cases.append(_sample_case("dense-130x70-acc", [(130, 70, None, False, True, _pads(130, 70))], acc=True))
    for nG in (68, 70):  # z's pitch is nG: a full float4 then the scalar edge in the last tile
        cases.append(_sample_case(f"loader-65x{nG}-aligned", [(65, nG, 64, True, False, (3, 4, 4))]))
    cases.append(_sample_case("loader-65x68-odd-offsets", [(65, 68, 64, True, False, (3, 4, 4))], odd=True))
    cases.append(_sample_case("group8", [(nA, nG, nA - 1 if i % 2 else None, i % 4 == 1, d, _pads(nA, nG))
                                         for i, (nA, nG, d) in enumerate(GROUP8)]))
    cases.append(_sample_case("group9-chunks", [(nA, nG, nA - 1 if i % 2 == 0 else None, i % 4 == 0, d,
                                                 _pads(nA, nG)) for i, (nA, nG, d) in enumerate(GROUP9)],
                              acc=True))
    return tuple(cases)


def _put_sample(flat, j, S, acc):
    """The (nG x nA) sample into W's columns < wcols and the bias, added or written."""
    w = idx(j.oW, j.nG, j.wcols, j.ldW)
    flat[w] = (flat[w] + S[:, :j.wcols]) if acc else S[:, :j.wcols]
    if j.wcols < j.nA and j.oB is not None:
        b = j.oB + np.arange(j.nG)
        flat[b] = (flat[b] + S[:, -1]) if acc else S[:, -1]


def sample_reference(case):
    flat = case.arena.array().astype(np.float64)
    for j in case.jobs:
        _put_sample(flat, j, (j.LA @ j.z @ j.LG.T).T, case.accumulate)
    return flat.astype(F32)


def sample_model(case, mistake=None):
    """kfac_sample_ly then kfac_sample_out, one 64x64 tile at a time."""
    flat = case.arena.array().astype(np.float64)
    acc = case.accumulate and mistake != "acc_ignored"
    with np.errstate(all="ignore"):
        for j in case.jobs:
            nA, nG = j.nA, j.nG
            LA = _read(flat, j.oLA, nA, nA, nA if mistake == "ldA" else j.ldA)
            LG = _read(flat, j.oLG, nG, nG, nG if mistake == "ldG" else j.ldG)
            z = _read(flat, j.oZ, nA, nG, nG)
            Y = np.zeros((nA, nG))
            for a0 in range(0, nA, TILE):
                kend = nA if (j.dense and mistake != "dense1") else min(nA, a0 + TILE)
                if mistake == "kshort1":
                    kend = max(kend - BK, 0)
                Y[a0:a0 + TILE] = LA[a0:a0 + TILE, :kend] @ z[:kend]
            S = np.zeros((nG, nA))
            for g0 in range(0, nG, TILE):
                kend = nG if (j.dense and mistake != "dense2") else min(nG, g0 + TILE)
                if mistake == "kshort2":
                    kend = max(kend - BK, 0)
                S[g0:g0 + TILE] = LG[g0:g0 + TILE, :kend] @ Y[:, :kend].T
            ldW = j.wcols if mistake == "ldW" else j.ldW
            wc = nA if (mistake == "bias_to_W") else j.wcols
            w = idx(j.oW, nG, wc, ldW)
            flat[w] = (flat[w] + S[:, :wc]) if acc else S[:, :wc]
            if j.wcols < nA and j.oB is not None and mistake not in ("bias_dropped", "bias_to_W"):
                b = j.oB + np.arange(nG)
                flat[b] = (flat[b] + S[:, -1]) if acc else S[:, -1]
    return flat.astype(F32)


def sample_bounds(case):
    """Y, the sample, and the accumulated output."""
    out = {"Y": 0.0, "sample": 0.0, "out": 0.0}
    for j in case.jobs:
        Y = np.abs(j.LA) @ np.abs(j.z)
        S = (Y @ np.abs(j.LG).T).T
        out["Y"] = max(out["Y"], _absmax(Y))
        out["sample"] = max(out["sample"], _absmax(S))
        pre = max(_absmax(np.nan_to_num(j.W0)), _absmax(np.nan_to_num(j.b0)) if j.b0 is not None else 0.0)
        out["out"] = max(out["out"], _absmax(S) + pre)
    return out


# -------------------------------------------------------------------------- quadform
QUAD_MISTAKES = ("lower1_forced", "lower2_forced", "k1_late", "abs_ignored", "abs_always", "ldJ",
                 "ld1", "ld2")
QUAD_SHAPES = ((65, 65), (130, 33), (33, 130), (64, 128))


def _quad_job(ar, tag, nA, nG, nb, lower1, lower2, has_v, ldJ=None):
    r = _rng("quad", tag, nA, nG, nb, lower1, lower2)
    j = NS(tag=tag, nA=nA, nG=nG, lower1=int(lower1), lower2=int(lower2),
           K1=(lower_factor if lower1 else full_factor)(r, nA),
           K2=(lower_factor if lower2 else full_factor)(r, nG), J=ints(r, (nb, nA * nG)),
           ldJ=nA * nG + 5 if ldJ is None else ldJ, ld1=nA + (3 if (nA + 3) % 4 == 0 else 1),
           ld2=nG + (3 if (nG + 3) % 4 == 0 else 5))
    j.oJ = ar.put(f"{tag}.J", pad(j.J, j.ldJ))
    j.o1 = ar.put(f"{tag}.K1", pad(j.K1, j.ld1))
    j.o2 = ar.put(f"{tag}.K2", pad(j.K2, j.ld2))
    j.oV = ar.put(f"{tag}.v", np.full(nb, np.nan)) if has_v else None
    return j


def _quad_case(cid, specs, nb, abs_sum, via="raw"):
    """specs: (nA, nG, lower1, lower2, has_v) per job.  via="wrapper": through
    variance.kron_quadform(per_term=True), which allocates out and v itself."""
    ar = Arena()
    jobs = [_quad_job(ar, f"{cid}.job{i}", nA, nG, nb, l1, l2, hv and via == "raw")
            for i, (nA, nG, l1, l2, hv) in enumerate(specs)]
    oOut = ar.put(f"{cid}.out", np.full(nb, np.nan)) if via == "raw" else None
    c = NS(kind="quad", id=cid, jobs=jobs, nb=nb, abs_sum=int(abs_sum), arena=ar, via=via, oOut=oOut)
    c.covers = {"k1_late"}
    for j in jobs:
        if not j.lower1 and j.nA > TILE:
            c.covers.add("lower1_forced")
        if not j.lower2 and j.nG > TILE:
            c.covers.add("lower2_forced")
        if j.nA > 1:
            c.covers.add("ld1")
        if j.nG > 1:
            c.covers.add("ld2")
    if nb > 1:
        c.covers.add("ldJ")
    if len(jobs) > 1:
        c.covers.add("abs_ignored" if abs_sum else "abs_always")
    return c


QUAD_GROUP8 = ((130, 33, 1, 0, True), (33, 33, 0, 0, False), (65, 65, 0, 1, True), (1, 70, 1, 1, True),
               (64, 128, 1, 1, False), (97, 1, 0, 0, True), (33, 130, 0, 0, True), (63, 64, 1, 0, False))


@functools.lru_cache(maxsize=None)
def quad_cases():
    cases = []
    for nA, nG in QUAD_SHAPES:
        for l1 in (1, 0):
            for l2 in (1, 0):
                cases.append(_quad_case(f"flags{l1}{l2}-{nA}x{nG}", [(nA, nG, l1, l2, True)], 3, True))
    cases.append(_quad_case("nb1-65x65", [(65, 65, 1, 1, True)], 1, False))
    cases.append(_quad_case("nb1-130x33-full", [(130, 33, 0, 0, True)], 1, True))
    cases.append(_quad_case("group8-abs", QUAD_GROUP8, 3, True))
    cases.append(_quad_case("group8-signed", QUAD_GROUP8, 3, False))
    nine = [(nA, nG, 1, 1, True) for nA, nG, *_ in QUAD_GROUP8] + [(65, 33, 1, 1, True)]
    cases.append(_quad_case("fold9-lower-abs", nine, 3, True, via="wrapper"))
    cases.append(_quad_case("fold9-full-signed", [(a, g, 0, 0, True) for a, g, *_ in nine], 3, False,
                            via="wrapper"))
    return tuple(cases)


def _quad_out(V, abs_sum):
    """(float)s per job; (float)total per call of at most 8 jobs; `acc += part` in fp32 over
    the calls (variance.kron_quadform's fold) when there are more than 8."""
    V = np.asarray(V, dtype=np.float64)  # exact integers below 2^53
    parts = [(np.abs(V[i:i + 8]) if abs_sum else V[i:i + 8]).sum(axis=0).astype(F32)
             for i in range(0, len(V), 8)]
    out = parts[0]
    if len(parts) > 1:
        out = np.zeros_like(parts[0])
        for p in parts:
            out = (out + p).astype(F32)
    return V.astype(F32), out


def quad_reference(case):
    """(v (njobs, nb), out (nb,)) fp32."""
    V = []
    for j in case.jobs:
        M = j.J.reshape(case.nb, j.nA, j.nG)
        V.append(np.einsum("bag,bag->b", M, j.K1 @ M @ j.K2.T))
    assert max(_absmax(v) for v in V) * len(V) < 2.0 ** 53
    return _quad_out(V, case.abs_sum)


def quad_model(case, mistake=None):
    """kfac_quad_tiles per (job, row, tile) with its K-ranges, then kfac_quad_reduce."""
    flat = case.arena.array().astype(np.float64)
    nb, V = case.nb, []
    with np.errstate(all="ignore"):
        for j in case.jobs:
            nA, nG = j.nA, j.nG
            M = _read(flat, j.oJ, nb, nA * nG, nA * nG if mistake == "ldJ" else j.ldJ).reshape(nb, nA, nG)
            K1 = _read(flat, j.o1, nA, nA, nA if mistake == "ld1" else j.ld1)
            K2 = _read(flat, j.o2, nG, nG, nG if mistake == "ld2" else j.ld2)
            l1 = j.lower1 or mistake == "lower1_forced"
            l2 = j.lower2 or mistake == "lower2_forced"
            s = np.zeros(nb)
            for a0 in range(0, nA, TILE):
                k0 = (a0 if l1 else 0) + (TILE if mistake == "k1_late" else 0)
                P = np.einsum("ka,bkg->bag", K1[k0:, a0:a0 + TILE], M[:, k0:, :])
                for g0 in range(0, nG, TILE):
                    kq = min(nG, g0 + TILE) if l2 else nG
                    Q = np.einsum("bak,gk->bag", M[:, a0:a0 + TILE, :kq], K2[g0:g0 + TILE, :kq])
                    s += (P[:, :, g0:g0 + TILE] * Q).sum(axis=(1, 2))
            V.append(s)
        abs_sum = (case.abs_sum or mistake == "abs_always") and mistake != "abs_ignored"
        return _quad_out(V, abs_sum)


def quad_expected(case, v, out):
    """The flat buffer after a raw call that produced (v, out)."""
    flat = case.arena.array()
    for j, vj in zip(case.jobs, v):
        if j.oV is not None:
            flat[j.oV:j.oV + case.nb] = vj
    flat[case.oOut:case.oOut + case.nb] = out
    return flat


def quad_bounds(case):
    """P and Q (fp32 accumulators), and the double sums."""
    out = {"P": 0.0, "Q": 0.0, "sum": 0.0}
    for j in case.jobs:
        M = np.abs(j.J.reshape(case.nb, j.nA, j.nG))
        P, Q = np.abs(j.K1).T @ M, M @ np.abs(j.K2).T
        out["P"], out["Q"] = max(out["P"], _absmax(P)), max(out["Q"], _absmax(Q))
        out["sum"] += _absmax((P * Q).sum(axis=(1, 2)))
    return out


# ------------------------------------------------------------------------------- EFB
EFB_MISTAKES = ("vg_untransposed", "acc_ignored", "acc_always", "ld_state", "ld_grad", "ld_diag", "ldA",
                "ldG")
EFB_SHAPES = ((65, 65), (130, 33), (33, 130))
EFB_SCALE = 32.0


def _efb_job(ar, tag, nA, nG, diag):
    r = _rng("efb", tag, nA, nG, diag)
    j = NS(tag=tag, nA=nA, nG=nG, VA=full_factor(r, nA), VG=full_factor(r, nG),
           grads=[ints(r, (nG, nA)) for _ in range(2)], has_diag=diag,
           ldA=nA + 3, ldG=nG + 1, ld_grad=nA + 7, ld_state=nA + 5, ld_diag=nA + 9)
    j.oVA = ar.put(f"{tag}.VA", pad(j.VA, j.ldA))
    j.oVG = ar.put(f"{tag}.VG", pad(j.VG, j.ldG))
    j.oGr = [ar.put(f"{tag}.grad{i}", pad(g, j.ld_grad)) for i, g in enumerate(j.grads)]
    j.oS = ar.put(f"{tag}.state", np.full((nG, j.ld_state), np.nan))
    j.oD = ar.put(f"{tag}.diag", np.full((nG, j.ld_diag), np.nan)) if diag else None
    return j


def _efb_case(cid, specs):
    """specs: (nA, nG, diag) per job.  Two batches: accumulate = 0 onto NaN, then 1."""
    ar = Arena()
    jobs = [_efb_job(ar, f"{cid}.job{i}", *s) for i, s in enumerate(specs)]
    c = NS(kind="efb", id=cid, jobs=jobs, arena=ar,
           covers={"vg_untransposed", "acc_ignored", "acc_always", "ld_grad", "ldA"})
    if any(j.nG > 1 for j in jobs):
        c.covers |= {"ld_state", "ldG"}
        if any(j.has_diag for j in jobs):
            c.covers.add("ld_diag")
    return c


EFB_GROUP9 = ((130, 33, True), (1, 70, True), (65, 65, False), (33, 33, True), (33, 130, True),
              (97, 1, True), (64, 128, False), (63, 64, True), (129, 65, True))


@functools.lru_cache(maxsize=None)
def efb_cases():
    cases = [_efb_case(f"{nA}x{nG}", [(nA, nG, True)]) for nA, nG in EFB_SHAPES]
    cases.append(_efb_case("65x65-nodiag", [(65, 65, False)]))
    cases.append(_efb_case("group8", EFB_GROUP9[:8]))
    cases.append(_efb_case("group9-chunks", EFB_GROUP9))
    return tuple(cases)


def _efb_put(flat, where, new, acc):
    flat[where] = (flat[where].astype(F32) + new).astype(F32) if acc else new


def efb_reference(case):
    flat = case.arena.array()
    for i in range(2):
        for j in case.jobs:
            P = (j.VG.T @ j.grads[i] @ j.VA).astype(F32)  # exact: |P| < 2^24
            _efb_put(flat, idx(j.oS, j.nG, j.nA, j.ld_state), P * P, i > 0)
            if j.has_diag:
                g = j.grads[i].astype(F32)
                _efb_put(flat, idx(j.oD, j.nG, j.nA, j.ld_diag), g * g * F32(EFB_SCALE), i > 0)
    return flat


def efb_model(case, mistake=None):
    """kfac_efb_project (T, diag) then kfac_efb_square, per batch."""
    flat = case.arena.array()
    with np.errstate(all="ignore"):
        for i in range(2):
            acc = (i > 0 or mistake == "acc_always") and mistake != "acc_ignored"
            for j in case.jobs:
                nA, nG = j.nA, j.nG
                VA = _read(flat, j.oVA, nA, nA, nA if mistake == "ldA" else j.ldA).astype(np.float64)
                VG = _read(flat, j.oVG, nG, nG, nG if mistake == "ldG" else j.ldG).astype(np.float64)
                g = _read(flat, j.oGr[i], nG, nA, nA if mistake == "ld_grad" else j.ld_grad)
                T = (VG if mistake == "vg_untransposed" else VG.T) @ g.astype(np.float64)
                P = (T @ VA).astype(F32)
                _efb_put(flat, idx(j.oS, nG, nA, nA if mistake == "ld_state" else j.ld_state), P * P, acc)
                if j.has_diag:
                    _efb_put(flat, idx(j.oD, nG, nA, nA if mistake == "ld_diag" else j.ld_diag),
                             g * g * F32(EFB_SCALE), acc)
    return flat


def efb_bounds(case):
    out = {"T": 0.0, "P": 0.0}
    for j in case.jobs:
        for g in j.grads:
            T = np.abs(j.VG).T @ np.abs(g)
            out["T"], out["P"] = max(out["T"], _absmax(T)), max(out["P"], _absmax(T @ np.abs(j.VA)))
    return out


# ------------------------------------------------------------------------------ Gram
GRAM_MISTAKES = ("scatter_qp", "sigma_once", "c_not_squared", "ldA", "ldG", "ldo")
GRAM_SHAPES = ((65, 33, 9, 8), (130, 70, 8, 9), (33, 65, 3, 12))
SIGMAS = (0.5, 1.0, 2.0, 4.0)


def _gram_job(ar, tag, nA, nG, la, lg):
    r = _rng("gram", tag, nA, nG, la, lg)
    j = NS(tag=tag, nA=nA, nG=nG, la=la, lg=lg, UA=ints(r, (nA, la), -1, 1), UG=ints(r, (nG, lg), -1, 1),
           c=ints(r, (nA, nG), 1, 3), sigma=r.choice(SIGMAS, size=la * lg),
           ldA=la + 3, ldG=lg + 3, ldo=la * lg + 5)
    j.oUA = ar.put(f"{tag}.UA", pad(j.UA, j.ldA))
    j.oUG = ar.put(f"{tag}.UG", pad(j.UG, j.ldG))
    j.oC = ar.put(f"{tag}.c", j.c)
    j.oSig = ar.put(f"{tag}.sigma", j.sigma)
    j.oOut = ar.put(f"{tag}.out", np.full((la * lg, j.ldo), np.nan))
    return j


def _gram_case(cid, shapes):
    ar = Arena()
    return NS(kind="gram", id=cid, jobs=[_gram_job(ar, f"{cid}.job{i}", *s) for i, s in enumerate(shapes)],
              arena=ar, covers=set(GRAM_MISTAKES))


@functools.lru_cache(maxsize=None)
def gram_cases():
    cases = [_gram_case("x".join(map(str, s)), [s]) for s in GRAM_SHAPES]
    cases.append(_gram_case("group3", GRAM_SHAPES))
    return tuple(cases)


def gram_reference(case):
    """diag(sigma) V^T V diag(sigma) with V = c * kron(UA, UG) formed explicitly, in int64."""
    flat = case.arena.array()
    for j in case.jobs:
        V = j.c.reshape(-1, 1) * np.kron(j.UA, j.UG)
        G = j.sigma[:, None] * (V.T @ V).astype(np.float64) * j.sigma[None, :]
        flat[idx(j.oOut, j.la * j.lg, j.la * j.lg, j.ldo)] = G
    return flat


def gram_model(case, mistake=None):
    """kfac_inf_tq then kfac_inf_gram with its (p,p') x (q,q') -> (p,q) x (p',q') scatter."""
    flat = case.arena.array()
    with np.errstate(all="ignore"):
        for j in case.jobs:
            nA, nG, la, lg = j.nA, j.nG, j.la, j.lg
            UA = _read(flat, j.oUA, nA, la, la if mistake == "ldA" else j.ldA).astype(np.float64)
            UG = _read(flat, j.oUG, nG, lg, lg if mistake == "ldG" else j.ldG).astype(np.float64)
            c = _read(flat, j.oC, nA, nG, nG).astype(np.float64)
            sig = flat[j.oSig:j.oSig + la * lg].astype(np.float64)
            Tq = np.einsum("ag,gq,gr->aqr", c if mistake == "c_not_squared" else c * c, UG, UG)
            X = np.einsum("ap,as,aqr->psqr", UA, UA, Tq)
            G = (X.transpose(2, 0, 3, 1) if mistake == "scatter_qp" else X.transpose(0, 2, 1, 3))
            G = G.reshape(la * lg, la * lg)
            G = sig[:, None] * G * (1.0 if mistake == "sigma_once" else sig[None, :])
            flat[idx(j.oOut, la * lg, la * lg, la * lg if mistake == "ldo" else j.ldo)] = G
    return flat


def gram_bounds(case):
    out = {"Tq": 0.0, "X": 0.0}
    for j in case.jobs:
        UA, UG = np.abs(j.UA), np.abs(j.UG)
        Tq = np.einsum("ag,gq,gr->aqr", j.c * j.c, UG, UG)
        out["Tq"] = max(out["Tq"], _absmax(Tq))
        out["X"] = max(out["X"], _absmax(np.einsum("ap,as,aqr->psqr", UA, UA, Tq)))
    return out


# -------------------------------------------------------------------------- tri-pack
TRI_MISTAKES = ("offset_by_position", "mirror_in_lower", "ldF")
TRI_SIZES = (1, 63, 64, 65, 129)
TRI_JOBS, TRI_CHUNK, TRI_PAD = 20, 16, 3
SYMMETRIC, LOWER = 0, 1  # kfac_tri_mode


@functools.lru_cache(maxsize=None)
def tri_case(op):
    """op: "pack", "unpack_sym" or "unpack_lower".  Twenty factors, views (ldF = n + 3) into
    wider blocks; packed offsets assigned in a seeded permuted order."""
    r = _rng("tri")
    sizes = [TRI_SIZES[i % len(TRI_SIZES)] for i in range(TRI_JOBS)]
    order = r.permutation(TRI_JOBS)
    offsets, off = [0] * TRI_JOBS, 0
    for i in order:
        offsets[i] = off
        off += sizes[i] * (sizes[i] + 1) // 2
    ar, jobs = Arena(), []
    for i, n in enumerate(sizes):
        F = np.triu(ints(r, (n, n), -9, -1), 1) + np.tril(ints(r, (n, n), 1, 9))  # above < 0 < below
        j = NS(n=n, ldF=n + TRI_PAD, offset=offsets[i], F=F)
        j.oF = ar.put(f"tri.job{i}.F", pad(F, j.ldF) if op == "pack" else np.full((n, j.ldF), np.nan))
        jobs.append(j)
    packed = np.full(off, np.nan) if op == "pack" else 1.0 + np.arange(off)
    c = NS(kind="tri", id=op, op=op, jobs=jobs, total=off, arena=ar, packed=packed,
           mode=LOWER if op == "unpack_lower" else SYMMETRIC,
           covers={"offset_by_position", "ldF"} | ({"mirror_in_lower"} if op == "unpack_lower" else set()))
    c.oP = ar.put("tri.packed", packed)
    return c


def _tri_apply(flat, c, offsets, ldF_of, mirror):
    for j, off in zip(c.jobs, offsets):
        n = j.n
        i, k = np.tril_indices(n)  # row-major: packed position i (i + 1) / 2 + k
        where = c.oP + off + np.arange(len(i))
        if c.op == "pack":
            flat[where] = flat[j.oF + i * ldF_of(j) + k]
        else:
            F = np.zeros((n, n), dtype=F32)
            F[i, k] = flat[where]
            if mirror:
                F[k, i] = flat[where]
            flat[idx(j.oF, n, n, ldF_of(j))] = F
    return flat


def tri_reference(c):
    return _tri_apply(c.arena.array(), c, [j.offset for j in c.jobs], lambda j: j.ldF, c.mode == SYMMETRIC)


def tri_model(c, mistake=None):
    offsets = [j.offset for j in c.jobs]
    if mistake == "offset_by_position":  # back to back in job order within each chunk
        for c0 in range(0, len(c.jobs), TRI_CHUNK):
            off = min(offsets[c0:c0 + TRI_CHUNK])
            for i in range(c0, min(c0 + TRI_CHUNK, len(c.jobs))):
                offsets[i] = off
                off += c.jobs[i].n * (c.jobs[i].n + 1) // 2
    ldF_of = (lambda j: j.n) if mistake == "ldF" else (lambda j: j.ldF)
    return _tri_apply(c.arena.array(), c, offsets, ldF_of,
                      c.mode == SYMMETRIC or mistake == "mirror_in_lower")


FAMILIES = {  # kind -> (cases, reference, model, bounds, mistakes)
    "sample": (sample_cases, sample_reference, sample_model, sample_bounds, SAMPLE_MISTAKES),
    "efb": (efb_cases, efb_reference, efb_model, efb_bounds, EFB_MISTAKES),
    "gram": (gram_cases, gram_reference, gram_model, gram_bounds, GRAM_MISTAKES),
}
