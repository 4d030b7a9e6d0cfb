"""Integer-exact, whole-buffer cases for the four oldest covariance calls: kfac_kron_cov,
kfac_kron_cov_outer, kfac_kron_cov_sweep and kfac_kron_cov_outer_sweep (a plain helper
module, like conv_rows_cases: no GPU, no torch device).

Data.  Factor-side matrices (K1, K2, V_A, V_G) hold at most three +-1 per column
(`sparse_signs`); dense-route rows J are {-1, 0, 1} at full density; outer-route a and D rows
hold at most eight +-1 and no all-zero row; sweep weights are integers in {0, 1, 2, 3}.  (What
a dropped element must reach is never 0: the last element of a J row, the last weight of a
vector, an entry in the last row of a dense factor, and D columns that reach V's last column
and the first one of a second Gram segment.)  So
every value the kernels form -- U, T or p, V, their squares, the weighted squares, every Gram
partial, scale times Gram, the sum over jobs and the accumulate prefill -- is an integer, and
`bound(case)` (ONE int64 evaluation of the whole chain on the absolute values of every
operand) is the largest magnitude any partial sum in any order can reach.  Below 2^24 every
fp32 partial sum is an exact integer whatever its order, the fp64 reduces are exact and so is
the final cast: the device result must have the bits of the int64 reference.

Reference.  `reference(case)` is int64 einsum written from the formulas in the headers of
covariance.hip and covariance_outer.hip (for the sweeps the int64 form of
glm_sweep_cases.dense_ref / outer_ref), never from the kernels.  `reference(case, mistake)`
evaluates the same chain with one named mistake a kernel could make (MISTAKES); the host test
shows each of them changes the result on the cases listed for it.

Layout.  Every operand of a case and its `cov` live in ONE NaN-filled fp32 buffer, regions
GAP floats apart, pitches above the widths (ldJ = nA*nG + 7, ld1 = nA + 3, ld2 = nG + 1,
lda = cols + 3, ldD = nG + 5, ldwA = nA + 3, ldwG = nG + 2 unless the case names another);
a region starts on a 16-byte boundary of the buffer unless the case skews it by one float.
`cov` is contiguous, prefilled with NaN, or with small integers for an accumulate case.  The
GPU test compares the whole buffer with `want(case)`."""
import functools
import zlib
from types import SimpleNamespace as NS

import numpy as np

F32 = np.float32
GAP = 8
LIMIT = 1 << 24
TILE, GSEG, WSEG, WTG, RNTG = 64, 2048, 256, 4, 16  # covariance_common.h, covariance_outer.hip
GUARD = 256                                         # bytes on each side of the workspace
ROUTES = ("dense", "outer", "sweep", "outer_sweep")


def sparse_signs(rng, n, lower):
    """n x n with at most three +-1 per column (on and below the diagonal if lower)."""
    K = np.zeros((n, n), dtype=np.int64)
    for c in range(n):
        first = c if lower else 0
        rows = rng.choice(np.arange(first, n), size=min(3, n - first), replace=False)
        K[rows, c] = rng.choice([-1, 1], size=rows.size)
    return K


# ------------------------------------------------------------------ case tables
# kfac_kron_cov: ((nA, nG, nb, nc), options); every entry runs as `lower` and as `dense`
DENSE = (
    ((1, 1, 1, 1), {}),
    ((5, 3, 2, 1), {}),                       # nc = 1
    ((27, 6, 4, 3), {}),
    ((64, 32, 1, 32), {"ldJ": 2048, "tag": "ldJ=K"}),  # K = GSEG: one full segment, a full quadrant, 16-byte loads
    ((683, 3, 2, 2), {}),                     # K = 2049: one element in segment 1; eleven a-tiles
    ((65, 33, 2, 31), {}),                    # K = 2145; one row alone in a-tile 1, one column alone in g-tile 1
    ((64, 64, 2, 5), {}),
    ((63, 65, 3, 2), {}),
    ((20, 130, 2, 3), {}),                    # three g-tiles
    ((20, 8, 3, 5), {"ldJ": 164, "tag": "ldJ=K+4"}),                      # vector path with a pitch
    ((20, 8, 3, 5), {"ldJ": 166, "tag": "ldJ=K+6"}),                      # scalar fallback with nG % 4 == 0
    ((20, 8, 3, 5), {"ldJ": 164, "skew": ("J",), "tag": "ldJ=K+4,Jskew"}),  # J one float past a 16-byte boundary
    ((20, 8, 3, 5), {"ld1": 24, "ld2": 12, "skew": ("K1", "K2"), "tag": "ld=n+4,Kskew"}),
)
# kfac_kron_cov_outer: ((cols, has_ones, nG, nb, nc), options); `lower` and `dense`
OUTER = (
    ((1, 0, 1, 1, 1), {}),
    ((63, 1, 10, 3, 10), {}),                 # the ones entry ends a tile
    ((64, 1, 5, 2, 3), {}),                   # the ones entry alone in the second tile
    ((64, 0, 7, 2, 3), {}),
    ((130, 1, 130, 70, 2), {}),               # samples cross the 64-sample row-norm tile
    ((12, 1, 6, 64, 2), {}),
    ((12, 1, 6, 65, 2), {}),
    ((20, 1, 2048, 2, 32), {}),               # nG = GSEG
    ((20, 1, 2049, 2, 3), {}),                # one element in segment 1
    ((20, 1, 8, 3, 5), {"lda": 24, "ldD": 12, "tag": "ld=n+4"}),
)
# kfac_kron_cov_sweep: ((nA, nG, nb, nc, nt), options); dense only by the ABI
SWEEP = (
    ((16, 16, 2, 3, 1), {}),                  # K = WSEG
    ((257, 1, 2, 2, 5), {}),                  # K = 257 with nG = 1; nt = 5 crosses a WTG group
    ((3, 86, 1, 32, 4), {}),                  # K = 258
    ((27, 6, 3, 10, 64), {}),
    ((65, 33, 2, 31, 17), {}),
)
# kfac_kron_cov_outer_sweep: ((cols, has_ones, nG, nb, nc, nt), options)
OUTER_SWEEP = (
    ((1, 0, 1, 1, 1, 1), {}),
    ((63, 1, 256, 2, 3, 16), {}),             # nG = WSEG, nt = RNTG
    ((64, 1, 257, 3, 2, 17), {}),
    ((130, 1, 10, 70, 2, 5), {}),
    ((20, 1, 40, 65, 32, 64), {}),
)
# one call of eight jobs per route: the jobs' shapes from the tables above, one (nb, nc[, nt])
JOBS8 = {
    "dense": (((1, 1), (5, 3), (27, 6), (64, 32), (683, 3), (65, 33), (63, 65), (20, 130)), (2, 3)),
    "outer": (((1, 0, 1), (63, 1, 10), (64, 1, 5), (64, 0, 7), (130, 1, 130), (12, 1, 6), (20, 1, 2049),
               (20, 1, 8)), (3, 5)),
    "sweep": (((16, 16), (257, 1), (3, 86), (27, 6), (65, 33), (3, 86), (16, 16), (27, 6)), (2, 3, 5)),
    "outer_sweep": (((1, 0, 1), (63, 1, 256), (64, 1, 257), (130, 1, 10), (20, 1, 40), (63, 1, 256),
                     (130, 1, 10), (20, 1, 40)), (3, 3, 5)),
}


def _job_spec(route, shape, lower, opts):
    if route in ("dense", "sweep"):
        nA, nG = shape
        cols, ones = nA, 0
    else:
        cols, ones, nG = shape
        nA = cols + ones
    j = NS(nA=nA, nG=nG, cols=cols, ones=ones, lower=bool(lower), skew=tuple(opts.get("skew", ())),
           nnz=opts.get("nnz", 8))
    j.ldJ = opts.get("ldJ", nA * nG + 7)
    j.ld1, j.ld2 = opts.get("ld1", nA + 3), opts.get("ld2", nG + 1)
    j.lda, j.ldD = opts.get("lda", cols + 3), opts.get("ldD", nG + 5)
    j.ldwA, j.ldwG = opts.get("ldwA", nA + 3), opts.get("ldwG", nG + 2)
    return j


def _build_specs():
    specs = {}

    def add(cid, route, jobs, nb, nc, nt=0, accumulate=False):
        assert cid not in specs, cid
        specs[cid] = NS(id=cid, route=route, jobs=tuple(jobs), nb=nb, nc=nc, nt=nt, accumulate=accumulate,
                        sweep=route in ("sweep", "outer_sweep"), outer=route in ("outer", "outer_sweep"))

    def name(route, shape, opts, lower=None):
        parts = [route, "x".join(map(str, shape))] + ([opts["tag"]] if "tag" in opts else [])
        return "-".join(parts + ([] if lower is None else ["lower" if lower else "dense"]))

    for shape, opts in DENSE:
        for lower in (True, False):
            add(name("dense", shape, opts, lower), "dense", [_job_spec("dense", shape[:2], lower, opts)], *shape[2:])
    for shape, opts in OUTER:
        for lower in (True, False):
            add(name("outer", shape, opts, lower), "outer", [_job_spec("outer", shape[:3], lower, opts)], *shape[3:])
    for shape, opts in SWEEP:
        add(name("sweep", shape, opts), "sweep", [_job_spec("sweep", shape[:2], False, opts)], *shape[2:])
    for shape, opts in OUTER_SWEEP:
        add(name("outer_sweep", shape, opts), "outer_sweep", [_job_spec("outer_sweep", shape[:3], False, opts)],
            *shape[3:])
    for route, (shapes, call) in JOBS8.items():
        for acc in (False, True):
            sweep = route in ("sweep", "outer_sweep")
            # the plain calls mix lower and dense factors
            jobs = [_job_spec(route, s, (not sweep) and i % 2 == 0, {}) for i, s in enumerate(shapes)]
            add(f"{route}-jobs8" + ("-acc" if acc else ""), route, jobs, *call, accumulate=acc)
    return specs


SPECS = _build_specs()
IDS = list(SPECS)
ROUTE_IDS = {r: [cid for cid in IDS if SPECS[cid].route == r] for r in ROUTES}
SINGLE_IDS = {r: [cid for cid in ROUTE_IDS[r] if "jobs8" not in cid] for r in ROUTES}
JOBS8_IDS = {r: [cid for cid in ROUTE_IDS[r] if "jobs8" in cid] for r in ROUTES}


# ------------------------------------------------------------------ data
def _sparse_rows(rng, shape, nnz, forced=()):
    """(groups, rows, width) int8: every row holds exactly min(nnz, width) entries of +-1 (no
    all-zero row).  The positions of a group's rows come from one pool of nnz + 4 columns, so
    the rows of a group overlap; the pool holds `forced`, and the group's first row takes the
    forced columns first."""
    groups, rows, width = shape
    out = np.zeros(shape, dtype=np.int8)
    forced = np.unique(np.asarray(forced, dtype=np.int64))
    size = min(width, max(nnz + 4, forced.size))
    k = min(nnz, width)
    for g in range(groups):
        rest = np.setdiff1d(np.arange(width), forced)
        pool = np.concatenate([forced, rng.choice(rest, size=size - forced.size, replace=False)])
        for r in range(rows):
            if r == 0 and forced.size:
                extra = rng.choice(pool[forced.size:], size=max(0, k - forced.size), replace=False)
                pos = np.concatenate([forced[:k], extra])
            else:
                pos = rng.choice(pool, size=k, replace=False)
            out[g, r, pos] = rng.choice([-1, 1], size=pos.size)
    return out


def _weights(rng, nt, n):
    """(nt, n) int8 weights in {0..3}; a vector of two or more entries holds a 0 and a 3.  The
    last entry is never 0 (it weights the last element of a row), so a single entry is 1, 2 or 3."""
    w = rng.integers(0, 4, size=(nt, n)).astype(np.int8)
    w[:, -1] = rng.integers(1, 4, size=nt)
    for t in range(nt if n > 1 else 0):
        i = int(rng.integers(n - 1))
        j = int(rng.choice(np.setdiff1d(np.arange(n), [i])))
        w[t, i], w[t, j] = 0, 3
    return w


def _reach_last_row(rng, K):
    """K with an entry in its last row (a dense draw can leave it empty, and then the ones
    entry of abar, or the last element of a row, reaches nothing): one entry of a column moved."""
    if not K[-1].any():
        c = int(rng.integers(K.shape[1]))
        r = int(rng.choice(np.flatnonzero(K[:, c])))
        K[-1, c], K[r, c] = K[r, c], 0
    return K


def _first_nonzero_rows(K, columns):
    return [int(np.flatnonzero(K[:, g])[0]) for g in columns]


def _job_data(spec, j, index):
    """The int8 operands of job `index` of case `spec`."""
    rng = np.random.default_rng(zlib.crc32(repr(("glm_exact", spec.id.replace("-acc", ""), index)).encode()))
    d = NS()
    d.K1 = _reach_last_row(rng, sparse_signs(rng, j.nA, j.lower)).astype(np.int8)
    d.K2 = _reach_last_row(rng, sparse_signs(rng, j.nG, j.lower)).astype(np.int8)
    if spec.outer:
        d.a = _sparse_rows(rng, (spec.nb, 1, j.cols), j.nnz)[:, 0]
        # D reaches the last column of V and the first one of a second Gram segment
        special = [j.nG - 1] + [s for s in (GSEG, WSEG) if s < j.nG]
        d.D = _sparse_rows(rng, (spec.nb, spec.nc, j.nG), j.nnz, _first_nonzero_rows(d.K2, special))
    else:
        d.J = rng.integers(-1, 2, size=(spec.nb, spec.nc, j.nA * j.nG)).astype(np.int8)
        d.J[:, :, -1] = rng.choice([-1, 1], size=(spec.nb, spec.nc))  # the last element of a row is never 0
    if spec.sweep:
        d.wA, d.wG = _weights(rng, spec.nt, j.nA), _weights(rng, spec.nt, j.nG)
    return d


def _operands(spec, j):
    """(name, rows, cols, pitch) of job j's regions, in buffer order."""
    rows = spec.nb * spec.nc
    ops = [("a", spec.nb, j.cols, j.lda), ("D", rows, j.nG, j.ldD)] if spec.outer else \
        [("J", rows, j.nA * j.nG, j.ldJ)]
    ops += [("K1", j.nA, j.nA, j.ld1), ("K2", j.nG, j.nG, j.ld2)]
    if spec.sweep:
        ops += [("wA", spec.nt, j.nA, j.ldwA), ("wG", spec.nt, j.nG, j.ldwG)]
    return ops


def _index(region):
    return region.off + np.arange(region.rows)[:, None] * region.ld + np.arange(region.cols)[None, :]


@functools.lru_cache(maxsize=None)
def case(cid):
    """The case's spec, data, flat buffer and where everything sits in it (elements)."""
    spec = SPECS[cid]
    c = NS(**vars(spec))
    c.data = [_job_data(spec, j, i) for i, j in enumerate(spec.jobs)]
    c.regions, end = [], 0
    for i, (j, d) in enumerate(zip(spec.jobs, c.data)):
        for name, rows, cols, ld in _operands(spec, j):
            assert ld >= cols
            off = (end + GAP + 3) // 4 * 4 + (1 if name in j.skew else 0)
            c.regions.append(NS(name=f"{name}[{i}]", op=name, job=i, off=off, rows=rows, cols=cols, ld=ld,
                                end=off + rows * ld))
            end = off + rows * ld
    c.cov_shape = ((spec.nt,) if spec.sweep else ()) + (spec.nb, spec.nc, spec.nc)
    ncov = int(np.prod(c.cov_shape))
    off = (end + GAP + 3) // 4 * 4
    c.cov = NS(name="cov", op="cov", job=-1, off=off, rows=1, cols=ncov, ld=ncov, end=off + ncov)
    c.regions.append(c.cov)
    c.size = c.cov.end + GAP
    flat = np.full(c.size, np.nan, dtype=F32)
    for r in c.regions[:-1]:
        flat[_index(r)] = getattr(c.data[r.job], r.op).reshape(r.rows, r.cols)
    if spec.accumulate:  # a symmetric integer prefill
        rng = np.random.default_rng(zlib.crc32(repr(("glm_exact prefill", cid)).encode()))
        P = rng.integers(-2, 3, size=c.cov_shape).astype(np.int64)
        c.prefill = P + np.swapaxes(P, -1, -2)
        flat[c.cov.off:c.cov.end] = c.prefill.reshape(-1)
    else:
        c.prefill = None
    c.flat = flat
    flat.setflags(write=False)
    return c


def region_of(c, element):
    """The name of the region element `element` of the flat buffer falls in."""
    for r in c.regions:
        if r.off <= element < r.end:
            row, col = divmod(element - r.off, r.ld)
            return f"{r.name} row {row} column {col}" + (" (padding)" if col >= r.cols else "")
    return "a gap between regions"


# ------------------------------------------------------------------ int64 reference
# name -> what a kernel would have done (the host test lists the cases that must see it)
MISTAKES = {
    "K1_transposed": "K1 read as its transpose",
    "K2_transposed": "K2 read as its transpose",
    "flatten_ga": "a Jacobian row viewed with element (a, g) at g*nA + a",
    "drop_last": "the last K element of every row left out of the Gram",
    "drop_segment2_first": "the first element of the second Gram segment left out",
    "ones_omitted": "the ones entry of abar omitted",
    "ones_from_a": "the ones entry of abar taken from a[b][cols-1]",
    "sample_offset_32": "sample b's rows taken at offset 32*b instead of nc*b",
    "mirror_upper": "the (unwritten) upper triangle of the partials mirrored instead of the lower",
    "accumulate_ignored": "accumulate ignored",
    "rank1_swapped": "the rank-one weight indexed wA[k % nA] * wG[k / nA]",
    "tau_next": "grid point tau given tau + 1's weights",
    "rownorm_next_tile": "the row-norm weights of the neighbouring column tile",
    "scale_next_sample": "the scale s_j[b] of the neighbouring sample",
}


class _Peak:
    """The largest magnitude seen (meaningful on an absolute-value evaluation)."""

    def __init__(self):
        self.value = 0

    def __call__(self, x):
        if x.size:
            self.value = max(self.value, int(np.abs(x).max()))
        return x


def _gram(X, w, seg, mistake, see):
    """(nt or 1, nb, nc, nc): sum_k w[t][k] X[b][c][k] X[b][d][k], X (nb, nc, K) int64, w (nt, K) or None."""
    nb, nc, K = X.shape
    if mistake == "sample_offset_32":
        rows = (32 * np.arange(nb)[:, None] + np.arange(nc)[None, :]) % (nb * nc)
        X = X.reshape(nb * nc, K)[rows]
    if mistake == "drop_last":
        X = X.copy()
        X[:, :, K - 1] = 0
    if mistake == "drop_segment2_first" and K > seg:
        X = X.copy()
        X[:, :, seg] = 0
    see(X * X)
    if w is None:
        return see(np.einsum("bck,bdk->bcd", X, X))[None]
    see(w[:, None, None, :] * (X * X)[None])
    return see(np.stack([np.einsum("bck,bdk->bcd", X * wt[None, None, :], X) for wt in w]))


def _dense_job(spec, j, d, mistake, ab, see):
    """sum_k (w[k]) T[b][c][k] T[b][d][k], T_r = K1^T M_r K2 flattened a*nG + g."""
    cast = (lambda t: np.abs(t.astype(np.int64))) if ab else (lambda t: t.astype(np.int64))
    K1, K2, J = cast(d.K1), cast(d.K2), cast(d.J)
    nb, nc, nA, nG = spec.nb, spec.nc, j.nA, j.nG
    M = J.reshape(nb, nc, nG, nA).transpose(0, 1, 3, 2) if mistake == "flatten_ga" else J.reshape(nb, nc, nA, nG)
    K1 = K1.T if mistake == "K1_transposed" else K1
    K2 = K2.T if mistake == "K2_transposed" else K2
    U = see(np.einsum("ka,bckg->bcag", K1, M))
    T = see(np.einsum("bcag,gh->bcah", U, K2)).reshape(nb, nc, nA * nG)
    w = None
    if spec.sweep:
        wA, wG = cast(d.wA), cast(d.wG)
        k = np.arange(nA * nG)
        w = wA[:, k % nA] * wG[:, k // nA] if mistake == "rank1_swapped" else wA[:, k // nG] * wG[:, k % nG]
        if mistake == "tau_next":
            w = np.roll(w, -1, axis=0)
        see(w)
    return _gram(T, w, WSEG if spec.sweep else GSEG, mistake, see)


def _outer_job(spec, j, d, mistake, ab, see):
    """s[t][b] * sum_g (wG[t][g]) V[b][c][g] V[b][d][g], s = sum_i (wA[t][i]) (abar K1)[b][i]^2, V = D K2."""
    cast = (lambda t: np.abs(t.astype(np.int64))) if ab else (lambda t: t.astype(np.int64))
    K1, K2, a, D = cast(d.K1), cast(d.K2), cast(d.a), cast(d.D)
    K1 = K1.T if mistake == "K1_transposed" else K1
    K2 = K2.T if mistake == "K2_transposed" else K2
    abar = a
    if j.ones:
        one = np.ones((spec.nb, 1), dtype=np.int64)
        if mistake == "ones_omitted":
            one = 0 * one
        if mistake == "ones_from_a":
            one = a[:, -1:]
        abar = np.concatenate([a, one], axis=1)
    p = see(abar @ K1)                       # (nb, nA)
    V = see(D.reshape(-1, j.nG) @ K2).reshape(spec.nb, spec.nc, j.nG)
    if spec.sweep:
        wA, wG = cast(d.wA), cast(d.wG)
        if mistake == "rownorm_next_tile":   # column i of tile t weighted as column i of tile t + 1 (0 past nA)
            tiles = -(-j.nA // TILE)
            i = np.arange(j.nA)
            src = ((i // TILE + 1) % tiles) * TILE + i % TILE
            wA = np.where(src < j.nA, wA[:, np.minimum(src, j.nA - 1)], 0)
        if mistake == "tau_next":
            wA, wG = np.roll(wA, -1, axis=0), np.roll(wG, -1, axis=0)
        see(wA[:, None, :] * (p * p)[None])
        s = see(np.einsum("ti,bi->tb", wA, p * p))
    else:
        wG = None
        s = see((p * p).sum(axis=1))[None]
    if mistake == "scale_next_sample":
        s = np.roll(s, -1, axis=1)
    return see(s[:, :, None, None] * _gram(V, wG, WSEG if spec.sweep else GSEG, mistake, see))


def _evaluate(c, mistake, ab):
    assert mistake is None or mistake in MISTAKES, mistake
    see = _Peak()
    job = _outer_job if c.outer else _dense_job
    total = 0
    for j, d in zip(c.jobs, c.data):
        total = see(total + job(c, j, d, mistake, ab, see))
    if mistake == "mirror_upper":  # only the lower triangle of a partial is written: what is left is the diagonal
        total = total * np.eye(c.nc, dtype=np.int64)
    if c.accumulate and mistake != "accumulate_ignored":
        total = see(total + (np.abs(c.prefill) if ab else c.prefill))
    return total.reshape(c.cov_shape), see.value


def reference(c, mistake=None):
    """cov as int64, c.cov_shape; with `mistake`, what the named mistake would give."""
    if mistake is None:
        return _reference(c.id)
    return _evaluate(c, mistake, False)[0]


@functools.lru_cache(maxsize=None)
def _reference(cid):
    ref = _evaluate(case(cid), None, False)[0]
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def _bound(cid):
    return _evaluate(case(cid), None, True)[1]


def bound(c):
    """The largest magnitude any partial sum of the case can reach: the whole chain once on
    the absolute values of every operand."""
    return _bound(c.id)


def want(c):
    """The flat buffer after the call: the int64 reference in `cov`, everything else as it was."""
    out = np.array(c.flat)
    out[c.cov.off:c.cov.end] = reference(c).reshape(-1)
    return out


def same(a, b):
    """Equal element for element, NaN matching NaN."""
    return np.array_equal(np.asarray(a, dtype=F32), np.asarray(b, dtype=F32), equal_nan=True)


def differing(got, expect):
    """Indices where got and expect differ (NaN matching NaN)."""
    return np.flatnonzero(~((got == expect) | (np.isnan(got) & np.isnan(expect))))


# ------------------------------------------------------------------ the raw calls
def native_jobs(N, c, base):
    """The ctypes job array of case c on its flat buffer uploaded at byte address `base`."""
    at = {r.name: base + 4 * r.off for r in c.regions}
    jobs = []
    for i, j in enumerate(c.jobs):
        p = lambda op: at[f"{op}[{i}]"]  # noqa: E731
        if c.route == "dense":
            jobs.append(N.CovJob(p("J"), j.ldJ, j.nA, j.nG, p("K1"), j.ld1, p("K2"), j.ld2, int(j.lower), int(j.lower)))
        elif c.route == "outer":
            jobs.append(N.CovOuterJob(p("a"), j.lda, j.cols, j.ones, p("D"), j.ldD, j.nG, 0, p("K1"), j.ld1,
                                      p("K2"), j.ld2, int(j.lower), int(j.lower)))
        elif c.route == "sweep":
            jobs.append(N.CovSweepJob(p("J"), j.ldJ, j.nA, j.nG, p("K1"), j.ld1, p("K2"), j.ld2, p("wA"), j.ldwA,
                                      p("wG"), j.ldwG))
        else:
            jobs.append(N.CovOuterSweepJob(p("a"), j.lda, j.cols, j.ones, p("D"), j.ldD, j.nG, 0, p("K1"), j.ld1,
                                           p("K2"), j.ld2, p("wA"), j.ldwA, p("wG"), j.ldwG))
    return N.as_array(type(jobs[0]), jobs)


SYMBOL = {"dense": "kfac_kron_cov", "outer": "kfac_kron_cov_outer", "sweep": "kfac_kron_cov_sweep",
          "outer_sweep": "kfac_kron_cov_outer_sweep"}


def workspace_bytes(N, c, jobs):
    """The query's answer for case c (host only)."""
    query = getattr(N.lib(), SYMBOL[c.route] + "_workspace_bytes")
    return query(jobs, len(c.jobs), c.nb, c.nc, *((c.nt,) if c.sweep else ()))


def call(N, c, jobs, base, workspace, nbytes, stream):
    """The raw C entry point of c's route on the flat buffer at `base`; returns its status."""
    fn = getattr(N.lib(), SYMBOL[c.route])
    return fn(jobs, len(c.jobs), c.nb, c.nc, *((c.nt,) if c.sweep else ()), int(c.accumulate),
              base + 4 * c.cov.off, workspace, nbytes, stream)
