"""Term-exact inputs for the bf16x3 factor kernels (a plain helper module, like host_double).

A bf16x3 kernel splits every operand element into three bf16 parts, x = hi + mid + lo
(split3, bnn_kfac_amd/csrc/bf16x3.h), and sums six of the nine part products: hi hi, hi mid,
mid hi, mid mid, hi lo, lo hi.  The inputs built here make that six-term sum exactly
representable in fp32 in every summation order, with all three parts non-zero, so a kernel
must reproduce `six_term` bit for bit and any lost, doubled or mis-paired small term shows.

Live elements take
  "full" values  s {1, 1 + 2^-9, 1 + 2^-9 + 2^-18}, s = +-1: parts (s, 0, 0), (s, s 2^-9, 0)
                 and (s, s 2^-9, s 2^-18);
  "pure" values  {-1, 0, 1};
every other element is 0.  (1 + 2^-18 alone is not used: its mid part is 2^-18 and mid mid
leaves the grid.)  Every kept product is then a multiple of 2^-18, and with at most R = 16
live K-rows per output entry every partial sum stays below 32 < 2^6: 24 bits, one to spare.
The one entry outside that bound is ones x ones, the row count: a sum of hi hi = 1 terms, an
integer below 2^24 and exact for that reason.

Row-major and CHANNEL operands: a column (channel) c is pure when (c + c // 32) % 4 == 3,
full otherwise -- three quarters full, mixed inside every 32-column panel -- and a full
column's 16 live elements are 5 / 6 / 5 of the three full values in a shuffled order: an odd
number of lo parts (5) and of mid parts (11), so the hi lo and hi mid sums against a full
column cannot cancel.  PATCH operands: the live pixels are one compact patch of sites shared
by all channels; each channel's 16 sites are 3 / 4 / 5 full values and 4 pure ones (0 and three +-1), shuffled.

A job with n <= 32 in a row-major launch group runs on the fp32 MFMA (factor_task_narrow_direct):
its products are the full fp32 ones, mid lo and lo lo included, which no fp32 sum holds
exactly.  Such a job (`fp32`) draws its full values from s {1, 1 + 2^-9} only: lo is zero,
the nine-term product equals the six-term one and stays on the 2^-18 grid, so the bit-exact
comparison holds for it too; the lo conditions do not apply to it.

The table `GROUPS` is shared by the host test of the data (test_x3_exact_data.py) and the
GPU test of the kernels (test_gpu_x3_term_exact.py)."""
import functools

import numpy as np

from oracle import kfac_oracle as O

U9, U18 = 2.0 ** -9, 2.0 ** -18
FULL = np.array([1.0, 1.0 + U9, 1.0 + U9 + U18])
R = 16  # live K-rows per output entry (PATCH jobs: live sites; see patch_sites)
# the six kept products, as (name, part of the row operand, part of the column operand):
# term (p, q) adds parts[p]^T parts[q]
TERMS = (("hh", 0, 0), ("hm", 0, 1), ("mh", 1, 0), ("mm", 1, 1), ("hl", 0, 2), ("lh", 2, 0))


def _bf16(x):
    """float32 -> the nearest bf16 (ties to even), as float32 (v_cvt_pk_bf16_f32)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7fff)
    return ((u + r) & np.uint32(0xffff0000)).view(np.float32)


def split3(x):
    """split3 of bf16x3.h on a float32 array: bf16 of x, of the fp32 residual, and of that
    one's residual.  Returns fp64 arrays h, m, l with h + m + l == x exactly."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    h = _bf16(x)
    r = x - h
    m = _bf16(r)
    s = r - m
    l = _bf16(s)
    h, m, l = (p.astype(np.float64) for p in (h, m, l))
    assert np.array_equal(h + m + l, x.astype(np.float64))
    return h, m, l


def six_term(cols_h, cols_m, cols_l):
    """The factor a bf16x3 kernel computes from the operand's column parts ((K, n) each, the
    ones column in cols_h): h^T h + h^T m + m^T h + m^T m + h^T l + l^T h, in fp64."""
    parts = (cols_h, cols_m, cols_l)
    return sum(parts[p].T @ parts[q] for _, p, q in TERMS)


def sequential_fp32(parts, rng, terms=TERMS):
    """The kernels' arithmetic in its plainest form: every (K-row, term) rank-one product
    added to an fp32 accumulator, one at a time, in a shuffled order."""
    h = parts[0]
    K, n = h.shape
    acc = np.zeros((n, n), np.float32)
    p32 = [p.astype(np.float32) for p in parts]
    support = [[np.flatnonzero(p[k]) for p in parts] for k in range(K)]
    for idx in rng.permutation(K * len(terms)):
        k, (_, p, q) = idx // len(terms), terms[idx % len(terms)]
        i, j = support[k][p], support[k][q]
        if i.size and j.size:
            acc[np.ix_(i, j)] += np.outer(p32[p][k, i], p32[q][k, j])
    return acc


def pure_column(c):
    return (c + c // 32) % 4 == 3


def _signs(rng, shape):
    return rng.integers(0, 2, size=shape) * 2.0 - 1.0


def _live_columns(rng, cols, fp32):
    """(R, cols) live elements of a row-major / CHANNEL operand."""
    counts = (7, 9, 0) if fp32 else (5, 6, 5)
    kinds = np.repeat(np.arange(3), counts)
    kinds = rng.permuted(np.tile(kinds, (cols, 1)), axis=1).T
    v = FULL[kinds] * _signs(rng, (R, cols))
    pure = np.array([pure_column(c) for c in range(cols)])
    v[:, pure] = rng.integers(-1, 2, size=(R, int(pure.sum())))
    return v.astype(np.float32)


def live_rows(rng, rows, nseg):
    """R live rows of nseg batches of `rows`: row 0, the last row, both sides of a 16-row
    and of a 32-row boundary, both sides of every batch boundary, the rest drawn."""
    K = rows * nseg
    must = {0, 15, 16, 31, 32, K - 1}
    for s in range(1, nseg):
        must |= {s * rows - 1, s * rows}
    rest = [k for k in rng.permutation(K) if k not in must]
    out = sorted(must | set(rest[:R - len(must)]))
    assert len(out) == R
    return out


def patch_sites(where, B, H, W, ph=4, pw=4):
    """The live pixels (image, row, column) of a PATCH operand: one ph x pw patch against
    the top-left padding of the first image, in the bottom-right corner of the last image,
    or in the interior of the middle one."""
    b, r0, c0 = {"topleft": (0, 0, 0), "bottomright": (B - 1, H - ph, W - pw),
                 "interior": (B // 2, (H - ph) // 2, (W - pw) // 2)}[where]
    return [(b, r0 + r, c0 + c) for r in range(ph) for c in range(pw)]


class Job:
    """One factor job: its operand on the host, its column parts and its expected factor."""

    def __init__(self, name, layout, ones, batches, conv=None, fp32=False):
        self.name, self.layout, self.ones, self.batches = name, layout, ones, batches
        self.conv = conv  # PATCH: (kernel, stride, padding)
        self.fp32 = fp32  # computed on the fp32 MFMA (module docstring): no lo parts

    def _columns(self, a):
        """(K, cols) operand columns of one array shaped like the operand."""
        if self.layout == "rowmajor":
            return a
        if self.layout == "channel":
            B, C = a.shape[:2]
            return a.reshape(B, C, -1).transpose(0, 2, 1).reshape(-1, C)
        k, s, p = self.conv
        u = O.unfold(a, k, p, s)  # (the split is elementwise and the padding zero: it
        return u.transpose(0, 2, 1).reshape(-1, u.shape[1])  # commutes with the im2col)

    @functools.cached_property
    def parts(self):
        """(h, m, l): fp64 (K, n) column parts, the ones column (pure) in h."""
        x = np.concatenate(self.batches)
        out = [self._columns(p) for p in split3(x)]
        if self.ones:
            K = out[0].shape[0]
            out = [np.concatenate([p, np.full((K, 1), float(i == 0))], 1) for i, p in enumerate(out)]
        return tuple(out)

    @functools.cached_property
    def want(self):
        return six_term(*self.parts)

    @property
    def n(self):
        return self.parts[0].shape[1]


def _rowmajor_job(rng, cols, ones, rows, nseg):
    x = np.zeros((rows * nseg, cols), np.float32)
    fp32 = cols + ones <= 32
    x[live_rows(rng, rows, nseg)] = _live_columns(rng, cols, fp32)
    return Job(f"{cols}+{int(ones)}", "rowmajor", ones, list(x.reshape(nseg, rows, cols)), fp32=fp32)


def _patch_job(rng, spec, where):
    B, C, H, W, _, k, s, p, bias = spec
    sites = patch_sites(where, B, H, W)
    assert len(sites) == R
    x = np.zeros((B, C, H, W), np.float32)
    kinds = np.repeat(np.arange(4), (3, 4, 5, 4))  # 3 = pure
    for c in range(C):
        kd = rng.permutation(kinds)
        # (the pure sites: one 0 and three +-1, so 15 of a channel's 16 hi parts are +-1 --
        # an odd count, and the bias row's sum over them cannot cancel)
        pure = np.zeros(R)
        pure[np.flatnonzero(kd == 3)[1:]] = 1.0
        v = np.where(kd < 3, FULL[np.minimum(kd, 2)], pure) * _signs(rng, R)
        for (b, r, q), val in zip(sites, v):
            x[b, c, r, q] = val
    return Job(where, "patch", bias, [x], conv=(k, s, p))


def _channel_job(rng, B, C, hw):
    """16 live positions, all channels: the first image's first two k-steps, the last image
    and the last k-step (16 positions) of an image."""
    L = hw * hw
    g = np.zeros((B, C, L), np.float32)
    last = 16 * ((L - 1) // 16)  # first position of an image's last k-step
    pos = [(0, 0), (0, 1), (0, 15), (0, 16), (0, 17), (0, last), (0, L - 1), (B // 2, 7), (B // 2, last),
           (B // 2, L - 1), (B - 1, 0), (B - 1, 15), (B - 1, 16), (B - 1, last), (B - 1, L - 2), (B - 1, L - 1)]
    assert len(set(pos)) == R
    v = _live_columns(rng, C, False)
    for (b, q), row in zip(pos, v):
        g[b, :, q] = row
    return Job(f"{B}x{C}x{hw}", "channel", False, [g.reshape(B, C, hw, hw)])


TILES_SIZES = [(256, True), (320, False), (784, True), (10, True)]  # (cols, ones)
SYRK3_SIZES = [(2048, False), (2052, True)]
# (B, Cin, H, W, Cout, kernel, stride, padding, bias): the shapes test_gpu_factors.py routes
# to each conv family
CONV_SPECS = {
    "conv_x3": [(2, 20, 10, 10, 5, (3, 3), (1, 1), (0, 0), True), (3, 1, 20, 20, 4, (4, 8), (1, 1), (0, 0), True)],
    "conv_x3s": [(5, 2, 11, 13, 4, (3, 4), (2, 1), (1, 2), True), (2, 2, 9, 9, 3, (4, 4), (1, 1), (1, 1), False)],
    "conv_x3f": [(3, 9, 5, 13, 5, (3, 4), (1, 1), (1, 2), True), (2, 10, 7, 8, 3, (3, 5), (1, 1), (1, 1), False)],
}
CHANNEL_SIZES = [(5, 9, 22), (40, 32, 6)]  # (B, C, hw)
PLACES = ["topleft", "bottomright", "interior"]


class Group:
    """The jobs of one kfac_factor_update call, all on one kernel family."""

    def __init__(self, gid, family, njobs, build, mode="plain"):
        self.id, self.family, self.njobs, self.mode, self._build = gid, family, njobs, mode, build

    @functools.cached_property
    def jobs(self):  # (built once; the two tests share the data and the expected factors)
        return self._build()


def _groups():
    out = []

    def rowmajor(sizes, seed, rows, nseg):
        def build():
            rng = np.random.default_rng(seed)
            return [_rowmajor_job(rng, cols, ones, rows, nseg) for cols, ones in sizes]
        return build
    for seed in range(3):
        out.append(Group(f"tiles_x3-seed{seed}", "tiles_x3", len(TILES_SIZES), rowmajor(TILES_SIZES, seed, 96, 1)))
    out.append(Group("tiles_x3-nseg3", "tiles_x3", len(TILES_SIZES), rowmajor(TILES_SIZES, 3, 64, 3)))
    out.append(Group("tiles_x3-deferred", "tiles_x3", len(TILES_SIZES), rowmajor(TILES_SIZES, 4, 96, 1),
                     mode="deferred"))
    out.append(Group("syrk3", "syrk3", len(SYRK3_SIZES), rowmajor(SYRK3_SIZES, 5, 96, 1)))
    for family, specs in CONV_SPECS.items():
        for i, spec in enumerate(specs):
            for where in PLACES:
                seed = 100 + 10 * len(out)
                out.append(Group(f"{family}-{i}-{where}", family, 1,
                                 lambda spec=spec, where=where, seed=seed:
                                 [_patch_job(np.random.default_rng(seed), spec, where)]))
    for i, (B, C, hw) in enumerate(CHANNEL_SIZES):
        out.append(Group(f"channel_x3-{i}", "channel_x3", 1,
                         lambda B=B, C=C, hw=hw, i=i: [_channel_job(np.random.default_rng(200 + i), B, C, hw)]))
    return out


GROUPS = _groups()
GROUP_IDS = [g.id for g in GROUPS]
