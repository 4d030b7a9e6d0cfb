"""GPU: the fp64 inversion (invert.hip, invert_merged.hip, invert_blocked.hip,
invert_tiles.inc) against the rounding-derived bounds of inv_cases.py: every case at the tile,
diagonal-block, task-pairing, panel-block and look-ahead edges of either path, strided and
unaligned operands, calls of more than one group, and the value of `info`.

A call's path is set by its largest job, so the blocked kernels (64-tiles) are reached with
small jobs by putting one n = 1537 job in the call; "alone on the blocked path" below means
alone with that companion."""
import numpy as np
import pytest
import torch

import inv_cases as C

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
GRAPH, LOOKAHEAD = "KFAC_INV_GRAPH", "KFAC_INV_LOOKAHEAD"


class Spec:
    """One job: an fp32 F, its damping and output kind, and (when it is a named case) the
    oracle that judges it."""

    def __init__(self, F, scale=1.0, shift=0.0, kind=C.CHOL, name=None):
        self.F, self.scale, self.shift, self.kind, self.name = F, float(scale), float(shift), kind, name
        self.n = F.shape[0]

    @classmethod
    def case(cls, name, n, kind=C.CHOL):
        F, scale, shift = C.problem(name, n)
        return cls(F, scale, shift, kind, name)

    def check(self, out, tag=""):
        if self.name is not None:
            f = C.check_output(self.name, self.n, self.kind, out)
        else:
            o = C.oracle_of(self.F, self.scale, self.shift)
            f = (C.check_chol(o.R, o.G, out, tag=tag) if self.kind == C.CHOL
                 else C.check_inverse(o.R, out, tag=tag))
            if self.kind == C.CHOL:
                f.update(C.check_forward(o, out, tag))
        print(f"INV-GPU {C.family_of(self.name) if self.name else 'custom'} {self.name}-{self.n}-{self.kind}"
              f"{tag}: {f['ratio']:.4f} forward {f.get('forward', float('nan')):.4f}")
        return f


def _big(kind=C.CHOL):
    return Spec.case("spd_1e2", C.BLOCKED_N, kind)


def _layout(specs, dev, pad_f, pad_o):
    """Device operands of a call.  Contiguous (pad 0), or F as a view with ldF = n + pad_f
    whose base is one element past the allocation's (NaN around it) and out as a view with
    ldo = n + pad_o (the sentinel around it).  Outputs start as NaN."""
    from bnn_kfac_amd import _native as N
    kinds = {C.CHOL: N.OUT_INV_CHOL, C.INVERSE: N.OUT_INVERSE}
    jobs, keep = [], []
    for s in specs:
        n, off = s.n, 1 if pad_f else 0
        fb = torch.full((off + n * (n + pad_f),), float("nan"), dtype=torch.float32, device=dev)
        Fv = fb[off:].view(n, n + pad_f)[:, :n]
        Fv.copy_(torch.from_numpy(np.array(s.F)))  # (a copy: the shared cases are read-only)
        ob = torch.full((n, n + pad_o), SENTINEL, dtype=torch.float32, device=dev)
        ob[:, :n] = float("nan")
        jobs.append(N.invert_job(Fv, ob[:, :n], s.scale, s.shift, kinds[s.kind]))
        assert jobs[-1].ldF == n + pad_f and jobs[-1].ldo == n + pad_o
        keep.append((fb, ob))
    return jobs, keep


def _run(specs, dev, pad_f=0, pad_o=0):
    """One grouped call; returns ([out n x n numpy], info numpy, [out's padding numpy])."""
    from bnn_kfac_amd import _native as N
    jobs, keep = _layout(specs, dev, pad_f, pad_o)
    info = N.invert(jobs, dev)
    torch.cuda.synchronize()
    outs, pads = [], []
    for s, (_, ob) in zip(specs, keep):
        o = ob.cpu().numpy()
        outs.append(np.ascontiguousarray(o[:, :s.n]))
        pads.append(o[:, s.n:])
    return outs, info.cpu().numpy(), pads


class _knob:
    """A launch knob set for a block and restored after it."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        from bnn_kfac_amd import _native as N
        self.before = N.get_knob(self.name)
        N.set_knob(self.name, self.value)

    def __exit__(self, *exc):
        from bnn_kfac_amd import _native as N
        N.set_knob(self.name, self.before)


def _run_knob(specs, dev, knob, value, **kw):
    with _knob(knob, value):
        return _run(specs, dev, **kw)


def _same(a, b):
    """Bitwise equality (NaN equal to NaN: a failed job's output is not compared at all)."""
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------ 1. bounds
def _merged_case(name, n, dev):
    for kind in C.kinds_of(name):
        s = Spec.case(name, n, kind)
        (on,), info_on, _ = _run_knob([s], dev, GRAPH, 1)
        (off,), info_off, _ = _run_knob([s], dev, GRAPH, 0)
        assert info_on[0] == 0 and info_off[0] == 0, (name, n, kind, info_on, info_off)
        s.check(on)
        assert _same(on, off), f"{name}-{n}-{kind}: graph replay and plain launches differ"
        if name == "nonsym_grid":  # the run on F is the run on its symmetric part
            (sym,), info, _ = _run([Spec(C.sym_part(s.F), s.scale, s.shift, kind)], dev)
            assert info[0] == 0 and _same(on, sym), f"{name}-{n}-{kind}: F and (F + F^T)/2 differ"


@pytest.mark.parametrize("name", C.NAMES)
def test_merged_bounds(hip_device, name):
    """Every case at T = 1 .. 7 tiles of 32 (n = 1 .. 193), both kinds where the case allows,
    the graph replay (staged outputs) bit-equal to the plain launches."""
    for n in C.MERGED_SMALL:
        _merged_case(name, n, hip_device)


@pytest.mark.parametrize("name", C.NAMES)
def test_merged_bounds_largest(hip_device, name):
    """n = 1536, the largest size on 32-tiles (T = 48)."""
    _merged_case(name, C.MERGED_LARGE, hip_device)


@pytest.mark.parametrize("name", C.NAMES)
def test_blocked_bounds(hip_device, name):
    """Every case as companions of one n = 1537 job (64-tiles: T = 1, 2, 3, 6, 7, 12, 13),
    both kinds where the case allows, the look-ahead split bit-equal to the single bulk."""
    for sizes in C.BLOCKED_CALLS:
        for kind in C.kinds_of(name):
            specs = [_big()] + [Spec.case(name, n, kind) for n in sizes]
            la1, info1, _ = _run_knob(specs, hip_device, LOOKAHEAD, 1)
            la0, info0, _ = _run_knob(specs, hip_device, LOOKAHEAD, 0)
            assert not info1.any() and not info0.any(), (name, sizes, kind, info1, info0)
            for s, a in zip(specs[1:], la1[1:]):
                s.check(a, " blocked")
            for s, a, b in zip(specs, la1, la0):
                assert _same(a, b), f"{name}-{s.n}-{kind}: look-ahead 1 and 0 differ"


@pytest.mark.parametrize("kind", [C.CHOL, C.INVERSE])
def test_blocked_largest_job(hip_device, kind):
    """The n = 1537 job itself (T = 25: five panel blocks, four with look-ahead)."""
    s = _big(kind)
    (la1,), info1, _ = _run_knob([s], hip_device, LOOKAHEAD, 1)
    (la0,), info0, _ = _run_knob([s], hip_device, LOOKAHEAD, 0)
    assert info1[0] == 0 and info0[0] == 0
    s.check(la1, " blocked")
    assert _same(la1, la0)


# ------------------------------------------------------------------------ 2. strides
STRIDED_GROUPS = {
    # all inverse-Cholesky: the graph replay, staged outputs, inv_copy_out's ldo
    "merged_graph": lambda: [Spec.case("kfac_A_1e-4", 33), Spec.case("spd_1e2_skew", 97),
                             Spec.case("nonsym_grid", 16), Spec.case("kfac_G", 65)],
    # a full inverse in the group: plain launches, emit_out / emit_zero_block / inv_out's ldo
    "merged_plain": lambda: [Spec.case("kfac_A_1e-4", 33), Spec.case("spd_1e5_skew", 97, C.INVERSE),
                             Spec.case("nonsym_grid", 17), Spec.case("kfac_G", 65, C.INVERSE)],
    "blocked": lambda: [_big(), Spec.case("spd_1e5_skew", 65), Spec.case("kfac_A_1e-4", 129, C.INVERSE),
                        Spec.case("nonsym_grid", 17, C.INVERSE)],
}


@pytest.mark.parametrize("group", STRIDED_GROUPS)
def test_strided_unaligned_operands(hip_device, group):
    """ldF = n + 3 from a base one element off the allocation's (NaN all around F), ldo =
    n + 5 (a sentinel around out): the bits of the contiguous call, the sentinel intact.
    Contiguous, strided, contiguous on one shape: the merged path's cached graph is
    re-parameterised in place between them."""
    specs = STRIDED_GROUPS[group]()
    c0, i0, _ = _run(specs, hip_device)
    st, i1, pads = _run(specs, hip_device, pad_f=3, pad_o=5)
    c1, i2, _ = _run(specs, hip_device)
    assert not i0.any() and not i1.any() and not i2.any()
    for s, a, b, c, pad in zip(specs, c0, st, c1, pads):
        if s.n < C.BLOCKED_N:
            s.check(a, f" {group}")
        assert _same(a, b), f"{s.name}-{s.n}: strided and contiguous differ"
        assert _same(a, c), f"{s.name}-{s.n}: the second contiguous call differs"
        assert pad.shape == (s.n, 5) and (pad == SENTINEL).all(), f"{s.name}-{s.n}: padding written"


# ------------------------------------------------------------------------ 3. more than 8 jobs
def _check_against_alone(specs, dev, companion=None, skip_check=()):
    """One grouped call; every job meets its bound and equals, bit for bit, the same job
    solved alone on the same path (with `companion` first when given)."""
    outs, info, _ = _run(specs, dev)
    assert not info.any(), info
    for i, (s, got) in enumerate(zip(specs, outs)):
        if i not in skip_check:
            s.check(got, f" job {i} of {len(specs)}")
        if companion is not None and i == 0:
            continue
        alone, info1, _ = _run(([companion] if companion is not None else []) + [s], dev)
        assert not info1.any()
        assert _same(got, alone[-1]), f"job {i} ({s.name}-{s.n}-{s.kind}) differs from its solo solve"


def test_ten_jobs_two_modes(hip_device):
    """Group 0: eight inverse-Cholesky jobs (graph replay, staged).  Group 1 (info + 8, its
    own workspace offset): a full inverse and an inverse-Cholesky (plain launches)."""
    sizes = (33, 1, 65, 17, 97, 32, 161, 16, 64, 40)
    names = ("kfac_A_1e-4", "spd_1e5", "kfac_G", "nonsym_grid", "spd_1e5_skew", "block_diag",
             "kfac_A_bench", "graded_diag", "spd_1e2_skew", "kfac_A_1e-3")
    kinds = (C.CHOL,) * 8 + (C.INVERSE, C.CHOL)
    _check_against_alone([Spec.case(nm, n, k) for nm, n, k in zip(names, sizes, kinds)], hip_device)


def test_seventeen_equal_jobs(hip_device):
    """Groups of 8, 8 and 1 jobs of n = 40, every one inverse-Cholesky: the second group has
    the shape of the first, whose graph entry is still busy."""
    specs = [Spec.case(nm, 40) for nm in C.NAMES]
    specs.append(Spec(C.problem("spd_1e2", 40)[0], 2.0, 0.3))
    assert len(specs) == 17
    _check_against_alone(specs, hip_device)


def test_nine_jobs_blocked(hip_device):
    """1537 first, then eight small jobs: the second group runs the blocked kernels with a
    small job only (T = 7 of 64: one panel block and its look-ahead split)."""
    sizes = (64, 1, 129, 17, 63, 65, 16, 385)
    names = ("kfac_A_1e-4", "spd_1e5", "kfac_G", "nonsym_grid", "spd_1e5_skew", "block_diag",
             "graded_diag", "kfac_A_bench")
    kinds = (C.CHOL, C.INVERSE, C.CHOL, C.INVERSE, C.CHOL, C.CHOL, C.CHOL, C.INVERSE)
    specs = [_big()] + [Spec.case(nm, n, k) for nm, n, k in zip(names, sizes, kinds)]
    _check_against_alone(specs, hip_device, companion=_big(), skip_check=(0,))


# ------------------------------------------------------------------------ 4. pivot verdicts
def _failing(n, p, kind=C.CHOL):
    return Spec(C.planted(n, p), 1.0, 0.0, kind)


@pytest.mark.parametrize("n,p", C.PLANTED_MERGED)
def test_planted_pivot_merged(hip_device, n, p):
    """info is the 1-based index of the first non-positive pivot of P R P: through the staged
    verdict and inv_copy_out (graph), and straight from check_pivots (plain, either kind)."""
    for graph in (1, 0):
        for kind in (C.CHOL, C.INVERSE):
            _, info, _ = _run_knob([_failing(n, p, kind)], hip_device, GRAPH, graph)
            assert info[0] == p, (n, p, graph, kind, info)


def test_zero_pivots(hip_device):
    """A pivot that is exactly 0, and R = 0."""
    specs = [Spec(C.zero_pivot(n, i0)) for n, i0 in C.ZERO_PIVOTS]
    want = [n - i0 for n, i0 in C.ZERO_PIVOTS]
    specs.append(Spec(np.zeros((50, 50), np.float32), 3.0, 0.0))
    want.append(1)
    for graph in (1, 0):
        _, info, _ = _run_knob(specs, hip_device, GRAPH, graph)
        assert info.tolist() == want, (graph, info)
    _, info, _ = _run([_big()] + specs, hip_device)
    assert info.tolist() == [0] + want, info


def test_planted_pivot_blocked(hip_device):
    """The planted cases as companions of an SPD 1537 job (tile edge 64), both kinds."""
    cases = C.PLANTED_MERGED
    for kind in (C.CHOL, C.INVERSE):
        for part in (cases[:6], cases[6:]):
            _, info, _ = _run([_big()] + [_failing(n, p, kind) for n, p in part], hip_device)
            assert info.tolist() == [0] + [p for _, p in part], (kind, info)


@pytest.mark.parametrize("n,p", C.PLANTED_BLOCKED)
def test_planted_pivot_blocked_largest(hip_device, n, p):
    """The last pivot of the last tile (T = 25) and the very first one."""
    _, info, _ = _run([_failing(n, p), Spec.case("kfac_G", 65)], hip_device)
    assert info.tolist() == [p, 0], info


@pytest.mark.parametrize("graph", [1, 0])
def test_failing_jobs_leave_neighbours_alone(hip_device, graph):
    """Failing jobs at positions 0, 7 (the last of group 0) and 8 (the first of group 1): the
    other jobs report 0 and are bit-equal to the same call with SPD jobs in those places."""
    sizes = (33, 17, 65, 40, 97, 16, 64, 65, 100, 32)
    names = ("kfac_A_1e-4", "spd_1e5", "kfac_G", "nonsym_grid", "spd_1e5_skew", "block_diag",
             "graded_diag", "kfac_A_bench", "spd_1e2", "kfac_A_1e-3")
    good = [Spec.case(nm, n) for nm, n in zip(names, sizes)]
    bad = {0: (33, 32), 7: (65, 64), 8: (100, 49)}
    mixed = [_failing(*bad[i]) if i in bad else s for i, s in enumerate(good)]
    with _knob(GRAPH, graph):
        want, info0, _ = _run(good, hip_device)
        got, info, _ = _run(mixed, hip_device)
    assert not info0.any()
    assert info.tolist() == [bad[i][1] if i in bad else 0 for i in range(10)], info
    for i, s in enumerate(good):
        if i not in bad:
            assert _same(got[i], want[i]), f"job {i} changed beside a failing job"
            s.check(got[i], f" job {i}, graph {graph}")


@pytest.mark.parametrize("path", ["merged_graph", "merged_plain", "blocked"])
def test_no_stale_verdict(hip_device, path):
    """kfac_invert with ONE info buffer: a failing call, then an SPD call of the same shape;
    the second call's verdict is 0 (_native.invert cannot show this: it allocates info per
    call)."""
    from bnn_kfac_amd import _native as N
    first = [_failing(65, 64), _failing(40, 1)]
    second = [Spec.case("kfac_G", 65), Spec.case("spd_1e5", 40)]
    if path == "blocked":
        first, second = [_big()] + first, [_big()] + second
    info = torch.full((len(first),), 77, dtype=torch.int32, device=hip_device)
    seen = []
    with _knob(GRAPH, 0 if path == "merged_plain" else 1):
        for specs in (first, second):
            jobs, keep = _layout(specs, hip_device, 0, 0)
            arr = N.as_array(N.InvertJob, jobs)
            stream = N.stream_handle(hip_device)
            ws = N.workspace.get(hip_device, N.lib().kfac_invert_workspace_bytes(arr, len(jobs)), stream)
            N.check(N.lib().kfac_invert(arr, len(jobs), ws.data_ptr(), ws.numel(), info.data_ptr(), stream),
                    "kfac_invert")
            torch.cuda.synchronize()
            seen.append(info.cpu().tolist())
    lead = [0] if path == "blocked" else []
    assert seen == [lead + [64, 1], lead + [0, 0]], seen


@pytest.mark.parametrize("path", ["merged", "blocked"])
def test_nan_in_F(hip_device, path):
    """One NaN in F (at F[5][9], n = 40) gives info != 0 (check_pivots' `!(piv > 0)` is
    written for it) and leaves the neighbours' bits alone.  The index is not asserted.
    Observed on the MI355X, on either path: info = 35 = n - min(5, 9).  The NaN enters R' at
    (34, 30) and (30, 34) (0-based, flipped); pivot 31 is still clean, the elimination of
    column 30 spreads the NaN over row and column 34, and pivot 35 is the first it reaches."""
    F = C.problem("spd_1e2", 40)[0].copy()
    F[5, 9] = np.nan
    good = [Spec.case("kfac_G", 65), Spec.case("spd_1e2", 40), Spec.case("kfac_A_1e-4", 33)]
    mixed = [good[0], Spec(F, 1.0, 0.01), good[2]]
    if path == "blocked":
        good, mixed = [_big()] + good, [_big()] + mixed
    want, info0, _ = _run(good, hip_device)
    got, info, _ = _run(mixed, hip_device)
    k = len(good) - 2
    print(f"INV-GPU nan {path}: info {info.tolist()}")
    assert not info0.any() and info[k] != 0
    assert [v for i, v in enumerate(info.tolist()) if i != k] == [0] * (len(good) - 1)
    for i in range(len(good)):
        if i != k:
            assert _same(got[i], want[i]), f"job {i} changed beside a NaN job"
