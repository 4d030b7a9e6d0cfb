"""CPU: the conv factor cases of tests/conv_factor_cases.py (no GPU calls).

What test_gpu_conv_factor_exact.py relies on is proved here from the data, the router and the
planner: the sweep's size and its floors per family, that every sum is an exact fp32 integer, that
the int64 reference agrees with the oracle, that the numpy model of the kernels reproduces the
reference, and that every planted mistake of the model changes the result on every case its
predicate names -- so a kernel making that mistake fails the GPU test on those cases."""
import numpy as np
import pytest

import conv_factor_cases as C
from oracle import kfac_oracle as O


def _N():
    from bnn_kfac_amd import _native as N
    return N


def test_family_ids_match_the_header():
    N = _N()
    assert C.FAMILY == {N.PROF_FACTOR_TILES: "tiles", N.PROF_FACTOR_CONV: "conv",
                        N.PROF_FACTOR_CHANNEL_SMALL: "channel_small", N.PROF_FACTOR_CONV_X3: "conv_x3",
                        N.PROF_FACTOR_CONV_X3S: "conv_x3s", N.PROF_FACTOR_CONV_X3F: "conv_x3f",
                        N.PROF_FACTOR_CHANNEL_X3: "channel_x3"}


def test_route_argument_checks():
    N = _N()
    case = C.fixed()["multi"][0]
    j, keep = C.host_job(N, case)
    fam = (N.c_i32 * 1)()
    arr = N.as_array(N.FactorJob, [j])
    assert N.lib().kfac_factor_route(arr, 1, fam) == N.KFAC_OK and C.FAMILY[fam[0]] == case.family
    assert N.lib().kfac_factor_route(arr, 1, None) == N.KFAC_EINVAL
    assert N.lib().kfac_factor_route(None, 1, fam) == N.KFAC_EINVAL
    assert N.lib().kfac_factor_route(None, 0, None) == N.KFAC_OK
    # a shorter last batch is a row-major notion: a conv job that sets it is refused
    j.x.last_rows = int(j.x.rows) - case.L
    arr = N.as_array(N.FactorJob, [j])
    assert N.lib().kfac_factor_route(arr, 1, fam) == N.KFAC_EINVAL
    splits, nbytes = (N.c_i32 * 1)(), (N.ctypes.c_size_t * 1)()
    assert N.lib().kfac_factor_accum_plan(arr, 1, splits, nbytes) == N.KFAC_EINVAL


def test_route_follows_the_launch_groups():
    """Row-major jobs share a group (one family for all), conv jobs route alone, and the answer
    comes back in the caller's order."""
    N = _N()
    conv = C.fixed()["large"][0]
    rm = []
    for cols in (784, 10):
        j = N.FactorJob()
        j.x = N.Operand(C.BASE, N.ROWMAJOR, cols, 4096, 0, 0, cols)
        j.alpha, j.F, j.ldF = 1.0, C.BASE, cols
        rm.append(j)
    jobs = [rm[0], C.host_job(N, conv)[0], rm[1]]
    assert N.factor_route(jobs) == [N.PROF_FACTOR_X3, N.PROF_FACTOR_CONV_X3S, N.PROF_FACTOR_X3]
    assert N.factor_route([rm[1]]) == [N.PROF_FACTOR_TILES]


def test_patch_sweep_counts_and_floors():
    kept, routed, classes = C.patch_sweep()
    ncand = sum(routed.values())
    per = {f: [c for c in kept if c.family == f] for f in C.PATCH_FAMILIES}
    print("candidates", ncand, "routed", routed, "kept", {f: len(v) for f, v in per.items()},
          "input floats", sum(3 * c.sB + 2 * C.GUARD for c in kept), "classes", classes)
    assert ncand == 53928
    assert set(routed) == set(C.PATCH_FAMILIES)
    assert len({c.id for c in kept}) == len(kept)
    for f, cases in per.items():
        assert len(cases) >= C.FLOORS[f], (f, len(cases))
        if f == "conv_x3f":
            # x3f_search takes stride 1 x 1 only, so the grid cannot hold an unequal stride for
            # it; the day its geometry takes another stride this line asks for the case
            assert all((c.sh, c.sw) == (1, 1) for c in cases)
        else:
            assert any(c.sh != c.sw for c in cases), f"{f}: no unequal stride"
        assert any(c.ph != c.pw for c in cases), f"{f}: no unequal padding"
        assert any(c.kh != c.kw for c in cases), f"{f}: no kh != kw"
        assert any(not c.ones for c in cases), f"{f}: no case without bias"
        assert all(c.img <= 20 * 32 * 32 and c.B == 3 for c in cases)
    # every family-specific class a candidate of the grid has is kept, and the ones the kernels'
    # geometries distinguish are there
    cls = {f: {C.family_class(c) for c in per[f]} for f in per}
    assert cls == classes
    assert cls["conv_x3s"] >= {(1, False), (1, True), (2, False), (2, True), (4, True)}  # (g8, kw odd)
    assert cls["conv_x3f"] >= {(nb, nv) for nb in (4, 5) for nv in (1, 2)}
    assert cls["conv_x3"] >= {(1, False), (1, True), (2, False), (2, True), (3, False)}  # (ceil(nq / 8), L > 256)
    assert cls["conv"] >= {(m, big) for m in (0, 1, 2) for big in (False, True)}
    assert cls["tiles"] == {1, 2, 3}
    assert all(c.key == C.sweep_key(c) for c in kept)


def test_channel_sweep_covers_every_instance():
    cases = C.channel_sweep()
    assert len({c.id for c in cases}) == len(cases)
    staged = [c for c in cases if c.family != "tiles"]
    for fam, ns in C.CH_N.items():
        for B in (3, 5):
            got = {(c.cols, c.L) for c in staged if c.family == fam and c.B == B}
            assert {n for n, _ in got} == set(ns), (fam, B)
            # every last k-step (4, 12 and 16 positions) at every n
            for n in ns:
                assert {L % 16 for nn, L in got if nn == n} >= {4, 12, 0}, (fam, n)
    for c in staged:
        assert c.sB == c.img + 4 and c.guard % 4 == 0 and not c.ones
    # the fallbacks: each routed to kfac_factor_tiles, for every reason, and -- but where
    # sB = n L + 4 isolates another reason -- at sB = n L + 3
    fb = [c for c in cases if c.family == "tiles"]
    assert fb == [c for c in cases if hasattr(c, "fallback")]
    assert {c.fallback for c in fb} == {"L%4", "sB%4", "base+1", "ones", "large"}
    for c in fb:
        assert c.sB == c.img + (4 if "sB+4" in c.id else 3), c.id
        assert {"L%4": c.L % 4 != 0, "sB%4": c.sB % 4 != 0, "base+1": c.guard % 4 == 1, "ones": c.ones,
                "large": c.img > 4 * 2048}[c.fallback], c.id
    for why in ("base+1", "ones", "large"):
        assert {"sB+4" in c.id for c in fb if c.fallback == why} == {False, True}


def test_fixed_cases_route_and_split_as_planned():
    f = C.fixed()
    for mode in ("large", "multi", "deferred"):
        for c in f[mode]:
            assert c.family == c.want_family, (c.id, c.family)
            if c.family == "tiles":
                continue
            # tasks own 2 or 3 images, not all the same number -- but for (1030, 16, 12), whose
            # 515 splits take two images each (chx3_n16_odd is that family's uneven case)
            assert c.splits < c.B, (c.id, c.B, c.splits)
            if mode != "multi":  # (a multi-batch case: a task across the batch boundary, below)
                assert (c.B % c.splits != 0) == ("chx3_n16]" not in c.id), (c.id, c.B, c.splits)
    assert [c.splits for c in f["large"]] == [130, 130, 130, 515, 130, 258, 344, 515, 515, 515]
    multi = {c.id: c for c in f["multi"]}
    for name, splits in (("x3s", 131), ("x3f_n101", 131), ("x3", 131), ("fp32_n224", 131), ("fp32_n10", 515)):
        c = multi[f"multi[{name}]"]
        assert c.splits == splits and C.launches(c) == 1
        assert C.MISTAKES["stops_at_batch"](c)
    for c in f["multi"]:
        assert len(c.batches) == 3 and c.batches[0] % 2 == 1
        assert len({p % 16 for p in C.fake_ptrs(c)}) == 1
        assert c.family == "tiles" or C.MISTAKES["stops_at_batch"](c), c.id
    assert C.launches(multi["multi[tiles]"]) == 3
    for c in f["deferred"]:
        assert c.steps == (c.B, 7, c.B - 1) and c.splits > 7 and c.beta == 1.0 and C.launches(c) == 3


def _cases(which):
    return {"patch": lambda: C.patch_sweep()[0], "channel": C.channel_sweep,
            "fixed": lambda: sum(C.fixed().values(), [])}[which]()


GROUPS = ("patch", "channel", "fixed")


@pytest.mark.parametrize("which", GROUPS)
def test_data_is_exact_and_reference_matches_oracle(which):
    for c in _cases(which):
        bufs = C.inputs(c)
        for s, buf in enumerate(bufs):
            x = C.images(c, s)
            assert np.isfinite(x).all() and np.array_equal(x, np.rint(x)) and np.abs(x).max() <= 3
            live = np.zeros(buf.size, dtype=bool)
            live[c.guard + np.arange(c.batches[s])[:, None] * c.sB + np.arange(c.img)[None, :]] = True
            assert np.isnan(buf[~live]).all() and not live[:C.GUARD].any() and not live[-C.GUARD:].any()
        K = C.krows(c)
        assert 9 * K < 2 ** 24, (c.id, K)
        S = C.reference(c)
        assert np.array_equal(S, S.T) and np.abs(S).max() <= 9 * K
        want = C.expected(c)
        region = np.zeros(want.size, dtype=bool)
        region[C.F_OFF + np.arange(c.n)[:, None] * c.ldF + np.arange(c.n)[None, :]] = True
        assert np.isfinite(want[region]).all() and np.isnan(want[~region]).all()
        assert np.array_equal(want[region].astype(np.float32).astype(np.float64), want[region])
        assert c.alpha in (1.0, 0.5) and c.beta in (0.0, 1.0) and c.ldF == c.n + 3
        # the oracle, in fp64: per update, its per-batch mean times the update's rows
        T = np.zeros((c.n, c.n))
        for m, nb, _ in C.updates(c):
            for s in range(nb):
                x = C.images(c, s)[:m].astype(np.float64)
                if c.layout == "patch":
                    A = O.conv_factor_A(x, (c.kh, c.kw), (c.ph, c.pw), (c.sh, c.sw), c.ones, dtype=np.float64)
                else:
                    A = O.grad_factor(x.reshape(m, c.cols, c.L, 1), dtype=np.float64)
                    if c.ones:  # (the oracle's G has no ones column: border it)
                        col = x.sum(axis=(0, 2)) / (m * c.L)
                        A = np.block([[A, col[:, None]], [col[None, :], np.ones((1, 1))]])
                T += A * (m * c.L)
        assert np.array_equal(np.rint(T).astype(np.int64), S) and np.abs(T - S).max() < 1e-6, c.id


@pytest.mark.parametrize("which", GROUPS)
def test_model_matches_reference_and_mistakes_show(which):
    cases = _cases(which)
    shown = {m: set() for m in C.MISTAKES}
    for c in cases:
        want = C.expected(c)
        assert np.array_equal(C.model_factor(c), want, equal_nan=True), c.id
        for m, named in C.MISTAKES.items():
            if named(c):
                assert not np.array_equal(C.model_factor(c, m), want, equal_nan=True), (c.id, m)
                shown[m].add((c.layout, c.family))
    print({m: sorted(v) for m, v in shown.items()})
    patch = {("patch", f) for f in C.PATCH_FAMILIES}
    channel = {("channel", f) for f in ("channel_small", "channel_x3", "conv", "tiles")}
    big = {("patch", "conv_x3s"), ("patch", "conv_x3f"), ("patch", "conv_x3"), ("patch", "conv"),
           ("channel", "channel_small"), ("channel", "channel_x3"), ("channel", "conv")}
    every = ("sB_contiguous", "beta_ignored", "alpha_twice", "ldF_as_n")
    need = {
        # (kfac_factor_conv_x3f takes stride 1 x 1 only)
        "patch": dict({m: patch for m in every + ("record_sB", "pad_swapped", "kernel_swapped", "last_row_dropped",
                                                  "last_col_dropped", "ones_per_image")},
                      stride_swapped=patch - {("patch", "conv_x3f")}),
        "channel": dict({m: channel for m in every}, ones_per_image={("channel", "tiles")}),
        "fixed": dict({m: big for m in every + ("uneven_last_dropped", "empty_task_zeroes", "stops_at_batch")},
                      batch_base0=big | {("patch", "tiles")}),
    }[which]
    for m, fams in need.items():
        assert shown[m] >= fams, (m, sorted(fams - shown[m]))
