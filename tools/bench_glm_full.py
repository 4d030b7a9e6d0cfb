"""Time the per-entry-weight GLM covariance calls (variance.kron_covariance_full /
kron_covariance_outer_full) on synthetic inputs generated from a seed on the device
(orthogonal V_A, V_G; W = 10^U(-3, 3) per entry), nb = 64, nc = 10:
  785 x 128   : nt in {1, 8}, both routes (the dense route's rows are outer([a | 1], delta))
  4097 x 4096 : nt in {1, 8}, outer route only (one dense row of it is 67 MB)
Per case and route, alternated call by call in one session:
  full_ms   : the new call
  torch_ms  : the same formula from torch ops on the same GPU -- dense: Y = V_A^T M V_G, then
              einsum("tig,bcig,bdig->tbcd", W, Y, Y); outer: R = ((abar V_A)^2) @ W,
              Q = Delta V_G, einsum("bcg,tbg,bdg->tbcd", Q, R, Q)
  sweep_ms  : kron_covariance_sweep / kron_covariance_outer_sweep at the same shape with nt
              rank-one weightings, for scale (the calls the new ones generalise)
  max_diff_vs_torch_over_max : the new call against the torch evaluation, worst grid point
  full_err_vs_fp64_over_max / torch_err_vs_fp64_over_max : each against the torch evaluation
              in fp64 on the same fp32 inputs (computed once, outside the timings)
GPU times are HIP-event times of single calls after a warm-up, medians over `--reps` calls.
`--only full` runs the new calls alone (kernel traces).  Prints one JSON line per case, then
the whole."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bnn_kfac_amd import _native as N  # noqa: E402
from bnn_kfac_amd.variance import (kron_covariance_full, kron_covariance_outer_full,  # noqa: E402
                                   kron_covariance_outer_sweep, kron_covariance_sweep)

NB, NC = 64, 10
CASES = [(785, 128, ("dense", "outer")), (4097, 4096, ("outer",))]
NTS = (1, 8)


def alternate_ms(fns, warmup, reps):
    """Medians of HIP-event times of each of `fns`, called in turn `reps` times."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for fn, t in zip(fns, times):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            t.append(a.elapsed_time(b))
    return [statistics.median(t) for t in times]


def torch_dense(J, VA, VG, W):
    nb, nc = J.shape[:2]
    Y = VA.T @ J.view(nb, nc, VA.shape[0], VG.shape[0]) @ VG
    return torch.einsum("tig,bcig,bdig->tbcd", W, Y, Y)


def torch_outer(a, D, VA, VG, W):
    abar = torch.cat([a, a.new_ones(a.shape[0], 1)], dim=1)
    R = ((abar @ VA) ** 2) @ W                       # (nt, nb, nG)
    Q = D @ VG
    return torch.einsum("bcg,tbg,bdg->tbcd", Q, R, Q)


def worst(got, want):
    return float(((got - want).abs().amax(dim=(1, 2, 3)) / want.abs().amax(dim=(1, 2, 3))).max())


def run_case(nA, nG, routes, dev, args):
    gen = torch.Generator(device=dev).manual_seed(1000 * nA + nG)
    rand = lambda *s: torch.randn(*s, device=dev, generator=gen)  # noqa: E731
    a, D = rand(NB, nA - 1), rand(NB, NC, nG)
    VA, VG = torch.linalg.qr(rand(nA, nA))[0].contiguous(), torch.linalg.qr(rand(nG, nG))[0].contiguous()
    res = {"nA": nA, "nG": nG, "nb": NB, "nc": NC}
    for nt in NTS:
        W = 10.0 ** (6.0 * torch.rand(nt, nA, nG, device=dev, generator=gen) - 3.0)
        wA = 10.0 ** (6.0 * torch.rand(nt, nA, device=dev, generator=gen) - 3.0)
        wG = 10.0 ** (6.0 * torch.rand(nt, nG, device=dev, generator=gen) - 3.0)
        for route in routes:
            if route == "dense":
                abar = torch.cat([a, a.new_ones(NB, 1)], dim=1)
                J = torch.einsum("bi,bcg->bcig", abar, D).reshape(NB, NC, nA * nG).contiguous()
                full = lambda: kron_covariance_full([(J, VA, VG, W)])  # noqa: E731
                composed = lambda: torch_dense(J, VA, VG, W)  # noqa: E731
                sweep = lambda: kron_covariance_sweep([(J, VA, VG, wA, wG)])  # noqa: E731
                exact = lambda: torch_dense(J.double(), VA.double(), VG.double(), W.double())  # noqa: E731
            else:
                exact = lambda: torch_outer(a.double(), D.double(), VA.double(), VG.double(), W.double())  # noqa: E731
                full = lambda: kron_covariance_outer_full([(a, D, VA, VG, W)])  # noqa: E731
                composed = lambda: torch_outer(a, D, VA, VG, W)  # noqa: E731
                sweep = lambda: kron_covariance_outer_sweep([(a, D, VA, VG, wA, wG)])  # noqa: E731
            r = {}
            if args.only == "full":
                r["full_ms"], = alternate_ms([full], args.warmup, args.reps)
            else:
                r["full_ms"], r["torch_ms"], r["sweep_ms"] = alternate_ms([full, composed, sweep], args.warmup,
                                                                          args.reps)
                r["max_diff_vs_torch_over_max"] = worst(full(), composed())
                ref = exact()
                r["full_err_vs_fp64_over_max"] = worst(full().double(), ref)
                r["torch_err_vs_fp64_over_max"] = worst(composed().double(), ref)
                del ref
            res[f"{route}_nt{nt}"] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["all", "full"], default="all")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"workload": "GLM covariance with per-entry eigenbasis weights", "lib": N.LIB_PATH}
    for nA, nG, routes in CASES:
        out[f"{nA}x{nG}"] = run_case(nA, nG, routes, dev, args)
        print(json.dumps({f"{nA}x{nG}": out[f"{nA}x{nG}"]}), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
