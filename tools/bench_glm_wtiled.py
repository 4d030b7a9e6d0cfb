"""Time the class-tiled weighted GLM covariance calls (variance.kron_covariance_full_tiled,
kron_covariance_outer_full_tiled, kron_covariance_sweep_tiled, kron_covariance_outer_sweep_tiled)
on a 256 -> 100 head (nA = 257 with the bias, nG = 100, nc = 100), nb = 64, nt in {1, 6}, on
synthetic inputs generated from a seed on the device (orthogonal V_A, V_G; weights
10^U(-3, 3)), both routes (the dense route's rows are outer([a | 1], delta)).
Per route, alternated call by call in one session:
  full_nt{1,6}_ms / sweep_nt{1,6}_ms : the new calls
  yardstick_ms  : the unweighted class-tiled call on the same shapes (kron_covariance_tiled /
                  kron_covariance_outer_tiled with K1 = V_A, K2 = V_G dense): the same
                  projections, ONE Gram per tile pair
  *_per_point_ms: (nt = 6 minus nt = 1) / 5, what one more grid point costs (its Gram tasks,
                  which stage their panels again, and its reduce); above the yardstick's whole
                  time it would mean re-staging costs more than a full unweighted call
  *_err_vs_fp64_over_max : the new call against the same formula from torch ops in fp64 on the
                  same fp32 inputs, worst grid point (computed once, outside the timings)
GPU times are HIP-event times of single calls after a warm-up, medians over `--reps` calls.
There is no pass mark.  Prints one JSON line per route, then the whole."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_glm_full import alternate_ms, torch_dense, torch_outer, worst  # noqa: E402
from bnn_kfac_amd import _native as N  # noqa: E402
from bnn_kfac_amd.variance import (kron_covariance_full_tiled, kron_covariance_outer_full_tiled,  # noqa: E402
                                   kron_covariance_outer_sweep_tiled, kron_covariance_outer_tiled,
                                   kron_covariance_sweep_tiled, kron_covariance_tiled)

NB, NC, NA, NG = 64, 100, 257, 100
NTS = (1, 6)


def run_route(route, dev, args):
    gen = torch.Generator(device=dev).manual_seed(1000 * NA + NG)
    rand = lambda *s: torch.randn(*s, device=dev, generator=gen)  # noqa: E731
    a, D = rand(NB, NA - 1), rand(NB, NC, NG)
    VA, VG = torch.linalg.qr(rand(NA, NA))[0].contiguous(), torch.linalg.qr(rand(NG, NG))[0].contiguous()
    W = 10.0 ** (6.0 * torch.rand(NTS[-1], NA, NG, device=dev, generator=gen) - 3.0)
    wA = 10.0 ** (6.0 * torch.rand(NTS[-1], NA, device=dev, generator=gen) - 3.0)
    wG = 10.0 ** (6.0 * torch.rand(NTS[-1], NG, device=dev, generator=gen) - 3.0)
    if route == "dense":
        abar = torch.cat([a, a.new_ones(NB, 1)], dim=1)
        J = torch.einsum("bi,bcg->bcig", abar, D).reshape(NB, NC, NA * NG).contiguous()
        full = lambda nt: kron_covariance_full_tiled([(J, VA, VG, W[:nt])])  # noqa: E731
        sweep = lambda nt: kron_covariance_sweep_tiled([(J, VA, VG, wA[:nt], wG[:nt])])  # noqa: E731
        yard = lambda: kron_covariance_tiled([(J, VA, VG)], lower=False)  # noqa: E731
        # fp64 in chunks of samples: one chunk's Y is nb x nc x nA x nG doubles
        exact = lambda Wt: torch.cat([torch_dense(J[b:b + 8].double(), VA.double(), VG.double(), Wt.double())  # noqa: E731
                                      for b in range(0, NB, 8)], dim=1)
    else:
        full = lambda nt: kron_covariance_outer_full_tiled([(a, D, VA, VG, W[:nt])])  # noqa: E731
        sweep = lambda nt: kron_covariance_outer_sweep_tiled([(a, D, VA, VG, wA[:nt], wG[:nt])])  # noqa: E731
        yard = lambda: kron_covariance_outer_tiled([(a, D, VA, VG)], lower=False)  # noqa: E731
        exact = lambda Wt: torch_outer(a.double(), D.double(), VA.double(), VG.double(), Wt.double())  # noqa: E731
    fns = [lambda: full(1), lambda: full(6), lambda: sweep(1), lambda: sweep(6), yard]
    names = ["full_nt1_ms", "full_nt6_ms", "sweep_nt1_ms", "sweep_nt6_ms", "yardstick_ms"]
    r = dict(zip(names, alternate_ms(fns, args.warmup, args.reps)))
    r["full_per_point_ms"] = (r["full_nt6_ms"] - r["full_nt1_ms"]) / 5
    r["sweep_per_point_ms"] = (r["sweep_nt6_ms"] - r["sweep_nt1_ms"]) / 5
    r["full_err_vs_fp64_over_max"] = worst(full(6).double(), exact(W))
    r["sweep_err_vs_fp64_over_max"] = worst(sweep(6).double(), exact(wA[:, :, None] * wG[:, None, :]))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--routes", default="outer,dense")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"workload": "class-tiled weighted GLM covariance, 256 -> 100 head", "lib": N.LIB_PATH,
           "nA": NA, "nG": NG, "nb": NB, "nc": NC}
    for route in args.routes.split(","):
        out[route] = run_route(route, dev, args)
        print(json.dumps({route: out[route]}), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
