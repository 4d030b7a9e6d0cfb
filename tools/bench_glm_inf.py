"""Time variance.glm_predictive_inf(jacobians="factored") on the wide MLP (784-4096-4096-10,
batch 64, INF rank 100) next to variance.glm_predictive_efb(jacobians="factored") on the same
model, as a yardstick.

The posteriors are synthetic, generated from a seed on the device: orthogonal V_A, V_G per
layer; EFB eigenvalues lambda[g, i] = 1 / ((1 + i)(1 + g)) (a product of two decaying
spectra); the INF state is what INF._dim_reduction keeps of them at `--rank` plus a random
correction with some negative entries.  Damping (add, multiply) = (0.04, 200).
Per call, alternated in one session, HIP-event medians over `--reps` calls after a warm-up:
  inf_ms         : glm_predictive_inf, factors included (kfac_kron_gram, the Cholesky inverse)
  inf_cov_ms     : kron_covariance_outer_inf alone on the three layers' captures
  efb_ms         : glm_predictive_efb
  efb_cov_ms     : kron_covariance_outer_full alone on the same captures
and per layer (ra, rg) and the H / t flop counts 2 nb ra nA nG and 2 nb nc ra nG rg.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import types

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bnn_kfac_amd import _native as N  # noqa: E402
from bnn_kfac_amd.curvatures import INF  # noqa: E402
from bnn_kfac_amd.variance import (glm_predictive_efb, glm_predictive_inf, inf_covariance_factors,  # noqa: E402
                                   kron_covariance_outer_full, kron_covariance_outer_inf, layer_io_jacobians)

ADD, MULTIPLY = 0.04, 200.0


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rank", type=int, default=100)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--width", type=int, default=4096)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    rand = lambda *s: torch.randn(*s, device=dev, generator=gen)  # noqa: E731
    torch.manual_seed(0)
    w = args.width
    net = nn.Sequential(nn.Linear(784, w), nn.ReLU(), nn.Linear(w, w), nn.ReLU(), nn.Linear(w, 10)).to(dev)
    layers = [net[0], net[2], net[4]]
    efb = types.SimpleNamespace(model=net, state={}, eigvecs={}, inv_state={})
    inf = types.SimpleNamespace(model=net, state={})
    shapes = {}
    for layer in layers:
        nA, nG = layer.in_features + 1, layer.out_features
        VA, VG = torch.linalg.qr(rand(nA, nA))[0].contiguous(), torch.linalg.qr(rand(nG, nG))[0].contiguous()
        lam = 1.0 / ((1.0 + torch.arange(nG, device=dev))[:, None] * (1.0 + torch.arange(nA, device=dev))[None, :])
        efb.state[layer], efb.eigvecs[layer] = lam, (VA, VG)
        efb.inv_state[layer] = torch.reciprocal(MULTIPLY * lam + ADD).sqrt()
        UA, UG, lr = INF._dim_reduction(VA, VG, lam.t().contiguous().view(-1), args.rank)
        corr = 0.1 * torch.rand(nA * nG, device=dev, generator=gen) - 0.01
        inf.state[layer] = (UA.contiguous(), UG.contiguous(), lr.contiguous(), corr)
        ra, rg = UA.shape[1], UG.shape[1]
        shapes[f"{nA}x{nG}"] = {"ra": ra, "rg": rg, "h_flop": 2 * args.batch * ra * nA * nG,
                                "t_flop": 2 * args.batch * 10 * ra * nG * rg}
    x = torch.rand(args.batch, 784, device=dev, generator=gen)
    _, io = layer_io_jacobians(net, layers, x)
    factors = inf_covariance_factors(inf, ADD, MULTIPLY, layers)
    inf_terms = [(a, D, *factors[layer]) for layer, (a, D) in zip(layers, io)]
    efb_terms = [(a, D, *efb.eigvecs[layer], (efb.inv_state[layer].t() ** 2).contiguous().unsqueeze(0))
                 for layer, (a, D) in zip(layers, io)]
    fns = [lambda: glm_predictive_inf(inf, x, ADD, MULTIPLY, layers=layers, chunk=args.batch, jacobians="factored"),
           lambda: kron_covariance_outer_inf(inf_terms),
           lambda: glm_predictive_efb(efb, x, layers=layers, chunk=args.batch, jacobians="factored"),
           lambda: kron_covariance_outer_full(efb_terms)]
    ms = alternate_ms(fns, args.warmup, args.reps)
    cov = fns[0]()[1]
    out = {"workload": "GLM predictive under the INF posterior, factored route", "lib": N.LIB_PATH,
           "model": f"784-{w}-{w}-10", "batch": args.batch, "rank": args.rank, "layers": shapes,
           "inf_ms": ms[0], "inf_cov_ms": ms[1], "efb_ms": ms[2], "efb_cov_ms": ms[3],
           "cov_finite": bool(torch.isfinite(cov).all()), "cov_diag_min": float(torch.diagonal(cov, dim1=1, dim2=2).min())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
