"""Time the Monte-Carlo GLM predictive under the INF posterior.

Columns, alternated call by call in one process on the same inputs (HIP events around every
call, `--warmup` warm rounds first, the median of `--reps` with min - max):
  inf_mc    : variance.glm_predictive_mc(inf, x, n_draws=S, jacobians="factored")
  inf_call  : kron_draws_outer_inf alone on all layers' captures (projections, q, the draw tile
              kernel, the second term and the reduce)
  efb_mc    : glm_predictive_mc under an EFB on the same model, as the yardstick
  torch_loop: S x (inf_posterior_sample per layer + forward + softmax statistics in torch), the
              way the same statistics are obtained without the draw calls
and, from the shapes, the work of the widest layer's draw tile kernel (Z and C bytes =
S * nA * nG * 8 per 64-sample tile, flops = 2 S N nA nG) and of its F g projection
(2 S ra nA nG flops) for the rates and shares DESIGN.md quotes.

The posteriors are tools/bench_glm_inf.py's synthetic ones at `--rank`.  Configurations: mlp
(784-128-10, N = 256, S = 100) and wide (784-4096-4096-10, N = 64, S = 8).  Prints one JSON line
per configuration.  --quick: a few calls of inf_mc only (for a kernel trace)."""
import argparse
import json
import os
import statistics
import sys
import types

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bnn_kfac_amd.curvatures import INF  # noqa: E402
from bnn_kfac_amd.variance import (glm_predictive_mc, inf_draw_factors, inf_posterior_sample,  # noqa: E402
                                   kron_draws_outer_inf, layer_io_jacobians)

ADD, MULTIPLY = 0.04, 200.0
CONFIGS = {"mlp": ((784, 128, 10), 256, 100), "wide": ((784, 4096, 4096, 10), 64, 8)}


def alternate_ms(fns, warmup, reps):
    """(median, min, max) of the HIP-event times of each of `fns`, called in turn `reps` times."""
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
    return [(statistics.median(t), min(t), max(t)) for t in times]


def build(widths, rank, dev, gen):
    rand = lambda *s: torch.randn(*s, device=dev, generator=gen)  # noqa: E731
    torch.manual_seed(0)
    mods = []
    for i, (d_in, d_out) in enumerate(zip(widths[:-1], widths[1:])):
        mods.append(nn.Linear(d_in, d_out))
        if i + 2 < len(widths):
            mods.append(nn.ReLU())
    net = nn.Sequential(*mods).to(dev)
    layers = [m for m in net if isinstance(m, nn.Linear)]
    efb = types.SimpleNamespace(model=net, state={}, eigvecs={}, inv_state={})
    inf = INF.__new__(INF)
    inf.model, inf._state, inf._inv_state = net, {}, {}
    for layer in layers:
        nA, nG = layer.in_features + 1, layer.out_features
        VA, VG = torch.linalg.qr(rand(nA, nA))[0].contiguous(), torch.linalg.qr(rand(nG, nG))[0].contiguous()
        lam = 1.0 / ((1.0 + torch.arange(nG, device=dev))[:, None] * (1.0 + torch.arange(nA, device=dev))[None, :])
        efb.state[layer], efb.eigvecs[layer] = lam, (VA, VG)
        efb.inv_state[layer] = torch.reciprocal(MULTIPLY * lam + ADD).sqrt()
        UA, UG, lr = INF._dim_reduction(VA, VG, lam.t().contiguous().view(-1), rank)
        corr = 0.1 * torch.rand(nA * nG, device=dev, generator=gen) - 0.01
        inf._state[layer] = (UA.contiguous(), UG.contiguous(), lr.contiguous(), corr)
    return net, layers, inf, efb


def torch_loop(net, layers, factors, x, draws, gen):
    psum, hsum = 0.0, 0.0
    saved = [(layer.weight.detach().clone(), layer.bias.detach().clone()) for layer in layers]
    with torch.no_grad():
        for _ in range(draws):
            for layer, (w, b) in zip(layers, saved):
                UA, UG = factors[layer][:2]
                z = torch.randn(1, UA.shape[0], UG.shape[0], device=x.device, generator=gen)
                e = torch.randn(1, UA.shape[1] * UG.shape[1], device=x.device, generator=gen)
                s = inf_posterior_sample(*factors[layer], z, e)[0]
                layer.weight.copy_(w + s[:-1].t())
                layer.bias.copy_(b + s[-1])
            logp = torch.log_softmax(net(x).double(), dim=1)
            p = logp.exp()
            psum = psum + p
            hsum = hsum - (p * logp).sum(dim=1)
        for layer, (w, b) in zip(layers, saved):
            layer.weight.copy_(w)
            layer.bias.copy_(b)
    return psum / draws, hsum / draws


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=list(CONFIGS) + ["all"], default="all")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rank", type=int, default=100)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in (list(CONFIGS) if args.config == "all" else [args.config]):
        widths, n, draws = CONFIGS[name]
        gen = torch.Generator(device=dev).manual_seed(0)
        net, layers, inf, efb = build(widths, args.rank, dev, gen)
        x = torch.rand(n, widths[0], device=dev, generator=gen)
        kw = dict(n_draws=draws, layers=layers, chunk=n, jacobians="factored", generator=gen)
        inf_mc = lambda: glm_predictive_mc(inf, x, add=ADD, multiply=MULTIPLY, **kw)  # noqa: E731
        if args.quick:
            for _ in range(3):
                inf_mc()
            torch.cuda.synchronize()
            continue
        _, io = layer_io_jacobians(net, layers, x)
        factors = inf_draw_factors(inf, ADD, MULTIPLY, layers)
        terms = [(a, D, *factors[layer]) for layer, (a, D) in zip(layers, io)]
        z = [torch.randn(draws, f[0].shape[0], f[1].shape[0], device=dev, generator=gen) for f in factors.values()]
        e = [torch.randn(draws, f[0].shape[1] * f[1].shape[1], device=dev, generator=gen) for f in factors.values()]
        fns = [inf_mc,
               lambda: kron_draws_outer_inf(terms, z, e),
               lambda: glm_predictive_mc(efb, x, **kw),
               lambda: torch_loop(net, layers, factors, x, draws, gen)]
        ms = alternate_ms(fns, args.warmup, args.reps)
        res = inf_mc()
        wide = max(factors.values(), key=lambda f: f[2].numel())
        nA, nG, ra, rg = wide[0].shape[0], wide[1].shape[0], wide[0].shape[1], wide[1].shape[1]
        col = lambda t: {"ms": t[0], "ms_min_max": t[1:]}  # noqa: E731
        print(json.dumps({
            "config": name, "widths": widths, "N": n, "draws": draws, "rank": args.rank, "reps": args.reps,
            "inf_mc": col(ms[0]), "inf_call": col(ms[1]), "efb_mc": col(ms[2]), "torch_loop": col(ms[3]),
            "inf_mc_over_efb_mc": ms[0][0] / ms[2][0], "torch_loop_over_inf_mc": ms[3][0] / ms[0][0],
            "widest_layer": {"nA": nA, "nG": nG, "ra": ra, "rg": rg,
                             "tile_zc_bytes": 8.0 * draws * nA * nG * -(-n // 64),
                             "tile_flop": 2.0 * draws * n * nA * nG,
                             "fg_proj_flop": 2.0 * draws * ra * nA * nG},
            "probs_finite": bool(torch.isfinite(res.probs).all()),
            "mi_max": float(res.mutual_information.max())}))


if __name__ == "__main__":
    main()
