"""Time the Monte-Carlo GLM predictive against the sampling loop it replaces.

  glm_mc   : variance.glm_predictive_mc(kfac, x, n_draws=S, jacobians="factored")
  sampling : S x (kfac.sample_and_replace() + forward + softmax statistics in torch),
             the way the same statistics are obtained without it
both in one process on the same inputs, and the largest Linear layer's kron_draws_outer call
on its own (U, V, the draw kernel and the reduce), with the work that call needs computed
from the shapes: Z bytes = S * nA * nG * 4 per 64-sample tile, flops = 2 S N nA nG.

Configurations: mlp (784-128-10, N = 256, S = 100) and wide (784-4096-4096-10, N = 64, S = 8).
HIP events around every run, warm runs first, the median of --runs (>= 20) runs.  Prints one
JSON line per configuration.  --quick: a few runs of glm_mc only (for a kernel trace).
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bnn_kfac_amd.curvatures import KFAC  # noqa: E402
from bnn_kfac_amd.variance import glm_predictive_mc, kron_draws_outer, layer_io_jacobians  # noqa: E402

CONFIGS = {"mlp": ((784, 128, 10), 256, 100), "wide": ((784, 4096, 4096, 10), 64, 8)}


def build(widths, dev):
    torch.manual_seed(0)
    mods = []
    for i, (d_in, d_out) in enumerate(zip(widths[:-1], widths[1:])):
        mods.append(nn.Linear(d_in, d_out))
        if i + 2 < len(widths):
            mods.append(nn.ReLU())
    net = nn.Sequential(*mods).to(dev)
    kfac = KFAC(net)
    g = torch.Generator(device=dev).manual_seed(0)
    for _ in range(4):
        x = torch.randn(512, widths[0], device=dev, generator=g)
        logits = net(x)
        y = torch.distributions.Categorical(logits=logits.detach()).sample()
        net.zero_grad()
        nn.functional.cross_entropy(logits, y).backward()
        kfac.update(batch_size=x.shape[0])
    kfac.invert(0.04, 200.0)
    return net, kfac, g


def timed(fn, warm, runs):
    """Median and spread (ms) of `runs` event-timed calls after `warm` untimed ones."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end))
    return statistics.median(times), min(times), max(times)


def sampling_loop(kfac, net, x, draws):
    psum, hsum = 0.0, 0.0
    with torch.no_grad():
        for _ in range(draws):
            kfac.sample_and_replace()
            logp = torch.log_softmax(net(x).double(), dim=1)
            p = logp.exp()
            psum = psum + p
            hsum = hsum - (p * logp).sum(dim=1)
    net.load_state_dict(kfac.model_state)
    return psum / draws, hsum / draws


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=list(CONFIGS) + ["all"], default="all")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in (list(CONFIGS) if args.config == "all" else [args.config]):
        widths, n, draws = CONFIGS[name]
        net, kfac, g = build(widths, dev)
        x = torch.randn(n, widths[0], device=dev, generator=g)
        mc = lambda: glm_predictive_mc(kfac, x, n_draws=draws, jacobians="factored", generator=g)  # noqa: E731
        if args.quick:
            for _ in range(3):
                mc()
            torch.cuda.synchronize()
            continue
        t_mc = timed(mc, args.warmup, args.runs)
        t_loop = timed(lambda: sampling_loop(kfac, net, x, draws), args.warmup, args.runs)
        # the largest Linear layer's draw call alone
        layers = [m for m in net if isinstance(m, nn.Linear)]
        _, io = layer_io_jacobians(net, layers, x)
        layer, (a, D) = max(zip(layers, io), key=lambda t: t[0].weight.numel())
        K1, K2 = kfac.inv_state[layer]
        nA, nG = K1.shape[0], K2.shape[0]
        z = torch.randn(draws, nA, nG, device=dev, generator=g)
        t_call = timed(lambda: kron_draws_outer([(a, D, K1, K2)], [z]), args.warmup, args.runs)
        z_bytes = 4.0 * draws * nA * nG * -(-n // 64)
        flops = 2.0 * draws * n * nA * nG
        print(json.dumps({
            "config": name, "widths": widths, "N": n, "draws": draws, "runs": args.runs,
            "glm_mc_ms": t_mc[0], "glm_mc_ms_min_max": t_mc[1:],
            "sampling_loop_ms": t_loop[0], "sampling_loop_ms_min_max": t_loop[1:],
            "speedup": t_loop[0] / t_mc[0],
            "outer_call": {"layer": [nA, nG], "ms": t_call[0], "ms_min_max": t_call[1:],
                           "z_GB_per_s": z_bytes / t_call[0] / 1e6, "TFLOP_per_s": flops / t_call[0] / 1e9}}))


if __name__ == "__main__":
    main()
