"""Queue schedules of KFAC.update() (a plain helper module): one table, run on the GPU bit for bit
(test_gpu_update_schedules.py) and on the CPU through host_double (test_update_schedules_host.py).

A schedule is one setting of the queue's knobs (defer_reduce, defer_batches, defer_bytes,
launch_first, merge_launches, double_buffer), one pattern of batch sizes, and whether
`kfac.state` is read mid-pass.  It runs three passes with reset() between them, each pass on
fresh records of the same shapes: the third pass runs on cached job templates alone.

Records are integers in [-3, 3] and batch sizes powers of two, so every term of
A = sum_b [a_b 1]^T [a_b 1] / rows_b and G = sum_b g_b^T g_b / rows_b is dyadic; `bound` is the
largest magnitude in units of the finest power of two that occurs (the per-batch mean of the
largest batch, times the ragged batch's in-kernel rescale last_rows / rows).  Below 2^24 every
fp32 partial sum is exact in any order and the device result is ONE fp32 matrix."""
import zlib
from types import SimpleNamespace as NS

import numpy as np
import torch
import torch.nn as nn

NETS = {
    # factor orders 257 / 36 / 37 / 10: the launch group routes to kfac_factor_tiles_x3
    "x3": lambda: nn.Sequential(nn.Linear(256, 36), nn.ReLU(), nn.Linear(36, 10)),
    # 21 / 12 / 12 / 5: the fp32 kfac_factor_tiles
    "fp32": lambda: nn.Sequential(nn.Linear(20, 12), nn.ReLU(), nn.Linear(12, 5, bias=False)),
}
# name -> (batch sizes of a pass, the update whose records are views one float into their allocation)
PATTERNS = {
    "full": ((64,) * 6, None),
    "short last": ((64, 64, 64, 64, 16), None),
    "short mid-pass": ((64, 64, 16, 64, 64), None),
    "two short sizes": ((64, 64, 32, 64, 64, 16), None),
    "view": ((32,) * 5, 2),
    "70 updates": ((16,) * 70, None),
}
DEFER_BATCHES = (1, 2, 3, 64, 128)
LAUNCH_FIRST = (1, 3, 16, 128)
PASSES = 3


def update_bytes(net, rows):
    dims = {"x3": (256, 36, 36, 10), "fp32": (20, 12, 12, 5)}[net]
    return 4 * rows * sum(dims)


def _table():
    out, k = [], 0
    for net in NETS:
        for pat, (sizes, view_at) in PATTERNS.items():
            for v in range(2 if pat == "70 updates" else 3):
                s = NS(net=net, pattern=pat, sizes=sizes, view_at=view_at,
                       defer_reduce=k % 7 != 6, defer_batches=DEFER_BATCHES[k % 5],
                       launch_first=LAUNCH_FIRST[(k // 2) % 4],
                       # large, or smaller than two updates of the largest batch
                       defer_bytes=512 << 20 if k % 3 else update_bytes(net, max(sizes)) * 3 // 2,
                       merge_launches=k % 2 == 0, double_buffer=k % 4 != 3,
                       read_mid=len(sizes) // 2 if k % 3 == 1 else None)
                if pat == "70 updates":  # one flush of more than KSEG batches from Python
                    s.defer_reduce, s.defer_batches, s.launch_first, s.defer_bytes = True, 128, 128, 512 << 20
                    s.read_mid = None
                s.name = (f"{net}/{pat}/{v}: defer_reduce={s.defer_reduce} defer_batches={s.defer_batches} "
                          f"defer_bytes={s.defer_bytes} launch_first={s.launch_first} merge_launches={s.merge_launches} "
                          f"double_buffer={s.double_buffer} read_mid={s.read_mid}")
                out.append(s)
                k += 1
    return out


SCHEDULES = _table()
IDS = [f"{s.net}-{s.pattern.replace(' ', '_')}-{i}" for i, s in enumerate(SCHEDULES)]


def layers(net):
    return [m for m in net if isinstance(m, nn.Linear)]


_DATA = {}


def records(s, p):
    """[update][layer] -> (a, g) int-valued fp32 numpy arrays of pass p."""
    key = (s.net, s.sizes, p)
    if key not in _DATA:
        rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
        dims = [(m.in_features, m.out_features) for m in layers(NETS[s.net]())]
        _DATA[key] = [[(rng.integers(-3, 4, size=(B, i)).astype(np.float32),
                        rng.integers(-3, 4, size=(B, o)).astype(np.float32)) for i, o in dims] for B in s.sizes]
    return _DATA[key]


def _sum(s, p, absolute=False):
    net = NETS[s.net]()
    out = []
    for li, m in enumerate(layers(net)):
        A = G = 0.0
        for rec in records(s, p):
            a, g = (x.astype(np.float64) for x in rec[li])
            if m.bias is not None:
                a = np.concatenate([a, np.ones((len(a), 1))], axis=1)
            if absolute:
                a, g = np.abs(a), np.abs(g)
            A = A + a.T @ a / len(a)
            G = G + g.T @ g / len(g)
        out += [A, G]
    return out


_REF = {}


def reference(s, p):
    """[A0, G0, A1, G1] of pass p (fp64, exact: dyadic terms)."""
    key = (s.net, s.sizes, p)
    if key not in _REF:
        _REF[key] = _sum(s, p)
    return _REF[key]


def bound(s, p):
    unit = (1.0 / max(s.sizes)) * (min(s.sizes) / max(s.sizes))
    return max(float(F.max()) for F in _sum(s, p, True)) / unit


def _tensor(x, device, view):
    t = torch.from_numpy(x)
    if not view:
        return t.to(device) if device.type != "cpu" else t.clone()
    flat = torch.empty(t.numel() + 1, dtype=torch.float32, device=device)
    out = flat[1:].view(t.shape)
    out.copy_(t)
    return out


def run(s, device, compare, after_pass=None):
    """Runs the schedule's passes; compare(what, got tensor, want fp64 array) per factor,
    after_pass(kfac, p) once the factors of pass p are compared."""
    from bnn_kfac_amd.curvatures import KFAC
    net = NETS[s.net]()
    kfac = KFAC(net)
    kfac.defer_reduce, kfac.defer_batches, kfac.defer_bytes = s.defer_reduce, s.defer_batches, s.defer_bytes
    kfac.launch_first, kfac.merge_launches, kfac.double_buffer = s.launch_first, s.merge_launches, s.double_buffer
    ls = layers(net)
    for p in range(PASSES):
        if p:
            kfac.reset()
        for u, rec in enumerate(records(s, p)):
            for m, (a, g) in zip(ls, rec):
                kfac.record[m] = [_tensor(a, device, u == s.view_at), _tensor(g, device, u == s.view_at)]
            kfac.update(len(rec[0][0]))
            if u == s.read_mid:
                _ = kfac.state
        state = kfac.state
        assert list(state) == ls
        want = reference(s, p)
        for li, m in enumerate(ls):
            for f, name in enumerate("AG"):
                compare(f"schedule {s.name}, pass {p}, layer {li} ({m}), factor {name}", state[m][f], want[2 * li + f])
        if after_pass is not None:
            after_pass(kfac, p)


def first_wrong(got, want):
    bad = np.argwhere(~(got == want))
    i, j = (int(v) for v in bad[0])
    return f"[{i}][{j}] got {got[i, j]!r} want {want[i, j]!r} ({len(bad)} entries differ)"
