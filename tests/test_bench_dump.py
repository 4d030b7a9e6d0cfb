"""`bench.py --dump-outputs DIR` and the plain / `--full` split.

CPU: dump_outputs writes every layer's A, G, L_A, L_G as float32, whole while an array
fits its share of the byte budget and as the same seeded sample of its elements
otherwise, the same from call to call.

GPU: one plain `bench.py --gpus 1` run (2 steps of 2 full batches and a ragged third)
prints a line whose `--full` legs are null, and the arrays it dumps are the last timed
step's: A / G against the fp64 oracle on the regenerated records at rtol 1e-5 and L
against O.invert_factor on the dumped factor within 1e-4 of max|L| (the tolerances of
test_gpu_c2.py, the same path at full size).
"""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import bench
from conftest import ROOT
from oracle import kfac_oracle as O

IMAGES, BATCH = 9000, 4096  # 2 full batches + 808 rows


def _fake_kfac(sizes):
    g = torch.Generator().manual_seed(3)
    layers = [object() for _ in sizes]
    state = {l: [torch.randn(a, a, generator=g), torch.randn(b, b, generator=g)] for l, (a, b) in zip(layers, sizes)}
    inv = {l: tuple(t.tril() for t in state[l]) for l in layers}
    return types.SimpleNamespace(state=state, inv_state=inv), layers


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    kfac, layers = _fake_kfac([(40, 7), (9, 3)])
    # 8 arrays, 400 elements each: the 40 x 40 ones (1600) are sampled, the others whole
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 8 * 4 * 400)
    bench.dump_outputs(str(tmp_path / "a"), kfac, layers)
    bench.dump_outputs(str(tmp_path / "b"), kfac, layers)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(f"layer{i}_{n}.npy" for i in range(2) for n in ("A", "G", "L_A", "L_G"))
    total = 0
    for name in names:
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype == np.float32
        np.testing.assert_array_equal(a, b)
        total += a.nbytes
    assert total <= 8 * 4 * 400
    whole = kfac.state[layers[1]][0].numpy()
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "layer1_A.npy"), whole)
    big = kfac.state[layers[0]][0].numpy().reshape(-1)
    idx = np.sort(np.random.default_rng(0).integers(0, big.size, size=400))
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "layer0_A.npy"), big[idx])


def test_full_and_dump_outputs_options_parse():
    # a run that cannot start (no GPU visible, 2 ranks asked) still knows both options
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--full",
                        "--dump-outputs", "unused"], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "only 0 GPU(s) visible" in p.stderr
    assert not os.path.exists(os.path.join(ROOT, "unused"))


@pytest.mark.gpu
def test_plain_run_dumps_last_step_outputs(hip_device, tmp_path):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2",
                          "--warmup", "1", "--images", str(IMAGES), "--batch", str(BATCH),
                          "--dump-outputs", str(tmp_path)],
                         capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["dtype"] == "f32"
    assert line["value"] == pytest.approx(IMAGES / (1e-3 * line["ms_per_step"]))
    for leg in ("roofline", "cpu_baseline", "serial_images_per_s", "e2e_images_per_s", "other_configs",
                "eig", "parity"):
        assert line[leg] is None, leg

    specs = bench.CONFIGS["mlp"]
    recs = [(a.cpu().numpy(), g.cpu().numpy())
            for a, g in bench.synthetic_records(specs, IMAGES, hip_device, seed=1234)]
    starts = list(range(0, IMAGES, BATCH))
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= 64 * 10 ** 6
    for li, (l, (x, g)) in enumerate(zip(specs, recs)):
        wA = sum(O.linear_factor_A(x[i:i + BATCH], True, np.float64) for i in starts)
        wG = sum(O.grad_factor(g[i:i + BATCH], np.float64) for i in starts)
        for name, ref in (("A", wA), ("G", wG)):
            F = np.load(tmp_path / f"layer{li}_{name}.npy")
            assert F.dtype == np.float32 and F.shape == ref.shape
            np.testing.assert_allclose(F, ref, rtol=1e-5, atol=1e-6 * np.abs(ref).max(),
                                       err_msg=f"layer {li} {name}")
            L = np.load(tmp_path / f"layer{li}_L_{name}.npy")
            want = O.invert_factor(F.astype(np.float64), *bench.DAMPING)
            np.testing.assert_allclose(L, want, rtol=1e-4, atol=1e-4 * np.abs(want).max(),
                                       err_msg=f"layer {li} L_{name}")
