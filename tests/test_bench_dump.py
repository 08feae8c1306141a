"""bench.py's contract with whoever compares builds (-m gpu): `--steps K` times exactly K steps, the result line holds
`ms_per_step`, and `--dump-outputs DIR` writes the loss and the five gradients of the last timed step, which equal an eager
evaluation of the same seeded inputs.  The benchmark runs in a CHILD process, as a driver would start it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WRT = ("fake", "h_fake", "h_real", "m_real", "m_fake")


@pytest.mark.gpu
def test_bench_steps_and_dumped_outputs(tmp_path):
    out_dir = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--no-cpu-baseline", "--no-train", "--no-configs", "--no-pmc", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert res["steps"] == 3 and res["warmup"] == 1
    assert res["ms_per_step"] > 0 and abs(res["value"] * res["ms_per_step"] - 1e3) < 1e-6 * 1e3
    assert sorted(os.listdir(out_dir)) == sorted(n + ".npy" for n in ["loss"] + ["grad_" + k for k in WRT])
    assert res["dumped_outputs"]["arrays"] == sorted(["loss"] + ["grad_" + k for k in WRT])

    from kccotgan_amd import gan_utils as G
    inp = cases.gen_inputs("cfg2", 0, "near")               # bench.py's headline inputs (configs[1], seed 0)
    t = {k: torch.from_numpy(v).cuda().requires_grad_(k in WRT) for k, v in inp.items()}
    loss = G.compute_sinkhorn_loss(t["real"], t["fake"], 1.0 / 15.0, 0.8, 100, t["h_fake"], t["m_real"], t["h_real"],
                                   t["m_fake"], video=True)
    grads = torch.autograd.grad(loss, [t[k] for k in WRT])
    dumped_loss = np.load(out_dir / "loss.npy")
    assert dumped_loss.dtype == np.float32 and dumped_loss.shape == ()
    assert float(dumped_loss) == res["config"]["loss"]
    np.testing.assert_allclose(dumped_loss, loss.detach().cpu().numpy(), rtol=1e-6)
    for k, g in zip(WRT, grads):
        d = np.load(out_dir / ("grad_%s.npy" % k))
        ref = g.cpu().numpy()
        assert d.dtype == np.float32 and d.shape == inp[k].shape, k
        np.testing.assert_allclose(d, ref, rtol=1e-5, atol=1e-6 * float(np.abs(ref).max()), err_msg=k)


# what only `bench.py --full` measures: a plain run prints the headline and nothing of this
FULL_ONLY = ("event_timing", "with_exact_shortcut", "eager_launches_ms_per_step", "roofline", "sinkhorn", "configs",
             "box_probe", "kernel_smoothing", "train_steps_per_sec", "train_steps_per_sec_data_parallel", "cpu_baseline")


@pytest.mark.gpu
def test_plain_bench_run_holds_the_headline_only():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["metric"] == "sinkhorn_loss_evals_per_sec" and res["higher_is_better"] is True and res["dtype"] == "f32"
    assert res["unit"] == "loss-evals/s (fwd+bwd)" and res["steps"] == 3 and res["warmup"] == 1
    assert res["ms_per_step"] > 0 and abs(res["value"] * res["ms_per_step"] - 1e3) < 1e-6 * 1e3
    assert res["config"]["sinkhorn_iters_executed"] == [100, 100, 100]
    assert not [k for k in FULL_ONLY if k in res] and "dumped_outputs" not in res
