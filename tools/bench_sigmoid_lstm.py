#!/usr/bin/env python3
"""gan._SigmoidLSTM forward + backward at the trainer's shape (B, T, F, U) = (64, 30, 32, 8) (BASELINE configs[1], the last
layer of both discriminators) on the HIP path (one kccot_sigmoid_lstm launch each way) and on the tensor-op loop over T
(KCCOT_SIGMOID_LSTM=torch; the code of the commit before the kernels), in ONE process.

    python tools/bench_sigmoid_lstm.py [--reps 100] [--warmup 20] [--out profiles/sigmoid_lstm_bench.json]

Per path: 100 repetitions of module forward + backward after warm-up, each timed with a pair of events (host launch overhead
is part of what the layer costs a training step, so the launches are eager); median, p10 and p90 in microseconds; kernel
launches of one call counted with torch.profiler."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import kccotgan_amd  # noqa: F401
import torch
from torch.profiler import ProfilerActivity, profile
from kccotgan_amd import gan

SHAPE = dict(B=64, T=30, F=32, U=8)


def step(m, x, w):
    for p in m.parameters():
        p.grad = None
    x.grad = None
    (m(x) * w).sum().backward()


def measure(hip, m, x, w, reps, warmup):
    gan._SLSTM_HIP = hip
    for _ in range(warmup):
        step(m, x, w)
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step(m, x, w)
        b.record()
        b.synchronize()
        us.append(1e3 * a.elapsed_time(b))
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step(m, x, w)
        torch.cuda.synchronize()
    kernels = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    q = torch.tensor(us, dtype=torch.float64).quantile(torch.tensor([0.1, 0.5, 0.9], dtype=torch.float64)).tolist()
    return {"p10_us": q[0], "median_us": q[1], "p90_us": q[2], "launches_per_call": len(kernels),
            "sigmoid_lstm_kernels_per_call": sum("sigmoid_lstm" in k for k in kernels), "repetitions": reps, "warmup": warmup}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sigmoid_lstm_bench.json"))
    a = ap.parse_args()
    torch.manual_seed(0)
    m = gan._SigmoidLSTM(SHAPE["F"], SHAPE["U"]).cuda()
    x = torch.randn(SHAPE["B"], SHAPE["T"], SHAPE["F"], device="cuda", requires_grad=True)
    w = torch.randn(SHAPE["B"], SHAPE["T"], SHAPE["U"], device="cuda")
    was = gan._SLSTM_HIP
    try:
        out = {"shape": SHAPE, "what": "gan._SigmoidLSTM forward + backward, eager launches, event-timed per call",
               "device": torch.cuda.get_device_name(0),
               "hip": measure(True, m, x, w, a.reps, a.warmup), "loop": measure(False, m, x, w, a.reps, a.warmup)}
    finally:
        gan._SLSTM_HIP = was
    out["loop_median_over_hip_median"] = out["loop"]["median_us"] / out["hip"]["median_us"]
    out["hip_p90_below_loop_p10"] = out["hip"]["p90_us"] < out["loop"]["p10_us"]
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
