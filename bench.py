#!/usr/bin/env python3
"""Benchmark of the hot path: one step = one compute_sinkhorn_loss evaluation, forward + backward
(gradients w.r.t. fake, h_fake, h_real, m_real, m_fake -- what the reference's generator step
differentiates, kernel_train.py:287-289), on synthetic video already resident in HBM.  At N=1 the
step is a hipGraph replay of the kernels (kccotgan_amd/graph.py; KCCOT_BENCH_EAGER=1 times eager
launches instead, also reported as `eager_launches_ms_per_step`).

Workload = BASELINE.json configs[1]: Moving-MNIST shape [B=64, H=64, T=30, W=64, C=1], J=8,
scaling_coef=1/15, epsilon=1, 100 Sinkhorn iterations (the as-called behaviour of the
reference: gan_utils.py:221-223).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times the K steps, writes --dump-outputs and prints the
headline keys.  The other blocks -- those listed below from `event_timing` to `cpu_baseline`, and `with_exact_shortcut`,
`eager_launches_ms_per_step`, `box_probe`, `kernel_smoothing`, `train_steps_per_sec_data_parallel` -- are measured only
with --full, after the timed region; --no-cpu-baseline / --no-train / --no-configs / --no-pmc leave parts of them out.
  value / ms_per_step  loss evaluations per second / the BASELINE "Sinkhorn-loss ms/iter": EXACTLY K steps between
                       two barriers, one wall-clock interval, max over ranks (the driver's contract).
  event_timing         the same step replayed >= 100 more times with a HIP event between consecutive replays (on the
                       stream the replays run on): median / p10 / p90 / min per step.
  roofline             the dominant kernel of cost assembly (the K-split partial-Gram kernel) timed alone with stream
                       events, against the BINDING bound of the pipe it executes on: the default kernel runs bf16
                       MFMAs (exact 3-way split), whose ideal (6.0 us) is below the HBM ideal (7.9 us) -> bound "hbm",
                       frac = algorithmic bytes / time / 8 TB/s.  The f32-MFMA-equivalent figure is a secondary key.
                       `traffic` = PMC bytes per launch from the rocprofv3 pass named in `traffic_source`.
  sinkhorn             the two latency-bound solver kernels timed alone: us per dependent half-step next to the
                       exp-issue floor of one CU (4096 v_exp_f32 at 16 per cycle = 256 cycles).
  train_steps_per_sec  the other half of BASELINE.json's metric: disc step + gen step (kernel_train.py:313-314) of the
                       PyTorch-ROCm G/D around this loss at the configs[1] shape, a few iterations in a child
                       process (bounded; MIOpen fast-find mode, stated in the block).
  configs              fwd+bwd time of the other BASELINE configs: single-GPU equivalents at N=1; the sharded step
                       at the N a config names when --gpus matches it.
  cpu_baseline         the CPU oracle in the reference's own formulation on this box's host cores, bounded sample
                       (N=1, rank 0 only).
  dumped_outputs       with --dump-outputs DIR: the loss and the five gradients of the LAST timed step, written as
                       DIR/loss.npy, DIR/grad_<name>.npy (float32, in full).  The inputs are seeded (tests/golden/cases.py),
                       so two builds run with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import signal
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import numpy as np   # noqa: E402
import torch         # noqa: E402
import kccotgan_amd  # noqa: E402,F401  (before the first CUDA call: its MIOpen solver switch must precede the GPU context)

SHAPE = dict(B=64, H=64, T=30, W=64, C=1, J=8)
SC = 1.0 / 15.0
HBM_PEAK_GBS = 8000.0         # MI355X_MICROARCH.md: HBM3E 8 TB/s (spec)
MFMA_F32_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: f32-input MFMA = f32 vector peak
MFMA_BF16_PEAK_TFLOPS = 2500.0  # dense bf16
PEAK_CLOCK_GHZ = 2.4
WRT = ("fake", "h_fake", "h_real", "m_real", "m_fake")
# BASELINE.json configs[2..4]: name -> (B, H, T, W, C, L, GPUs named by the config)
OTHER_CONFIGS = {
    "configs[2]": (128, 64, 30, 64, 3, 100, 4),
    "configs[3]": (256, 64, 30, 64, 3, 200, 8),
    "configs[4]": (512, 128, 48, 128, 3, 300, 8),
}


def make_inputs(B, seed, device, regime="near"):
    import cases
    shape_name = "cfg2"
    assert cases.SHAPES[shape_name][0] == SHAPE["B"]
    inp = cases.gen_inputs(shape_name, seed, regime)
    if B != SHAPE["B"]:
        inp = {k: v[:B] for k, v in inp.items()}
    return inp, {k: torch.from_numpy(v).to(device) for k, v in inp.items()}


def loss_step(G, t):
    loss = G.compute_sinkhorn_loss(t["real"], t["fake"], SC, 0.8, 100, t["h_fake"], t["m_real"], t["h_real"],
                                   t["m_fake"], video=True)
    grads = torch.autograd.grad(loss, [t[k] for k in WRT])
    return loss, grads


def dump_outputs(out_dir, loss, grads, suffix=""):
    """What a caller of the timed step receives -- the loss and its gradients w.r.t. WRT -- as `out_dir/<name><suffix>.npy`
    (float32, in full: 31.7 MB at the headline shape).  Returns the names written."""
    if not isinstance(grads, dict):
        grads = dict(zip(WRT, grads))
    arrays = {"loss": loss}
    arrays.update(("grad_" + k, grads[k]) for k in WRT)
    arrays = {k: v.detach().float().cpu().numpy() for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    assert total <= 64 << 20, "outputs of one step are %d bytes, more than the 64 MB a dump may hold" % total
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + suffix + ".npy"), a)
    return sorted(n + suffix for n in arrays)


def event_stats(step, reps):
    """`reps` replays with an event recorded on the current stream between consecutive ones: per-step GPU durations
    (the host queues ahead of the GPU, so consecutive events bracket exactly one step)."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    torch.cuda.synchronize()
    ev[0].record()
    for i in range(reps):
        step()
        ev[i + 1].record()
    torch.cuda.synchronize()
    d = np.array([ev[i].elapsed_time(ev[i + 1]) for i in range(reps)])
    return {"reps": reps, "median_ms": float(np.median(d)), "p10_ms": float(np.percentile(d, 10)),
            "p90_ms": float(np.percentile(d, 90)), "min_ms": float(d.min()), "mean_ms": float(d.mean()),
            "clock": "HIP events on the replay stream"}


def time_launches(launch, reps=200, warm=10):
    for _ in range(warm):
        launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3   # us


def time_cost_kernel(t, reps=200):
    """Average duration of the dominant cost kernel alone (KCCOT_COST_PARTIAL_ONLY) and of the whole cost stage,
    measured with events on the stream the kernels are launched on (torch's current stream)."""
    from kccotgan_amd import _lib
    from kccotgan_amd._lib import lib, ptr, stream_of, workspace, check
    B = t["real"].shape[0]
    real, fake = t["real"].detach().reshape(B, -1), t["fake"].detach().reshape(B, -1)
    K = real.shape[1]
    T, J = t["h_fake"].shape[1], t["h_fake"].shape[2]
    C3 = torch.empty(3, B, B, device=real.device)
    ws, wsb = workspace(lib.kccot_pairwise_cost3_workspace_bytes(B, K), real)
    hf, hr, mr, mf = (t[k].detach() for k in ("h_fake", "h_real", "m_real", "m_fake"))

    def launch(flags):
        check(lib.kccot_pairwise_cost3_f32(ptr(real), ptr(fake), B, K, SC, ptr(hf), ptr(hr), ptr(mr), ptr(mf),
                                           T, J, flags, ptr(C3), ws, wsb, stream_of(real)), "pairwise_cost3")

    out = {"partial": time_launches(lambda: launch(_lib.COST_PARTIAL_ONLY), reps),
           "stage": time_launches(lambda: launch(0), reps)}
    return out, K, C3


def pmc_child(mode="gram"):
    """`bench.py --pmc-child [gram|smooth]`: the launches the counter passes of live_pmc_traffic() / live_smoothing_traffic()
    observe and nothing else.  gram: 20 launches of the dominant cost kernel (KCCOT_COST_PARTIAL_ONLY) at configs[1].
    smooth: KernelSmoothing at the configs[1] shape -- temporal forward, 3-D forward, temporal backward, 3-D backward, five
    calls each, the four groups separated by a one-element torch fill (the marker the parent splits the dispatch list at)."""
    from kccotgan_amd import _lib
    from kccotgan_amd._lib import lib, ptr, stream_of, workspace, check
    dev = torch.device("cuda", 0)
    if mode == "smooth":
        B, H, T, W, C = SHAPE["B"], SHAPE["H"], SHAPE["T"], SHAPE["W"], SHAPE["C"]
        x = torch.rand(B, H, T, W, C, device=dev); g = torch.randn_like(x)
        o = torch.empty_like(x); d = torch.empty_like(x); m = torch.empty(1, device=dev)
        wsb = int(lib.kccot_smooth_workspace_bytes(B, H, T, W, C))
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        marker = torch.empty(1, device=dev)
        t_ax, all_ax = _lib.SMOOTH_T, _lib.SMOOTH_T | _lib.SMOOTH_H | _lib.SMOOTH_W
        torch.cuda.synchronize()
        for direction in ("fwd", "bwd"):
            for axes in (t_ax, all_ax):
                if direction == "bwd":      # a valid (out, max) pair of this kind for the adjoint
                    check(lib.kccot_smooth_fwd_f32(ptr(x), B, H, T, W, C, 5.0, 3, axes, ptr(o), ptr(m), ws.data_ptr(), wsb, None), "smooth_fwd")
                marker.fill_(1.0)
                for _ in range(5):
                    if direction == "fwd":
                        check(lib.kccot_smooth_fwd_f32(ptr(x), B, H, T, W, C, 5.0, 3, axes, ptr(o), ptr(m), ws.data_ptr(), wsb, None), "smooth_fwd")
                    else:
                        check(lib.kccot_smooth_bwd_f32(ptr(g), ptr(o), ptr(m), B, H, T, W, C, 5.0, 3, axes, ptr(d), ws.data_ptr(), wsb, None), "smooth_bwd")
                marker.fill_(2.0)
        torch.cuda.synchronize()
        return
    _, t = make_inputs(SHAPE["B"], 0, dev)
    B = SHAPE["B"]
    real, fake = t["real"].reshape(B, -1), t["fake"].reshape(B, -1)
    K = real.shape[1]
    T, J = t["h_fake"].shape[1], t["h_fake"].shape[2]
    C3 = torch.empty(3, B, B, device=dev)
    ws, wsb = workspace(lib.kccot_pairwise_cost3_workspace_bytes(B, K), real)
    for _ in range(20):
        check(lib.kccot_pairwise_cost3_f32(ptr(real), ptr(fake), B, K, SC, ptr(t["h_fake"]), ptr(t["h_real"]), ptr(t["m_real"]),
                                           ptr(t["m_fake"]), T, J, _lib.COST_PARTIAL_ONLY, ptr(C3), ws, wsb, stream_of(real)),
              "pairwise_cost3")
    torch.cuda.synchronize()


def pmc_passes(mode, timeout_s=120):
    """Two rocprofv3 passes (--pmc FETCH_SIZE, then --pmc WRITE_SIZE: one counter per pass, no trace domain besides the kernel
    trace, as MI355X_MICROARCH.md's HBM section prescribes) over `bench.py --pmc-child <mode>`.  Returns ({counter: [(kernel
    name, bytes) in dispatch order]}, None) -- counters in KiB -> bytes, no other correction applied here -- or (None, reason):
    no rocprofv3, a profiler already attached to this process, a timeout (the whole process group is killed: rocprofv3 is a
    launcher, killing only it would orphan the python child that owns the GPU), a non-zero exit."""
    import csv, glob, shutil, tempfile
    exe = shutil.which("rocprofv3")
    if not exe:
        return None, "rocprofv3 not on PATH"
    if any("rocprof" in os.environ.get(k, "").lower() for k in ("LD_PRELOAD", "ROCP_TOOL_LIBRARIES", "HSA_TOOLS_LIB")):
        return None, "this process already runs under a profiler"
    out = {}
    tmp = tempfile.mkdtemp(prefix="kccot_pmc_", dir="/tmp")
    try:
        env = dict(os.environ, TMPDIR="/tmp")
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            out_dir = os.path.join(tmp, counter)
            cmd = [exe, "--kernel-trace", "--pmc", counter, "--output-format", "csv", "-d", out_dir, "--",
                   sys.executable, os.path.abspath(__file__), "--pmc-child", mode]
            proc = subprocess.Popen(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, start_new_session=True)
            try:
                stdout, _ = proc.communicate(timeout=timeout_s)
            except subprocess.TimeoutExpired:
                try:
                    os.killpg(proc.pid, signal.SIGKILL)
                except ProcessLookupError:
                    pass
                proc.communicate()
                return None, "rocprofv3 --pmc %s timed out after %d s (process group killed)" % (counter, timeout_s)
            if proc.returncode != 0:
                tail = " | ".join(stdout.decode(errors="replace").strip().splitlines()[-3:])
                return None, "rocprofv3 --pmc %s exited with %d: %s" % (counter, proc.returncode, tail[-300:])
            rows = []
            for f in glob.glob(os.path.join(out_dir, "**", "*counter_collection.csv"), recursive=True):
                for row in csv.DictReader(open(f)):
                    if row.get("Counter_Name") == counter:
                        rows.append((int(row.get("Dispatch_Id", len(rows))), row.get("Kernel_Name", ""), float(row["Counter_Value"]) * 1024.0))
            if not rows:
                return None, "no %s rows" % counter
            rows.sort()
            out[counter] = [(k, v) for _, k, v in rows]
    except Exception as e:            # the bench line must not depend on the profiler
        return None, "counter pass failed: %r" % (e,)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return out, None


def live_pmc_traffic(kernel_prefix="gram128_partial"):
    """HBM-side bytes per launch of the dominant kernel, MEASURED IN THIS RUN (pmc_passes("gram")): FETCH_SIZE doubled (gfx950
    counts a wide coalesced read at half its bytes).  Returns (bytes, note) or (None, reason): any failure leaves the
    committed figure of profiles/hbm_traffic.json."""
    res, why = pmc_passes("gram")
    if res is None:
        return None, why
    per = {}
    for counter, rows in res.items():
        vals = [v for k, v in rows if kernel_prefix in k]
        if not vals:
            return None, "no %s rows for %s" % (counter, kernel_prefix)
        per[counter] = (sum(vals) / len(vals), len(vals))
    fetch, write = 2.0 * per["FETCH_SIZE"][0], per["WRITE_SIZE"][0]
    return fetch + write, ("measured in this run: rocprofv3 --kernel-trace --pmc FETCH_SIZE / WRITE_SIZE in two separate passes "
                           "over %d + %d launches of a child process (bench.py --pmc-child), KiB units, FETCH_SIZE x2 (gfx950 "
                           "wide-read correction): fetch %.2f MB + write %.2f MB"
                           % (per["FETCH_SIZE"][1], per["WRITE_SIZE"][1], fetch / 1e6, write / 1e6))


def live_smoothing_traffic():
    """HBM-side bytes per KernelSmoothing CALL at the configs[1] shape, measured in this run (pmc_passes("smooth")): the child
    runs temporal forward / 3-D forward / temporal backward / 3-D backward, five calls each between one-element torch fills;
    the dispatch list of each pass is cut at those markers and the kccot kernels between a pair are summed and divided by
    five.  FETCH_SIZE doubled as for the Gram kernel.  Returns ({"temporal_fwd": bytes, ...}, note) or (None, reason)."""
    res, why = pmc_passes("smooth")
    if res is None:
        return None, why
    names = ("temporal_fwd", "conv3d_fwd", "temporal_bwd", "conv3d_bwd")
    tot = {n: 0.0 for n in names}
    for counter, rows in res.items():
        groups, cur, opened = [], None, False
        for k, v in rows:
            if "FillFunctor" in k:
                if not opened:
                    cur, opened = [], True
                else:
                    groups.append(cur)
                    cur, opened = None, False
            elif opened and "kccot::" in k:
                cur.append(v)
        if len(groups) != 4 or not all(groups):
            return None, "could not split the %s dispatch list at the markers (%d groups)" % (counter, len(groups))
        for n, g in zip(names, groups):
            tot[n] += (2.0 if counter == "FETCH_SIZE" else 1.0) * sum(g) / 5.0
    return tot, "measured in this run: two rocprofv3 --pmc passes (FETCH_SIZE x2, WRITE_SIZE) over bench.py --pmc-child smooth, five calls per kind"


def time_sinkhorn(C3, L=100, reps=50):
    """The three-problem solve and its reverse sweep alone (every iteration executed: main sets the option
    "sinkhorn_shortcut" = 0): us per launch and per dependent half-step."""
    from kccotgan_amd._lib import lib, ptr, stream_of, check, workspace
    n = C3.shape[1]
    dev = C3.device
    uh, vh = torch.empty(3, L, n, device=dev), torch.empty(3, L, n, device=dev)
    cost3, loss = torch.empty(3, device=dev), torch.empty(1, device=dev)
    nits = torch.zeros(6, dtype=torch.int32, device=dev)
    ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    g = torch.ones(1, device=dev)
    dC3 = torch.empty_like(C3)
    st = stream_of(C3)
    fwd = lambda: check(lib.kccot_sinkhorn_divergence_fwd_f32(ptr(C3), n, 1.0, L, 100, 1e-2, ptr(uh), ptr(vh), ptr(cost3),
                                                              ptr(nits), ptr(loss), ptr(ticket), None, 0, st), "sk_fwd")
    bwd = lambda: check(lib.kccot_sinkhorn_divergence_bwd_f32(ptr(C3), ptr(uh), ptr(vh), ptr(nits), n, 1.0, L, ptr(g),
                                                              ptr(dC3), None, 0, st), "sk_bwd")
    f_us = time_launches(fwd, reps, 5)
    b_us = time_launches(bwd, reps, 5)
    its = int(nits[:3].max())
    floor_us = 256.0 / (PEAK_CLOCK_GHZ * 1e3)
    fused = {}
    if lib.kccot_sinkhorn_fused_eligible(n, L):
        # what the loss path runs when a gradient is wanted: solves + reverse sweep in ONE launch, history in LDS
        fu = lambda: check(lib.kccot_sinkhorn_divergence_fused_f32(ptr(C3), n, 1.0, L, 100, 1e-2, ptr(cost3), ptr(nits),
                                                                   ptr(loss), ptr(ticket), ptr(dC3), st), "sk_fused")
        fu_us = time_launches(fu, reps, 5)
        fused = {"fused_fwd_bwd_us": fu_us, "fused_us_per_half_step": fu_us / (4 * its),
                 "fused_over_floor": fu_us / (4 * its) / floor_us, "two_launch_fwd_plus_bwd_us": f_us + b_us}
    # the multi-CU solver of the larger configs (n = 256 = configs[3]): one problem per XCD, duals through that XCD's L2
    multi = {}
    try:
        from kccotgan_amd import _lib as _kl
        nm = 256
        Cm = torch.rand((3, nm, nm), device=C3.device) * 30
        uhm, vhm = torch.empty(3, L, nm, device=C3.device), torch.empty(3, L, nm, device=C3.device)
        cm, nim = torch.empty(3, device=C3.device), torch.zeros(6, dtype=torch.int32, device=C3.device)
        wsm, wsbm = workspace(lib.kccot_sinkhorn_workspace_bytes(3, nm), Cm)
        fm = lambda: check(lib.kccot_sinkhorn_fwd_f32(ptr(Cm), 3, nm, 1.0, L, 100, 1e-2, 0, ptr(uhm), ptr(vhm), ptr(cm), ptr(nim),
                                                      None, wsm, wsbm, st), "sk_fwd_n256")
        for mode, key in ((1, "xcd_l2_exchange"), (0, "agent_scope_exchange")):
            with _kl.options(sinkhorn_coop_xcd=mode):
                us = time_launches(fm, 20, 3)
            multi["n256_fwd_us_per_iteration_" + key] = us / max(int(nim[:3].max()), 1)
    except Exception as e:
        multi = {"n256_error": repr(e)}
    return {"n": n, "iterations": its, "fwd_us": f_us, "bwd_us": b_us, **fused, "multi_cu": multi,
            "fwd_us_per_half_step": f_us / (2 * its), "bwd_us_per_half_step": b_us / (2 * its),
            "fwd_cycles_per_half_step_at_2.4GHz": f_us / (2 * its) * PEAK_CLOCK_GHZ * 1e3,
            "exp_issue_floor_cycles": 256, "exp_issue_floor_us_per_half_step": floor_us,
            "fwd_over_floor": f_us / (2 * its) / floor_us,
            "note": "one CU per problem: n*n v_exp_f32 per half-step at 16 lanes/cycle/CU (quarter rate) = 256 cycles; "
                    "latency-bound chain, not a roofline fraction (SURVEY.md 8d)"}


def cpu_baseline(inp, budget_s=25.0):
    """The CPU oracle in the reference's formulation ([B,B,T,D] broadcast, three separate cost
    builds, eager per-iteration Sinkhorn ops, autograd through the unrolled loop), fp32, all host
    threads torch uses.  Bounded: at least one evaluation, then as many as fit in the budget."""
    from oracle import gan_utils_torch as ot
    t = {k: torch.from_numpy(v) for k, v in inp.items()}
    for k in WRT:
        t[k].requires_grad_(True)
    n, t0 = 0, time.perf_counter()
    while True:
        loss = ot.compute_sinkhorn_loss(t["real"], t["fake"], SC, 0.8, 100, t["h_fake"], t["m_real"], t["h_real"],
                                        t["m_fake"], video=True)
        torch.autograd.grad(loss, [t[k] for k in WRT])
        n += 1
        el = time.perf_counter() - t0
        if el > budget_s or el + el / n > 1.6 * budget_s:
            break
    return dict(value=n / el, unit="loss-evals/s", cores=torch.get_num_threads(), kind="port",
                sample="%d fwd+bwd evaluations of configs[1] (B=64,T=30,64x64x1, reference formulation, torch-CPU fp32) "
                       "in %.1f s; host has %d logical cpus" % (n, el, os.cpu_count()),
                loss=float(loss))


def train_steps_child(timeout_s=150, fallback_timeout_s=240):
    """train-steps/sec in a CHILD process (a fault in stock MIOpen convolutions must not cost the headline line):
    tools/bench_train.py at the configs[1] shape.  First with MIOpen's default find mode, which reads the solver choices
    shipped in kccotgan_amd/miopen_db (first iteration: seconds); if that database does not match the installed MIOpen
    the exhaustive search would take ~5 minutes, so the child is stopped after `timeout_s` and the measurement is
    repeated with MIOPEN_FIND_MODE=2 (fast find: first iteration ~10 s, steady state ~2.6x slower).
    The line says which of the two it was."""
    def run(env, limit):
        cmd = [sys.executable, os.path.join(ROOT, "tools", "bench_train.py"), "--json", "--iters", "3", "--kernel", "none"]
        p = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        try:
            out, err = p.communicate(timeout=limit)
        except subprocess.TimeoutExpired:
            p.kill()
            p.communicate()
            return None, "child exceeded %d s" % limit
        if p.returncode != 0:
            return None, "child exit code %d: %s" % (p.returncode, err.strip()[-300:])
        return json.loads(out.strip().splitlines()[-1]), None

    t0 = time.perf_counter()
    base = dict(os.environ)
    base.pop("KCCOT_OPTIONS", None)                 # the trainer child runs on the shipped defaults
    base.pop("MIOPEN_FIND_MODE", None)
    try:
        r, err = run(base, timeout_s)
        mode = "default find mode + shipped find-db (kccotgan_amd/miopen_db)"
        if r is None:
            first_err = err
            r, err = run(dict(base, MIOPEN_FIND_MODE="2"), fallback_timeout_s)
            mode = "MIOPEN_FIND_MODE=2 fast find (default-mode child: %s)" % first_err
        if r is None:
            return {"value": None, "error": err}
    except Exception as e:
        return {"value": None, "error": repr(e)}
    return {"value": r["train_steps_per_sec"], "unit": "train-steps/s (disc step + gen step)",
            "ms_per_train_step": r["ms_per_train_step"], "iterations_timed": r["iterations"],
            "first_iteration_s": r["first_iteration_s"],
            "config": "B=64, T=30 (5 context + 25 predicted), 64x64x1, filter sizes 8, z 128, kernel=none, "
                      "PyTorch-ROCm G/D (MIOpen, %s, faulting NHWC bwd solver off) + HIP loss path" % mode,
            "pM": r["pm"], "loss": r["loss"], "child_wall_s": time.perf_counter() - t0}


def box_probe(dev):
    """What this box's memory system delivers on multi-GB buffers, independent of any kccot kernel: a 4 GiB device-to-device
    copy (read + write).  Context for the `configs` block: some boxes of the pool run every multi-GB workload 3-4x slower than
    others (configs[4]: 82 ms against 27.7 ms with the same library) while everything up to a few hundred MB is unaffected."""
    try:
        n = 1 << 30
        a = torch.empty(n, dtype=torch.float32, device=dev).fill_(1.0)
        b = torch.empty_like(a)
        b.copy_(a)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(3):
            b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 3
        del a, b
        torch.cuda.empty_cache()
        return {"d2d_copy_4GiB_ms": ms, "read_plus_write_GBps": 2 * 4 * n / ms / 1e6}
    except Exception as e:
        return {"error": repr(e)}


def config_inputs(B, H, T, W, C, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    real = torch.rand((B, H, T, W, C), device=dev, generator=g)
    fake = (real + 0.05 * torch.randn(real.shape, device=dev, generator=g)).clamp_(0, 1)
    t = {"real": real, "fake": fake}
    for k in ("h_fake", "m_real", "h_real", "m_fake"):
        t[k] = torch.rand((B, T, SHAPE["J"]), device=dev, generator=g)
    return t


def single_gpu_configs(G, dev):
    """One-GPU fwd+bwd time of BASELINE configs[2..4] at full size (what every rank of the sharded path would do
    without the all-gather, plus all row blocks instead of B/G of them).  L > 100 through honor_eps_l (the
    keyword route of the reference, gan_utils.py:124); the executed iteration counts are reported."""
    out = {}
    for name, (B, H, T, W, C, L, ngpu) in OTHER_CONFIGS.items():
        t = config_inputs(B, H, T, W, C, dev)
        for k in WRT:
            t[k].requires_grad_(True)

        def step():
            loss = G.compute_sinkhorn_loss(t["real"], t["fake"], SC, 1.0, L, t["h_fake"], t["m_real"], t["h_real"],
                                           t["m_fake"], honor_eps_l=True)
            return loss, torch.autograd.grad(loss, [t[k] for k in WRT])

        loss, grads = step()
        torch.cuda.synchronize()
        reps = 5 if B <= 256 else 2
        st = event_stats(step, reps)
        K = H * T * W * C
        alg_bytes = 2 * B * K * 4 + 16 * B * T * SHAPE["J"] + 12 * B * B
        # the same step replayed as a hipGraph (how the headline is timed: no host launch gaps between its ~15 kernels)
        graph_ms = None
        try:
            from kccotgan_amd.graph import GraphedLossStep
            gs = GraphedLossStep(t, SC, 1.0, L, warmup=1, honor_eps_l=True, clone=False)
            gl, _ = gs()
            torch.cuda.synchronize()
            if abs(float(gl) - float(loss)) <= 1e-6 * abs(float(loss)):
                graph_ms = event_stats(lambda: gs(), reps)["median_ms"]
                # the LAST replay must still be the same evaluation (a solve that gives up runs fast: NaN, negative count)
                if not (abs(float(gs.loss) - float(loss)) <= 1e-6 * abs(float(loss)) and int(gs.nits.min()) > 0):
                    graph_ms = None
            del gs
        except Exception as e:
            sys.stderr.write("bench: graph replay of %s failed: %r\n" % (name, e))
        out[name] = {"B": B, "K": K, "L": L, "gpus_named_by_config": ngpu, "n_gpus_here": 1,
                     "ms_fwd_bwd_median": st["median_ms"], "ms_fwd_bwd_min": st["min_ms"], "reps": reps,
                     "ms_fwd_bwd_graph_replay_median": graph_ms,
                     "sinkhorn_iters": G.last_info["compute_sinkhorn_loss"].tolist(),
                     "loss": float(loss), "finite": bool(torch.isfinite(grads[0]).all()),
                     "algorithmic_MB_fwd": alg_bytes / 1e6, "algorithmic_GFLOP_fwd": 4 * B * B * K / 1e9,
                     "ideal_ms_fwd_hbm": alg_bytes / (HBM_PEAK_GBS * 1e9) * 1e3,
                     "ideal_ms_fwd_f32_mfma": 4 * B * B * K / (MFMA_F32_PEAK_TFLOPS * 1e12) * 1e3}
        del t, grads, loss
        torch.cuda.empty_cache()
    return out


def time_smoothing(dev):
    """KernelSmoothing forward and backward, kernel time with HIP events, at the configs[1]
    shape and at the one-GPU shapes of the larger BASELINE configs that fit: us per call and the fraction of the HBM
    roofline at the algorithmic bytes (forward: read + write the tensor once; backward: read gradient and forward
    output, write the input gradient)."""
    from kccotgan_amd import _lib
    from kccotgan_amd._lib import lib, ptr, check
    shapes = {"configs[1]": (SHAPE["B"], SHAPE["H"], SHAPE["T"], SHAPE["W"], SHAPE["C"])}
    for name, c in OTHER_CONFIGS.items():
        shapes[name] = c[:5]
    out = {}
    # HBM-side traffic per call from the committed counter passes (tools/pmc_smooth.sh -> profiles/smooth_traffic.json):
    # every smoothing kernel moves its tensor exactly once, so the ratio is the number of tensor passes over the minimum
    traffic = {}
    tf_path = os.path.join(ROOT, "profiles", "smooth_traffic.json")
    if os.path.exists(tf_path):
        traffic = json.load(open(tf_path)).get("calls", {})
    for name, (B, H, T, W, C) in shapes.items():
        n = B * H * T * W * C
        if n * 4 * 5 > 60e9:
            continue
        x = torch.rand(B, H, T, W, C, device=dev); g = torch.randn_like(x)
        o = torch.empty_like(x); d = torch.empty_like(x); m = torch.empty(1, device=dev)
        wsb = int(lib.kccot_smooth_workspace_bytes(B, H, T, W, C))
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        rec = {"shape_BHTWC": [B, H, T, W, C], "sigma": 5.0, "radius": 3}
        for key, axes in (("temporal", _lib.SMOOTH_T), ("conv3d", _lib.SMOOTH_T | _lib.SMOOTH_H | _lib.SMOOTH_W)):
            fwd = lambda: check(lib.kccot_smooth_fwd_f32(ptr(x), B, H, T, W, C, 5.0, 3, axes, ptr(o), ptr(m), ws.data_ptr(), wsb,
                                                         None), "smooth_fwd")
            bwd = lambda: check(lib.kccot_smooth_bwd_f32(ptr(g), ptr(o), ptr(m), B, H, T, W, C, 5.0, 3, axes, ptr(d), ws.data_ptr(),
                                                         wsb, None), "smooth_bwd")
            reps = 100 if n < 5e7 else 10
            tf = time_launches(fwd, reps=reps, warm=3)
            tb = time_launches(bwd, reps=reps, warm=3)
            rec[key] = {"fwd_us": tf, "bwd_us": tb, "fwd_hbm_frac": 8.0 * n / (tf * 1e-6) / (HBM_PEAK_GBS * 1e9),
                        "bwd_hbm_frac": 12.0 * n / (tb * 1e-6) / (HBM_PEAK_GBS * 1e9)}
            for direction in ("fwd", "bwd"):
                t_rec = traffic.get("%dx%dx%dx%dx%d_%s_%s" % (B, H, T, W, C, key, direction))
                if t_rec:
                    rec[key][direction + "_traffic_over_algorithmic"] = t_rec["traffic_over_algorithmic"]
        out[name] = rec
        del x, g, o, d, ws
        torch.cuda.empty_cache()
    return out


def _all_ok(ok, dev, dist):
    """True only if EVERY rank succeeded (one rank failing alone -- out of memory, a workspace -- must not leave the others
    blocked in the next barrier: all ranks learn it here and skip the timed region together)."""
    flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=dev if dist.get_backend() == "nccl" else "cpu")
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    return int(flag) == 1


def _max_over_ranks(x, dev, dist):
    tt = torch.tensor([x], dtype=torch.float64, device=dev if dist.get_backend() == "nccl" else "cpu")
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    return float(tt)


def sharded_shape(tag, B, H, T, W, C, L, rank, world, dev, dist, barrier, steps=5):
    """The batch-sharded loss step (kccotgan_amd.dist) of ONE global shape on `world` ranks, timed with EVERY protocol the
    shape supports -- `gather` (all-gather the batch, row blocks on the matrix pipe: what BASELINE.json's north star
    prescribes), `gather_chunks` (the same with the videos travelling as 4 column ranges, Gram sums accumulated behind the
    arrivals) and `ksplit` (all-to-all into K-slices, all-reduced fp64 Gram sums) -- and, per protocol, the device time of
    each phase (max over ranks, ms per step: input exchange, cost rows, cost exchange, Sinkhorn forward / reverse sweep,
    gradient rows; kccotgan_amd.dist.phase_ms) so that the curve can be read against DESIGN.md section 6's table."""
    from kccotgan_amd import dist as kd
    Bl = B // world
    K = H * T * W * C
    t = config_inputs(Bl, H, T, W, C, dev, seed=100 + rank)       # this rank's shard only
    shard = {k: v.requires_grad_(k != "real") for k, v in t.items()}
    protocols = [("gather", "gather", None)]
    if B > 64 and K >= 4096:
        protocols.append(("gather_chunks", "gather", "4"))
    if kd.ksplit_supported(B, K, world):
        protocols.append(("ksplit", "ksplit", None))
    rec = {"B": B, "per_rank_B": Bl, "K": K, "L": L, "n_gpus_here": world, "steps": steps, "protocols": {}}
    for label, proto, chunks in protocols:
        if chunks:
            os.environ["KCCOT_DIST_GATHER_CHUNKS"] = chunks        # every rank alike
        else:
            os.environ.pop("KCCOT_DIST_GATHER_CHUNKS", None)
        step = lambda: kd.sharded_loss_step(shard, SC, epsilon=1.0, L=L, protocol=proto)
        note(rank, "sharded %s B=%d K=%d: %s" % (tag, B, K, label))
        err, loss = None, None
        try:
            loss, _ = step()
            torch.cuda.synchronize()
        except Exception as e:
            err = repr(e)
        if not _all_ok(err is None, dev, dist):
            rec["protocols"][label] = {"error": err or "another rank failed"}
            continue
        barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss, _g = step()
        barrier()
        el = _max_over_ranks(time.perf_counter() - t0, dev, dist)
        # phases: three more steps with an event at every boundary
        kd.phase_timing(True)
        for _ in range(3):
            step()
        ph = kd.phase_ms()
        kd.phase_timing(False)
        n = max(ph.pop("steps", 1), 1)
        phases = {k: _max_over_ranks(v / n, dev, dist) for k, v in sorted(ph.items())}
        rec["protocols"][label] = {"ms_fwd_bwd": el / steps * 1e3, "loss": float(loss.detach()), "phases_ms_max_over_ranks": phases,
                                   "sinkhorn_iters": kd.last_info["nits"].tolist() if "nits" in kd.last_info else None}
    os.environ.pop("KCCOT_DIST_GATHER_CHUNKS", None)
    ok = {k: v["ms_fwd_bwd"] for k, v in rec["protocols"].items() if "ms_fwd_bwd" in v}
    if ok:
        best = min(ok, key=ok.get)
        rec["ms_fwd_bwd"], rec["protocol"] = ok[best], best
        rec["samples_per_sec"] = B / (ok[best] * 1e-3)
    del t, shard
    torch.cuda.empty_cache()
    return rec


def note(rank, msg):
    """Progress line on stderr (rank 0): a run of several minutes must not look hung to whoever watches the log."""
    if rank == 0:
        sys.stderr.write("bench: %s\n" % msg)
        sys.stderr.flush()


def dp_train_children(rank, world, local_rank, backend, timeout_s=200):
    """Data-parallel train-steps/s (disc step + gen step, kernel_train.py:313-314, GLOBAL-batch loss through
    kccotgan_amd.dist) in CHILD processes, one per rank, with a rendezvous of their own -- a fault in stock MIOpen must not
    cost the line, and the children can be given a time limit.  Two runs: `weak` (per-rank batch 64: the configs[1] trainer
    replicated, global batch 64 N; MIOpen's solver choices come from the shipped find-db) and `strong` (global batch 64,
    per-rank 64 / N; shapes the find-db does not hold, so MIOpen's fast find mode is used and the line says so)."""
    port = int(os.environ.get("MASTER_PORT", "29500"))
    out = {}
    for label, per_rank, find2, off in (("weak_per_rank_batch_64", 64, False, 17), ("strong_global_batch_64", 64 // world, True, 18)):
        if per_rank < 1 or (64 % world and label.startswith("strong")):
            continue
        env = dict(os.environ, MASTER_PORT=str(port + off), KCCOT_TRAIN_DIST_BACKEND=backend)
        for k in [k for k in env if k.startswith("TORCHELASTIC_")]:
            env.pop(k)        # (TORCHELASTIC_USE_AGENT_STORE would make the children look for the launcher's store on THEIR port)
        env.pop("KCCOT_OPTIONS", None)
        env.pop("MIOPEN_FIND_MODE", None)
        if find2:
            env["MIOPEN_FIND_MODE"] = "2"
        cmd = [sys.executable, os.path.join(ROOT, "tools", "bench_train.py"), "--json", "--iters", "3", "--kernel", "none",
               "--dist", "--batch", str(per_rank)]
        note(rank, "data-parallel trainer children: %s" % label)
        t0 = time.perf_counter()
        p = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
        try:
            so, se = p.communicate(timeout=timeout_s)
            err = None if p.returncode == 0 else "child exit code %d: %s" % (p.returncode, se.strip()[-300:])
        except subprocess.TimeoutExpired:
            try:
                os.killpg(p.pid, signal.SIGKILL)
            except ProcessLookupError:
                pass
            so, se = p.communicate()
            err = "child exceeded %d s" % timeout_s
        if rank == 0:
            if err:
                out[label] = {"value": None, "error": err}
            else:
                try:
                    r = json.loads(so.strip().splitlines()[-1])
                    out[label] = {"value": r["train_steps_per_sec"], "unit": "train-steps/s (disc step + gen step), all ranks in step",
                                  "ms_per_train_step": r["ms_per_train_step"], "per_rank_batch": per_rank,
                                  "global_batch": per_rank * world, "samples_per_sec": per_rank * world * r["train_steps_per_sec"],
                                  "first_iteration_s": r["first_iteration_s"], "miopen_find_mode": r["find_mode"],
                                  "loss": r["loss"], "pM": r["pm"], "child_wall_s": time.perf_counter() - t0}
                except Exception as e:
                    out[label] = {"value": None, "error": "unreadable child output: %r" % (e,)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also record everything else: event timing, the exact-shortcut and eager "
                         "timings, roofline, Sinkhorn kernels, configs[2..4], kernel smoothing, train-steps/sec, CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-train", action="store_true", help="--full: skip the train-steps/sec child process")
    ap.add_argument("--no-configs", action="store_true", help="--full: skip the configs[2..4] block")
    ap.add_argument("--no-pmc", action="store_true", help="--full: do not re-measure roofline.traffic (two rocprofv3 counter "
                                                          "passes over a child process); report the committed figure")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the loss and gradients of the last timed step to DIR/<name>.npy (N > 1: <name>.rank<r>.npy, "
                         "each rank its shard)")
    ap.add_argument("--pmc-child", nargs="?", const="gram", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.pmc_child:
        pmc_child(args.pmc_child)
        return

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        if world == 1 and args.gpus > 1:
            raise SystemExit("bench.py --gpus %d must be launched with torch.distributed.run (WORLD_SIZE=%d)"
                             % (args.gpus, world))
    # KCCOT_BENCH_BACKEND=gloo rehearses the N>1 path on ONE GPU (all ranks on cuda:0, collectives
    # staged through the host); the driver's multi-GPU runs use nccl (= RCCL), one GPU per rank.
    backend = os.environ.get("KCCOT_BENCH_BACKEND", "nccl")
    ndev = torch.cuda.device_count()
    dev_index = local_rank if (backend == "nccl" or local_rank < ndev) else local_rank % max(ndev, 1)
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    from kccotgan_amd import gan_utils as G
    # The headline is timed with the Sinkhorn solver's exact periodic-state shortcut DISABLED, so that all
    # 3 x 100 iterations (and the full reverse sweep) are executed whatever the data: `value` then
    # does not depend on how quickly the synthetic batch happens to reach its fp32 fixed point.  The
    # shipped default (shortcut on, bit-identical results) is timed separately below.
    from kccotgan_amd import _lib as kl
    kl.set_option("sinkhorn_shortcut", 0)
    inp, t = make_inputs(SHAPE["B"], 0, dev)
    for k in WRT:
        t[k].requires_grad_(True)

    mode = "eager launches"
    if world > 1:
        from kccotgan_amd import dist as kd
        shard = kd.shard_batch(t, rank, world)
        step = lambda: kd.sharded_loss_step(shard, SC)
        if os.environ.get("KCCOT_BENCH_EAGER") != "1":
            # the collectives stay RCCL calls; the two compute segments between them replay as hipGraphs
            # (kccotgan_amd/graph.py: the eager sharded step is host-bound, 0.36 ms of Python for 0.22 ms of kernels)
            gstep = None
            try:
                if os.environ.get("KCCOT_DIST_PROTOCOL") == "ksplit":
                    # opt-in: contraction-sharded protocol (all-to-all into K-slices, all-reduced Gram sums)
                    from kccotgan_amd.graph import GraphedKSplitStep
                    gstep = GraphedKSplitStep(shard, SC)
                else:
                    from kccotgan_amd.graph import GraphedShardedStep
                    gstep = GraphedShardedStep(shard, SC)
            except Exception as e:
                sys.stderr.write("bench: sharded graph capture failed on rank %d (%r)\n" % (rank, e))
                torch.cuda.synchronize()
            # every rank must issue the same collectives: use the graphed step only if ALL ranks captured it
            flag = torch.tensor([1 if gstep is not None else 0], dtype=torch.int32, device=dev if backend == "nccl" else "cpu")
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            if int(flag) == 1:
                step = lambda: gstep()
                mode = "RCCL all-gathers + hipGraph replay of the compute between them"
            elif rank == 0:
                sys.stderr.write("bench: timing eager launches on all ranks\n")
    elif os.environ.get("KCCOT_BENCH_EAGER") == "1":
        step = lambda: loss_step(G, t)
    else:
        # the step as a training loop would run it: forward + backward captured once into a hipGraph
        # (kccotgan_amd/graph.py) and replayed -- the same kernels with the same arguments, one
        # hipGraphLaunch instead of several launches issued from Python
        try:
            from kccotgan_amd.graph import GraphedLossStep
            graphed = GraphedLossStep(t, SC)
            step = lambda: graphed()
            mode = "hipGraph replay of forward+backward"
        except Exception as e:   # capture is an optimisation of the launch path, never a reason to lose the measurement
            sys.stderr.write("bench: graph capture failed (%r); timing eager launches\n" % (e,))
            torch.cuda.synchronize()
            step = lambda: loss_step(G, t)

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    # Untimed replays in front of the W warm-up steps until the card has been busy for ~60 ms: W = 10 steps are 2 ms, not enough
    # for the clocks to come back from the idle state the host-side capture leaves them in, and the timed window (K steps = 4-10 ms)
    # is short enough for that ramp to show as +20 % in one run out of a few (profiles/r4ci6_bench.json: 0.227 ms in the window,
    # 0.193 ms median of the per-step events right behind it, identical kernel durations).  Same step, nothing timed, bounded.
    # (N > 1: the step holds collectives, so every rank must run the SAME number of them: a fixed count there)
    settle = 0
    t_settle = time.perf_counter()
    while (settle < 400 and time.perf_counter() - t_settle < 0.06) if world == 1 else settle < 20:
        for _ in range(10):
            loss, _g = step()
        torch.cuda.synchronize()
        settle += 10
    for _ in range(args.warmup):
        loss, _g = step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss, _g = step()
    barrier()
    el = time.perf_counter() - t0
    if dist is not None:
        tt = torch.tensor([el], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        el = float(tt)
    ms = el / args.steps * 1e3
    # before anything replays the step again: the graphed step returns static buffers that the next replay overwrites
    dumped = dump_outputs(args.dump_outputs, loss, _g, ".rank%d" % rank if world > 1 else "") if args.dump_outputs else None
    if world > 1 and mode.startswith("RCCL"):
        nits, nexec = gstep.nits.tolist(), gstep.nits_executed.tolist()
    elif world > 1:
        from kccotgan_amd import dist as kd
        nits, nexec = kd.last_info["nits"].tolist(), kd.last_info["nits_executed"].tolist()
    elif mode == "eager launches":
        nits = G.last_info["compute_sinkhorn_loss"].tolist()
        nexec = G.last_info["compute_sinkhorn_loss_executed"].tolist()
    else:
        nits, nexec = graphed.nits.tolist(), graphed.nits_executed.tolist()

    out = {
        "metric": "sinkhorn_loss_evals_per_sec", "value": args.steps / el, "unit": "loss-evals/s (fwd+bwd)",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "settle_steps_before_warmup": settle, "ms_per_step": ms,
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": "BASELINE configs[1]: Moving-MNIST shape B=64,T=30,64x64x1, J=8, 100 Sinkhorn iters, "
                               "compute_sinkhorn_loss fwd+bwd", "global_batch": SHAPE["B"],
                   "parallelism": "single GPU" if world == 1 else (
                       ("contraction-sharded x%d: all-to-all into K-slices, all-reduced fp64 Gram sums, replicated Sinkhorn, all-to-all back" % world)
                       if os.environ.get("KCCOT_DIST_PROTOCOL") == "ksplit" else
                       ("batch-sharded x%d: RCCL all-gather of the shards, replicated cost assembly (B <= 64) and Sinkhorn, per-rank gradients" % world)),
                   "sinkhorn_iters": nits, "sinkhorn_iters_executed": nexec, "sinkhorn_exact_shortcut": "off",
                   "launch": mode, "loss": float(loss)},
    }
    if dumped:
        out["dumped_outputs"] = {"dir": os.path.abspath(args.dump_outputs), "arrays": dumped}

    def finish():
        if rank == 0:
            print(json.dumps(out), flush=True)
        if dist is not None:
            dist.barrier()          # rank 0 may have measured the roofline block after the timed region: leave together
            dist.destroy_process_group()

    if not args.full:               # a plain run: the headline is all it measures
        finish()
        return
    # ---- per-step distribution with HIP events (all ranks replay -- the sharded step has collectives; rank 0 reports)
    try:
        reps = max(100, args.steps)
        st = event_stats(step, reps)
        if rank == 0:
            out["event_timing"] = st
    except Exception as e:
        sys.stderr.write("bench: event timing failed: %r\n" % (e,))
    barrier()

    if rank == 0 and world == 1:
      try:
        # the shipped default: exact shortcut on.  Same outputs bit for bit (tests/test_gpu_parity.py::
        # test_sinkhorn_periodic_state_shortcut_is_bit_exact); how much it saves depends on the data.
        kl.set_option("sinkhorn_shortcut", 1)
        from kccotgan_amd.graph import GraphedLossStep

        def timed(fn):
            for _ in range(args.warmup):
                r = fn()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(args.steps):
                r = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t1) / args.steps * 1e3, r

        extra = {}
        for regime, seed in (("near", 0), ("far", 1)):
            _, tr = make_inputs(SHAPE["B"], seed, dev, regime)
            gs = GraphedLossStep(tr, SC)
            ms_g, (l2, _g) = timed(lambda: gs())
            for k in WRT:
                tr[k].requires_grad_(True)
            ms_e, _r = timed(lambda: loss_step(G, tr))
            extra[regime] = {"ms_per_step": ms_g, "ms_per_step_eager_launches": ms_e, "loss": float(l2),
                             "sinkhorn_iters": gs.nits.tolist(), "sinkhorn_iters_executed": gs.nits_executed.tolist()}
        out["with_exact_shortcut"] = extra
        kl.set_option("sinkhorn_shortcut", 0)
        out["eager_launches_ms_per_step"] = timed(lambda: loss_step(G, t))[0]     # shortcut off, like the headline
      except Exception as e:     # auxiliary measurements must not cost the headline line
        sys.stderr.write("bench: auxiliary timings failed: %r\n" % (e,))
        kl.set_option("sinkhorn_shortcut", 0)
    if rank == 0:       # the dominant kernel is the same on every rank at any N (replicated cost assembly at B <= 64)
      try:
        kt, K, C3 = time_cost_kernel(t)
        B, T, J = SHAPE["B"], SHAPE["T"], SHAPE["J"]
        alg_bytes = 2 * B * K * 4 + 16 * B * T * J + 12 * B * B            # read real+fake once
        alg_flops = 4 * B * B * K                                          # xy full + xx, yy triangles (8(d))
        f32_path = kl.get_option("gram_f32") == 1
        t_s = kt["partial"] * 1e-6
        traffic, traffic_source = None, None
        tf = os.path.join(ROOT, "profiles", "hbm_traffic.json")
        if os.path.exists(tf):
            rec = json.load(open(tf))
            traffic = rec.get("gram128_partial_bytes_per_launch")
            traffic_source = rec.get("source", "profiles/hbm_traffic.json (committed rocprofv3 --pmc pass, not measured in this run)")
        committed = traffic
        if world == 1 and not args.no_pmc and not f32_path:
            live, note = live_pmc_traffic()
            if live:
                traffic, traffic_source = live, note
            else:
                traffic_source = "%s [live counter pass skipped: %s]" % (traffic_source, note)
        hbm = alg_bytes / t_s / 1e9
        tfl = alg_flops / t_s / 1e12
        ideal_hbm_us = alg_bytes / (HBM_PEAK_GBS * 1e9) * 1e6
        if f32_path:
            # f32-input MFMA kernel: ideal 12.8 us on the f32 MFMA pipe vs 7.9 us of HBM -> MFMA-bound
            exec_flops = 10 * 2 * 32 * 32 * K
            roof = {"kernel": "gram128_partial<f32 MFMA>", "bound": "mfma", "achieved": tfl,
                    "peak": MFMA_F32_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": tfl / MFMA_F32_PEAK_TFLOPS,
                    "executed_mfma_tflops": exec_flops / t_s / 1e12,
                    "ideal_us": {"hbm": ideal_hbm_us, "f32_mfma": alg_flops / (MFMA_F32_PEAK_TFLOPS * 1e12) * 1e6},
                    "hbm_achieved_GBs": hbm, "hbm_frac": hbm / HBM_PEAK_GBS}
        else:
            # The kernel issues v_mfma_f32_32x32x16_bf16 (exact three-way split, six products): on the pipe it
            # executes on the ideals are 15.1 GFLOP / 2.5 PFLOP/s = 6.0 us (bf16 MFMA) against 62.9 MB / 8 TB/s
            # = 7.9 us (HBM) -> the BINDING bound is HBM, and `frac` is the HBM fraction the north star asks for.
            exec_flops = 6 * 10 * 2 * 32 * 32 * K
            roof = {"kernel": "gram128_partial_x3ws", "bound": "hbm", "achieved": hbm, "peak": HBM_PEAK_GBS,
                    "unit": "GB/s", "frac": hbm / HBM_PEAK_GBS,
                    "ideal_us": {"hbm": ideal_hbm_us, "bf16_mfma_executed": exec_flops / (MFMA_BF16_PEAK_TFLOPS * 1e12) * 1e6,
                                 "f32_mfma_equivalent": alg_flops / (MFMA_F32_PEAK_TFLOPS * 1e12) * 1e6},
                    "executed_bf16_mfma_tflops": exec_flops / t_s / 1e12,
                    "bf16_mfma_frac": exec_flops / t_s / 1e12 / MFMA_BF16_PEAK_TFLOPS,
                    "bf16_mfma_frac_of_measured_sustained": exec_flops / t_s / 1e12 / 1750.0,
                    "measured_sustained_note": "v_mfma_f32_32x32x16_bf16 sustains 2.48 PFLOP/s with constant operands and 1.72-1.82 "
                                               "with data-like operand bits on this part (tools/micro/mfma_feed.hip, "
                                               "profiles/r02r_micro_mfma_feed.txt); informational, `peak` stays the guide's figure",
                    "f32_mfma_equivalent": {"achieved_tflops": tfl, "peak": MFMA_F32_PEAK_TFLOPS,
                                            "frac": tfl / MFMA_F32_PEAK_TFLOPS,
                                            "note": "algorithmic fp32 flops / time against the f32-input MFMA peak; "
                                                    "applies to the option gram_f32 = 1, secondary here"}}
        roof.update({"traffic": traffic, "traffic_source": traffic_source,
                     "traffic_over_algorithmic": (traffic / alg_bytes) if traffic else None,
                     "traffic_committed_pass": committed,
                     "kernel_us": kt["partial"], "cost_stage_us": kt["stage"],
                     # the same algorithmic bytes over the WHOLE cost stage (Gram partials + fp64 reduction + finalize: three
                     # launches), for whoever reads the step rather than the kernel
                     "cost_stage_frac": alg_bytes / (kt["stage"] * 1e-6) / 1e9 / HBM_PEAK_GBS,
                     "algorithmic_bytes": alg_bytes, "algorithmic_flops": alg_flops,
                     "timing": "200 launches between two events on the launch stream"})
        out["roofline"] = roof
        out["sinkhorn"] = time_sinkhorn(C3)
      except Exception as e:
        sys.stderr.write("bench: roofline block failed: %r\n" % (e,))
    # ---- the other BASELINE configs
    if not args.no_configs:
        cfgs = None
        try:
            if world == 1:
                cfgs = single_gpu_configs(G, dev)
            else:
                # EVERY BASELINE config whose batch the ranks divide (not only at the GPU count the config names), plus the
                # weak-scaling line of the headline shape: per-rank batch 64 -> global batch 64 N at configs[1]'s frames
                cfgs = {}
                rehearsal = backend != "nccl"      # host-staged collectives: fewer steps, and no multi-GB shapes
                nst = 2 if rehearsal else 5
                for name, (B, H, T, W, C, L, ngpu) in OTHER_CONFIGS.items():
                    if rehearsal and 4.0 * B * H * T * W * C > 2e9:
                        continue
                    if B % world == 0:                       # every rank takes the same branch: world is global
                        cfgs[name] = sharded_shape(name, B, H, T, W, C, L, rank, world, dev, dist, barrier, steps=nst)
                        cfgs[name]["gpus_named_by_config"] = ngpu
                        cfgs[name]["scaling"] = "strong (the config's global batch on this many GPUs)"
                wk = sharded_shape("weak", SHAPE["B"] * world, SHAPE["H"], SHAPE["T"], SHAPE["W"], SHAPE["C"], 100, rank, world,
                                   dev, dist, barrier, steps=nst)
                wk["scaling"] = "weak (per-rank batch 64 at configs[1]'s frames: the loss of the GLOBAL batch 64 N, what the data-parallel trainer evaluates)"
                cfgs["configs[1] frames, per-rank batch 64"] = wk
        except Exception as e:
            sys.stderr.write("bench: configs block failed on rank %d: %r\n" % (rank, e))
        if rank == 0 and cfgs:
            out["configs"] = cfgs
            out["box_probe"] = box_probe(dev)
        if rank == 0 and world == 1:
            try:
                out["kernel_smoothing"] = time_smoothing(dev)
                # configs[1]: the traffic ratios re-measured in this run (the other shapes keep the committed passes' figures)
                if not args.no_pmc and "configs[1]" in out["kernel_smoothing"]:
                    rec = out["kernel_smoothing"]["configs[1]"]
                    torch.cuda.empty_cache()
                    live, note = live_smoothing_traffic()
                    n_el = float(np.prod(rec["shape_BHTWC"]))
                    if live:
                        for key in ("temporal", "conv3d"):
                            for direction, alg in (("fwd", 8.0 * n_el), ("bwd", 12.0 * n_el)):
                                rec[key][direction + "_traffic_over_algorithmic_committed_pass"] = rec[key].get(direction + "_traffic_over_algorithmic")
                                rec[key][direction + "_traffic_bytes"] = live["%s_%s" % (key, direction)]
                                rec[key][direction + "_traffic_over_algorithmic"] = live["%s_%s" % (key, direction)] / alg
                        rec["traffic_source"] = note
                    else:
                        rec["traffic_source"] = "profiles/smooth_traffic.json (committed counter passes) [live counter pass skipped: %s]" % note
            except Exception as e:
                sys.stderr.write("bench: kernel_smoothing block failed: %r\n" % (e,))
    if world > 1 and not args.no_train:
        # the half of BASELINE.json's metric that CAN scale: data-parallel train-steps/s (every rank spawns its child)
        try:
            torch.cuda.empty_cache()
            barrier()
            r = dp_train_children(rank, world, local_rank, backend)
            if rank == 0:
                out["train_steps_per_sec_data_parallel"] = r
        except Exception as e:
            sys.stderr.write("bench: data-parallel train block failed on rank %d: %r\n" % (rank, e))
        barrier()
    if rank == 0 and world == 1:
      try:
        if not args.no_train:
            torch.cuda.empty_cache()
            out["train_steps_per_sec"] = train_steps_child()
      except Exception as e:
        sys.stderr.write("bench: train_steps_per_sec failed: %r\n" % (e,))
      try:
        if not args.no_cpu_baseline:      # the CPU baseline is timed at N = 1 only
            out["cpu_baseline"] = cpu_baseline(inp)
            out["cpu_baseline"]["gpu_over_cpu"] = out["value"] / out["cpu_baseline"]["value"]
      except Exception as e:
        sys.stderr.write("bench: cpu_baseline failed: %r\n" % (e,))
    finish()


if __name__ == "__main__":
    main()
