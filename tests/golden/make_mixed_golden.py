#!/usr/bin/env python3
"""Generate tests/golden/mixed_*.npz by EXECUTING the reference's own gan_utils.py (as make_golden.py does: the NumPy
stand-in ``oracle/refshim`` first on sys.path, ``gan_utils`` imported verbatim from the reference directory).

    python tests/golden/make_mixed_golden.py [--ref /root/reference] [--only NAME ...]

The reference has no mixed loss; each of its four terms is ``compute_sinkhorn(a, b, h, M, sc)`` (gan_utils.py:124,
bi_causal = False) called exactly as compute_sinkhorn_loss calls it, and the cost matrix of each term is the
reference's ``modified_cost(a, b, h, M, sc)``.  The one line not written by the reference is the combination
loss = (W1 + W2) - W3 - W4.  Stored per case, in fp32 and (suffix _f64) fp64: w1..w4, nits1..nits4 (executed
iterations, via the stand-in's lse_calls counter), C1..C4, loss; plus the checksum of the regenerated inputs.
"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cases  # noqa: E402
import mixed_cases  # noqa: E402
from make_golden import counted, flatten, load_reference, memoise_cost_xy  # noqa: E402


def run_case(tf, gu, shape, seed, regime, dtype):
    sfx = "" if dtype == np.float32 else "_f64"
    tf.set_float(dtype)
    restore = memoise_cost_xy(gu) if shape == "cfg2" else (lambda: None)
    try:
        inp = mixed_cases.gen_inputs(shape, seed, regime)
        v = {k: inp[k].astype(dtype) for k in mixed_cases.KEYS}
        for k in ("real", "fake", "real_p", "fake_p"):
            v[k] = flatten(v[k])
        sc = dtype(cases.SC)
        out = {}
        w = []
        for t, (a, b, h, m, _sign) in enumerate(mixed_cases.TERMS, 1):
            val, n = counted(tf, gu.compute_sinkhorn, v[a], v[b], v[h], v[m], sc)
            out["w%d" % t], out["nits%d" % t] = val, n
            out["C%d" % t] = gu.modified_cost(v[a], v[b], v[h], v[m], sc)
            w.append(val)
        out["loss"] = (w[0] + w[1]) - w[2] - w[3]
        res = {k + sfx: np.asarray(x) for k, x in out.items()}
        if dtype == np.float32:
            res["checksum"] = mixed_cases.checksum(inp)
        return res
    finally:
        restore()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--only", nargs="*", default=None)
    args = ap.parse_args()
    tf, gu = load_reference(args.ref)
    for shape, seed, regime in mixed_cases.CASES:
        name = mixed_cases.case_name(shape, seed, regime)
        if args.only and name not in args.only and shape not in args.only:
            continue
        t0 = time.time()
        res = {}
        for dtype in (np.float32, np.float64):
            res.update(run_case(tf, gu, shape, seed, regime, dtype))
        tf.set_float(np.float32)
        for k, x in res.items():
            if not k.endswith("_f64") and k != "checksum" and not k.startswith("nits"):
                assert x.dtype == np.float32, (k, x.dtype)
        np.savez(os.path.join(HERE, name + ".npz"), **res)
        print("%-26s loss=%.6f (f64 %.9f) nits=%s  %.1fs" % (
            name, res["loss"], res["loss_f64"], [int(res["nits%d" % t]) for t in range(1, 5)], time.time() - t0), flush=True)


if __name__ == "__main__":
    main()
