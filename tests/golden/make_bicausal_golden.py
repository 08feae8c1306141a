#!/usr/bin/env python3
"""Generate tests/golden/bicausal_*.npz by EXECUTING the reference's own gan_utils.py (as make_golden.py does: the NumPy
stand-in ``oracle/refshim`` first on sys.path, ``gan_utils`` imported verbatim from the reference directory).

    python tests/golden/make_bicausal_golden.py [--ref /root/reference] [--only NAME ...]

The reference has no bi-causal loss; each of its three terms is ``compute_sinkhorn(a, b, hy, Mx, sc, hx=hx, My=My,
bi_causal=True)`` (gan_utils.py:124) with the operands and (hy, Mx) of compute_sinkhorn_loss's three calls
(gan_utils.py:221-223) and the (hx, My) slots filled as in bicausal_cases.TERMS; the cost matrix of each term is the
reference's ``bi_causal_modified_cost``.  The one line not written by the reference is the combination
loss = 2 w_xy - w_xx - w_yy.  Stored per case, in fp32 and (suffix _f64) fp64: w_xy, w_xx, w_yy, nits_xy, nits_xx,
nits_yy (executed iterations, via the stand-in's lse_calls counter), C_xy, C_xx, C_yy, loss; plus the checksum of the
regenerated inputs.
"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bicausal_cases  # noqa: E402
import cases  # noqa: E402
from make_golden import counted, flatten, load_reference, memoise_cost_xy  # noqa: E402


def run_case(tf, gu, shape, seed, regime, eps, L, dtype):
    sfx = "" if dtype == np.float32 else "_f64"
    tf.set_float(dtype)
    restore = memoise_cost_xy(gu) if shape == "cfg2" else (lambda: None)
    try:
        inp = cases.gen_inputs(shape, seed, regime)
        v = {k: inp[k].astype(dtype) for k in ("real", "fake", "h_fake", "m_real", "h_real", "m_fake")}
        for k in ("real", "fake"):
            v[k] = flatten(v[k])
        sc = dtype(cases.SC)
        out = {}
        for tag, a, b, hy, mx, hx, my in bicausal_cases.TERMS:
            val, n = counted(tf, gu.compute_sinkhorn, v[a], v[b], v[hy], v[mx], sc, hx=v[hx], My=v[my],
                             epsilon=dtype(eps), L=L, bi_causal=True)
            out["w_" + tag], out["nits_" + tag] = val, n
            out["C_" + tag] = gu.bi_causal_modified_cost(v[a], v[b], v[hy], v[mx], v[hx], v[my], sc)
        out["loss"] = 2 * out["w_xy"] - out["w_xx"] - out["w_yy"]
        res = {k + sfx: np.asarray(x) for k, x in out.items()}
        if dtype == np.float32:
            res["checksum"] = cases.checksum(inp)
        return res
    finally:
        restore()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--only", nargs="*", default=None)
    args = ap.parse_args()
    tf, gu = load_reference(args.ref)
    for shape, seed, regime, eps, L in bicausal_cases.CASES:
        name = bicausal_cases.case_name(shape, seed, regime, eps, L)
        if args.only and name not in args.only and shape not in args.only:
            continue
        t0 = time.time()
        res = {}
        for dtype in (np.float32, np.float64):
            res.update(run_case(tf, gu, shape, seed, regime, eps, L, dtype))
        tf.set_float(np.float32)
        for k, x in res.items():
            if not k.endswith("_f64") and k != "checksum" and not k.startswith("nits"):
                assert x.dtype == np.float32, (k, x.dtype)
        np.savez(os.path.join(HERE, name + ".npz"), **res)
        print("%-36s loss=%.6f (f64 %.9f) nits=%s  %.1fs" % (
            name, res["loss"], res["loss_f64"], [int(res["nits_" + t[0]]) for t in bicausal_cases.TERMS],
            time.time() - t0), flush=True)


if __name__ == "__main__":
    main()
