#!/usr/bin/env python3
"""Where does a Sinkhorn half-step spend its cycles?  Loads the DIAGNOSTIC twin library
(libkccot_diag.so, built with -DKCCOT_DIAG: s_memtime stamps around the phases of iteration 50)
and prints per-wave cycle counts between stamps.  Never used by the product path.  KCCOT_LIB_PATH names another
build of the twin (stamps of two trees side by side).
usage: diag_sinkhorn.py [n [golden file]]      the forward kernel (sinkhorn_fwd_reg)
       diag_sinkhorn.py fused [n [golden file]] the fused solve + sweep, one-role and role-split: one sweep iteration
                                               (pass A, pass B) and one forward iteration, mean over waves and launches"""
import ctypes, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# KCCOT_LIB_PATH: another build of the diagnostic twin (A/B stamps of two trees), as kccotgan_amd/_lib.py reads it
lib = ctypes.CDLL(os.environ.get("KCCOT_LIB_PATH") or os.path.join(ROOT, "kccotgan_amd", "csrc", "libkccot_diag.so"))
vp, ci, cf, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
lib.kccot_sinkhorn_fwd_f32.argtypes = [vp, ci, ci, cf, ci, ci, cf, ci, vp, vp, vp, vp, vp, vp, sz, vp]
FUSED = len(sys.argv) > 1 and sys.argv[1] == "fused"
if FUSED:
    del sys.argv[1]
n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
g = np.load(os.path.join(ROOT, "tests", "golden", sys.argv[2] if len(sys.argv) > 2 else "cfg2_s0_near.npz"))
C = torch.from_numpy(np.stack([g["C_xy"], g["C_xx"], g["C_yy"]])).cuda()[:, :n, :n].contiguous()
L = 100
SLOTS = 32          # KCCOT_DIAG_SLOTS of sinkhorn.hip


def fused_stamps(roles, launches=20):
    """Stamps of sweep iteration 50 and forward iteration 50 of the fused kernel, [launch, wave, slot] of problem 0.
    Slots: 0 pass A starts / 1 plan_b evaluated (one role: after the gv read, the wave that is on the chain; roles: the
    column waves; on the row waves slot 1 = the gradients have arrived) / 2 DPP sum done / 3 gu written / 4 after the
    barrier / 5 plan_a evaluated (roles: row waves; column waves: gradients arrived) / 6 DPP sum / 7 gv written / 8 after
    the closing barrier; 9 / 10: a forward iteration's start and end; 11 / 12 and 13 / 14: around the whole forward loop and
    the whole sweep loop (one stamp pair per 100 iterations: the stamps of iteration 50 are the only disturbance inside).
    16: kernel entry (16 -> 11 the prologue); between the loops (12 -> 13): 17 the cost's partial sums are formed, 20 the
    final-cost adjoint is written, 13 behind the barrier that opens the sweep; behind the sweep (14 -> 22): 21 behind the
    barrier of the dC transpose, 19 the cost hand-off has returned (the publishing wave), 22 the wave's stores have completed
    (kernel exit).  The role kernel's forward iteration 50: 9 the iteration starts (the row role leaves the barrier that closed
    iteration 49), 27 behind the iteration's first barrier, 10 behind its second; in the role that is on the chain between two of
    these, 23 the other role's duals have arrived (only in builds that form self - c2 off the chain, KCCOT_FWD_TRIM & 8), 24 the
    line's max is known, 25 its sum, 26 the new dual is written.  Every stamp costs about 40 cycles itself."""
    lib.kccot_sinkhorn_divergence_fused_f32.argtypes = [vp, ci, cf, ci, ci, cf, vp, vp, vp, vp, vp, vp]
    lib.kccot_set_option.argtypes = [ctypes.c_char_p, ci]
    lib.kccot_diag_fused_stamps.argtypes = [vp]
    assert lib.kccot_set_option(b"sinkhorn_shortcut", 0) == 0 and lib.kccot_set_option(b"sinkhorn_fused_roles", roles) == 0
    cost = torch.empty(3, device="cuda"); nits = torch.empty(6, dtype=torch.int32, device="cuda")
    loss = torch.empty(1, device="cuda"); ticket = torch.zeros(1, dtype=torch.int32, device="cuda"); dC = torch.empty_like(C)
    diag = torch.zeros(3 * 16 * SLOTS, dtype=torch.int64, device="cuda")
    lib.kccot_diag_fused_stamps(diag.data_ptr())
    out = []
    for rep in range(launches + 3):
        diag.zero_()
        assert lib.kccot_sinkhorn_divergence_fused_f32(C.data_ptr(), n, 1.0, L, 100, 1e-2, cost.data_ptr(), nits.data_ptr(),
                                                       loss.data_ptr(), ticket.data_ptr(), dC.data_ptr(), None) == 0
        torch.cuda.synchronize()
        if rep >= 3:
            out.append(diag.cpu().numpy().reshape(3, 16, SLOTS)[0].copy())
    lib.kccot_diag_fused_stamps(None)
    return np.stack(out), nits.tolist()


if FUSED:
    for roles in (0, 1):
        d, its = fused_stamps(roles)
        nw = int((d[0, :, 0] != 0).sum())
        groups = [("all waves", range(nw))] if not roles else [("row waves", range(nw // 2)), ("column waves", range(nw // 2, nw))]
        print("sinkhorn_fused_roles=%d  n=%d  waves=%d  nits %s" % (roles, n, nw, its))
        for name, ws in groups:
            ws = list(ws)
            seg = lambda a, b: float(np.mean(d[:, ws, b] - d[:, ws, a])) if (d[:, ws, a] != 0).all() and (d[:, ws, b] != 0).all() else float("nan")
            print("  %-12s pass A: to plan/gradients %.0f  to DPP sum %.0f  to write %.0f  to barrier exit %.0f | pass B: %.0f  %.0f  %.0f  %.0f"
                  " | sweep iteration %.0f cycles | forward iteration %.0f cycles | whole forward loop %.0f, whole sweep loop %.0f cycles" % (
                      name, seg(0, 1), seg(1, 2), seg(2, 3), seg(0, 4), seg(4, 5), seg(5, 6), seg(6, 7), seg(4, 8), seg(0, 8), seg(9, 10),
                      seg(11, 12), seg(13, 14)))
            # the serial sections around the two loops
            print("  %-12s prologue %.0f | forward %.0f | between the loops %.0f (cost sums %.0f, adjoint written %.0f, barrier %.0f) | sweep %.0f"
                  " | behind the sweep %.0f (to the transpose barrier's exit %.0f, stores completed %.0f) | entry to exit %.0f cycles" % (
                      name, seg(16, 11), seg(11, 12), seg(12, 13), seg(12, 17), seg(17, 20), seg(20, 13), seg(13, 14), seg(14, 22),
                      seg(14, 21), seg(21, 22), seg(16, 22)))
        if roles:
            # forward iteration 50 by role: the half-step of the role that is on the chain, and what the other role sees
            for name, ws, a in (("row waves", list(range(nw // 2)), 9), ("column waves", list(range(nw // 2, nw)), 27)):
                seg = lambda x, y: float(np.mean(d[:, ws, y] - d[:, ws, x])) if (d[:, ws, x] != 0).all() and (d[:, ws, y] != 0).all() else float("nan")
                print("  %-12s forward half-step: barrier exit -> duals read %.0f -> max known %.0f (from the barrier exit) -> sum known %.0f -> "
                      "dual written %.0f -> next barrier exit %.0f | the other role's half-step (barrier to barrier) %.0f cycles" % (
                          name, seg(a, 23), seg(a, 24), seg(24, 25), seg(25, 26), seg(26, 27 if a == 9 else 10),
                          seg(27, 10) if a == 9 else seg(9, 27)))
        t0, t1 = d[:, :nw, 16].min(axis=1), d[:, :nw, 22].max(axis=1)
        seg_all = lambda a, b: float(np.mean(d[:, :nw, b].max(axis=1) - d[:, :nw, a].min(axis=1)))
        print("  workgroup    first entry to last exit %.0f cycles: prologue %.0f, forward %.0f, between the loops %.0f, sweep %.0f, behind the sweep %.0f"
              % (float(np.mean(t1 - t0)), seg_all(16, 11), float(np.mean(d[:, :nw, 12].max(axis=1) - d[:, :nw, 11].max(axis=1))),
                 float(np.mean(d[:, :nw, 13].max(axis=1) - d[:, :nw, 12].max(axis=1))),
                 float(np.mean(d[:, :nw, 14].max(axis=1) - d[:, :nw, 13].max(axis=1))),
                 float(np.mean(d[:, :nw, 22].max(axis=1) - d[:, :nw, 14].max(axis=1)))))
        at = lambda s: float(np.mean(d[:, :nw, s].max(axis=1) - t0))
        print("  workgroup    cycles after the first entry: forward loop left %.0f, sweep loop entered %.0f, left %.0f, cost hand-off returned %.0f, last exit %.0f"
              % (at(12), at(13), at(14), at(19), at(22)))
    sys.exit(0)

uh = torch.empty(3, L, n, device="cuda"); vh = torch.empty(3, L, n, device="cuda")
cost = torch.empty(3, device="cuda"); nits = torch.empty(6, dtype=torch.int32, device="cuda")
diag = torch.zeros(3 * 16 * SLOTS, dtype=torch.int64, device="cuda")
for rep in range(3):
    rc = lib.kccot_sinkhorn_fwd_f32(C.data_ptr(), 3, n, 1.0, L, 100, 1e-2, 0, uh.data_ptr(), vh.data_ptr(), cost.data_ptr(),
                                    nits.data_ptr(), None, diag.data_ptr(), diag.numel() * 8, None)
    assert rc == 0
torch.cuda.synchronize()
d = diag.cpu().numpy().reshape(3, 16, SLOTS)
names = ["row half-step", "store u", "barrier 1", "col half-step", "store v", "barrier 2", "detect"]
print("nits", nits.tolist())
print("cost", cost.tolist())
for w in range(16):
    st = d[0, w, :8]
    if st[0] == 0: continue
    print("wave %2d: " % w + "  ".join("%s %d" % (names[k], st[k + 1] - st[k]) for k in range(7 if st[7] else 6)) + "  | total %d" % (st[6] - st[0]))
