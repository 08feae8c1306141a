"""CPU tier of the early-stopped Sinkhorn solves: the float64 reference, the inputs and the conditions on those inputs that
tests/test_gpu_sinkhorn_early_stop.py holds every kernel family to.

Past Lmin iterations the loop ends as soon as sum|u - u_prev| < thresh, and every reverse sweep then starts from the count the
forward wrote, in a history that was sized for L.  stopped_sweep is the tape-free loop and reverse sweep of
tests/test_weight_grad_cpu.py:sweep with Lmin, thresh and the stop mode as parameters; it is proved here against sweep, against
the oracle's loop in both stop modes and against float64 autograd through the stopped loop.

The inputs (stop_problems) are chosen so that the count is a property of the inputs and not of rounding.  For every problem,
with k the float64 count and errs[t] the float64 sum|u - u_prev| of iteration t + 1:

    Lmin < k < L - 1                                         the stop rule, not a bound of the loop, ends the solve
    errs[k-2] - thresh >= G  and  thresh - errs[k-1] >= G    G = max(0.2 thresh, 16 n max|u| 2^-24)
    the float32 run of stopped_sweep stops at k as well
    at least two of the three problems of a launch have different k.

16 n max|u| 2^-24 bounds the float32 rounding of n differences of duals of size max|u| (each dual carries a few ulps); at
n = 1024 and |u| ~ 3 it is about 0.3 thresh.  The picker scans seeds and scales for thresh = 1e-2, the production value.  With
unequal weights spanning two orders of magnitude max|u| is about 7 and at n = 1024 G exceeds 1e-2 itself: that launch alone
places its thresh at sqrt(errs[k-2] errs[k-1]) of a chosen k (stop_thresh); the file prints which launches do (-s).
"""
import functools

import pytest
import torch

import test_weight_grad_cpu as WG
import test_weighted_sinkhorn_cpu as W
from oracle import gan_utils_torch as ot
from test_weighted_sinkhorn_cpu import F64

F32 = torch.float32
THRESH = W.THRESH
STOP_EPS, STOP_L, STOP_LMIN = 0.5, 40, 3
SEEDS = 4
SCALES = (1.0, 0.8, 1.25, 0.5, 0.6, 0.42, 1.5, 0.7, 0.35)          # problem p of a launch scans them from the 3 p-th on
REG_SIZES = (7, 24, 48, 64, 128)
STREAM_SIZES = (131, 132, 256, 260, 516, 1024)
SIZES = REG_SIZES + STREAM_SIZES
COND_SIZES = (48, 132, 260)


# ================================================================ the reference
def stopped_loop(C, a, b, eps, L, Lmin=W.LMIN, thresh=THRESH, stop_on_index=False, dtype=F64):
    """(U, V, errs, nits): the weighted loop with its whole history, U[t] / V[t] the duals after t iterations, errs[t - 1] the
    sum|u - u_prev| of iteration t.  COUNT mode stops once err < thresh and nits >= Lmin, INDEX mode once err < thresh and the
    loop index nits - 1 >= Lmin.  Every operation in `dtype`."""
    C, a, b = C.to(dtype), a.to(dtype), b.to(dtype)
    la, lb = torch.log(a), torch.log(b)
    U, V, errs = [torch.zeros_like(a)], [torch.zeros_like(b)], []
    nits = 0
    for i in range(int(L)):
        u = eps * (la - torch.logsumexp((-C + U[-1][:, None] + V[-1][None, :]) / eps, dim=1)) + U[-1]
        v = eps * (lb - torch.logsumexp((-C + u[:, None] + V[-1][None, :]) / eps, dim=0)) + V[-1]
        errs.append(float((u - U[-1]).abs().sum()))
        U.append(u)
        V.append(v)
        nits += 1
        if thresh > errs[-1] and ((i >= Lmin) if stop_on_index else (nits >= Lmin)):
            break
    return U, V, errs, nits


def stopped_sweep(C, a, b, eps, L, Lmin=W.LMIN, thresh=THRESH, stop_on_index=False, g=1.0, dtype=F64):
    """(cost, nits, dC, da, db, U[nits], V[nits], errs) of g W(C; a, b): stopped_loop, then the reverse sweep from nits with the
    two sums of tests/test_weight_grad_cpu.py (the adjoint of v_0 = 0 is a constant's and is not added)."""
    U, V, errs, nits = stopped_loop(C, a, b, eps, L, Lmin, thresh, stop_on_index, dtype)
    C, a, b = C.to(dtype), a.to(dtype), b.to(dtype)
    la, lb = torch.log(a), torch.log(b)
    pi = torch.exp((-C + U[nits][:, None] + V[nits][None, :]) / eps)
    cost = (pi * C).sum()
    dC = g * pi * (1.0 - C / eps)
    gu = g * (pi * C).sum(1) / eps
    gv = g * (pi * C).sum(0) / eps
    sa = torch.zeros_like(a)
    sb = gv.clone() if nits > 0 else torch.zeros_like(b)
    for t in range(nits, 0, -1):
        Qt = torch.exp((-C + U[t][:, None] + (V[t] - eps * lb)[None, :]) / eps)          # column sums 1: dv_t/du_t = -Qt
        w = Qt * gv[None, :]
        dC = dC + w
        gu = (gu if t == nits else torch.zeros_like(gu)) - w.sum(1)
        sa = sa + gu
        Pt = torch.exp((-C + (U[t] - eps * la)[:, None] + V[t - 1][None, :]) / eps)      # row sums 1: du_t/dv_{t-1} = -Pt
        w = Pt * gu[:, None]
        dC = dC + w
        gv = -w.sum(0)
        if t > 1:
            sb = sb + gv
    return cost, nits, dC, eps * sa / a, eps * sb / b, U[nits], V[nits], errs


def differentiable_stopped_cost(C, a, b, eps, k):
    """The cost after exactly k iterations, with a tape: what autograd sees of a loop that stopped at k."""
    la, lb = torch.log(a), torch.log(b)
    u, v = torch.zeros_like(a), torch.zeros_like(b)
    for _ in range(k):
        u = eps * (la - torch.logsumexp((-C + u[:, None] + v[None, :]) / eps, dim=1)) + u
        v = eps * (lb - torch.logsumexp((-C + u[:, None] + v[None, :]) / eps, dim=0)) + v
    return (torch.exp((-C + u[:, None] + v[None, :]) / eps) * C).sum()


# ================================================================ the conditions
def margin(n, U, thresh=THRESH):
    umax = max(float(u.abs().max()) for u in U)
    return max(0.2 * thresh, 16.0 * n * umax * 2.0 ** -24)


def stop_count(C, a, b, eps, L, Lmin, thresh=THRESH):
    """(k, ok, figures): the float64 count and whether the problem meets the per-problem conditions of the docstring."""
    n = C.shape[0]
    U, _, errs, k = stopped_loop(C, a, b, eps, L, Lmin, thresh)
    if not Lmin < k < L - 1:
        return k, False, (k,)
    G = margin(n, U, thresh)
    ok = errs[k - 2] - thresh >= G and thresh - errs[k - 1] >= G
    k32 = stopped_loop(C, a.float(), b.float(), eps, L, Lmin, thresh, dtype=F32)[3] if ok else -1          # not run for nothing
    ok = ok and k32 == k
    return k, ok, (k, errs[k - 2] / thresh, errs[k - 1] / thresh, G / thresh, k32)


def uniform(n):
    return torch.full((n,), 1.0 / n, dtype=F32)


def cond_weights(n, Q=2):
    """The Q weight rows of test_gpu_conditional_sinkhorn.problem(n): random_weights(n, 3000 + 10 n + q), float32."""
    return torch.stack([W.random_weights(n, 3000 + 10 * n + q) for q in range(Q)]).float()


@functools.lru_cache(maxsize=None)
def stop_problems(n):
    """(C [3,n,n] float32, a, b [3,n] float32, (eps, L, Lmin)): small_cost matrices scaled so that the three problems of a
    launch converge at different speeds, random_weights marginals (the device reads these float32 values).  Each matrix is the
    first (seed, scale) of its scan at which the conditions hold at thresh = 1e-2 with uniform weights, with (a[p], b[p]) and,
    at the sizes of the conditional launch, with each of its weight rows for both marginals; the third is also the first that
    leaves two different counts in the launch under each of those marginals.  Where no matrix meets them with weights (n >= 516:
    small weights make max|u| about 7, and G exceeds 1e-2 / 2) the scan asks for the uniform pair alone, and the weighted
    launch places its thresh (stop_thresh)."""
    eps, L, Lmin = STOP_EPS, STOP_L, STOP_LMIN
    a = torch.stack([W.random_weights(n, 1000 + 10 * n + p) for p in range(3)]).float()
    b = torch.stack([W.random_weights(n, 2000 + 10 * n + p) for p in range(3)]).float()
    cw = cond_weights(n) if n in COND_SIZES else []

    def candidates(p, weighted):
        pairs = [(uniform(n), uniform(n))] + ([(a[p], b[p])] + [(w, w) for w in cw] if weighted else [])
        for seed in range(SEEDS):
            base = W.small_cost(n, 100 * n + 10 * seed + p).double()
            for i in range(len(SCALES)):
                C = (SCALES[(3 * p + i) % len(SCALES)] * base).float()
                got = []
                for wa, wb in pairs:
                    got.append(stop_count(C, wa, wb, eps, L, Lmin))
                    if not got[-1][1]:
                        break
                else:
                    yield C, tuple(k for k, _, _ in got)

    for weighted in (True, False):
        first = [next(candidates(p, weighted), None) for p in (0, 1)]
        if None in first:
            continue
        (C0, k0), (C1, k1) = first
        for C2, k2 in candidates(2, weighted):
            ks = list(zip(k0, k1, k2))          # per pair of marginals; the conditional launch holds all its weight rows
            if all(len(set(c)) >= 2 for c in ks[:2]) and (not ks[2:] or len(set(sum(ks[2:], ()))) >= 2):
                return torch.stack([C0, C1, C2]), a, b, (eps, L, Lmin)
    raise AssertionError("no (seed, scale) meets the conditions at n = %d with thresh = %g" % (n, THRESH))


@functools.lru_cache(maxsize=None)
def stop_thresh(n, kind):
    """The thresh of the launch `kind` ('uniform', 'ab', 'cond') at size n: 1e-2 where every problem of the launch meets the
    conditions there; otherwise the first sqrt(errs[k-2] errs[k-1]) of its first problem, k = Lmin + 2 .., at which all of them
    do and two counts differ."""
    C, _, _, (eps, L, Lmin) = stop_problems(n)
    if kind == "cond":
        w = cond_weights(n)
        probs = [(C[k], w[q], w[q]) for q in range(len(w)) for k in range(3)]
    else:
        wa, wb = weights_of(n, kind)
        probs = [(C[p], wa[p], wb[p]) for p in range(3)]
    errs = stopped_loop(*probs[0], eps, L, L, THRESH)[2]
    for thresh in [THRESH] + [(errs[k - 2] * errs[k - 1]) ** 0.5 for k in range(Lmin + 2, L - 1)]:
        got = [stop_count(Cp, ap, bp, eps, L, Lmin, thresh) for Cp, ap, bp in probs]
        if all(ok for _, ok, _ in got) and len({k for k, _, _ in got}) >= 2:
            return thresh
    raise AssertionError("no thresh meets the conditions at n = %d (%s)" % (n, kind))


def weights_of(n, kind):
    """The marginals of a launch: 'uniform' (what the unweighted kernels assume), 'ab' (unequal row and column weights)."""
    _, a, b, _ = stop_problems(n)
    return (torch.stack([uniform(n)] * 3),) * 2 if kind == "uniform" else (a, b)


def references(n, kind, gcost=(1.0, -0.5, 2.0), Lmin=STOP_LMIN, L=STOP_L, stop_on_index=False, dtype=F64):
    """stopped_sweep of the three problems of stop_problems(n) in `dtype`: a tuple of its eight results, one list each.
    Computed once per set of arguments; nobody writes to what it returns."""
    return _references(n, kind, tuple(gcost), int(Lmin), int(L), bool(stop_on_index), dtype)


@functools.lru_cache(maxsize=None)
def _references(n, kind, gcost, Lmin, L, stop_on_index, dtype):
    C, _, _, (eps, _, _) = stop_problems(n)
    a, b = weights_of(n, kind)
    r = [stopped_sweep(C[p], a[p], b[p], eps, L, Lmin, stop_thresh(n, kind), stop_on_index, gcost[p], dtype) for p in range(3)]
    return tuple([x[i] for x in r] for i in range(8))


@functools.lru_cache(maxsize=None)
def cond_problem(n, Q=2):
    """The conditional launch: the shared C3 of stop_problems(n) and the weight rows cond_weights(n), each both marginals of its
    three problems."""
    C3, _, _, setting = stop_problems(n)
    return C3, cond_weights(n, Q), setting


FUSED_SIZES = (24, 48)


@functools.lru_cache(maxsize=None)
def fused_problems(n):
    """Cmix [4,n,n] of the four-problem fused launch: the matrices of stop_problems(n) and the first of their transposes that
    meets the conditions with uniform weights (another problem: rows and columns change roles)."""
    C, _, _, (eps, L, Lmin) = stop_problems(n)
    for p in range(3):
        Ct = C[p].t().contiguous()
        if stop_count(Ct, uniform(n), uniform(n), eps, L, Lmin)[1]:
            return torch.cat([C, Ct[None]])
    raise AssertionError("no transpose meets the conditions at n = %d" % n)


@functools.lru_cache(maxsize=None)
def fused_references(n, gcost, dtype=F64):
    """stopped_sweep of the problems of fused_problems(n)[:len(gcost)] with uniform weights, g = gcost[p]."""
    C = fused_problems(n)
    eps, L, Lmin = STOP_EPS, STOP_L, STOP_LMIN
    return [stopped_sweep(C[p], uniform(n), uniform(n), eps, L, Lmin, THRESH, False, gcost[p], dtype) for p in range(len(gcost))]


API_SHAPE = (132, 2, 4, 4, 1, 2)          # B, T, H, W, C, J: small frames
API_EPS, API_L = 1.0, 130
API_FEATS = ("h_fake", "m_real", "h_real", "m_fake")


@functools.lru_cache(maxsize=None)
def api_inputs():
    """float32 inputs of the public-API case: compute_sinkhorn_loss(..., honor_eps_l=True) at B = 132, eps = 1, L = 130."""
    B, T, H, Wd, Cc, J = API_SHAPE
    g = torch.Generator().manual_seed(132)
    t = {k: torch.rand(B, H, T, Wd, Cc, generator=g) for k in ("real", "fake")}
    t.update({k: torch.rand(B, T, J, generator=g) for k in API_FEATS})
    return t


def api_costs(d):
    """The three cost matrices of compute_sinkhorn_loss on the tensors d (any dtype), as the oracle forms them."""
    x, y = ot.flatten_video(d["real"]), ot.flatten_video(d["fake"])
    return [ot.modified_cost(p, q, d[h], d[m], W.cases.SC) for p, q, h, m in
            ((x, y, "h_fake", "m_real"), (x, x, "h_real", "m_real"), (y, y, "h_fake", "m_fake"))]


# ================================================================ 1. the reference against sweep, the oracle and autograd
@pytest.mark.parametrize("n,L", [(6, 12), (17, 130)])
def test_stopped_sweep_equals_sweep_where_the_arguments_overlap(n, L):
    C = W.small_cost(n, 40 + n)
    for a, b in ((W.random_weights(n, 3 + n), W.random_weights(n, 4 + n)), (torch.full((n,), 1.0 / n, dtype=F64),) * 2):
        want = WG.sweep(C, a, b, 0.8, L, g=-0.5)
        got = stopped_sweep(C, a, b, 0.8, L, W.LMIN, THRESH, False, -0.5)
        assert got[1] == want[1] and (L == 12 or want[1] < L)          # L = 130: the stop at Lmin = 100 fires in both
        assert abs(float(got[0]) - float(want[0])) <= 1e-12 * abs(float(want[0]))
        for i in (2, 3, 4):
            assert float((got[i] - want[i]).abs().max()) <= 1e-12 * float(want[i].abs().max()), i
        assert len(got[7]) == got[1]


@pytest.mark.parametrize("stop_on_index", [False, True])
def test_stopped_sweep_equals_the_oracle_loop_in_both_stop_modes(stop_on_index):
    n = 17
    C = W.small_cost(n, 57).double()
    uni = torch.full((n,), 1.0 / n, dtype=F64)          # the oracle's own 1/n, not its float32 rounding
    for eps, L in ((1.0, 130), (0.8, 100), (1.0, 101)):
        want, nits = ot.sinkhorn_from_cost(C, eps, L, W.LMIN, stop_on_index)
        got = stopped_sweep(C, uni, uni, eps, L, W.LMIN, THRESH, stop_on_index)
        assert got[1] == nits == min(L, 101 if stop_on_index else 100), (eps, L, nits)
        assert abs(float(got[0]) - float(want)) <= 1e-12 * abs(float(want))


@pytest.mark.parametrize("n", [7, 24, 48])
def test_stopped_sweep_equals_autograd_through_the_stopped_loop(n):
    C, a, b, (eps, L, Lmin) = stop_problems(n)
    for kind in ("uniform", "ab"):
        wa, wb = weights_of(n, kind)
        for p in range(3):
            r = stopped_sweep(C[p], wa[p], wb[p], eps, L, Lmin, THRESH, False, 1.0)
            assert Lmin < r[1] < L - 1
            Cl, al, bl = (x.double().requires_grad_(True) for x in (C[p], wa[p], wb[p]))
            cost = differentiable_stopped_cost(Cl, al, bl, eps, r[1])
            assert abs(float(cost.detach()) - float(r[0])) <= 1e-12 * abs(float(r[0]))
            for name, got, ref in zip(("dC", "da", "db"), r[2:5], torch.autograd.grad(cost, (Cl, al, bl))):
                err = float((got - ref).abs().max()) / float(ref.abs().max())
                print("n=%d %s p=%d k=%d %s: %.2e" % (n, kind, p, r[1], name, err))
                assert err <= 1e-10, (name, err)


# ================================================================ 2. the inputs meet the conditions
def launch_problems(n, kind):
    """[(tag, C, a, b)] of the launch `kind` at size n."""
    C, _, _, _ = stop_problems(n)
    if kind == "cond":
        w = cond_weights(n)
        return [("q=%d k=%d" % (q, k), C[k], w[q], w[q]) for q in range(len(w)) for k in range(3)]
    wa, wb = weights_of(n, kind)
    return [("p=%d" % p, C[p], wa[p], wb[p]) for p in range(3)]


@pytest.mark.parametrize("n", SIZES)
def test_inputs_meet_the_conditions(n):
    C, a, b, (eps, L, Lmin) = stop_problems(n)
    assert Lmin == 3 and L == 40 and tuple(C.shape) == (3, n, n) and C.dtype == F32
    tiny = float(torch.finfo(F32).tiny)
    assert float(a.min()) >= tiny and float(b.min()) >= tiny
    for kind in ("uniform", "ab") + (("cond",) if n in COND_SIZES else ()):
        thresh = stop_thresh(n, kind)
        ks = []
        for tag, Cp, ap, bp in launch_problems(n, kind):
            assert float(ap.min()) >= tiny and float(bp.min()) >= tiny
            k, ok, fig = stop_count(Cp, ap, bp, eps, L, Lmin, thresh)
            print("n=%d %s %s thresh %.4g: k=%d errs[k-2]/thresh %.2f errs[k-1]/thresh %.3f G/thresh %.2f float32 k=%d"
                  % ((n, kind, tag, thresh) + fig))
            assert ok, (n, kind, tag, fig)
            ks.append(k)
        assert len(set(ks)) >= 2, (n, kind, ks)


def test_which_cases_place_their_threshold():
    """Printed (-s): the launches that do not keep thresh = 1e-2.  Every family keeps it somewhere: the unweighted launches at
    every size, the weighted ones at every register size and at the streaming sizes up to 516, the conditional ones everywhere."""
    placed = [(n, kind) for n in SIZES for kind in ("uniform", "ab") + (("cond",) if n in COND_SIZES else ())
              if stop_thresh(n, kind) != THRESH]
    print("launches that place thresh at sqrt(errs[k-2] errs[k-1]): %s"
          % (", ".join("n=%d %s thresh=%.4g" % (n, kind, stop_thresh(n, kind)) for n, kind in placed) or "none"))
    assert THRESH == 1e-2
    assert all(kind == "ab" and n > 516 for n, kind in placed), placed


# ================================================================ 3. the boundaries, on the reference
@pytest.mark.parametrize("kind", ["uniform", "ab"])
def test_boundaries_of_the_stop_rule(kind):
    n = 48
    C, _, _, (eps, L, Lmin) = stop_problems(n)
    wa, wb = weights_of(n, kind)
    for p in range(3):
        k = references(n, kind)[1][p]

        def count(L_, Lmin_, index):
            return stopped_loop(C[p], wa[p], wb[p], eps, L_, Lmin_, THRESH, index)[3]

        assert count(k, Lmin, False) == k             # the loop's bound ends it where the rule would have
        assert count(k + 1, Lmin, False) == k
        assert count(k - 1, Lmin, False) == k - 1
        for m in (k, k + 2):
            assert count(L, m, False) == m and count(L, m, True) == m + 1
        assert count(L, k - 1, True) == k             # index k - 1 is iteration k
        for m in range(1, k - 1):
            assert count(L, m, False) == k and count(L, m, True) == k


# ================================================================ 4. the fused launch's fourth problem, the public-API case
@pytest.mark.parametrize("n", FUSED_SIZES)
def test_fused_problems_meet_the_conditions(n):
    Cmix = fused_problems(n)
    assert tuple(Cmix.shape) == (4, n, n) and same_values(Cmix[:3], stop_problems(n)[0])
    ks = []
    for p in range(4):
        k, ok, fig = stop_count(Cmix[p], uniform(n), uniform(n), STOP_EPS, STOP_L, STOP_LMIN)
        print("n=%d fused p=%d: k=%d errs[k-2]/thresh %.2f errs[k-1]/thresh %.3f G/thresh %.2f float32 k=%d" % ((n, p) + fig))
        assert ok, (n, p, fig)
        ks.append(k)
    assert len(set(ks[:3])) >= 2 and [r[1] for r in fused_references(n, (1.0, 1.0, -1.0, -1.0))] == ks


def same_values(x, y):
    return bool((x == y).all())


def test_public_api_case_stops_at_lmin_by_a_margin():
    """L = 130 > Lmin = 100 at eps = 1: the oracle's loss (eps = 1, L = 100 whatever it is passed) runs 100 iterations, and a
    loop allowed 130 stops after 100 too, its error there below thresh - G."""
    d = {k: v.double() for k, v in api_inputs().items()}
    n = API_SHAPE[0]
    uni = torch.full((n,), 1.0 / n, dtype=F64)
    for p, C in enumerate(api_costs(d)):
        U, _, errs, k = stopped_loop(C, uni, uni, API_EPS, API_L)
        G = margin(n, U)
        print("B=%d problem %d: count %d, err at iteration 100 %.3e, thresh - G %.3e" % (n, p, k, errs[99], THRESH - G))
        assert k == 100 and errs[99] < THRESH - G
        assert ot.sinkhorn_from_cost(C, API_EPS, API_L)[1] == 100 and ot.sinkhorn_from_cost(C, API_EPS, 100)[1] == 100
        assert stopped_loop(C.float(), uni, uni, API_EPS, API_L, dtype=F32)[3] == 100
