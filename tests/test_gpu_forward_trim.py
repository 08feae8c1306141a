"""The trimmed forward half-step of the fused solve + reverse sweep (the DPP max as one statement, the add tree on
two-wide pairs, and in the role kernel the row addresses moved on and the stop rule's |du| formed in the other role's
half-step) against the two-launch path, BIT for bit, through the C ABI.

kccot_sinkhorn_divergence_fused_f32 runs with the role kernel (option "sinkhorn_fused_roles" = 1) and with the one-role
kernel (= 0); the reference is kccot_sinkhorn_divergence_fwd_f32 + kccot_sinkhorn_divergence_bwd_f32 with the dual history in
global memory, computed once per case.  Compared: cost, nits reported and executed, loss, dC, as 32-bit patterns (NaN
payloads and the sign of zero included); every output starts poisoned, the ticket must be left at zero.

Lanes per line: 8 on both paths (the headline instance <8,8> at every n), and the library's own choice with the reference at
the lanes the fused kernel then takes (16 at n <= 32: one and two entries per lane).  n = 7, 32, 33, 64; L = 1, 2, 100.
Further cases: a stop rule that is evaluated and NOT met at least once and then met (|du| is formed in the iteration that
stops and in the one before it, and in no other), the shortcut on and jumping, a second launch on one ticket word, and cost
matrices with a row whose max-shifted entries peak at +inf (an entry of C is -inf), a row of +inf (every entry -inf after
the sign flip: the line's max is -inf) and a NaN entry: the non-finite-max guard `finite ? mx : 0` on every class of input.
The guard's identity itself is checked on the host over a list of special values."""
import math
import struct

import pytest
import torch

from test_gpu_fused_roles import DEV, L, _random_costs, _reset_flags, _seeded_costs, _solve  # noqa: F401 (fixtures)

NS = [7, 32, 33, 64]
KEYS = ("cost", "nits", "executed", "loss", "dC")
_ref_cache = {}


def _two_launch(L, C, ref_lanes, Lit, Lmin, thresh, key):
    """The two-launch path on three problems; computed once per key and left unchanged by its users."""
    if key in _ref_cache:
        return _ref_cache[key]
    from kccotgan_amd._lib import ptr
    n = C.shape[1]
    uh = torch.full((3, max(Lit, 1), n), float("nan"), device=DEV)
    vh = torch.full_like(uh, float("nan"))
    cost = torch.full((3,), float("nan"), device=DEV)
    nits = torch.full((6,), -7, dtype=torch.int32, device=DEV)
    loss = torch.full((1,), float("nan"), device=DEV)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    dC = torch.full_like(C, float("nan"))
    one = torch.ones(1, device=DEV)
    with L.options(sinkhorn_fused=0, sinkhorn_lanes_per_line=ref_lanes):
        rc = L.lib.kccot_sinkhorn_divergence_fwd_f32(ptr(C), n, 1.0, Lit, Lmin, thresh, ptr(uh), ptr(vh), ptr(cost), ptr(nits),
                                                     ptr(loss), ptr(ticket), None, 0, None)
        assert rc == 0, L.lib.kccot_last_error()
        rc = L.lib.kccot_sinkhorn_divergence_bwd_f32(ptr(C), ptr(uh), ptr(vh), ptr(nits), n, 1.0, Lit, ptr(one), ptr(dC), None, 0, None)
        torch.cuda.synchronize()
        assert rc == 0, L.lib.kccot_last_error()
    ref = dict(cost=cost, nits=nits[:3], executed=nits[3:], loss=loss, dC=dC)
    assert (ref["nits"] != -7).all() and (ref["executed"] != -7).all(), (key, "reference not written")
    _ref_cache[key] = ref
    return ref


def _same_bits(got, ref, what):
    bad = [k for k in KEYS if not torch.equal(got[k].view(torch.int32), ref[k].view(torch.int32))]
    for k in bad:                                                      # shown when the assertion below fails
        g, r = got[k].view(torch.int32).flatten(), ref[k].view(torch.int32).flatten()
        d = (g != r).nonzero().flatten()
        both_nan = bool((torch.isnan(got[k].float().flatten()[d]) & torch.isnan(ref[k].float().flatten()[d])).all())
        print(what, k, "%d of %d words differ, NaN on both sides in all of them: %s; first: %s against %s" % (
            d.numel(), g.numel(), both_nan, [hex(x & 0xffffffff) for x in g[d][:3].tolist()],
            [hex(x & 0xffffffff) for x in r[d][:3].tolist()]))
    assert not bad, (what, bad)
    assert int(got["ticket"]) == 0, (what, "ticket")


def _check(L, C, lanes, Lit, Lmin, thresh, key):
    """Both fused bodies against the two-launch path.  lanes = 8: the option is 8 on both paths; lanes = 0: the library's choice
    for the fused launch (16 lanes at n <= 32, 8 above), the reference at those lanes."""
    n = C.shape[1]
    ref = _two_launch(L, C, lanes if lanes else (8 if n > 32 else 0), Lit, Lmin, thresh, key)
    ran_roles = 0
    for roles in (1, 0):
        with L.options(sinkhorn_fused_roles=roles, sinkhorn_lanes_per_line=lanes):
            assert L.lib.kccot_sinkhorn_fused_eligible(n, Lit) == 1, key
            ran_roles += int(L.lib.kccot_sinkhorn_fused_roles_eligible(n, Lit) == 1)
            _same_bits(_solve(L, C, Lit, Lmin, thresh), ref, (key, "roles=%d" % roles))
    assert ran_roles == 1, (key, "the role kernel runs exactly when the option is on")
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [8, 0])
@pytest.mark.parametrize("n", NS)
def test_every_iteration_executed(L, n, lanes):
    L.set_option("sinkhorn_shortcut", 0)
    C = _random_costs(3, n, 9100 + n)
    for Lit in (1, 2, 100):
        ref = _check(L, C, lanes, Lit, Lit, 1e-2, ("all", n, lanes, Lit))
        assert ref["nits"].tolist() == [Lit] * 3 and ref["executed"].tolist() == [Lit] * 3


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [8, 0])
@pytest.mark.parametrize("n", [33, 64])
def test_a_stop_rule_that_is_missed_and_then_met(L, n, lanes):
    """Lmin = 2 < L = 100.  The threshold is the largest of a decade ladder at which the two-launch path stops strictly between
    Lmin + 1 and L on every problem: the rule is then evaluated at least twice, missed first and met last."""
    L.set_option("sinkhorn_shortcut", 0)
    C = _random_costs(3, n, 9200 + n)
    chosen = None
    for thresh in (1e3, 1e2, 1e1, 1e0, 1e-1, 1e-2, 1e-3):
        ref = _two_launch(L, C, 8, 100, 2, thresh, ("ladder", n, thresh))
        if all(3 <= k < 100 for k in ref["nits"].tolist()):
            chosen = thresh
            break
    assert chosen is not None, "no threshold of the ladder stops the solve between iterations 3 and 99"
    ref = _check(L, C, lanes, 100, 2, chosen, ("ladder", n, chosen))
    assert all(3 <= k < 100 for k in ref["nits"].tolist()) and ref["executed"].tolist() == ref["nits"].tolist()
    # and a stop at the first evaluation, and a rule that is evaluated in every iteration and never met
    _check(L, C, lanes, 100, 3, 1e30, ("first", n, lanes))
    ref = _check(L, C, lanes, 100, 1, 0.0, ("never", n, lanes))
    assert ref["nits"].tolist() == [100] * 3


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [8, 0])
@pytest.mark.parametrize("n", [33, 64])
def test_the_shortcut_on_and_jumping(L, n, lanes):
    L.set_option("sinkhorn_shortcut", 1)
    C = _seeded_costs("near", 3, n)
    ref = _check(L, C, lanes, 100, 100, 1e-2, ("near", n, lanes))
    assert int(ref["executed"][0]) < 100 and int(ref["nits"][0]) == 100, (ref["executed"], ref["nits"])


@pytest.mark.gpu
@pytest.mark.parametrize("roles", [1, 0])
def test_a_second_launch_on_the_same_ticket(L, roles):
    from kccotgan_amd._lib import ptr
    L.set_option("sinkhorn_shortcut", 0)
    L.set_option("sinkhorn_fused_roles", roles)
    L.set_option("sinkhorn_lanes_per_line", 8)
    n, Lit = 33, 100
    Cs = [_random_costs(3, n, 9300), _random_costs(3, n, 9301)]
    refs = [_two_launch(L, C, 8, Lit, Lit, 1e-2, ("ticket", k)) for k, C in enumerate(Cs)]
    L.set_option("sinkhorn_lanes_per_line", 8)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    outs = []
    for C in Cs:
        o = dict(cost=torch.full((3,), float("nan"), device=DEV), nits=torch.full((6,), -7, dtype=torch.int32, device=DEV),
                 loss=torch.full((1,), float("nan"), device=DEV), dC=torch.full_like(C, float("nan")))
        rc = L.lib.kccot_sinkhorn_divergence_fused_f32(ptr(C), n, 1.0, Lit, Lit, 1e-2, ptr(o["cost"]), ptr(o["nits"]), ptr(o["loss"]),
                                                       ptr(ticket), ptr(o["dC"]), None)
        assert rc == 0, L.lib.kccot_last_error()
        outs.append(o)
    torch.cuda.synchronize()
    for k, (o, ref) in enumerate(zip(outs, refs)):
        _same_bits(dict(cost=o["cost"], nits=o["nits"][:3], executed=o["nits"][3:], loss=o["loss"], dC=o["dC"], ticket=ticket), ref,
                   ("launch", k))


def _special_costs(n, kind):
    C = _random_costs(3, n, 9400 + n).clone()
    if kind == "max_plus_inf":
        C[0, 1, 2] = -math.inf              # y = (U - c2) + V = +inf: the line's max is +inf
        C[2, n - 1, 0] = -math.inf
    elif kind == "all_minus_inf":
        C[0, 1, :] = math.inf               # every y of row 1 is -inf: the max is -inf
        C[1, :, n - 1] = math.inf           # ... and of column n - 1
    else:
        C[0, 1, 2] = math.nan
        C[1, n - 1, n - 1] = math.nan
    return C


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["max_plus_inf", "all_minus_inf", "nan"])
@pytest.mark.parametrize("n", [33, 64])
def test_non_finite_maxima_take_the_guard_the_two_launch_path_takes(L, n, kind):
    """Every word of every output, NaNs included: a NaN cost or NaN entry of dC leaves these kernels as 0x7fc00000
    (canonical_nan, sinkhorn.hip; DESIGN 4.4 has what the sign of a NaN did without it)."""
    L.set_option("sinkhorn_shortcut", 0)
    C = _special_costs(n, kind)
    for Lit in (2, 100):
        for lanes in (8, 0):
            _check(L, C, lanes, Lit, Lit, 1e-2, (kind, n, Lit))


def test_the_guard_identity_on_special_values():
    """tf.reduce_logsumexp's shift: (mx > -inf && mx < inf) ? mx : 0, and the one-compare forms it may be emitted as
    (|mx| < inf; the class test "not NaN, not +-inf"): the same selected BITS for every special input."""
    def bits(x):
        return struct.unpack("<I", struct.pack("<f", x))[0]

    def f32(b):
        return struct.unpack("<f", struct.pack("<I", b))[0]

    specials = [0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0x00000001, 0x80000001,
                0x007fffff, 0x7f7fffff, 0xff7fffff, 0x3f800000, 0xc2280000]
    for b in specials:
        mx = f32(b)
        two_compares = b if (mx > -math.inf and mx < math.inf) else 0
        one_compare = b if abs(mx) < math.inf else 0
        exponent_all_ones = (b >> 23) & 0xff == 0xff                      # v_cmp_class: NaN or +-inf
        class_test = 0 if exponent_all_ones else b
        assert two_compares == one_compare == class_test, hex(b)
        if two_compares:
            assert bits(f32(two_compares)) == b
