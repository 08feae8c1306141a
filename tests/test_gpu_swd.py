"""The sliced Wasserstein distance on the GPU (include/kccot_swd.h, csrc/swd.hip) against the fp64 oracle of tests/swd_oracle.py,
through the C ABI with every output and the workspace between guard zones, and through the Python API and the trainer.

Tolerances: min(4 x the largest error measured on an MI355X over the grid, cap); the measurements are against the oracle.
    directions  |z - ref|                 cap 1e-5 (|z| <= 5.77, the angle rounded to <= 2^-22 rad, a few ulp of the functions)
    proj        |a - ref| per element     cap (adds per chunk + 4) 2^-24 sum_k |x_k| |theta^_k| + 1e-5 sum_k |x_k| / |theta|
    order       exactly numpy's stable argsort of the DEVICE's proj rows
    SW2         |v - ref| / ref           cap 1e-4, ref the oracle's own fp64 sort (the value is continuous in the projections)
    gradients   |d - ref| / max|ref|      cap 2.5e-5; ref the oracle's own gradient where tests/test_swd_cpu.py shows adjacent
                                          gaps >= 1e-4 of the range (GAPPED), else the oracle's gradient at the device's order
    measured    directions 7.077e-07   proj 0.0156 of its cap   SW2 5.141e-06   gradients 1.602e-05
    allowed     directions 2.83e-06    proj 0.0624 of its cap   SW2 2.06e-05    gradients 2.5e-05 (the cap)
The gradient error is the fp32 rounding of the projections (a chain of up to 512 adds per chunk: about 1e-6 absolute on values of
order 1..10) relative to their rank-wise differences (about 0.05 for the "noise" inputs): a property of the arithmetic of the
definition, not of a kernel.
fake bit-equal to real must give 0.0 and all-zero gradients exactly.  Each grid test prints its figures before it asserts
(DESIGN.md section 16)."""
import functools

import numpy as np
import pytest
import torch

import abi_guard as ag
import swd_oracle as so

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MEASURED = {"dir": 7.077e-07, "proj_frac": 0.0156, "sw2": 5.141e-06, "grad": 1.602e-05}
TOL_DIR = min(4 * MEASURED["dir"], so.DIR_CAP)
TOL_PROJ_FRAC = min(4 * MEASURED["proj_frac"], 1.0)
TOL_SW2 = min(4 * MEASURED["sw2"], so.SW2_CAP)
TOL_GRAD = min(4 * MEASURED["grad"], so.GRAD_CAP)

GAPPED = so.GAPPED
SHAPES = [(1, 7, 3), (2, 5, 1), (3, 1, 4), (4, 3, 5), (64, 1536, 8), (70, 1028, 16), (130, 516, 8), (1024, 8, 2),
          (5, 70, 130)]                       # the last: more than one projection tile forward, more than one projection step backward


def _lib():
    from kccotgan_amd import _lib
    return _lib


def _chunk_shapes():
    kc = _lib().swd_plan(8, 1024, 4)["kc"]
    shapes = [(8, kc + 5, 4), (8, 2 * kc + 3, 4)]
    assert [_lib().swd_plan(*s)["chunks"] for s in shapes] == [2, 3]
    return shapes


@pytest.fixture(scope="module")
def worst():
    w = {"dir": 0.0, "proj_frac": 0.0, "sw2": 0.0, "grad": 0.0}
    yield w
    print("\nworst over the grid: directions %.3e  proj %.4f of its cap  SW2 %.3e  gradients %.3e"
          % (w["dir"], w["proj_frac"], w["sw2"], w["grad"]))


@functools.lru_cache(maxsize=None)
def _case(kind, B, K, P, s):
    real, fake, seed = so.make(kind, B, K, s)
    a, b, _ = so.projections(real, fake, seed, P)
    for v in (real, fake, a, b):
        v.setflags(write=False)
    return real, fake, seed, a, b, so.sw2(real, fake, seed, P)


def _dev(v):
    return torch.from_numpy(np.array(v)).to(DEV)            # (a copy: the cached inputs are read-only)


def _done(rc, *bufs):
    torch.cuda.synchronize()
    assert rc == 0, _lib().lib.kccot_last_error()
    for b in bufs:
        assert b.verify() is None, b.verify()


def k_fwd(real, fake, P, seed, offset=0):
    """kccot_swd_fwd_f32 on guarded buffers -> (proj [2,P,B], order [2,P,B], inv_norm [P], swd) as CPU tensors"""
    L = _lib()
    B, K = real.shape
    x, y = _dev(real), _dev(fake)
    gi = [ag.guarded_input("real", x, 4 * offset), ag.guarded_input("fake", y, 4 * offset)]
    nb = L.lib.kccot_swd_workspace_bytes(B, K, P)
    assert nb > 0
    proj, order = ag.guarded(2 * P * B * 4, "output", "proj_out"), ag.guarded(2 * P * B * 4, "output", "order_out")
    inv, out, ws = ag.guarded(P * 4, "output", "inv_norm_out"), ag.guarded(4, "output", "swd_out"), ag.guarded(nb, "workspace", "ws")
    _done(L.lib.kccot_swd_fwd_f32(gi[0].ptr, gi[1].ptr, B, K, P, seed, proj.ptr, order.ptr, inv.ptr, out.ptr, ws.ptr, nb,
                                  None), proj, order, inv, out, ws, *gi)
    assert torch.equal(gi[0].view(torch.float32, (B, K)), x) and torch.equal(gi[1].view(torch.float32, (B, K)), y)
    res = (proj.view(torch.float32, (2, P, B)), order.view(torch.int32, (2, P, B)), inv.view(torch.float32, (P,)),
           out.view(torch.float32, (1,)))
    for r in res:
        assert not bool(ag.unwritten(r).any()), "an output was not written everywhere"
    return tuple(r.cpu() for r in res)


def k_bwd(g, proj, order, inv, B, K, P, seed, want_real=True, want_fake=True):
    """kccot_swd_bwd_f32 on guarded buffers -> (dreal | None, dfake | None) on the device"""
    L = _lib()
    gi = [ag.guarded_input("gswd", torch.tensor([g], dtype=torch.float32, device=DEV)), ag.guarded_input("proj", proj.to(DEV)),
          ag.guarded_input("order", order.to(DEV)), ag.guarded_input("inv_norm", inv.to(DEV))]
    nb = L.lib.kccot_swd_workspace_bytes(B, K, P)
    ws = ag.guarded(nb, "workspace", "ws")
    dr = ag.guarded(B * K * 4, "output", "dreal") if want_real else None
    df = ag.guarded(B * K * 4, "output", "dfake") if want_fake else None
    outs = [o for o in (dr, df) if o is not None]
    _done(L.lib.kccot_swd_bwd_f32(gi[0].ptr, gi[1].ptr, gi[2].ptr, gi[3].ptr, B, K, P, seed, dr.ptr if dr else None,
                                  df.ptr if df else None, ws.ptr, nb, None), ws, *outs, *gi)
    res = []
    for o in (dr, df):
        if o is None:
            res.append(None)
            continue
        d = o.view(torch.float32, (B, K))
        assert not bool(ag.unwritten(d).any()), o.name + " not written everywhere"
        res.append(d.clone())
    return tuple(res)


def k_dirs(seed, K, p_begin, p_count):
    L = _lib()
    out = ag.guarded(p_count * K * 4, "output", "out")
    _done(L.lib.kccot_swd_directions_f32(seed, K, p_begin, p_count, out.ptr, None), out)
    d = out.view(torch.float32, (p_count, K))
    assert not bool(ag.unwritten(d).any())
    return d.cpu().numpy()


def _rel(got, ref):
    m = float(np.abs(ref).max())
    return float(np.abs(got - ref).max()) / m if m > 0 else float(np.abs(got).max())


def _check_case(kind, B, K, P, s, worst, own_sort, offset=0):
    real, fake, seed, a, b, ref_v = _case(kind, B, K, P, s)
    kc = _lib().swd_plan(B, K, P)["kc"]
    proj, order, inv, val = k_fwd(real, fake, P, seed, offset)
    proj, order = proj.numpy(), order.numpy()
    # 2. proj against the oracle, element by element inside its cap
    fr = 0.0
    for plane, x, ref in ((0, real, a), (1, fake, b)):
        cap = so.proj_cap(x, seed, P, kc)
        err = np.abs(proj[plane].T.astype(np.float64) - ref)
        assert not bool((err[cap == 0] > 0).any())                         # an all-zero row projects to exactly 0
        fr = max(fr, float((err[cap > 0] / cap[cap > 0]).max(initial=0.0)))
    th = so.directions(seed, K, 0, P)
    inv_err = float(np.abs(inv.numpy() * np.sqrt((th * th).sum(1)) - 1).max())
    # 3. order: the stable argsort of the device's own projections
    want = np.argsort(proj, axis=2, kind="stable")
    # 4. the value
    got_v = float(val)
    e_v = abs(got_v - ref_v) / ref_v if ref_v > 0 else abs(got_v)
    # 5. gradients
    g = 0.75
    ref_dr, ref_df = so.gradients(real, fake, seed, P, g, None if own_sort else order)
    dr, df = k_bwd(g, torch.from_numpy(proj), torch.from_numpy(order), inv, B, K, P, seed)
    e_g = max(_rel(dr.cpu().numpy(), ref_dr), _rel(df.cpu().numpy(), ref_df))
    print("%s (%d,%d,%d) seed %d: proj %.4f of its cap  1/norm %.2e  SW2 %.3e (%.6e)  gradients %.3e"
          % (kind, B, K, P, s, fr, inv_err, e_v, got_v, e_g))
    worst["proj_frac"], worst["sw2"], worst["grad"] = max(worst["proj_frac"], fr), max(worst["sw2"], e_v), max(worst["grad"], e_g)
    # |theta| moves by at most TOL_DIR sqrt(K) with its elements, and by the rounding of its chunk sums
    assert fr <= TOL_PROJ_FRAC and inv_err <= (min(kc, K) + 4) * 2.0 ** -24 + TOL_DIR * np.sqrt(K / (th * th).sum(1).min())
    assert np.array_equal(order, want), "order is not the stable argsort of the device's projections"
    assert e_v <= TOL_SW2
    assert e_g <= TOL_GRAD
    # each gradient alone, the other NULL: the same bits
    assert torch.equal(k_bwd(g, torch.from_numpy(proj), torch.from_numpy(order), inv, B, K, P, seed, want_fake=False)[0], dr)
    assert torch.equal(k_bwd(g, torch.from_numpy(proj), torch.from_numpy(order), inv, B, K, P, seed, want_real=False)[1], df)


# ---- 1. directions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,K,p_begin,p_count", [(0, 4096, 0, 64), (100, 1023, 0, 16), ((1 << 63) + 12345, 7, 3, 5), (7, 1, 0, 3),
                                                    (2 ** 64 - 1, 258, 65530, 5)])
def test_directions_against_the_oracle(seed, K, p_begin, p_count, worst):
    got, ref = k_dirs(seed, K, p_begin, p_count), so.directions(seed, K, p_begin, p_count)
    err = float(np.abs(got - ref).max())
    print("directions seed %d K %d p %d..%d: |z - ref| %.3e  max|z| %.3f" % (seed, K, p_begin, p_begin + p_count, err, np.abs(got).max()))
    worst["dir"] = max(worst["dir"], err)
    assert np.isfinite(got).all() and err <= TOL_DIR


def test_directions_from_p_begin_are_the_rows_of_the_full_call():
    full = k_dirs(5, 1030, 0, 12)
    assert np.array_equal(k_dirs(5, 1030, 4, 8), full[4:]) and np.array_equal(k_dirs(5, 517, 4, 3), full[4:7, :517])


# ---- 2. - 5. the grid --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K,P,s", GAPPED)
def test_gap_conditioned_cases_against_the_oracles_own_sort(B, K, P, s, worst):
    _check_case("noise", B, K, P, s, worst, own_sort=True)


@pytest.mark.parametrize("kind", ["noise", "ties"])
@pytest.mark.parametrize("B,K,P", SHAPES)
def test_shapes_against_the_oracle_at_the_devices_matching(B, K, P, kind, worst):
    _check_case(kind, B, K, P, 1, worst, own_sort=False)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("kind", ["noise", "ties"])
def test_k_past_one_and_two_chunks(which, kind, worst):
    B, K, P = _chunk_shapes()[which]
    _check_case(kind, B, K, P, 2, worst, own_sort=False)


@pytest.mark.parametrize("B,K,P", [(8, 1023, 16), (8, 2052, 33), (70, 1028, 16)])
def test_unaligned_base_pointers(B, K, P, worst):
    _check_case("noise", B, K, P, 0, worst, own_sort=(B, K, P, 0) in GAPPED, offset=1)
    # the vector-load path and the scalar path add the same products in the same order
    real, fake, seed = _case("noise", B, K, P, 0)[:3]
    for got, ref in zip(k_fwd(real, fake, P, seed, 1), k_fwd(real, fake, P, seed, 0)):
        assert ag.same_bits(got, ref)


# ---- 6. exact zeros, ties -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K,P", [(2, 5, 1), (8, 1023, 16), (70, 1028, 16), (130, 516, 8)])
def test_fake_bit_equal_to_real_gives_exact_zeros(B, K, P):
    real, _, seed = _case("noise", B, K, P, 0)[:3]
    proj, order, inv, val = k_fwd(real, real.copy(), P, seed)
    assert float(val) == 0.0 and torch.equal(proj[0], proj[1]) and torch.equal(order[0], order[1])
    dr, df = k_bwd(1.0, proj, order, inv, B, K, P, seed)
    assert float(dr.abs().max()) == 0.0 and float(df.abs().max()) == 0.0


@pytest.mark.parametrize("B,K,P", [(4, 3, 5), (70, 1028, 16)])
def test_tied_projections_keep_the_lower_sample_index_first(B, K, P):
    real, fake, seed = _case("ties", B, K, P, 1)[:3]
    assert np.array_equal(real[1], real[2]) and np.array_equal(fake[1], fake[2]) and np.array_equal(real[0], fake[0])
    proj, order, _, _ = k_fwd(real, fake, P, seed)
    assert torch.equal(proj[:, :, 1], proj[:, :, 2]) and torch.equal(proj[0, :, 0], proj[1, :, 0])
    rank = torch.argsort(order.long(), dim=2)                  # rank of every sample
    assert bool((rank[:, :, 2] == rank[:, :, 1] + 1).all())


# ---- 7. bits -----------------------------------------------------------------------------------------------------------------------------
def _py_run(x, y, P, seed, g):
    """forward + backward through the library on plain torch buffers (capturable)"""
    L = _lib()
    B, K = x.shape
    proj, order = torch.empty((2, P, B), device=DEV), torch.empty((2, P, B), dtype=torch.int32, device=DEV)
    inv, out, dr, df = torch.empty(P, device=DEV), torch.empty(1, device=DEV), torch.empty_like(x), torch.empty_like(x)
    ws, wsb = L.workspace(L.lib.kccot_swd_workspace_bytes(B, K, P), x)
    st = L.stream_of(x)

    def run():
        L.check(L.lib.kccot_swd_fwd_f32(L.ptr(x), L.ptr(y), B, K, P, seed, L.ptr(proj), L.ptr(order), L.ptr(inv), L.ptr(out), ws, wsb,
                                        st), "swd_fwd")
        L.check(L.lib.kccot_swd_bwd_f32(L.ptr(g), L.ptr(proj), L.ptr(order), L.ptr(inv), B, K, P, seed, L.ptr(dr), L.ptr(df), ws, wsb,
                                        st), "swd_bwd")
    return run, (proj, order, inv, out, dr, df)


@pytest.mark.parametrize("B,K,P", [(8, 1023, 16), (70, 1028, 16)])
def test_identical_calls_and_a_graph_replay_give_identical_bits_and_the_seed_matters(B, K, P):
    real, fake, seed = _case("noise", B, K, P, 0)[:3]
    x, y = _dev(real), _dev(fake)
    g = torch.tensor([1.25], device=DEV)
    run, outs = _py_run(x, y, P, seed, g)
    run()
    torch.cuda.synchronize()
    first = [o.clone() for o in outs]
    for o in outs:
        o.fill_(0) if o.dtype == torch.int32 else o.fill_(float("nan"))
    run()
    torch.cuda.synchronize()
    assert all(ag.same_bits(a, b) for a, b in zip(outs, first))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run_s, outs_s = _py_run(x, y, P, seed, g)
        run_s()                                                # warm-up on the capture stream
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            run_s()
    for o in outs_s:
        o.zero_()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert all(ag.same_bits(a, b) for a, b in zip(outs_s, first))
    other = k_fwd(real, fake, P, seed + 1)[3]
    assert float(other) != float(first[3]) and float(other) > 0


# ---- 8. Python ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K,P", [(8, 1023, 16), (70, 1028, 16)])
def test_autograd_function_equals_the_abi_results(B, K, P):
    from kccotgan_amd import swd
    real, fake, seed = _case("noise", B, K, P, 0)[:3]
    proj, order, inv, val = k_fwd(real, fake, P, seed)
    dr, df = k_bwd(1.0, proj, order, inv, B, K, P, seed)
    shape = (B, K // 4, 4) if K % 4 == 0 else (B, K)
    x = _dev(real).view(shape).requires_grad_(True)
    y = _dev(fake).view(shape).requires_grad_(True)
    v = swd.sliced_wasserstein2(x, y, P, seed)
    assert v.shape == () and ag.same_bits(v.detach().view(1), val.to(DEV))
    v.backward()
    assert x.grad.shape == shape and ag.same_bits(x.grad.view(B, K), dr) and ag.same_bits(y.grad.view(B, K), df)
    # fake alone: no gradient w.r.t. real is computed, the same bits
    y2 = y.detach().clone().requires_grad_(True)
    (2.0 * swd.sliced_wasserstein2(x.detach(), y2, P, seed)).backward()
    ref2 = k_bwd(2.0, proj, order, inv, B, K, P, seed, want_real=False)[1]
    assert ag.same_bits(y2.grad.view(B, K), ref2)
    assert np.array_equal(swd.directions(seed, K, 2, 3).cpu().numpy(), k_dirs(seed, K, 2, 3))


def test_trainer_swd_is_finite_and_leaves_the_networks_unchanged(monkeypatch):
    from kccotgan_amd import gan
    from kccotgan_amd.kernel_train import KCCOTTrainer
    monkeypatch.setattr(gan, "_NATIVE", {"convlstm", "deconv", "dconv"})
    B, H, W, C, T, iT = 2, 64, 64, 1, 6, 2          # the smallest configuration of tests/test_gpu_train_step.py
    tr = KCCOTTrainer(B, total_time_steps=T, int_time_steps=iT, x_height=H, x_width=W, channels=C, kernel="none", warmup=10,
                      device=DEV)
    nets = (tr.context_encoder, tr.decoder)
    before = [t.detach().clone() for net in nets for t in list(net.parameters()) + list(net.buffers())]
    data = torch.rand(B, H, T, W, C, device=DEV)
    v = tr.swd(data, n_projections=16, seed=3)
    after = [t for net in nets for t in list(net.parameters()) + list(net.buffers())]
    assert v.shape == () and bool(torch.isfinite(v)) and float(v) >= 0 and not v.requires_grad
    assert len(before) == len(after) and all(torch.equal(a, b) for a, b in zip(before, after))
