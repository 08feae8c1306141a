"""CPU tier of the bi-causal Sinkhorn loss: the fixtures of tests/golden/make_bicausal_golden.py against regenerated
inputs and the numpy / torch oracle compositions, the public signature, and the trainer's refusals (raised before any
device work)."""
import inspect
import os

import numpy as np
import pytest
import torch

import bicausal_cases
import cases
from oracle import gan_utils_np as on
from oracle import gan_utils_torch as ot

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _load(case):
    return np.load(os.path.join(GOLD, bicausal_cases.case_name(*case) + ".npz"))


def _flat(d, fl):
    d = dict(d)
    d["real"], d["fake"] = fl(d["real"]), fl(d["fake"])
    return d


@pytest.mark.parametrize("case", bicausal_cases.CASES, ids=lambda c: bicausal_cases.case_name(*c))
def test_bicausal_fixture_checksums_and_layout(case):
    g = _load(case)
    np.testing.assert_array_equal(cases.checksum(cases.gen_inputs(*case[:3])), g["checksum"])
    B = cases.SHAPES[case[0]][0]
    for tag in ("xy", "xx", "yy"):
        assert g["C_" + tag].dtype == np.float32 and g["C_%s_f64" % tag].dtype == np.float64
        assert g["C_" + tag].shape == (B, B)
    w = {t: float(g["w_%s_f64" % t]) for t in ("xy", "xx", "yy")}
    assert float(g["loss_f64"]) == 2 * w["xy"] - w["xx"] - w["yy"]


@pytest.mark.parametrize("case", [c for c in bicausal_cases.CASES if c[0] != "cfg2"],
                         ids=lambda c: bicausal_cases.case_name(*c))
def test_numpy_oracle_composition_reproduces_the_fixture(case):
    shape, seed, regime, eps, L = case
    g = _load(case)
    d = _flat({k: v.astype(np.float64) for k, v in cases.gen_inputs(shape, seed, regime).items()}, on.flatten_video)
    w = {}
    for tag, a, b, hy, mx, hx, my in bicausal_cases.TERMS:
        cost, nits, C = on.compute_sinkhorn_ex(d[a], d[b], d[hy], d[mx], cases.SC, hx=d[hx], My=d[my], epsilon=eps, L=L,
                                               bi_causal=True, dtype=np.float64)
        assert nits == int(g["nits_" + tag])
        np.testing.assert_allclose(C, g["C_%s_f64" % tag], rtol=1e-12, atol=1e-12 * np.abs(C).max())
        assert abs(float(cost) - float(g["w_%s_f64" % tag])) <= 1e-9 * abs(float(g["w_%s_f64" % tag]))
        w[tag] = float(cost)
    loss = 2 * w["xy"] - w["xx"] - w["yy"]
    assert abs(loss - float(g["loss_f64"])) <= 1e-9 * max(abs(x) for x in w.values())


@pytest.mark.parametrize("case", [c for c in bicausal_cases.CASES if c[0] in ("tiny", "small")],
                         ids=lambda c: bicausal_cases.case_name(*c))
def test_torch_oracle_composition_reproduces_the_fixture(case):
    shape, seed, regime, eps, L = case
    g = _load(case)
    d = _flat({k: torch.from_numpy(v).double() for k, v in cases.gen_inputs(shape, seed, regime).items()}, ot.flatten_video)
    w = {tag: float(ot.compute_sinkhorn(d[a], d[b], d[hy], d[mx], cases.SC, hx=d[hx], My=d[my], epsilon=eps, L=L,
                                        bi_causal=True))
         for tag, a, b, hy, mx, hx, my in bicausal_cases.TERMS}
    for tag, v in w.items():
        assert abs(v - float(g["w_%s_f64" % tag])) <= 1e-9 * abs(float(g["w_%s_f64" % tag]))
    assert abs(2 * w["xy"] - w["xx"] - w["yy"] - float(g["loss_f64"])) <= 1e-9 * max(abs(x) for x in w.values())


def test_degenerate_case_of_the_composition_is_the_one_batch_loss():
    # h_real = 0 and m_fake constant in time: every causal term the bi-causal loss adds is zero
    inp = cases.gen_inputs("small", 0, "near")
    d = {k: torch.from_numpy(v).double() for k, v in inp.items()}
    d["h_real"] = torch.zeros_like(d["h_real"])
    d["m_fake"] = d["m_fake"][:, :1].expand_as(d["m_fake"]).contiguous()
    x, y = ot.flatten_video(d["real"]), ot.flatten_video(d["fake"])
    w = {tag: ot.compute_sinkhorn(dd[a], dd[b], dd[hy], dd[mx], cases.SC, hx=dd[hx], My=dd[my], bi_causal=True)
         for dd in [dict(d, real=x, fake=y)] for tag, a, b, hy, mx, hx, my in bicausal_cases.TERMS}
    one = ot.compute_sinkhorn_loss(d["real"], d["fake"], cases.SC, 0.8, 100, d["h_fake"], d["m_real"], d["h_real"],
                                   d["m_fake"])
    assert abs(float(2 * w["xy"] - w["xx"] - w["yy"]) - float(one)) <= 1e-12 * abs(float(one))


def test_public_signature():
    from kccotgan_amd import gan_utils as G
    assert "compute_bicausal_sinkhorn_loss" in G.__all__
    sig = inspect.signature(G.compute_bicausal_sinkhorn_loss)
    assert list(sig.parameters) == list(inspect.signature(G.compute_sinkhorn_loss).parameters)
    assert sig.parameters["video"].default is True
    assert sig.parameters["honor_eps_l"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["honor_eps_l"].default is False


def test_trainer_refuses_bicausal_with_mixed():
    from kccotgan_amd.kernel_train import KCCOTTrainer
    with pytest.raises(ValueError):
        KCCOTTrainer(2, device="cpu", mixed_sinkhorn=True, bi_causal=True)


def test_trainer_refuses_bicausal_with_data_parallelism():
    from kccotgan_amd.kernel_train import KCCOTTrainer
    with pytest.raises(NotImplementedError):
        KCCOTTrainer(2, device="cpu", bi_causal=True, group=object())
