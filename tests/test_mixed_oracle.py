"""CPU tier of the mixed (two-minibatch) Sinkhorn divergence: the fixtures of tests/golden/make_mixed_golden.py against
regenerated inputs and the torch oracle composition, the identity with the one-batch loss, and the public signature."""
import inspect
import os

import numpy as np
import pytest
import torch

import cases
import mixed_cases
from oracle import gan_utils_torch as ot

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _load(shape, seed, regime):
    return np.load(os.path.join(GOLD, mixed_cases.case_name(shape, seed, regime) + ".npz"))


def _terms(d):
    fl = ot.flatten_video
    return [ot.compute_sinkhorn(fl(d[a]), fl(d[b]), d[h], d[m], cases.SC) for a, b, h, m, _ in mixed_cases.TERMS]


@pytest.mark.parametrize("shape,seed,regime", mixed_cases.CASES)
def test_mixed_fixture_checksums(shape, seed, regime):
    g = _load(shape, seed, regime)
    np.testing.assert_array_equal(mixed_cases.checksum(mixed_cases.gen_inputs(shape, seed, regime)), g["checksum"])
    for t in range(1, 5):
        assert g["C%d" % t].dtype == np.float32 and g["C%d_f64" % t].dtype == np.float64


@pytest.mark.parametrize("shape,seed,regime", [c for c in mixed_cases.CASES if c[0] != "cfg2"])
def test_torch_oracle_composition_reproduces_the_fixture(shape, seed, regime):
    g = _load(shape, seed, regime)
    d = {k: torch.from_numpy(v).double() for k, v in mixed_cases.gen_inputs(shape, seed, regime).items()}
    w = _terms(d)
    for t in range(4):
        assert abs(float(w[t]) - float(g["w%d_f64" % (t + 1)])) <= 1e-9 * abs(float(g["w%d_f64" % (t + 1)]))
    loss = (w[0] + w[1]) - w[2] - w[3]
    assert abs(float(loss) - float(g["loss_f64"])) <= 1e-9 * max(abs(float(x)) for x in w)


def test_identity_case_of_the_composition_is_the_one_batch_loss():
    inp = cases.gen_inputs("small", 0, "near")
    d = {k: torch.from_numpy(v).double() for k, v in inp.items()}
    mixed = dict(real=d["real"], fake=d["fake"], real_p=d["real"], fake_p=d["fake"], h_fake=d["h_fake"], m_real=d["m_real"],
                 h_real_p=d["h_real"], m_fake=d["m_fake"], h_fake_p=d["h_fake"], m_real_p=d["m_real"])
    w = _terms(mixed)
    one = ot.compute_sinkhorn_loss(d["real"], d["fake"], cases.SC, 0.8, 100, d["h_fake"], d["m_real"], d["h_real"],
                                   d["m_fake"])
    assert abs(float((w[0] + w[1]) - w[2] - w[3]) - float(one)) <= 1e-12 * abs(float(one))


def test_public_signature():
    from kccotgan_amd import gan_utils as G
    assert "compute_mixed_sinkhorn_loss" in G.__all__
    sig = inspect.signature(G.compute_mixed_sinkhorn_loss)
    assert list(sig.parameters) == ["f_real", "f_fake", "f_real_p", "f_fake_p", "scaling_coef", "sinkhorn_eps", "sinkhorn_l",
                                    "h_fake", "m_real", "h_real_p", "m_fake", "h_fake_p", "m_real_p", "video",
                                    "honor_eps_l"]
    assert sig.parameters["video"].default is True
    assert sig.parameters["honor_eps_l"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["honor_eps_l"].default is False
