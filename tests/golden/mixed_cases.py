"""Inputs of the mixed (two-minibatch) Sinkhorn divergence cases: the primed batch x', y' and the features h_real_p,
h_fake_p, m_real_p next to the first batch of ``cases.gen_inputs`` (same shapes and regimes, a separate seed stream).
Used by ``make_mixed_golden.py`` (build container) and by the tests; every fixture stores a float64 checksum of the
regenerated tensors."""
import numpy as np

import cases

# (shape name, seed, regime) of tests/golden/mixed_<name>.npz
CASES = [
    ("tiny", 0, "near"),
    ("small", 0, "near"), ("small", 1, "far"),
    ("deci64", 0, "near"), ("deci64", 1, "far"),
    ("cfg2", 0, "near"),
]

_SEED_BASE = 7919          # primed batch seeds: _SEED_BASE + seed (cases.gen_inputs uses `seed` itself)

KEYS = ("real", "fake", "real_p", "fake_p", "h_fake", "m_real", "h_real_p", "m_fake", "h_fake_p", "m_real_p")


def case_name(shape, seed, regime):
    return "mixed_" + cases.case_name(shape, seed, regime)


def gen_inputs(shape, seed, regime):
    """dict of KEYS: real, fake, h_fake, m_real, m_fake from cases.gen_inputs (h_real is not used by the mixed loss);
    real_p, fake_p [B,H,T,W,C] and h_real_p, h_fake_p, m_real_p [B,T,J] drawn the same way from the primed stream."""
    base = cases.gen_inputs(shape, seed, regime)
    B, H, T, W, C, J = cases.SHAPES[shape]
    rng = np.random.default_rng(_SEED_BASE + seed)
    real_p = rng.random((B, H, T, W, C), dtype=np.float32)
    if regime == "near":
        noise = rng.standard_normal((B, H, T, W, C), dtype=np.float32)
        fake_p = np.clip(real_p + np.float32(0.05) * noise, 0.0, 1.0).astype(np.float32)
    elif regime == "far":
        fake_p = rng.random((B, H, T, W, C), dtype=np.float32)
    else:
        raise ValueError(regime)
    out = {k: base[k] for k in ("real", "fake", "h_fake", "m_real", "m_fake")}
    out.update(real_p=real_p, fake_p=fake_p)
    for k in ("h_real_p", "h_fake_p", "m_real_p"):
        out[k] = rng.random((B, T, J), dtype=np.float32)
    return out


def checksum(inp):
    return np.array([np.sum(inp[k], dtype=np.float64) for k in KEYS])


# term -> (row operand, column operand, h, M, sign): loss = (W1 + W2) - W3 - W4
TERMS = (("real", "fake", "h_fake", "m_real", 1.0),
         ("real_p", "fake_p", "h_fake_p", "m_real_p", 1.0),
         ("real", "real_p", "h_real_p", "m_real", -1.0),
         ("fake", "fake_p", "h_fake_p", "m_fake", -1.0))
