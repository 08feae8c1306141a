"""Cases of the bi-causal Sinkhorn loss fixtures (tests/golden/bicausal_*.npz): inputs are ``cases.gen_inputs`` (the
one-batch loss's four features take a second role, no new inputs), each case optionally with an (epsilon, L) request
honoured through the keywords.  Used by ``make_bicausal_golden.py`` (build container) and by the tests."""
import cases

# (shape name, seed, regime, epsilon, L): (1.0, 100) is what the loss runs by default (sinkhorn_eps / sinkhorn_l ignored)
CASES = [
    ("tiny", 0, "near", 1.0, 100), ("tiny", 1, "far", 1.0, 100),
    ("small", 0, "near", 1.0, 100), ("small", 1, "far", 1.0, 100),
    ("deci64", 0, "near", 1.0, 100), ("deci64", 1, "far", 1.0, 100),
    ("cfg2", 0, "near", 1.0, 100),
    ("small", 2, "near", 0.8, 200),     # the honor_eps_l path (these inputs still stop at Lmin = 100 iterations)
]

# term -> (row operand, column operand, hy, Mx, hx, My) of compute_sinkhorn(x, y, hy, Mx, sc, hx=, My=, bi_causal=True)
TERMS = (("xy", "real", "fake", "h_fake", "m_real", "h_real", "m_fake"),
         ("xx", "real", "real", "h_real", "m_real", "h_real", "m_real"),
         ("yy", "fake", "fake", "h_fake", "m_fake", "h_fake", "m_fake"))
WEIGHTS = {"xy": 2.0, "xx": -1.0, "yy": -1.0}


def default_eps_l(eps, L):
    return (eps, L) == (1.0, 100)


def case_name(shape, seed, regime, eps, L):
    name = "bicausal_" + cases.case_name(shape, seed, regime)
    return name if default_eps_l(eps, L) else name + "_e%g_L%d" % (eps, L)
