"""One case per instantiation of the three planner-driven tile kernels, and one per tiling regime.  Not a test module: the table
behind tests/test_tile_plans_cpu.py (which holds it to the planners on the CPU) and tests/test_gpu_tile_instantiations.py
(which runs every case against float64).

    csrc/smooth_sigma.hip   dsigma_tile<R, NI>         chosen by ds_shape + ds_plan   kccot_smooth_dsigma_plan
    csrc/smooth_aniso.hip   aniso_tile<RS, NI, JOB>    chosen by an_plan              kccot_smooth_aniso_plan
    csrc/ssim.hip           ssim_walk<R, BWD>          tiled by ss_plan               kccot_ssim_plan

The part between the two marker lines is WRITTEN by tools/find_tile_plan_cases.py, from the plan queries alone (no GPU): for
every instantiation the shape with the fewest elements inside BOX that reaches it, for every regime the smallest shape inside
REGIME_BOX.  Everything above the markers is written by hand; the tool imports it (the regime predicates), so the two cannot
drift apart.  After a planner is re-tuned: `python tools/find_tile_plan_cases.py --write`, then both test modules.

Cases OUTSIDE the 4 M-element box: none.  Every instantiation that the launch switches can name, and with them everything the
planner picks at the BASELINE shapes with the trainer's radius 3 (BASELINE_PICKS), is reached by a shape of BOX: UNREACHED and
WIDE are empty.  (BOX steps through 3 * 2^k and the odd T lengths as well as the powers of two; the batch goes up to 256.)  Should
a re-tuning push a BASELINE pick out of BOX, the tool looks for it in WIDE_BOX -- every axis up to its BASELINE length, which
tests/test_gpu_smoothing_fp64.py already runs -- and lists the key in WIDE; tests/test_tile_plans_cpu.py refuses a BASELINE
pick in UNREACHED.

Regimes of the smoothing kernels (in the kernel's own view of the shape; `ragged` = the last piece is shorter):
    T3 / W3 / C3 / H3   three or more pieces along that axis (so an interior piece exists, both halos from neighbours) with a
                        ragged last piece
    NI>1                more than one owned position per thread
each for a symmetric and for a causal T.  Regimes of ssim_walk, forward and backward: every radius 0..7; ntw >= 3 (an interior
column tile); ct < min(C, 16) with ntc >= 3 (backward only: the forward's cost never prefers a narrower channel tile, see
SSIM_CASES); the branch B T tiles >= 1024 that stops cutting H into segments."""

FORM_FLAGS = {"T": 1, "causalT": 1 | 8, "HW": 2 | 4, "THW": 1 | 2 | 4, "causalTHW": 1 | 2 | 4 | 8}   # axes_flags of dsigma
FORMS = tuple(FORM_FLAGS)
JOBS = ("fwd", "adj", "dsigma")
BASELINE = {"cfg1": (64, 64, 30, 64, 1), "cfg2": (128, 64, 30, 64, 3), "cfg3": (256, 64, 30, 64, 3)}     # BASELINE.json configs[1..3]
BASELINE_RADIUS = 3                     # KernelSmoothing(6, 6), the trainer's default
MAX_ELEMS = 4 << 20                     # the box: at most 4 M elements
MIN_ELEMS = 256                         # and no case below one workgroup's worth of positions

# The shapes searched for an instantiation: the product of these lists, cut at MAX_ELEMS.
BOX = {"B": (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 256), "H": (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64),
       "T": (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 30), "W": (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64),
       "C": (1, 2, 3, 4, 8, 16)}
# The wider search for what the planner picks at BASELINE and BOX does not reach: no axis beyond its BASELINE length.
WIDE_BOX = {"B": (16, 32, 48, 64, 96, 128, 192, 256), "H": (16, 32, 64), "T": (8, 10, 15, 16, 20, 30), "W": (16, 32, 64), "C": (1, 2, 3)}
# The shapes searched for a regime: long single axes next to short ones.
REGIME_BOX = {"B": (1, 2, 3), "H": (4, 5, 8, 9, 16, 33, 64, 100, 200), "T": (4, 5, 8, 9, 30, 100, 300, 700, 1000),
              "W": (4, 5, 8, 9, 16, 33, 64, 100, 300, 1000), "C": (1, 2, 3, 5, 20, 100, 300, 600, 1000)}
SMOOTH_REGIMES = ("T3", "W3", "C3", "H3", "NI>1")


# What the launch switches can name and the constexpr limits admit.  tests/test_tile_plans_cpu.py pins each line below to the
# text of the .hip source it restates, so a change there fails until this table (and the cases) follow.
DS_RADII, DS_NIS = tuple(range(1, 8)), tuple(range(1, 9))       # launch_tile<R>, launch_tile_ni<R, NI> of smooth_sigma.hip
AN_RADII, AN_NIS = tuple(range(0, 8)), (1, 2, 4, 8)             # launch_tile_rs<RS>, launch_tile_ni<RS, NI> of smooth_aniso.hip


def ds_max_ni(radius):
    return 8 if radius <= 3 else (6 if radius == 4 else (5 if radius == 5 else 4))


def an_max_ni(rs, job):
    return (8 if rs <= 3 else 4) if job == "fwd" else (8 if rs <= 1 else (4 if rs <= 3 else 2))


def dsigma_nameable():
    return [(r, ni) for r in DS_RADII for ni in DS_NIS if ni <= ds_max_ni(r)]


def aniso_nameable():
    return [(rs, ni, job) for job in JOBS for rs in AN_RADII for ni in AN_NIS if ni <= an_max_ni(rs, job)]


def box_shapes(box, max_elems=MAX_ELEMS):
    """the shapes of a box in ascending number of elements (ties: in the order of the tuples)"""
    out = [(b, h, t, w, c) for b in box["B"] for h in box["H"] for t in box["T"] for w in box["W"] for c in box["C"]
           if b * h * t * w * c <= max_elems]
    return sorted(out, key=lambda s: (s[0] * s[1] * s[2] * s[3] * s[4], s))


def elems(shape):
    n = 1
    for d in shape:
        n *= d
    return n


ANISO_RT = BASELINE_RADIUS              # the temporal radius of every anisotropic case (RS runs over 0..7)


def dsigma_allowed(shape, r, form):
    """the entry point's rule: REFLECT needs r < the length of every symmetric axis; a causal T takes any radius"""
    B, H, T, W, C = shape
    return not ((form in ("T", "THW") and r >= T) or (form in ("HW", "THW", "causalTHW") and (r >= H or r >= W)))


def aniso_allowed(shape, rt, rs, causal):
    B, H, T, W, C = shape
    return (causal or rt < T) and rs < H and rs < W


def _long_enough(L, r, causal=False):
    """an axis worth a case: both borders and an interior position (symmetric: L >= 2r + 2; causal: a full row, L >= r + 2)"""
    return L >= (r + 2 if causal else 2 * r + 2)


def dsigma_worthwhile(shape, r, form):
    """The search keeps only shapes of MIN_ELEMS elements or more whose smoothed axes are long enough: the smallest shape that
    reaches <R, 1> is one element, where every form gives 0 and a wrong kernel passes."""
    B, H, T, W, C = shape
    return (elems(shape) >= MIN_ELEMS and (form == "HW" or _long_enough(T, r, form.startswith("causal"))) and
            (form in ("T", "causalT") or (_long_enough(H, r) and _long_enough(W, r))))


def aniso_worthwhile(shape, rt, rs, causal):
    B, H, T, W, C = shape
    return elems(shape) >= MIN_ELEMS and _long_enough(T, rt, causal) and _long_enough(H, rs) and _long_enough(W, rs)


def smooth_regime(p, regime, H, T, W, C):
    """does the plan p (a dict of a plan query) lie in `regime`; H, T, W, C: the kernel's view of the shape"""
    if not p["launches"]:
        return False
    if regime == "NI>1":
        return p["NI"] > 1
    n, ext, L = {"T3": ("ntt", "tt", T), "W3": ("ntw", "wt", W), "C3": ("ntc", "ct", C), "H3": ("nseg", "hs", H)}[regime]
    return p[n] >= 3 and L % p[ext] != 0


# ---- ssim_walk: written by hand (the cases are tiny); (name, shape, radius, regimes of the forward, regimes of the backward).
# "ct_cut" is a regime of the backward alone: forward, a tile of ct channels holds 256 / ct columns, so its cost
# (wt + 2r) / wt * 16 / ct only grows when ct shrinks, for every r and W: ss_plan never picks ct < min(C, 16) there.
SSIM_SHAPE_R = (1, 20, 2, 21, 3)        # the radius cases: 2 * 7 < 20; a 6 x 7 map at r = 7
SSIM_CASES = [("r%d" % r, SSIM_SHAPE_R, r, ("radius",), ("radius",)) for r in range(8)] + [
    ("ntw3", (1, 12, 1, 100, 8), 2, ("ntw3",), ("ntw3",)),
    ("ct_cut", (1, 30, 1, 30, 20), 7, (), ("ct_cut",)),
    ("noseg", (64, 16, 16, 16, 1), 1, ("noseg",), ("noseg",)),
]


def ssim_regime(p, regime, shape, r, backward, one_sample_plan=None):
    """does the plan p of kccot_ssim_plan lie in `regime`.  noseg: segments are not cut because B T tiles >= 1024 -- and the same
    frame in a batch of one IS cut (one_sample_plan), so the branch decides something."""
    B, H, T, W, C = shape
    if regime == "radius":
        return True
    if regime == "ntw3":            # an interior tile: its first column q0 > (backward: 2r, forward: 0) and q0 + wt < W - 2r
        return p["ntw"] >= 3 and any(tw * p["wt"] > (2 * r if backward else 0) and (tw + 1) * p["wt"] < W - 2 * r
                                     for tw in range(1, p["ntw"] - 1))
    if regime == "ct_cut":
        return p["ct"] < min(C, 16) and p["ntc"] >= 3 and C % p["ct"] != 0
    if regime == "noseg":
        return p["nseg"] == 1 and B * T * p["ntw"] * p["ntc"] >= 1024 and one_sample_plan is not None and one_sample_plan["nseg"] > 1
    raise KeyError(regime)


# ---- BEGIN GENERATED (tools/find_tile_plan_cases.py --write)
# (R, NI): (shape, form)
DSIGMA_INST = {
    (1, 1): ((1, 1, 4, 4, 16), 'causalT'),
    (1, 2): ((24, 48, 6, 6, 8), 'THW'),
    (1, 3): ((1, 16, 24, 48, 16), 'THW'),
    (1, 4): ((8, 64, 24, 48, 3), 'causalT'),
    (1, 5): ((24, 4, 24, 48, 8), 'THW'),
    (1, 6): ((4, 64, 14, 48, 16), 'causalT'),
    (1, 7): ((3, 48, 14, 64, 16), 'THW'),
    (1, 8): ((2, 64, 30, 64, 16), 'causalT'),
    (2, 1): ((1, 1, 4, 4, 16), 'causalT'),
    (2, 2): ((24, 48, 6, 6, 8), 'THW'),
    (2, 3): ((1, 24, 24, 48, 16), 'THW'),
    (2, 4): ((3, 16, 30, 64, 16), 'THW'),
    (2, 5): ((6, 48, 30, 48, 3), 'THW'),
    (2, 6): ((4, 64, 14, 48, 16), 'T'),
    (2, 7): ((3, 64, 14, 64, 16), 'THW'),
    (2, 8): ((2, 64, 30, 64, 16), 'T'),
    (3, 1): ((1, 1, 8, 2, 16), 'T'),
    (3, 2): ((1, 24, 24, 48, 16), 'T'),
    (3, 3): ((1, 24, 24, 48, 16), 'THW'),
    (3, 4): ((3, 16, 30, 64, 16), 'THW'),
    (3, 5): ((3, 32, 24, 48, 8), 'THW'),
    (3, 6): ((4, 64, 14, 48, 16), 'T'),
    (3, 7): ((3, 64, 14, 64, 16), 'THW'),
    (3, 8): ((2, 64, 30, 64, 16), 'T'),
    (4, 1): ((1, 1, 8, 2, 16), 'causalT'),
    (4, 2): ((1, 24, 24, 48, 16), 'T'),
    (4, 3): ((1, 24, 24, 48, 16), 'THW'),
    (4, 4): ((3, 16, 30, 64, 16), 'THW'),
    (4, 5): ((3, 16, 24, 48, 16), 'THW'),
    (4, 6): ((4, 64, 14, 48, 16), 'T'),
    (5, 1): ((1, 1, 8, 2, 16), 'causalT'),
    (5, 2): ((2, 48, 30, 48, 3), 'T'),
    (5, 3): ((3, 12, 14, 48, 16), 'causalTHW'),
    (5, 4): ((3, 16, 30, 64, 16), 'THW'),
    (5, 5): ((3, 32, 24, 48, 8), 'THW'),
    (6, 1): ((1, 1, 8, 2, 16), 'causalT'),
    (6, 2): ((2, 48, 30, 48, 3), 'T'),
    (6, 3): ((3, 24, 14, 24, 16), 'causalTHW'),
    (6, 4): ((8, 64, 24, 48, 3), 'causalT'),
    (7, 1): ((1, 1, 16, 1, 16), 'T'),
    (7, 2): ((2, 48, 30, 48, 3), 'T'),
    (7, 3): ((3, 16, 14, 24, 16), 'causalTHW'),
    (7, 4): ((8, 64, 24, 48, 3), 'T'),
}
# (RS, NI, job): (shape, radius_t, causal)
ANISO_INST = {
    (0, 1, 'adj'): ((1, 2, 8, 2, 8), 3, False),
    (0, 1, 'dsigma'): ((1, 2, 8, 2, 8), 3, False),
    (0, 1, 'fwd'): ((1, 2, 8, 2, 8), 3, False),
    (0, 2, 'adj'): ((32, 64, 30, 3, 3), 3, False),
    (0, 2, 'dsigma'): ((32, 64, 30, 3, 3), 3, False),
    (0, 2, 'fwd'): ((32, 64, 30, 3, 3), 3, False),
    (0, 4, 'adj'): ((4, 64, 24, 64, 3), 3, False),
    (0, 4, 'dsigma'): ((4, 64, 24, 64, 3), 3, False),
    (0, 4, 'fwd'): ((4, 64, 24, 64, 3), 3, False),
    (0, 8, 'adj'): ((8, 64, 24, 64, 3), 3, False),
    (0, 8, 'dsigma'): ((8, 64, 24, 64, 3), 3, False),
    (0, 8, 'fwd'): ((8, 64, 24, 64, 3), 3, False),
    (1, 1, 'adj'): ((1, 4, 8, 4, 2), 3, True),
    (1, 1, 'dsigma'): ((1, 4, 8, 4, 2), 3, True),
    (1, 1, 'fwd'): ((1, 4, 8, 4, 2), 3, True),
    (1, 2, 'adj'): ((3, 64, 20, 8, 8), 3, False),
    (1, 2, 'dsigma'): ((3, 64, 20, 8, 8), 3, False),
    (1, 2, 'fwd'): ((3, 64, 20, 8, 8), 3, False),
    (1, 4, 'adj'): ((12, 64, 10, 4, 16), 3, False),
    (1, 4, 'dsigma'): ((12, 64, 10, 4, 16), 3, False),
    (1, 4, 'fwd'): ((12, 64, 10, 4, 16), 3, False),
    (1, 8, 'adj'): ((12, 6, 20, 64, 16), 3, False),
    (1, 8, 'dsigma'): ((12, 6, 20, 64, 16), 3, False),
    (1, 8, 'fwd'): ((12, 6, 20, 64, 16), 3, False),
    (2, 1, 'adj'): ((1, 6, 6, 8, 1), 3, True),
    (2, 1, 'dsigma'): ((1, 6, 6, 8, 1), 3, True),
    (2, 1, 'fwd'): ((1, 6, 6, 8, 1), 3, True),
    (2, 2, 'adj'): ((12, 48, 10, 8, 8), 3, False),
    (2, 2, 'dsigma'): ((12, 48, 10, 8, 8), 3, False),
    (2, 2, 'fwd'): ((12, 48, 10, 8, 8), 3, False),
    (2, 4, 'adj'): ((24, 64, 10, 8, 8), 3, False),
    (2, 4, 'dsigma'): ((24, 64, 10, 8, 8), 3, False),
    (2, 4, 'fwd'): ((24, 64, 10, 8, 8), 3, False),
    (2, 8, 'fwd'): ((2, 64, 24, 48, 16), 3, False),
    (3, 1, 'adj'): ((1, 8, 5, 8, 1), 3, True),
    (3, 1, 'dsigma'): ((1, 8, 5, 8, 1), 3, True),
    (3, 1, 'fwd'): ((1, 8, 5, 8, 1), 3, True),
    (3, 2, 'adj'): ((3, 12, 20, 48, 16), 3, True),
    (3, 2, 'dsigma'): ((3, 12, 20, 48, 16), 3, True),
    (3, 2, 'fwd'): ((3, 12, 20, 48, 16), 3, True),
    (3, 4, 'adj'): ((1, 64, 24, 48, 16), 3, False),
    (3, 4, 'dsigma'): ((1, 64, 24, 48, 16), 3, False),
    (3, 4, 'fwd'): ((1, 64, 24, 48, 16), 3, False),
    (3, 8, 'fwd'): ((4, 48, 24, 48, 16), 3, False),
    (4, 1, 'adj'): ((1, 12, 5, 12, 1), 3, True),
    (4, 1, 'dsigma'): ((1, 12, 5, 12, 1), 3, True),
    (4, 1, 'fwd'): ((1, 12, 5, 12, 1), 3, True),
    (4, 2, 'adj'): ((1, 48, 14, 48, 16), 3, False),
    (4, 2, 'dsigma'): ((1, 48, 14, 48, 16), 3, False),
    (4, 2, 'fwd'): ((1, 48, 14, 48, 16), 3, False),
    (4, 4, 'fwd'): ((2, 48, 24, 48, 16), 3, False),
    (5, 1, 'adj'): ((1, 12, 5, 12, 1), 3, True),
    (5, 1, 'dsigma'): ((1, 12, 5, 12, 1), 3, True),
    (5, 1, 'fwd'): ((1, 12, 5, 12, 1), 3, True),
    (5, 2, 'adj'): ((3, 48, 5, 48, 16), 3, True),
    (5, 2, 'dsigma'): ((3, 48, 5, 48, 16), 3, True),
    (5, 2, 'fwd'): ((3, 48, 5, 48, 16), 3, True),
    (5, 4, 'fwd'): ((4, 48, 24, 48, 8), 3, False),
    (6, 1, 'adj'): ((1, 16, 5, 16, 1), 3, True),
    (6, 1, 'dsigma'): ((1, 16, 5, 16, 1), 3, True),
    (6, 1, 'fwd'): ((1, 16, 5, 16, 1), 3, True),
    (6, 2, 'adj'): ((3, 24, 10, 48, 16), 3, False),
    (6, 2, 'dsigma'): ((3, 24, 10, 48, 16), 3, False),
    (6, 2, 'fwd'): ((3, 24, 10, 48, 16), 3, False),
    (6, 4, 'fwd'): ((3, 64, 14, 48, 16), 3, False),
    (7, 1, 'adj'): ((1, 16, 5, 16, 1), 3, True),
    (7, 1, 'dsigma'): ((1, 16, 5, 16, 1), 3, True),
    (7, 1, 'fwd'): ((1, 16, 5, 16, 1), 3, True),
    (7, 2, 'adj'): ((3, 24, 10, 48, 16), 3, False),
    (7, 2, 'dsigma'): ((3, 24, 10, 48, 16), 3, False),
    (7, 2, 'fwd'): ((3, 24, 10, 48, 16), 3, False),
    (7, 4, 'fwd'): ((3, 48, 14, 48, 16), 3, False),
}
# (regime, form): (shape, radius)
DSIGMA_REGIME = {
    ('C3', 'THW'): ((1, 8, 8, 8, 100), 3),
    ('C3', 'causalTHW'): ((1, 8, 5, 8, 100), 3),
    ('H3', 'THW'): ((3, 33, 9, 64, 2), 3),
    ('H3', 'causalTHW'): ((3, 9, 5, 8, 100), 3),
    ('NI>1', 'HW'): ((128, 8, 30, 12, 3), 3),
    ('NI>1', 'T'): ((1, 24, 24, 48, 16), 3),
    ('NI>1', 'THW'): ((1, 24, 24, 48, 16), 3),
    ('NI>1', 'causalT'): ((2, 64, 30, 48, 3), 3),
    ('NI>1', 'causalTHW'): ((3, 16, 14, 48, 16), 3),
    ('T3', 'THW'): ((1, 8, 30, 9, 2), 3),
    ('T3', 'causalTHW'): ((1, 8, 30, 9, 2), 3),
    ('W3', 'THW'): ((1, 8, 8, 33, 2), 3),
    ('W3', 'causalTHW'): ((1, 8, 8, 33, 2), 3),
}
# (regime, T stencil, job): (shape, radius_t, radius_s)
ANISO_REGIME = {
    ('C3', 'causal', 'adj'): ((1, 8, 5, 8, 100), 3, 3),
    ('C3', 'causal', 'dsigma'): ((1, 8, 5, 8, 100), 3, 3),
    ('C3', 'causal', 'fwd'): ((1, 8, 5, 8, 100), 3, 3),
    ('C3', 'sym', 'adj'): ((1, 8, 8, 8, 100), 3, 3),
    ('C3', 'sym', 'dsigma'): ((1, 8, 8, 8, 100), 3, 3),
    ('C3', 'sym', 'fwd'): ((1, 8, 8, 8, 100), 3, 3),
    ('H3', 'causal', 'adj'): ((3, 9, 5, 8, 100), 3, 3),
    ('H3', 'causal', 'dsigma'): ((3, 9, 5, 8, 100), 3, 3),
    ('H3', 'causal', 'fwd'): ((3, 9, 5, 8, 100), 3, 3),
    ('H3', 'sym', 'adj'): ((3, 33, 9, 64, 2), 3, 3),
    ('H3', 'sym', 'dsigma'): ((3, 33, 9, 64, 2), 3, 3),
    ('H3', 'sym', 'fwd'): ((3, 33, 9, 64, 2), 3, 3),
    ('NI>1', 'causal', 'adj'): ((3, 12, 20, 48, 16), 3, 3),
    ('NI>1', 'causal', 'dsigma'): ((3, 12, 20, 48, 16), 3, 3),
    ('NI>1', 'causal', 'fwd'): ((3, 12, 20, 48, 16), 3, 3),
    ('NI>1', 'sym', 'adj'): ((3, 12, 20, 48, 16), 3, 3),
    ('NI>1', 'sym', 'dsigma'): ((3, 12, 20, 48, 16), 3, 3),
    ('NI>1', 'sym', 'fwd'): ((3, 12, 20, 48, 16), 3, 3),
    ('T3', 'causal', 'adj'): ((1, 8, 30, 9, 2), 3, 3),
    ('T3', 'causal', 'dsigma'): ((1, 8, 30, 9, 2), 3, 3),
    ('T3', 'causal', 'fwd'): ((1, 8, 30, 9, 2), 3, 3),
    ('T3', 'sym', 'adj'): ((1, 8, 30, 9, 2), 3, 3),
    ('T3', 'sym', 'dsigma'): ((1, 8, 30, 9, 2), 3, 3),
    ('T3', 'sym', 'fwd'): ((1, 8, 30, 9, 2), 3, 3),
    ('W3', 'causal', 'adj'): ((1, 8, 8, 33, 2), 3, 3),
    ('W3', 'causal', 'dsigma'): ((1, 8, 8, 33, 2), 3, 3),
    ('W3', 'causal', 'fwd'): ((1, 8, 8, 33, 2), 3, 3),
    ('W3', 'sym', 'adj'): ((1, 8, 8, 33, 2), 3, 3),
    ('W3', 'sym', 'dsigma'): ((1, 8, 8, 33, 2), 3, 3),
    ('W3', 'sym', 'fwd'): ((1, 8, 8, 33, 2), 3, 3),
}
# the cases above that lie outside BOX: found in WIDE_BOX, for what the planner picks at BASELINE
WIDE = {'dsigma': [], 'aniso': []}
# what the planner picks at BASELINE (radius 3, every form / job / causal setting)
BASELINE_PICKS = {'dsigma': [(3, 1), (3, 2), (3, 4), (3, 6), (3, 8)], 'aniso': [(3, 2, 'adj'), (3, 2, 'dsigma'), (3, 2, 'fwd'), (3, 4, 'adj'), (3, 4, 'dsigma'), (3, 4, 'fwd'), (3, 8, 'fwd')]}
# nameable, admitted by the constexpr limits, reached by no shape of the box searched for it
UNREACHED = {
    'dsigma': {
    },
    'aniso': {
    },
}
# the instantiations that the cases of test_gpu_smooth_sigma.py and test_gpu_aniso_smoothing.py reach, by the real
# planner: what the suite held to fp64 before this table
OLDER_GRIDS = {'dsigma': {'nameable': 43, 'reached': [(1, 1), (1, 2), (2, 1), (3, 1), (4, 1), (7, 1)]}, 'aniso': {'nameable': 72, 'reached': [(0, 1, 'adj'), (0, 1, 'dsigma'), (0, 1, 'fwd'), (1, 1, 'adj'), (1, 1, 'dsigma'), (1, 1, 'fwd'), (2, 1, 'adj'), (2, 1, 'dsigma'), (2, 1, 'fwd'), (3, 1, 'adj'), (3, 1, 'dsigma'), (3, 1, 'fwd'), (4, 1, 'adj'), (4, 1, 'dsigma'), (4, 1, 'fwd'), (7, 1, 'adj'), (7, 1, 'dsigma'), (7, 1, 'fwd')]}}
# ---- END GENERATED
