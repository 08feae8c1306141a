"""dsigma_tile and aniso_tile give the bits they gave before their shared pieces moved into csrc/tile_walk.h.

Both kernels promise "the same call gives the same bits" (no float atomics, fixed-order fp64 sums), so a refactoring is held to
EQUALITY with its parent, not to a tolerance: tests/golden/tile_walk_bits_parent.json holds one SHA-256 per case over the raw
output bytes, recorded on an MI355X at the commit before the move by tests/golden/make_tile_walk_bits.py, which calls case()
below.  The inputs are those of tests/test_gpu_tile_instantiations.py (which holds the same cases to float64): every case of
tile_plan_cases.DSIGMA_INST and ANISO_INST, so every instantiation the launch switches can name runs; the outputs of an
anisotropic case are out and mx (fwd), din (adj) and the two dsigma floats (dsigma).  On top: the sharded anisotropic backward
(STATS_ONLY, then EXTERNAL_STATS on two one-sample shards), a dsigma call with stats_in handed in, and the calls in which
tile_combine sees each mask setting and no partials at all (a radius of 0).  No oracle work: each case is a few kernel calls.

A DELIBERATE numerical change to either kernel (another summation order, another stencil form) re-records the file on the
commit that makes it; an accidental one fails here."""
import functools
import hashlib
import json
import os

import pytest
import torch

import smooth_aniso_oracle as ao
import test_gpu_aniso_smoothing as GA
import test_gpu_smooth_sigma as GS
import tile_plan_cases as tp

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tile_walk_bits_parent.json")
SIGMA = 1.3
SIGMA_T, SIGMA_S = 1.3, 2.0
SMALL = (2, 8, 9, 8, 1)


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def _sid(shape):
    return "x".join(map(str, shape))


@functools.lru_cache(maxsize=1)
def _ds_inputs(shape, r, form):
    x, g = GS._rand(shape, 61), GS._rand(shape, 62, normal=True)
    out, mx = GS._forward(x, SIGMA, r, form)
    return x, g, out, mx


@functools.lru_cache(maxsize=1)
def _an_inputs(shape, cfg):
    x, g = GA.video(shape, 12), GA.rand(shape, 13, normal=True)
    out, mx = GA.k_fwd(x, cfg)
    return x, g, out, mx


def _aniso(shape, rt, rs, causal, job):
    cfg = (SIGMA_T, SIGMA_S, rt, rs, causal)
    x, g, out, mx = _an_inputs(shape, cfg)
    if job == "fwd":
        return _sha(out, mx)
    if job == "adj":
        return _sha(GA.k_bwd(g, out, mx, cfg))
    return _sha(GA.k_dsigma(x, g, out, mx, cfg))


def _aniso_sharded_bwd():
    cfg = (SIGMA_T, SIGMA_S, 3, 3, False)
    x, g, out, mx = _an_inputs(SMALL, cfg)
    shards = [(g[b:b + 1].contiguous(), out[b:b + 1].contiguous()) for b in range(SMALL[0])]
    stats = []
    for gs, o in shards:
        st = torch.full((2,), float("nan"), device=GA.DEV)
        assert GA.k_bwd(gs, o, mx, cfg, st, ao.STATS_ONLY) is None
        stats.append(st)
    total = torch.stack(stats).sum(0)
    dins = [GA.k_bwd(gs, o, mx, cfg, total.clone(), ao.EXTERNAL_STATS) for gs, o in shards]
    return _sha(total, torch.cat(dins))


def _dsigma(shape, r, form, stats_in=False):
    x, g, out, mx = _ds_inputs(shape, r, form)
    stats = GS._stats(g, out, mx, SIGMA, r, form) if stats_in else None
    return _sha(GS._dsigma(x, g, out, mx, SIGMA, r, form, stats))


# name -> a thunk that returns the case's SHA-256; in the order of (shape, radii) so that the jobs of one forward follow each other
CASES = {}
for (_R, _NI), (_shape, _form) in sorted(tp.DSIGMA_INST.items()):
    CASES["dsigma R%d NI%d %s %s" % (_R, _NI, _form, _sid(_shape))] = functools.partial(_dsigma, _shape, _R, _form)
for (_RS, _NI, _job), (_shape, _rt, _causal) in sorted(tp.ANISO_INST.items(), key=lambda kv: (kv[1], kv[0][0], tp.JOBS.index(kv[0][2]))):
    CASES["aniso RS%d NI%d %s rt%d %s %s" % (_RS, _NI, _job, _rt, "causal" if _causal else "sym", _sid(_shape))] = \
        functools.partial(_aniso, _shape, _rt, _RS, _causal, _job)
CASES["aniso sharded bwd %s" % _sid(SMALL)] = _aniso_sharded_bwd
CASES["dsigma stats_in THW r3 %s" % _sid(SMALL)] = functools.partial(_dsigma, SMALL, 3, "THW", True)
CASES["dsigma radius 0 (no partials) %s" % _sid(SMALL)] = functools.partial(_dsigma, SMALL, 0, "THW")
# tile_combine's mask: the T component alone, the spatial one alone, both (every dsigma case above), and no launch at all
CASES["aniso dsigma rt3 rs0 %s" % _sid(SMALL)] = functools.partial(_aniso, SMALL, 3, 0, False, "dsigma")
CASES["aniso dsigma rt0 rs3 %s" % _sid(SMALL)] = functools.partial(_aniso, SMALL, 0, 3, False, "dsigma")
CASES["aniso dsigma rt0 rs0 (no partials) %s" % _sid(SMALL)] = functools.partial(_aniso, SMALL, 0, 0, False, "dsigma")
assert all(tp.elems(v[0]) <= tp.MAX_ELEMS for v in list(tp.DSIGMA_INST.values()) + list(tp.ANISO_INST.values()))


def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=1)
def _golden():
    return json.load(open(GOLDEN))


def test_the_golden_file_holds_exactly_the_cases():
    assert sorted(_golden()["sha256"]) == sorted(CASES) and len(CASES) == 43 + 72 + 6


@pytest.mark.parametrize("name", list(CASES))
def test_case_gives_the_parents_bits(name):
    assert case(name) == _golden()["sha256"][name], name
