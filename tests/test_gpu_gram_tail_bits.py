"""The four Gram paths of the cost assembly give the bits they gave before their shared tail moved into csrc/gram_tail.h.

Every kernel behind kccot_pairwise_cost3_f32, kccot_pairwise_cost_f32 and the row-block calls promises "the same call gives the
same bits" (fixed-order fp64 sums, no float atomics), so a refactoring is held to EQUALITY with its parent, not to a tolerance:
tests/golden/gram_tail_bits_parent.json holds one SHA-256 per case over the raw output bytes, recorded on an MI355X at the
commit before the move by tests/golden/make_gram_tail_bits.py, which calls case() below.  The inputs are _tile_inputs of
tests/test_gpu_parity.py (which holds the same paths to float64) with T = 5, J = 4.  The cases are the smallest shapes that
reach each instantiation and each branch of the shared code: the stack of 64 + 64 rows in its loss form (compact record, ragged
rows, a partial mask, the f32-input kernel's slab layout, no features) and its pairwise forms (x != y, x == y), the blocked form,
the 128-row and the 256-row tiles (one panel, ragged K, off-diagonal pairs, materialised difference rows), the row blocks of a
batch-sharded rank (every panel mix, first and last block, norms = NULL, the two-stage form over column ranges) and the split at
the fp64 Gram sums, whose result must ALSO equal the one-call result of the same case bit for bit.  No oracle work: each case
is a handful of launches.

A DELIBERATE numerical change to these kernels (another summation order, another distance formula) re-records the file on the
commit that makes it; an accidental one fails here."""
import ctypes
import functools
import hashlib
import json
import os

import pytest
import torch

import cases
import test_gpu_parity as GP

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gram_tail_bits_parent.json")
T, J = 5, 4


def _L():
    from kccotgan_amd import _lib
    return _lib


def _sha(*tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=2)
def _inputs(B, K):
    _L()                                                    # the package before the first device call
    return GP._tile_inputs(B, K, 9000 + B + K, T=T, J=J)


def _call3(real, fake, f, flags, C3, ws):
    L = _L()
    B, K = real.shape
    feats = [L.ptr(t) for t in f] if f else [None] * 4
    L.check(L.lib.kccot_pairwise_cost3_f32(L.ptr(real), L.ptr(fake), B, K, cases.SC, *feats, T, J, flags, L.ptr(C3), ws.data_ptr(),
                                           ws.numel(), None), "pairwise_cost3")


def _ws3(B, K):
    return torch.zeros(int(_L().lib.kccot_pairwise_cost3_workspace_bytes(B, K)), dtype=torch.uint8, device=GP.DEV)


def _cost3_tensor(B, K, opts, features=True):
    real, fake, f = _inputs(B, K)
    C3 = torch.full((3, B, B), float("nan"), device=GP.DEV)
    with _L().options(**dict(opts)):
        _call3(real, fake, f if features else None, 0, C3, _ws3(B, K))
    return C3


def _cost3(B, K, opts=(), features=True):
    return _sha(_cost3_tensor(B, K, opts, features))


def _split(B, K, opts=()):
    """SUMS_ONLY, then FROM_GRAM_SUMS: the doubles inside the reported span and the result, which is the one-call result"""
    L = _L()
    real, fake, f = _inputs(B, K)
    one = _cost3_tensor(B, K, opts)
    two, ws = torch.full((3, B, B), float("nan"), device=GP.DEV), _ws3(B, K)
    off, cnt = ctypes.c_size_t(0), ctypes.c_size_t(0)
    with L.options(**dict(opts)):
        L.check(L.lib.kccot_pairwise_cost3_gram_sums_span(B, K, ctypes.byref(off), ctypes.byref(cnt)), "span")
        assert cnt.value > 0 and off.value + 8 * cnt.value <= ws.numel()
        _call3(real, fake, f, L.COST_GRAM_SUMS_ONLY, two, ws)
        torch.cuda.synchronize()
        sums = ws[off.value:off.value + 8 * cnt.value].clone()
        _call3(real, fake, f, L.COST_FROM_GRAM_SUMS, two, ws)
    torch.cuda.synchronize()
    assert torch.equal(one, two), "the split result is not the one-call result"
    return _sha(sums, two)


def _pairwise(Bx, By, K, same):
    from kccotgan_amd import gan_utils as G
    real, fake, f = _inputs(max(Bx, By), K)
    x = real[:Bx].contiguous()
    y = x if same else fake[:By].contiguous()
    h1, M1, h2, M2 = f[0][:Bx].contiguous(), f[2][:By].contiguous(), f[1][:Bx].contiguous(), f[3][:By].contiguous()
    assert G.cost_flags == 0
    return _sha(G._PairwiseCost.apply(x, y, h1, M1, h2, M2, cases.SC))


def _rows(B, m, K, r0, own_norms=False):
    from kccotgan_amd.dist import HipOps as H
    L = _L()
    real, fake, f = _inputs(B, K)
    if not own_norms:
        return _sha(H.cost3_rows(real, fake, f[0], f[1], f[2], f[3], cases.SC, r0, m, H.row_norms(real, fake)))
    out = torch.full((3, m, B), float("nan"), device=GP.DEV)
    ws = torch.zeros(int(L.lib.kccot_pairwise_cost3_rows_gram_workspace_bytes(m, B, K)), dtype=torch.uint8, device=GP.DEV)
    L.check(L.lib.kccot_pairwise_cost3_rows_gram_f32(L.ptr(real), L.ptr(fake), B, K, cases.SC, L.ptr(f[0]), L.ptr(f[1]), L.ptr(f[2]),
                                                     L.ptr(f[3]), T, J, r0, m, None, L.ptr(out), ws.data_ptr(), ws.numel(), None), "rows_gram")
    return _sha(out)


def _rows_two_stage(B, m, K, r0):
    from kccotgan_amd.dist import HipOps as H, gather_chunk_bounds
    L = _L()
    real, fake, f = _inputs(B, K)
    bounds = gather_chunk_bounds(K, 4)
    assert len(bounds) == 4
    gsum = torch.full((int(L.lib.kccot_pairwise_cost3_rows_gram_sums_count(m, B)),), float("nan"), dtype=torch.float64, device=GP.DEV)
    for c, (a, b) in enumerate(bounds):
        H.rows_gram_sums(real[:, a:b].contiguous(), fake[:, a:b].contiguous(), r0, m, gsum, c > 0)
    return _sha(gsum, H.rows_gram_from_sums(gsum, B, f[0], f[1], f[2], f[3], cases.SC, r0, m, H.row_norms(real, fake)))


T128 = (("cost_tile256", 0),)
F32 = (("gram_f32", 1),)
P = functools.partial
# name -> a thunk that returns the case's SHA-256; cases that share their inputs follow each other
CASES = {
    "stack64 loss B=64 K=4100 (compact record)": P(_cost3, 64, 4100),
    "stack64 split B=64 K=4100": P(_split, 64, 4100),
    "stack64 loss B=64 K=4100 gram_f32=1 (slabs, SPLIT_89)": P(_cost3, 64, 4100, F32),
    "stack64 loss B=37 K=3076 (ragged rows)": P(_cost3, 37, 3076),
    "stack64 loss B=7 K=256 (partial mask)": P(_cost3, 7, 256),
    "stack64 loss B=64 K=512 no features": P(_cost3, 64, 512, (), False),
    "stack64 pairwise x!=y 48x64 K=516 both causal terms": P(_pairwise, 48, 64, 516, False),
    "stack64 pairwise x==y B=128 K=512 both causal terms": P(_pairwise, 128, 128, 512, True),
    "blocked B=192 K=512": P(_cost3, 192, 512),
    "tile128 B=128 K=2596 cost_tile256=0": P(_cost3, 128, 2596, T128),
    "tile128 split B=128 K=2596 cost_tile256=0": P(_split, 128, 2596, T128),
    "tile128 B=256 K=2560 cost_tile256=0": P(_cost3, 256, 2560, T128),
    "tile128 split B=256 K=2560 cost_tile256=0": P(_split, 256, 2560, T128),
    "tile128 B=384 K=1540": P(_cost3, 384, 1540),
    "tile128 split B=384 K=1540": P(_split, 384, 1540),
    "tile128 B=640 K=2596 (ediff_rows)": P(_cost3, 640, 2596),
    "tile256 B=128 K=2596 (one panel, ragged)": P(_cost3, 128, 2596),
    "tile256 split B=128 K=2596": P(_split, 128, 2596),
    "tile256 B=128 K=4096": P(_cost3, 128, 4096),
    "tile256 B=256 K=2560": P(_cost3, 256, 2560),
    "tile256 split B=256 K=2560": P(_split, 256, 2560),
    "tile256 B=256 K=2596": P(_cost3, 256, 2596),
    "tile256 B=512 K=3076 (off-diagonal pairs)": P(_cost3, 512, 3076),
    "tile256 B=768 K=1536": P(_cost3, 768, 1536),
}
for _B, _m, _K in ((128, 32, 1024), (256, 32, 2596), (384, 64, 1540), (512, 64, 3072)):
    for _r0 in (0, _B - _m):
        CASES["rows B=%d rows=%d K=%d row_begin=%d" % (_B, _m, _K, _r0)] = P(_rows, _B, _m, _K, _r0)
CASES["rows B=256 rows=32 K=2596 row_begin=224 norms=NULL"] = P(_rows, 256, 32, 2596, 224, True)
CASES["rows two-stage B=256 rows=64 K=4132 row_begin=64 (gsum and result)"] = P(_rows_two_stage, 256, 64, 4132, 64)


def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=1)
def _golden():
    return json.load(open(GOLDEN))


def test_the_golden_file_holds_exactly_the_cases():
    assert sorted(_golden()["sha256"]) == sorted(CASES) and len(CASES) == 24 + 8 + 2


def test_the_cases_take_the_paths_their_names_say():
    """the span of the fp64 sums names the path: the compact record of the 64 + 64 stack, 128 x 128 or 256 x 256 doubles per pair"""
    L = _L()

    def count(B, K, opts=()):
        off, cnt = ctypes.c_size_t(0), ctypes.c_size_t(0)
        with L.options(**dict(opts)):
            L.check(L.lib.kccot_pairwise_cost3_gram_sums_span(B, K, ctypes.byref(off), ctypes.byref(cnt)), "span")
        return cnt.value

    assert 0 < count(64, 4100) < count(64, 4100, F32) == 10 * 1024 == count(7, 256)
    assert count(192, 512) == 0                                                      # blocked: no split
    for B, K, opts in ((128, 2596, T128), (256, 2560, T128), (384, 1540, ()), (640, 2596, ())):
        nt = 2 * B // 128
        assert count(B, K, opts) == nt * (nt + 1) // 2 * 128 * 128
    for B, K in ((128, 2596), (128, 4096), (256, 2560), (256, 2596), (512, 3076), (768, 1536)):
        nt = max(1, 2 * B // 256)
        assert count(B, K) == nt * (nt + 1) // 2 * 256 * 256


@pytest.mark.parametrize("name", list(CASES))
def test_case_gives_the_parents_bits(name):
    assert case(name) == _golden()["sha256"][name], name
