"""The definition of include/kccot_swd.h transcribed in numpy: Philox4x32-10 in uint64 arithmetic, the directions, SW2 and its
closed-form gradients in float64 (also at a given matching), the input makers and the error caps of the GPU tests.  Not a test
module: pytest does not collect it."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two ints -> four uint64 arrays holding 32-bit words"""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def unit(r):
    return ((r >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def directions(seed, K, p_begin, p_count):
    """[p_count, K] float64: the raw directions p_begin .. p_begin + p_count - 1"""
    nq = (K + 3) // 4
    q = np.arange(nq, dtype=np.uint64)[None, :]
    p = np.arange(p_begin, p_begin + p_count, dtype=np.uint64)[:, None]
    r = philox4x32_10((q & MASK, q >> np.uint64(32), p, 0), (seed & 0xFFFFFFFF, seed >> 32))
    z = np.empty((p_count, nq, 4))
    for a in (0, 2):
        rad, ang = np.sqrt(-2.0 * np.log(unit(r[a]))), 2.0 * np.pi * unit(r[a + 1])
        z[:, :, a], z[:, :, a + 1] = rad * np.cos(ang), rad * np.sin(ang)
    return z.reshape(p_count, 4 * nq)[:, :K]


def unit_directions(seed, K, P):
    th = directions(seed, K, 0, P)
    return th / np.sqrt((th * th).sum(1, keepdims=True))


def projections(real, fake, seed, P):
    """(a [B,P], b [B,P], theta^ [P,K]) in float64"""
    th = unit_directions(seed, real.shape[1], P)
    return real.astype(np.float64) @ th.T, fake.astype(np.float64) @ th.T, th


def stable_order(v):
    """[B,P] -> [P,B]: the sample index at every rank, ties to the lower index"""
    return np.argsort(v.T, axis=1, kind="stable")


def sw2(real, fake, seed, P):
    a, b, _ = projections(real, fake, seed, P)
    d = np.sort(a, axis=0) - np.sort(b, axis=0)
    return float((d * d).sum() / (P * real.shape[0]))


def sw2_torch(real, fake, th):
    """The same value as a differentiable torch float64 expression of real and fake (th: unit directions [P,K])"""
    import torch
    d = torch.sort(real @ th.T, dim=0, stable=True)[0] - torch.sort(fake @ th.T, dim=0, stable=True)[0]
    return (d * d).sum() / (th.shape[0] * real.shape[0])


def gradients(real, fake, seed, P, g=1.0, order=None):
    """(dreal, dfake) [B,K] float64 at the oracle's own stable matching, or at `order` [2,P,B] (sample index at every rank)"""
    a, b, th = projections(real, fake, seed, P)
    B = real.shape[0]
    oa, ob = (stable_order(a), stable_order(b)) if order is None else (np.asarray(order[0]), np.asarray(order[1]))
    da, db = np.zeros_like(a), np.zeros_like(b)
    cols = np.arange(P)[:, None]
    d = a.T[cols, oa] - b.T[cols, ob]                          # [P,B] by rank
    da.T[cols, oa] = 2.0 * g / (P * B) * d
    db.T[cols, ob] = -2.0 * g / (P * B) * d
    return da @ th, db @ th


def min_gap(real, fake, seed, P):
    """The smallest adjacent gap of the sorted projections of either batch, relative to that projection's range"""
    worst = np.inf
    for v in projections(real, fake, seed, P)[:2]:
        s = np.sort(v, axis=0)
        if s.shape[0] > 1:
            worst = min(worst, float((np.diff(s, axis=0) / (s[-1] - s[0])).min()))
    return worst


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def make(kind, B, K, s):
    """(real, fake, direction seed).  "noise": fake = clip(real + 0.05 N(0,1)); "ties": values on a 1/8 grid, row 2 a copy of row 1 in
    both batches (tied projections inside a batch), every third row of fake bit-equal to the same row of real"""
    rng = np.random.default_rng(s)
    if kind == "noise":
        real = rng.random((B, K), dtype=np.float32)
        fake = np.clip(real + np.float32(0.05) * rng.standard_normal((B, K)).astype(np.float32), 0, 1).astype(np.float32)
    else:
        real = (rng.integers(0, 9, (B, K)) / 8.0).astype(np.float32)
        fake = (rng.integers(0, 9, (B, K)) / 8.0).astype(np.float32)
        if B > 2:
            real[2], fake[2] = real[1], fake[1]
        fake[::3] = real[::3]
    return real, fake, s + 100


# (B, K, P, data seed) of the "noise" cases that the GPU tests compare with the oracle's OWN sort: tests/test_swd_cpu.py asserts
# that their adjacent gaps are >= MIN_GAP of the projection's range
GAPPED = [(8, 1023, 16, s) for s in range(4)] + [(8, 2052, 33, s) for s in range(3)]
MIN_GAP = 1e-4


# ---- caps --------------------------------------------------------------------------------------------------------------------------
DIR_CAP = 1e-5            # |z| <= 5.77, the angle rounded to <= 2^-22 rad, a few ulp of log, sqrt, sin and cos
SW2_CAP = 1e-4            # the project's bar for a loss
GRAD_CAP = 2.5e-5         # the project's gradient bar, of max|ref|


def proj_cap(x, seed, P, kc):
    """[B,P]: (adds per chunk + 4) 2^-24 sum_k |x_k| |theta^_k| + DIR_CAP sum_k |x_k| / |theta_p|"""
    th = directions(seed, x.shape[1], 0, P)
    nrm = np.sqrt((th * th).sum(1))
    ax = np.abs(x.astype(np.float64))
    return (min(kc, x.shape[1]) + 4) * 2.0 ** -24 * (ax @ np.abs(th / nrm[:, None]).T) + DIR_CAP * ax.sum(1)[:, None] / nrm[None, :]
