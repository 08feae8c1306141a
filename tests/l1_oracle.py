"""The definition of include/kccot_l1.h transcribed in torch: the L1 cost block, the closed-form adjoints, the input makers, and the
bounds of the GPU tests (tests/test_gpu_l1_cost.py).  Not a test module: pytest does not collect it.  Everything runs on the
device and in the dtype of its inputs (the GPU tests feed it float64 on the GPU); the causal terms and the solver of the loss
tests are oracle.gan_utils_torch's (CPU, float64)."""
import torch

U = 2.0 ** -24          # unit roundoff of float32

# ---- the shapes of the GPU tests ------------------------------------------------------------------------------------------------
# forward: the direct kernel's own boundaries (RA = 1, 2, 4, 8 at 16, 32, 64 rows and above; 64-column tiles; a k-tile of 32;
# vector loads only with K % 4 == 0 and a 16-byte aligned base; more than 48 chunks take cost_reduce_chunks).  offset: x and y
# begin one float into their storage.
FWD_SHAPES = [(1, 1, 1, 0), (3, 5, 7, 0), (16, 17, 70, 0), (33, 64, 128, 0), (64, 64, 1600, 0), (65, 130, 100, 0), (8, 8, 64, 1)]
SAME_SHAPES = [(17, 36), (130, 68)]
T, J = 6, 3
VIDEO = (4, 6, 5, 1)    # [B,4,6,5,1]: K = 120
COST3_B = [2, 8, 64, 70]
IT = 2                  # context frames of the "ties" videos
# backward: the forward's shapes plus the boundaries of l1_sign_apply's own tiling -- the row group of 8 (7, 8, 9 target rows),
# the column tile of 1024 (1023, 1024, 1028 columns: a k tail with and without vector loads, a second column tile) and an
# unaligned base (offset 1), and source counts around the 4 rows in flight (3, 4, 5)
BWD_SHAPES = FWD_SHAPES + [(7, 3, 1023, 0), (8, 4, 1024, 0), (9, 5, 1028, 0), (9, 4, 1028, 1), (5, 9, 2052, 0)]
BWD_SAME = SAME_SHAPES + [(9, 1028)]
BWD_COST3 = [(2, 120), (8, 120), (64, 120), (70, 120), (9, 1028), (5, 1023)]

# The longest fp32 chain of the forward at these shapes: every shape has few output tiles, so plan_direct cuts K into chunks of
# ONE k-tile (32 columns).  A thread then adds 16 terms into each half of its packed accumulator (15 roundings: the first add
# to +0 is exact), each term carrying the rounding of its difference (1), and adds the two halves (1): n = 17.  The chunks are
# summed in fp64, rounded once to fp32 (1) and multiplied by sc (1).  All terms are non-negative, so |C - ref| <= (n + 2) u ref.
FWD_CHAIN = 17
CAP_FWD = (FWD_CHAIN + 2) * U


def fwd_chunk(K):
    """The chunk plan_direct picks at the shapes above (few tiles: as many chunks as k-tiles, up to 1024)"""
    assert (K + 31) // 32 <= 1024
    return 32


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def rows(kind, Bx, By, K, seed, device="cpu", offset=0):
    """x [Bx,K], y [By,K] float32.  "noise": uniform.  "ties": multiples of 1/8 in [0, 1], so that different samples tie often.
    offset: the tensors are views that begin `offset` floats into their storage (an unaligned base)."""
    g = _gen(seed)
    out = []
    for n in (Bx, By):
        v = torch.rand((n * K + offset,), generator=g)
        if kind == "ties":
            v = torch.round(v * 8.0) / 8.0
        out.append(v.to(device)[offset:].view(n, K))
    return out


def videos(kind, B, seed, device="cpu", shape=VIDEO):
    """real, fake [B,H,T,W,C] float32; "ties": values on the 1/8 grid and fake[:, :, :IT] = real[:, :, :IT] bit for bit (the
    trainer's fake = cat(real_in, fake_pred): the context frames of sample i tie in the xy term at i = j)."""
    K = 1
    for d in shape:
        K *= d
    real, fake = (v.view(B, *shape).clone() for v in rows(kind, B, B, K, seed))
    if kind == "ties":
        fake[:, :, :IT] = real[:, :, :IT]
    return real.to(device), fake.to(device)


def context_mask(B, shape=VIDEO):
    """[B,K] bool: the flattened positions of the context frames"""
    m = torch.zeros((B, *shape), dtype=torch.bool)
    m[:, :, :IT] = True
    return m.view(B, -1)


def features(B, seed, device="cpu"):
    """h_fake, h_real, m_real, m_fake [B,T,J] float32"""
    g = _gen(seed)
    return [(torch.rand((B, T, J), generator=g) - 0.5).to(device) for _ in range(4)]


def upstream(shape, seed, device="cpu"):
    """g of both signs"""
    return (torch.rand(shape, generator=_gen(seed)) - 0.5).to(device)


# ---- the definition -------------------------------------------------------------------------------------------------------------
def l1_block(x, y, sc, rows_per_step=16):
    """C[i,j] = sc * sum_k |x[i,k] - y[j,k]|"""
    out = []
    for i0 in range(0, x.shape[0], rows_per_step):
        out.append((x[i0:i0 + rows_per_step, None, :] - y[None, :, :]).abs().sum(-1))
    return torch.cat(out) * sc


def _sgn_sum(W, a, S, rows_per_step=16):
    """out[r,k] = sum_c W[r,c] sgn(a[r,k] - S[c,k]), torch.sign(0) = 0"""
    out = []
    for r0 in range(0, a.shape[0], rows_per_step):
        sg = torch.sign(a[r0:r0 + rows_per_step, None, :] - S[None, :, :])
        out.append((W[r0:r0 + rows_per_step, :, None] * sg).sum(1))
    return torch.cat(out)


def adjoint_x(g, x, y, sc):
    return sc * _sgn_sum(g, x, y)


def adjoint_y(g, x, y, sc):
    return sc * _sgn_sum(g.t(), y, x)


def adjoint_same(g, x, sc):
    return sc * _sgn_sum(g + g.t(), x, x)


def adjoint_fake(g3, real, fake, sc):
    """dfake of the loss form; real, fake [B,K]"""
    return sc * (_sgn_sum(g3[0].t(), fake, real) + _sgn_sum(g3[2] + g3[2].t(), fake, fake))


def coef_abs_rowsum_max(form, g):
    """max_r sum_c |W[r,c]| of the coefficient matrix of one form ("x", "y", "same", "fake"), in float64"""
    g = g.double()
    W = {"x": lambda: g, "y": lambda: g.t(), "same": lambda: g + g.t(),
         "fake": lambda: torch.cat((g[0].t(), g[2] + g[2].t()), dim=1)}[form]()
    return float(W.abs().sum(1).max())


def bwd_cap(form, g, ref, sc):
    """N 2^-24 max_r sum_c |sc W[r,c]| / max|ref| for ref = sc * (the sum): the N - 1 sequential fp32 additions of terms +-W and
    the product with sc are N roundings, each of at most 2^-24 of sum_c |W[r,c]|.  (A two-term coefficient carries the rounding
    of its sum, and its form has one source that ties everywhere -- the row itself -- and adds nothing.)"""
    N = {"x": g.shape[-1], "y": g.shape[-2], "same": g.shape[-1], "fake": 2 * g.shape[-1]}[form]
    return N * U * sc * coef_abs_rowsum_max(form, g) / float(ref.abs().max())


def f32(v):
    """v rounded to float32, as a Python float (the scaling coefficient the kernels receive)"""
    return float(torch.tensor(v, dtype=torch.float32))


def fp32_forward_like_the_kernel(x, y, sc, chunk):
    """A plain float32 evaluation in the kernel's chunk shape: per chunk two sequential float32 sums (even and odd pairs of
    columns as the packed accumulator holds them), added; the chunks added in float64, rounded once, times sc."""
    Bx, K = x.shape
    tot = torch.zeros((Bx, y.shape[0]), dtype=torch.float64)
    for k0 in range(0, K, chunk):
        d = (x[:, None, k0:k0 + chunk] - y[None, :, k0:k0 + chunk]).abs()      # float32
        lo = torch.zeros_like(tot, dtype=torch.float32)
        hi = torch.zeros_like(lo)
        for k in range(d.shape[-1]):
            if k % 2 == 0:
                lo = lo + d[..., k]
            else:
                hi = hi + d[..., k]
        tot += (lo + hi).double()
    return tot.float() * torch.tensor(sc, dtype=torch.float32)
