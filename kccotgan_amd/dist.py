"""Batch-sharded evaluation of compute_sinkhorn_loss over the GPUs of one node (one process per
GPU, torch.distributed over RCCL/xGMI).  The reference has no distributed code at all
(SURVEY.md section 5); this is the new design of SURVEY.md section 8(e):

  1. every rank owns B/G samples of real / fake and of the four feature tensors;
  2. ALL-GATHER the video shards and the (KB-sized) features -> every rank holds [B,K] of both;
  3. rank g builds the ROW BLOCKS C_xy[I_g,:], C_xx[I_g,:], C_yy[I_g,:] ([B/G, B] each) -- on the matrix pipe
     (csrc/cost_rows.hip) when it owns 32 or 64 samples and B % 128 == 0: the Gram row block [X_I ; E_I][X ; E]^T plus the
     all-gathered row norms x.x, e.e, x.e (3 doubles per sample); on the direct-difference kernel otherwise;
  4. ALL-GATHER the row blocks (3*B*B*4 bytes in total) -> the full cost matrices, replicated;
  5. every rank runs the identical (deterministic) Sinkhorn forward and reverse sweep: the loss
     and dLoss/dC are bitwise the same everywhere, no communication;
  6. rank g forms the gradients of ITS samples from the replicated dLoss/dC and the gathered
     videos (kccot_pairwise_cost3_bwd_rows_f32): NO reduce-scatter of video-sized gradients.

sharded_bicausal_sinkhorn_loss is the same for the bi-causal loss (gan_utils.compute_bicausal_sinkhorn_loss): after step 4
(or the ksplit finalize) every rank adds the second causal term of each matrix to its replicated C3 (one launch,
KCCOT_COST_BICAUSAL_TERM_ONLY); step 6 keeps the video gradient and forms the feature gradients with the bi-causal table.

sharded_mixed_sinkhorn_loss is the mixed divergence over two minibatches (gan_utils.compute_mixed_sinkhorn_loss, DESIGN.md
section 10.1): the four videos are gathered into the stacked R = [x; x'], F = [y; y'] of the single-GPU loss; at B <= 64
every rank runs the single-GPU loss call itself, above that rank g builds its rows of the four cost matrices from two
row-block calls on the stacked problem (rows g B/G and B + g B/G), adds their causal terms (KCCOT_COST_CAUSAL_ADD), and
the gathered Cmix goes to the solves (KCCOT_MIXED_CMIX_GIVEN).

sharded_rbf_mmd2 is the RBF-kernel MMD of the global batch (mmd.rbf_mmd2): the same gathers and
row blocks of plain squared distances, then each rank turns its three [B/G, B] blocks into kernel values and fp64 sums
(KCCOT_COST_RBF_SUM) and the 3 doubles are all-reduced; it can reuse the videos a sharded loss has already gathered.

The returned loss is the GLOBAL-batch loss (identical on every rank).  Parameter gradients that
flow back through a rank's local samples are therefore partial sums: combine them with an
all-reduce SUM (not the mean DistributedDataParallel applies by default).

The arithmetic is done by the HIP library (``HipOps``).  ``ops`` is injectable so that the
sharding / collective logic can be exercised over gloo on a CPU-only box by the tests (which plug
in the CPU oracle there); the product never does.
"""
import os

import torch
import torch.distributed as dist

from . import _lib
from . import gan_utils
from ._lib import lib, check, ptr, stream_of, workspace

_THRESH = 10 ** (-2)
_LMIN = 100

last_info = {}   # executed Sinkhorn iteration counts of the latest sharded evaluation (device tensor)


class _Phases:
    """Optional per-phase device timing of the sharded step (bench.py's N > 1 blocks: gathers, row block, Sinkhorn, gradient
    rows -- DESIGN.md section 6's table, measured).  Off by default: `phase_timing(True)` makes the autograd functions below
    drop a HIP event on the current stream at every phase boundary (a collective issued without async_op makes the current
    stream wait for it, so the interval that ENDS at a boundary holds the phase's transfers and kernels in stream order);
    `phase_ms()` synchronises and returns {phase: ms since the previous boundary}, summed over the steps recorded since the
    last call, plus "steps"."""
    enabled = False
    marks = []

    @classmethod
    def mark(cls, name):
        if cls.enabled and torch.cuda.is_available():
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            cls.marks.append((name, e))


def phase_timing(on):
    _Phases.enabled = bool(on)
    _Phases.marks = []


def phase_ms():
    torch.cuda.synchronize()
    out, steps, prev = {}, 0, None
    for name, e in _Phases.marks:
        if name == "start":
            steps += 1
        elif prev is not None:
            out[name] = out.get(name, 0.0) + prev.elapsed_time(e)
        prev = e
    _Phases.marks = []
    out["steps"] = steps
    return out


_mark = _Phases.mark


class HipOps:
    """The four device operations of the sharded path, through the C-ABI."""

    @staticmethod
    def cost_rows(x_rows, y_full, h_rows, M_full, sc):
        Bx, K = x_rows.shape
        By = y_full.shape[0]
        T, J = h_rows.shape[1], h_rows.shape[2]
        C = _lib.empty((Bx, By), torch.float32, x_rows.device)
        ws, wsb = workspace(lib.kccot_pairwise_cost_workspace_bytes(Bx, By, K), x_rows)
        # row blocks pair sample i with ALL samples j, so the pair-difference stack of the fused
        # single-GPU kernel does not apply; the direct-difference kernel keeps the small distances of
        # the GAN regime exact (a rank only builds B/G rows, the VALU rate is ample)
        check(lib.kccot_pairwise_cost_f32(ptr(x_rows), ptr(y_full), Bx, By, K, sc, ptr(h_rows), ptr(M_full), None, None,
                                          T, J, _lib.COST_FORCE_DIRECT, ptr(C), ws, wsb, stream_of(x_rows)),
              "pairwise_cost")
        return C

    @staticmethod
    def rows_gram_supported(row_count, B, K):
        """The row block on the matrix pipe (kccot_pairwise_cost3_rows_gram_f32): 32 or 64 rows per rank, B % 128 == 0.
        Depends on (row_count, B, K) and the process-wide options only, so all ranks agree."""
        return bool(lib.kccot_pairwise_cost3_rows_gram_supported(int(row_count), int(B), int(K)))

    @staticmethod
    def row_norms(real_l, fake_l):
        """x.x, e.e, x.e (e = fake - real) of this rank's rows, [Bl,3] float64 -- the column-side diagonal Gram entries every
        other rank's row block needs (all-gathered by the caller: 24 bytes per sample)."""
        Bl, K = real_l.shape
        out = _lib.empty((Bl, 3), torch.float64, real_l.device)
        ws, wsb = workspace(lib.kccot_row_norms_workspace_bytes(Bl), real_l)
        check(lib.kccot_row_norms_f64(ptr(real_l), ptr(fake_l), Bl, K, _lib.ptr_f64(out), ws, wsb, stream_of(real_l)), "row_norms")
        return out

    @staticmethod
    def cost3_rows(real, fake, h_fake, h_real, m_real, m_fake, sc, row_begin, row_count, norms=None):
        """Row blocks [3, row_count, B] of (xy, xx, yy): on the matrix pipe when the gathered `norms` [B,3] are given
        (kccot_pairwise_cost3_rows_gram_f32), else one launch of the direct-difference kernel
        (kccot_pairwise_cost3_rows_f32)."""
        B, K = real.shape
        T, J = h_fake.shape[1], h_fake.shape[2]
        out = _lib.empty((3, row_count, B), torch.float32, real.device)
        if norms is not None:
            ws, wsb = workspace(lib.kccot_pairwise_cost3_rows_gram_workspace_bytes(row_count, B, K), real)
            check(lib.kccot_pairwise_cost3_rows_gram_f32(ptr(real), ptr(fake), B, K, sc, ptr(h_fake), ptr(h_real), ptr(m_real),
                                                         ptr(m_fake), T, J, row_begin, row_count, _lib.ptr_f64(norms.contiguous()),
                                                         ptr(out), ws, wsb, stream_of(real)), "pairwise_cost3_rows_gram")
            return out
        ws, wsb = workspace(lib.kccot_pairwise_cost3_rows_workspace_bytes(row_count, B, K), real)
        check(lib.kccot_pairwise_cost3_rows_f32(ptr(real), ptr(fake), B, K, sc, ptr(h_fake), ptr(h_real), ptr(m_real),
                                                ptr(m_fake), T, J, row_begin, row_count, ptr(out), ws, wsb,
                                                stream_of(real)), "pairwise_cost3_rows")
        return out

    @staticmethod
    def rows_gram_sums(real_c, fake_c, row_begin, row_count, gsum, accumulate):
        """fp64 Gram sums of the rank's row block over ONE column range (real_c, fake_c: [B, Kc] of all samples), written to
        or added to `gsum` (kccot_pairwise_cost3_rows_gram_sums_f64)."""
        B, Kc = real_c.shape
        ws, wsb = workspace(lib.kccot_pairwise_cost3_rows_gram_workspace_bytes(row_count, B, Kc), real_c)
        check(lib.kccot_pairwise_cost3_rows_gram_sums_f64(ptr(real_c), ptr(fake_c), B, Kc, row_begin, row_count, _lib.ptr_f64(gsum),
                                                          1 if accumulate else 0, ws, wsb, stream_of(real_c)), "rows_gram_sums")

    @staticmethod
    def rows_gram_from_sums(gsum, B, h_fake, h_real, m_real, m_fake, sc, row_begin, row_count, norms):
        T, J = h_fake.shape[1], h_fake.shape[2]
        out = _lib.empty((3, row_count, B), torch.float32, gsum.device)
        check(lib.kccot_pairwise_cost3_rows_gram_from_sums_f32(_lib.ptr_f64(gsum), B, sc, ptr(h_fake), ptr(h_real), ptr(m_real), ptr(m_fake),
                                                               T, J, row_begin, row_count, _lib.ptr_f64(norms.contiguous()), ptr(out),
                                                               stream_of(gsum)), "rows_gram_from_sums")
        return out

    @staticmethod
    def replicate_costs(B, K):
        """Batches of at most 64: every rank assembles the WHOLE [3,B,B] with the one-pass MFMA kernels (31 us at
        configs[1]) instead of its row block on the direct kernel (46-100 us) followed by another all-gather --
        cheaper, one collective fewer, and the same pair-difference arithmetic as the single-GPU loss.  Larger batches
        keep the row blocks (cost ~ B^2 K / G).  KCCOT_DIST_ROW_BLOCKS=1 forces the row-block protocol (tests, A/B).
        The choice depends on (B, K) only, so all ranks agree."""
        return B <= 64 and K % 4 == 0 and K >= 256 and os.environ.get("KCCOT_DIST_ROW_BLOCKS") != "1"

    @staticmethod
    def cost3_full(real, fake, h_fake, h_real, m_real, m_fake, sc):
        B, K = real.shape
        T, J = h_fake.shape[1], h_fake.shape[2]
        C3 = _lib.empty((3, B, B), torch.float32, real.device)
        ws, wsb = workspace(lib.kccot_pairwise_cost3_workspace_bytes(B, K), real)
        check(lib.kccot_pairwise_cost3_f32(ptr(real), ptr(fake), B, K, sc, ptr(h_fake), ptr(h_real), ptr(m_real),
                                           ptr(m_fake), T, J, 0, ptr(C3), ws, wsb, stream_of(real)), "pairwise_cost3")
        return C3

    @staticmethod
    def sinkhorn3_fwd(C3, eps, L):
        nprob, n, _ = C3.shape
        dev = C3.device
        Lh = max(int(L), 1)
        u_hist = _lib.empty((nprob, Lh, n), torch.float32, dev)
        v_hist = _lib.empty((nprob, Lh, n), torch.float32, dev)
        cost = _lib.empty((nprob,), torch.float32, dev)
        nits = _lib.empty((2 * nprob,), torch.int32, dev)
        ws, wsb = workspace(lib.kccot_sinkhorn_workspace_bytes(nprob, n), C3)
        check(lib.kccot_sinkhorn_fwd_f32(ptr(C3), nprob, n, float(eps), int(L), _LMIN, _THRESH, _lib.STOP_COUNT,
                                         ptr(u_hist), ptr(v_hist), ptr(cost), ptr(nits), None, ws, wsb,
                                         stream_of(C3)), "sinkhorn_fwd")
        return cost, (C3, u_hist, v_hist, nits, float(eps), Lh)

    @staticmethod
    def sinkhorn3_bwd(saved, gcost3):
        C3, u_hist, v_hist, nits, eps, Lh = saved
        nprob, n, _ = C3.shape
        dC3 = _lib.empty_like(C3)
        ws, wsb = workspace(lib.kccot_sinkhorn_workspace_bytes(nprob, n), C3)
        check(lib.kccot_sinkhorn_bwd_f32(ptr(C3), ptr(u_hist), ptr(v_hist), ptr(nits), nprob, n, eps, Lh,
                                         ptr(gcost3.contiguous()), ptr(dC3), ws, wsb, stream_of(C3)), "sinkhorn_bwd")
        return dC3

    @staticmethod
    def divergence_fwd(C3, eps, L):
        """The three solves AND 2 xy - xx - yy in one launch (n <= 128; larger n: two launches inside the library)."""
        small, _, saved = gan_utils._divergence_fwd(C3, eps, L, _LMIN)
        return small[3:].reshape(()), saved

    @staticmethod
    def divergence_bwd(saved, g):
        return gan_utils._divergence_bwd(saved, g)

    @staticmethod
    def cost3_bwd_rows(dC3, real, fake, h_fake, h_real, m_real, m_fake, sc, row_begin, row_count):
        B, K = real.shape
        T, J = h_fake.shape[1], h_fake.shape[2]
        dev = real.device
        dfake = _lib.empty((row_count, K), torch.float32, dev)
        dhf, dhr, dmr, dmf = (_lib.empty((row_count, T, J), torch.float32, dev) for _ in range(4))
        ws, wsb = workspace(lib.kccot_pairwise_cost3_bwd_workspace_bytes(B, K), real)
        check(lib.kccot_pairwise_cost3_bwd_rows_f32(ptr(dC3), ptr(real), ptr(fake), B, K, sc, ptr(h_fake), ptr(h_real),
                                                    ptr(m_real), ptr(m_fake), T, J, row_begin, row_count, ptr(dfake),
                                                    ptr(dhf), ptr(dhr), ptr(dmr), ptr(dmf), ws, wsb, stream_of(real)),
              "pairwise_cost3_bwd_rows")
        return dfake, dhf, dhr, dmr, dmf

    # ---- the bi-causal loss (gan_utils.compute_bicausal_sinkhorn_loss) ----
    @staticmethod
    def dfake_rows(dC3, real, fake, sc, row_begin, row_count):
        """The video gradient of this rank's rows alone (kccot_pairwise_cost3_bwd_rows_f32, feature pointers NULL): the
        bi-causal loss changes only the causal terms, so its distance part -- and this gradient -- is the one-batch loss's."""
        B, K = real.shape
        dfake = _lib.empty((row_count, K), torch.float32, real.device)
        ws, wsb = workspace(lib.kccot_pairwise_cost3_bwd_workspace_bytes(B, K), real)
        check(lib.kccot_pairwise_cost3_bwd_rows_f32(ptr(dC3), ptr(real), ptr(fake), B, K, sc, None, None, None, None, 1, 1,
                                                    row_begin, row_count, ptr(dfake), None, None, None, None, ws, wsb,
                                                    stream_of(real)), "pairwise_cost3_bwd_rows")
        return dfake

    @staticmethod
    def bicausal_term(C3, h_fake, h_real, m_real, m_fake, sc):
        """The replicated one-batch C3 [3,B,B] -> the bi-causal cost matrices, in place: the second causal term of each
        matrix (KCCOT_COST_BICAUSAL_TERM_ONLY: the launch and summation order of the single-GPU loss)."""
        B = C3.shape[1]
        T, J = h_fake.shape[1], h_fake.shape[2]
        check(lib.kccot_pairwise_cost3_f32(None, None, B, 0, sc, ptr(h_fake), ptr(h_real), ptr(m_real), ptr(m_fake), T, J,
                                           _lib.COST_BICAUSAL_TERM_ONLY, ptr(C3), None, 0, stream_of(C3)),
              "pairwise_cost3(bi-causal term)")
        return C3

    @staticmethod
    def bicausal_feature_grads(dC3, real, fake, h_fake, h_real, m_real, m_fake, sc, row_begin, row_count, whole=False):
        """dh_fake, dh_real, dm_real, dm_fake of this rank's rows under the bi-causal job table (include/kccot.h).  They are
        products of the replicated dC3 with the gathered features, formed for all B samples and sliced.
        whole=True (replicated assembly, B <= 64): ONE launch, the single-GPU loss's backward with dC3 as its unit gradient
        and no video gradient (its workspace, of the size the replicated cost assembly already holds).  Otherwise one
        kccot_pairwise_cost_bwd_f32 per causal term with dx = dy = NULL (no workspace at all; the weight 2 of the xx / yy
        terms folded into sc), and the two terms of each gradient added: the row-block and ksplit paths allocate nothing
        that grows with K."""
        B, K = real.shape
        T, J = h_fake.shape[1], h_fake.shape[2]
        dev, st = real.device, stream_of(real)
        feats = (ptr(h_fake), ptr(h_real), ptr(m_real), ptr(m_fake))
        if whole:
            df = _lib.empty((4, B, T, J), torch.float32, dev)
            ws, wsb = workspace(lib.kccot_bicausal_sinkhorn_loss_workspace_bytes(B, K), real)
            # eps / L are only checked on this path: the solves' state is not read after a fused forward
            check(lib.kccot_bicausal_sinkhorn_loss_bwd_f32(ptr(_one(dev)), ptr(real), ptr(fake), B, K, sc, *feats, T, J, 1.0, 0,
                                                           None, None, None, None, ptr(dC3), None, *(ptr(d) for d in df),
                                                           ws, wsb, st), "bicausal_sinkhorn_loss_bwd(feature gradients)")
        else:
            part = _lib.empty((2, 4, B, T, J), torch.float32, dev)     # [term][dh_fake, dh_real, dm_real, dm_fake]
            #        g    rows h  cols M  weight  dh slot    dM slot
            for p, h, M, w, sh, sm in ((0, h_fake, m_real, 1.0, (0, 0), (0, 2)), (0, h_real, m_fake, 1.0, (0, 1), (0, 3)),
                                       (1, h_real, m_real, 2.0, (1, 1), (1, 2)), (2, h_fake, m_fake, 2.0, (1, 0), (1, 3))):
                check(lib.kccot_pairwise_cost_bwd_f32(ptr(dC3[p]), ptr(real), ptr(fake), B, B, K, sc * w, ptr(h), ptr(M), T, J, 0,
                                                      None, None, ptr(part[sh]), ptr(part[sm]), None, 0, st),
                      "pairwise_cost_bwd(bi-causal term)")
            df = part[0] + part[1]
        return tuple(df[i, row_begin:row_begin + row_count] for i in range(4))

    # ---- the mixed divergence over two minibatches (gan_utils.compute_mixed_sinkhorn_loss) ----
    @staticmethod
    def _mixed_state(B, L, keep, dev):
        """Output buffers of one mixed forward: costs | loss, iteration counts, and dCmix_unit (fused solve + sweep) or the
        dual history -- the single-GPU loss's choice (gan_utils._SinkhornLoss)."""
        Lh = max(int(L), 1)
        fused = bool(keep and lib.kccot_sinkhorn_fused_eligible(B, int(L)))
        st = {"small": _lib.empty((5,), torch.float32, dev), "nits": _lib.empty((8,), torch.int32, dev), "fused": fused,
              "Lh": Lh, "dCu": None, "uh": None, "vh": None}
        if fused:
            st["dCu"] = _lib.empty((4, B, B), torch.float32, dev)
        elif keep:
            st["uh"], st["vh"] = _lib.empty((4, Lh, B), torch.float32, dev), _lib.empty((4, Lh, B), torch.float32, dev)
        return st

    @staticmethod
    def _mixed_fwd(R, F, B, K, sc, feats, T, J, eps, L, flags, Cmix, st, ws, wsb):
        small = st["small"]
        check(lib.kccot_mixed_sinkhorn_loss_fwd_f32(R, F, B, K, sc, *feats, T, J, float(eps), int(L), _LMIN, _THRESH, flags,
                                                    ptr(Cmix), ptr(st["uh"]), ptr(st["vh"]), ptr(st["dCu"]), ptr(small),
                                                    ptr(st["nits"]), ptr(small[4:]), ptr(gan_utils._ticket(Cmix.device)),
                                                    ws, wsb, stream_of(Cmix)), "mixed_sinkhorn_loss_fwd")
        st["Cmix"], st["eps"] = Cmix, float(eps)
        return small[4:].reshape(()), st

    @staticmethod
    def mixed_loss_full(R, F, feats, sc, eps, L, keep):
        """Replicated regime: the unchanged single-GPU loss call on the gathered stacked R, F [2B,K] and the six gathered
        features -- Cmix [4,B,B], the loss and the iteration counts are those of compute_mixed_sinkhorn_loss bit for bit."""
        B, K = R.shape[0] // 2, R.shape[1]
        T, J = feats[0].shape[1], feats[0].shape[2]
        st = HipOps._mixed_state(B, L, keep, R.device)
        ws, wsb = workspace(lib.kccot_mixed_sinkhorn_loss_workspace_bytes(B, K), R)
        Cmix = _lib.empty((4, B, B), torch.float32, R.device)
        loss, st = HipOps._mixed_fwd(ptr(R), ptr(F), B, K, sc, [ptr(f) for f in feats], T, J, eps, L, gan_utils.cost_flags,
                                     Cmix, st, ws, wsb)
        return loss, Cmix, st

    @staticmethod
    def mixed_cost_rows(R, F, sc, row_begin, row_count, norms=None):
        """Rows [row_begin, row_begin + row_count) of the plain scaled distances of the stacked problem, [3, row_count, 2B]
        = (RF, RR, FF): on the matrix pipe when the gathered stacked `norms` [2B,3] are given, else on the direct kernel.
        Both entries demand four feature pointers: one zero [2B,1,1] tensor with T = J = 1 (no causal term; d + 0 is exact)."""
        zero = _zeros_feat(R.shape[0], R.device)
        return HipOps.cost3_rows(R, F, zero, zero, zero, zero, sc, row_begin, row_count, norms)

    @staticmethod
    def causal_add(C, h_rows, M, sc):
        """C [Bx,By] += sc causal(h_rows, M) in place (KCCOT_COST_CAUSAL_ADD: the single-GPU Cmix's summation order)."""
        Bx, By = C.shape
        T, J = h_rows.shape[1], h_rows.shape[2]
        check(lib.kccot_pairwise_cost_f32(None, None, Bx, By, 0, sc, ptr(h_rows.contiguous()), ptr(M), None, None, T, J,
                                          _lib.COST_CAUSAL_ADD, ptr(C), None, 0, stream_of(C)), "pairwise_cost(causal add)")
        return C

    @staticmethod
    def mixed_loss_given(Cmix, eps, L, keep):
        """Row-block regime: the four solves, the combination and (fused) the reverse sweep on the gathered Cmix
        (KCCOT_MIXED_CMIX_GIVEN); n > 128 runs the multi-CU solver inside the library."""
        B = Cmix.shape[1]
        st = HipOps._mixed_state(B, L, keep, Cmix.device)
        ws, wsb = (None, 0) if st["fused"] else workspace(lib.kccot_sinkhorn_workspace_bytes(4, B), Cmix)
        return HipOps._mixed_fwd(None, None, B, 0, 0.0, [None] * 6, 1, 1, eps, L, _lib.MIXED_CMIX_GIVEN, Cmix, st, ws, wsb)

    @staticmethod
    def mixed_dcmix(st, g):
        """d loss / d Cmix at the upstream scalar g: dCmix_unit * g (fused), or the reverse sweep of the four problems with
        gcost4 = g {1, 1, -1, -1} formed on the device (history)."""
        g = g.reshape(1).float()
        if st["fused"]:
            return st["dCu"] * g
        Cmix = st["Cmix"]
        B = Cmix.shape[1]
        gc = g * _mix_weights(g.device)
        dC = _lib.empty_like(Cmix)
        ws, wsb = workspace(lib.kccot_sinkhorn_workspace_bytes(4, B), Cmix)
        check(lib.kccot_sinkhorn_bwd_f32(ptr(Cmix), ptr(st["uh"]), ptr(st["vh"]), ptr(st["nits"]), 4, B, st["eps"], st["Lh"],
                                         ptr(gc), ptr(dC), ws, wsb, stream_of(Cmix)), "sinkhorn_bwd")
        return dC

    @staticmethod
    def mixed_dfake_rows(dCmix, R, F, sc, row_begin, row_count):
        """The video gradients of this rank's rows of y and y': g3 [3,2B,2B] of the stacked problem from dCmix (the block
        map of mixed_cost_bwd: dC1 -> RF (0,0), dC2 -> RF (1,1), dC4 -> FF (0,1)), then two row calls of the cost backward."""
        B = dCmix.shape[1]
        g3 = torch.zeros((3, 2 * B, 2 * B), dtype=torch.float32, device=dCmix.device)
        g3[0, :B, :B] = dCmix[0]
        g3[0, B:, B:] = dCmix[1]
        g3[2, :B, B:] = dCmix[3]
        return (HipOps.dfake_rows(g3, R, F, sc, row_begin, row_count),
                HipOps.dfake_rows(g3, R, F, sc, B + row_begin, row_count))

    @staticmethod
    def mixed_feature_grads(dCmix, g, st, R, F, feats, sc, row_begin, row_count, whole=False):
        """The six feature gradients of this rank's rows (h_fake, m_real, h_real_p, m_fake, h_fake_p, m_real_p), formed for
        all B samples and sliced.  whole=True (replicated regime): the single-GPU loss's backward with dF = NULL (after a
        fused forward with its dCmix_unit and g, else with dCmix at g = 1: the single-GPU call's operands and bits).
        Otherwise one kccot_pairwise_cost_bwd_f32 per block with dx = dy = NULL -- nothing that grows with K:
        dh_fake <- C1, dm_real <- C1 + C3, dh_real_p <- C3, dm_fake <- C4, dh_fake_p <- C2 + C4, dm_real_p <- C2."""
        B, K = R.shape[0] // 2, R.shape[1]
        T, J = feats[0].shape[1], feats[0].shape[2]
        dev, stm = R.device, stream_of(R)
        if whole:
            df = _lib.empty((6, B, T, J), torch.float32, dev)
            ws, wsb = workspace(lib.kccot_mixed_sinkhorn_loss_workspace_bytes(B, K), R)
            gl, dCu = (g.reshape(1).float().contiguous(), st["dCu"]) if st["fused"] else (_one(dev), dCmix)
            check(lib.kccot_mixed_sinkhorn_loss_bwd_f32(ptr(gl), ptr(R), ptr(F), B, K, sc, *(ptr(f) for f in feats), T, J,
                                                        st["eps"], st["Lh"], None, None, None, None, ptr(dCu), None,
                                                        *(ptr(d) for d in df), ws, wsb, stm),
                  "mixed_sinkhorn_loss_bwd(feature gradients)")
            out = [df[i] for i in range(6)]
        else:
            h_fake, m_real, h_real_p, m_fake, h_fake_p, m_real_p = feats
            part = _lib.empty((4, 2, B, T, J), torch.float32, dev)            # [block][dh, dM]
            for k, (h, M) in enumerate(((h_fake, m_real), (h_fake_p, m_real_p), (h_real_p, m_real), (h_fake_p, m_fake))):
                check(lib.kccot_pairwise_cost_bwd_f32(ptr(dCmix[k]), ptr(R), ptr(F), B, B, K, sc, ptr(h), ptr(M), T, J, 0,
                                                      None, None, ptr(part[k, 0]), ptr(part[k, 1]), None, 0, stm),
                      "pairwise_cost_bwd(mixed block)")
            out = [part[0, 0], part[0, 1] + part[2, 1], part[2, 0], part[3, 1], part[1, 0] + part[3, 0], part[1, 1]]
        return tuple(d[row_begin:row_begin + row_count] for d in out)

    # ---- the RBF-kernel MMD (mmd.rbf_mmd2) ----
    @staticmethod
    def mmd_cost_rows(real, fake, row_begin, row_count, norms=None):
        """Rows [row_begin, row_begin + row_count) of the plain squared distances, [3, row_count, B] = (xy, xx, yy), sc = 1:
        on the matrix pipe when the gathered `norms` [B,3] are given, else on the direct kernel (one zero [B,1,1] feature
        tensor with T = J = 1: no causal term)."""
        zero = _zeros_feat(real.shape[0], real.device)
        return HipOps.cost3_rows(real, fake, zero, zero, zero, zero, 1.0, row_begin, row_count, norms)

    @staticmethod
    def rbf_sum_rows(blk, gamma):
        """The three distance row blocks [3,Bl,B] -> exp(-gamma blk) IN PLACE and their three fp64 sums (KCCOT_COST_RBF_SUM,
        one call per block).  Each call has a workspace of its own: its first double is the block's sum."""
        _, Bl, B = blk.shape
        nd = (int(lib.kccot_pairwise_cost_workspace_bytes(Bl, B, 1)) + 7) // 8
        ws = _lib.empty((3, nd), torch.float64, blk.device)
        for p in range(3):
            check(lib.kccot_pairwise_cost_f32(None, None, Bl, B, 0, float(gamma), None, None, None, None, 1, 1,
                                              _lib.COST_RBF_SUM, ptr(blk[p]), ws[p].data_ptr(), nd * 8, stream_of(blk)),
                  "pairwise_cost(rbf sum)")
        return blk, ws[:, 0].contiguous()

    @staticmethod
    def rbf_mmd_grad(K3, gamma, g):
        """gD3 [3,B,B] = g d mmd^2 / d D3 from the gathered kernel matrices (kccot_rbf_mmd_bwd_f32)."""
        gD3 = _lib.empty_like(K3)
        g = g.reshape(1).float().contiguous()
        check(lib.kccot_rbf_mmd_bwd_f32(ptr(K3), K3.shape[1], float(gamma), ptr(g), ptr(gD3), stream_of(K3)), "rbf_mmd_bwd")
        return gD3


# the operations the sharded mixed loss needs of an ops object (an injected one must provide all of them)
MIXED_OPS = ("replicate_costs", "mixed_loss_full", "mixed_cost_rows", "causal_add", "mixed_loss_given", "mixed_dcmix",
             "mixed_dfake_rows", "mixed_feature_grads")
# ... and the sharded RBF-kernel MMD
MMD_OPS = ("mmd_cost_rows", "rbf_sum_rows", "rbf_mmd_grad", "dfake_rows")

_ones = {}
_zero_feats = {}
_mix_w = {}


def _zeros_feat(n, device):
    """A zero [n,1,1] feature tensor per (n, device): the four feature pointers of a row-block call without causal terms."""
    t = _zero_feats.get((n, device))
    if t is None:
        t = torch.zeros((n, 1, 1), dtype=torch.float32, device=device)
        _zero_feats[(n, device)] = t
    return t


def _mix_weights(device):
    """{1, 1, -1, -1} on the device: d loss / d cost4 of (W1 + W2) - W3 - W4 at g = 1."""
    t = _mix_w.get(device)
    if t is None:
        t = torch.tensor([1.0, 1.0, -1.0, -1.0], dtype=torch.float32, device=device)
        _mix_w[device] = t
    return t


def _one(device):
    """One device float 1.0 per device (the upstream scalar of a library backward)."""
    t = _ones.get(device)
    if t is None:
        t = torch.ones((1,), dtype=torch.float32, device=device)
        _ones[device] = t
    return t


def _record(ops, bicausal, saved, C3):
    """Iteration counts of the latest sharded evaluation, where raise_if_solver_aborted() looks for them."""
    if ops is not HipOps:
        return
    nits, executed = saved[3][:3], saved[3][3:]
    last_info["nits"], last_info["nits_executed"] = nits, executed
    if bicausal:
        tag = "compute_bicausal_sinkhorn_loss"
        gan_utils.last_info[tag], gan_utils.last_info[tag + "_executed"] = nits, executed
        last_info["C3"] = C3               # the replicated bi-causal cost matrices
    else:
        gan_utils.last_info["compute_sinkhorn_loss"] = nits    # raise_if_solver_aborted() covers the sharded loss too


# ---- contraction-sharded protocol ("ksplit") ------------------------------------------------------------------
# Instead of gathering the whole batch on every rank, the [B/G, K] shards are all-to-all'ed into [B, K/G] slices:
# every rank holds ALL samples but 1/G of the features.  The Gram kernels split K anyway, so rank g forms the fp64
# Gram sums of its slice (KCCOT_COST_GRAM_SUMS_ONLY), the 80 KB (B <= 64) of sums are all-reduced(SUM), and the
# finalize step (KCCOT_COST_FROM_GRAM_SUMS) gives every rank the full cost matrices -- the same arithmetic as one GPU,
# with the K-chunks summed in a different grouping.  Backward: the video gradient of ALL samples on the rank's slice,
# all-to-all back.  7/8 of a shard leaves a rank per tensor instead of 7 shards arriving, and the two HBM-heavy
# kernels shrink with G.  Opt-in (protocol="ksplit" / KCCOT_DIST_PROTOCOL=ksplit) until it has been timed on a
# multi-GPU node; needs K % G == 0, K/G % 4 == 0, K/G >= 256 and a Gram path for B (B <= 64 or B % 128 == 0).
def ksplit_supported(B, K, world):
    if world < 1 or K % world:
        return False
    Ks = K // world
    if Ks % 4 or Ks < 256:
        return False
    import ctypes
    off, cnt = ctypes.c_size_t(0), ctypes.c_size_t(0)
    check(lib.kccot_pairwise_cost3_gram_sums_span(B, Ks, ctypes.byref(off), ctypes.byref(cnt)), "gram_sums_span")
    return cnt.value > 0


def all_to_all_slices(t, group=None):
    """[B/G, K] shard -> [B, K/G] slice: rows in global sample order, columns = this rank's K-range."""
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    Bl, K = t.shape
    Ks = K // world
    if dist.get_backend(group) != "nccl":        # gloo has no all_to_all: rehearsal through an all-gather
        return t.contiguous() if world == 1 else all_gather_cat(t, group)[:, rank * Ks:(rank + 1) * Ks].contiguous()
    send = t.reshape(Bl, world, Ks).transpose(0, 1).contiguous()          # [G, Bl, Ks]: chunk g goes to rank g
    recv = torch.empty_like(send)
    dist.all_to_all_single(recv, send, group=group)
    return recv.reshape(world * Bl, Ks)


def all_to_all_rows(t, group=None):
    """Inverse of all_to_all_slices: [B, K/G] slice (all samples) -> [B/G, K] rows of this rank's samples."""
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    B, Ks = t.shape
    Bl = B // world
    if dist.get_backend(group) != "nccl":
        if world == 1:
            return t.contiguous()
        full = all_gather_cat(t.contiguous(), group).reshape(world, B, Ks)   # [source rank = K-range][sample][Ks]
        return full[:, rank * Bl:(rank + 1) * Bl].transpose(0, 1).reshape(Bl, world * Ks).contiguous()
    send = t.reshape(world, Bl, Ks).contiguous()                          # chunk g = the rows of rank g's samples
    recv = torch.empty_like(send)
    dist.all_to_all_single(recv, send, group=group)                       # recv[g] = K-range g of my samples
    return recv.transpose(0, 1).reshape(Bl, world * Ks).contiguous()


def _all_reduce_sum(t, group):
    if dist.get_world_size(group) == 1:
        return
    if dist.get_backend(group) == "gloo" and t.is_cuda:
        h = t.cpu()
        dist.all_reduce(h, op=dist.ReduceOp.SUM, group=group)
        t.copy_(h)
    else:
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)


class _KSplitLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, real_l, fake_l, h_fake_l, h_real_l, m_real_l, m_fake_l, sc, eps, L, group, bicausal):
        import ctypes
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        Bl = real_l.shape[0]
        B = Bl * world
        _mark("start")
        real_s = all_to_all_slices(real_l, group)
        fake_s = all_to_all_slices(fake_l, group)
        Ks = real_s.shape[1]
        feats = all_gather_cat(torch.stack([h_fake_l, h_real_l, m_real_l, m_fake_l], dim=1), group)
        h_fake, h_real, m_real, m_fake = (feats[:, i].contiguous() for i in range(4))
        _mark("exchange_inputs")
        T, J = h_fake.shape[1], h_fake.shape[2]
        dev = real_s.device
        # a workspace of its own: the Gram sums must survive between the two calls (the shared scratch is reused)
        wsb = int(lib.kccot_pairwise_cost3_workspace_bytes(B, Ks))
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        off, cnt = ctypes.c_size_t(0), ctypes.c_size_t(0)
        check(lib.kccot_pairwise_cost3_gram_sums_span(B, Ks, ctypes.byref(off), ctypes.byref(cnt)), "gram_sums_span")
        if cnt.value == 0:
            raise NotImplementedError("ksplit protocol: no Gram path for B=%d, K/G=%d" % (B, Ks))
        C3 = _lib.empty((3, B, B), torch.float32, dev)
        args = (ptr(real_s), ptr(fake_s), B, Ks, sc, ptr(h_fake), ptr(h_real), ptr(m_real), ptr(m_fake), T, J)
        check(lib.kccot_pairwise_cost3_f32(*args, _lib.COST_GRAM_SUMS_ONLY, ptr(C3), ws.data_ptr(), wsb, stream_of(real_s)),
              "pairwise_cost3(gram sums)")
        gsum = ws[off.value:off.value + 8 * cnt.value].view(torch.float64)
        _mark("cost_gram_sums")
        _all_reduce_sum(gsum, group)
        _mark("exchange_costs")
        check(lib.kccot_pairwise_cost3_f32(*args, _lib.COST_FROM_GRAM_SUMS, ptr(C3), ws.data_ptr(), wsb, stream_of(real_s)),
              "pairwise_cost3(from gram sums)")
        _mark("cost_finalize")
        if bicausal:
            HipOps.bicausal_term(C3, h_fake, h_real, m_real, m_fake, sc)
            _mark("bicausal_term")
        loss, saved = HipOps.divergence_fwd(C3, eps, L)
        _mark("sinkhorn_fwd")
        _record(HipOps, bicausal, saved, C3)
        ctx.saved_state = (saved, real_s, fake_s, h_fake, h_real, m_real, m_fake)
        ctx.cfg = (sc, rank * Bl, Bl, group, bicausal)
        return loss

    @staticmethod
    def backward(ctx, g):
        saved, real_s, fake_s, h_fake, h_real, m_real, m_fake = ctx.saved_state
        sc, row_begin, Bl, group, bicausal = ctx.cfg
        if ctx.needs_input_grad[0]:
            raise NotImplementedError("the loss path never differentiates w.r.t. real (kernel_train.py:252,289)")
        _mark("between_fwd_and_bwd")
        dC3 = HipOps.divergence_bwd(saved, g.reshape(()))
        _mark("sinkhorn_bwd")
        B, Ks = real_s.shape
        T, J = h_fake.shape[1], h_fake.shape[2]
        # video gradient of ALL samples on this rank's K-slice, then back to the sample-sharded layout
        dfake_s = _lib.empty((B, Ks), torch.float32, real_s.device)
        ws, wsb = workspace(lib.kccot_pairwise_cost3_bwd_workspace_bytes(B, Ks), real_s)
        check(lib.kccot_pairwise_cost3_bwd_f32(ptr(dC3), ptr(real_s), ptr(fake_s), B, Ks, sc, None, None, None, None, 1, 1,
                                               ptr(dfake_s), None, None, None, None, ws, wsb, stream_of(real_s)),
              "pairwise_cost3_bwd")
        _mark("gradient")
        dfake = all_to_all_rows(dfake_s, group)
        _mark("exchange_gradient")
        # feature gradients of this rank's samples (KB-sized products of dC3 with the gathered features)
        if bicausal:
            dhf, dhr, dmr, dmf = HipOps.bicausal_feature_grads(dC3, real_s, fake_s, h_fake, h_real, m_real, m_fake, sc,
                                                               row_begin, Bl)
        else:
            dhf, dhr, dmr, dmf = (_lib.empty((Bl, T, J), torch.float32, real_s.device) for _ in range(4))
            check(lib.kccot_pairwise_cost3_bwd_rows_f32(ptr(dC3), ptr(real_s), ptr(fake_s), B, Ks, sc, ptr(h_fake), ptr(h_real),
                                                        ptr(m_real), ptr(m_fake), T, J, row_begin, Bl, None, ptr(dhf), ptr(dhr),
                                                        ptr(dmr), ptr(dmf), None, 0, stream_of(real_s)), "pairwise_cost3_bwd_rows")
        _mark("gradient")
        return None, dfake, dhf, dhr, dmr, dmf, None, None, None, None, None


def all_gather_cat(t, group=None):
    """Concatenate the ranks' equally shaped tensors along dim 0.  RCCL handles device tensors
    directly; the gloo backend (CPU rehearsal) is staged through host memory."""
    world = dist.get_world_size(group)
    if world == 1:
        return t
    t = t.contiguous()
    if dist.get_backend(group) == "gloo" and t.is_cuda:
        parts = [torch.empty(t.shape, dtype=t.dtype) for _ in range(world)]
        dist.all_gather(parts, t.cpu(), group=group)
        return torch.cat(parts, 0).to(t.device)
    out = torch.empty((world * t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    dist.all_gather_into_tensor(out, t, group=group)
    return out


def gather_chunk_bounds(K, nchunks):
    """Column ranges of the chunked video all-gather (KCCOT_DIST_GATHER_CHUNKS): `nchunks` ranges of whole 32-column load
    granules (the last one takes the remainder), every range at least 256 columns wide.  A function of (K, nchunks) only, so
    all ranks cut alike."""
    gran = (K + 31) // 32
    n = max(1, min(int(nchunks), gran // 8))
    per = (gran + n - 1) // n
    bounds, a = [], 0
    while a < K:
        b = min(K, a + per * 32)
        if K - b < 256:
            b = K
        bounds.append((a, b))
        a = b
    return bounds


def _gather_columns_async(t_l, bounds, group, force_collective=False):
    """all-gather the column ranges of a [Bl, K] shard as separate collectives: [(work or None, [B, Kc] tensor)] in range
    order.  RCCL: async_op -- the collectives queue up on the communicator's stream and `work.wait()` makes the compute
    stream wait for ONE of them, so what is computed on range c overlaps the transfers of ranges c + 1, ...; gloo (CPU
    rehearsal with device tensors): staged through the host, no overlap.
    Coverage: the RCCL branch (async_op + work.wait()) has run at world size 1 only (tools/nccl_selftest.py forces the
    collective there); with two or more ranks it has not executed anywhere yet -- a one-GPU box cannot hold two RCCL ranks,
    and the two-rank gloo test takes the synchronous branch.  bench.py times it as `gather_chunks` on the first multi-GPU run."""
    world = dist.get_world_size(group)
    out = []
    for a, b in bounds:
        piece = t_l[:, a:b].contiguous()
        if world == 1 and not force_collective:
            out.append((None, piece))
        elif dist.get_backend(group) == "gloo":
            out.append((None, all_gather_cat(piece, group)))
        else:
            full = torch.empty((world * piece.shape[0], b - a), dtype=piece.dtype, device=piece.device)
            out.append((dist.all_gather_into_tensor(full, piece, group=group, async_op=True), full))
    return out


class _AllGatherLocalGrad(torch.autograd.Function):
    """all-gather whose backward hands back the LOCAL slice of the incoming gradient.  For a
    quantity every rank computes identically from the gathered tensor (replicated loss) that slice
    is the partial derivative through this rank's samples; the parameter-gradient all-reduce SUM
    completes it."""

    @staticmethod
    def forward(ctx, t, group):
        ctx.cfg = (dist.get_rank(group), t.shape[0])
        return all_gather_cat(t, group)

    @staticmethod
    def backward(ctx, g):
        rank, Bl = ctx.cfg
        return g[rank * Bl:(rank + 1) * Bl].contiguous(), None


def all_gather_local_grad(t, group=None):
    return _AllGatherLocalGrad.apply(t, group)


class _ShardedLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, real_l, fake_l, h_fake_l, h_real_l, m_real_l, m_fake_l, sc, eps, L, group, ops, bicausal):
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        Bl = real_l.shape[0]
        _mark("start")
        # B > 64 on the HIP ops: the row block runs on the matrix pipe and needs x.x, e.e, x.e of every sample -- each rank
        # computes its own rows' from its local shard and the 24 bytes per sample are gathered ahead of the videos
        norms = None
        if (hasattr(ops, "row_norms") and not ops.replicate_costs(Bl * world, real_l.shape[1])
                and ops.rows_gram_supported(Bl, Bl * world, real_l.shape[1]) and os.environ.get("KCCOT_DIST_ROWS") != "direct"):
            norms = all_gather_cat(ops.row_norms(real_l, fake_l), group)
        # KCCOT_DIST_GATHER_CHUNKS = N > 1 (matrix-pipe row blocks only): the videos travel as N column ranges and the Gram
        # sums of a range are formed while the later ranges are still in flight (opt-in: it has not
        # been timed on more than one GPU).  The ranges are kept as they arrive -- the backward works range by range too.
        nchunks = int(os.environ.get("KCCOT_DIST_GATHER_CHUNKS", "0") or 0)
        chunked = norms is not None and nchunks > 1 and hasattr(ops, "rows_gram_sums")
        bounds = gather_chunk_bounds(real_l.shape[1], nchunks) if chunked else None
        chunked = chunked and len(bounds) > 1
        whole = False                # the whole C3 assembled on every rank (no row blocks)
        if chunked:
            pieces_r = _gather_columns_async(real_l, bounds, group)
            pieces_f = _gather_columns_async(fake_l, bounds, group)
            real = fake = None
        else:
            real = all_gather_cat(real_l, group)
            fake = all_gather_cat(fake_l, group)
        # the four [Bl,T,J] feature shards travel as one message
        feats = all_gather_cat(torch.stack([h_fake_l, h_real_l, m_real_l, m_fake_l], dim=1), group)
        h_fake, h_real, m_real, m_fake = (feats[:, i].contiguous() for i in range(4))
        _mark("exchange_inputs")       # (chunked gather: only the small messages -- the video ranges are waited for below)
        if chunked:
            B = Bl * world
            gsum = _lib.empty((int(lib.kccot_pairwise_cost3_rows_gram_sums_count(Bl, B)),), torch.float64, real_l.device)
            real, fake = [], []
            for c, ((wr, r_c), (wf, f_c)) in enumerate(zip(pieces_r, pieces_f)):      # fixed range order: reproducible sums
                for w in (wr, wf):
                    if w is not None:
                        w.wait()
                ops.rows_gram_sums(r_c, f_c, rank * Bl, Bl, gsum, c > 0)
                real.append(r_c)
                fake.append(f_c)
            blk = ops.rows_gram_from_sums(gsum, B, h_fake, h_real, m_real, m_fake, sc, rank * Bl, Bl, norms)
            _mark("cost_rows_overlapping_the_gather")
            C3 = all_gather_cat(blk.transpose(0, 1).contiguous(), group).transpose(0, 1).contiguous()  # [3,B,B]
            _mark("exchange_costs")
        elif hasattr(ops, "cost3_full") and ops.replicate_costs(real.shape[0], real.shape[1]):
            C3 = ops.cost3_full(real, fake, h_fake, h_real, m_real, m_fake, sc)     # small batch: replicated assembly
            whole = True
            _mark("cost_replicated")
        else:
            # row blocks of the three cost matrices (gan_utils.py:221-223)
            if norms is not None:                # the Gram row block on the matrix pipe
                blk = ops.cost3_rows(real, fake, h_fake, h_real, m_real, m_fake, sc, rank * Bl, Bl, norms)
            elif hasattr(ops, "cost3_rows"):     # one launch for the three row blocks
                blk = ops.cost3_rows(real, fake, h_fake, h_real, m_real, m_fake, sc, rank * Bl, Bl)
            else:
                blk = torch.stack([ops.cost_rows(real_l, fake, h_fake_l, m_real, sc),
                                   ops.cost_rows(real_l, real, h_real_l, m_real, sc),
                                   ops.cost_rows(fake_l, fake, h_fake_l, m_fake, sc)], dim=0)        # [3,Bl,B]
            _mark("cost_rows")
            C3 = all_gather_cat(blk.transpose(0, 1).contiguous(), group).transpose(0, 1).contiguous()  # [3,B,B]
            _mark("exchange_costs")
        if bicausal:                             # every rank adds the second causal terms to its replicated C3
            C3 = ops.bicausal_term(C3, h_fake, h_real, m_real, m_fake, sc)
            _mark("bicausal_term")
        if hasattr(ops, "divergence_fwd"):       # solves + combination in one launch
            loss, saved = ops.divergence_fwd(C3, eps, L)
        else:
            cost3, saved = ops.sinkhorn3_fwd(C3, eps, L)
            loss = (2.0 * cost3[0] - cost3[1]) - cost3[2]       # gan_utils.py:225
        _mark("sinkhorn_fwd")
        _record(ops, bicausal, saved, C3)
        ctx.saved_state = (saved, real, fake, h_fake, h_real, m_real, m_fake)
        ctx.cfg = (sc, rank * Bl, Bl, ops, bicausal, whole)
        return loss

    @staticmethod
    def backward(ctx, g):
        saved, real, fake, h_fake, h_real, m_real, m_fake = ctx.saved_state
        sc, row_begin, Bl, ops, bicausal, whole = ctx.cfg
        if ctx.needs_input_grad[0]:
            raise NotImplementedError("the loss path never differentiates w.r.t. real (kernel_train.py:252,289)")
        g = g.reshape(())
        _mark("between_fwd_and_bwd")
        if hasattr(ops, "divergence_bwd"):
            dC3 = ops.divergence_bwd(saved, g)
        else:
            gcost3 = torch.stack([2.0 * g, -g, -g])             # d(2 xy - xx - yy)
            dC3 = ops.sinkhorn3_bwd(saved, gcost3)
        _mark("sinkhorn_bwd")
        if bicausal:
            # the video gradient is the one-batch loss's (range by range after a chunked gather); the feature gradients
            # follow the bi-causal job table
            reals, fakes = (real, fake) if isinstance(real, list) else ([real], [fake])
            parts = [_dfake_rows(ops, dC3, r_c, f_c, h_fake, h_real, m_real, m_fake, sc, row_begin, Bl)
                     for r_c, f_c in zip(reals, fakes)]
            dfake = parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)
            dhf, dhr, dmr, dmf = ops.bicausal_feature_grads(dC3, reals[0], fakes[0], h_fake, h_real, m_real, m_fake, sc,
                                                            row_begin, Bl, whole)
        elif isinstance(real, list):     # chunked gather: the video gradient is separable in the columns, range by range
            parts = [ops.cost3_bwd_rows(dC3, r_c, f_c, h_fake, h_real, m_real, m_fake, sc, row_begin, Bl)
                     for r_c, f_c in zip(real, fake)]
            dfake = torch.cat([p[0] for p in parts], dim=1)
            dhf, dhr, dmr, dmf = parts[0][1:]                    # the feature gradients do not depend on the videos
        else:
            dfake, dhf, dhr, dmr, dmf = ops.cost3_bwd_rows(dC3, real, fake, h_fake, h_real, m_real, m_fake, sc, row_begin, Bl)
        _mark("gradient")
        return None, dfake, dhf, dhr, dmr, dmf, None, None, None, None, None, None


def _dfake_rows(ops, dC3, real, fake, h_fake, h_real, m_real, m_fake, sc, row_begin, row_count):
    if hasattr(ops, "dfake_rows"):
        return ops.dfake_rows(dC3, real, fake, sc, row_begin, row_count)
    return ops.cost3_bwd_rows(dC3, real, fake, h_fake, h_real, m_real, m_fake, sc, row_begin, row_count)[0]


def sharded_sinkhorn_loss(f_real_l, f_fake_l, scaling_coef, h_fake_l, m_real_l, h_real_l, m_fake_l, group=None,
                          ops=None, epsilon=1.0, L=100, protocol=None):
    """compute_sinkhorn_loss (gan_utils.py:204-227) of the GLOBAL batch from per-rank shards.
    Arguments are this rank's [B/G, ...] slices, in the reference's order h_fake, m_real, h_real,
    m_fake.  epsilon / L default to what the reference effectively runs (1.0, 100)."""
    return _sharded_loss(f_real_l, f_fake_l, scaling_coef, h_fake_l, m_real_l, h_real_l, m_fake_l, group, ops, epsilon, L,
                         protocol, False)


def sharded_bicausal_sinkhorn_loss(f_real_l, f_fake_l, scaling_coef, h_fake_l, m_real_l, h_real_l, m_fake_l, group=None,
                                   ops=None, epsilon=1.0, L=100, protocol=None):
    """gan_utils.compute_bicausal_sinkhorn_loss, 2 W(x,y) - W(x,x) - W(y,y) with the bi-causal cost, of the GLOBAL batch
    from per-rank shards: the same arguments, order and protocols as sharded_sinkhorn_loss, and the same result on every
    rank.  Each protocol assembles the one-batch C3 exactly as sharded_sinkhorn_loss does (replicated at B <= 64; row
    blocks all-gathered; ksplit: all-reduced Gram sums), then every rank adds the second causal term of each matrix to its
    replicated C3 (KCCOT_COST_BICAUSAL_TERM_ONLY, the single-GPU loss's launch).  Backward: the video gradient rows are the
    one-batch loss's; the feature gradients follow the bi-causal job table.  Records
    gan_utils.last_info["compute_bicausal_sinkhorn_loss"] (and dist.last_info["C3"]).  Injected ``ops`` must provide
    ``bicausal_term`` and ``bicausal_feature_grads``."""
    ops = ops or HipOps
    missing = [n for n in ("bicausal_term", "bicausal_feature_grads") if not hasattr(ops, n)]
    if missing:
        raise NotImplementedError("sharded bi-causal loss: the ops %r lack %s" % (getattr(ops, "__name__", ops), ", ".join(missing)))
    return _sharded_loss(f_real_l, f_fake_l, scaling_coef, h_fake_l, m_real_l, h_real_l, m_fake_l, group, ops, epsilon, L,
                         protocol, True)


def _sharded_loss(f_real_l, f_fake_l, scaling_coef, h_fake_l, m_real_l, h_real_l, m_fake_l, group, ops, epsilon, L, protocol,
                  bicausal):
    ops = ops or HipOps
    Bl = f_real_l.shape[0]
    cast = (lambda v: v.float()) if ops is HipOps else (lambda v: v)   # the HIP kernels are fp32
    flat = lambda v: cast(v.reshape(Bl, -1)).contiguous()
    feat = lambda v: cast(v).contiguous()
    # protocol: "gather" (the default, and what BASELINE.json's north star prescribes: all-gather the batch; replicated
    # assembly at B <= 64, row blocks above), "ksplit" (opt-in: shard the contraction -- all-to-all into K-slices,
    # all-reduced fp64 Gram sums; by byte counts and per-rank kernel times it should win above B = 64, DESIGN.md
    # section 6, but it has never been timed on more than one GPU, so it stays opt-in until a SCALE record exists),
    # or "auto" (ksplit above B = 64 when the shape allows it, gather otherwise).
    protocol = protocol or os.environ.get("KCCOT_DIST_PROTOCOL", "gather")
    if protocol not in ("auto", "gather", "ksplit"):
        raise ValueError("unknown protocol %r" % (protocol,))
    if protocol == "auto":
        world = dist.get_world_size(group)
        K = f_real_l.reshape(Bl, -1).shape[1]
        protocol = "ksplit" if (ops is HipOps and Bl * world > 64 and ksplit_supported(Bl * world, K, world)) else "gather"
    if protocol == "ksplit":
        if ops is not HipOps:
            raise ValueError("the ksplit protocol runs on the HIP ops only")
        world = dist.get_world_size(group)
        K = f_real_l.reshape(Bl, -1).shape[1]
        if not ksplit_supported(Bl * world, K, world):
            raise NotImplementedError("ksplit protocol: unsupported shape B=%d K=%d on %d ranks" % (Bl * world, K, world))
        return _KSplitLoss.apply(flat(f_real_l), flat(f_fake_l), feat(h_fake_l), feat(h_real_l), feat(m_real_l),
                                 feat(m_fake_l), float(scaling_coef), float(epsilon), int(L), group, bicausal).reshape(())
    return _ShardedLoss.apply(flat(f_real_l), flat(f_fake_l), feat(h_fake_l), feat(h_real_l), feat(m_real_l),
                              feat(m_fake_l), float(scaling_coef), float(epsilon), int(L), group, ops, bicausal).reshape(())


# ---- the mixed divergence over two minibatches ----------------------------------------
def _gather_into(out, t, group):
    """all-gather the equally shaped [Bl, ...] shards straight into `out` [G Bl, ...] (a contiguous view, e.g. one half of
    a stacked buffer): RCCL writes it in place (also at world size 1); gloo is staged through the host."""
    world = dist.get_world_size(group)
    t = t.contiguous()
    if dist.get_backend(group) == "nccl":
        dist.all_gather_into_tensor(out, t, group=group)
    elif world == 1:
        out.copy_(t)
    else:
        out.copy_(all_gather_cat(t, group))


class _ShardedMixedLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x_l, y_l, xp_l, yp_l, h_fake_l, m_real_l, h_real_p_l, m_fake_l, h_fake_p_l, m_real_p_l, sc, eps, L,
                group, ops):
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        Bl, K = x_l.shape
        B = Bl * world
        dev, dt = x_l.device, x_l.dtype
        keep = any(ctx.needs_input_grad[1:10])
        whole = ops.replicate_costs(B, K)           # the whole Cmix on every rank (B <= 64): the single-GPU loss call
        _mark("start")
        # row blocks on the matrix pipe need x.x, e.e, x.e of every sample of the stacked problem: each rank's own rows of
        # (x, y) and (x', y'), gathered into the two halves of [2B,3] (stacked order)
        norms = None
        if (not whole and hasattr(ops, "row_norms") and ops.rows_gram_supported(Bl, 2 * B, K)
                and os.environ.get("KCCOT_DIST_ROWS") != "direct"):
            norms = torch.empty((2 * B, 3), dtype=torch.float64, device=dev)
            _gather_into(norms[:B], ops.row_norms(x_l, y_l), group)
            _gather_into(norms[B:], ops.row_norms(xp_l, yp_l), group)
        # the four videos straight into the halves of the stacked R = [x; x'], F = [y; y'] (no torch.cat)
        R = torch.empty((2 * B, K), dtype=dt, device=dev)
        F = torch.empty((2 * B, K), dtype=dt, device=dev)
        for out, t in ((R[:B], x_l), (R[B:], xp_l), (F[:B], y_l), (F[B:], yp_l)):
            _gather_into(out, t, group)
        # the six [Bl,T,J] feature shards travel as one message
        fl = (h_fake_l, m_real_l, h_real_p_l, m_fake_l, h_fake_p_l, m_real_p_l)
        allf = all_gather_cat(torch.stack(fl, dim=1), group)
        feats = tuple(allf[:, i].contiguous() for i in range(6))
        _mark("exchange_inputs")
        if whole:
            # one call: the cost stage, the four solves and (fused) the reverse sweep -- the phase holds the solves too
            loss, Cmix, state = ops.mixed_loss_full(R, F, feats, sc, eps, L, keep)
            _mark("cost_replicated")
        else:
            h_fake, m_real, h_real_p, m_fake, h_fake_p, m_real_p = feats
            top = ops.mixed_cost_rows(R, F, sc, rank * Bl, Bl, norms)          # rows I of (RF, RR, FF)
            bot = ops.mixed_cost_rows(R, F, sc, B + rank * Bl, Bl, norms)      # rows B + I
            # this rank's rows of C1 = RF[0:B,0:B], C2 = RF[B:,B:], C3 = RR[0:B,B:], C4 = FF[0:B,B:]
            blk = torch.stack([top[0, :, :B], bot[0, :, B:], top[1, :, B:], top[2, :, B:]])     # [4,Bl,B]
            _mark("cost_rows")
            lo = slice(rank * Bl, (rank + 1) * Bl)
            for k, (h, M) in enumerate(((h_fake, m_real), (h_fake_p, m_real_p), (h_real_p, m_real), (h_fake_p, m_fake))):
                c = ops.causal_add(blk[k], h[lo], M, sc)
                if c.data_ptr() != blk[k].data_ptr():
                    blk[k] = c
            _mark("causal_add")
            Cmix = all_gather_cat(blk.transpose(0, 1).contiguous(), group).transpose(0, 1).contiguous()   # [4,B,B]
            _mark("exchange_costs")
            loss, state = ops.mixed_loss_given(Cmix, eps, L, keep)
            _mark("sinkhorn_fwd")
        if ops is HipOps:
            nits, executed = state["nits"][:4], state["nits"][4:]
            last_info["nits"], last_info["nits_executed"] = nits, executed
            last_info["Cmix"] = Cmix                 # the replicated cost matrices
            tag = "compute_mixed_sinkhorn_loss"      # raise_if_solver_aborted((tag,)) covers the sharded loss too
            gan_utils.last_info[tag], gan_utils.last_info[tag + "_executed"] = nits, executed
        ctx.saved_state = (state, R, F, feats)
        ctx.cfg = (sc, rank * Bl, Bl, ops, whole)
        return loss

    @staticmethod
    def backward(ctx, g):
        state, R, F, feats = ctx.saved_state
        sc, row_begin, Bl, ops, whole = ctx.cfg
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[2]:
            raise NotImplementedError("the loss path never differentiates w.r.t. real (kernel_train.py:252,289)")
        g = g.reshape(())
        _mark("between_fwd_and_bwd")
        dCmix = ops.mixed_dcmix(state, g)
        _mark("sinkhorn_bwd")
        dy, dyp = ops.mixed_dfake_rows(dCmix, R, F, sc, row_begin, Bl)
        df = ops.mixed_feature_grads(dCmix, g, state, R, F, feats, sc, row_begin, Bl, whole)
        _mark("gradient")
        return (None, dy, None, dyp) + tuple(df) + (None,) * 5


def sharded_mixed_sinkhorn_loss(f_real_l, f_fake_l, f_real_p_l, f_fake_p_l, scaling_coef, h_fake_l, m_real_l, h_real_p_l,
                                m_fake_l, h_fake_p_l, m_real_p_l, group=None, ops=None, epsilon=1.0, L=100, protocol=None):
    """gan_utils.compute_mixed_sinkhorn_loss, (W(x,y) + W(x',y')) - W(x,x') - W(y,y'), of the GLOBAL batch from per-rank
    shards: the arguments are this rank's [B/G, ...] slices of x, y, x', y' and of the six features, in the order of the
    single-GPU function; epsilon / L as sharded_sinkhorn_loss.  Returns the same loss on every rank.  Differentiable
    w.r.t. both fake shards and all six feature shards; a real shard that requires a gradient raises NotImplementedError.

    The four videos are all-gathered into the stacked R = [x; x'], F = [y; y'] of the single-GPU loss.  B <= 64
    (``ops.replicate_costs``; KCCOT_DIST_ROW_BLOCKS=1 forces the row blocks): every rank runs the single-GPU loss call on
    them -- Cmix, loss and iteration counts bit-identical to compute_mixed_sinkhorn_loss.  Above: rank g forms its rows of
    the four cost matrices from two row-block calls on the stacked problem (rows g B/G and B + g B/G; the matrix pipe when
    the shape allows it), adds their causal terms in the single-GPU summation order (KCCOT_COST_CAUSAL_ADD), all-gathers
    them into Cmix [4,B,B], and solves on it (KCCOT_MIXED_CMIX_GIVEN).  Backward: each rank forms the gradient rows of
    its samples from the replicated d loss / d Cmix, no communication.

    Records gan_utils.last_info["compute_mixed_sinkhorn_loss"] and ``..._executed`` (so raise_if_solver_aborted covers
    it) and dist.last_info["Cmix"].  protocol: "gather" (default) or "auto" (= "gather"); "ksplit" is not implemented for
    this loss.  KCCOT_DIST_GATHER_CHUNKS does not apply to it.  Injected ``ops`` must provide MIXED_OPS."""
    ops = ops or HipOps
    missing = [n for n in MIXED_OPS if not hasattr(ops, n)]
    if missing:
        raise NotImplementedError("sharded mixed loss: the ops %r lack %s" % (getattr(ops, "__name__", ops), ", ".join(missing)))
    protocol = protocol or os.environ.get("KCCOT_DIST_PROTOCOL", "gather")
    if protocol == "ksplit":
        raise NotImplementedError("sharded mixed loss: the ksplit protocol is not implemented for the mixed divergence")
    if protocol not in ("auto", "gather"):
        raise ValueError("unknown protocol %r" % (protocol,))
    if f_real_l.requires_grad or f_real_p_l.requires_grad:
        raise NotImplementedError("the loss path never differentiates w.r.t. real (kernel_train.py:252,289)")
    Bl = f_real_l.shape[0]
    vids = (f_real_l, f_fake_l, f_real_p_l, f_fake_p_l)
    if any(v.shape != vids[0].shape for v in vids[1:]):
        raise ValueError("the four video shards must have the same shape: %s" % ([tuple(v.shape) for v in vids],))
    fl = (h_fake_l, m_real_l, h_real_p_l, m_fake_l, h_fake_p_l, m_real_p_l)
    if any(t.dim() != 3 or t.shape != fl[0].shape for t in fl) or fl[0].shape[0] != Bl:
        raise ValueError("the six feature shards must all be [B/G,T,J] with the videos' B/G; got %s" % ([tuple(t.shape) for t in fl],))
    cast = (lambda v: v.float()) if ops is HipOps else (lambda v: v)   # the HIP kernels are fp32
    flat = lambda v: cast(v.reshape(Bl, -1)).contiguous()
    return _ShardedMixedLoss.apply(*(flat(v) for v in vids), *(cast(t).contiguous() for t in fl), float(scaling_coef),
                                   float(epsilon), int(L), group, ops).reshape(())


# ---- the RBF-kernel MMD of the global batch -------------------------------------------
class _ShardedRbfMMD2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, real_l, fake_l, gamma, group, ops, real_all, fake_all):
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        Bl, K = real_l.shape
        B = Bl * world
        dev = real_l.device
        keep = ctx.needs_input_grad[1]
        _mark("start")
        # matrix-pipe row blocks need x.x, e.e, x.e of every sample: each rank's own rows, 24 bytes per sample gathered
        norms = None
        if (hasattr(ops, "row_norms") and hasattr(ops, "rows_gram_supported") and ops.rows_gram_supported(Bl, B, K)
                and os.environ.get("KCCOT_DIST_ROWS") != "direct"):
            norms = torch.empty((B, 3), dtype=torch.float64, device=dev)
            _gather_into(norms, ops.row_norms(real_l, fake_l), group)
        if real_all is None:                         # the videos straight into preallocated [B,K] buffers
            real_all = torch.empty((B, K), dtype=real_l.dtype, device=dev)
            fake_all = torch.empty((B, K), dtype=real_l.dtype, device=dev)
            _gather_into(real_all, real_l, group)
            _gather_into(fake_all, fake_l, group)
        _mark("exchange_inputs")
        blk = ops.mmd_cost_rows(real_all, fake_all, rank * Bl, Bl, norms)        # [3,Bl,B] squared distances
        _mark("cost_rows")
        blk, sums = ops.rbf_sum_rows(blk, gamma)                                 # kernel values, their 3 fp64 sums
        _mark("mmd_rows")
        _all_reduce_sum(sums, group)
        K3 = None
        if keep:    # the kernel matrices for the backward travel now: no collective inside backward
            K3 = all_gather_cat(blk.transpose(0, 1).contiguous(), group).transpose(0, 1).contiguous()      # [3,B,B]
        _mark("reduce")
        # sums = (Sxy, Sxx, Syy); the expression of the single-GPU kernel (csrc/martingale.hip, rbf_mmd)
        m = ((sums[1] + sums[2] - 2.0 * sums[0]) / float(B * B)).to(real_l.dtype)
        ctx.saved_state = (K3, real_all, fake_all)
        ctx.cfg = (gamma, rank * Bl, Bl, ops)
        return m

    @staticmethod
    def backward(ctx, g):
        K3, real_all, fake_all = ctx.saved_state
        gamma, row_begin, Bl, ops = ctx.cfg
        if ctx.needs_input_grad[0]:
            raise NotImplementedError("the loss path never differentiates w.r.t. real (kernel_train.py:252,289)")
        _mark("between_fwd_and_bwd")
        gD3 = ops.rbf_mmd_grad(K3, gamma, g.reshape(()))
        dfake = ops.dfake_rows(gD3, real_all, fake_all, 1.0, row_begin, Bl)
        _mark("gradient")
        return None, dfake, None, None, None, None, None


def sharded_rbf_mmd2(real_l, fake_l, gamma=None, group=None, ops=None, gathered=None):
    """mmd.rbf_mmd2 -- mean(Kxx) + mean(Kyy) - 2 mean(Kxy), K(a,b) = exp(-gamma |a-b|^2), biased, diagonals included -- of
    the GLOBAL batch of B = G B/G samples from per-rank shards ``real_l``, ``fake_l`` [B/G, ...].  ``gamma=None``: 1 / K, K
    the flattened feature count (sklearn's default).  Returns the same bits on every rank.  Differentiable w.r.t. ``fake_l``
    (each rank receives the gradient of its own samples; combine parameter gradients with an all-reduce SUM, as for the
    sharded losses); a real shard that requires a gradient raises NotImplementedError.

    Data flow: row norms of the local shard and the two videos are all-gathered (``gathered=(real_all, fake_all)``: videos
    [B, ...] that a sharded loss has gathered already are used instead, so a training step pays that all-gather once; they
    are read, never differentiated: the gradient still goes to ``fake_l``); rank g forms its rows of the three squared-
    distance matrices (the matrix pipe when kccot_pairwise_cost3_rows_gram_supported, the direct kernel otherwise;
    KCCOT_DIST_ROWS=direct forces the latter), turns them into kernel values and three fp64 sums in place
    (KCCOT_COST_RBF_SUM), the 3 doubles are all-reduced(SUM), mmd^2 = (Sxx + Syy - 2 Sxy) / B^2.  When ``fake_l`` requires
    a gradient the kernel row blocks are all-gathered in the forward (3 B^2 floats), so the backward -- kccot_rbf_mmd_bwd_f32
    on the full matrices, kccot_pairwise_cost3_bwd_rows_f32 for this rank's rows -- has no collective.  The ksplit protocol
    and KCCOT_DIST_GATHER_CHUNKS do not apply.  Injected ``ops`` must provide MMD_OPS.

    Without an initialised process group (and ``group=None``) this is ``mmd.rbf_mmd2(real_l, fake_l, gamma)``."""
    ops = ops or HipOps
    missing = [n for n in MMD_OPS if not hasattr(ops, n)]
    if missing:
        raise NotImplementedError("sharded rbf mmd: the ops %r lack %s" % (getattr(ops, "__name__", ops), ", ".join(missing)))
    if real_l.requires_grad:
        raise NotImplementedError("the loss path never differentiates w.r.t. real (kernel_train.py:252,289)")
    if real_l.shape != fake_l.shape or real_l.dim() < 2:
        raise ValueError("the real and fake shards must have the same shape [B/G, ...]: %s vs %s"
                         % (tuple(real_l.shape), tuple(fake_l.shape)))
    Bl = real_l.shape[0]
    Kf = real_l[0].numel()
    if Bl < 1 or Kf < 1:
        raise ValueError("empty shard %s" % (tuple(real_l.shape),))
    gamma = 1.0 / Kf if gamma is None else float(gamma)
    if not gamma > 0.0:
        raise ValueError("gamma must be positive (got %r)" % (gamma,))
    if gathered is not None and (len(gathered) != 2 or gathered[0].shape != gathered[1].shape
                                 or gathered[0].shape[1:] != real_l.shape[1:]):
        raise ValueError("gathered must be (real_all, fake_all), two [B, ...] videos of the shards' sample shape")
    if group is None and ops is HipOps and not (dist.is_available() and dist.is_initialized()):
        from . import mmd
        return mmd.rbf_mmd2(real_l, fake_l, gamma)
    cast = (lambda v: v.float()) if ops is HipOps else (lambda v: v)   # the HIP kernels are fp32
    real_all = fake_all = None
    if gathered is not None:
        B = Bl * dist.get_world_size(group)
        if gathered[0].shape[0] != B:
            raise ValueError("gathered videos hold %d samples, the global batch has %d" % (gathered[0].shape[0], B))
        real_all, fake_all = (cast(v.detach().reshape(B, -1)).contiguous() for v in gathered)
    flat = lambda v: cast(v.reshape(Bl, -1)).contiguous()
    return _ShardedRbfMMD2.apply(flat(real_l), flat(fake_l), gamma, group, ops, real_all, fake_all).reshape(())


# ---- helpers used by bench.py ---------------------------------------------------------------------
def shard_batch(t, rank, world):
    """Slice the leading (batch) axis of every tensor of a dict into this rank's shard."""
    out = {}
    for k, v in t.items():
        B = v.shape[0]
        if B % world:
            raise ValueError("batch %d is not divisible by %d ranks" % (B, world))
        s = v.detach()[rank * (B // world):(rank + 1) * (B // world)].contiguous()
        out[k] = s.requires_grad_(k != "real")
    return out


def sharded_loss_step(shard, sc, group=None, epsilon=1.0, L=100, protocol=None, bi_causal=False):
    fn = sharded_bicausal_sinkhorn_loss if bi_causal else sharded_sinkhorn_loss
    loss = fn(shard["real"], shard["fake"], sc, shard["h_fake"], shard["m_real"], shard["h_real"], shard["m_fake"], group,
              epsilon=epsilon, L=L, protocol=protocol)
    grads = torch.autograd.grad(loss, [shard[k] for k in ("fake", "h_fake", "h_real", "m_real", "m_fake")])
    return loss, grads


_MIXED_WRT = ("fake", "fake_p", "h_fake", "m_real", "h_real_p", "m_fake", "h_fake_p", "m_real_p")


def sharded_mixed_loss_step(shard, sc, group=None, epsilon=1.0, L=100):
    """sharded_mixed_sinkhorn_loss of one rank's shard dict (real, fake, real_p, fake_p and the six features) and its
    gradients w.r.t. _MIXED_WRT.  Both real videos are detached here, whatever the caller passed."""
    loss = sharded_mixed_sinkhorn_loss(shard["real"].detach(), shard["fake"], shard["real_p"].detach(), shard["fake_p"], sc,
                                       shard["h_fake"], shard["m_real"], shard["h_real_p"], shard["m_fake"], shard["h_fake_p"],
                                       shard["m_real_p"], group, epsilon=epsilon, L=L)
    grads = torch.autograd.grad(loss, [shard[k] for k in _MIXED_WRT])
    return loss, grads
