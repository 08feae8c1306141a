"""Guarded device buffers and the entry-point table of the bounds tests (tests/test_gpu_abi_bounds.py).

Not a test module and not a conftest: pytest does not collect it.  The table (ENTRIES) imports without a GPU, so the CPU
suite can check that every entry point of include/kccot.h that writes device memory has bounds coverage.

A guarded buffer is ONE torch uint8 allocation laid out as [front guard | payload | back guard]:
  - the payload starts at a multiple of 256 bytes (plus an optional 4-byte offset, for the misaligned-pointer cases);
  - the back guard is at least max(1 MiB, payload bytes), so a record overrun hundreds of KB long still lands in it;
  - both guards hold GUARD_WORD (a NaN as fp32) and are compared byte for byte by verify().
Workspaces are exactly kccot_*_workspace_bytes(...) bytes long: the guard begins where the query says the workspace ends.
"""
import numpy as np

GUARD_WORD = 0x7FBADBAD      # guard zones; also the workspace "sentinel" fill (a NaN as fp32)
FILL_WORD = 0x7FF1F1F1       # output pre-fill: NaN as fp32, NaN as fp64 (two words), an unlikely int32
FRONT = 4096
MIN_BACK = 1 << 20


class Guarded:
    """One payload of `nbytes` between two guard zones.  `offset` (0 or a multiple of 4 below 256) shifts the payload off
    its 256-byte alignment: the pointer handed to the library is then only 4-byte aligned."""

    def __init__(self, name, nbytes, offset=0, device="cuda"):
        import torch
        assert offset % 4 == 0 and 0 <= offset < 256
        self.name, self.nbytes, self.offset = name, int(nbytes), int(offset)
        self.back = max(MIN_BACK, self.nbytes)
        self.lo = FRONT + self.offset
        self.hi = self.lo + self.nbytes
        total = self.hi + self.back
        total += (-total) % 4
        self.buf = torch.empty(total, dtype=torch.uint8, device=device)
        self.words = self.buf.view(torch.int32)          # (storage offset 0: the whole allocation as words)
        self.words.fill_(_s32(GUARD_WORD))
        self.expect_front = self.buf[:self.lo].clone()
        self.expect_back = self.buf[self.hi:].clone()

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.lo if self.nbytes else None

    def payload(self):
        return self.buf[self.lo:self.hi]

    def view(self, dtype, shape):
        import torch
        p = self.payload().view(dtype)
        n = int(np.prod(shape)) if len(shape) else 1
        assert p.numel() == n, (self.name, p.numel(), n)
        return p.view(*shape) if len(shape) else p.view(())

    def fill(self, word):
        import torch
        if self.nbytes:
            self.payload().view(torch.int32).fill_(_s32(word))

    def zero(self):
        if self.nbytes:
            self.payload().zero_()

    def verify(self):
        """Message naming the damaged side(s), or None."""
        msgs = []
        for side, got, want, base in (("front", self.buf[:self.lo], self.expect_front, -self.lo),
                                      ("back", self.buf[self.hi:], self.expect_back, 0)):
            bad = (got != want).nonzero()
            if bad.numel():
                first = int(bad[0, 0]) + base
                msgs.append("%s: %d bad bytes %s the payload, first at payload offset %d (payload %d bytes)"
                            % (self.name, int(bad.numel()), "behind" if side == "back" else "in front of", first if side == "front"
                               else self.nbytes + first, self.nbytes))
        return "; ".join(msgs) or None


def _s32(w):
    return w - (1 << 32) if w >= (1 << 31) else w


def guarded(nbytes, kind, name="buffer", offset=0):
    """kind: "output" (payload pre-filled with FILL_WORD), "workspace" (GUARD_WORD sentinel), "zero" (zeros),
    "input" (left to the caller: copy_in)."""
    g = Guarded(name, nbytes, offset)
    if kind == "output":
        g.fill(FILL_WORD)
    elif kind == "workspace":
        g.fill(GUARD_WORD)
    elif kind == "zero":
        g.zero()
    return g


def guarded_input(name, t, offset=0):
    """A copy of tensor `t` in a guarded buffer (the library must neither write it nor read past it)."""
    g = Guarded(name, t.numel() * t.element_size(), offset, t.device)
    g.view(t.dtype, tuple(t.shape)).copy_(t)
    return g


def unwritten(t):
    """Boolean mask (per element of `t`) of elements that still hold the output pre-fill."""
    import torch
    w = t.contiguous().view(torch.int32)
    if t.element_size() == 8:
        w = w.view(-1, 2)
        return ((w[:, 0] == _s32(FILL_WORD)) & (w[:, 1] == _s32(FILL_WORD))).view(t.shape)
    return (w == _s32(FILL_WORD)).view(t.shape)


def same_bits(a, b):
    import torch
    if a.element_size() == 8:
        return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- the entry-point table --------------------------------------------------------------------------------------------
# symbol -> (test that covers it, device outputs and the region the header says is written, workspace query or None).
# Regions: "all" = every element; "rows" = the [row_begin, row_begin + row_count) block; "hist" = u_hist / v_hist up to the
# executed iterations (the rest keeps the pre-fill); "stats" = only stats_inout under STATS_ONLY (din untouched);
# "ticket" = one int32 that is zero on entry and must be zero again on exit.
COST_B = (1, 7, 8, 63, 64, 65, 127, 128, 129, 256, 257)
SINKHORN_N = (1, 2, 33, 64, 65, 128, 129, 256, 257, 1024)
LOSS_B = (8, 40, 64, 65, 192, 256)


def E(test, outputs, ws=None):
    return {"test": test, "outputs": outputs, "ws": ws}


ENTRIES = {
    "kccot_pairwise_cost_f32": E("test_pairwise_cost", {"C_out": "all"}, "kccot_pairwise_cost_workspace_bytes"),
    "kccot_pairwise_cost3_f32": E("test_cost3", {"C3": "all"}, "kccot_pairwise_cost3_workspace_bytes"),
    "kccot_pairwise_cost3_rows_f32": E("test_cost3_rows", {"C3_rows": "all"}, "kccot_pairwise_cost3_rows_workspace_bytes"),
    "kccot_row_norms_f64": E("test_rows_gram", {"norms_out": "all"}, "kccot_row_norms_workspace_bytes"),
    "kccot_pairwise_cost3_rows_gram_f32": E("test_rows_gram", {"C3_rows": "all"}, "kccot_pairwise_cost3_rows_gram_workspace_bytes"),
    "kccot_pairwise_cost3_rows_gram_sums_f64": E("test_rows_gram", {"gsum": "all"}, "kccot_pairwise_cost3_rows_gram_workspace_bytes"),
    "kccot_pairwise_cost3_rows_gram_from_sums_f32": E("test_rows_gram", {"C3_rows": "all"}),
    "kccot_pairwise_cost3_bwd_f32": E("test_cost3_bwd", {"dfake": "all", "dh_fake": "all", "dh_real": "all", "dm_real": "all",
                                                         "dm_fake": "all"}, "kccot_pairwise_cost3_bwd_workspace_bytes"),
    "kccot_pairwise_cost3_bwd_rows_f32": E("test_cost3_bwd", {"dfake": "rows", "dh_fake": "rows", "dh_real": "rows",
                                                              "dm_real": "rows", "dm_fake": "rows"},
                                           "kccot_pairwise_cost3_bwd_workspace_bytes"),
    "kccot_pairwise_cost3_bwd_scaled_f32": E("test_cost3_bwd", {"dfake": "all", "dh_fake": "all", "dh_real": "all",
                                                                "dm_real": "all", "dm_fake": "all"},
                                             "kccot_pairwise_cost3_bwd_workspace_bytes"),
    "kccot_pairwise_cost_bwd_f32": E("test_pairwise_cost_bwd", {"dx": "all", "dy": "all", "dh": "all", "dM": "all"},
                                     "kccot_pairwise_cost_bwd_workspace_bytes"),
    "kccot_sinkhorn_fwd_f32": E("test_sinkhorn", {"u_hist": "hist", "v_hist": "hist", "cost_out": "all", "nits_out": "all",
                                                  "pi_out": "all"}, "kccot_sinkhorn_workspace_bytes"),
    "kccot_sinkhorn_bwd_f32": E("test_sinkhorn", {"dC_out": "all"}, "kccot_sinkhorn_workspace_bytes"),
    "kccot_sinkhorn_divergence_fwd_f32": E("test_divergence", {"u_hist": "hist", "v_hist": "hist", "cost3_out": "all",
                                                               "nits_out": "all", "loss_out": "all", "ticket": "ticket"},
                                           "kccot_sinkhorn_workspace_bytes"),
    "kccot_sinkhorn_divergence_bwd_f32": E("test_divergence", {"dC3_out": "all"}, "kccot_sinkhorn_workspace_bytes"),
    "kccot_sinkhorn_divergence_fused_f32": E("test_divergence", {"cost3_out": "all", "nits_out": "all", "loss_out": "all",
                                                                 "ticket": "ticket", "dC3_unit": "all"}),
    "kccot_sinkhorn_loss_fwd_f32": E("test_sinkhorn_loss", {"C3": "all", "u_hist": "hist", "v_hist": "hist", "cost3_out": "all",
                                                            "nits_out": "all", "loss_out": "all", "ticket": "ticket"},
                                     "kccot_sinkhorn_loss_workspace_bytes"),
    "kccot_sinkhorn_loss_bwd_f32": E("test_sinkhorn_loss", {"dfake": "all", "dh_fake": "all", "dh_real": "all", "dm_real": "all",
                                                            "dm_fake": "all"}, "kccot_sinkhorn_loss_workspace_bytes"),
    "kccot_sinkhorn_loss_fused_fwd_f32": E("test_sinkhorn_loss", {"C3": "all", "dC3_unit": "all", "cost3_out": "all",
                                                                  "nits_out": "all", "loss_out": "all", "ticket": "ticket"},
                                           "kccot_sinkhorn_loss_workspace_bytes"),
    "kccot_sinkhorn_loss_fused_bwd_f32": E("test_sinkhorn_loss", {"dfake": "all", "dh_fake": "all", "dh_real": "all",
                                                                  "dm_real": "all", "dm_fake": "all"},
                                           "kccot_sinkhorn_loss_workspace_bytes"),
    "kccot_mixed_divergence_fwd_f32": E("test_mixed_divergence", {"loss_out": "all"}),
    "kccot_mixed_divergence_bwd_f32": E("test_mixed_divergence", {"gcost3_out": "all"}),
    "kccot_mixed_sinkhorn_loss_fwd_f32": E("test_two_sample_losses", {"Cmix": "all", "u_hist": "hist", "v_hist": "hist",
                                                                      "dCmix_unit": "all", "cost4_out": "all", "nits_out": "all",
                                                                      "loss_out": "all", "ticket": "ticket"},
                                           "kccot_mixed_sinkhorn_loss_workspace_bytes"),
    "kccot_mixed_sinkhorn_loss_bwd_f32": E("test_two_sample_losses", {"dF": "all", "dh_fake": "all", "dm_real": "all",
                                                                      "dh_real_p": "all", "dm_fake": "all", "dh_fake_p": "all",
                                                                      "dm_real_p": "all"},
                                           "kccot_mixed_sinkhorn_loss_workspace_bytes"),
    "kccot_bicausal_sinkhorn_loss_fwd_f32": E("test_two_sample_losses", {"C3": "all", "u_hist": "hist", "v_hist": "hist",
                                                                         "dC3_unit": "all", "cost3_out": "all", "nits_out": "all",
                                                                         "loss_out": "all", "ticket": "ticket"},
                                              "kccot_bicausal_sinkhorn_loss_workspace_bytes"),
    "kccot_bicausal_sinkhorn_loss_bwd_f32": E("test_two_sample_losses", {"dfake": "all", "dh_fake": "all", "dh_real": "all",
                                                                         "dm_real": "all", "dm_fake": "all"},
                                              "kccot_bicausal_sinkhorn_loss_workspace_bytes"),
    "kccot_martingale_fwd_f32": E("test_martingale", {"pm_out": "all"}),
    "kccot_martingale_bwd_f32": E("test_martingale", {"dM": "all"}),
    "kccot_convlstm_cell_fwd_f32": E("test_convlstm_cell", {"c_out": "all", "h_out": "all"}),
    "kccot_convlstm_cell_bwd_f32": E("test_convlstm_cell", {"dg": "all", "dc_prev": "all"}),
    "kccot_channel_layernorm_fwd_f32": E("test_channel_layernorm", {"y": "all", "mean": "all", "rstd": "all"}),
    "kccot_channel_layernorm_bwd_f32": E("test_channel_layernorm", {"dx": "all", "partials": "all"}),
    "kccot_rbf_mmd_f32": E("test_rbf_mmd", {"K3_out": "all", "mmd_out": "all"}),
    "kccot_rbf_mmd_bwd_f32": E("test_rbf_mmd", {"gD3": "all"}),
    "kccot_smooth_fwd_f32": E("test_smoothing", {"out": "all", "max_inout": "all"}, "kccot_smooth_workspace_bytes"),
    "kccot_smooth_bwd_f32": E("test_smoothing", {"din": "all"}, "kccot_smooth_workspace_bytes"),
    "kccot_smooth_bwd_sharded_f32": E("test_smoothing", {"stats_inout": "stats", "din": "all"}, "kccot_smooth_workspace_bytes"),
}

# entry points whose non-const pointers are HOST pointers (queries; nothing on the device is written)
HOST_OUTPUTS = {"kccot_get_option": ["value"], "kccot_pairwise_cost3_gram_sums_span": ["byte_offset", "n_doubles"]}
