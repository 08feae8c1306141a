"""ctypes binding of the C-ABI library ``csrc/libkccot.so`` (declared in ``include/kccot.h``, ``include/kccot_models.h``,
``include/kccot_weighted.h``, ``include/kccot_conditional.h``, ``include/kccot_weight_grad.h``,
``include/kccot_smooth_causal3.h``, ``include/kccot_smooth_sigma.h``, ``include/kccot_smooth_aniso.h``,
``include/kccot_metrics.h``, ``include/kccot_l1.h`` and ``include/kccot_swd.h``).

The HIP library is the product: there is NO CPU fallback anywhere in this package.  If the
shared object is missing or a call is made without a GPU tensor the import / call fails loudly.
PyTorch is used for device memory, streams and autograd plumbing only.
"""
import ctypes
import os

import torch  # must be imported first: the library then binds to the HIP runtime torch already loaded

_HERE = os.path.dirname(os.path.abspath(__file__))
# KCCOT_LIB_PATH: load another build of the SAME library (tools only: csrc/libkccot_diag.so, the diagnostic twin with
# in-kernel stamps and timing-experiment kernel variants; never set by the package or the tests)
LIB_PATH = os.environ.get("KCCOT_LIB_PATH") or os.path.join(_HERE, "csrc", "libkccot.so")

EINVAL, EUNSUPPORTED, EWORKSPACE, EABORTED = -1, -2, -3, -4

COST_SAME, COST_FORCE_DIRECT, COST_FORCE_MFMA, COST_PARTIAL_ONLY = 1, 2, 4, 8
COST_GRAM_SUMS_ONLY, COST_FROM_GRAM_SUMS, COST_BICAUSAL_TERM_ONLY = 16, 32, 64
COST_CAUSAL_ADD, MIXED_CMIX_GIVEN, COST_RBF_SUM = 128, 256, 512
COST_L1 = 1024            # the L1 ground cost on the direct-difference kernel; with COST_SAME / COST_FORCE_DIRECT only
STOP_COUNT, STOP_INDEX = 0, 1
SMOOTH_T, SMOOTH_H, SMOOTH_W, SMOOTH_NO_DIVIDE, SMOOTH_EXTERNAL_MAX = 1, 2, 4, 16, 32
SMOOTH_STATS_ONLY, SMOOTH_EXTERNAL_STATS = 64, 128
SMOOTH_CAUSAL_T = 8       # one-sided (past-only) T stencil; with SMOOTH_T alone

_c = ctypes
_fp = _c.c_void_p      # device pointers travel as plain addresses
_i, _i64, _f, _u, _sz = _c.c_int, _c.c_int64, _c.c_float, _c.c_uint, _c.c_size_t
_u64 = _c.c_uint64

# name -> (restype, argtypes); mirrors include/kccot.h one to one
SIGNATURES = {
    "kccot_version": (_i, []),
    "kccot_last_error": (_c.c_char_p, []),
    "kccot_set_option": (_i, [_c.c_char_p, _i]),
    "kccot_get_option": (_i, [_c.c_char_p, _c.POINTER(_i)]),
    "kccot_option_count": (_i, []),
    "kccot_option_name": (_c.c_char_p, [_i]),
    "kccot_pairwise_cost_workspace_bytes": (_sz, [_i, _i, _i64]),
    "kccot_pairwise_cost_f32": (_i, [_fp, _fp, _i, _i, _i64, _f, _fp, _fp, _fp, _fp, _i, _i, _u, _fp, _fp, _sz, _fp]),
    "kccot_pairwise_cost3_workspace_bytes": (_sz, [_i, _i64]),
    "kccot_pairwise_cost3_f32": (_i, [_fp, _fp, _i, _i64, _f, _fp, _fp, _fp, _fp, _i, _i, _u, _fp, _fp, _sz, _fp]),
    "kccot_pairwise_cost3_gram_sums_span": (_i, [_i, _i64, _c.POINTER(_sz), _c.POINTER(_sz)]),
    "kccot_pairwise_cost3_rows_workspace_bytes": (_sz, [_i, _i, _i64]),
    "kccot_pairwise_cost3_rows_f32": (_i, [_fp, _fp, _i, _i64, _f, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _fp, _fp, _sz, _fp]),
    "kccot_pairwise_cost3_rows_gram_supported": (_i, [_i, _i, _i64]),
    "kccot_pairwise_cost3_rows_gram_workspace_bytes": (_sz, [_i, _i, _i64]),
    "kccot_row_norms_workspace_bytes": (_sz, [_i]),
    "kccot_row_norms_f64": (_i, [_fp, _fp, _i, _i64, _fp, _fp, _sz, _fp]),
    "kccot_pairwise_cost3_rows_gram_f32": (_i, [_fp, _fp, _i, _i64, _f, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _fp, _fp, _fp, _sz, _fp]),
    "kccot_pairwise_cost3_rows_gram_sums_count": (_sz, [_i, _i]),
    "kccot_pairwise_cost3_rows_gram_sums_f64": (_i, [_fp, _fp, _i, _i64, _i, _i, _fp, _i, _fp, _sz, _fp]),
    "kccot_pairwise_cost3_rows_gram_from_sums_f32": (_i, [_fp, _i, _f, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _fp, _fp, _fp]),
    "kccot_pairwise_cost3_bwd_workspace_bytes": (_sz, [_i, _i64]),
    "kccot_pairwise_cost3_bwd_f32": (_i, [_fp, _fp, _fp, _i, _i64, _f, _fp, _fp, _fp, _fp, _i, _i,
                                          _fp, _fp, _fp, _fp, _fp, _fp, _sz, _fp]),
    "kccot_pairwise_cost3_bwd_rows_f32": (_i, [_fp, _fp, _fp, _i, _i64, _f, _fp, _fp, _fp, _fp, _i, _i, _i, _i,
                                               _fp, _fp, _fp, _fp, _fp, _fp, _sz, _fp]),
    "kccot_pairwise_cost_bwd_workspace_bytes": (_sz, [_i, _i]),
    "kccot_pairwise_cost_bwd_f32": (_i, [_fp, _fp, _fp, _i, _i, _i64, _f, _fp, _fp, _i, _i, _u,
                                         _fp, _fp, _fp, _fp, _fp, _sz, _fp]),
    "kccot_sinkhorn_workspace_bytes": (_sz, [_i, _i]),
    "kccot_sinkhorn_fwd_f32": (_i, [_fp, _i, _i, _f, _i, _i, _f, _i, _fp, _fp, _fp, _fp, _fp, _fp, _sz, _fp]),
    "kccot_sinkhorn_status": (_i, [_fp, _i, _fp]),
    "kccot_sinkhorn_bwd_f32": (_i, [_fp, _fp, _fp, _fp, _i, _i, _f, _i, _fp, _fp, _fp, _sz, _fp]),
    "kccot_sinkhorn_divergence_fwd_f32": (_i, [_fp, _i, _f, _i, _i, _f, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _sz, _fp]),
    "kccot_sinkhorn_divergence_bwd_f32": (_i, [_fp, _fp, _fp, _fp, _i, _f, _i, _fp, _fp, _fp, _sz, _fp]),
    "kccot_sinkhorn_loss_workspace_bytes": (_sz, [_i, _i64]),
    "kccot_sinkhorn_loss_fwd_f32": (_i, [_fp, _fp, _i, _i64, _f, _fp, _fp, _fp, _fp, _i, _i, _f, _i, _i, _f, _u,
                                         _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _sz, _fp]),
    "kccot_sinkhorn_loss_bwd_f32": (_i, [_fp, _fp, _fp, _i, _i64, _f, _fp, _fp, _fp, _fp, _i, _i, _f, _i,
                                         _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _sz, _fp]),
    "kccot_sinkhorn_fused_eligible": (_i, [_i, _i]),
    "kccot_sinkhorn_fused_roles_eligible": (_i, [_i, _i]),
    "kccot_sinkhorn_divergence_fused_f32": (_i, [_fp, _i, _f, _i, _i, _f, _fp, _fp, _fp, _fp, _fp, _fp]),
    "kccot_pairwise_cost3_bwd_scaled_f32": (_i, [_fp, _fp, _fp, _fp, _i, _i64, _f, _fp, _fp, _fp, _fp, _i, _i,
                                                 _fp, _fp, _fp, _fp, _fp, _fp, _sz, _fp]),
    "kccot_sinkhorn_loss_fused_fwd_f32": (_i, [_fp, _fp, _i, _i64, _f, _fp, _fp, _fp, _fp, _i, _i, _f, _i, _i, _f, _u,
                                               _fp, _fp, _fp, _fp, _fp, _fp, _fp, _sz, _fp]),
    "kccot_sinkhorn_loss_fused_bwd_f32": (_i, [_fp, _fp, _fp, _fp, _i, _i64, _f, _fp, _fp, _fp, _fp, _i, _i,
                                               _fp, _fp, _fp, _fp, _fp, _fp, _sz, _fp]),
    "kccot_mixed_divergence_fwd_f32": (_i, [_fp, _fp, _fp]),
    "kccot_mixed_divergence_bwd_f32": (_i, [_fp, _fp, _fp]),
    "kccot_mixed_sinkhorn_loss_workspace_bytes": (_sz, [_i, _i64]),
    "kccot_mixed_sinkhorn_loss_fwd_f32": (_i, [_fp, _fp, _i, _i64, _f, _fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _f, _i, _i, _f,
                                               _u, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _sz, _fp]),
    "kccot_mixed_sinkhorn_loss_bwd_f32": (_i, [_fp, _fp, _fp, _i, _i64, _f, _fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _f, _i,
                                               _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _sz, _fp]),
    "kccot_bicausal_sinkhorn_loss_workspace_bytes": (_sz, [_i, _i64]),
    "kccot_bicausal_sinkhorn_loss_fwd_f32": (_i, [_fp, _fp, _i, _i64, _f, _fp, _fp, _fp, _fp, _i, _i, _f, _i, _i, _f, _u,
                                                  _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _sz, _fp]),
    "kccot_bicausal_sinkhorn_loss_bwd_f32": (_i, [_fp, _fp, _fp, _i, _i64, _f, _fp, _fp, _fp, _fp, _i, _i, _f, _i, _fp, _fp,
                                                  _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _sz, _fp]),
    "kccot_martingale_fwd_f32": (_i, [_fp, _i, _i, _i, _f, _f, _fp, _fp]),
    "kccot_martingale_bwd_f32": (_i, [_fp, _i, _i, _i, _f, _f, _fp, _fp, _fp]),
    "kccot_rbf_mmd_f32": (_i, [_fp, _i, _f, _fp, _fp, _fp]),
    "kccot_rbf_mmd_bwd_f32": (_i, [_fp, _i, _f, _fp, _fp, _fp]),
    "kccot_smooth_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "kccot_smooth_fwd_f32": (_i, [_fp, _i, _i, _i, _i, _i, _f, _i, _u, _fp, _fp, _fp, _sz, _fp]),
    "kccot_channel_layernorm_chunks": (_i, [_i, _i, _i]),
    "kccot_channel_layernorm_fwd_f32": (_i, [_fp, _fp, _fp, _i, _i, _i, _f, _fp, _fp, _fp, _fp]),
    "kccot_channel_layernorm_bwd_f32": (_i, [_fp, _fp, _fp, _fp, _fp, _i, _i, _i, _fp, _fp, _fp]),
    "kccot_convlstm_cell_fwd_f32": (_i, [_fp, _fp, _fp, _i, _i, _i, _fp, _fp, _fp]),
    "kccot_convlstm_cell_bwd_f32": (_i, [_fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _i, _fp, _fp, _fp]),
    "kccot_smooth_bwd_f32": (_i, [_fp, _fp, _fp, _i, _i, _i, _i, _i, _f, _i, _u, _fp, _fp, _sz, _fp]),
    "kccot_smooth_bwd_sharded_f32": (_i, [_fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _f, _i, _u, _fp, _fp, _sz, _fp]),
}


# name -> (restype, argtypes); mirrors include/kccot_models.h one to one (model-side kernels, outside the versioned
# surface of kccot.h)
MODEL_SIGNATURES = {
    "kccot_sigmoid_lstm_fwd_f32": (_i, [_fp, _fp, _i, _i, _i, _fp, _fp, _fp]),
    "kccot_sigmoid_lstm_bwd_f32": (_i, [_fp, _fp, _fp, _fp, _fp, _i, _i, _i, _fp, _fp]),
}


# name -> (restype, argtypes); mirrors include/kccot_weighted.h one to one (the Sinkhorn solver and the one-batch loss with
# weighted marginals: an extension outside the versioned surface of kccot.h)
WEIGHTED_SIGNATURES = {
    "kccot_sinkhorn_weighted_fwd_f32": (_i, [_fp, _fp, _fp, _i, _i, _f, _i, _i, _f, _i, _fp, _fp, _fp, _fp, _fp, _fp, _sz,
                                             _fp]),
    "kccot_sinkhorn_weighted_bwd_f32": (_i, [_fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _f, _i, _fp, _fp, _fp, _sz, _fp]),
    "kccot_weighted_sinkhorn_loss_workspace_bytes": (_sz, [_i, _i64]),
    "kccot_weighted_sinkhorn_loss_fwd_f32": (_i, [_fp, _fp, _i, _i64, _f, _fp, _fp, _fp, _fp, _i, _i, _f, _i, _i, _f, _u,
                                                  _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _sz, _fp]),
    "kccot_weighted_sinkhorn_loss_bwd_f32": (_i, [_fp, _fp, _fp, _i, _i64, _f, _fp, _fp, _fp, _fp, _i, _i, _f, _i, _fp, _fp,
                                                  _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _sz, _fp]),
}


# name -> (restype, argtypes); mirrors include/kccot_conditional.h one to one (the kernel-conditional Sinkhorn loss -- Q
# weighted solves on shared cost matrices -- and its weight estimator: an extension outside the versioned surface of kccot.h)
CONDITIONAL_SIGNATURES = {
    "kccot_conditional_weights_f32": (_i, [_fp, _i, _i, _f, _fp, _fp]),
    "kccot_sinkhorn_conditional_workspace_bytes": (_sz, [_i, _i]),
    "kccot_sinkhorn_conditional_fwd_f32": (_i, [_fp, _fp, _fp, _i, _i, _f, _i, _i, _f, _fp, _fp, _fp, _fp, _fp, _fp, _sz, _fp]),
    "kccot_sinkhorn_conditional_bwd_f32": (_i, [_fp, _fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _f, _i, _fp, _fp, _sz, _fp]),
    "kccot_conditional_sinkhorn_loss_workspace_bytes": (_sz, [_i, _i64, _i]),
    "kccot_conditional_sinkhorn_loss_fwd_f32": (_i, [_fp, _fp, _i, _i64, _f, _fp, _fp, _fp, _fp, _i, _i, _f, _i, _i, _f, _u,
                                                     _fp, _fp, _i, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _sz, _fp]),
    "kccot_conditional_sinkhorn_loss_bwd_f32": (_i, [_fp, _fp, _fp, _i, _i64, _f, _fp, _fp, _fp, _fp, _i, _i, _f, _i, _fp, _fp,
                                                     _i, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _sz, _fp]),
}


# name -> (restype, argtypes); mirrors include/kccot_weight_grad.h one to one (the gradients of the weighted solver, the weighted
# loss and the kernel-conditional loss w.r.t. their WEIGHTS, and the adjoint of the weight estimator: an extension outside the
# versioned surface of kccot.h)
WEIGHT_GRAD_SIGNATURES = {
    "kccot_sinkhorn_weighted_bwd_dw_f32": (_i, [_fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _f, _i, _fp, _fp, _fp, _fp, _fp, _sz, _fp]),
    "kccot_weighted_sinkhorn_loss_dw_workspace_bytes": (_sz, [_i, _i64]),
    "kccot_weighted_sinkhorn_loss_bwd_dw_f32": (_i, [_fp, _fp, _fp, _i, _i64, _f, _fp, _fp, _fp, _fp, _i, _i, _f, _i, _fp, _fp,
                                                     _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _sz, _fp]),
    "kccot_sinkhorn_conditional_dw_workspace_bytes": (_sz, [_i, _i]),
    "kccot_sinkhorn_conditional_bwd_dw_f32": (_i, [_fp, _fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _f, _i, _fp, _fp, _fp, _fp, _fp,
                                                   _sz, _fp]),
    "kccot_conditional_sinkhorn_loss_dw_workspace_bytes": (_sz, [_i, _i64, _i]),
    "kccot_conditional_sinkhorn_loss_bwd_dw_f32": (_i, [_fp, _fp, _fp, _i, _i64, _f, _fp, _fp, _fp, _fp, _i, _i, _f, _i, _fp,
                                                        _fp, _i, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp,
                                                        _fp, _sz, _fp]),
    "kccot_conditional_weights_bwd_f32": (_i, [_fp, _fp, _fp, _i, _i, _f, _fp, _fp, _fp]),
    "kccot_conditional_weights_dev_f32": (_i, [_fp, _i, _i, _fp, _fp, _fp]),
    "kccot_conditional_weights_bwd_dev_f32": (_i, [_fp, _fp, _fp, _i, _i, _fp, _fp, _fp, _fp]),
}


# name -> (restype, argtypes); mirrors include/kccot_smooth_causal3.h one to one (the causal 3-D smoothing -- past-only in
# time, symmetric in space: an extension outside the versioned surface of kccot.h).  flags: the protocol bits only.
SMOOTH3C_SIGNATURES = {
    "kccot_smooth_causal3_fwd_f32": (_i, [_fp, _i, _i, _i, _i, _i, _f, _i, _u, _fp, _fp, _fp, _sz, _fp]),
    "kccot_smooth_causal3_bwd_f32": (_i, [_fp, _fp, _fp, _i, _i, _i, _i, _i, _f, _i, _u, _fp, _fp, _sz, _fp]),
    "kccot_smooth_causal3_bwd_sharded_f32": (_i, [_fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _f, _i, _u, _fp, _fp, _sz, _fp]),
}


# name -> (restype, argtypes); mirrors include/kccot_smooth_sigma.h one to one (the gradient of the kernel smoothing w.r.t. its
# bandwidth sigma: an extension outside the versioned surface of kccot.h).  axes_flags: axis bits and SMOOTH_CAUSAL_T only.
SMOOTH_SIGMA_SIGNATURES = {
    "kccot_smooth_dsigma_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "kccot_smooth_dsigma_f32": (_i, [_fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _f, _i, _u, _fp, _fp, _sz, _fp]),
    "kccot_smooth_dsigma_plan": (_i, [_i, _i, _i, _i, _i, _i, _u, _fp]),      # host only; out: DSIGMA_PLAN_INTS ints
}


# name -> (restype, argtypes); mirrors include/kccot_smooth_aniso.h one to one (the anisotropic 3-D smoothing -- one bandwidth
# and radius along T, another along H and W: an extension outside the versioned surface of kccot.h).  flags: SMOOTH_CAUSAL_T
# and the protocol bits only.
SMOOTH_ANISO_SIGNATURES = {
    "kccot_smooth_aniso_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "kccot_smooth_aniso_fwd_f32": (_i, [_fp, _i, _i, _i, _i, _i, _f, _i, _f, _i, _u, _fp, _fp, _fp, _sz, _fp]),
    "kccot_smooth_aniso_bwd_f32": (_i, [_fp, _fp, _fp, _i, _i, _i, _i, _i, _f, _i, _f, _i, _u, _fp, _fp, _sz, _fp]),
    "kccot_smooth_aniso_bwd_sharded_f32": (_i, [_fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _f, _i, _f, _i, _u, _fp, _fp, _sz, _fp]),
    "kccot_smooth_aniso_dsigma_f32": (_i, [_fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _f, _i, _f, _i, _u, _fp, _fp, _sz, _fp]),
    "kccot_smooth_aniso_plan": (_i, [_i, _i, _i, _i, _i, _i, _i, _u, _i, _fp]),      # host only; out: ANISO_PLAN_INTS ints
}


# name -> (restype, argtypes); mirrors include/kccot_metrics.h one to one (per-frame SSIM with its adjoint w.r.t. the generated
# video, and the mean squared error behind PSNR: an extension outside the versioned surface of kccot.h)
METRICS_SIGNATURES = {
    "kccot_ssim_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "kccot_ssim_fwd_f32": (_i, [_fp, _fp, _i, _i, _i, _i, _i, _f, _i, _f, _fp, _fp, _fp, _sz, _fp]),
    "kccot_ssim_bwd_f32": (_i, [_fp, _fp, _fp, _i, _i, _i, _i, _i, _f, _i, _f, _fp, _fp, _sz, _fp]),
    "kccot_ssim_plan": (_i, [_i, _i, _i, _i, _i, _i, _i, _fp]),      # host only; out: SSIM_PLAN_INTS ints
}


# name -> (restype, argtypes); mirrors include/kccot_l1.h one to one (the adjoint of the L1 ground cost, whose forward is the
# flag COST_L1 of the two cost entry points: an extension outside the versioned surface of kccot.h)
L1_SIGNATURES = {
    "kccot_l1_cost_bwd_workspace_bytes": (_sz, [_i, _i]),
    "kccot_l1_cost_bwd_f32": (_i, [_fp, _fp, _fp, _i, _i, _i64, _f, _u, _fp, _fp, _fp, _sz, _fp]),
    "kccot_l1_cost3_bwd_workspace_bytes": (_sz, [_i]),
    "kccot_l1_cost3_bwd_f32": (_i, [_fp, _fp, _fp, _i, _i64, _f, _fp, _fp, _sz, _fp]),
}


# name -> (restype, argtypes); mirrors include/kccot_swd.h one to one (the sliced Wasserstein distance between two batches on
# directions generated on chip, and its adjoint: an extension outside the versioned surface of kccot.h)
SWD_SIGNATURES = {
    "kccot_swd_workspace_bytes": (_sz, [_i, _i64, _i]),
    "kccot_swd_fwd_f32": (_i, [_fp, _fp, _i, _i64, _i, _u64, _fp, _fp, _fp, _fp, _fp, _sz, _fp]),
    "kccot_swd_bwd_f32": (_i, [_fp, _fp, _fp, _fp, _i, _i64, _i, _u64, _fp, _fp, _fp, _sz, _fp]),
    "kccot_swd_directions_f32": (_i, [_u64, _i64, _i, _i, _fp, _fp]),
    "kccot_swd_plan": (_i, [_i, _i64, _i, _fp]),      # host only; out: SWD_PLAN_INTS ints
}


class KccotError(RuntimeError):
    pass


# ---- the host-only plan queries: which tiling, and which instantiation of the tile kernel, a launch would use (no device
# call: they work without a GPU).  The field names are those of the headers.
DSIGMA_PLAN_INTS, ANISO_PLAN_INTS, SSIM_PLAN_INTS = 17, 13, 8
SWD_PLAN_INTS = 8
_SWD_PLAN = ("kc", "chunks", "pt", "rt", "npt", "nrt", "np", "kt")
_DSIGMA_PLAN = ("launches", "R", "NI", "tt", "wt", "ct", "hs", "ntt", "ntw", "ntc", "nseg", "grid", "Bv", "Hv", "Tv", "Wv", "Cv")
_ANISO_PLAN = ("launches", "RS", "NI", "job", "tt", "wt", "ct", "hs", "ntt", "ntw", "ntc", "nseg", "grid")
_SSIM_PLAN = ("wt", "ct", "hs", "nt", "ntw", "ntc", "nseg", "grid")
ANISO_JOBS = {"fwd": 0, "adj": 1, "dsigma": 2}


def _plan(fn, names, what, *args):
    out = (_i * len(names))()
    check(fn(*args, out), what)
    return dict(zip(names, out))


def smooth_dsigma_plan(shape, radius, axes_flags):
    """kccot_smooth_dsigma_plan as a dict (include/kccot_smooth_sigma.h)"""
    return _plan(lib.kccot_smooth_dsigma_plan, _DSIGMA_PLAN, "smooth_dsigma_plan", *shape, radius, axes_flags)


def smooth_aniso_plan(shape, radius_t, radius_s, causal, job):
    """kccot_smooth_aniso_plan as a dict (include/kccot_smooth_aniso.h); job: "fwd", "adj" or "dsigma" """
    return _plan(lib.kccot_smooth_aniso_plan, _ANISO_PLAN, "smooth_aniso_plan", *shape, radius_t, radius_s,
                 SMOOTH_CAUSAL_T if causal else 0, ANISO_JOBS[job])


def ssim_plan(shape, radius, backward):
    """kccot_ssim_plan as a dict (include/kccot_metrics.h)"""
    return _plan(lib.kccot_ssim_plan, _SSIM_PLAN, "ssim_plan", *shape, radius, int(bool(backward)))


def swd_plan(B, K, P):
    """kccot_swd_plan as a dict (include/kccot_swd.h)"""
    return _plan(lib.kccot_swd_plan, _SWD_PLAN, "swd_plan", B, K, P)


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "kccotgan_amd: %s is missing -- build it with `make -C kccotgan_amd/csrc` "
            "(or `python -c 'import __graft_entry__ as g; g.build()'`).  There is no CPU fallback." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in (list(SIGNATURES.items()) + list(MODEL_SIGNATURES.items()) + list(WEIGHTED_SIGNATURES.items()) +
                              list(CONDITIONAL_SIGNATURES.items()) + list(WEIGHT_GRAD_SIGNATURES.items()) +
                              list(SMOOTH3C_SIGNATURES.items()) + list(SMOOTH_SIGMA_SIGNATURES.items()) +
                              list(SMOOTH_ANISO_SIGNATURES.items()) + list(METRICS_SIGNATURES.items()) +
                              list(L1_SIGNATURES.items()) + list(SWD_SIGNATURES.items())):
        fn = getattr(lib, name)  # AttributeError here = headers and library out of step
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


# ---- debugging aid: KCCOT_DEBUG_CANARY=1 surrounds every buffer the wrappers hand to the library
# (outputs and workspace) with sentinel-filled guard zones and verifies them after every call.
_CANARY = os.environ.get("KCCOT_DEBUG_CANARY") == "1"
_GUARD = 4096            # elements on either side
_SENT = 1234567.0
_guards = []


def empty(shape, dtype=torch.float32, device=None):
    if not _CANARY:
        return torch.empty(shape, dtype=dtype, device=device)
    n = 1
    for d in shape:
        n *= int(d)
    buf = torch.full((n + 2 * _GUARD,), _SENT, dtype=dtype, device=device)
    _guards.append((buf, n))
    del _guards[:-400]
    return buf[_GUARD:_GUARD + n].view(tuple(shape))


def empty_like(t):
    return empty(tuple(t.shape), t.dtype, t.device)


def _verify_guards(what):
    if torch.cuda.is_current_stream_capturing():
        return                      # no synchronisation inside a hipGraph capture: the next eager call verifies
    torch.cuda.synchronize()
    for buf, n in _guards:
        lo, hi = buf[:_GUARD], buf[_GUARD + n:]
        if not (bool((lo == _SENT).all()) and bool((hi == _SENT).all())):
            bad_lo = int((lo != _SENT).sum())
            bad_hi = int((hi != _SENT).sum())
            raise KccotError("guard zone overwritten after %s: buffer of %d elements (%s), %d bad below, %d bad above"
                             % (what, n, buf.dtype, bad_lo, bad_hi))


def check(rc, what):
    if _CANARY:
        _verify_guards(what)
    if rc == 0:
        return
    msg = lib.kccot_last_error().decode("utf-8", "replace")
    if rc == EINVAL:
        raise ValueError("%s: %s" % (what, msg))
    if rc == EUNSUPPORTED:
        raise NotImplementedError("%s: %s" % (what, msg))
    raise KccotError("%s failed (code %d): %s" % (what, rc, msg))


def set_option(name, value):
    """kccot_set_option (include/kccot.h lists the options).  Process-wide."""
    check(lib.kccot_set_option(name.encode(), int(value)), "set_option(%s)" % name)


def get_option(name):
    v = _i(0)
    check(lib.kccot_get_option(name.encode(), ctypes.byref(v)), "get_option(%s)" % name)
    return v.value


def option_names():
    return [lib.kccot_option_name(k).decode() for k in range(lib.kccot_option_count())]


class options:
    """``with options(sinkhorn_shortcut=0, gram_f32=1): ...`` -- set, run, restore (tests, bench, A/B tools)."""

    def __init__(self, **kv):
        self.kv = kv
        self.old = {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = get_option(k)
            set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            set_option(k, v)
        return False


def require_gpu(t):
    if not t.is_cuda:
        raise KccotError("kccotgan_amd needs tensors on a ROCm device (got %s); there is no CPU path" % t.device)


def ptr(t, dtypes=(torch.float32, torch.int32)):
    """Device address of a tensor (None -> NULL).  Refuses anything the kernels cannot read: the ABI's `float*` / `int*`
    parameters take fp32 / int32 tensors only -- a float64 tensor here would be reinterpreted, not converted."""
    if t is None:
        return None
    if not t.is_cuda:
        raise KccotError("kccotgan_amd needs tensors on a ROCm device (got %s); there is no CPU path" % t.device)
    if t.dtype not in dtypes:
        raise TypeError("kccotgan_amd kernel argument must be %s (got %s)" % (" / ".join(str(d) for d in dtypes), t.dtype))
    if not t.is_contiguous():
        raise ValueError("kccotgan_amd kernels need contiguous tensors")
    return t.data_ptr()


def ptr_f64(t):
    """Device address of a float64 tensor: ONLY for the `double*` parameters of the ABI (fp64 Gram sums and row norms of
    the sharded path: kccot_row_norms_f64, kccot_pairwise_cost3_rows_gram*_f64/_from_sums_f32)."""
    return ptr(t, (torch.float64,))


def stream_of(t):
    return torch.cuda.current_stream(t.device).cuda_stream


_ws_cache = {}


def workspace(nbytes, ref, stream=None):
    """A per-(device, stream) scratch buffer, grown on demand.  Calls issued on one stream are
    ordered, so successive kernels may reuse it.  ``stream``: stream_of(ref), if the caller has it."""
    if nbytes <= 0:
        return None, 0
    key = (ref.device, stream_of(ref) if stream is None else stream)
    buf = _ws_cache.get(key)
    if _CANARY:
        # a buffer of exactly the requested size (float32 view so that the guard sentinel is exact), so that the guard
        # zone starts at nbytes: a cached larger buffer would hide an overrun into its slack.  The previous one stays
        # referenced by _guards until it is verified.  nbytes is a multiple of 4 for every workspace query.
        if buf is None or buf.numel() * 4 != (int(nbytes) + 3) // 4 * 4:
            buf = empty(((int(nbytes) + 3) // 4,), torch.float32, ref.device)
            _ws_cache[key] = buf
        return buf.data_ptr(), int(nbytes)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes), dtype=torch.uint8, device=ref.device)
        _ws_cache[key] = buf
    return buf.data_ptr(), buf.numel()
