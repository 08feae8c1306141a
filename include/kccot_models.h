/* kccot_models.h -- C ABI of the model-side HIP kernels of libkccot.so that are not part of the loss library's
 * versioned surface (include/kccot.h, KCCOT_VERSION): kernels behind layers of the PyTorch models in kccotgan_amd/gan.py.
 * Strict C99.  Error codes, kccot_last_error() and kccot_stream_t are those of kccot.h; every call is asynchronous on
 * `stream`, allocates nothing, never synchronises the host and can be captured in a hipGraph.  All tensors are dense
 * float32 in device memory, 4-byte alignment is enough.
 */
#ifndef KCCOT_MODELS_H
#define KCCOT_MODELS_H

#include "kccot.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * The last layer of both discriminators, tf.keras.layers.LSTM(units, activation='sigmoid',
 * return_sequences=True) (the reference's gan.py:418), the whole recurrence in ONE launch each way.
 *   gx [B,T,4U]: the input projection of every step, bias included (gate order i, f, c, o as in Keras)
 *   wh [4U,U]:   the recurrent weights in nn.Linear layout (row = gate output, column = unit of h)
 * With h_{-1} = c_{-1} = 0, for t = 0..T-1:
 *   g = gx[b,t] + wh h_{t-1};   c_t = s(g_f) c_{t-1} + s(g_i) s(g_c);   h_t = s(g_o) s(c_t);   s = logistic sigmoid
 * Forward writes h_seq [B,T,U] and, unless c_seq is NULL (inference), c_seq [B,T,U].
 * Backward (full back-propagation through time) takes the forward's h_seq and c_seq and the upstream gradient
 * dh_seq [B,T,U] and writes dgx [B,T,4U], the gradient of gx; the gates are recomputed from gx and h_seq.  The gradient
 * of wh is the matrix product dgx[:,1:]^T h_seq[:,:-1], left to the caller.
 * Sample b's results depend on sample b's inputs and wh only: the same bits for every B and every position in the
 * batch.  No atomics.  1 <= U <= 64 (larger: KCCOT_EUNSUPPORTED); any B >= 1, T >= 1.
 * KCCOT_EINVAL: a NULL pointer other than the forward's c_seq, or B, T or U < 1 -- before any launch. */
int kccot_sigmoid_lstm_fwd_f32(const float* gx, const float* wh, int B, int T, int U, float* h_seq, float* c_seq,
                               kccot_stream_t stream);
int kccot_sigmoid_lstm_bwd_f32(const float* gx, const float* wh, const float* h_seq, const float* c_seq,
                               const float* dh_seq, int B, int T, int U, float* dgx, kccot_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KCCOT_MODELS_H */
