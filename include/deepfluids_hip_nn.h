/*
 * deepfluids_hip_nn.h -- C-ABI of libdeepfluids_hip_nn.so (gfx950 / MI355X only): the latent-space integrator (arch='nn').
 *
 * The network of the reference's `NN` (model.py:218-224) is linear -> BN -> ELU -> dropout, twice, then linear.  Its three linear
 * layers run on df_linear_fwd / df_linear_bwd of the main library; this library holds what those cannot do: the block between the
 * linear layers (forward in training and inference mode, backward), the step that feeds a window's prediction back in and its adjoint,
 * the fixed-order MSE of the windowed loss, and the whole rollout of `test_nn` (trainer.py:698-747) as ONE launch.
 *
 * A library and a header of their own: deepfluids_hip.h is frozen at DF_VERSION 207.  The library links against libdeepfluids_hip.so
 * and follows every convention of deepfluids_hip.h: device pointers, caller-owned dense fp32 buffers, asynchronous on `stream`,
 * 0 / DF_E* / hipError_t, and the message of a failure is read with df_last_error() of the main library.
 *
 * All arithmetic is fp32 in the order written, no fused multiply-add, no atomics; every sum has the order given here ("fp32 per thread,
 * fp64 across threads, a fixed combine", as deepfluids_hip_metrics.h), so two calls on the same input give the same bits.
 *
 * ---- the dropout mask (this project's own: the reference draws from TensorFlow's generator) ------------------------------------------
 *   mix(h):  h ^= h >> 16;  h *= 0x7FEB352D;  h ^= h >> 15;  h *= 0x846CA68B;  h ^= h >> 16     (uint32; the lattice-noise mix of
 *            deepfluids_hip.h)
 *   k = mix(seed ^ (step * 0x8DA6B343) ^ (window * 0xD8163841) ^ (layer * 0xCB1AB31F))
 *   h = mix(k ^ (row * 0x8DA6B343) ^ (col * 0xD8163841));   u = float(h >> 8) * 2^-24 in [0, 1);   element (row, col) is KEPT iff
 *   u < keep_prob.  A kept element is multiplied by inv = 1.0f / keep_prob (rounded once, on the host).  The mask is never stored: the
 *   backward pass recomputes it.  It depends on the element's own row and column only, not on B or N.
 *
 * ---- elu (alpha 1) ---------------------------------------------------------------------------------------------------------------------
 *   elu(y) = y for y > 0;  -1 for y < -17.5;  otherwise exp(y) - 1 in these fp32 steps, so that a restatement repeats it bit for bit:
 *   n = rint(y * 1.44269502f) (ties to even);  r = (y - n * 0.693359375f) - n * -2.12194440e-4f;
 *   q = 2.48015873e-5f;  then q = q * r + c for c = 1.98412698e-4f, 1.38888889e-3f, 8.33333333e-3f, 4.16666667e-2f, 1.66666667e-1f, 0.5f;
 *   p = r + (r * r) * q;  s = 2^n;  elu = s * p + (s - 1).   (|r| <= 0.347: the series is cut below 2e-8 of p; about 2 ulp in all.)
 *
 * ---- df_nn_bn_elu_dropout_fwd: training mode ------------------------------------------------------------------------------------------
 * x [B,N] pre-activation; gamma, beta, moving_mean, moving_var, mean, rstd [N]; act, out [B,N].  Per column c:
 *   column sums: a workgroup owns 32 consecutive columns and has 32 row threads per column; row thread q adds rows q, q + 32, q + 64 ...
 *   in ascending order to an fp32 accumulator that starts at 0; the 32 accumulators become fp64 and are added in ascending q from 0.0
 *   (called S(.) below).  Columns do not interact, so a column's numbers do not depend on N or on its neighbours.
 *   mean = float(S(x) / double(B));   var = float(S(d*d) / double(B)) with d = x - mean (biased);
 *   rstd = float(1.0 / sqrt(double(var) + double(eps)))                                         (fp64 divide and square root)
 *   per element: xh = (x - mean) * rstd;  y = xh * gamma + beta;  e = elu(y);  act = e;  out = kept ? e * inv : 0
 *   moving_mean = moving_mean * decay + mean * (1.0f - decay)
 *   moving_var  = moving_var * decay + (var * (float(B) / float(max(B - 1, 1)))) * (1.0f - decay)          (updated in place)
 * act (the ELU output before the mask), mean and rstd are what the backward pass reads.
 *
 * ---- df_nn_bn_elu_dropout_bwd ------------------------------------------------------------------------------------------------------------
 * gout [B,N] the gradient of `out`; x, act, gamma, mean, rstd as above; gx [B,N], ggamma, gbeta [N] are written (not accumulated).
 *   per element: gd = kept ? gout * inv : 0;  dy = act < 0 ? gd * (act + 1) : gd  (an exact zero takes gd);  xh = (x - mean) * rstd
 *   gbeta = float(S(dy));  ggamma = float(S(dy * xh));  ib = 1.0f / float(B) (host)
 *   gx = (gamma * rstd) * ((dy - gbeta * ib) - xh * (ggamma * ib))
 *
 * ---- df_nn_bn_elu_infer: inference mode (moving statistics, no mask) ----------------------------------------------------------------------
 *   rstd = float(1.0 / sqrt(double(moving_var) + double(eps)));  xh = (x - moving_mean) * rstd;  y = xh * gamma + beta;
 *   out = elu(y).  Elementwise; out may be x.
 *
 * ---- df_nn_window_advance_fwd / _bwd (build_model_nn, trainer.py:608-614) -----------------------------------------------------------------
 * x, x_next [B,Z+P]; y [B,Z]; xw [B,W,Z+P]; 0 <= i < W - 1.
 *   x_next[b,j] = x[b,j] + y[b,j] * ratio  (j < Z);   x_next[b,Z+j] = xw[b,i+1,Z+j]  (j < P)
 *   adjoint: gx[b,j] = gx_next[b,j] (j < Z), gx[b,Z+j] = 0;  gy[b,j] = gx_next[b,j] * ratio.   gx or gy may be NULL.
 *
 * ---- df_nn_rows_copy ----------------------------------------------------------------------------------------------------------------------
 * dst[b * dst_stride + j] = src[b * src_stride + j], b < B, j < Z <= both strides (in floats): puts a window's prediction [B,Z] into
 * its place of yw_ [B,W,Z] and takes its gradient out again.
 *
 * ---- df_nn_mse_fwd / _bwd: mean((a - b)^2) over n elements ------------------------------------------------------------------------------
 *   workgroup w owns elements 1024 w .. 1024 w + 1023; its thread t (0..255) adds d*d (d = a - b) of elements 1024 w + 256 i + t,
 *   i = 0..3 ascending, to an fp32 accumulator from 0; the 256 accumulators become fp64 and are added as a tree inside each 64-thread wave
 *   (off = 32, 16, 8, 4, 2, 1: lane l < off takes v[l] + v[l + off]), then the four wave sums in ascending order.  A second launch of one
 *   workgroup: thread t adds the workgroup sums t, t + 256, ... ascending in fp64, the same tree, out = float(total / double(n)).
 *   backward: ga = (gout[0] * (2.0f / float(n))) * (a - b).
 *   ws: df_nn_mse_workspace_bytes(n) bytes, 8-byte aligned; -1 for n <= 0.
 *
 * ---- df_nn_rollout: all scenes, all frames, one launch ------------------------------------------------------------------------------------
 * x_test [S*(F-1), Z+P], y_test [S*(F-1), Z] (normalised, data_nn.py), z_out [S,F,Z].  Layers: w1 [Z+P,N1] b1 [N1], bn1 = gamma1, beta1,
 * mm1, mv1 [N1]; w2 [N1,N2] b2, bn2 [N2]; w3 [N2,Z] b3 [Z].  One workgroup of 1024 threads per scene s; the activations stay in LDS.
 *   xin = x_test[s (F-1)];  z_out[s,0,j] = xin[j] * code_std
 *   for t = 0 .. F-2, r = s (F-1) + t:
 *     h1 = elu(bn1(xin . w1 + b1));  h2 = elu(bn2(h1 . w2 + b2));  y = h2 . w3 + b3         (bn / elu as df_nn_bn_elu_infer)
 *     pred[j] = y[j] * out_std + xin[j] * code_std;   for j >= Z - P:  pred[j] = y_test[r,j] * out_std + x_test[r,j] * code_std
 *     z_out[s,t+1,j] = pred[j];   xin[j] = pred[j] / code_std (j < Z);   xin[Z+j] = x_test[r+1,Z+j] (j < P, when t < F-2)
 *   matrix-vector product v . w [K,N] + b: the columns are taken in chunks of 1024; in a chunk of nb columns k is split into
 *   Sk = 1024 / nb (integer) interleaved parts, part q adds v[k] * w[k,n] for k = q, q + Sk, ... ascending to an fp32 accumulator from 0;
 *   the Sk accumulators become fp64 and are added in ascending q from 0.0; the result is float(total) + b[n].
 *   LDS: 4 (Z + P + 2 N1 + 2 N2 + Z + 1024) bytes, at most 64 KiB (DF_ESHAPE beyond).
 *
 * Errors, on the host and before any launch: DF_EINVAL (a null pointer that is not optional; a non-positive extent; i outside
 * 0 .. W-2; keep_prob outside (0, 1]; decay outside [0, 1]; eps or code_std not positive), DF_ESHAPE (B N, B W (Z+P) or S F (Z+P)
 * >= 2^31; P > Z; F < 2; a stride below Z; the rollout's LDS need), DF_EALIGN (fp32 buffers: 4 bytes; ws: 8 bytes), DF_EWORKSPACE.
 */
#ifndef DEEPFLUIDS_HIP_NN_H
#define DEEPFLUIDS_HIP_NN_H

#include "deepfluids_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int df_nn_bn_elu_dropout_fwd(const float* x, const float* gamma, const float* beta, float* moving_mean, float* moving_var, float* act,
                             float* out, float* mean, float* rstd, int64_t B, int64_t N, float eps, float decay, float keep_prob,
                             uint32_t seed, uint32_t step, uint32_t window, uint32_t layer, df_stream_t stream);
int df_nn_bn_elu_dropout_bwd(const float* x, const float* act, const float* gout, const float* gamma, const float* mean,
                             const float* rstd, float* gx, float* ggamma, float* gbeta, int64_t B, int64_t N, float keep_prob,
                             uint32_t seed, uint32_t step, uint32_t window, uint32_t layer, df_stream_t stream);
int df_nn_bn_elu_infer(const float* x, const float* gamma, const float* beta, const float* moving_mean, const float* moving_var,
                       float* out, int64_t B, int64_t N, float eps, df_stream_t stream);

int df_nn_window_advance_fwd(const float* x, const float* y, const float* xw, float* x_next, int64_t B, int64_t W, int64_t Z, int64_t P,
                             int64_t i, float ratio, df_stream_t stream);
int df_nn_window_advance_bwd(const float* gx_next, float* gx, float* gy, int64_t B, int64_t Z, int64_t P, float ratio,
                             df_stream_t stream);
int df_nn_rows_copy(const float* src, int64_t src_stride, float* dst, int64_t dst_stride, int64_t B, int64_t Z, df_stream_t stream);

int64_t df_nn_mse_workspace_bytes(int64_t n);
int df_nn_mse_fwd(const float* a, const float* b, int64_t n, float* out, void* ws, int64_t ws_bytes, df_stream_t stream);
int df_nn_mse_bwd(const float* a, const float* b, const float* gout, float* ga, int64_t n, df_stream_t stream);

int df_nn_rollout(const float* x_test, const float* y_test, const float* w1, const float* b1, const float* gamma1, const float* beta1,
                  const float* mm1, const float* mv1, const float* w2, const float* b2, const float* gamma2, const float* beta2,
                  const float* mm2, const float* mv2, const float* w3, const float* b3, float* z_out, int64_t S, int64_t F, int64_t Z,
                  int64_t P, int64_t N1, int64_t N2, float eps, float code_std, float out_std, df_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DEEPFLUIDS_HIP_NN_H */
