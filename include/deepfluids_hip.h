/*
 * deepfluids_hip.h -- C-ABI of libdeepfluids_hip.so (gfx950 / MI355X only).
 *
 * The drop-in boundary of the Deep Fluids velocity-field train step.  The reference
 * (byungsook/deep-fluids, TF 1.15) has no FFI of its own: its boundary is the Python call
 * surface of ops.py / model.py.  deep_fluids_amd/ops.py + model.py reproduce that surface and
 * call THIS library through ctypes; each entry point below cites the reference lines whose
 * arithmetic it replaces (paths relative to the upstream repo root).
 *
 * Conventions:
 *   - every pointer is a DEVICE pointer to fp32, channels-last, C-contiguous data unless noted;
 *     2-D tensors are [B,Y,X,C], 3-D tensors [B,Z,Y,X,C] ("x: bzyxd", ops.py:228);
 *   - the caller owns and frees every buffer including workspaces (sizes via *_workspace_bytes);
 *     the library keeps no tensor state and allocates nothing;
 *   - all work is enqueued asynchronously on `stream` (a hipStream_t passed as void*), nothing
 *     synchronises internally, so calls compose with PyTorch's current stream and hipGraph capture;
 *   - return 0 on success, <0 = DF_E* argument error, >0 = hipError_t; never throws, never
 *     aborts; a message for the calling thread's last failure is kept in df_last_error();
 *   - re-entrant; no global state besides read-only kernel handles: algorithm choices are call arguments
 *     (`algo`, DF_CONV_VALU_ONLY), never process-wide switches.  The library exports exactly what this header declares.
 */
#ifndef DEEPFLUIDS_HIP_H
#define DEEPFLUIDS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DF_VERSION 207 /* 0.2.7: + df_wino2d43_conv_bits, df_wino2d43_signbits_bytes, df_wino2d43_conv_addup_bits, df_lrelu_words2d_bwd_pool2x; 0.2.6: + df_wino43_*, df_wino2d43_*, df_conv_s2_dgrad_form; 0.2.5: + df_adam_tf1_step_dev, df_gd_step(_dev), df_store_scalars (hipGraph replay of the train step); 0.2.4: + df_conv_s2_dgrad; 0.2.3: + df_conv_s2_wgrad; 0.2.2: + df_conv_wgrad_form, df_upconv_wgrad_form; 0.2.1: + df_lrelu_bwd_pool2x, df_wino_conv_fwd_addup_bits, df_lrelu_bits_bwd_pool2x (0.2.0: df_conv_wgrad_algo, df_upconv_wgrad_algo, DF_CONV_VALU_ONLY, df_velocity_loss2d/3d) */

enum {
  DF_OK = 0,
  DF_EINVAL = -1,    /* null pointer / non-positive extent */
  DF_ESHAPE = -2,    /* extent unsupported by this kernel (e.g. forward difference needs n >= 2) */
  DF_EALIGN = -3,    /* pointer not aligned as the function's comment requires (16 bytes where it names no figure) */
  DF_EWORKSPACE = -4 /* workspace too small */
};

/* flags for df_conv_fwd.  Every conv entry point that takes `flags` names the bits it accepts in its comment; any other bit
 * (DF_CONV_ADDUP outside the add-up forms, DF_CONV_VALU_ONLY where the entry point has no thin-layer kernels, an undefined bit) is
 * DF_EINVAL, as is a flag whose operand is NULL. */
enum {
  DF_CONV_LRELU = 1,      /* y = max(v, leak*v)            ops.py:9-10 fused into the conv epilogue   */
  DF_CONV_RESIDUAL = 2,   /* y += residual (after act)      model.py:35,40,77,82                       */
  DF_CONV_MASK = 4,       /* y *= (mask_src > 0 ? 1 : leak) lrelu backward fused into the dgrad epilogue */
  DF_CONV_BIAS = 8,       /* v += bias[cout]                slim.conv* biases                          */
  DF_CONV_ADDUP = 16,     /* second output y2 = y + nearest_up2x(xc)  (df_wino_conv_fwd_addup only)     */
  DF_CONV_VALU_ONLY = 32  /* thin layers (Cin or Cout <= 4): take the general-shape vector-ALU kernel even where the
                             matrix-core form exists (the parity tests compare the two)                    */
};

typedef void* df_stream_t; /* hipStream_t */

int df_version(void);
const char* df_last_error(void);

/* ---- forward-difference stencils (HBM-bound) ----------------------------------------------
 * Alignment.  Every pointer is a float pointer and must be 4-byte aligned.  Where a function needs more, its comment names the
 * pointer and the alignment, and the function returns DF_EALIGN when the pointer has less (NULL counts as aligned).  The rule: an
 * OUTPUT that a kernel writes through a vector type must be aligned to that type; an INPUT that a fast kernel reads through a vector
 * type may have any 4-byte alignment -- the function then takes a kernel that reads it by 4-byte loads, with the same results bit
 * for bit.  Buffers are dense (no strides) and exactly as long as their shape says; nothing outside them is read or written. */

/* curl(x) ops.py:264-274.  psi [B,Y,X,1] -> u [B,Y,X,2] = (D_y psi, -D_x psi).
 * Alignment: psi 4 bytes; u 8 bytes (DF_EALIGN). */
int df_curl2d_fwd(const float* psi, float* u, int64_t B, int64_t Y, int64_t X, df_stream_t stream);
/* adjoint of df_curl2d_fwd: gu [B,Y,X,2] -> gpsi [B,Y,X,1].
 * Alignment: gu 4 bytes; gpsi 4 bytes. */
int df_curl2d_bwd(const float* gu, float* gpsi, int64_t B, int64_t Y, int64_t X, df_stream_t stream);

/* jacobian(x) ops.py:205-225.  x [B,Y,X,2] -> j [B,Y,X,4] = (dudx,dudy,dvdx,dvdy), w [B,Y,X,1] = dvdx-dudy.
 * j or w may be NULL (that output is not produced).
 * Alignment: x 4 bytes (8-byte loads where it is 8-byte aligned, 4-byte loads otherwise); j 16 bytes (DF_EALIGN); w 4 bytes. */
int df_jacobian2d_fwd(const float* x, float* j, float* w, int64_t B, int64_t Y, int64_t X, df_stream_t stream);
/* adjoint: gj [..,4] and/or gw [..,1] (either may be NULL, not both) -> gx [..,2].
 * Alignment: gj 4 bytes; gw 4 bytes; gx 8 bytes (DF_EALIGN). */
int df_jacobian2d_bwd(const float* gj, const float* gw, float* gx, int64_t B, int64_t Y, int64_t X,
                      df_stream_t stream);

/* jacobian3(x) ops.py:227-262.  x [B,Z,Y,X,3] -> j [..,9] = (dudx,dudy,dudz,dvdx,dvdy,dvdz,dwdx,dwdy,dwdz),
 * c [..,3] = (dwdy-dvdz, dudz-dwdx, dvdx-dudy).  j or c may be NULL.
 * `curl3(x)` of the north star == df_jacobian3d_fwd(x, NULL, c, ...)  (trainer3.py:18).
 * Alignment: x 4 bytes (the 16-byte-load kernel needs X % 4 == 0 and x 16-byte aligned; otherwise the one-voxel-per-lane kernel
 * runs); j 16 bytes, c 16 bytes (DF_EALIGN). */
int df_jacobian3d_fwd(const float* x, float* j, float* c, int64_t B, int64_t Z, int64_t Y, int64_t X,
                      df_stream_t stream);
/* adjoint: gj [..,9] and/or gc [..,3] (either may be NULL, not both) -> gx [..,3].
 * Alignment: gj, gc, gx 4 bytes (the 16-byte kernels need X % 4 == 0 and all three 16-byte aligned; otherwise the one-voxel-per-lane
 * kernel runs, which reads and writes single floats). */
int df_jacobian3d_bwd(const float* gj, const float* gc, float* gx, int64_t B, int64_t Z, int64_t Y, int64_t X,
                      df_stream_t stream);

/* divergence ops.py:276-284: x [B,Y,X,2] -> [B,Y-1,X-1,1];  divergence3 ops.py:286-290: x [B,Z,Y,X,3] -> [B,Z-1,Y-1,X-1,1].
 * Alignment: x 4 bytes; d 4 bytes. */
int df_divergence2d(const float* x, float* d, int64_t B, int64_t Y, int64_t X, df_stream_t stream);
int df_divergence3d(const float* x, float* d, int64_t B, int64_t Z, int64_t Y, int64_t X, df_stream_t stream);

/* ---- fused tail of the velocity-field train step (trainer.py:140-146,170-172; trainer3.py:18-24,49-51) ----------------------
 * u = curl(psi) | jacobian3(psi)[1];  l1 = mean|u - x|;  jl1 = mean|J(u) - J(x)|  with J = jacobian(.)[0] | jacobian3(.)[0] and
 * the ground-truth Jacobian of trainer.py:29-32 recomputed on the fly: one kernel over psi and x (36 B/voxel in 3-D instead of the
 * 240 B/voxel of the five reference ops; the 9-channel Jacobians are never materialised).
 *   psi [B,Z,Y,X,3] | [B,Y,X,1], x [B,Z,Y,X,3] | [B,Y,X,2];  u (nullable) receives the velocity field, bit-identical to
 *   df_jacobian3d_fwd(psi, NULL, u) | df_curl2d_fwd;  l1 / jl1: device scalars.
 * Backward: gpsi = curl^T( g_l1/N1 sign(u - x) + J^T( g_jl1/NJ sign(J(u) - J(x)) ) ) from the saved u and x;  g_l1 / g_jl1 are
 * device scalars (NULL = 1).  One workspace serves both directions (df_velocity_loss*_workspace_bytes = the larger of the two needs;
 * a workspace of exactly that size is enough, no byte outside it is touched, and neither direction reads what an earlier call left).
 * Alignment: psi, x, u, gpsi, l1, jl1, g_l1, g_jl1 4 bytes -- in 3-D the tiled and the 16-byte kernels need psi, x and u (backward:
 * u and x) 16-byte aligned and X % 4 == 0, and any other input, u == NULL included, takes the one-voxel-per-lane kernels; gpsi as gx
 * of df_jacobian3d_bwd.  workspace: 8 bytes for *_fwd (fp64 partial sums), 16 bytes for *_bwd (DF_EALIGN); one shared workspace is
 * therefore 16-byte aligned.  workspace_bytes below the direction's own need: DF_EWORKSPACE. */
int64_t df_velocity_loss3d_workspace_bytes(int64_t B, int64_t Z, int64_t Y, int64_t X);
int df_velocity_loss3d_fwd(const float* psi, const float* x, float* u, float* l1, float* jl1, int64_t B, int64_t Z, int64_t Y,
                           int64_t X, void* workspace, int64_t workspace_bytes, df_stream_t stream);
int df_velocity_loss3d_bwd(const float* u, const float* x, const float* g_l1, const float* g_jl1, float* gpsi, int64_t B, int64_t Z,
                           int64_t Y, int64_t X, void* workspace, int64_t workspace_bytes, df_stream_t stream);
int64_t df_velocity_loss2d_workspace_bytes(int64_t B, int64_t Y, int64_t X);
int df_velocity_loss2d_fwd(const float* psi, const float* x, float* u, float* l1, float* jl1, int64_t B, int64_t Y, int64_t X,
                           void* workspace, int64_t workspace_bytes, df_stream_t stream);
int df_velocity_loss2d_bwd(const float* u, const float* x, const float* g_l1, const float* g_jl1, float* gpsi, int64_t B, int64_t Y,
                           int64_t X, void* workspace, int64_t workspace_bytes, df_stream_t stream);


/* ---- losses (trainer.py:170-172, trainer3.py:49-51) -------------------------------------- */

/* workspace for df_l1_mean_fwd (bytes). */
int64_t df_l1_mean_workspace_bytes(int64_t n);
/* out[0] = mean(|a-b|) over n elements; deterministic two-stage reduction (fp64 partials). */
int df_l1_mean_fwd(const float* a, const float* b, int64_t n, float* out, void* workspace, int64_t workspace_bytes,
                   df_stream_t stream);
/* ga[i] = sign(a[i]-b[i]) * scale * (gout ? gout[0] : 1) / n   (tf Abs grad: sign, 0 at 0). */
int df_l1_mean_bwd(const float* a, const float* b, const float* gout, float scale, float* ga, int64_t n,
                   df_stream_t stream);

/* ---- element-wise / small layers ---------------------------------------------------------- */

/* lrelu(x, leak) ops.py:9-10 and its backward (slope 1 where y > 0 else leak; y = saved OUTPUT). */
int df_lrelu_fwd(const float* x, float* y, float leak, int64_t n, df_stream_t stream);
int df_lrelu_bwd(const float* gy, const float* y, float* gx, float leak, int64_t n, df_stream_t stream);

/* y = a + b (residual add model.py:35,40,77,82), n elements. */
int df_add(const float* a, const float* b, float* y, int64_t n, df_stream_t stream);

/* nearest-neighbour 2x up-sampling of every spatial axis, channels-last (src = dst>>1):
 * upscale ops.py:75-77 (D=1), upscale3 ops.py:79-91.  x [B,D,H,W,C] -> y [B,2D|1,2H,2W,C]; C % 4 == 0. */
int df_upsample2x_fwd(const float* x, float* y, int64_t B, int64_t D, int64_t H, int64_t W, int64_t C, int is_3d,
                      df_stream_t stream);
/* The backward tail of an up-sampling generator block (`x = lrelu(conv4(.)) + upscale(xc)`, model.py:36-40 / 78-82) in ONE pass
 * over the incoming gradient: gx = gy * (y > 0 ? 1 : leak)  (== df_lrelu_bwd; y = conv4's saved output, fine resolution
 * [B,2D|1,2H,2W,C]) and gpool = 2x2(x2) sum-pool of gy  (== df_upsample2x_bwd, the skip gradient w.r.t. xc, [B,D,H,W,C]).
 * B, D, H, W are the COARSE extents; C % 4 == 0.  Bit-identical to the two separate calls. */
int df_lrelu_bwd_pool2x(const float* gy, const float* y, float* gx, float* gpool, float leak, int64_t B, int64_t D, int64_t H,
                        int64_t W, int64_t C, int is_3d, df_stream_t stream);
/* adjoint (2x2(x2) sum-pool): gy [B,2D|1,2H,2W,C] -> gx [B,D,H,W,C]. */
int df_upsample2x_bwd(const float* gy, float* gx, int64_t B, int64_t D, int64_t H, int64_t W, int64_t C, int is_3d,
                      df_stream_t stream);

/* ---- wrapper generality (conv_general.hip): the shapes of the reference's call surface that its trainers never use ------------------
 * ops.py:12-16 `conv2d / conv3d(x, o_dim, k=4, s=2, act)` = slim.conv2d / conv3d, padding 'SAME', ANY cubic kernel 1 <= k <= 7 and stride
 * 1 <= s <= 4, any extents (odd ones included): out = ceil(n / s), pad_total = max((out - 1) s + k - n, 0), pad_before = pad_total / 2.
 * 2-D: D = 1, kz = 1; 3-D: kz = k.  Weights in the TF layout [kz, k, k, Cin, Cout] (no packing).  Plain vector-ALU kernels, fixed summation
 * order: correct on every shape, not fast -- k = 3, s in {1, 2} on even extents take the matrix-core kernels above. */
int df_conv_general_out_dims(int64_t D, int64_t H, int64_t W, int kz, int k, int s, int64_t* Do, int64_t* Ho, int64_t* Wo);
/* y [B,Do,Ho,Wo,Cout] = conv(x [B,D,H,W,Cin], w) (+ bias) (+ lrelu);  flags: DF_CONV_BIAS | DF_CONV_LRELU. */
int df_conv_general_fwd(const float* x, const float* w, const float* bias, float* y, int64_t B, int64_t D, int64_t H, int64_t W, int64_t Cin,
                        int64_t Cout, int kz, int k, int s, int flags, float leak, df_stream_t stream);
/* gx [B,D,H,W,Cin] from gy [B,Do,Ho,Wo,Cout] (B, D, H, W = the INPUT extents of the forward conv). */
int df_conv_general_dgrad(const float* gy, const float* w, float* gx, int64_t B, int64_t D, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int kz,
                          int k, int s, df_stream_t stream);
/* gw [kz,k,k,Cin,Cout] and gb [Cout] (gb may be NULL).  Expected cost: one workgroup per (tap, input channel) walks ALL output voxels in four
 * sub-ranges (gb: 16 sub-ranges per 64 channels) -- a correctness path, SECONDS per call on 10^7-voxel grids; training at such sizes with a
 * kernel / stride the matrix-core kernels do not take needs a dedicated kernel first. */
int df_conv_general_wgrad(const float* x, const float* gy, float* gw, float* gb, int64_t B, int64_t D, int64_t H, int64_t W, int64_t Cin,
                          int64_t Cout, int kz, int k, int s, df_stream_t stream);
/* ops.py:66-73 `resize_nearest_neighbor(x, new_size)` = tf.image.resize_nearest_neighbor, align_corners=False, ANY target size:
 * y[.., o, ..] = x[.., min(floor(o * in / out), in - 1), ..] per spatial axis (D = Do = 1 for 2-D); bwd = its adjoint in gather form. */
int df_resize_nn_fwd(const float* x, float* y, int64_t B, int64_t D, int64_t H, int64_t W, int64_t C, int64_t Do, int64_t Ho, int64_t Wo,
                     df_stream_t stream);
int df_resize_nn_bwd(const float* gy, float* gx, int64_t B, int64_t D, int64_t H, int64_t W, int64_t C, int64_t Do, int64_t Ho, int64_t Wo,
                     df_stream_t stream);

/* linear ops.py:23-24 (slim.fully_connected): y[B,N] = x[B,K] . w[K,N] + bias[N]  (bias may be NULL). */
int64_t df_linear_workspace_bytes(int64_t B, int64_t K, int64_t N); /* > 0 only for the large-K/small-N split-K path */
int df_linear_fwd(const float* x, const float* w, const float* bias, float* y, int64_t B, int64_t K, int64_t N,
                  void* workspace, int64_t workspace_bytes, df_stream_t stream);
/* backward: gw[K,N] = x^T gy, gb[N] = sum_b gy, gx[B,K] = gy w^T (gx / gw / gb may be NULL). */
int df_linear_bwd(const float* x, const float* w, const float* gy, float* gx, float* gw, float* gb, int64_t B,
                  int64_t K, int64_t N, df_stream_t stream);

/* tf.concat([a, b], axis=-1) of two channels-last tensors with `rows` voxels (encoder skips, model.py:138,174) and the
 * reverse split of the gradient (16-byte vectorised when both channel counts are multiples of 4). */
int df_concat2_fwd(const float* a, const float* b, float* y, int64_t rows, int64_t Ca, int64_t Cb, df_stream_t stream);
int df_concat2_bwd(const float* gy, float* ga, float* gb, int64_t rows, int64_t Ca, int64_t Cb, df_stream_t stream);

/* zero insertion used by the stride-2 conv backward: out[B,2D|1,2H,2W,C][2o+1] = g[B,D,H,W,C][o], zeros elsewhere. */
int df_dilate2_odd(const float* g, float* out, int64_t B, int64_t D, int64_t H, int64_t W, int64_t C, int is_3d,
                   df_stream_t stream);

/* tf.sigmoid (AE latent code with use_sparse, model.py:196,210) and its backward from the saved output. */
/* Bernoulli-KL sparsity of the auto-encoder code (trainer3.py:272-277): out = sum_{j<n} KL(Bern(rho) || Bern(mean_b z[b][j]));
 * z is [B, ncol] (sigmoid outputs), the first n columns take part.  bwd: gz[B, ncol] = gout * scale * dloss/dz (0 for j >= n). */
int df_kl_bernoulli_fwd(const float* z, int64_t B, int64_t ncol, int64_t n, float rho, float* out, df_stream_t stream);
int df_kl_bernoulli_bwd(const float* z, const float* gout, float scale, float* gz, int64_t B, int64_t ncol, int64_t n, float rho,
                        df_stream_t stream);
int df_sigmoid_fwd(const float* x, float* y, int64_t n, df_stream_t stream);
int df_sigmoid_bwd(const float* gy, const float* y, float* gx, int64_t n, df_stream_t stream);

/* mean((a-b)^2) (loss_p, trainer.py:395 / trainer3.py:268-270); workspace as df_l1_mean_fwd. */
int df_mse_mean_fwd(const float* a, const float* b, int64_t n, float* out, void* workspace, int64_t workspace_bytes,
                    df_stream_t stream);
int df_mse_mean_bwd(const float* a, const float* b, const float* gout, float scale, float* ga, int64_t n,
                    df_stream_t stream);

/* gb[c] = sum over rows of g[rows, C]  (conv bias gradient), deterministic. */
int64_t df_colsum_workspace_bytes(int64_t rows, int64_t C);
int df_colsum(const float* g, float* gb, int64_t rows, int64_t C, void* workspace, int64_t workspace_bytes,
              df_stream_t stream);

/* tf.train.AdamOptimizer update (trainer.py:160-162,184; "epsilon-hat" form), applied to one
 * flat parameter slab:  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  p -= lr_t m / (sqrt(v) + eps),
 * with lr_t = lr sqrt(1-b2^t)/(1-b1^t) computed by the caller on the host. */
int df_adam_tf1_step(float* p, const float* g, float* m, float* v, int64_t n, float lr_t, float beta1, float beta2,
                     float eps, float grad_scale, df_stream_t stream);

/* The same update with the two per-step scalars read from DEVICE memory -- scalars[0] = lr_t, scalars[1] = grad_scale -- so that a
 * captured hipGraph of the whole train step (one `sess.run(g_optim)`, trainer.py:265-269) replays with the values the host stored
 * before the launch; arithmetic identical to df_adam_tf1_step (bitwise-equal parameters). */
int df_adam_tf1_step_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* scalars, float beta1, float beta2,
                         float eps, df_stream_t stream);

/* tf.train.GradientDescentOptimizer (the `gd` option, trainer.py:163-165):  p -= (lr * grad_scale) * g  over one flat slab;
 * _dev: scalars[0] = lr, scalars[1] = grad_scale from device memory (graph replay, as above). */
int df_gd_step(float* p, const float* g, int64_t n, float lr, float grad_scale, df_stream_t stream);
int df_gd_step_dev(float* p, const float* g, int64_t n, const float* scalars, df_stream_t stream);

/* dst[0..n-1] = v0..v(n-1), n <= 4, by a one-thread kernel whose arguments travel by value: the host-side update of the device
 * scalars above, ordered on `stream` before the graph launch, with no host buffer that a later step could overwrite early. */
int df_store_scalars(float* dst, int64_t n, float v0, float v1, float v2, float v3, df_stream_t stream);

/* ---- convolutions on MFMA (exact fp32: v_mfma_f32_32x32x2_f32) ----------------------------- */

/* slim.conv2d / conv3d, k=3, stride 1, padding SAME, channels-last (ops.py:12-16; model.py:26,42,68,84).
 * Weights are given in TF layout [kz,ky,kx,Cin,Cout] (2-D: kz = 1) and are re-packed once per update into
 * the MFMA operand order by df_conv_pack_weights:
 *   mode 0: forward operand;  mode 1: dgrad operand (taps mirrored, Cin/Cout swapped).
 * Packed size, in floats: taps * Kpad * Npad with K = cin, N = cout (mode 0) or K = cout, N = cin (modes 1, 2); Kpad = K rounded up to
 * 16 (the *_bf16x3 packs: 32), Npad = N rounded up to its N tile (32 up to N = 32, 64 up to 64, 128 above).  The up-sampling packs
 * (df_upconv_packed_elems) hold 4 classes x 4 taps (2-D) or 8 x 8 (3-D) of that. */
int64_t df_conv_packed_elems(int64_t taps, int64_t cin, int64_t cout, int mode);
int df_conv_pack_weights(const float* w, float* wp, int64_t taps, int64_t cin, int64_t cout, int mode,
                         df_stream_t stream);
/* y[B,D,H,W,Cout] = epilogue( conv_same(x[B,D,H,W,Cin], w) ).  D = 1 and kz = 1 for 2-D.
 * `wp` packed with mode 0 (forward) or mode 1 (then x is dL/dy and y is dL/dx: the dgrad).
 * flags: DF_CONV_BIAS | LRELU | RESIDUAL | MASK | VALU_ONLY; bias / residual / mask_src are used only when their flag is set.
 * Alignment: wp 16 bytes (DF_EALIGN); x, y, bias, residual, mask_src 4 bytes (the kernels that read or write them through
 * 16-byte types run only where they are 16-byte aligned; the general kernels take their place otherwise). */
int df_conv_fwd(const float* x, const float* wp, const float* bias, const float* residual, const float* mask_src,
                float* y, int64_t B, int64_t D, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int kz, int flags,
                float leak, df_stream_t stream);
/* k=3, stride 2, TF 'SAME' on even input extents (pad 0 before / 1 after): the encoder's down-sampling convs
 * (model.py:141-143, 177-179).  x [B,2Do|1,2Ho,2Wo,Cin] -> y [B,Do,Ho,Wo,Cout]; `wp` packed with mode 0;
 * flags: DF_CONV_BIAS | DF_CONV_LRELU only. */
int df_conv_s2_fwd(const float* x, const float* wp, const float* bias, float* y, int64_t B, int64_t Do, int64_t Ho,
                   int64_t Wo, int64_t Cin, int64_t Cout, int kz, int flags, float leak, df_stream_t stream);
/* Weight (and bias) gradient of that stride-2 conv: gw[tz][ty][tx][ci][co] = sum_{b,o} x[b][2o + t][ci] gy[b][o][co] (TF autodiff of
 * slim.conv3d(stride=2); model.py:141-143, 177-179) computed natively on the OUTPUT grid -- no zero-inserted gradient tensor.
 * x [B,2Do|1,2Ho,2Wo,Cin], gy [B,Do,Ho,Wo,Cout]; gw TF layout [kz,3,3,Cin,Cout]; gb may be NULL.  Instantiated for Wo in {8,16,32,64},
 * even Cin, Cout >= 32 (df_conv_s2_wgrad_workspace_bytes returns 0 otherwise: use df_dilate2_odd + df_conv_wgrad). */
int64_t df_conv_s2_wgrad_workspace_bytes(int64_t B, int64_t Do, int64_t Ho, int64_t Wo, int64_t Cin, int64_t Cout, int kz);
int df_conv_s2_wgrad(const float* x, const float* gy, float* gw, float* gb, int64_t B, int64_t Do, int64_t Ho, int64_t Wo, int64_t Cin,
                     int64_t Cout, int kz, void* workspace, int64_t workspace_bytes, df_stream_t stream);
/* Input gradient of that stride-2 conv (TF autodiff of slim.conv2d/conv3d(stride=2): model.py:141-143, 177-179; the discriminator's
 * model.py:94-99): gx [B,2Do|1,2Ho,2Wo,Cin] from gy [B,Do,Ho,Wo,Cout].  `wp` = df_upconv_pack_weights(w, Cin, Cout, kz, mode 2).  Per axis
 * dx[2m] = g[m-1] w[2] + g[m] w[0], dx[2m+1] = g[m] w[1]: 8 (4) parity classes with 8,4,4,2,4,2,2,1 (4,2,2,1) LIVE taps; each class runs a
 * kernel specialised on its tap counts (27 tap-products per coarse voxel and channel pair; the generic 2x2x2-tap parity-class kernel --
 * df_upconv_fwd on the same operand, used here for channel counts without a specialisation -- multiplies 64, a stride-1 dgrad on the
 * zero-inserted gradient 216).  Every output voxel is written exactly once (no accumulation). */
int df_conv_s2_dgrad(const float* gy, const float* wp, float* gx, int64_t B, int64_t Do, int64_t Ho, int64_t Wo, int64_t Cin, int64_t Cout,
                     int kz, df_stream_t stream);
/* Which kernel df_conv_s2_dgrad takes for this gradient pointer (alignment) and channel counts (Cin / Cout of the FORWARD conv):
 * 1 = each parity class on its live taps only, 0 = the generic 2x2(x2)-tap parity-class kernel (zero-padded taps).  Host-only. */
int df_conv_s2_dgrad_form(const float* gy, int64_t Cin, int64_t Cout);
/* ---- up-sampling-aware first conv of a generator block --------------------------------------------------------------
 * model.py:36-37 / 78-79 feed `upscale(x, 2)` into the next block's first conv.  conv(nearest_up2x(xc), w) is computed
 * WITHOUT materialising the up-sampled tensor as 8 (3-D) / 4 (2-D) parity-class convs with 2x2x2 / 2x2 pre-summed taps
 * on the coarse grid (27/8 = 3.4x fewer FLOPs; identical up to fp32 summation order).
 *   xc [B,Dc|1,Hc,Wc,Cin] (coarse)  ->  y [B,2Dc|1,2Hc,2Wc,Cout] (fine).  Weights: TF layout [kz,3,3,Cin,Cout].
 *   df_upconv_fwd flags: DF_CONV_BIAS | DF_CONV_LRELU only; channel counts > 4 (DF_ESHAPE), also for df_upconv_dgrad.
 * Pack modes: 0 forward operand; 1 operand of df_upconv_dgrad; 2 DGRAD OPERAND OF THE STRIDE-2 CONV (df_conv_s2_fwd): the adjoint of
 *   y[o] = sum_t x[2o+t] w[t] is dx[2m] = g[m-1] w[2] + g[m] w[0], dx[2m+1] = g[m] w[1] per axis, i.e. the same parity-class / offset
 *   structure; run it as  df_upconv_fwd(g [B,Do,Ho,Wo,Cout], wp(mode 2), NULL, dx [B,2Do,2Ho,2Wo,Cin], B, Do, Ho, Wo, Cin := Cout,
 *   Cout := Cin, kz, 0, 0, stream)  -- 64 tap-products per coarse voxel instead of the 216 of a stride-1 dgrad on the
 *   zero-inserted gradient (model.py:141-143, 177-179: the encoder's / discriminator's down-sampling layers). */
int64_t df_upconv_packed_elems(int64_t cin, int64_t cout, int kz, int mode);
int df_upconv_pack_weights(const float* w, float* wp, int64_t cin, int64_t cout, int kz, int mode, df_stream_t stream);
int df_upconv_fwd(const float* xc, const float* wp, const float* bias, float* y, int64_t B, int64_t Dc, int64_t Hc,
                  int64_t Wc, int64_t Cin, int64_t Cout, int kz, int flags, float leak, df_stream_t stream);
/* acc[B,Dc,Hc,Wc,Cin] += d(loss)/d(xc) given g = d(loss)/d(y) on the fine grid; `wp` packed with mode 1. */
int df_upconv_dgrad(const float* g, const float* wp, float* acc, int64_t B, int64_t Dc, int64_t Hc, int64_t Wc,
                    int64_t Cin, int64_t Cout, int kz, df_stream_t stream);
/* gw[kz,3,3,Cin,Cout] (the ORIGINAL 3-wide filter) and gb from the coarse input and the fine gradient. */
int64_t df_upconv_wgrad_workspace_bytes(int64_t B, int64_t Dc, int64_t Hc, int64_t Wc, int64_t Cin, int64_t Cout, int kz);
int df_upconv_wgrad(const float* xc, const float* gy, float* gw, float* gb, int64_t B, int64_t Dc, int64_t Hc, int64_t Wc,
                    int64_t Cin, int64_t Cout, int kz, void* workspace, int64_t workspace_bytes, df_stream_t stream);
/* algo: 0 best available | 1 generic direct kernel on the parity classes | 2, 3 three-product parity-class kernel |
 * 4 the 27-point Winograd-(x,y,z) form wherever instantiated (df_upconv_wgrad == algo 0). */
int df_upconv_wgrad_algo(const float* xc, const float* gy, float* gw, float* gb, int64_t B, int64_t Dc, int64_t Hc, int64_t Wc,
                         int64_t Cin, int64_t Cout, int kz, void* workspace, int64_t workspace_bytes, int algo,
                         df_stream_t stream);
/* y[fine] = a[fine] + nearest_up2x(bc[coarse])  (block-end residual `x += x0` with x0 = upscale(.), model.py:35-40). */
int df_add_up2x(const float* a, const float* bc, float* y, int64_t B, int64_t D, int64_t H, int64_t W, int64_t C, int is_3d,
                df_stream_t stream);

/* ---- Winograd F(2x2x2, 3x3x3) form of the 3-D stride-1 convolution (conv_wino.hip) ------------------------------------
 * Same result as df_conv_fwd with kz = 3 up to fp32 rounding order (all arithmetic fp32, 3.4x fewer matrix-core FLOPs);
 * same epilogue flags.  Needs Cin % 32 == 0, Cout % 32 == 0, D*H*W*max(Cin,Cout) <= 2^29 (one batch volume below 2 GiB), Cin*Cout <= 2^24 and at
 * most 256 cout slices of 32 channels (Cout <= 8192; df_wino_upconv_dgrad: Cin <= 8192, its kernel's output channels), else DF_ESHAPE.  Weights: TF layout [3,3,3,Cin,Cout], transformed and
 * packed once per update by df_wino_pack_weights (mode 0: forward operand, mode 1: dgrad operand). */
int64_t df_wino_packed_elems(int64_t cin, int64_t cout, int mode);
int df_wino_pack_weights(const float* w, float* wp, int64_t cin, int64_t cout, int mode, df_stream_t stream);
int df_wino_conv_fwd(const float* x, const float* wp, const float* bias, const float* residual, const float* mask_src,
                     float* y, int64_t B, int64_t D, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int flags, float leak,
                     df_stream_t stream);

/* Up-sampling-aware variant: y[B,2Dc,2Hc,2Wc,Cout] = lrelu(conv_same(nearest_up2x(xc), w) + bias) without materialising the up-sampled
 * tensor and with only 27 of the 64 Winograd products (the others are identically zero for a duplicated input).  `wp` is the mode-0
 * pack of df_wino_pack_weights; flags must be DF_CONV_BIAS | DF_CONV_LRELU. */
int df_wino_upconv_fwd(const float* xc, const float* wp, const float* bias, float* y, int64_t B, int64_t Dc, int64_t Hc,
                       int64_t Wc, int64_t Cin, int64_t Cout, int flags, float leak, df_stream_t stream);

/* Its adjoint w.r.t. xc: acc[B,Dc,Hc,Wc,Cin] += sum-pool2x(conv_same^T(g, w)) for g = d(loss)/d(y) on the fine grid
 * [B,2Dc,2Hc,2Wc,Cout]; the pooled inverse transform needs the same 27 points.  `wp` is the mode-1 pack of
 * df_wino_pack_weights(w, wp, Cin, Cout, 1).  Drop-in for df_upconv_dgrad (kz = 3, channels multiples of 32). */
int df_wino_upconv_dgrad(const float* g, const float* wp, float* acc, int64_t B, int64_t Dc, int64_t Hc, int64_t Wc, int64_t Cin,
                         int64_t Cout, df_stream_t stream);

/* Last conv of an up-sampling generator block with the block-end skip add fused in (model.py:35,40,77,82 `x += x0`, x0 = upscale(xc)):
 *   y = lrelu(conv_same(x, w) + bias)  (kept for the backward pass),   y2 = y + nearest_up2x(xc),  xc [B,D/2,H/2,W/2,Cout].
 * Same packed weights and shape limits as df_wino_conv_fwd; D, H, W even. */
int df_wino_conv_fwd_addup(const float* x, const float* wp, const float* bias, const float* xc, float* y, float* y2, int64_t B,
                           int64_t D, int64_t H, int64_t W, int64_t Cin, int64_t Cout, float leak, df_stream_t stream);

/* ---- round 6: F(2,3) x F(2,3) x F(4,3) Winograd family (conv_wino43.hip) -------------------------------------------------------------
 * The same convolution as df_wino_conv_fwd* (slim.conv3d k=3 s=1 SAME, model.py:66-70; dgrad = mode-1 operand) with a 2 x 2 x 4 output
 * tile: 6 matrix multiply-adds per output voxel and (cin, cout) pair instead of 8, about one bit of fp32 accuracy less.
 * Shape limits as df_wino_conv_fwd, with Cin*Cout <= 2^22; Cout <= 8192 (256 cout slices) as there.
 * ONE entry point covers every fused epilogue of the F(2,3)^3 family; the sign words it writes / reads have the SAME layout
 * (df_wino_signbits_bytes, df_lrelu_bits_bwd_pool2x), so the two families can be mixed layer by layer:
 *   flags        DF_CONV_BIAS | LRELU | RESIDUAL (fine tensor `residual`) | MASK | ADDUP (`residual` = the COARSE tensor, y2 = y + up2x)
 *   mask_src     fp32 activation whose sign is the lrelu mask of DF_CONV_MASK, or
 *   mask_bits    the same mask as sign words (exactly one of the two with DF_CONV_MASK)
 *   sign_bits    non-null: also emit the sign words of y;  y == NULL (only with ADDUP + sign_bits): y itself is not written. */
int64_t df_wino43_packed_elems(int64_t cin, int64_t cout, int mode);
int df_wino43_pack_weights(const float* w, float* wp, int64_t cin, int64_t cout, int mode, df_stream_t stream);
int df_wino43_conv(const float* x, const float* wp, const float* bias, const float* residual, const float* mask_src, const void* mask_bits,
                   float* y, float* y2, void* sign_bits, int64_t B, int64_t D, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int flags,
                   float leak, df_stream_t stream);

/* The 2-D twin (conv_wino2d43.hip): slim.conv2d k=3 s=1 SAME (ops.py:12-13; model.py:24-28) as Winograd F(2,3) x F(4,3) -- 3 matrix multiply-adds
 * per output pixel and (cin, cout) pair instead of the 4 of df_wino2d_conv_fwd; same arguments, flags (BIAS | LRELU | RESIDUAL | MASK with an
 * fp32 mask_src), shape limits (Cout <= 8192 among them) and error convention as df_wino2d_conv_fwd; mode 1 of the pack = the dgrad operand. */
int64_t df_wino2d43_packed_elems(int64_t cin, int64_t cout, int mode);
int df_wino2d43_pack_weights(const float* w, float* wp, int64_t cin, int64_t cout, int mode, df_stream_t stream);
int df_wino2d43_conv(const float* x, const float* wp, const float* bias, const float* residual, const float* mask_src, float* y, int64_t B,
                     int64_t H, int64_t W, int64_t Cin, int64_t Cout, int flags, float leak, df_stream_t stream);
/* ... with sign words (the 2-D twin of df_wino_conv_fwd_bits below; reference: the lrelu of slim.conv2d's activation_fn, ops.py:12-13, whose slope TF's
 * autodiff multiplies into the gradient -- model.py:24-28): flags == BIAS | LRELU + sign_bits: the forward conv also writes (activation > 0) as ONE
 * 32-bit word per (tile block of 16 x 32 pixels, 32-cout slice, thread) = its 32 outputs; flags == MASK + mask_bits: the dgrad of the SAME geometry
 * (B, H, W, channel count of the masked tensor) reads those words instead of the fp32 activation (1/32 of the bytes).  df_wino2d43_signbits_bytes
 * = the buffer size (16-byte aligned buffers).  Results bit-identical to the fp32-mask path. */
int64_t df_wino2d43_signbits_bytes(int64_t B, int64_t H, int64_t W, int64_t C);
int df_wino2d43_conv_bits(const float* x, const float* wp, const float* bias, const void* mask_bits, float* y, void* sign_bits, int64_t B, int64_t H,
                          int64_t W, int64_t Cin, int64_t Cout, int flags, float leak, df_stream_t stream);
/* The block tail of a 2-D up-sampling generator block on sign words (the twins of df_wino_conv_fwd_addup_bits / df_lrelu_bits_bwd_pool2x; reference:
 * model.py:36-40 -- x = conv(...); x += x0 with x0 = upscale(previous block)).  df_wino2d43_conv_addup_bits: y2 = lrelu(conv(x) + bias) + nearest_up2x(xc),
 * xc = the COARSE tensor [B, H/2, W/2, Cout]; the conv's own activation is NOT written, only its sign words (all the backward pass needs of it).
 * df_lrelu_words2d_bwd_pool2x: gx = gy * lrelu'(activation) from those words and gpool[B, Hc, Wc, C] = the 2 x 2 sum-pool of gy (the skip path's
 * gradient), one pass over gy [B, 2 Hc, 2 Wc, C].  Bit-identical to df_wino2d43_conv + df_add_up2x / df_lrelu_bwd_pool2x. */
int df_wino2d43_conv_addup_bits(const float* x, const float* wp, const float* bias, const float* xc, float* y2, void* sign_bits, int64_t B, int64_t H,
                                int64_t W, int64_t Cin, int64_t Cout, float leak, df_stream_t stream);
int df_lrelu_words2d_bwd_pool2x(const float* gy, const void* mask_bits, float* gx, float* gpool, float leak, int64_t B, int64_t Hc, int64_t Wc, int64_t C,
                                df_stream_t stream);

/* Sign-bit masks.  A masked dgrad (DF_CONV_MASK) multiplies its output by the lrelu slope of the layer below, i.e. it needs ONE BIT
 * per element of that layer's activation; read from the fp32 activation that is 3.2 GB per top-level launch at cfg3.  The forward
 * conv that produced the activation can emit the bits instead (one byte per lane: the signs of its 8 outputs, 1/32 of the bytes) and
 * the dgrad of the SAME geometry (B, D, H, W and channel count) reads those:
 *   df_wino_conv_fwd_bits(flags = DF_CONV_BIAS | DF_CONV_LRELU, bias, mask_bits = NULL, sign_bits = out)   forward, writes y and bits(y > 0)
 *   df_wino_upconv_fwd_bits(...)                                                                            the same for the 27-point form
 *   df_wino_conv_fwd_bits(flags = DF_CONV_MASK, bias = NULL, mask_bits = in, sign_bits = NULL)             masked dgrad (mode-1 weights)
 * The byte layout is private to the two kernels (tile block, cout slice, wave, cout block, lane); df_wino_signbits_bytes sizes it. */
int64_t df_wino_signbits_bytes(int64_t B, int64_t D, int64_t H, int64_t W, int64_t C);
int df_wino_conv_fwd_bits(const float* x, const float* wp, const float* bias, const void* mask_bits, float* y, void* sign_bits, int64_t B,
                          int64_t D, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int flags, float leak, df_stream_t stream);
int df_wino_upconv_fwd_bits(const float* xc, const float* wp, const float* bias, float* y, void* sign_bits, int64_t B, int64_t Dc,
                            int64_t Hc, int64_t Wc, int64_t Cin, int64_t Cout, float leak, df_stream_t stream);
/* The block tail on sign bits: df_wino_conv_fwd_addup without its first output -- y2 = lrelu(conv_same(x, w) + bias) + nearest_up2x(xc)
 * and the sign bits of the lrelu output (sized by df_wino_signbits_bytes(B, D, H, W, Cout)); the pre-add activation itself (3.2 GB per
 * top-level layer at cfg3) is never written.  df_lrelu_bits_bwd_pool2x is the matching backward tail (== df_lrelu_bwd_pool2x with the
 * mask read from those bits: gx = gy * (bit ? 1 : leak), gpool = 2x2x2 sum-pool of gy); B, Dc, Hc, Wc the COARSE extents
 * (gy / gx [B,2Dc,2Hc,2Wc,C], gpool [B,Dc,Hc,Wc,C]), C % 32 == 0. */
int df_wino_conv_fwd_addup_bits(const float* x, const float* wp, const float* bias, const float* xc, float* y2, void* sign_bits,
                                int64_t B, int64_t D, int64_t H, int64_t W, int64_t Cin, int64_t Cout, float leak, df_stream_t stream);
int df_lrelu_bits_bwd_pool2x(const float* gy, const void* mask_bits, float* gx, float* gpool, float leak, int64_t B, int64_t Dc, int64_t Hc,
                             int64_t Wc, int64_t C, df_stream_t stream);

/* 2-D twin: Winograd F(2x2, 3x3) form of the stride-1 3x3 convolution (conv_wino2d.hip): 2.25x fewer matrix-core FLOPs than df_conv_fwd
 * with kz = 1, fp32 throughout, same epilogue flags.  Needs Cin % 32 == 0, Cout % 32 == 0, H*W*max(Cin,Cout) <= 2^29, Cin*Cout <= 2^24 and at most
 * 256 cout slices of 32 channels (Cout <= 8192; df_wino2d_upconv_dgrad: Cin <= 8192, its kernel's output channels), else DF_ESHAPE. */

int64_t df_wino2d_packed_elems(int64_t cin, int64_t cout, int mode);
int df_wino2d_pack_weights(const float* w, float* wp, int64_t cin, int64_t cout, int mode, df_stream_t stream);
int df_wino2d_conv_fwd(const float* x, const float* wp, const float* bias, const float* residual, const float* mask_src,
                       float* y, int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int flags, float leak,
                       df_stream_t stream);
/* 2-D up-sampling-aware forms (9 of the 16 Winograd products): forward y[B,2Hc,2Wc,Cout] = lrelu(conv_same(nearest_up2x(xc), w) + bias)
 * (mode-0 pack of df_wino2d_pack_weights; flags = DF_CONV_BIAS | DF_CONV_LRELU) and its adjoint acc[B,Hc,Wc,Cin] += sum-pool2x(conv_same^T(g, w))
 * (mode-1 pack).  Drop-ins for df_upconv_fwd / df_upconv_dgrad with kz = 1, channels multiples of 32. */
int df_wino2d_upconv_fwd(const float* xc, const float* wp, const float* bias, float* y, int64_t B, int64_t Hc, int64_t Wc, int64_t Cin,
                         int64_t Cout, int flags, float leak, df_stream_t stream);
int df_wino2d_upconv_dgrad(const float* g, const float* wp, float* acc, int64_t B, int64_t Hc, int64_t Wc, int64_t Cin, int64_t Cout,
                           df_stream_t stream);


/* ---- opt-in "bf16x3" precision mode (conv_bf16.hip) ---------------------------------------------------------------------
 * fp32 operands are split a = hi + lo into two bf16 words and a*b ~= hi*hi + hi*lo + lo*hi runs on the bf16 matrix pipe
 * (3 x v_mfma_f32_32x32x16_bf16, fp32 accumulate): 16 significand bits per operand, ~5x the fp32 MFMA rate.  Same arguments
 * as the fp32 twins; weights must be packed by the matching *_bf16x3 pack call.  Needs Cin % 4 == 0, channels >= 16 (DF_ESHAPE)
 * and the input tensor (x / xc / g) 16-byte aligned (DF_EALIGN: this mode has no scalar-load kernel).  flags: those of the fp32 twin
 * without DF_CONV_VALU_ONLY (no thin layers here). */
int64_t df_conv_packed_elems_bf16x3(int64_t taps, int64_t cin, int64_t cout, int mode);   /* in 4-byte units */
int df_conv_pack_weights_bf16x3(const float* w, float* wp, int64_t taps, int64_t cin, int64_t cout, int mode,
                                df_stream_t stream);
int df_conv_fwd_bf16x3(const float* x, const float* wp, const float* bias, const float* residual, const float* mask_src,
                       float* y, int64_t B, int64_t D, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int kz, int flags,
                       float leak, df_stream_t stream);
int64_t df_upconv_packed_elems_bf16x3(int64_t cin, int64_t cout, int kz, int mode);
int df_upconv_pack_weights_bf16x3(const float* w, float* wp, int64_t cin, int64_t cout, int kz, int mode,
                                  df_stream_t stream);
int df_upconv_fwd_bf16x3(const float* xc, const float* wp, const float* bias, float* y, int64_t B, int64_t Dc, int64_t Hc,
                         int64_t Wc, int64_t Cin, int64_t Cout, int kz, int flags, float leak, df_stream_t stream);
int df_upconv_dgrad_bf16x3(const float* g, const float* wp, float* acc, int64_t B, int64_t Dc, int64_t Hc, int64_t Wc,
                           int64_t Cin, int64_t Cout, int kz, df_stream_t stream);
/* weight gradients in the same mode (workspaces: the fp32 *_workspace_bytes); rows with W not in {16,32,64,96,112} or thin
 * channels fall back to the exact fp32 kernels. */
int df_conv_wgrad_bf16x3(const float* x, const float* gy, float* gw, float* gb, int64_t B, int64_t D, int64_t H, int64_t W,
                         int64_t Cin, int64_t Cout, int kz, void* workspace, int64_t workspace_bytes, df_stream_t stream);
int df_upconv_wgrad_bf16x3(const float* xc, const float* gy, float* gw, float* gb, int64_t B, int64_t Dc, int64_t Hc,
                           int64_t Wc, int64_t Cin, int64_t Cout, int kz, void* workspace, int64_t workspace_bytes,
                           df_stream_t stream);

/* gw[kz,3,3,Cin,Cout] = sum_voxels x[voxel+tap][cin] * gy[voxel][cout]   (split over voxel ranges,
 * deterministic second-pass reduction through the workspace).  If gb != NULL it also receives the bias gradient
 * gb[cout] = sum_voxels gy[voxel][cout] (accumulated on the fly from the operand registers). */
int64_t df_conv_wgrad_workspace_bytes(int64_t B, int64_t D, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int kz);
int df_conv_wgrad(const float* x, const float* gy, float* gw, float* gb, int64_t B, int64_t D, int64_t H, int64_t W,
                  int64_t Cin, int64_t Cout, int kz, void* workspace, int64_t workspace_bytes, df_stream_t stream);
/* The same with the algorithm chosen by the caller instead of by size (df_conv_wgrad == algo 0):
 *   algo & 7: 0 best available | 1 direct kernels only | 2 at most Winograd in x | 3 Winograd F(2x2,3x3) in (x,y) wherever
 *             instantiated | 4 Winograd F(2x2x2,3x3x3) in (x,y,z) wherever instantiated (shapes without that form fall
 *             back towards 0 -- every choice returns the same gradient up to fp32 summation order);
 *   algo >> 3: number of voxel ranges of the partial sums (0 = default; <= 256).
 * Workspace: df_conv_wgrad_workspace_bytes covers every `algo & 7` with the default range count; a range override that needs
 * more is rejected with DF_EWORKSPACE. */
int df_conv_wgrad_algo(const float* x, const float* gy, float* gw, float* gb, int64_t B, int64_t D, int64_t H, int64_t W,
                       int64_t Cin, int64_t Cout, int kz, void* workspace, int64_t workspace_bytes, int algo,
                       df_stream_t stream);
/* Which kernel family df_conv_wgrad_algo runs for these arguments (16-byte aligned operands assumed) -- the size-based choices made
 * visible so that a silent fall-back to a slower form shows up in the caller's log (bench.py `dispatch`):
 *   0 direct MFMA | 1 Winograd in x | 2 Winograd in (x,y) | 3 Winograd in (x,y,z) | 10 thin layer (Cin or Cout <= 4) on the matrix
 *   cores | 11 thin layer on the vector ALU; negative = invalid arguments.  df_upconv_wgrad_form: 3 = 27-point Winograd-(x,y,z)
 *   form on the coarse input, 0 = parity-class kernels.  (No reference counterpart: TF picks cuDNN algorithms internally.)
 * Both queries see no pointers and keep assuming 16-byte aligned operands.  The launch itself looks at x and gy: the thin matrix-core
 * form (10 -> 11), the zero-padded rows, the staged default of the 128 -> 128 levels (-> the register-ring kernel of algo 4, same bits)
 * and the 27-point up-sampling form (3 -> 0) need 16 bytes; every 8-byte kernel (Winograd forms, bf16x3, parity-class pairs, exact-row
 * direct kernels) needs 8; an operand that is only 4-byte aligned takes the direct kernel with scalar loads (form 0).  Every fallback
 * returns the same gradient up to fp32 summation order. */
int df_conv_wgrad_form(int64_t B, int64_t D, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int kz, int algo);
int df_upconv_wgrad_form(int64_t B, int64_t Dc, int64_t Hc, int64_t Wc, int64_t Cin, int64_t Cout, int kz, int algo);

/* ---- uint8 image views for the sample sheets written during training (ops.py:154-188; trainer.py:144-147, trainer3.py:22-25) ----
 * Every value is uint8(clip((v + 1) * 127.5, 0, 255)) in fp32 (the cast truncates).  Outputs are DEVICE pointers to uint8.
 *
 * denorm_img3 / plane_view (ops.py:163-188) of x [B,Z,Y,X,C], C in 1..4, in one pass over x:
 *   xy [B,Y,X,C] = mean over z;  zy [B,Y,Z,C] = mean over x, y as the row (plane_view(.., xy_plane=False));
 *   xym [B,Y,X,C] = slice z = Z/2;  zym [B,Y,Z,C] = slice x = X/2.   Any output may be NULL (skipped), not all of them.
 * The means are sequential fp32 sums (ascending z / x) divided by the extent; run-to-run bitwise deterministic.
 * Errors: DF_EINVAL null input / non-positive extent / every output null, DF_ESHAPE C outside 1..4 or a [Z, X*C] row-plane beyond the
 * workgroup's LDS, DF_EALIGN input not 4-byte aligned. */
int df_plane_views3d(const float* x, uint8_t* xy, uint8_t* zy, uint8_t* xym, uint8_t* zym, int64_t B, int64_t Z, int64_t Y, int64_t X,
                     int64_t C, df_stream_t stream);
/* The same four views of u [B,Z,Y,X,3] and of curl(u) = the c of df_jacobian3d_fwd (trainer3.py:22-25: G and G_vort), the curl never
 * written: the c* views equal df_plane_views3d of df_jacobian3d_fwd's c bit for bit.  Every extent >= 2 (DF_ESHAPE otherwise). */
int df_velocity_views3d(const float* u, uint8_t* xy, uint8_t* zy, uint8_t* xym, uint8_t* zym, uint8_t* cxy, uint8_t* czy, uint8_t* cxym,
                        uint8_t* czym, int64_t B, int64_t Z, int64_t Y, int64_t X, df_stream_t stream);
/* denorm_img (ops.py:154-161): x [B,H,W,C] (nchw = 0) or [B,C,H,W] (nchw != 0) -> out [B,H,W,Co] uint8, always channels-last;
 * C = 2 gets a zero third channel (mapped like every value: 127), C > 3 keeps the first three, C = 1 | 3 is kept.
 * Errors: DF_EINVAL null pointer / non-positive extent, DF_ESHAPE C < 1, DF_EALIGN input not 4-byte aligned. */
int df_denorm_img2d(const float* x, uint8_t* out, int64_t B, int64_t H, int64_t W, int64_t C, int nchw, df_stream_t stream);

/* ---- density advection through a velocity field: the advect() mode of the reference's scene scripts (scene/smoke_pos_size.py:45-109,
 * scene/smoke3_vel_buo.py:49-125), which call mantaflow's advectSemiLagrange(order, boundaryWidth, clampMode).  mantaflow cannot be run
 * beside this library, so bit parity with it is NOT claimed: the definition below is the contract (tests/advect_ref.py restates it).
 *
 * density [B,(Z,)Y,X], velocity [B,(Z,)Y,X,C] with C = 2 (2-D) | 3 (3-D), fp32; channels are the (x, y[, z]) MAC face values
 * (copyArrayToGridMAC: component x of cell i sits on its low-x face); cell (i,j,k) is [..,k,j,i].  bnd >= 1 is the boundary width with
 * 2*bnd + 2 <= every extent; a cell is interior when bnd <= index < extent - bnd on every axis, else it is on the band.
 *   uc          = (0.5 * (vx(i,j,k) + vx(i+1,j,k))) * vel_scale, likewise y and z (interior cells only)
 *   interp(g,p) = linear interpolation of the cell-centred grid g, per axis q = p - 0.5, n = (int)q, s1 = q - n, s0 = 1 - s1;
 *                 q < 0 -> n = 0, s0 = 1, s1 = 0;  n >= extent - 1 -> n = extent - 2, s0 = 0, s1 = 1;  sum over the 2^d corners n, n+1,
 *                 s0*a + s1*b per axis, x innermost
 *   SL(g, +-dt) = interp(g, (i+.5, j+.5, k+.5) -+ dt*uc) on interior cells, 0 on the band
 * df_advect_sl*:  fwd = SL(density, dt) -- the whole step of order 1, the first half of order 2.
 * df_advect_mc*:  the second half of order 2 (MacCormack), one pass: bwd = SL(fwd, -dt), cor = fwd + 0.5 * (orig - bwd);
 *                 c = trunc((i,j,k) - dt*uc) per axis (no +0.5: mantaflow's doClampComponent) clamped to [0, extent - 2]; min / max of
 *                 orig over those of the 2^d corners c, c+1 that are interior cells (clamp_mode 1: also those around
 *                 trunc((i,j,k) + dt*uc)); none interior -> out = fwd;  clamp_mode 2 (the reference's default): out = fwd if
 *                 cor < min or cor > max, else cor;  clamp_mode 1: out = clamp(cor, min, max);  band: out = 0.
 * The order of the scheme is the caller's choice of entry points (1: sl alone; 2: sl, then mc on its result).  The step gathers: the
 * output must not alias an input.  Non-finite velocities select edge cells, never memory outside the arrays.
 * Errors: DF_EINVAL null pointer / non-positive extent / bnd < 1 / clamp_mode not 1 | 2 / output aliasing an input, DF_ESHAPE an
 * extent < 2*bnd + 2 or too large, DF_EALIGN a pointer not 4-byte aligned. */
int df_advect_sl2d(const float* density, const float* vel, float* fwd, int64_t B, int64_t Y, int64_t X, float dt, float vel_scale, int bnd,
                   df_stream_t stream);
int df_advect_sl3d(const float* density, const float* vel, float* fwd, int64_t B, int64_t Z, int64_t Y, int64_t X, float dt,
                   float vel_scale, int bnd, df_stream_t stream);
int df_advect_mc2d(const float* orig, const float* fwd, const float* vel, float* out, int64_t B, int64_t Y, int64_t X, float dt,
                   float vel_scale, int bnd, int clamp_mode, df_stream_t stream);
int df_advect_mc3d(const float* orig, const float* fwd, const float* vel, float* out, int64_t B, int64_t Z, int64_t Y, int64_t X, float dt,
                   float vel_scale, int bnd, int clamp_mode, df_stream_t stream);
/* Source stamp before a step (Sphere.applyToGrid): out[i] = mask[i] ? value : density[i] over n cells, mask a DEVICE pointer to uint8;
 * out == density stamps in place. */
int df_density_source(const float* density, const uint8_t* mask, float value, float* out, int64_t n, df_stream_t stream);
/* The d_adv frame (scene/smoke_pos_size.py:105-106): img [B,Y,X] uint8, row Y-1-y = uint8(clip(255 * density[b,y,:], 0, 255)); 3-D: of
 * the z mean (sequential ascending fp32 sum divided by Z).  The reference casts without the clip, so values outside [0,1] wrap there
 * and saturate here. */
int df_density_image2d(const float* density, uint8_t* img, int64_t B, int64_t Y, int64_t X, df_stream_t stream);
int df_density_image3d(const float* density, uint8_t* img, int64_t B, int64_t Z, int64_t Y, int64_t X, df_stream_t stream);

/* ---- a liquid carried through a velocity field: the advect() mode of the reference's liquid scene scripts (scene/liquid3_vis.py:47-148,
 * scene/liquid_pos_size.py:47-132), which seed marker particles in the liquid body and, per frame, trace them with mantaflow's
 * pp.advectInGrid(IntRK4, deleteInObstacle=False) and rebuild a surface level set with gridParticleIndex + unionParticleLevelset.
 * mantaflow cannot be run beside this library, so bit parity with it is NOT claimed: the definition below is the contract
 * (tests/particles_ref.py restates it).  Left out: extrapolateMACSimple (a generator emits velocities everywhere), markFluidCells,
 * resetOutflow, adjustNumber resampling (N is constant over a sequence), averagedParticleLevelset and phi.setBound (meshing: the
 * "liquid surface meshes" block at the end of this header).
 *
 * pos [B,N,D] fp32 positions in cell units (x, y[, z]), D = 2 | 3; cell (i,j,k) spans [i,i+1) x [j,j+1) x [k,k+1) and is [..,k,j,i] in
 * the grids.  vel [B,(Z,)Y,X,D] fp32 MAC face values (component a of cell i sits on the cell's low-a face: the layout of df_advect_*),
 * multiplied by vel_scale.  phi [B,(Z,)Y,X] fp32.  All arithmetic fp32, no fused multiply-add, in the order written.
 *   u(p)     MAC sample.  Component a is interpolated multilinearly in the frame q_a = p_a, q_b = p_b - 0.5 (b != a).  Per axis:
 *            q < 0 or NaN -> n = 0, s0 = 1, s1 = 0;  trunc(q) >= extent - 1 -> n = extent - 2, s0 = 0, s1 = 1;  else n = (int)q,
 *            s1 = q - n, s0 = 1 - s1.  Sum over the 2^D corners n, n+1 as s0*a + s1*b per axis, x innermost; then * vel_scale.
 *   trace    k1 = u(p), k2 = u(p + (0.5*dt)*k1), k3 = u(p + (0.5*dt)*k2), k4 = u(p + dt*k3),
 *            p' = p + (dt * (((k1 + 2*k2) + 2*k3) + k4)) / 6, then per axis p' = min(max(p', bnd), (extent - bnd) - 2^-10) (a NaN
 *            becomes bnd): particles are pushed back into the domain, none is deleted.  bnd >= 0, 2*bnd + 2 <= every extent.
 *   keys     key = b*ncell + ((k*Y + j)*X + i), int32, i = min((int)p_x, X - 1) (p_x < 0 or NaN -> 0), likewise j, k.
 *   ranges   the caller sorts the B*N keys STABLY (particles of one cell keep their index order), permutes the positions with
 *            df_particles_gather and builds cell_start [B*ncell + 1] int32: cell_start[c] = the number of keys < c, so that the
 *            particles of cell c are rows cell_start[c] .. cell_start[c+1] - 1 of pos_sorted [B*N,D].
 *   levelset radius = (0.5 * sqrt(D)) * (radius_factor + 0.01), w = (int)radius_factor + 1;  phi(c) = min(radius, min over the particles
 *            p of the cells within +-w of c on every axis that lie inside the grid of |centre(c) - p| - radius), centre = (i+.5, j+.5
 *            [, k+.5]), |v| = sqrt((vx*vx + vy*vy) + vz*vz).  A particle outside the window is farther than w + 0.5 from the centre,
 *            so whenever 2*radius <= w + 0.5 -- which holds for radius_factor 0.5, 1 and 2 in 2-D and 3-D, NOT for every value --
 *            this equals the minimum over ALL particles of the batch entry.  No atomics: results are deterministic.
 * df_particles_advect*: pos_out may be pos_in.  N = 0: nothing is launched (positions may then be null), phi = radius everywhere.
 * Non-finite positions or velocities and out-of-range entries of order / cell_start select edge cells or edge particles, never
 * memory outside the arrays.
 * Errors: DF_EINVAL null pointer / non-positive extent / N < 0 / bnd < 0 / radius_factor outside [0, 1024] / gather in place,
 * DF_ESHAPE an extent < 2 or < 2*bnd + 2 or too large, B*N or (keys, level set) B*ncell beyond int32, DF_EALIGN a pointer not 4-byte
 * (order: 8-byte) aligned. */
int df_particles_advect2d(const float* pos_in, float* pos_out, const float* vel, int64_t B, int64_t N, int64_t Y, int64_t X, float dt,
                          float vel_scale, int bnd, df_stream_t stream);
int df_particles_advect3d(const float* pos_in, float* pos_out, const float* vel, int64_t B, int64_t N, int64_t Z, int64_t Y, int64_t X,
                          float dt, float vel_scale, int bnd, df_stream_t stream);
int df_particles_cell_keys2d(const float* pos, int32_t* keys, int64_t B, int64_t N, int64_t Y, int64_t X, df_stream_t stream);
int df_particles_cell_keys3d(const float* pos, int32_t* keys, int64_t B, int64_t N, int64_t Z, int64_t Y, int64_t X, df_stream_t stream);
/* pos_sorted[r] = pos[order[r]] over n = B*N records of dim = 2 | 3 floats; order is a DEVICE pointer to int64 (the indices a sort
 * returns). */
int df_particles_gather(const float* pos, const int64_t* order, float* pos_sorted, int64_t n, int dim, df_stream_t stream);
int df_particle_levelset_union2d(const float* pos_sorted, const int32_t* cell_start, float* phi, int64_t B, int64_t N, int64_t Y, int64_t X,
                                 float radius_factor, df_stream_t stream);
int df_particle_levelset_union3d(const float* pos_sorted, const int32_t* cell_start, float* phi, int64_t B, int64_t N, int64_t Z, int64_t Y,
                                 int64_t X, float radius_factor, df_stream_t stream);

/* ---- the smoke solver step: the main() loop of the reference's default 2-D scene (scene/smoke_pos_size.py:186-195), a closed box
 * (open_bound=False):  source.applyToGrid, advectSemiLagrange(vel, density), advectSemiLagrange(vel, vel), setWallBcs, addBuoyancy,
 * solvePressure(cgAccuracy, cgMaxIterFac), setWallBcs.  The first two statements are df_density_source and df_advect_* above; the
 * rest is below.  mantaflow cannot be run beside this library, so bit parity with it is NOT claimed: the definition below is the
 * contract (tests/smoke_ref.py restates it; tests/smoke_obs_ref.py the obstacle rules and tests/smoke_open_ref.py the open sides further
 * down, tests/smoke_inflow_ref.py the noise inflow, the cylinder stamp and the per-entry force after that).  Left out: mantaflow's
 * convective outflow extrapolation (a zero-gradient fill stands in for it), the MIC(0) preconditioner.
 *
 * Layouts as for df_advect_*: density, pressure [B,(Z,)Y,X]; velocity [B,(Z,)Y,X,D], D = 2 | 3 MAC face values, component a of cell c
 * on c's low-a face; cell (i,j,k) is [..,k,j,i]; e_a the unit step along axis a.  A cell is interior when bnd <= index < extent - bnd
 * on every axis, else a wall cell; bnd >= 1 and every extent >= 2*bnd + 2.  Velocities are in cells per unit time (no vel_scale).  All
 * arithmetic fp32, no fused multiply-add, in the order written.
 *
 * 1. MAC self-advection (SemiLagrangeMAC / MacCormackCorrectMAC / the MAC clamp).  For component a of an interior cell c
 *      uface_a(c)[a] = vel[c][a];  uface_a(c)[b] = 0.25 * (((vel[c][b] + vel[c-e_a][b]) + vel[c+e_b][b]) + vel[c-e_a+e_b][b]), b != a
 *      fwd[c][a]     = interp(vel[..,a], centre(c) - dt*uface_a(c)), centre = (i+.5, j+.5[, k+.5]);  wall cells: 0 in every component
 *    interp is the rule of df_advect_* (q = p - 0.5 on EVERY axis, the same edge cases, s0*a + s1*b per axis, x innermost) applied to
 *    the one component as a cell-centred grid.  df_mac_advect_sl* is this, the whole step of order 1.
 *    df_mac_advect_mc* is the second half of order 2, one pass, neither bwd nor cor is stored:  where c and c - e_a are both interior
 *      bwd = interp(fwd[..,a], centre(c) + dt*uface_a(c)),  cor = fwd[c][a] + 0.5 * (vel[c][a] - bwd)
 *    and the clamp of df_advect_mc* per component with dt*uface_a in place of dt*uc: min / max of vel[..,a] over the interior cells among
 *    the corners of clamp(trunc((i,j,k) - dt*uface_a), 0, extent - 2) (clamp_mode 1: and of ... + dt*uface_a); none interior -> fwd;
 *    clamp_mode 2: fwd if cor < min or cor > max, else cor; clamp_mode 1: clamp(cor, min, max).  Elsewhere in interior cells out = fwd;
 *    wall cells 0.  Both gather: the output must not alias an input.
 * 2. Walls and buoyancy, df_wall_buoyancy*: component a of cell c is kept where c and c - e_a are both interior, else it is 0 (for a
 *    closed box this is setWallBcs).  Kept: out = vel[c][a] + (0.5 * force[a]) * (rho[c] + rho[c-e_a]).  out may be vel.  mantaflow's
 *    addBuoyancy uses force = -gravity * dt / dx; the drivers in ops.py default to dx = 1 / max(extent), restated from memory and not
 *    checked against mantaflow.
 * 3. Pressure projection.  On interior cells b[c] = -(((vel[c+e_x][x] - vel[c][x]) + (vel[c+e_y][y] - vel[c][y])) [+ (.. z ..)]) and
 *    (A x)[c] = n_c * x[c] - (sum of x over the interior neighbours, in the order x-, x+, y-, y+, z-, z+), n_c their number.  A is
 *    singular (constants); the system is consistent when the wall faces of vel are 0, as after step 2 (the b then sum to zero).
 *    Plain conjugate gradients from x = 0, per batch entry:  r = p = b, rr = r.r;  an entry stops, and is frozen from then on, when
 *    max|r| <= accuracy, when rr is not > 0, or after max_iter iterations;  else  beta = rr / rr_old (0 in the first iteration),
 *    p = r + beta*p, q = A p, alpha = rr / p.q (0 if p.q is not > 0), x = x + alpha*p, r = r - alpha*q.  An entry with b = 0 stops at
 *    iteration 0 with x = 0; nothing divides 0 by 0.  Dot products and max|r| are sums of one partial per workgroup of 256 consecutive
 *    cells of ONE entry (inside it: xor butterfly over the 64 lanes, then the 4 waves ascending), combined by 256 strided running sums
 *    and the same tree: the order depends on the extents alone, so an entry's result does not depend on the rest of the batch, and two
 *    runs agree bit for bit.  No floating-point atomics.
 *    mantaflow preconditions its CG with MIC(0), a sequential sweep; this solver does not.  Both stop at the same criterion, so the
 *    projected fields agree to the accuracy of the solve and not beyond.
 *      df_pressure_workspace_bytes(B, Z, Y, X)  (Z = 1 in 2-D) the caller's scratch: r, two p, q, partials, per-entry scalars
 *      df_pressure_init*          b, r = p = b, pressure = 0, first partials
 *      df_pressure_cg_direction*  iteration k = 0, 1, ..: the entry's decision, then p, q and the p.q partials     (launch 1)
 *      df_pressure_cg_update*     iteration k: alpha, x and r updates, the r.r and max|r| partials                    (launch 2)
 *      df_pressure_status         after direction(k): *active_count = entries still iterating, iterations[e] = updates entry e has
 *                                 been given (either pointer may be null; device pointers to int32)
 *      df_pressure_correct*       out[c][a] = vel[c][a] - (p[c] - p[c-e_a]) where c and c - e_a are interior, else 0 (the second
 *                                 setWallBcs); out may be vel.
 *    The caller runs init, then direction(k), update(k) for k = 0, 1, .. with the SAME accuracy and max_iter until status reports no
 *    active entry -- which direction(max_iter) guarantees -- and then correct.  Calls after an entry froze leave it untouched, so the
 *    result does not depend on how often the caller looks.
 * Errors: DF_EINVAL null pointer / non-positive extent / bnd < 1 / clamp_mode not 1 | 2 / negative k, max_iter or accuracy / an output
 * aliasing an array that is read at a neighbour / the workspace overlapping the velocity, the pressure or an int32 output, DF_ESHAPE an extent < 2*bnd + 2 or too large, DF_EALIGN a pointer not 4-byte
 * aligned, DF_EWORKSPACE ws_bytes below df_pressure_workspace_bytes (which itself returns a negative DF_E* code for bad extents). */
int df_mac_advect_sl2d(const float* vel, float* fwd, int64_t B, int64_t Y, int64_t X, float dt, int bnd, df_stream_t stream);
int df_mac_advect_sl3d(const float* vel, float* fwd, int64_t B, int64_t Z, int64_t Y, int64_t X, float dt, int bnd, df_stream_t stream);
int df_mac_advect_mc2d(const float* vel, const float* fwd, float* out, int64_t B, int64_t Y, int64_t X, float dt, int bnd, int clamp_mode,
                       df_stream_t stream);
int df_mac_advect_mc3d(const float* vel, const float* fwd, float* out, int64_t B, int64_t Z, int64_t Y, int64_t X, float dt, int bnd,
                       int clamp_mode, df_stream_t stream);
int df_wall_buoyancy2d(const float* vel, const float* density, float* out, int64_t B, int64_t Y, int64_t X, float fx, float fy, int bnd,
                       df_stream_t stream);
int df_wall_buoyancy3d(const float* vel, const float* density, float* out, int64_t B, int64_t Z, int64_t Y, int64_t X, float fx, float fy,
                       float fz, int bnd, df_stream_t stream);
int64_t df_pressure_workspace_bytes(int64_t B, int64_t Z, int64_t Y, int64_t X);
int df_pressure_init2d(const float* vel, float* pressure, void* ws, int64_t ws_bytes, int64_t B, int64_t Y, int64_t X, int bnd,
                       df_stream_t stream);
int df_pressure_init3d(const float* vel, float* pressure, void* ws, int64_t ws_bytes, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd,
                       df_stream_t stream);
int df_pressure_cg_direction2d(void* ws, int64_t ws_bytes, int64_t B, int64_t Y, int64_t X, int bnd, int64_t k, float accuracy,
                               int64_t max_iter, df_stream_t stream);
int df_pressure_cg_direction3d(void* ws, int64_t ws_bytes, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd, int64_t k, float accuracy,
                               int64_t max_iter, df_stream_t stream);
int df_pressure_cg_update2d(float* pressure, void* ws, int64_t ws_bytes, int64_t B, int64_t Y, int64_t X, int bnd, int64_t k,
                            df_stream_t stream);
int df_pressure_cg_update3d(float* pressure, void* ws, int64_t ws_bytes, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd, int64_t k,
                            df_stream_t stream);
int df_pressure_status(const void* ws, int64_t ws_bytes, int64_t B, int64_t Z, int64_t Y, int64_t X, int64_t k, int32_t* active_count,
                       int32_t* iterations, df_stream_t stream);
int df_pressure_correct2d(const float* vel, const float* pressure, float* out, int64_t B, int64_t Y, int64_t X, int bnd, df_stream_t stream);
int df_pressure_correct3d(const float* vel, const float* pressure, float* out, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd,
                          df_stream_t stream);

/* ---- the same step around obstacles: the main() loop of the reference's scene/smoke3_obs_buo.py:211-219 (a closed box with a sphere
 * obstacle stamped into the flag grid).  setWallBcs, KnAddBuoyancy and MacCormackCorrect(MAC) with obstacle flags are restated from
 * memory of mantaflow and cannot be checked against it here; as for the rest of this block, parity is with the restatement under
 * tests/ (tests/smoke_obs_ref.py), not with mantaflow.
 *
 * obstacle [B,(Z,)Y,X] uint8, nonzero = solid, one per batch entry (the sphere's position is a scene parameter).  A cell is FLUID when
 * it is interior in the sense above and not an obstacle.  df_obstacle_flags* packs, in one pass, one byte per cell into flags
 * [B,(Z,)Y,X]: bit 0 = the cell is fluid, bits 1..6 = its x-, x+, y-, y+, z-, z+ neighbour is fluid (a neighbour outside the grid is
 * not; the z bits are 0 in 2-D).  flags must not overlap obstacle.  Every `_flags` entry point takes such a flags array, built with the
 * SAME bnd, right after its array arguments and is otherwise its counterpart above with "interior" read as "fluid":
 *   - a face is kept by df_wall_buoyancy*_flags, updated by df_pressure_correct*_flags and corrected by df_mac_advect_mc*_flags where c
 *     and c - e_a are both fluid; every other face is 0 after the first two (solid faces carry no flow);
 *   - b, n_c and the neighbour sums of A run over fluid cells and fluid neighbours (n_c is the popcount of bits 1..6); p stays 0 on
 *     every other cell;
 *   - the min / max of the MacCormack clamps run over the fluid cells among the corners (none fluid -> fwd).
 * Two things keep ignoring obstacles, as mantaflow's SemiLagrange / SemiLagrangeMAC do: the first-order value fwd is that of
 * df_advect_sl* / df_mac_advect_sl*, which have no `_flags` variant, and df_density_source stamps regardless.  The MacCormack
 * correction and clamp apply where c is fluid (df_advect_mc*_flags) or where c and c - e_a are (df_mac_advect_mc*_flags, component
 * a); elsewhere in the interior the output is fwd, on wall cells 0.
 * A is now singular once per connected fluid region; the system stays consistent when the solid faces of vel are 0, as after
 * df_wall_buoyancy*_flags (b then sums to zero over every region).  A fluid cell without a fluid neighbour has n_c = 0 and only solid
 * faces, so b = 0 there: r never leaves 0, p stays 0, its velocity stays 0, nothing divides by n_c.  An entry that is solid everywhere
 * has b = 0 and stops at iteration 0.  df_pressure_workspace_bytes and df_pressure_status are shared with the entry points above.
 * Bit rule: with an all-zero obstacle every `_flags` entry point returns the bits of its counterpart.
 * A flags byte is believed only where the cell is interior by its index, so no flags content selects memory outside the arrays.
 * Errors: those of the counterparts, and DF_EINVAL for null flags or flags that overlap an output or the workspace. */
int df_obstacle_flags2d(const uint8_t* obstacle, uint8_t* flags, int64_t B, int64_t Y, int64_t X, int bnd, df_stream_t stream);
int df_obstacle_flags3d(const uint8_t* obstacle, uint8_t* flags, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd, df_stream_t stream);
int df_advect_mc2d_flags(const float* orig, const float* fwd, const float* vel, float* out, const uint8_t* flags, int64_t B, int64_t Y,
                         int64_t X, float dt, float vel_scale, int bnd, int clamp_mode, df_stream_t stream);
int df_advect_mc3d_flags(const float* orig, const float* fwd, const float* vel, float* out, const uint8_t* flags, int64_t B, int64_t Z,
                         int64_t Y, int64_t X, float dt, float vel_scale, int bnd, int clamp_mode, df_stream_t stream);
int df_mac_advect_mc2d_flags(const float* vel, const float* fwd, float* out, const uint8_t* flags, int64_t B, int64_t Y, int64_t X, float dt,
                             int bnd, int clamp_mode, df_stream_t stream);
int df_mac_advect_mc3d_flags(const float* vel, const float* fwd, float* out, const uint8_t* flags, int64_t B, int64_t Z, int64_t Y, int64_t X,
                             float dt, int bnd, int clamp_mode, df_stream_t stream);
int df_wall_buoyancy2d_flags(const float* vel, const float* density, float* out, const uint8_t* flags, int64_t B, int64_t Y, int64_t X,
                             float fx, float fy, int bnd, df_stream_t stream);
int df_wall_buoyancy3d_flags(const float* vel, const float* density, float* out, const uint8_t* flags, int64_t B, int64_t Z, int64_t Y,
                             int64_t X, float fx, float fy, float fz, int bnd, df_stream_t stream);
int df_pressure_init2d_flags(const float* vel, float* pressure, void* ws, int64_t ws_bytes, const uint8_t* flags, int64_t B, int64_t Y,
                             int64_t X, int bnd, df_stream_t stream);
int df_pressure_init3d_flags(const float* vel, float* pressure, void* ws, int64_t ws_bytes, const uint8_t* flags, int64_t B, int64_t Z,
                             int64_t Y, int64_t X, int bnd, df_stream_t stream);
int df_pressure_cg_direction2d_flags(void* ws, int64_t ws_bytes, const uint8_t* flags, int64_t B, int64_t Y, int64_t X, int bnd, int64_t k,
                                     float accuracy, int64_t max_iter, df_stream_t stream);
int df_pressure_cg_direction3d_flags(void* ws, int64_t ws_bytes, const uint8_t* flags, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd,
                                     int64_t k, float accuracy, int64_t max_iter, df_stream_t stream);
int df_pressure_cg_update2d_flags(float* pressure, void* ws, int64_t ws_bytes, const uint8_t* flags, int64_t B, int64_t Y, int64_t X, int bnd,
                                  int64_t k, df_stream_t stream);
int df_pressure_cg_update3d_flags(float* pressure, void* ws, int64_t ws_bytes, const uint8_t* flags, int64_t B, int64_t Z, int64_t Y, int64_t X,
                                  int bnd, int64_t k, df_stream_t stream);
int df_pressure_correct2d_flags(const float* vel, const float* pressure, float* out, const uint8_t* flags, int64_t B, int64_t Y, int64_t X,
                                int bnd, df_stream_t stream);
int df_pressure_correct3d_flags(const float* vel, const float* pressure, float* out, const uint8_t* flags, int64_t B, int64_t Z, int64_t Y,
                                int64_t X, int bnd, df_stream_t stream);

/* ---- the same step with open sides and a moving source: the main() loops of the reference's scene/smoke3_rot.py and scene/smoke3_mov.py
 * (open_bound 'xXyYzZ', a sphere source whose centre changes every frame), of scene/smoke3_vel_buo.py ('XyY'; its inflow is further down) and
 * the open_bound option of scene/smoke_pos_size.py ('xXyY').  mantaflow cannot be run beside this library: setOpenBound's corner rule, the
 * Dirichlet cells of its pressure solve and KnAddBuoyancy are restated from memory, and parity is with the NumPy restatement of THIS
 * definition (tests/smoke_open_ref.py), NOT with mantaflow.
 *
 * Layouts, bnd, "interior", "fluid" and the flags byte are those of the blocks above.
 * open_sides: an int; bits 0..5 mark the sides x-, x+, y-, y+, z-, z+ as open (the order of the flags byte's neighbour bits).  In 2-D
 * the z bits must be 0.
 * Cell classes.  A band cell (not interior by its index) is OPEN when, on every axis where its index lies outside [bnd, extent - bnd),
 * the side it lies on is open; every other band cell is a WALL cell, so an edge or corner shared with a closed side stays wall
 * (setOpenBound's rule).  The class depends on the index alone, an obstacle mask does not change it.  A face neighbour of an interior
 * cell is never an edge or corner cell, so "the a- neighbour of c is open" is p[a] == bnd && open(a-), and likewise on the high side.
 * Live face.  Component a of cell c is LIVE when one of c, c - e_a is fluid and the other is fluid or open.  With open_sides = 0 this
 * is the "kept face" above.
 *   - Pressure: p = 0 in open cells (Dirichlet).  n_c = fluid neighbours + open neighbours, the neighbour sums still run over fluid
 *     neighbours only, b is unchanged.  A fluid region that touches an open cell is a non-singular SPD system and its b need not sum to
 *     zero; a region that touches none is what it was.  ONLY df_pressure_cg_direction*_open differs from its counterpart, in n_c:
 *     df_pressure_init*(_flags), df_pressure_cg_update*(_flags), df_pressure_status and the workspace are used as they are.
 *   - Walls and buoyancy: a live face is kept; the buoyancy term is added only where c and c - e_a are both fluid (KnAddBuoyancy), a
 *     fluid-open face is kept without it.  Non-live components of fluid, solid and wall cells are 0; every component of an open cell that
 *     is not live is copied through unchanged, because it holds filled values.
 *   - Correction: on live faces out = vel - (p[c] - p[c - e_a]) with p read from the array (0 outside the fluid); everything else follows
 *     the walls-and-buoyancy rule.  This also corrects the face between the last fluid cell and an open cell, so EVERY fluid cell ends
 *     divergence free.  Deviation: as far as can be recalled, mantaflow's CorrectVelocity skips outflow cells there.
 *   - MAC self-advection: fwd as above for every component of an interior cell, and additionally for component a of an open cell whose
 *     c - e_a is interior by its index (the high-side boundary face; df_mac_advect_sl*_open has no flags argument because the
 *     first-order value keeps ignoring obstacles).  The MacCormack correction and clamp apply where the face is live; min / max still
 *     run over fluid corners only (none fluid -> fwd).  Other components of open cells are written 0, wall cells 0.
 *   - Fill, df_open_extrapolate*: in place, for every open cell c and component a, vel[c][a] = vel[c'][a] with c' = c clamped to
 *     [bnd, extent_a - bnd] on axis a and to [bnd, extent_b - bnd - 1] on every other axis b.  The sources are exactly the fixed points
 *     of that map (interior cells and the first high layer along a), and a fixed point copies onto itself: race free in place.  This is a
 *     zero-gradient fill, NOT mantaflow's extrapolateVelConvectiveBC, which divides by a bulk velocity and cannot be restated from
 *     memory.  Density needs nothing: df_advect_* already write 0 on the band, which is what resetOutflow(real=density) does.  The
 *     callers in ops.py run the fill after the self-advection and after the correction.
 *   - Sphere stamp, df_density_sphere_source*: out[c] = value where ((i+.5-cx)^2 + (j+.5-cy)^2) [+ (k+.5-cz)^2] <= radius*radius, else
 *     density[c]; (cx, cy[, cz]) = centers[b] for batch entry b, centers [B,D] fp32 in DEVICE memory.  fp32, no fused multiply-add, in
 *     that order.  out may be density.  A NaN centre stamps nothing.
 * Every `_open` entry point takes flags (may be NULL: no obstacles) after its arrays and open_sides after bnd.
 * Bit rule: with open_sides = 0 every `_open` entry point returns the bits of its closed counterpart -- with flags == NULL those of the
 * plain one, with flags those of the `_flags` one -- and df_open_extrapolate* writes nothing.
 * As for the flags: a byte is believed where the cell is interior by its index, and its low-neighbour bit also where the cell is a
 * high-side boundary cell by its index; no flags content selects memory outside the arrays.
 * Errors: those of the counterparts, and DF_EINVAL for open_sides outside 0..63, for z bits in 2-D, and for centres that overlap the
 * output. */
int df_mac_advect_sl2d_open(const float* vel, float* fwd, int64_t B, int64_t Y, int64_t X, float dt, int bnd, int open_sides,
                            df_stream_t stream);
int df_mac_advect_sl3d_open(const float* vel, float* fwd, int64_t B, int64_t Z, int64_t Y, int64_t X, float dt, int bnd, int open_sides,
                            df_stream_t stream);
int df_mac_advect_mc2d_open(const float* vel, const float* fwd, float* out, const uint8_t* flags, int64_t B, int64_t Y, int64_t X, float dt,
                            int bnd, int open_sides, int clamp_mode, df_stream_t stream);
int df_mac_advect_mc3d_open(const float* vel, const float* fwd, float* out, const uint8_t* flags, int64_t B, int64_t Z, int64_t Y, int64_t X,
                            float dt, int bnd, int open_sides, int clamp_mode, df_stream_t stream);
int df_wall_buoyancy2d_open(const float* vel, const float* density, float* out, const uint8_t* flags, int64_t B, int64_t Y, int64_t X,
                            float fx, float fy, int bnd, int open_sides, df_stream_t stream);
int df_wall_buoyancy3d_open(const float* vel, const float* density, float* out, const uint8_t* flags, int64_t B, int64_t Z, int64_t Y,
                            int64_t X, float fx, float fy, float fz, int bnd, int open_sides, df_stream_t stream);
int df_pressure_cg_direction2d_open(void* ws, int64_t ws_bytes, const uint8_t* flags, int64_t B, int64_t Y, int64_t X, int bnd,
                                    int open_sides, int64_t k, float accuracy, int64_t max_iter, df_stream_t stream);
int df_pressure_cg_direction3d_open(void* ws, int64_t ws_bytes, const uint8_t* flags, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd,
                                    int open_sides, int64_t k, float accuracy, int64_t max_iter, df_stream_t stream);
int df_pressure_correct2d_open(const float* vel, const float* pressure, float* out, const uint8_t* flags, int64_t B, int64_t Y, int64_t X,
                               int bnd, int open_sides, df_stream_t stream);
int df_pressure_correct3d_open(const float* vel, const float* pressure, float* out, const uint8_t* flags, int64_t B, int64_t Z, int64_t Y,
                               int64_t X, int bnd, int open_sides, df_stream_t stream);
int df_open_extrapolate2d(float* vel, int64_t B, int64_t Y, int64_t X, int bnd, int open_sides, df_stream_t stream);
int df_open_extrapolate3d(float* vel, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd, int open_sides, df_stream_t stream);
int df_density_sphere_source2d(const float* density, const float* centers, float radius, float value, float* out, int64_t B, int64_t Y,
                               int64_t X, df_stream_t stream);
int df_density_sphere_source3d(const float* density, const float* centers, float radius, float value, float* out, int64_t B, int64_t Z,
                               int64_t Y, int64_t X, df_stream_t stream);

/* ---- the noise inflow, the cylinder stamp and the per-entry force: what the main() loop of the reference's scene/smoke3_vel_buo.py:212-232
 * does beyond the blocks above -- densityInflow(flags, density, noise, shape=Cylinder, scale, sigma), Cylinder.applyToGrid(grid=vel,
 * value=inflow), and an inflow velocity and a buoyancy that differ per scene.  mantaflow cannot be run beside this library: KnApplyNoiseInfl,
 * the cylinder's distance and ApplyShapeToMACGrid are restated from memory, and mantaflow's NoiseField(loadFromFile=True) is wavelet
 * noise read from a tile file, which cannot be restated at all.  A seeded lattice value noise of this project's OWN stands in for it.
 * Parity is with the NumPy restatement of THIS definition (tests/smoke_inflow_ref.py), NOT with mantaflow.
 *
 * Layouts as above.  All arithmetic fp32, no fused multiply-add, in the order written; sqrt and / are the correctly rounded ones;
 * max(x, y) and min(x, y) are only ever taken of numbers.
 * Cylinder.  cyl [B, 2*D + 1] fp32 in DEVICE memory, one per batch entry, in cell units: centre (cx, cy[, cz]), half-axis vector
 * (zx, zy[, zz]), radius.  |z|^2 = (zx*zx + zy*zy) [+ zz*zz], |z| = sqrt(|z|^2), a = z / |z| per component.  An entry is VALID when all
 * its 2*D + 1 numbers are finite and 0 < |z|^2 < inf; an entry that is not (a zero-length axis, a NaN) stamps nothing, in both entry
 * points.  For a point q:  d = q - centre;  h = (dx*ax + dy*ay) [+ dz*az];  r2 = max(((dx*dx + dy*dy) [+ dz*dz]) - h*h, 0).
 * Coordinates are meant to stay below 2^60 in magnitude, so that no square overflows.
 *   - Noise inflow, df_density_noise_inflow*: a cell that is not interior (bnd, as above; bnd = 0 is allowed here: no band) is copied
 *     through.  For an interior cell c, q = (i, j[, k]) -- the cell INDEX, as mantaflow's kernel passes it, not the centre:
 *       dh = |h| - |z|,  dr = sqrt(r2) - radius,  sdf = min(max(dh, dr), 0) + sqrt(max(dh, 0)^2 + max(dr, 0)^2)
 *     the exact signed distance of the finite cylinder.  Unless sdf <= sigma, out = density.  Else
 *       factor = min(max(1 - (0.5 / sigma) * (sdf + sigma), 0), 1),  target = (N(c) * scale) * factor,
 *       out = target > density ? target : density
 *     so a density that is not below the target comes back with its own bits.  target is 0 at sdf = sigma.
 *     A cell farther than (|z| + |radius|) + (sigma + 1) from the centre along any axis is copied without evaluating sdf; its sdf exceeds
 *     sigma by a whole cell, so this changes no result.
 *     N(c), the noise:  tq = time_anim * time;  per axis a  q_a = ((float(c_a) * pos_scale[a]) * inv_extent + pos_offset[a]) + tq, clamped
 *     to [-2^30, 2^30] (a NaN becomes -2^30);  f_a = floor(q_a),  t_a = q_a - f_a,  l_a = int32(f_a) reinterpreted as uint32,
 *     w_a = (t_a*t_a) * (3 - 2*t_a).  The lattice value at (ix, iy, iz), uint32 arithmetic mod 2^32, iz = 0 in 2-D:
 *       h = seed ^ (ix * 0x8DA6B343) ^ (iy * 0xD8163841) ^ (iz * 0xCB1AB31F);
 *       h ^= h >> 16;  h *= 0x7FEB352D;  h ^= h >> 15;  h *= 0x846CA68B;  h ^= h >> 16;   value = float(h >> 8) * 2^-23 - 1   in [-1, 1)
 *     D-linear interpolation with lerp(a, b, w) = a + w*(b - a): along x with w_x at (ly, lz), (ly+1, lz)[, (ly, lz+1), (ly+1, lz+1)], then
 *     along y with w_y[, then along z with w_z]; the high corners are l + 1 mod 2^32.  Then v = (v + val_offset) * val_scale, and with
 *     clamp != 0  v = min(max(v, clamp_neg), clamp_pos).  The noise is continuous across lattice planes (w = 0 returns the low corner
 *     exactly), so a floor that differs by rounding moves the value by rounding only.
 *     noise is a HOST pointer read during the call; inv_extent is 1 / X for mantaflow's scaling by the grid's x extent.  out may be density.
 *   - Cylinder stamp, df_mac_cylinder_stamp*: for batch entry b, component a of cell c is set to values[b][a] (values [B,D] fp32 in DEVICE
 *     memory) when the position of that face, q = (i, j+.5[, k+.5]) for x, (i+.5, j[, k+.5]) for y, (i+.5, j+.5, k) for z, satisfies
 *     |h| <= |z| and r2 < radius*radius; else it is copied through.  Faces are tested one by one.  There is no flags argument and no
 *     bnd: the stamp ignores obstacles and the band.  out may be vel.
 *   - Per-entry force, df_wall_buoyancy*_open_dev: df_wall_buoyancy*_open with force[a] of batch entry b read from forces [B,D] fp32 in
 *     DEVICE memory.  flags may be NULL and open_sides may be 0.  Bit rule: when every row equals (fx, fy[, fz]) it returns the bits of
 *     df_wall_buoyancy*_open with those scalars -- which, by that entry point's own bit rule, are those of the closed and `_flags` forms.
 * Errors: DF_EINVAL null pointer / non-positive extent / sigma not a positive number / bnd < 0 (inflow), < 1 (force) / open_sides as above /
 * cylinders, values or forces that overlap the output / out == density (force), DF_ESHAPE an extent too large (force: or < 2*bnd + 2),
 * DF_EALIGN a pointer not 4-byte aligned.  The cylinders live in device memory, so a zero-length axis is not an error here: it stamps
 * nothing. */
typedef struct df_noise_params {
  float pos_scale[3];   /* [2] is not read in 2-D */
  float pos_offset[3];
  float time_anim, val_offset, val_scale;
  int32_t clamp;        /* nonzero: clamp to [clamp_neg, clamp_pos] */
  float clamp_neg, clamp_pos;
  uint32_t seed;
  float inv_extent;
} df_noise_params;
int df_density_noise_inflow2d(const float* density, float* out, const float* cyl, const df_noise_params* noise, float time, float scale,
                              float sigma, int64_t B, int64_t Y, int64_t X, int bnd, df_stream_t stream);
int df_density_noise_inflow3d(const float* density, float* out, const float* cyl, const df_noise_params* noise, float time, float scale,
                              float sigma, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd, df_stream_t stream);
int df_mac_cylinder_stamp2d(const float* vel, const float* cyl, const float* values, float* out, int64_t B, int64_t Y, int64_t X,
                            df_stream_t stream);
int df_mac_cylinder_stamp3d(const float* vel, const float* cyl, const float* values, float* out, int64_t B, int64_t Z, int64_t Y, int64_t X,
                            df_stream_t stream);
int df_wall_buoyancy2d_open_dev(const float* vel, const float* density, float* out, const uint8_t* flags, const float* forces, int64_t B,
                                int64_t Y, int64_t X, int bnd, int open_sides, df_stream_t stream);
int df_wall_buoyancy3d_open_dev(const float* vel, const float* density, float* out, const uint8_t* flags, const float* forces, int64_t B,
                                int64_t Z, int64_t Y, int64_t X, int bnd, int open_sides, df_stream_t stream);

/* ---- the liquid solver step: the main() loops of the reference's liquid scenes (scene/liquid_pos_size.py:254-295, scene/liquid3_d_r.py),
 * a FLIP step in the script's order:  pp.advectInGrid(IntRK4), mapPartsToMAC, extrapolateMACFromWeight(distance=2), markFluidCells,
 * addGravity, setWallBcs, solvePressure, setWallBcs, extrapolateMACSimple(distance=4), flipVelocityUpdate(flipRatio).  The trace, the keys,
 * the gather and the ranges are df_particles_* above, the solve reuses df_pressure_init*_flags, df_pressure_cg_update*_flags,
 * df_pressure_status and the workspace; the rest is below.  mantaflow cannot be run beside this library: its kernels are restated from
 * memory, and parity is with the NumPy restatement of THIS definition (tests/liquid_ref.py), NOT with mantaflow.
 * In this block p = 0 sits at the centres of the air cells, a first-order surface; the averaged level set, phi.setBound and the
 * ghost-fluid surface treatment (solvePressure(phi=)) are the opt-in block at the end of this header.
 * Left out of this block: resetOutflow and open sides; obstacles inside the liquid; the MIC(0) preconditioner.  adjustNumber resampling,
 * extrapolateLsSimple and per-entry particle counts (here one call takes one N) are the opt-in block at the end of this header.
 *
 * Layouts, bnd, "interior", e_a, u(p) and the per-axis weights (n; s0, s1) are those of the blocks above.  pos, pvel [B,N,D] fp32 SORTED
 * by key (df_particles_gather with the order of the key sort, for both); vel, weight [B,(Z,)Y,X,D] fp32; marks [B,(Z,)Y,X,D] uint8;
 * flags [B,(Z,)Y,X] uint8.  All arithmetic fp32, no fused multiply-add, in the order written; no floating-point atomics; the result of a
 * batch entry does not depend on the rest of the batch.
 *   p2g      df_liquid_p2g*: the transpose of u(p).  For component a of cell c, every particle p of the 3^D cells around c that lie inside
 *            the grid is visited in ascending cell order (z, then y, then x), inside a cell in sorted order, with
 *            w = (w_x * w_y) [* w_z],  w_b = s0 if n == c_b, s1 if n + 1 == c_b, else 0, (n; s0, s1) the weights of q_b = p_b (b == a) or
 *            q_b = p_b - 0.5 (b != a): the weight with which u(p) reads that face (only the 2 cells along a and the 3 along every other
 *            axis can reach it; the others add w = 0).  num += w * pvel_a, den += w from 0;  weight = den, vel = den > 0 ? num / den : 0,
 *            known (may be NULL) = den > 0 ? 1 : 0.  N = 0: zeros everywhere, the particle arrays and cell_start may be NULL.
 *   extrapolate  df_mac_extrapolate*, ONE layer per call, layer = 1, 2, ...: a component a of cell c with mark 0, c and c - e_a interior,
 *            looks at the same component of c - e_x, c + e_x, c - e_y, c + e_y[, c - e_z, c + e_z] in that order; with cnt > 0 of them
 *            marked in 1..layer it becomes (sum of their values in that order) / (float)cnt and takes mark layer + 1.  Everything else
 *            is copied, so wall faces are never filled (they may be sources).  Reads (vel, mark), writes (vel_out, mark_out): no overlap.
 *   flags    df_liquid_flags*: the byte of df_obstacle_flags* with "fluid" = LIQUID = interior and cell_start[c + 1] > cell_start[c]
 *            (bit 0 the cell, bits 1..6 its x-, x+, y-, y+, z-, z+ neighbour).  touch (may be NULL) [..,D]: 1 where c or c - e_a is
 *            liquid -- the "known" of the second extrapolation.  N = 0: all air, cell_start may be NULL.
 *   forces   df_liquid_forces*: component a of c is 0 unless c and c - e_a are interior; there it gets + force[a] when c or c - e_a is
 *            liquid and is copied otherwise.  out may be vel.
 *   pressure rows for liquid cells only: b = -div, n_c = the neighbours interior by their index (liquid or air), the neighbour sums run
 *            over liquid neighbours, p = 0 in air.  ONLY df_pressure_cg_direction*_liquid differs from the `_flags` solve, in n_c.
 *            df_pressure_correct*_liquid: where c and c - e_a are interior and one of them is liquid, out = vel - (p[c] - p[c - e_a])
 *            with p as the array holds it; other faces between interior cells are copied, wall faces are 0.  A liquid region with no air
 *            neighbour is singular but consistent, as in a closed box.
 *            Bit rule: with every interior cell liquid both return the bits of df_pressure_cg_direction* / df_pressure_correct*.
 *   flip     df_flip_update*: un = u(vel, p), d = un - u(vel_old, p), pvel' = flip_ratio * (pvel + d) + (1 - flip_ratio) * un with
 *            1 - flip_ratio rounded to fp32 once on the host.  pvel_out may be pvel_in.  N = 0: nothing is launched.
 * Non-finite values and out-of-range entries of cell_start select edge cells or edge particles, never memory outside the arrays; a flags
 * byte is believed only where the cell is interior by its index.
 * Errors: DF_EINVAL null pointer / non-positive extent / N < 0 / bnd < 1 / layer outside 1..254 / flip_ratio outside [0, 1] / an output
 * that is or overlaps an array the launch gathers from (extrapolate in place, marks or flags over a velocity, outputs over cell_start),
 * DF_ESHAPE an extent < 2*bnd + 2 or too large, B*N or B*ncell beyond int32, DF_EALIGN a float or int32 pointer not 4-byte aligned,
 * DF_EWORKSPACE (the pressure entry points) a workspace smaller than df_pressure_workspace_bytes. */
int df_liquid_p2g2d(const float* pos_sorted, const float* pvel_sorted, const int32_t* cell_start, float* vel, float* weight, uint8_t* known,
                    int64_t B, int64_t N, int64_t Y, int64_t X, df_stream_t stream);
int df_liquid_p2g3d(const float* pos_sorted, const float* pvel_sorted, const int32_t* cell_start, float* vel, float* weight, uint8_t* known,
                    int64_t B, int64_t N, int64_t Z, int64_t Y, int64_t X, df_stream_t stream);
int df_mac_extrapolate2d(const float* vel, const uint8_t* mark, float* vel_out, uint8_t* mark_out, int64_t B, int64_t Y, int64_t X, int bnd,
                         int layer, df_stream_t stream);
int df_mac_extrapolate3d(const float* vel, const uint8_t* mark, float* vel_out, uint8_t* mark_out, int64_t B, int64_t Z, int64_t Y, int64_t X,
                         int bnd, int layer, df_stream_t stream);
int df_liquid_flags2d(const int32_t* cell_start, uint8_t* flags, uint8_t* touch, int64_t B, int64_t N, int64_t Y, int64_t X, int bnd,
                      df_stream_t stream);
int df_liquid_flags3d(const int32_t* cell_start, uint8_t* flags, uint8_t* touch, int64_t B, int64_t N, int64_t Z, int64_t Y, int64_t X,
                      int bnd, df_stream_t stream);
int df_liquid_forces2d(const float* vel, const uint8_t* flags, float* out, int64_t B, int64_t Y, int64_t X, float fx, float fy, int bnd,
                       df_stream_t stream);
int df_liquid_forces3d(const float* vel, const uint8_t* flags, float* out, int64_t B, int64_t Z, int64_t Y, int64_t X, float fx, float fy,
                       float fz, int bnd, df_stream_t stream);
int df_pressure_cg_direction2d_liquid(void* ws, int64_t ws_bytes, const uint8_t* flags, int64_t B, int64_t Y, int64_t X, int bnd, int64_t k,
                                      float accuracy, int64_t max_iter, df_stream_t stream);
int df_pressure_cg_direction3d_liquid(void* ws, int64_t ws_bytes, const uint8_t* flags, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd,
                                      int64_t k, float accuracy, int64_t max_iter, df_stream_t stream);
int df_pressure_correct2d_liquid(const float* vel, const float* pressure, float* out, const uint8_t* flags, int64_t B, int64_t Y, int64_t X,
                                 int bnd, df_stream_t stream);
int df_pressure_correct3d_liquid(const float* vel, const float* pressure, float* out, const uint8_t* flags, int64_t B, int64_t Z, int64_t Y,
                                 int64_t X, int bnd, df_stream_t stream);
int df_flip_update2d(const float* pos, const float* pvel_in, float* pvel_out, const float* vel, const float* vel_old, int64_t B, int64_t N,
                     int64_t Y, int64_t X, float flip_ratio, df_stream_t stream);
int df_flip_update3d(const float* pos, const float* pvel_in, float* pvel_out, const float* vel, const float* vel_old, int64_t B, int64_t N,
                     int64_t Z, int64_t Y, int64_t X, float flip_ratio, df_stream_t stream);

/* ---- implicit velocity diffusion: cgSolveDiffusion(flags, vel, alphaV) of the reference's viscous liquid scene (scene/liquid3_vis.py:277-281),
 * once per solver step between setWallBcs and addGravity.  mantaflow cannot be run beside this library: the system is restated from
 * memory (MakeLaplaceMatrix on an all-fluid dummy flag grid, scaled by alpha, plus the identity, identity rows in obstacle cells; u handed
 * in as the first guess) and reduced to its symmetric positive definite interior block; parity is with the NumPy restatement of THIS
 * definition (tests/diffuse_ref.py), NOT with mantaflow.
 * Left out: adjustNumber; the MIC(0) preconditioner; obstacles (the level set and the ghost-fluid surface: the block at the end) --
 * mantaflow's identity rows are the bnd band only.
 *
 * vel [B,(Z,)Y,X,D] fp32, alpha [B] fp32 >= 0 in DEVICE memory (the caller checks the values; a negative or non-finite alpha yields
 * meaningless numbers, never an access outside the arrays).  For every entry e and component a, u = vel[e,..,a] is a scalar grid, I the
 * cells interior by index (bnd <= index < extent - bnd on every axis; bnd >= 1, so all 2D axis neighbours of a cell of I exist):
 *      (1 + 2D*alpha) x_c - alpha * sum_{nb in I} x_nb  =  u_c + alpha * sum_{nb not in I} u_nb          for c in I,
 * cells outside I are Dirichlet data and are copied through bit for bit.  Plain conjugate gradients, the iteration and the stop rule of
 * the pressure solve (an entry is active while max|r| > accuracy && r.r > 0 && iterations < max_iter), over the B*D (entry, component)
 * pairs, each its own system that converges on its own; pair e*D + a takes the place of batch entry e of the pressure workspace:
 *      df_diffuse_workspace_bytes(B, Z, Y, X, D)  (Z = 1 for D = 2): df_pressure_workspace_bytes(B*D, Z, Y, X), then the planar x [B*D,n]
 *      df_diffuse_init*           x = u (every cell), r = p = alpha * (sum of all 2D neighbours of u, x-, x+, y-, y+[, z-, z+] from 0,
 *                                 - 2D * u) on I and 0 off it, the first partials.  alpha = 0: r = 0, no iteration, the input's bits.
 *      df_diffuse_cg_direction*   df_pressure_cg_direction* with q_c = p_c + alpha * (2D * p_c - sum_{nb in I} p_nb)
 *      df_diffuse_cg_update*      df_pressure_cg_update* on x (the same kernel)
 *      df_pressure_status         with B*D for B, on the same workspace pointer: iterations[e*D + a]
 *      df_diffuse_finish*         out[e,..,a] = x of pair e*D + a.  out may be vel (init has read all of it).
 * All arithmetic fp32, no fused multiply-add, in the order written; the partial sums are combined in an order that depends on the grid
 * extents alone, so a pair's result depends neither on the rest of the batch nor on the other components; frozen pairs are not touched.
 * Errors, on the host and before any launch: DF_EINVAL null pointer / non-positive extent / bnd < 1 / k < 0 / max_iter < 0 / accuracy < 0
 * / the workspace overlapping vel, alpha or out, DF_ESHAPE an extent < 2*bnd + 2 or too large, DF_EALIGN a pointer not 4-byte aligned,
 * DF_EWORKSPACE ws_bytes below df_diffuse_workspace_bytes (which itself returns a negative DF_E* code for bad extents or D). */
int64_t df_diffuse_workspace_bytes(int64_t B, int64_t Z, int64_t Y, int64_t X, int dim);
int df_diffuse_init2d(const float* vel, const float* alpha, void* ws, int64_t ws_bytes, int64_t B, int64_t Y, int64_t X, int bnd,
                      df_stream_t stream);
int df_diffuse_init3d(const float* vel, const float* alpha, void* ws, int64_t ws_bytes, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd,
                      df_stream_t stream);
int df_diffuse_cg_direction2d(const float* alpha, void* ws, int64_t ws_bytes, int64_t B, int64_t Y, int64_t X, int bnd, int64_t k,
                              float accuracy, int64_t max_iter, df_stream_t stream);
int df_diffuse_cg_direction3d(const float* alpha, void* ws, int64_t ws_bytes, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd, int64_t k,
                              float accuracy, int64_t max_iter, df_stream_t stream);
int df_diffuse_cg_update2d(void* ws, int64_t ws_bytes, int64_t B, int64_t Y, int64_t X, int bnd, int64_t k, df_stream_t stream);
int df_diffuse_cg_update3d(void* ws, int64_t ws_bytes, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd, int64_t k, df_stream_t stream);
int df_diffuse_finish2d(void* ws, int64_t ws_bytes, float* out, int64_t B, int64_t Y, int64_t X, int bnd, df_stream_t stream);
int df_diffuse_finish3d(void* ws, int64_t ws_bytes, float* out, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd, df_stream_t stream);

/* ---- the liquid solver's surface: averagedParticleLevelset(pp, pindex, flags, gpi, phi, radius_factor, 1, 1) + phi.setBound(1, bWidth)
 * and solvePressure(flags, vel, pressure, phi=phi), the two calls every liquid loop of the reference makes (scene/liquid_pos_size.py:254-295,
 * scene/liquid3_d_r.py, scene/liquid3_vis.py).  mantaflow cannot be run beside this library: both are restated from memory, the
 * definitions below are this library's own, and parity is with the NumPy restatement of THESE definitions (tests/liquid_gf_ref.py), NOT
 * with mantaflow.  Still left out: resetOutflow and open sides, obstacles inside the liquid, MIC(0); adjustNumber and extrapolateLsSimple
 * are the block after this one.
 * DF_VERSION is NOT raised by this block (it has stayed 207 through every solver block of this header): a client cannot tell from
 * df_version() whether these symbols exist and has to look them up (dlsym), as for the smoke and liquid blocks above.
 *
 * Layouts, bnd, "interior", e_a and the sorted particles are those of the blocks above; phi [B,(Z,)Y,X] fp32.  All arithmetic fp32, no
 * fused multiply-add, in the order written; no floating-point atomics; an entry's result does not depend on the rest of the batch.
 *   averaged level set   df_particle_levelset_averaged*: R = (0.5 * sqrt(D)) * (radius_factor + 0.01) (the radius of the union form),
 *            r = (int)R + 1, R4 = 4 * (R * R).  For cell c with centre x_c = index + 0.5, every particle p of the cells within +-r of c on
 *            every axis that lie inside the grid is visited in ascending cell order (z, then y, then x), inside a cell in sorted order:
 *            s2 = dx*dx + dy*dy [+ dz*dz] with d = x_c - p;  w = max(0, 1 - s2 / R4);  wacc += w;  pacc_a += w * p_a  (from 0).
 *            wacc > 1e-6: phi = sqrt(ex*ex + ey*ey [+ ez*ez]) - R with e_a = x_c,a - pacc_a / wacc; otherwise phi = R.  N = 0: phi = R
 *            everywhere, the particle arrays and cell_start may be NULL.
 *   smoothing            df_levelset_smooth*, ONE pass per call, out != in unless mode is 0.  mode 1: a cell off the outermost layer of the
 *            grid becomes t = (((self + x-) + x+) + y-) + y+ [+ z-) + z+] * (1 / (2D + 1)), that constant rounded to fp32 once; the
 *            outermost layer is copied.  mode 2: the same t, kept only where t < self.  mode 0: a copy.  band > 0: the cells within `band`
 *            of a side are set to bound_value instead of the pass's result (phi.setBound, fused into the last pass).
 *   ghost-fluid system   rows for the liquid cells of flags (df_liquid_flags*).  For a liquid cell i and a neighbour a that is interior by
 *            its index and not liquid:  denom = phi_i - phi_a;  theta = 0.5 if denom > -1e-4, else min(max(phi_i / denom, gf_clamp), 1)
 *            (a NaN gives gf_clamp).  Row i:  sum over liquid neighbours (p_i - p_n) + sum over air neighbours p_i * (1 / theta) = -div_i;
 *            wall neighbours contribute nothing.  diag_i = the sum, from 0 and in the order x-, x+, y-, y+[, z-, z+], of 1 per liquid
 *            neighbour and 1 / theta per air neighbour (1 if that sum is 0); off-diagonals -1 between liquid cells.  Symmetric, positive
 *            definite wherever a region touches air.
 *   solve    Jacobi-preconditioned conjugate gradients from p = 0 in the loop of the plain solve (two launches per iteration, every scalar
 *            on the device, fixed-order partials, entries converge on their own, frozen entries untouched):
 *      df_pressure_workspace_bytes_gf(B, Z, Y, X)   df_pressure_workspace_bytes, then diag [B,n] and z [B,n]
 *      df_pressure_init*_gf           x = 0, r = b, diag, z = p = r / diag, the first r.z and max|r| partials
 *      df_pressure_cg_direction*_gf   beta = r.z / (r.z)_old, p = z + beta * p_old, q = diag * p - sum over liquid neighbours, the p.q partials;
 *                                     an entry stays active while max|r| > accuracy (the UNscaled residual) && r.z > 0 && iterations < max_iter
 *      df_pressure_cg_update*_gf      alpha = r.z / p.q, x += alpha p, r -= alpha q, z = r / diag, the next partials
 *      df_pressure_status             unchanged, on the same workspace pointer (its words lie where the plain solve keeps them)
 *   correction  df_pressure_correct*_gf: component a of cell c with c and c - e_a interior: both liquid: out = vel - (p[c] - p[c - e_a]);
 *            c alone liquid: out = vel - p[c] * (1 / theta); c - e_a alone liquid: out = vel + p[c - e_a] * (1 / theta), theta of the liquid
 *            cell towards the air cell (the air side's pressure replaced by the ghost value p_i * (1 - 1 / theta)); neither liquid:
 *            copied; every other face 0.  out may be vel.
 * A flags byte is believed only where the cell is interior by its index; non-finite phi changes numbers, never addresses.
 * Errors, on the host and before any launch: those of the blocks above, and DF_EINVAL for gf_clamp outside (0, 1], a smoothing mode
 * outside 0..2, a negative band, a null phi, a smoothing output that overlaps its input (modes 1, 2), a workspace that overlaps phi;
 * DF_EWORKSPACE for ws_bytes below df_pressure_workspace_bytes_gf. */
int df_particle_levelset_averaged2d(const float* pos_sorted, const int32_t* cell_start, float* phi, int64_t B, int64_t N, int64_t Y,
                                    int64_t X, float radius_factor, df_stream_t stream);
int df_particle_levelset_averaged3d(const float* pos_sorted, const int32_t* cell_start, float* phi, int64_t B, int64_t N, int64_t Z,
                                    int64_t Y, int64_t X, float radius_factor, df_stream_t stream);
int df_levelset_smooth2d(const float* phi_in, float* phi_out, int64_t B, int64_t Y, int64_t X, int mode, int band, float bound_value,
                         df_stream_t stream);
int df_levelset_smooth3d(const float* phi_in, float* phi_out, int64_t B, int64_t Z, int64_t Y, int64_t X, int mode, int band,
                         float bound_value, df_stream_t stream);
int64_t df_pressure_workspace_bytes_gf(int64_t B, int64_t Z, int64_t Y, int64_t X);
int df_pressure_init2d_gf(const float* vel, float* pressure, void* ws, int64_t ws_bytes, const uint8_t* flags, const float* phi, int64_t B,
                          int64_t Y, int64_t X, int bnd, float gf_clamp, df_stream_t stream);
int df_pressure_init3d_gf(const float* vel, float* pressure, void* ws, int64_t ws_bytes, const uint8_t* flags, const float* phi, int64_t B,
                          int64_t Z, int64_t Y, int64_t X, int bnd, float gf_clamp, df_stream_t stream);
int df_pressure_cg_direction2d_gf(void* ws, int64_t ws_bytes, const uint8_t* flags, int64_t B, int64_t Y, int64_t X, int bnd, int64_t k,
                                  float accuracy, int64_t max_iter, df_stream_t stream);
int df_pressure_cg_direction3d_gf(void* ws, int64_t ws_bytes, const uint8_t* flags, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd,
                                  int64_t k, float accuracy, int64_t max_iter, df_stream_t stream);
int df_pressure_cg_update2d_gf(float* pressure, void* ws, int64_t ws_bytes, const uint8_t* flags, int64_t B, int64_t Y, int64_t X, int bnd,
                               int64_t k, df_stream_t stream);
int df_pressure_cg_update3d_gf(float* pressure, void* ws, int64_t ws_bytes, const uint8_t* flags, int64_t B, int64_t Z, int64_t Y, int64_t X,
                               int bnd, int64_t k, df_stream_t stream);
int df_pressure_correct2d_gf(const float* vel, const float* pressure, float* out, const uint8_t* flags, const float* phi, int64_t B, int64_t Y,
                             int64_t X, int bnd, float gf_clamp, df_stream_t stream);
int df_pressure_correct3d_gf(const float* vel, const float* pressure, float* out, const uint8_t* flags, const float* phi, int64_t B, int64_t Z,
                             int64_t Y, int64_t X, int bnd, float gf_clamp, df_stream_t stream);

/* ---- the liquid solver's resampling: ragged particle batches, extrapolateLsSimple(phi, distance, inside) and adjustNumber(pp, vel, flags,
 * minParticles, maxParticles, phi, radiusFactor), the last calls of the reference's liquid loops (scene/liquid_pos_size.py,
 * scene/liquid3_d_r.py, scene/liquid3_vis.py) that this library did not have.  mantaflow cannot be run beside this library: all of it is
 * restated from memory, the definitions below are this library's own, and parity is with the NumPy restatement of THESE definitions
 * (tests/liquid_resample_ref.py), NOT with mantaflow.  Opt-in: nothing above calls any of it.  The step that uses it runs, per frame: trace,
 * keys, sort, p2g, 2 layers, flags, the averaged level set with its band, the extrapolation (4, inside), forces, the solve (the ghost-fluid
 * one sees the extrapolated phi), the resampling against the projected velocity, 4 layers, the FLIP update on old and new particles.  DF_VERSION is NOT raised.
 *
 *   ragged batches   pos, pvel [P,D] fp32 with P = B*N rows (N is only the capacity per entry that makes P a multiple of B);
 *            entry_start [B+1] int32 in DEVICE memory, non-decreasing.  Rows entry_start[b] .. entry_start[b+1] - 1 belong to entry b: the
 *            entry of row i is (the number of b in 0..B with entry_start[b] <= i) - 1, found by bisection; rows from entry_start[B] on
 *            (and below entry_start[0]) are unused.  df_particles_advect*_ragged, df_particles_cell_keys*_ragged and
 *            df_flip_update*_ragged are the entry points above with that entry in place of i / N: an unused row is neither read nor
 *            written by the trace and the FLIP update, and gets the key B*ncell, which sorts behind every cell.  The stable sort keeps the
 *            entries contiguous and in order, and the ranges over keys 0 .. B*ncell hold the live total in their last element, so every
 *            entry point driven by cell_start (p2g, flags, both level sets) takes a ragged batch as it is, with N = P / B.
 *            Bit rule: with entry_start[b] = b*N the ragged forms return the bits of the dense ones.  Whatever entry_start holds, the
 *            entry found lies in 0..B-1: it changes numbers, never addresses.
 *   extrapolation    of phi [B,(Z,)Y,X] over the cells off the outermost layer of the grid (index 1 .. extent - 2 on every axis); the
 *            outermost layer is never marked, read as a source or written.  df_levelset_extrapolate_marks*: mark 1 where phi > 0
 *            (inside = 1) or phi < 0 (inside = 0); mark 2 on an unmarked cell with a face neighbour marked 1; else 0.
 *            df_levelset_extrapolate_layer*, ONE layer per call, layer = 2, 3, ..., IN PLACE: a cell with mark 0 and n > 0 face
 *            neighbours marked `layer` becomes phi = (the sum of those neighbours' phi, from 0, in the order x-, x+, y-, y+[, z-, z+])
 *            / (float)n + direction, direction = -1 for inside = 1 and +1 otherwise, and takes mark layer + 1.  A launch writes cells
 *            marked 0 only and reads phi of cells marked `layer` only, so it is race free in place.  extrapolateLsSimple(distance) is the
 *            marks and the layers 2 .. distance; distance <= 1 changes nothing.  The marks handed to a layer call must be those of
 *            df_levelset_extrapolate_marks* (and the layers before it) on the same phi with the SAME `inside`; the library cannot check that.
 *   resampling       of SORTED ragged particles.  R = (0.5 * sqrt(D)) * (radius_factor + 0.01), surface = -2 * R.
 *            df_resample_count*: for every (entry, cell) its range of cell_start is walked in sorted order with a counter k from 0; for
 *            a particle p, phiv = the D-linear interpolation of the entry's cell-centred phi at p (weights (n; s0, s1) of q_a = p_a - 0.5,
 *            along x, then y[, then z], as u(p) combines them).  The particle is dropped if phiv > 0, else if k > max_particles and
 *            phiv <= surface; else it is kept and k += 1.  keep[row] = 1 or 0, kept[cell] = k, seeds[cell] = min_particles - k if the cell
 *            is interior and liquid by flags (df_liquid_flags*), phi[cell] <= surface and k < min_particles; else 0.
 *            The caller scans kept + seeds into new_start [B*ncell + 1] int32 (exclusive; the last element is the wanted total);
 *            new_entry_start[b] = new_start[b*ncell].
 *            df_resample_scatter*: for every (entry, cell) the kept particles of its range (position and velocity bits) go to rows
 *            new_start[cell] + 0, 1, ... in order, then seed m = 0 .. seeds - 1 follows: its coordinate a is
 *            float(c_a) + float(h >> 8) * 2^-24 with h the integer mix of the lattice noise above applied to
 *            seed ^ (step * 0x8DA6B343) ^ ((entry*ncell + cell) * 0xD8163841) ^ ((m*D + a) * 0xCB1AB31F), a 24-bit uniform in [0, 1).
 *            That sum can round up to float(c_a + 1); it is then replaced by the largest float below float(c_a + 1) (its bit pattern
 *            minus one), so a seed lies in [c_a, c_a + 1) and keeps its cell's key.  A seed's velocity is u(vel, p) of its entry.  The
 *            output is sorted by cell with new_start as its cell_start.  No row >= P is read or written: when the wanted total exceeds
 *            P the tail is left out, and the caller, who holds the total in new_start, has to refuse the result.
 * Every index read from device memory (cell_start, new_start, seeds, entry_start) is clamped before use; a flags byte is believed only
 * where the cell is interior by its index.  No atomics, no floating-point sums whose order depends on scheduling.
 * Errors, on the host and before any launch: those of the blocks above, and DF_EINVAL for a null entry_start (N > 0), inside outside 0..1,
 * layer outside 2..254, marks that overlap phi, min_particles outside 1..4096, max_particles outside min_particles..8192, scatter outputs
 * that overlap an input or each other; DF_ESHAPE when B*ncell*min_particles + P does not fit an int32. */
int df_particles_advect2d_ragged(const float* pos_in, float* pos_out, const float* vel, const int32_t* entry_start, int64_t B, int64_t N,
                                 int64_t Y, int64_t X, float dt, float vel_scale, int bnd, df_stream_t stream);
int df_particles_advect3d_ragged(const float* pos_in, float* pos_out, const float* vel, const int32_t* entry_start, int64_t B, int64_t N,
                                 int64_t Z, int64_t Y, int64_t X, float dt, float vel_scale, int bnd, df_stream_t stream);
int df_particles_cell_keys2d_ragged(const float* pos, int32_t* keys, const int32_t* entry_start, int64_t B, int64_t N, int64_t Y, int64_t X,
                                    df_stream_t stream);
int df_particles_cell_keys3d_ragged(const float* pos, int32_t* keys, const int32_t* entry_start, int64_t B, int64_t N, int64_t Z, int64_t Y,
                                    int64_t X, df_stream_t stream);
int df_flip_update2d_ragged(const float* pos, const float* pvel_in, float* pvel_out, const float* vel, const float* vel_old,
                            const int32_t* entry_start, int64_t B, int64_t N, int64_t Y, int64_t X, float flip_ratio, df_stream_t stream);
int df_flip_update3d_ragged(const float* pos, const float* pvel_in, float* pvel_out, const float* vel, const float* vel_old,
                            const int32_t* entry_start, int64_t B, int64_t N, int64_t Z, int64_t Y, int64_t X, float flip_ratio,
                            df_stream_t stream);
int df_levelset_extrapolate_marks2d(const float* phi, uint8_t* mark, int64_t B, int64_t Y, int64_t X, int inside, df_stream_t stream);
int df_levelset_extrapolate_marks3d(const float* phi, uint8_t* mark, int64_t B, int64_t Z, int64_t Y, int64_t X, int inside, df_stream_t stream);
int df_levelset_extrapolate_layer2d(float* phi, uint8_t* mark, int64_t B, int64_t Y, int64_t X, int inside, int layer, df_stream_t stream);
int df_levelset_extrapolate_layer3d(float* phi, uint8_t* mark, int64_t B, int64_t Z, int64_t Y, int64_t X, int inside, int layer,
                                    df_stream_t stream);
int df_resample_count2d(const float* pos_sorted, const int32_t* cell_start, const float* phi, const uint8_t* flags, uint8_t* keep, int32_t* kept,
                        int32_t* seeds, int64_t B, int64_t N, int64_t Y, int64_t X, int bnd, int min_particles, int max_particles,
                        float radius_factor, df_stream_t stream);
int df_resample_count3d(const float* pos_sorted, const int32_t* cell_start, const float* phi, const uint8_t* flags, uint8_t* keep, int32_t* kept,
                        int32_t* seeds, int64_t B, int64_t N, int64_t Z, int64_t Y, int64_t X, int bnd, int min_particles, int max_particles,
                        float radius_factor, df_stream_t stream);
int df_resample_scatter2d(const float* pos_sorted, const float* pvel_sorted, const int32_t* cell_start, const uint8_t* keep, const int32_t* seeds,
                          const int32_t* new_start, const float* vel, float* pos_out, float* pvel_out, int64_t B, int64_t N, int64_t Y,
                          int64_t X, int min_particles, uint32_t seed, uint32_t step, df_stream_t stream);
int df_resample_scatter3d(const float* pos_sorted, const float* pvel_sorted, const int32_t* cell_start, const uint8_t* keep, const int32_t* seeds,
                          const int32_t* new_start, const float* vel, float* pos_out, float* pvel_out, int64_t B, int64_t N, int64_t Z,
                          int64_t Y, int64_t X, int min_particles, uint32_t seed, uint32_t step, df_stream_t stream);

/* ---- multigrid preconditioner of the smoke pressure solve (opt-in; the plain solve above is untouched) -------------------------------
 * A V-cycle z = M r for the matrices of the plain, `_flags` and `_open` smoke solves, and the two kernels of the preconditioned
 * recurrence.  The definition below is this library's own (as the projection's is) and it is the one that is tested:
 * tests/smoke_mg_ref.py restates it in fp64 and as an op-for-op fp32 twin whose bits the kernels give.  The free-surface, ghost-fluid
 * and diffusion systems use the same hierarchy block and the same cycle through deepfluids_hip_liquid_mg.h (a library of its own: this
 * header is frozen), which adds their level 0 and an iteration whose rows are level 0.  DF_VERSION is NOT raised by this block either (tests pin 207): look the symbols up.
 *
 * Level 0 is the solve's own grid, band included, and the solve's own matrix, stored as face weights: w_a[c] for the face between c and
 *   c - e_a, 1 if both cells are fluid, else 0 (a neighbour outside the grid has no face); dir[c] = the number of open neighbours of a
 *   fluid cell (what open sides add to n_c), 0 elsewhere; diag[c] = the sum of the 2D incident w, plus dir[c].
 * Coarser levels: extents ceil(extent / 2) per axis, until every extent is <= 2.  Aggregate I holds the children 2I and 2I + 1 along each
 *   axis, where they exist.  The weights are the Galerkin product with piecewise-constant interpolation: w_a^c[I] = the sum of w_a[i]
 *   over the fine faces with i_a = 2 I_a and the other coordinates inside the aggregate (faces inside an aggregate vanish), dir^c[I] = the
 *   sum of dir over the children, diag^c = the sum of the incident w^c plus dir^c.  The children are summed in ascending x, then y, then
 *   z.  All of it is float32 and exact (small integers).  A cell with diag = 0 is inactive on its level: its value is 0 and its residual
 *   is 0.  There are no cell types above level 0: obstacles, walls, open sides, odd extents, split regions and enclosed cells are all
 *   carried by the weights.
 * (A x)[c] = diag[c] * x[c] - sum, the sum taken from 0 in the order x-, x+, y-, y+[, z-, z+] over the neighbours inside the grid, each
 *   term w * x[neighbour] with the weight of the face between them.
 * One damped-Jacobi sweep: x'[c] = x[c] + (omega * (r[c] - (A x)[c])) / diag[c] on active cells, omega = float(2) / float(3).
 * V-cycle on level l, from x = 0:  two sweeps, the first of them as x[c] = (omega * r[c]) / diag[c];  the residual r - A x;
 *   r^c[I] = the sum of the children's residuals from 0 in the order above;  e = the V-cycle of level l + 1 on r^c;
 *   x[c] += alpha * e[parent(c)] on active cells;  two sweeps.  The coarsest level runs eight sweeps, the first as above.  z is x of level
 *   0.  alpha in [1, 2) over-corrects for the piecewise-constant interpolation.  All arithmetic fp32, no fused multiply-add, in the order
 *   written; no reductions across cells, no atomics; an entry's result does not depend on the rest of the batch.
 * Because the coarse operators are Galerkin and the smoother is symmetric, M is symmetric positive semidefinite for every geometry.
 * The iteration is the preconditioned one in the form of the `_gf` entry points: CgState::rr and the `rr` partials hold r.z,
 *   p = z + beta * p; it stops on the UNscaled max|r| exactly as the plain solve does (accuracy, max_iter, the iteration counts and the
 *   frozen-entry rule are unchanged).  Every V-cycle kernel returns at once for an entry that is no longer active.
 *
 *   df_mg_hierarchy_bytes(dim, B, Z, Y, X)   the bytes of a hierarchy block (weights, per-level scratch and z); -1 for bad extents.
 *                                            dim = 2 takes Z = 1.  Extents as the solves accept them (every extent >= 4).
 *   df_mg_levels(dim, Z, Y, X)               the number of levels; -1 for bad extents
 *   df_mg_sweeps(coarsest)                   the scheme's sweep counts: 0 -> the pre- / post-sweeps (2), 1 -> the coarsest level's (8); else -1
 *   df_mg_omega()                            the damping as the kernels hold it, float(2) / float(3)
 *   df_mg_cycle_launches(dim, Z, Y, X)       kernel launches of one V-cycle: four per level of more than 1024 cells (and level 0), one for
 *                                            all smaller levels together (one workgroup per entry walks them, same arithmetic); -1 for
 *                                            bad extents
 *   df_mg_level_offset(.., level, array)     the float offset inside the block of an array [B, cells of the level]: array 0..dim-1 = w_a,
 *                                            dim = dir, dim + 1 = diag, dim + 2 = the level's right-hand side (level 0: z), dim + 3 and
 *                                            dim + 4 = the two x buffers; -1 if there is none
 *   df_mg_build          writes every level's weights from flags (nullable: no obstacles; df_obstacle_flags*), bnd and open_sides
 *   df_mg_apply          z = M r for r [B,(Z,)Y,X]; z is array dim + 2 of level 0.  Nothing of the block is read before it is written.
 *   df_pressure_mg_precondition   the same on the r of a solve's workspace (df_pressure_workspace_bytes), and the r.z partials.  k = -1:
 *                        after df_pressure_init*, before direction 0; k >= 0: after update k, skipping the entries update k skipped
 *   df_pressure_cg_direction_mg / df_pressure_cg_update_mg   df_pressure_cg_direction* / _update* for the preconditioned recurrence
 *                        (flags nullable, open_sides may be 0); update writes r and the max|r| partials, z comes from the cycle after it
 * Errors, on the host and before any launch: DF_EINVAL (null pointer, dim, alpha outside [1, 2), open_sides, overlapping arrays, k),
 * DF_ESHAPE (extents), DF_EALIGN, DF_EWORKSPACE (a hierarchy or a workspace too small). */
int64_t df_mg_hierarchy_bytes(int dim, int64_t B, int64_t Z, int64_t Y, int64_t X);
int df_mg_levels(int dim, int64_t Z, int64_t Y, int64_t X);
int df_mg_sweeps(int coarsest);
float df_mg_omega(void);
int df_mg_cycle_launches(int dim, int64_t Z, int64_t Y, int64_t X);
int64_t df_mg_level_offset(int dim, int64_t B, int64_t Z, int64_t Y, int64_t X, int level, int array);
int df_mg_build(void* hierarchy, int64_t hierarchy_bytes, const uint8_t* flags, int dim, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd,
                int open_sides, df_stream_t stream);
int df_mg_apply(void* hierarchy, int64_t hierarchy_bytes, const float* r, int dim, int64_t B, int64_t Z, int64_t Y, int64_t X, float alpha,
                df_stream_t stream);
int df_pressure_mg_precondition(void* hierarchy, int64_t hierarchy_bytes, void* ws, int64_t ws_bytes, int dim, int64_t B, int64_t Z, int64_t Y,
                                int64_t X, float alpha, int64_t k, df_stream_t stream);
int df_pressure_cg_direction_mg(void* ws, int64_t ws_bytes, void* hierarchy, int64_t hierarchy_bytes, const uint8_t* flags, int dim, int64_t B,
                                int64_t Z, int64_t Y, int64_t X, int bnd, int open_sides, int64_t k, float accuracy, int64_t max_iter,
                                df_stream_t stream);
int df_pressure_cg_update_mg(float* pressure, void* ws, int64_t ws_bytes, const uint8_t* flags, int dim, int64_t B, int64_t Z, int64_t Y,
                             int64_t X, int bnd, int64_t k, df_stream_t stream);

/* ---- liquid surface meshes: a 3-D level set as an indexed triangle mesh (opt-in; nothing above calls it) ------------------------------
 * What the reference's 3-D liquid scripts get from phi.createMesh(mesh) + mesh.save('obj/%04d.obj') (scene/liquid3_vis.py:136-143).  The
 * definition below is this library's own, NOT mantaflow's marching cubes, and no parity with mantaflow's mesh is claimed:
 * tests/liquid_mesh_ref.py restates it in fp64 and as an op-for-op fp32 twin whose bits the kernels give.  Marching tetrahedra on the Kuhn
 * (Freudenthal) split of the cubes between cell centres; 3-D only (no 2-D contours, no smoothMesh / subdivideMesh: smooth phi instead).
 * DF_VERSION is NOT raised by this block either (tests pin 207): look the symbols up.
 *
 *   samples    the cell centres of phi [B,Z,Y,X] (fp32, negative inside): sample (x, y, z) sits at (x + 0.5, y + 0.5, z + 0.5) in grid
 *              units, the particles' coordinates.  Inside means phi < 0 strictly: an exact zero (of either sign) is outside.
 *   meshed box samples lo .. hi per axis, lo = bnd', hi = extent - 1 - bnd'; bnd' = bnd, or bnd - 1 with `closed` (which needs bnd >= 1).
 *              With `closed` every sample with a coordinate <= lo or >= hi (the box's outer layer, and whatever lies beyond it for the
 *              normals' differences) is read as fmax(phi, closed_value), closed_value > 0: a liquid resting against a wall is capped
 *              and every mesh is a closed surface.  "The value of a sample" below is this effective value.
 *   edges      sample v owns the edges v -- v + d for the 7 non-zero 0/1 vectors d (a number 1..7: bit 0 = x, bit 1 = y, bit 2 = z)
 *              whose far end lies in the box.  An edge carries a vertex when exactly one of its ends is inside.  mask[v] holds bit d - 1
 *              for every such edge, and in bit 7 whether v itself is inside; 0 outside the box.
 *   vertices   p = (v + 0.5) + t * d with t = s_v / (s_v - s_{v+d}), always from the owner's end; per coordinate (float)v_a + 0.5f, plus t
 *              where d has the axis.  fp32, no contraction.  Order: by owner sample index (x fastest, over the whole batch), then d
 *              ascending; the edge (v, d) is row vertex_offset[v] + popcount(mask[v] & ((1 << (d - 1)) - 1)).  No hashing, no atomics,
 *              no sort: a mesh is indexed, one vertex per crossing edge, shared by every triangle around it.
 *   normals    (optional)  g(u) = the central differences of the sample values at u, (s(u + e_a) - s(u - e_a)) * 0.5, on the GRID's border
 *              the one-sided difference s(u + e_a) - s(u) resp. s(u) - s(u - e_a);  n = g(v) + t * (g(v + d) - g(v)) per component;
 *              len = sqrt((n_x n_x + n_y n_y) + n_z n_z);  n / len, or (0, 0, 0) unless len > 0.
 *   tets       the cube with corner c (every c with c + (1,1,1) in the box; cube index = the sample index of c) splits into 6 tets, one
 *              per permutation (a, b, g) of the axes, in lexicographic order with x < y < z (xyz, xzy, yxz, yzx, zxy, zyx):
 *              p0 = c, p1 = c + e_a, p2 = c + e_a + e_b, p3 = c + (1,1,1).  Tet edges are numbered by their corner pairs 01, 02, 03, 12,
 *              13, 23; the pair (i, j), i < j, is the grid edge owned by p_i with d = p_j - p_i.
 *   triangles  of a tet with n inside corners: n = 0, 4 none.  n = 1 (corner k inside, the others q1 < q2 < q3) and n = 3 (corner k
 *              outside): the triangle (k q1, k q2, k q3).  n = 2 (i < j inside, k < l outside): (i k, i l, j l), then (i k, j l, j k).
 *              Each is written with its last two vertices exchanged when flip = sigma ^ (n == 3) ^ (the permutation (a, b, g) is odd),
 *              sigma the parity of (k, q1, q2, q3) resp. (i, j, k, l) as a permutation of (0, 1, 2, 3).  That winds every triangle so
 *              that its normal points out of the liquid, towards larger phi.  At most 12 triangles per cube.  Order: by cube index (x
 *              fastest, over the whole batch), then tet, then as listed.  A face holds vertex rows LOCAL to its batch entry (row -
 *              vertex_offset[b * Z*Y*X]).
 *
 *   df_mesh_capacity_bound   what = 0: the edges of the box, the most vertices any phi can give; what = 1: 12 per cube; both times B.
 *                            Pure host arithmetic (no device); a DF_E* code (< 0) for bad arguments.
 *   df_mesh_count            mask, nvert (the vertices v owns, 0..7), ntri (the triangles of the cube with corner v, 0..12): [B*Z*Y*X] uint8.
 *                            The caller scans nvert and ntri over the whole batch into vertex_offset, face_offset [B*Z*Y*X + 1] int32
 *                            (exclusive; the last elements are the totals V and T), reads the two totals, and allocates.
 *   df_mesh_emit             vertices [V,3] (xyz), normals [V,3] (nullable: not computed), faces [T,3] int32.  Rows >= vertex_capacity
 *                            resp. face_capacity are not written, whatever the offsets hold: the caller, who holds the totals, has to
 *                            refuse a result that did not fit.  A mask bit is believed only where its edge exists by the sample's index.
 *                            bnd, closed and closed_value must be those of the count.  The batch is ragged in the entry_start style:
 *                            vertex_start[b] = vertex_offset[b * Z*Y*X], face_start[b] = face_offset[b * Z*Y*X].
 * Errors, on the host and before any launch: DF_EINVAL (null pointer, non-positive extent, bnd < 0, closed outside 0..1, closed with
 * bnd = 0, a closed_value that is not finite and > 0, a negative capacity), DF_ESHAPE (an extent below 2, bnd too wide for the grid: the box
 * has no cube; 12 * B*Z*Y*X >= 2^31, which covers the 7 vertices per sample as well), DF_EALIGN (4 bytes). */
int64_t df_mesh_capacity_bound(int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd, int closed, int what);
int df_mesh_count(const float* phi, uint8_t* mask, uint8_t* nvert, uint8_t* ntri, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd,
                  int closed, float closed_value, df_stream_t stream);
int df_mesh_emit(const float* phi, const uint8_t* mask, const int32_t* vertex_offset, const int32_t* face_offset, float* vertices,
                 float* normals, int32_t* faces, int64_t vertex_capacity, int64_t face_capacity, int64_t B, int64_t Z, int64_t Y, int64_t X,
                 int bnd, int closed, float closed_value, df_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DEEPFLUIDS_HIP_H */
