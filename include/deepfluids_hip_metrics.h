/*
 * deepfluids_hip_metrics.h -- C-ABI of libdeepfluids_hip_metrics.so (gfx950 / MI355X only): fused field metrics.
 *
 * How well a generated velocity field g reproduces a ground truth x: the error sums of the training losses, the divergence of both
 * fields and the extrema, per batch entry, in ONE pass over the two fields (each read from HBM once; the stencil halos are cache
 * hits; no temporary the size of a field).  What `Trainer.evaluate_` sweeps over a data set.
 *
 * A library and a header of their own: deepfluids_hip.h is frozen at DF_VERSION 207 (its entry points and enumerators are pinned by
 * count and digest), and nothing of the train step calls these.  The library links against libdeepfluids_hip.so and follows every
 * convention of deepfluids_hip.h: device pointers, caller-owned buffers, asynchronous on `stream`, 0 / DF_E* / hipError_t, and the
 * message of a failure is read with df_last_error() of the main library.
 *
 * ---- definition --------------------------------------------------------------------------------------------------------------
 * g, x      [B,Y,X,2] | [B,Z,Y,X,3] fp32, dense; D = 2 | 3 components.  Cell c of an entry is its flat index, x fastest:
 *           c = (z * Y + y) * X + x, N = (Z) Y X cells.
 * mask      NULL, or uint8 [B,N] (mask_per_entry = 1) or [N] (mask_per_entry = 0, shared by the batch).  A cell is COUNTED when the
 *           mask is NULL or its byte is non-zero.  Neighbours are read whatever their own byte says.
 * per counted cell, all fp32, no fused multiply-add, in the order written (d_k = g_k - x_k):
 *   a1 = (|d_0| + |d_1|) [+ |d_2|]          a2 = (d_0 d_0 + d_1 d_1) [+ d_2 d_2]         m = max(max(|d_0|, |d_1|) [, |d_2|])
 *   x1 = (|x_0| + |x_1|) [+ |x_2|]          x2 = (x_0 x_0 + x_1 x_1) [+ x_2 x_2]
 *   aj = the sum, from 0, of |D_a g_k - D_a x_k| over the axes a = x, y [, z] and, within an axis, the components k = 0 .. D-1.
 *        D_a is the forward difference of df_jacobian2d_fwd / df_jacobian3d_fwd: f[i+1] - f[i], and on the last position of the
 *        axis f[n-1] - f[n-2] (the difference is replicated).  These are the D*D components of `ops.jacobian` / `ops.jacobian3`,
 *        bit for bit; their sum over all cells is what g_loss_j_l1 averages.
 *   a cell with x < X-1, y < Y-1 [, z < Z-1] also HOLDS A DIVERGENCE, the value df_divergence2d / df_divergence3d store at
 *        [b,(z,)y,x]:  div f = (D_x f_0 + D_y f_1) [+ D_z f_2], the same differences as above.  |div g| and |div x| of it are used.
 * per entry, over its counted cells:
 *   count, div_count (the counted cells that hold a divergence), sums of a1, a2, x1, x2, aj, |div g|, |div x|; the maxima of m,
 *   |div g|, |div x| (0 when nothing is counted); argmax = the cell of max m, the LOWEST cell on a tie, -1 when count = 0.
 * summation order (no atomics, nothing depends on scheduling; an entry's numbers do not depend on B or on the other entries):
 *   workgroup w of an entry owns cells 1024 w .. 1024 w + 1023; its thread t (0..255) owns cells 1024 w + 256 i + t, i = 0..3.
 *   1. a thread adds its counted cells' terms in ascending i to fp32 accumulators that start at 0;
 *   2. the 256 thread sums become fp64 and are added as a tree inside each 64-thread wave: for off = 32, 16, 8, 4, 2, 1 lane l
 *      (l < off) takes v[l] + v[l + off]; then the four wave sums are added in ascending order, ((w0 + w1) + w2) + w3;
 *   3. a second launch, one workgroup per entry: thread t adds the workgroup sums t, t + 256, t + 512, ... in ascending order in
 *      fp64 from 0, the 256 results are added as in 2., and the fp64 total is rounded to fp32 once.
 *   Counts are integers; maxima are exact in any order; the arg-max ties are broken by the cell index at every step.
 *
 * out       [B, DF_FM_WORDS] 32-bit words per entry: int32 at DF_FM_COUNT, DF_FM_DIV_COUNT, DF_FM_ARGMAX; fp32 at DF_FM_SUM_ABS
 *           (a1), DF_FM_SUM_SQ (a2), DF_FM_MAX_ABS (m), DF_FM_SUM_ABS_X (x1), DF_FM_SUM_SQ_X (x2), DF_FM_SUM_ABS_JAC (aj),
 *           DF_FM_SUM_ABS_DIV_G, DF_FM_MAX_ABS_DIV_G, DF_FM_SUM_ABS_DIV_X, DF_FM_MAX_ABS_DIV_X; every other word is written as 0.
 * ws        df_field_metrics_workspace_bytes(dim, B, Z, Y, X) bytes (dim = 2 takes Z = 1), 8-byte aligned: the workgroup sums.
 *           Nothing is read from it before it is written; -1 for bad extents; pure host arithmetic, answers without a device.
 * Errors, on the host and before any launch: DF_EINVAL (null g, x, out or ws; a non-positive extent; mask_per_entry outside 0..1;
 * out or ws overlapping each other or an input), DF_ESHAPE (an extent below 2; N >= 2^31, which the int32 cell index cannot hold;
 * more than 2^31 - 1 workgroups), DF_EALIGN (g, x, out: 4 bytes; ws: 8 bytes), DF_EWORKSPACE (ws_bytes too small).
 */
#ifndef DEEPFLUIDS_HIP_METRICS_H
#define DEEPFLUIDS_HIP_METRICS_H

#include "deepfluids_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  DF_FM_COUNT = 0,
  DF_FM_DIV_COUNT = 1,
  DF_FM_ARGMAX = 2,
  DF_FM_SUM_ABS = 4,
  DF_FM_SUM_SQ = 5,
  DF_FM_MAX_ABS = 6,
  DF_FM_SUM_ABS_X = 7,
  DF_FM_SUM_SQ_X = 8,
  DF_FM_SUM_ABS_JAC = 9,
  DF_FM_SUM_ABS_DIV_G = 10,
  DF_FM_MAX_ABS_DIV_G = 11,
  DF_FM_SUM_ABS_DIV_X = 12,
  DF_FM_MAX_ABS_DIV_X = 13,
  DF_FM_WORDS = 16
};

int64_t df_field_metrics_workspace_bytes(int dim, int64_t B, int64_t Z, int64_t Y, int64_t X);
int df_field_metrics2d(const float* g, const float* x, const uint8_t* mask, int mask_per_entry, void* out, void* ws, int64_t ws_bytes,
                       int64_t B, int64_t Y, int64_t X, df_stream_t stream);
int df_field_metrics3d(const float* g, const float* x, const uint8_t* mask, int mask_per_entry, void* out, void* ws, int64_t ws_bytes,
                       int64_t B, int64_t Z, int64_t Y, int64_t X, df_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DEEPFLUIDS_HIP_METRICS_H */
