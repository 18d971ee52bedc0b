/*
 * deepfluids_hip_ssim.h -- C-ABI of libdeepfluids_hip_ssim.so (gfx950 / MI355X only): structural similarity (SSIM) of two image
 * batches, and everything one level of MS-SSIM needs, in ONE fused pass.
 *
 * What `ops.ssim`, `ops.ms_ssim` and `ops.field_ssim` call, and what `Trainer.evaluate_(ssim=True)` sweeps over a data set.  The
 * arithmetic is that of the reference's `ops.ssim` / `ops.ms_ssim` (ops.py:382-501), its quirks restated and not repaired.
 *
 * A library and a header of their own, like deepfluids_hip_metrics.h: deepfluids_hip.h is frozen at DF_VERSION 207.  The library links
 * against libdeepfluids_hip.so and follows every convention of deepfluids_hip.h: device pointers (the ONE exception, `taps`, is named
 * below), caller-owned buffers, asynchronous on `stream`, 0 / DF_E* / hipError_t, and the message of a failure is read with
 * df_last_error() of the main library.
 *
 * ---- definition --------------------------------------------------------------------------------------------------------------
 * a, b      [N,H,W,C] fp32, dense (NHWC), C in 1..4.
 * size      S = min(filter_size, H, W); at most DF_SSIM_MAX_SIZE.  The caller derives sigma = filter_sigma * S / filter_size.
 * taps      HOST memory, S floats, read during the call (they travel as a kernel argument): the normalised 1-D factor of the
 *           reference's `fspecial_gauss(S, sigma, C)`.  With u_i = i - S/2 (integer division) + (0.5 when S is even), i = 0..S-1:
 *           e_i = exp(-u_i^2 / (2 sigma^2)), t_i = e_i / sum_i e_i, all in fp64, each t_i rounded to fp32 once.  There is no exp on
 *           the device.  The reference's window [S,S,C,C] is normalised over ALL its S*S*C*C entries, so it is t_i t_j / C^2 for every
 *           pair of channels: each output channel is 1/C^2 times the sum over the input channels, and the C output channels are equal.
 *           ONE plane is computed for them.
 * per pixel, all fp32, no fused multiply-add, in the order written.  d = max_val - min_val (fp32, on the host):
 *   p_c = (a_c - min_val) / d,  q_c = (b_c - min_val) / d           (IEEE division), c = 0..C-1
 *   the five planes  P0 = sum_c p_c, P1 = sum_c q_c, P2 = sum_c p_c p_c, P3 = sum_c q_c q_c, P4 = sum_c p_c q_c, each sum starting
 *   with its c = 0 term and adding c = 1, 2, 3 in ascending order.
 * filter, a VALID correlation, separable, rows first (H' = H - S + 1, W' = W - S + 1 outputs):
 *   R_k[y][x] = sum_j t_j P_k[y][x + j]   for every row y of the image, then   F_k[y][x] = sum_i t_i R_k[y + i][x];
 *   each sum starts from +0 and adds its products in ascending j (i).
 * per output pixel, with s = fp32(1 / C^2), c1 = k1 * k1, c2 = k2 * k2 (fp32 products of the fp32 arguments; L = 1):
 *   mu1 = F0 s, mu2 = F1 s, e11 = F2 s, e22 = F3 s, e12 = F4 s
 *   mu11 = mu1 mu1, mu22 = mu2 mu2, mu12 = mu1 mu2, s11 = e11 - mu11, s22 = e22 - mu22, s12 = e12 - mu12
 *   v1 = 2 s12 + c2,  v2 = (s11 + s22) + c2
 *   ssim = ((2 mu12 + c1) v1) / (((mu11 + mu22) + c1) v2),   cs = v1 / v2
 * tiles: output tile (ty, tx) of an image holds the output pixels y = 32 ty .. 32 ty + 31, x = 32 tx .. 32 tx + 31 that exist;
 *   there are TY = ceil(H'/32) by TX = ceil(W'/32) of them, numbered ty * TX + tx.  One workgroup of 256 threads computes one tile of
 *   one image (so an image's numbers do not depend on N); thread t owns the pixels x = 32 tx + (t mod 32), y = 32 ty + 4 (t / 32) + i,
 *   i = 0..3.
 * summation order of the ssim and of the cs values (no atomics, nothing depends on scheduling):
 *   1. a thread adds the values of its pixels that exist in ascending i to an fp32 accumulator that starts at 0;
 *   2. the 256 thread sums become fp64 and are added as a tree inside each 64-thread wave: for off = 32, 16, 8, 4, 2, 1 lane l
 *      (l < off) takes v[l] + v[l + off]; then the four wave sums are added in ascending order, ((w0 + w1) + w2) + w3;
 *   3. a second launch, one workgroup per image: thread t adds the tile sums t, t + 256, t + 512, ... in ascending order in fp64 from
 *      0, and the 256 results are added as in 2.: the image's fp64 TOTAL.
 * out       [N, DF_SSIM_WORDS] 32-bit words per image, 8-byte aligned: int32 H' W' at DF_SSIM_COUNT; fp32 mean ssim at
 *           DF_SSIM_MEAN and mean cs at DF_SSIM_MEAN_CS, each fp32(total / fp64(count)); the fp64 totals at words DF_SSIM_SUM and
 *           DF_SSIM_SUM + 1 (ssim) and DF_SSIM_SUM_CS and DF_SSIM_SUM_CS + 1 (cs); word 3 is written as 0.
 * ssim_map, cs_map   NULL, or [N,H',W'] fp32: the two values of every output pixel (the reference's maps have C equal channels).
 * pool_a, pool_b     both NULL, or both [N,PH,PW,C] fp32 with PH = ceil(H/2), PW = ceil(W/2): the 2x2, stride-2 average pool of the RAW
 *           images (before the [0,1] map) with TF's 'SAME' padding, the input of the next MS-SSIM level.  Cell (py, px) holds, per
 *           channel, the sum of the elements (2py, 2px), (2py, 2px+1), (2py+1, 2px), (2py+1, 2px+1) that exist, added in that order
 *           from the first, times 1 / (their number: 4, 2 or 1).  Tile origins are even, so each cell is written by one workgroup: the
 *           one that stages its elements (tile (min(2py/32, TY-1), min(2px/32, TX-1))), from the registers it stages them from.
 * ws        df_ssim_workspace_bytes(N, H, W, filter_size) bytes, 8-byte aligned: the tile sums (16 bytes per tile).  Nothing is read
 *           from it before it is written; -1 for bad extents or a size above DF_SSIM_MAX_SIZE; pure host arithmetic, answers without
 *           a device.
 *
 * df_ssim_group_mean: `out` rows of df_ssim, taken as G groups of M consecutive images -> mean [G,2] fp64 (8-byte aligned):
 *   mean[g][0] = (sum of the M ssim totals) / (M * count), mean[g][1] the same of cs; one workgroup per group, the M totals added
 *   as in step 3 (thread t: images t, t + 256, ...; then the tree).  G = 1, M = N is the mean over a batch (`ops.ssim`, each level of
 *   `ops.ms_ssim`); G = B, M = Z the per-entry mean of a 3-D field folded to B Z images (`ops.field_ssim`).  The count is read from the
 *   group's first image (all images of one call have the same).
 *
 * Errors, on the host and before any launch: DF_EINVAL (null a, b, taps, out, ws or mean; only one of pool_a / pool_b; a non-positive
 * extent; C outside 1..4; filter_size < 1; max_val == min_val or either not finite; any two buffers overlapping where one of them is
 * written), DF_ESHAPE (S > DF_SSIM_MAX_SIZE; H W C >= 2^31; more than 2^31 - 1 workgroups), DF_EALIGN (a, b, maps, pools: 4 bytes;
 * out, ws, mean: 8 bytes), DF_EWORKSPACE (ws_bytes too small).
 */
#ifndef DEEPFLUIDS_HIP_SSIM_H
#define DEEPFLUIDS_HIP_SSIM_H

#include "deepfluids_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  DF_SSIM_COUNT = 0,
  DF_SSIM_MEAN = 1,
  DF_SSIM_MEAN_CS = 2,
  DF_SSIM_SUM = 4,
  DF_SSIM_SUM_CS = 6,
  DF_SSIM_WORDS = 8,
  DF_SSIM_MAX_SIZE = 11,
  DF_SSIM_MAX_CHANNELS = 4,
  DF_SSIM_TILE = 32
};

int64_t df_ssim_workspace_bytes(int64_t N, int64_t H, int64_t W, int filter_size);
int df_ssim(const float* a, const float* b, const float* taps, float* ssim_map, float* cs_map, float* pool_a, float* pool_b, void* out,
            void* ws, int64_t ws_bytes, int64_t N, int64_t H, int64_t W, int C, int filter_size, float k1, float k2, float min_val,
            float max_val, df_stream_t stream);
int df_ssim_group_mean(const void* out, void* mean, int64_t G, int64_t M, df_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DEEPFLUIDS_HIP_SSIM_H */
