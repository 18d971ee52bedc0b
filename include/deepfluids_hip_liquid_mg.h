/*
 * deepfluids_hip_liquid_mg.h -- C-ABI of libdeepfluids_hip_liquid_mg.so (gfx950 / MI355X only): the multigrid preconditioner of
 * deepfluids_hip.h ("multigrid preconditioner") for the three liquid systems -- the free-surface projection, the ghost-fluid
 * projection and the implicit velocity diffusion.  Opt-in: nothing of deepfluids_hip.h calls it.
 *
 * What `ops.solve_pressure_liquid(preconditioner=)`, `ops.diffuse_velocity(preconditioner=)`, `ops.liquid_step` / `ops.simulate_liquid`
 * call, and `ops.multigrid_hierarchy_liquid` / `ops.multigrid_hierarchy_diffusion`.
 *
 * A library and a header of their own, like deepfluids_hip_metrics.h: deepfluids_hip.h is frozen at DF_VERSION 207.  The library links
 * against libdeepfluids_hip.so and follows every convention of deepfluids_hip.h: device pointers, caller-owned buffers, asynchronous on
 * `stream`, 0 / DF_E* / hipError_t, and the message of a failure is read with df_last_error() of the main library.
 *
 * The definition below is this library's own and it is the one that is tested: tests/liquid_mg_ref.py restates it in fp64 and as an
 * op-for-op fp32 twin whose bits the kernels give.
 *
 * ---- definition --------------------------------------------------------------------------------------------------------------
 * A hierarchy block is the one of deepfluids_hip.h: df_mg_hierarchy_bytes, df_mg_levels, df_mg_level_offset describe it, df_mg_apply and
 * df_pressure_mg_precondition run the V-cycle on it, whatever system built it: a level is the face weights w_a[c] (the face between c
 * and c - e_a), dir[c] and diag[c], and the cycle reads nothing else.  A cell with diag = 0 is inactive.  The two builders below write
 * level 0 and then every coarser level exactly as df_mg_build does (the Galerkin product over aggregates of 2^D children, the sums in
 * ascending x, then y, then z; per coarse cell tot = 0, then tot += (low + high face weight) per axis x, y[, z], diag = tot + dir).
 * All arithmetic fp32, no fused multiply-add, in the order written.
 *
 * df_mg_build_liquid, phi == NULL: the free-surface system of df_pressure_cg_direction*_liquid.
 *   flags    [B,(Z,)Y,X] uint8, the layout of df_liquid_flags*: bit 0 the cell is liquid, bit 1 + 2a / 2 + 2a its low / high neighbour
 *            along axis a is.  A byte is believed only where the cell is interior by its index (bnd <= i_a < extent_a - bnd).
 *   w_a[c] = 1 where c and c - e_a are both liquid (c liquid and its low bit of axis a set), else 0.
 *   dir[c] = the number of neighbours of a liquid cell that are interior by index and not liquid (the air cells, where p = 0), 0 elsewhere.
 *   diag[c] = (the number of liquid neighbours) + dir[c]: the n_c of the `_liquid` direction kernel.  Small integers: exact, as is every
 *            coarser level.  A liquid cell with walls all round has diag = 0 and is inactive.
 * df_mg_build_liquid, phi != NULL: the ghost-fluid system of the `_gf` entry points (phi [B,(Z,)Y,X] fp32, gf_clamp in (0, 1]).
 *   w_a as above.  With t(c, n) = 1/theta of liquid cell c towards its air neighbour n, the function of deepfluids_hip.h ("ghost-fluid"):
 *   dir[c]  = the sum from 0 of t(c, n) over the air neighbours in the order x-, x+, y-, y+[, z-, z+];
 *   diag[c] = the chain of df_pressure_init*_gf: from 0, in the same order over ALL 2D neighbours, + 1 for a liquid one, + t(c, n) for
 *            an air one, nothing for a wall; 1 if the result is not > 0.  On the liquid cells it is bitwise the diag those entry points
 *            write.  Off the liquid w, dir and diag are 0 (the 1 that df_pressure_init*_gf stores there is a divisor, not a row).
 *   The sums are no longer integers and no longer exact; they are fixed-order fp32.
 * df_mg_build_diffusion: (I - alpha L) of df_diffuse_*, on I = the cells interior by index, for the B*D (entry, component) pairs of a
 *   velocity: the hierarchy is one of B*D systems (df_mg_hierarchy_bytes(dim, B*D, ..)), system e*D + a takes alpha[e].
 *   With cnt[c] = the number of the 2D neighbours of c that are in I:
 *   w_a[c] = alpha where c and c - e_a are both in I, else 0;
 *   dir[c] = 1 + alpha * float(2D - cnt[c]);   diag[c] = float(cnt[c]) * alpha + dir[c]   on I;   all 0 off I.
 *   alpha = 0 gives w = 0 and diag = 1.  (df_diffuse_init* leaves r = 0 then: no iteration, the input's bits.)
 *
 * The iteration is the preconditioned one of deepfluids_hip.h with the rows of level 0:
 *   init          df_pressure_init*_flags (free surface), df_pressure_init*_gf (ghost fluid; its workspace), df_diffuse_init*
 *   z = M r       df_pressure_mg_precondition(k = -1), and after every update k (diffusion: with B*D entries)
 *   direction k   df_pressure_cg_direction_mg_rows: the entry's decision exactly as in df_pressure_cg_direction_mg (r.z and max|r| from
 *                 the partials, the stop on the UNscaled max|r| against `accuracy`, `max_iter`, the frozen-entry rule, the state record);
 *                 p = z + beta * p and q[c] = diag[c] * p[c] - sum, the sum from 0 in the order x-, x+, y-, y+[, z-, z+] over the
 *                 neighbours inside the grid, each term w * p[neighbour], at EVERY cell of the entry (on an inactive cell z, w and diag
 *                 are 0, so p and q are); the p.q partials.  One kernel for the three systems: it takes no flags and no boundary width.
 *   update k      df_pressure_cg_update_mg with the flags (both pressure systems); df_diffuse_cg_update_mg for the diffusion, whose x
 *                 lies behind its workspace: the same kernel over the cells interior by index
 *   status, end   df_pressure_status; df_pressure_correct*_liquid / _gf; df_diffuse_finish*
 *
 * Errors, on the host and before any launch: DF_EINVAL (null pointer, dim, bnd, gf_clamp, overlapping arrays, k), DF_ESHAPE (extents),
 * DF_EALIGN, DF_EWORKSPACE (a hierarchy or a workspace too small).
 */
#ifndef DEEPFLUIDS_HIP_LIQUID_MG_H_
#define DEEPFLUIDS_HIP_LIQUID_MG_H_

#include "deepfluids_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int df_mg_build_liquid(void* hierarchy, int64_t hierarchy_bytes, const uint8_t* flags, const float* phi, int dim, int64_t B, int64_t Z, int64_t Y,
                       int64_t X, int bnd, float gf_clamp, df_stream_t stream);
int df_mg_build_diffusion(void* hierarchy, int64_t hierarchy_bytes, const float* alpha, int dim, int64_t B, int64_t Z, int64_t Y, int64_t X,
                          int bnd, df_stream_t stream);
int df_pressure_cg_direction_mg_rows(void* ws, int64_t ws_bytes, void* hierarchy, int64_t hierarchy_bytes, int dim, int64_t B, int64_t Z,
                                     int64_t Y, int64_t X, int64_t k, float accuracy, int64_t max_iter, df_stream_t stream);
int df_diffuse_cg_update_mg(void* ws, int64_t ws_bytes, int dim, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd, int64_t k,
                            df_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
