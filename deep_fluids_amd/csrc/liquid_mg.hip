// The multigrid preconditioner of multigrid.hip for the three liquid systems -- the free-surface and the ghost-fluid projection and the
// implicit velocity diffusion -- written for gfx950 from the definition in include/deepfluids_hip_liquid_mg.h; tests/liquid_mg_ref.py
// restates it, and its fp32 twin gives the bits of these kernels.  A level of a hierarchy is face weights w_a, dir and diag and the cycle
// reads nothing else, so all that a new system needs is its level 0 and an iteration whose rows are that level 0:
//   level 0       mg_level0_liquid_kernel (the flags byte of df_liquid_flags*, and phi for the ghost-fluid 1/theta: gf_inv_theta, the
//                 function of the `_gf` kernels) and mg_level0_diffusion_kernel (w = alpha on the cells interior by index, one system per
//                 (entry, component) pair); the coarser levels come from mg_coarsen_kernel (multigrid_common.hpp) as they are.
//   direction     cg_direction_rows_kernel: the head of every direction kernel (cg_head), p = z + beta p, and q = A p with the row of
//                 mg_Ax on level 0 -- diag * p - the sum of w * p[neighbour] -- at EVERY cell of the entry: an inactive cell (diag = 0) has
//                 z = 0 and w = 0, so its p and q are 0 and the kernel needs no flags, no boundary width and no system.  11 (2-D) or 15
//                 (3-D) coalesced loads and two stores per cell, no LDS beyond the four words of the reductions.
//   update        cg_update_kernel<kLeaveMg> (smoke_common.hpp) through df_pressure_cg_update_mg of the main library for the pressure
//                 systems; the diffusion's x lies behind its own workspace, which is all df_diffuse_cg_update_mg adds.
//   The cycle itself, the first z and every later one: df_pressure_mg_precondition of the main library, unchanged.
#include "multigrid_common.hpp"

#include "../../include/deepfluids_hip_liquid_mg.h"

namespace {

// Level 0 of the free-surface (GF = false) and the ghost-fluid (GF = true) system.  A flags byte is believed only where the cell is
// interior by its index.  w_a = 1 between two liquid cells.  The air neighbours of a liquid cell are those interior by index and not
// liquid: free surface: dir = their number, diag = liquid neighbours + dir (the n_c of the `_liquid` direction kernel; 0 between walls
// alone: inactive); ghost fluid: dir = the sum from 0 of their 1/theta in the order x-, x+, y-, y+[, z-, z+], and diag the chain of
// pressure_init_gf over the same order (1 per liquid neighbour, 1/theta per air neighbour; 1 if that is not > 0).  Off the liquid all is 0.
template <int D, bool GF>
__global__ __launch_bounds__(kThreads) void mg_level0_liquid_kernel(MgLevel L, const uint8_t* __restrict__ flags, const float* __restrict__ phi,
                                                                    int bnd, float gf_clamp) {
  const MgCell c = mdecode<D>(L);
  if (!c.in) return;
  const int64_t g = static_cast<int64_t>(c.e) * L.n + c.cell;
  const int64_t st[3] = {1, L.X, static_cast<int64_t>(L.X) * L.Y};
  const int ext[3] = {L.X, L.Y, L.Z};
  bool interior = true;
#pragma unroll
  for (int a = 0; a < D; ++a) interior = interior && c.p[a] >= bnd && c.p[a] < ext[a] - bnd;
  const unsigned fl = interior ? flags[g] : 0u;
  const bool liquid = (fl & kFluid) != 0u;
  const float pi = (GF && liquid) ? phi[g] : 0.0f;
  int cnt = 0, air = 0;
  float dir = 0.0f, dg = 0.0f;
#pragma unroll
  for (int a = 0; a < D; ++a) {                           // a liquid cell is interior by its index: both neighbours are inside the entry
    const bool lo = liquid && (fl & lo_bit(a)) != 0u, hi = liquid && (fl & hi_bit(a)) != 0u;
    L.w[a][g] = lo ? 1.0f : 0.0f;
    if (lo) { ++cnt; dg = dg + 1.0f; }
    else if (liquid && c.p[a] > bnd) {
      ++air;
      if (GF) { const float t = gf_inv_theta(pi, phi[g - st[a]], gf_clamp); dir = dir + t; dg = dg + t; }
    }
    if (hi) { ++cnt; dg = dg + 1.0f; }
    else if (liquid && c.p[a] + 1 < ext[a] - bnd) {
      ++air;
      if (GF) { const float t = gf_inv_theta(pi, phi[g + st[a]], gf_clamp); dir = dir + t; dg = dg + t; }
    }
  }
  if (!GF) { dir = static_cast<float>(air); dg = static_cast<float>(cnt + air); }
  else if (liquid && !(dg > 0.0f)) dg = 1.0f;
  L.dir[g] = dir;
  L.diag[g] = dg;
}

// Level 0 of (I - alpha L) on I, the cells interior by index; L.n cells per system, system e = (entry e / D, component e % D).  With cnt
// the neighbours of a cell of I that are in I: w_a = alpha between two cells of I, dir = 1 + alpha * float(2D - cnt),
// diag = float(cnt) * alpha + dir.  Off I all is 0.
template <int D>
__global__ __launch_bounds__(kThreads) void mg_level0_diffusion_kernel(MgLevel L, const float* __restrict__ dalpha, int bnd) {
  const MgCell c = mdecode<D>(L);
  if (!c.in) return;
  const int64_t g = static_cast<int64_t>(c.e) * L.n + c.cell;
  const int ext[3] = {L.X, L.Y, L.Z};
  const float al = dalpha[c.e / D];
  bool interior = true;
#pragma unroll
  for (int a = 0; a < D; ++a) interior = interior && c.p[a] >= bnd && c.p[a] < ext[a] - bnd;
  int cnt = 0;
#pragma unroll
  for (int a = 0; a < D; ++a) {
    const bool lo = interior && c.p[a] > bnd, hi = interior && c.p[a] + 1 < ext[a] - bnd;
    L.w[a][g] = lo ? al : 0.0f;
    cnt += (lo ? 1 : 0) + (hi ? 1 : 0);
  }
  const float dir = interior ? 1.0f + al * static_cast<float>(2 * D - cnt) : 0.0f;
  L.dir[g] = dir;
  L.diag[g] = interior ? static_cast<float>(cnt) * al + dir : 0.0f;
}

// direction(k) of the preconditioned recurrence with the rows of level 0: z = L.r, the cycle's output
template <int D>
__global__ __launch_bounds__(kThreads) void cg_direction_rows_kernel(PWs w, MgLevel L, PDims d, int par, int first, float accuracy,
                                                                     int max_iter) {
  __shared__ float lds[4];
  const PCell c = pdecode<D>(d);
  const CgGo go = cg_head(w, d, c, par, first, accuracy, max_iter, lds);
  if (!go.act) return;
  const float beta = go.beta;
  float pq = 0.0f;
  if (c.cell < d.n) {
    const int64_t eo = static_cast<int64_t>(c.e) * d.n;
    const float* __restrict__ z = L.r + eo;
    const float* __restrict__ po_ = w.p[par] + eo;
    auto pv = [&](int64_t k, int, int) { return z[k] + beta * po_[k]; };
    const float pc = pv(c.cell, 0, 0);
    const float qv = mg_Ax<D>(L, eo, c.p, c.cell, pc, pv);
    w.p[par ^ 1][eo + c.cell] = pc;
    w.q[eo + c.cell] = qv;
    pq = pc * qv;
  }
  pq = block_reduce<false>(pq, lds);
  if (threadIdx.x == 0) w.pq_part[static_cast<int64_t>(c.e) * d.nblk + c.j] = pq;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------
template <int D>
int build_liquid(const char* fn, MgPlan& p, const uint8_t* flags, const float* phi, int bnd, float gf_clamp, hipStream_t s) {
  const dim3 grid(mg_grid(p, 0)), blk(kThreads);
  if (phi) hipLaunchKernelGGL((mg_level0_liquid_kernel<D, true>), grid, blk, 0, s, p.lev[0], flags, phi, bnd, gf_clamp);
  else hipLaunchKernelGGL((mg_level0_liquid_kernel<D, false>), grid, blk, 0, s, p.lev[0], flags, phi, bnd, gf_clamp);
  mg_coarsen_all<D>(p, s);
  return df::launched(fn);
}

template <int D>
int build_diffusion(const char* fn, MgPlan& p, const float* alpha, int bnd, hipStream_t s) {
  hipLaunchKernelGGL((mg_level0_diffusion_kernel<D>), dim3(mg_grid(p, 0)), dim3(kThreads), 0, s, p.lev[0], alpha, bnd);
  mg_coarsen_all<D>(p, s);
  return df::launched(fn);
}

template <int D>
int direction_rows(const char* fn, PWs w, const MgLevel& L, PDims d, int64_t k, float accuracy, int max_iter, hipStream_t s) {
  const dim3 grid(static_cast<unsigned>(static_cast<int64_t>(d.nblk) * d.B)), blk(kThreads);
  hipLaunchKernelGGL((cg_direction_rows_kernel<D>), grid, blk, 0, s, w, L, d, (int)(k & 1), k == 0 ? 1 : 0, accuracy, max_iter);
  return df::launched(fn);
}

// the B entries of a diffusion are B*D systems
int pairs_ok(const char* fn, int dim, int64_t B) {
  DF_REQUIRE(dim == 2 || dim == 3, DF_EINVAL, "%s: dim must be 2 or 3 (got %d)", fn, dim);
  DF_REQUIRE(B > 0 && B < (1 << 24) / dim, B > 0 ? DF_ESHAPE : DF_EINVAL, "%s: %s", fn, B > 0 ? "extent too large" : "non-positive extent");
  return DF_OK;
}

}  // namespace

extern "C" {

int df_mg_build_liquid(void* hierarchy, int64_t hierarchy_bytes, const uint8_t* flags, const float* phi, int dim, int64_t B, int64_t Z, int64_t Y,
                       int64_t X, int bnd, float gf_clamp, df_stream_t stream) {
  const char* fn = "df_mg_build_liquid";
  MgPlan p;
  if (int e = mg_block(fn, dim, B, Z, Y, X, hierarchy, hierarchy_bytes, &p)) return e;
  if (int e = mg_bnd_ok(fn, dim, Z, Y, X, bnd)) return e;
  DF_REQUIRE(flags, DF_EINVAL, "%s: null flags", fn);
  const int64_t n = B * Z * Y * X;
  DF_REQUIRE(apart(flags, n, hierarchy, 4 * p.floats), DF_EINVAL, "%s: the flags overlap the hierarchy", fn);
  if (phi) {
    if (int e = gf_clamp_ok(fn, gf_clamp)) return e;
    DF_REQUIRE(aligned4(phi), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
    DF_REQUIRE(apart(phi, 4 * n, hierarchy, 4 * p.floats), DF_EINVAL, "%s: the level set overlaps the hierarchy", fn);
  }
  hipStream_t s = df::as_stream(stream);
  return dim == 2 ? build_liquid<2>(fn, p, flags, phi, bnd, gf_clamp, s) : build_liquid<3>(fn, p, flags, phi, bnd, gf_clamp, s);
}

int df_mg_build_diffusion(void* hierarchy, int64_t hierarchy_bytes, const float* alpha, int dim, int64_t B, int64_t Z, int64_t Y, int64_t X,
                          int bnd, df_stream_t stream) {
  const char* fn = "df_mg_build_diffusion";
  MgPlan p;
  if (int e = pairs_ok(fn, dim, B)) return e;
  if (int e = mg_block(fn, dim, B * dim, Z, Y, X, hierarchy, hierarchy_bytes, &p)) return e;
  if (int e = mg_bnd_ok(fn, dim, Z, Y, X, bnd)) return e;
  DF_REQUIRE(alpha, DF_EINVAL, "%s: null alpha", fn);
  DF_REQUIRE(aligned4(alpha), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  DF_REQUIRE(apart(alpha, 4 * B, hierarchy, 4 * p.floats), DF_EINVAL, "%s: alpha overlaps the hierarchy", fn);
  hipStream_t s = df::as_stream(stream);
  return dim == 2 ? build_diffusion<2>(fn, p, alpha, bnd, s) : build_diffusion<3>(fn, p, alpha, bnd, s);
}

int df_pressure_cg_direction_mg_rows(void* ws, int64_t ws_bytes, void* hierarchy, int64_t hierarchy_bytes, int dim, int64_t B, int64_t Z,
                                     int64_t Y, int64_t X, int64_t k, float accuracy, int64_t max_iter, df_stream_t stream) {
  const char* fn = "df_pressure_cg_direction_mg_rows";
  MgPlan p;
  PDims d;
  if (int e = mg_block(fn, dim, B, Z, Y, X, hierarchy, hierarchy_bytes, &p)) return e;
  if (int e = mg_ws(fn, ws, ws_bytes, p, hierarchy, 0, &d)) return e;
  if (int e = check_iter(fn, k, accuracy, max_iter)) return e;
  const PWs w = carve(ws, B, d.n, d.nblk);
  hipStream_t s = df::as_stream(stream);
  return dim == 2 ? direction_rows<2>(fn, w, p.lev[0], d, k, accuracy, (int)max_iter, s)
                  : direction_rows<3>(fn, w, p.lev[0], d, k, accuracy, (int)max_iter, s);
}

int df_diffuse_cg_update_mg(void* ws, int64_t ws_bytes, int dim, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd, int64_t k,
                            df_stream_t stream) {
  const char* fn = "df_diffuse_cg_update_mg";
  MgPlan p;
  if (int e = pairs_ok(fn, dim, B)) return e;
  if (int e = mg_plan(fn, dim, B * dim, Z, Y, X, nullptr, &p)) return e;
  if (int e = mg_bnd_ok(fn, dim, Z, Y, X, bnd)) return e;
  const MgLevel& L = p.lev[0];
  const PDims d{L.n, L.nblk, (int)p.B, L.Z, L.Y, L.X, bnd};
  if (int e = check_ws(fn, ws, ws_bytes, d, d.B * d.n)) return e;      // the workspace of df_diffuse_*: the CG's for B*D systems, then x
  DF_REQUIRE(k >= 0, DF_EINVAL, "%s: iteration %lld", fn, (long long)k);
  float* x = static_cast<float*>(ws) + ws_floats(d.B, d.n, d.nblk);
  const PWs w = carve(ws, d.B, d.n, d.nblk);
  const dim3 grid(static_cast<unsigned>(static_cast<int64_t>(d.nblk) * d.B)), blk(kThreads);
  const GfWs none{nullptr, nullptr};
  hipStream_t s = df::as_stream(stream);
  // the unmasked update over the cells interior by index: what df_pressure_cg_update_mg launches without flags
  if (dim == 2) hipLaunchKernelGGL((cg_update_kernel<2, false, kLeaveMg>), grid, blk, 0, s, x, w, none, nullptr, d, (int)(k & 1));
  else hipLaunchKernelGGL((cg_update_kernel<3, false, kLeaveMg>), grid, blk, 0, s, x, w, none, nullptr, d, (int)(k & 1));
  return df::launched(fn);
}

}  // extern "C"
