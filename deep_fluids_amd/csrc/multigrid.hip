// Multigrid V-cycle preconditioner of the smoke pressure solve, written for gfx950 from the definition in include/deepfluids_hip.h
// ("multigrid preconditioner"); tests/smoke_mg_ref.py restates it, and its fp32 twin gives the bits of these kernels: every pass is a
// pointwise stencil, the sums run in a fixed order, nothing is contracted (-ffp-contract=off) and nothing is reduced across cells.
//
//   hierarchy      one float32 block per hierarchy: per level the face weights w_a[c] (face between c and c - e_a), dir, diag, the
//                  level's right-hand side (level 0: z) and two x buffers, each [B, cells of the level].  Level 0 is the solve's own grid
//                  (band included); its weights are written once by mg_level0_kernel from the flags byte / the index tests / open_sides,
//                  so every level runs the same kernels.  Level l + 1 is the Galerkin product with piecewise-constant aggregates of 2^D
//                  children: one thread per coarse cell gathers, no atomics.  The counts are small integers: exact in float32.
//   V-cycle        four launches per level of more than 1024 cells (and level 0), one thread per cell (restriction: per coarse cell); the
//                  smaller levels all run in ONE launch, mg_small_kernel, one workgroup per batch entry walking them down and up with the
//                  same cell functions (without it a cycle is launch-bound on exactly the jobs that are launch-bound today).  Jacobi
//                  sweeps ping-pong between the two x buffers so that no thread reads a word another thread of the pass writes:
//     presmooth2   two damped-Jacobi sweeps from x = 0 in one launch: the first is (omega r) / diag pointwise, so the second takes its
//                  neighbours' values from r directly.
//     restrict     residual of the children computed on the fly and summed in ascending x, then y, then z.
//     correct_sweep  x + alpha e[parent] formed on the fly at the cell and its neighbours, then one sweep.
//     sweep        one sweep; on level 0 it writes z and the workgroup's r.z partial (the `rr` partials of the solve's workspace).
//                  The coarsest level (every extent <= 2) runs presmooth2 and six sweeps (inside mg_small_kernel).
//   iteration      the solve's own two kernels (smoke_common.hpp) for the preconditioned recurrence: cg_direction_kernel with the plain
//                  rows and the direction built from z (`rr` holds r.z, p = z + beta p), cg_update_kernel<kLeaveMg>, which writes r and
//                  the max|r| partials; z and the r.z partials come from the cycle that runs after it.  Every V-cycle kernel returns at
//                  once for an entry whose CgState::active is 0.
//   The levels are L2 resident at the sizes this is used for; the arrays are planar and every access of a pass is coalesced along x.
//   The layout of the block, a level's row (mg_Ax), the coarsening and the host-side plan live in multigrid_common.hpp (liquid_mg.hip
//   shares them).
#include "multigrid_common.hpp"

namespace {

using dfadv::open_hi;
using dfadv::open_lo;

constexpr float kOmega = 2.0f / 3.0f;
constexpr int kNu = 2;                                  // pre- and post-sweeps; mg_presmooth2 fuses exactly two
constexpr int kCoarsestSweeps = 8;
constexpr int kSmallCells = 1024;                       // levels (above level 0) of at most this many cells run in the one-workgroup kernel
constexpr int kSmallLevels = 12;                        // 1024 cells halve to nothing in at most 11 steps
static_assert(kNu == 2 && kCoarsestSweeps % 2 == 0, "the fused pre-sweep and the ping-pong of the coarsest level");

struct MgSmall {   // the levels of the one-workgroup kernel, finest first
  int count;
  MgLevel lev[kSmallLevels];
};

__device__ __forceinline__ bool mg_idle(const CgState* __restrict__ st, int e) { return st && !st[e].active; }

// one damped-Jacobi sweep at c: x + (omega (r - A x)) / diag, 0 on an inactive cell
template <int D, class F>
__device__ __forceinline__ float mg_jacobi(const MgLevel& L, int64_t eo, const int* p, int64_t c, float rc, float xc, F x) {
  const float dg = L.diag[eo + c];
  if (!(dg > 0.0f)) return 0.0f;
  const float t = rc - mg_Ax<D>(L, eo, p, c, xc, x);
  return xc + (kOmega * t) / dg;
}

// ---- the hierarchy -------------------------------------------------------------------------------------------------------------------------
// level 0 from the solve's own tests: a cell is fluid as pdecode has it (interior by its index, and the flags byte's bit 0 where there are
// flags); w_a = 1 between two fluid cells; dir = the open neighbours of a fluid cell (what OPEN adds to n_c in cg_direction_kernel)
template <int D>
__global__ __launch_bounds__(kThreads) void mg_level0_kernel(MgLevel L, const uint8_t* __restrict__ flags, int bnd, int os) {
  const MgCell c = mdecode<D>(L);
  if (!c.in) return;
  const int64_t g = static_cast<int64_t>(c.e) * L.n + c.cell;
  const int ext[3] = {L.X, L.Y, L.Z};
  bool interior = true;
#pragma unroll
  for (int a = 0; a < D; ++a) interior = interior && c.p[a] >= bnd && c.p[a] < ext[a] - bnd;
  const unsigned fl = (flags && interior) ? flags[g] : 0u;   // a flags byte is only believed where the cell is interior by its index
  const bool fluid = flags ? (fl & kFluid) != 0u : interior;
  int cnt = 0, dir = 0;
#pragma unroll
  for (int a = 0; a < D; ++a) {
    const bool lo = fluid && (flags ? (fl & lo_bit(a)) != 0u : c.p[a] > bnd);
    const bool hi = fluid && (flags ? (fl & hi_bit(a)) != 0u : c.p[a] + 1 < ext[a] - bnd);
    L.w[a][g] = lo ? 1.0f : 0.0f;
    cnt += (lo ? 1 : 0) + (hi ? 1 : 0);
    if (fluid) dir += ((c.p[a] == bnd && open_lo(os, a)) ? 1 : 0) + ((c.p[a] + 1 == ext[a] - bnd && open_hi(os, a)) ? 1 : 0);
  }
  L.dir[g] = static_cast<float>(dir);
  L.diag[g] = static_cast<float>(cnt + dir);
}

// (the coarser levels: mg_coarsen_kernel, multigrid_common.hpp)

// ---- the V-cycle ---------------------------------------------------------------------------------------------------------------------------
// The four passes at one cell (e: batch entry, p: the cell's coordinates); the kernels below run them one cell per thread, and
// mg_small_kernel runs them level after level inside one workgroup.  No __restrict__ here: in mg_small_kernel a pass reads what the
// pass before it wrote.
template <int D>
__device__ __forceinline__ void mg_presmooth2_at(const MgLevel& L, const float* r, float* xout, int e, int64_t cell, const int* p) {
  const int64_t eo = static_cast<int64_t>(e) * L.n;
  const float* re = r + eo;
  const float* dg = L.diag + eo;
  auto x1 = [&](int64_t k, int, int) { return dg[k] > 0.0f ? (kOmega * re[k]) / dg[k] : 0.0f; };
  xout[eo + cell] = mg_jacobi<D>(L, eo, p, cell, re[cell], x1(cell, 0, 0), x1);
}

// at coarse cell `cell` of C: r_coarse = the sum over the children of r - A x (0 on an inactive child)
template <int D>
__device__ __forceinline__ void mg_restrict_at(const MgLevel& F, const MgLevel& C, const float* r, const float* x, int e, int64_t cell,
                                               const int* p) {
  const int64_t eo = static_cast<int64_t>(e) * F.n;
  const float* xe = x + eo;
  const int ext[3] = {F.X, F.Y, F.Z};
  auto xv = [&](int64_t k, int, int) { return xe[k]; };
  float s = 0.0f;
  for (int dz = 0; dz < (D == 3 ? 2 : 1); ++dz)
    for (int dy = 0; dy < 2; ++dy)
      for (int dx = 0; dx < 2; ++dx) {
        const int q[3] = {2 * p[0] + dx, 2 * p[1] + dy, 2 * p[2] + dz};
        if (q[0] >= ext[0] || q[1] >= ext[1] || q[2] >= ext[2]) continue;
        const int64_t k = (static_cast<int64_t>(q[2]) * F.Y + q[1]) * F.X + q[0];
        if (F.diag[eo + k] > 0.0f) s += r[eo + k] - mg_Ax<D>(F, eo, q, k, xe[k], xv);
      }
  C.r[static_cast<int64_t>(e) * C.n + cell] = s;
}

template <int D>
__device__ __forceinline__ void mg_correct_sweep_at(const MgLevel& F, const MgLevel& C, const float* r, const float* xin, const float* ec,
                                                    float* xout, float alpha, int e, int64_t cell, const int* p) {
  const int64_t eo = static_cast<int64_t>(e) * F.n;
  const float* xe = xin + eo;
  const float* ee = ec + static_cast<int64_t>(e) * C.n;
  const float* dg = F.diag + eo;
  auto xc = [&](int64_t k, int a, int s) {
    if (!(dg[k] > 0.0f)) return 0.0f;
    int q[3] = {p[0], p[1], p[2]};
    q[a] += s;
    return xe[k] + alpha * ee[(static_cast<int64_t>(q[2] >> 1) * C.Y + (q[1] >> 1)) * C.X + (q[0] >> 1)];
  };
  xout[eo + cell] = mg_jacobi<D>(F, eo, p, cell, r[eo + cell], xc(cell, 0, 0), xc);
}

// one sweep; returns r * x' of the cell
template <int D>
__device__ __forceinline__ float mg_sweep_at(const MgLevel& L, const float* r, const float* xin, float* xout, int e, int64_t cell, const int* p) {
  const int64_t eo = static_cast<int64_t>(e) * L.n;
  const float* xe = xin + eo;
  auto xv = [&](int64_t k, int, int) { return xe[k]; };
  const float rc = r[eo + cell];
  const float z = mg_jacobi<D>(L, eo, p, cell, rc, xe[cell], xv);
  xout[eo + cell] = z;
  return rc * z;
}

template <int D>
__global__ __launch_bounds__(kThreads) void mg_presmooth2_kernel(MgLevel L, const float* __restrict__ r, float* __restrict__ xout,
                                                                 const CgState* __restrict__ st) {
  const MgCell c = mdecode<D>(L);
  if (mg_idle(st, c.e) || !c.in) return;
  mg_presmooth2_at<D>(L, r, xout, c.e, c.cell, c.p);
}

// one thread = one coarse cell
template <int D>
__global__ __launch_bounds__(kThreads) void mg_restrict_kernel(MgLevel F, MgLevel C, const float* __restrict__ r, const float* __restrict__ x,
                                                               const CgState* __restrict__ st) {
  const MgCell c = mdecode<D>(C);
  if (mg_idle(st, c.e) || !c.in) return;
  mg_restrict_at<D>(F, C, r, x, c.e, c.cell, c.p);
}

template <int D>
__global__ __launch_bounds__(kThreads) void mg_correct_sweep_kernel(MgLevel F, MgLevel C, const float* __restrict__ r,
                                                                    const float* __restrict__ xin, const float* __restrict__ ec,
                                                                    float* __restrict__ xout, float alpha, const CgState* __restrict__ st) {
  const MgCell c = mdecode<D>(F);
  if (mg_idle(st, c.e) || !c.in) return;
  mg_correct_sweep_at<D>(F, C, r, xin, ec, xout, alpha, c.e, c.cell, c.p);
}

// FINAL (level 0): xout is z, and the workgroup's r.z partial goes to rr_part (if there is one)
template <int D, bool FINAL>
__global__ __launch_bounds__(kThreads) void mg_sweep_kernel(MgLevel L, const float* __restrict__ r, const float* __restrict__ xin,
                                                            float* __restrict__ xout, float* __restrict__ rr_part,
                                                            const CgState* __restrict__ st) {
  __shared__ float lds[4];
  const MgCell c = mdecode<D>(L);
  if (mg_idle(st, c.e)) return;
  float rz = 0.0f;
  if (c.in) rz = mg_sweep_at<D>(L, r, xin, xout, c.e, c.cell, c.p);
  if (FINAL) {
    rz = block_reduce<false>(rz, lds);
    if (rr_part && threadIdx.x == 0) rr_part[static_cast<int64_t>(c.e) * L.nblk + c.j] = rz;
  }
}

// Every level of at most kSmallCells cells, down and up, in ONE launch: one workgroup per batch entry walks the levels, the threads stride
// over a level's cells, and a barrier stands between two passes.  The same cell functions in the same order as the per-level kernels,
// so the same bits.  The levels' arrays (a few KiB) stay in global memory: what one pass writes the next reads after __syncthreads(),
// which orders the global accesses of a workgroup (all of its waves share one CU's L1).  The finest of these levels takes its
// right-hand side from lev.r (the restriction above it wrote it) and leaves its result in lev.xa.
#define MG_EACH(L, body)                                                             \
  for (int64_t cell = threadIdx.x; cell < (L).n; cell += kThreads) {                 \
    int p[3];                                                                        \
    mcoords<D>((L), cell, p);                                                        \
    body;                                                                            \
  }                                                                                  \
  __syncthreads();

template <int D>
__global__ __launch_bounds__(kThreads) void mg_small_kernel(MgSmall S, float alpha, const CgState* __restrict__ st) {
  const int e = static_cast<int>(blockIdx.x);
  if (mg_idle(st, e)) return;
  const int last = S.count - 1;
  for (int l = 0; l < last; ++l) {
    const MgLevel& L = S.lev[l];
    const MgLevel& C = S.lev[l + 1];
    MG_EACH(L, mg_presmooth2_at<D>(L, L.r, L.xa, e, cell, p))
    MG_EACH(C, mg_restrict_at<D>(L, C, L.r, L.xa, e, cell, p))
  }
  {
    const MgLevel& L = S.lev[last];
    MG_EACH(L, mg_presmooth2_at<D>(L, L.r, L.xa, e, cell, p))
    float *from = L.xa, *to = L.xb;
    for (int i = 2; i < kCoarsestSweeps; ++i) {         // an even number of them: the result is in xa again
      MG_EACH(L, mg_sweep_at<D>(L, L.r, from, to, e, cell, p))
      float* t = from; from = to; to = t;
    }
  }
  for (int l = last - 1; l >= 0; --l) {
    const MgLevel& L = S.lev[l];
    const MgLevel& C = S.lev[l + 1];
    MG_EACH(L, mg_correct_sweep_at<D>(L, C, L.r, L.xa, C.xa, L.xb, alpha, e, cell, p))
    MG_EACH(L, mg_sweep_at<D>(L, L.r, L.xb, L.xa, e, cell, p))
  }
}
#undef MG_EACH

// ---- host side (aligned4, check_ws, check_apart, check_open, check_iter, DF_OPEN_CALL: smoke_common.hpp; mg_dims, mg_plan, mg_block, mg_grid,
//      mg_coarsen_all, mg_ws, mg_bnd_ok: multigrid_common.hpp)            ------------------------------------------------------------------------

// the first level (above level 0) of at most kSmallCells cells; the coarsest has at most 8, and at most kSmallLevels follow the first
int mg_first_small(const MgPlan& p) {
  int l = 1;
  while (p.lev[l].n > kSmallCells) ++l;
  return l;
}

template <int D>
int mg_build(const char* fn, MgPlan& p, const uint8_t* flags, int bnd, int os, hipStream_t s) {
  hipLaunchKernelGGL((mg_level0_kernel<D>), dim3(mg_grid(p, 0)), dim3(kThreads), 0, s, p.lev[0], flags, bnd, os);
  mg_coarsen_all<D>(p, s);
  return df::launched(fn);
}

// z = M r into lev[0].r; `st`: the state records of a solve (null: every entry runs), `rr_part`: where the r.z partials go (or null)
template <int D>
int mg_vcycle(const char* fn, MgPlan& p, const float* r0, float alpha, const CgState* st, float* rr_part, hipStream_t s) {
  const int last = p.levels - 1;                        // >= 1: every extent of level 0 is >= 4
  const int fs = mg_first_small(p);                     // levels fs..last run in mg_small_kernel; 1 <= fs <= last
  const dim3 blk(kThreads);
  for (int l = 0; l < fs; ++l) {
    MgLevel& L = p.lev[l];
    const float* r = l == 0 ? r0 : L.r;
    hipLaunchKernelGGL((mg_presmooth2_kernel<D>), dim3(mg_grid(p, l)), blk, 0, s, L, r, L.xa, st);
    hipLaunchKernelGGL((mg_restrict_kernel<D>), dim3(mg_grid(p, l + 1)), blk, 0, s, L, p.lev[l + 1], r, L.xa, st);
  }
  {
    MgSmall S;
    S.count = last - fs + 1;
    for (int l = fs; l <= last; ++l) S.lev[l - fs] = p.lev[l];
    hipLaunchKernelGGL((mg_small_kernel<D>), dim3(static_cast<unsigned>(p.B)), blk, 0, s, S, alpha, st);
  }
  for (int l = fs - 1; l >= 0; --l) {
    MgLevel& L = p.lev[l];
    const float* r = l == 0 ? r0 : L.r;
    hipLaunchKernelGGL((mg_correct_sweep_kernel<D>), dim3(mg_grid(p, l)), blk, 0, s, L, p.lev[l + 1], r, L.xa, p.lev[l + 1].xa, L.xb, alpha, st);
    if (l == 0) hipLaunchKernelGGL((mg_sweep_kernel<D, true>), dim3(mg_grid(p, 0)), blk, 0, s, L, r, L.xb, L.r, rr_part, st);
    else hipLaunchKernelGGL((mg_sweep_kernel<D, false>), dim3(mg_grid(p, l)), blk, 0, s, L, r, L.xb, L.xa, nullptr, st);
  }
  return df::launched(fn);
}

int mg_alpha_ok(const char* fn, float alpha) {
  DF_REQUIRE(alpha >= 1.0f && alpha < 2.0f, DF_EINVAL, "%s: alpha must lie in [1, 2) (got %g)", fn, (double)alpha);
  return DF_OK;
}

// the solve's direction kernel (the plain rows) with the direction built from z, the cycle's output, and r.z in the `rr` partials
template <int D, bool MASKED, bool OPEN>
int direction_mg(const char* fn, PWs w, const float* z, const uint8_t* flags, PDims d, int64_t k, float accuracy, int max_iter, hipStream_t s,
                 int os = 0) {
  const dim3 grid(static_cast<unsigned>(static_cast<int64_t>(d.nblk) * d.B)), blk(kThreads);
  hipLaunchKernelGGL((cg_direction_kernel<D, MASKED, OPEN>), grid, blk, 0, s, w, z, nullptr, flags, d, (int)(k & 1), k == 0 ? 1 : 0, accuracy,
                     max_iter, os);
  return df::launched(fn);
}

template <int D>
int update_mg(const char* fn, float* pressure, PWs w, const uint8_t* flags, PDims d, int64_t k, hipStream_t s) {
  const dim3 grid(static_cast<unsigned>(static_cast<int64_t>(d.nblk) * d.B)), blk(kThreads);
  const GfWs none{nullptr, nullptr};
  if (flags) hipLaunchKernelGGL((cg_update_kernel<D, true, kLeaveMg>), grid, blk, 0, s, pressure, w, none, flags, d, (int)(k & 1));
  else hipLaunchKernelGGL((cg_update_kernel<D, false, kLeaveMg>), grid, blk, 0, s, pressure, w, none, flags, d, (int)(k & 1));
  return df::launched(fn);
}

}  // namespace

extern "C" {

int64_t df_mg_hierarchy_bytes(int dim, int64_t B, int64_t Z, int64_t Y, int64_t X) {
  MgPlan p;
  if (mg_plan("df_mg_hierarchy_bytes", dim, B, Z, Y, X, nullptr, &p)) return -1;
  return 4 * p.floats;
}

int df_mg_sweeps(int coarsest) { return coarsest == 0 ? kNu : coarsest == 1 ? kCoarsestSweeps : -1; }

float df_mg_omega(void) { return kOmega; }

int df_mg_cycle_launches(int dim, int64_t Z, int64_t Y, int64_t X) {
  MgPlan p;
  if (mg_plan("df_mg_cycle_launches", dim, 1, Z, Y, X, nullptr, &p)) return -1;
  return 4 * mg_first_small(p) + 1;
}

int df_mg_levels(int dim, int64_t Z, int64_t Y, int64_t X) {
  MgPlan p;
  if (mg_plan("df_mg_levels", dim, 1, Z, Y, X, nullptr, &p)) return -1;
  return p.levels;
}

int64_t df_mg_level_offset(int dim, int64_t B, int64_t Z, int64_t Y, int64_t X, int level, int array) {
  MgPlan p;
  if (mg_plan("df_mg_level_offset", dim, B, Z, Y, X, nullptr, &p)) return -1;
  if (level < 0 || level >= p.levels || array < 0 || array >= dim + 5) return -1;
  return p.off[level][array < dim ? array : array + (3 - dim)];
}

int df_mg_build(void* hierarchy, int64_t hierarchy_bytes, const uint8_t* flags, int dim, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd,
                int open_sides, df_stream_t stream) {
  const char* fn = "df_mg_build";
  MgPlan p;
  if (int e = mg_block(fn, dim, B, Z, Y, X, hierarchy, hierarchy_bytes, &p)) return e;
  if (int e = mg_bnd_ok(fn, dim, Z, Y, X, bnd)) return e;
  if (int e = check_open(fn, dim, open_sides)) return e;
  DF_REQUIRE(!flags || apart(flags, B * Z * Y * X, hierarchy, 4 * p.floats), DF_EINVAL, "%s: the flags overlap the hierarchy", fn);
  return dim == 2 ? mg_build<2>(fn, p, flags, bnd, open_sides, df::as_stream(stream)) : mg_build<3>(fn, p, flags, bnd, open_sides, df::as_stream(stream));
}

int df_mg_apply(void* hierarchy, int64_t hierarchy_bytes, const float* r, int dim, int64_t B, int64_t Z, int64_t Y, int64_t X, float alpha,
                df_stream_t stream) {
  const char* fn = "df_mg_apply";
  MgPlan p;
  if (int e = mg_block(fn, dim, B, Z, Y, X, hierarchy, hierarchy_bytes, &p)) return e;
  if (int e = mg_alpha_ok(fn, alpha)) return e;
  DF_REQUIRE(r, DF_EINVAL, "%s: null r", fn);
  DF_REQUIRE(aligned4(r), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  DF_REQUIRE(apart(r, 4 * B * Z * Y * X, hierarchy, 4 * p.floats), DF_EINVAL, "%s: r overlaps the hierarchy", fn);
  return dim == 2 ? mg_vcycle<2>(fn, p, r, alpha, nullptr, nullptr, df::as_stream(stream))
                  : mg_vcycle<3>(fn, p, r, alpha, nullptr, nullptr, df::as_stream(stream));
}

int df_pressure_mg_precondition(void* hierarchy, int64_t hierarchy_bytes, void* ws, int64_t ws_bytes, int dim, int64_t B, int64_t Z, int64_t Y,
                                int64_t X, float alpha, int64_t k, df_stream_t stream) {
  const char* fn = "df_pressure_mg_precondition";
  MgPlan p;
  PDims d;
  if (int e = mg_block(fn, dim, B, Z, Y, X, hierarchy, hierarchy_bytes, &p)) return e;
  if (int e = mg_alpha_ok(fn, alpha)) return e;
  if (int e = mg_ws(fn, ws, ws_bytes, p, hierarchy, 0, &d)) return e;
  DF_REQUIRE(k >= -1, DF_EINVAL, "%s: iteration %lld", fn, (long long)k);
  const PWs w = carve(ws, B, d.n, d.nblk);
  const CgState* st = k < 0 ? nullptr : w.state[(k & 1) ^ 1];   // the record direction(k) wrote and update(k) read
  return dim == 2 ? mg_vcycle<2>(fn, p, w.r, alpha, st, w.rr_part, df::as_stream(stream))
                  : mg_vcycle<3>(fn, p, w.r, alpha, st, w.rr_part, df::as_stream(stream));
}

int df_pressure_cg_direction_mg(void* ws, int64_t ws_bytes, void* hierarchy, int64_t hierarchy_bytes, const uint8_t* flags, int dim, int64_t B,
                                int64_t Z, int64_t Y, int64_t X, int bnd, int open_sides, int64_t k, float accuracy, int64_t max_iter,
                                df_stream_t stream) {
  const char* fn = "df_pressure_cg_direction_mg";
  MgPlan p;
  PDims d;
  if (int e = mg_block(fn, dim, B, Z, Y, X, hierarchy, hierarchy_bytes, &p)) return e;
  if (int e = mg_bnd_ok(fn, dim, Z, Y, X, bnd)) return e;
  if (int e = check_open(fn, dim, open_sides)) return e;
  if (int e = mg_ws(fn, ws, ws_bytes, p, hierarchy, bnd, &d)) return e;
  if (int e = check_iter(fn, k, accuracy, max_iter)) return e;
  if (int e = check_apart(fn, ws, ws_bytes_needed(d), flags, B * d.n, "flags")) return e;
  const PWs w = carve(ws, B, d.n, d.nblk);
  hipStream_t s = df::as_stream(stream);
  return dim == 2 ? DF_OPEN_CALL(direction_mg, 2, fn, w, p.lev[0].r, flags, d, k, accuracy, (int)max_iter, s)
                  : DF_OPEN_CALL(direction_mg, 3, fn, w, p.lev[0].r, flags, d, k, accuracy, (int)max_iter, s);
}

int df_pressure_cg_update_mg(float* pressure, void* ws, int64_t ws_bytes, const uint8_t* flags, int dim, int64_t B, int64_t Z, int64_t Y,
                             int64_t X, int bnd, int64_t k, df_stream_t stream) {
  const char* fn = "df_pressure_cg_update_mg";
  DF_REQUIRE(pressure, DF_EINVAL, "%s: null pressure", fn);
  MgPlan p;
  PDims d;
  if (int e = mg_plan(fn, dim, B, Z, Y, X, nullptr, &p)) return e;
  if (int e = mg_bnd_ok(fn, dim, Z, Y, X, bnd)) return e;
  if (int e = mg_ws(fn, ws, ws_bytes, p, nullptr, bnd, &d)) return e;
  DF_REQUIRE(k >= 0, DF_EINVAL, "%s: iteration %lld", fn, (long long)k);
  const int64_t need = ws_bytes_needed(d);
  DF_REQUIRE(aligned4(pressure), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  if (int e = check_apart(fn, ws, need, pressure, 4 * B * d.n, "pressure")) return e;
  DF_REQUIRE(!flags || (apart(flags, B * d.n, ws, need) && apart(flags, B * d.n, pressure, 4 * B * d.n)), DF_EINVAL,
             "%s: the flags overlap the workspace or the pressure", fn);
  const PWs w = carve(ws, B, d.n, d.nblk);
  return dim == 2 ? update_mg<2>(fn, pressure, w, flags, d, k, df::as_stream(stream)) : update_mg<3>(fn, pressure, w, flags, d, k, df::as_stream(stream));
}

}  // extern "C"
