// What the pressure and diffusion solves of smoke.hip and the multigrid-preconditioned solve of multigrid.hip share.  Device: the grid of a
// solve (workgroups that never straddle batch entries), the per-entry state words, the fixed-order reductions, and the conjugate-gradient
// iteration itself: cg_head (the per-entry decision at the top of direction(k)), cg_direction_kernel and cg_update_kernel, one template
// each for the plain, liquid, diffusion, Jacobi (ghost fluid) and multigrid variants.  Host: the carving of the workspace and the argument
// checks every solve entry point makes (workspace, overlap, open_sides, iteration).  Every translation unit gets its own copy (anonymous
// namespace) and instantiates only what it launches.
#pragma once
#include "advect_common.hpp"
#include "df_common.hpp"
#include "stencil_common.hpp"

namespace {

using dfadv::kFluid;
using dfst::kThreads;
using dfst::xcd_block;

struct PDims {
  int64_t n;       // cells of one batch entry
  int nblk;        // workgroups of one batch entry
  int B, Z, Y, X, bnd;
};

struct CgState {   // per batch entry, 32 bytes
  float rr, maxr, alpha, beta, pq;
  int active, iters, pad;
};

struct PCell {
  int64_t cell;    // index inside the entry
  int e;           // batch entry
  int j;           // workgroup inside the entry
  int p[3];
  bool interior;   // MASKED: fluid
  unsigned fl;     // MASKED: the flags byte of a fluid cell, else 0
};

template <int D, bool MASKED = false>
__device__ __forceinline__ PCell pdecode(const PDims& d, const uint8_t* __restrict__ flags = nullptr) {
  PCell c;
  const int64_t logical = xcd_block(blockIdx.x, gridDim.x, 0);
  c.e = static_cast<int>(logical / d.nblk);
  c.j = static_cast<int>(logical - static_cast<int64_t>(c.e) * d.nblk);
  c.cell = static_cast<int64_t>(c.j) * kThreads + threadIdx.x;
  const int64_t row = c.cell / d.X;
  c.p[0] = static_cast<int>(c.cell - row * d.X);
  c.p[1] = static_cast<int>(row % d.Y);
  c.p[2] = D == 3 ? static_cast<int>(row / d.Y) : 0;
  c.interior = c.cell < d.n && c.p[0] >= d.bnd && c.p[0] < d.X - d.bnd && c.p[1] >= d.bnd && c.p[1] < d.Y - d.bnd &&
               (D == 2 || (c.p[2] >= d.bnd && c.p[2] < d.Z - d.bnd));
  c.fl = 0u;
  if (MASKED) {
    if (c.interior) c.fl = flags[static_cast<int64_t>(c.e) * d.n + c.cell];
    c.interior = (c.fl & kFluid) != 0u;
    if (!c.interior) c.fl = 0u;
  }
  return c;
}

// Fixed-order reductions over the workgroup: xor butterfly inside a wave (every lane ends with the same bits: a + b == b + a), then the
// four wave results in ascending order.  Every thread returns the total.  `lds` holds 4 floats and is free again after the call.
template <bool MAX>
__device__ __forceinline__ float block_reduce(float v, float* lds) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const float o = __shfl_xor(v, m);
    v = MAX ? fmaxf(v, o) : v + o;
  }
  __syncthreads();                                      // the previous use of lds is over
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return MAX ? fmaxf(fmaxf(fmaxf(lds[0], lds[1]), lds[2]), lds[3]) : ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// the nblk partials of one entry, combined by every workgroup of the entry in the same order
template <bool MAX>
__device__ __forceinline__ float entry_reduce(const float* __restrict__ part, int nblk, float* lds) {
  float a = 0.0f;
  for (int t = threadIdx.x; t < nblk; t += kThreads) a = MAX ? fmaxf(a, part[t]) : a + part[t];
  return block_reduce<MAX>(a, lds);
}

struct PWs {
  float *r, *p[2], *q, *pq_part, *rr_part, *mx_part;
  CgState* state[2];
};

struct GfWs {   // the two arrays of the Jacobi-preconditioned (ghost-fluid) iteration; null in every other
  float *diag, *z;
};

// ---- the iteration -------------------------------------------------------------------------------------------------------------------------
// The head of direction(k), the same for every variant: the entry's record (state[par], or the first iteration's), its r.r (preconditioned:
// r.z) and max|r| from the partials, the decision and beta = rr / rr_old, and the record of the next launch in state[par ^ 1].  A frozen
// entry carries its record over and touches nothing else.  !act: the workgroup has nothing more to do.
struct CgGo {
  bool act;
  float beta;
};

__device__ __forceinline__ CgGo cg_head(const PWs& w, const PDims& d, const PCell& c, int par, int first, float accuracy, int max_iter,
                                        float* lds) {
  const bool writer = c.j == 0 && threadIdx.x == 0;
  CgState s;
  if (first) s = CgState{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1, 0, 0};
  else s = w.state[par][c.e];
  if (!s.active) {
    if (writer) w.state[par ^ 1][c.e] = s;
    return CgGo{false, 0.0f};
  }
  const int64_t po = static_cast<int64_t>(c.e) * d.nblk;
  const float rr = entry_reduce<false>(w.rr_part + po, d.nblk, lds);
  const float mx = entry_reduce<true>(w.mx_part + po, d.nblk, lds);
  const bool act = mx > accuracy && rr > 0.0f && s.iters < max_iter;
  const float beta = first ? 0.0f : rr / s.rr;          // s.rr > 0: the entry was active
  if (writer) w.state[par ^ 1][c.e] = CgState{rr, mx, s.alpha, act ? beta : s.beta, s.pq, act ? 1 : 0, s.iters + (act ? 1 : 0), 0};
  return CgGo{act, beta};
}

// the row of q = A p at a cell, from n_c (the count of its neighbours), the direction pc there and the sum over its neighbours
enum CgRow {
  kRowCount,     // n_c * pc - sum: the pressure Laplacian
  kRowDiffuse,   // pc + alpha * (2D * pc - sum): I + alpha * Laplacian, the alpha of pair e is coef[e / D]
  kRowDiag,      // diag * pc - sum, diag = coef[cell]: the ghost-fluid rows
};

// p = src + beta * p_old at the cell and at its neighbours, p, q = A p and the workgroup's p.q partial.  src is r (plain, liquid,
// diffusion) or z = M r (Jacobi: r / diag, multigrid: the V-cycle's output); the decision always reads max|r| of the UNscaled residual.
// OPEN: p = 0 in open cells (Dirichlet), so an open neighbour counts in n_c and adds nothing to the sum
// LIQUID (with MASKED; "fluid" reads "liquid"): p = 0 in air cells, so n_c counts every neighbour that is interior by its index, as
// the unmasked path does, while the sums run over the liquid neighbours of the flags byte
// kRowDiffuse (unmasked, closed): the entries are the B*D (entry, component) pairs of a velocity; the sum is the one of the unmasked path
// (the direction is 0 off I)
template <int D, bool MASKED, bool OPEN, bool LIQUID = false, CgRow ROW = kRowCount>
__global__ __launch_bounds__(kThreads) void cg_direction_kernel(PWs w, const float* __restrict__ src, const float* __restrict__ coef,
                                                                const uint8_t* __restrict__ flags, PDims d, int par, int first,
                                                                float accuracy, int max_iter, int os) {
  using dfadv::hi_bit;
  using dfadv::lo_bit;
  using dfadv::open_hi;
  using dfadv::open_lo;
  __shared__ float lds[4];
  const PCell c = pdecode<D, MASKED>(d, flags);
  const CgGo go = cg_head(w, d, c, par, first, accuracy, max_iter, lds);
  if (!go.act) return;
  const float beta = go.beta;
  float pq = 0.0f;
  if (c.interior) {
    const int64_t eo = static_cast<int64_t>(c.e) * d.n;
    const float* __restrict__ r = src + eo;
    const float* __restrict__ po_ = w.p[par] + eo;
    const int64_t st[3] = {1, d.X, static_cast<int64_t>(d.X) * d.Y};
    const int ext[3] = {d.X, d.Y, d.Z};
    const float pc = r[c.cell] + beta * po_[c.cell];
    float sum = 0.0f;
    int cnt = 0;
#pragma unroll
    for (int a = 0; a < D; ++a) {
      const bool lo = MASKED ? (c.fl & lo_bit(a)) != 0u : c.p[a] > d.bnd;
      const bool hi = MASKED ? (c.fl & hi_bit(a)) != 0u : c.p[a] + 1 < ext[a] - d.bnd;
      if (lo) { const int64_t nb = c.cell - st[a]; sum += r[nb] + beta * po_[nb]; if (!MASKED) ++cnt; }
      if (hi) { const int64_t nb = c.cell + st[a]; sum += r[nb] + beta * po_[nb]; if (!MASKED) ++cnt; }
    }
    if (MASKED) cnt = __popc((c.fl >> 1) & ((1u << (2 * D)) - 1u));   // n_c: the neighbour bits of the D axes, those the loop visited
    if (LIQUID) {
      cnt = 0;
#pragma unroll
      for (int a = 0; a < D; ++a) cnt += (c.p[a] > d.bnd ? 1 : 0) + (c.p[a] + 1 < ext[a] - d.bnd ? 1 : 0);
    }
    if (OPEN) {
#pragma unroll
      for (int a = 0; a < D; ++a) cnt += ((c.p[a] == d.bnd && open_lo(os, a)) ? 1 : 0) + ((c.p[a] + 1 == ext[a] - d.bnd && open_hi(os, a)) ? 1 : 0);
    }
    float qv = static_cast<float>(cnt) * pc - sum;
    if (ROW == kRowDiffuse) qv = pc + coef[c.e / D] * (static_cast<float>(2 * D) * pc - sum);
    if (ROW == kRowDiag) qv = coef[eo + c.cell] * pc - sum;
    w.p[par ^ 1][eo + c.cell] = pc;
    w.q[eo + c.cell] = qv;
    pq = pc * qv;
  }
  pq = block_reduce<false>(pq, lds);
  if (threadIdx.x == 0) w.pq_part[static_cast<int64_t>(c.e) * d.nblk + c.j] = pq;
}

// what update(k) leaves for direction(k + 1) beside x and r
enum CgLeave {
  kLeavePlain,    // the r.r and max|r| partials
  kLeaveJacobi,   // z = r / diag beside r, r.z in the `rr` partials, max|r|
  kLeaveMg,       // the max|r| partials alone: z and the r.z partials come from the V-cycle that runs after it
};

// alpha = rr / p.q from the entry's p.q partials (0 unless p.q > 0); x += alpha p, r -= alpha q
template <int D, bool MASKED, CgLeave LEAVE = kLeavePlain>
__global__ __launch_bounds__(kThreads) void cg_update_kernel(float* __restrict__ x, PWs w, GfWs gw, const uint8_t* __restrict__ flags, PDims d,
                                                             int par) {
  __shared__ float lds[4];
  const PCell c = pdecode<D, MASKED>(d, flags);
  CgState* s = w.state[par ^ 1] + c.e;                  // what direction(k) has just written
  if (!s->active) return;
  const float rr_old = s->rr;
  const int64_t po = static_cast<int64_t>(c.e) * d.nblk;
  const float pq = entry_reduce<false>(w.pq_part + po, d.nblk, lds);
  const float alpha = pq > 0.0f ? rr_old / pq : 0.0f;
  if (c.j == 0 && threadIdx.x == 0) { s->alpha = alpha; s->pq = pq; }   // words no workgroup of this launch reads
  float rr = 0.0f, mx = 0.0f;
  if (c.interior) {
    const int64_t g = static_cast<int64_t>(c.e) * d.n + c.cell;
    x[g] = x[g] + alpha * w.p[par ^ 1][g];
    const float rn = w.r[g] - alpha * w.q[g];
    const float zn = LEAVE == kLeaveJacobi ? rn / gw.diag[g] : rn;
    w.r[g] = rn;
    if (LEAVE == kLeaveJacobi) gw.z[g] = zn;
    rr = rn * zn;
    mx = fabsf(rn);
  }
  if (LEAVE != kLeaveMg) rr = block_reduce<false>(rr, lds);
  mx = block_reduce<true>(mx, lds);
  if (threadIdx.x == 0) {
    if (LEAVE != kLeaveMg) w.rr_part[po + c.j] = rr;
    w.mx_part[po + c.j] = mx;
  }
}

// ---- ghost-fluid free surface: what the `_gf` kernels of smoke.hip and the ghost-fluid level 0 of liquid_mg.hip share ---------------------
// theta of liquid cell i (phi pi) and an interior air neighbour (phi pa), as 1/theta: denom = pi - pa; theta = 0.5 if denom > -1e-4,
// else min(max(pi / denom, gf_clamp), 1).  A NaN comes out as gf_clamp.
__device__ __forceinline__ float gf_inv_theta(float pi, float pa, float gf_clamp) {
  const float denom = pi - pa;
  const float theta = denom > -1e-4f ? 0.5f : fminf(fmaxf(pi / denom, gf_clamp), 1.0f);
  return 1.0f / theta;
}

int gf_clamp_ok(const char* fn, float gf_clamp) {
  DF_REQUIRE(gf_clamp > 0.0f && gf_clamp <= 1.0f, DF_EINVAL, "%s: gf_clamp must lie in (0, 1] (got %g)", fn, (double)gf_clamp);
  return DF_OK;
}

// ---- host side: the workspace and the checks every solve entry point makes -------------------------------------------------------------------
int64_t ws_floats(int64_t B, int64_t n, int64_t nblk) { return 4 * B * n + 3 * B * nblk + 2 * B * (int64_t)(sizeof(CgState) / 4); }

PWs carve(void* ws, int64_t B, int64_t n, int64_t nblk) {
  PWs w;
  float* f = static_cast<float*>(ws);
  const int64_t N = B * n, P = B * nblk;
  w.r = f; w.p[0] = f + N; w.p[1] = f + 2 * N; w.q = f + 3 * N;
  w.pq_part = f + 4 * N; w.rr_part = w.pq_part + P; w.mx_part = w.rr_part + P;
  w.state[0] = reinterpret_cast<CgState*>(w.mx_part + P);
  w.state[1] = w.state[0] + B;
  return w;
}

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// the bytes of a solve's workspace: the plain solve's, then `extra_floats` behind it (ghost fluid: diag and z, 2*B*n; diffusion: the
// planar x, B*D*n), so that df_pressure_status finds its words unchanged
int64_t ws_bytes_needed(const PDims& d, int64_t extra_floats = 0) { return 4 * (ws_floats(d.B, d.n, d.nblk) + extra_floats); }

int check_ws(const char* fn, const void* ws, int64_t ws_bytes, const PDims& d, int64_t extra_floats = 0) {
  DF_REQUIRE(ws, DF_EINVAL, "%s: null workspace", fn);
  DF_REQUIRE(aligned4(ws), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  const int64_t need = ws_bytes_needed(d, extra_floats);
  DF_REQUIRE(ws_bytes >= need, DF_EWORKSPACE, "%s: workspace of %lld bytes, %lld needed", fn, (long long)ws_bytes, (long long)need);
  return DF_OK;
}

// the workspace (the `need`ed bytes of it) shares no byte with an array the kernels read or write beside it (`p` may be null: none)
int check_apart(const char* fn, const void* ws, int64_t need, const void* p, int64_t bytes, const char* what) {
  DF_REQUIRE(!p || dfadv::apart(ws, need, p, bytes), DF_EINVAL, "%s: the workspace overlaps the %s", fn, what);
  return DF_OK;
}

// open_sides of an `_open` entry point: bits 0..5, and no z bit in 2-D
int check_open(const char* fn, int dim, int open_sides) {
  DF_REQUIRE(open_sides >= 0 && open_sides <= 63, DF_EINVAL, "%s: open_sides must be in 0..63 (got %d)", fn, open_sides);
  DF_REQUIRE(dim == 3 || open_sides < 16, DF_EINVAL, "%s: open_sides %d opens a z side of a 2-D grid", fn, open_sides);
  return DF_OK;
}

// k, accuracy and max_iter of a direction entry point
int check_iter(const char* fn, int64_t k, float accuracy, int64_t max_iter) {
  DF_REQUIRE(k >= 0 && max_iter >= 0 && max_iter < (1ll << 31), DF_EINVAL, "%s: iteration %lld of at most %lld", fn, (long long)k,
             (long long)max_iter);
  DF_REQUIRE(accuracy >= 0.0f, DF_EINVAL, "%s: accuracy must be >= 0", fn);
  return DF_OK;
}

// The one place that maps `flags` (null: no obstacles) and `open_sides` of the calling entry point to MASKED and OPEN of the host template
// F<D, MASKED, OPEN>; open_sides = 0 takes the closed instantiation (the same bits by construction), which has no trailing open_sides.
#define DF_OPEN_CALL(F, D, ...)                                                                                       \
  (open_sides == 0 ? (flags ? F<D, true, false>(__VA_ARGS__) : F<D, false, false>(__VA_ARGS__))                      \
                   : (flags ? F<D, true, true>(__VA_ARGS__, open_sides) : F<D, false, true>(__VA_ARGS__, open_sides)))

}  // namespace
