// What the multigrid preconditioner of the smoke solve (multigrid.hip) and its liquid and diffusion systems (liquid_mg.hip) share: the
// layout of a hierarchy block, a level's cell decode, the row (A x)[c] of a level, the Galerkin coarsening, and the host-side plan and
// checks.  A level is face weights w_a, dir and diag and nothing else, so everything here is the same for every system.  Every
// translation unit gets its own copy (anonymous namespace) and instantiates only what it launches.
#pragma once
#include "smoke_common.hpp"

namespace {

using df::ceil_div;
using dfadv::apart;
using dfadv::hi_bit;
using dfadv::lo_bit;

constexpr int kMaxLevels = 26;                          // extents < 2^24

struct MgLevel {   // one level, all B entries; every array [B, n]
  float *w[3], *dir, *diag, *r, *xa, *xb;
  int64_t n;
  int nblk, Z, Y, X;
};

struct MgPlan {
  int levels, D;
  int64_t B, floats;
  MgLevel lev[kMaxLevels];
  int64_t off[kMaxLevels][8];                           // float offsets of w[0..2], dir, diag, r, xa, xb inside the block (-1: none)
};

struct MgCell {
  int e, j;
  int64_t cell;
  int p[3];
  bool in;
};

template <int D>
__device__ __forceinline__ void mcoords(const MgLevel& L, int64_t cell, int* p) {
  const int64_t row = cell / L.X;
  p[0] = static_cast<int>(cell - row * L.X);
  p[1] = static_cast<int>(row % L.Y);
  p[2] = D == 3 ? static_cast<int>(row / L.Y) : 0;
}

template <int D>
__device__ __forceinline__ MgCell mdecode(const MgLevel& L) {
  MgCell c;
  c.e = static_cast<int>(blockIdx.x / static_cast<unsigned>(L.nblk));
  c.j = static_cast<int>(blockIdx.x - static_cast<unsigned>(c.e) * static_cast<unsigned>(L.nblk));
  c.cell = static_cast<int64_t>(c.j) * kThreads + threadIdx.x;
  mcoords<D>(L, c.cell, c.p);
  c.in = c.cell < L.n;
  return c;
}

// (A x)[c] = diag[c] x[c] - sum, the sum from 0 in the order x-, x+, y-, y+[, z-, z+] over the neighbours inside the grid, each term
// w * x.  `x(k, a, s)`: the value at cell k, which is c displaced by s along axis a.
template <int D, class F>
__device__ __forceinline__ float mg_Ax(const MgLevel& L, int64_t eo, const int* p, int64_t c, float xc, F x) {
  const int64_t st[3] = {1, L.X, static_cast<int64_t>(L.X) * L.Y};
  const int ext[3] = {L.X, L.Y, L.Z};
  float sum = 0.0f;
#pragma unroll
  for (int a = 0; a < D; ++a) {
    if (p[a] > 0) sum += L.w[a][eo + c] * x(c - st[a], a, -1);
    if (p[a] + 1 < ext[a]) sum += L.w[a][eo + c + st[a]] * x(c + st[a], a, 1);
  }
  return L.diag[eo + c] * xc - sum;
}

// ---- the coarser levels ----------------------------------------------------------------------------------------------------------------------
// the fine faces of axis a with i_a = ia and the other coordinates inside aggregate P, summed in ascending x, then y, then z
template <int D>
__device__ __forceinline__ float mg_face_sum(const MgLevel& F, int64_t eo, const int* P, int a, int ia) {
  const int ext[3] = {F.X, F.Y, F.Z};
  float s = 0.0f;
  for (int dz = 0; dz < (D == 3 ? 2 : 1); ++dz)
    for (int dy = 0; dy < 2; ++dy)
      for (int dx = 0; dx < 2; ++dx) {
        const int d[3] = {dx, dy, dz};
        if (d[a] != 0) continue;
        int q[3] = {2 * P[0] + dx, 2 * P[1] + dy, 2 * P[2] + dz};
        q[a] = ia;
        if (q[0] >= ext[0] || q[1] >= ext[1] || q[2] >= ext[2]) continue;
        s += F.w[a][eo + (static_cast<int64_t>(q[2]) * F.Y + q[1]) * F.X + q[0]];
      }
  return s;
}

// one thread = one coarse cell: its D low-face weights, dir, and diag (the high-face weights are summed again here, not read from the
// thread that owns them: the same sum in the same order, so the same bits; with the counts of the smoke and free-surface systems all of
// it is exact)
template <int D>
__global__ __launch_bounds__(kThreads) void mg_coarsen_kernel(MgLevel F, MgLevel C) {
  const MgCell c = mdecode<D>(C);
  if (!c.in) return;
  const int64_t eoF = static_cast<int64_t>(c.e) * F.n, g = static_cast<int64_t>(c.e) * C.n + c.cell;
  const int ext[3] = {F.X, F.Y, F.Z};
  float tot = 0.0f;
#pragma unroll
  for (int a = 0; a < D; ++a) {
    const float lo = mg_face_sum<D>(F, eoF, c.p, a, 2 * c.p[a]);     // i_a = 0 holds no face: its weights are 0 on every level
    const float hi = 2 * c.p[a] + 2 < ext[a] ? mg_face_sum<D>(F, eoF, c.p, a, 2 * c.p[a] + 2) : 0.0f;
    C.w[a][g] = lo;
    tot += lo + hi;
  }
  float dir = 0.0f;
  for (int dz = 0; dz < (D == 3 ? 2 : 1); ++dz)
    for (int dy = 0; dy < 2; ++dy)
      for (int dx = 0; dx < 2; ++dx) {
        const int q[3] = {2 * c.p[0] + dx, 2 * c.p[1] + dy, 2 * c.p[2] + dz};
        if (q[0] >= ext[0] || q[1] >= ext[1] || q[2] >= ext[2]) continue;
        dir += F.dir[eoF + (static_cast<int64_t>(q[2]) * F.Y + q[1]) * F.X + q[0]];
      }
  C.dir[g] = dir;
  C.diag[g] = tot + dir;
}

// ---- host side (aligned4, check_ws, check_apart: smoke_common.hpp) -----------------------------------------------------------------------------

// the extents the solves accept (check_dims / pplan of smoke.hip), without a boundary width
int mg_dims(const char* fn, int dim, int64_t B, int64_t Z, int64_t Y, int64_t X) {
  DF_REQUIRE(dim == 2 || dim == 3, DF_EINVAL, "%s: dim must be 2 or 3 (got %d)", fn, dim);
  DF_REQUIRE(B > 0 && Z > 0 && Y > 0 && X > 0, DF_EINVAL, "%s: non-positive extent", fn);
  DF_REQUIRE(dim == 3 || Z == 1, DF_EINVAL, "%s: a 2-D grid has Z = 1", fn);
  DF_REQUIRE(B < (1 << 24) && Z < (1 << 24) && Y < (1 << 24) && X < (1 << 24), DF_ESHAPE, "%s: extent too large", fn);
  DF_REQUIRE(X >= 4 && Y >= 4 && (dim == 2 || Z >= 4), DF_ESHAPE, "%s: every extent must be >= 4", fn);
  DF_REQUIRE(Z * Y * X < (1ll << 40) / B, DF_ESHAPE, "%s: extent too large", fn);
  DF_REQUIRE(ceil_div(Z * Y * X, kThreads) * B < (1ll << 31), DF_ESHAPE, "%s: extent too large", fn);
  return DF_OK;
}

// the levels and the layout of the block: level after level, per level D weights, dir, diag, r (level 0: z), xa, xb, each B * n floats
int mg_plan(const char* fn, int dim, int64_t B, int64_t Z, int64_t Y, int64_t X, void* h, MgPlan* p) {
  if (int e = mg_dims(fn, dim, B, Z, Y, X)) return e;
  p->D = dim;
  p->B = B;
  float* f = static_cast<float*>(h);
  int64_t off = 0;
  int l = 0;
  for (;; ++l) {
    MgLevel& L = p->lev[l];
    L.Z = (int)Z; L.Y = (int)Y; L.X = (int)X;
    L.n = Z * Y * X;
    L.nblk = (int)ceil_div(L.n, kThreads);
    const int64_t N = B * L.n;
    float** arr[8] = {&L.w[0], &L.w[1], &L.w[2], &L.dir, &L.diag, &L.r, &L.xa, &L.xb};
    for (int i = 0; i < 8; ++i) {
      const bool none = i == 2 && dim == 2;
      p->off[l][i] = none ? -1 : off;
      *arr[i] = (f && !none) ? f + off : nullptr;
      if (!none) off += N;
    }
    if (X <= 2 && Y <= 2 && Z <= 2) break;
    X = (X + 1) / 2; Y = (Y + 1) / 2; Z = (Z + 1) / 2;
  }
  p->levels = l + 1;
  p->floats = off;
  return DF_OK;
}

int mg_block(const char* fn, int dim, int64_t B, int64_t Z, int64_t Y, int64_t X, void* h, int64_t h_bytes, MgPlan* p) {
  DF_REQUIRE(h, DF_EINVAL, "%s: null hierarchy", fn);
  DF_REQUIRE(aligned4(h), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  if (int e = mg_plan(fn, dim, B, Z, Y, X, h, p)) return e;
  DF_REQUIRE(h_bytes >= 4 * p->floats, DF_EWORKSPACE, "%s: hierarchy of %lld bytes, %lld needed", fn, (long long)h_bytes,
             (long long)(4 * p->floats));
  return DF_OK;
}

unsigned mg_grid(const MgPlan& p, int l) { return static_cast<unsigned>(p.B * p.lev[l].nblk); }

// levels 1.. from level 0, whichever kernel wrote that
template <int D>
void mg_coarsen_all(MgPlan& p, hipStream_t s) {
  for (int l = 1; l < p.levels; ++l)
    hipLaunchKernelGGL((mg_coarsen_kernel<D>), dim3(mg_grid(p, l)), dim3(kThreads), 0, s, p.lev[l - 1], p.lev[l]);
}

// the workspace of the plain solve beside a hierarchy (`h` may be null: none)
int mg_ws(const char* fn, void* ws, int64_t ws_bytes, const MgPlan& p, const void* h, int bnd, PDims* d) {
  const MgLevel& L = p.lev[0];
  *d = PDims{L.n, L.nblk, (int)p.B, L.Z, L.Y, L.X, bnd};
  if (int e = check_ws(fn, ws, ws_bytes, *d)) return e;
  return check_apart(fn, ws, ws_bytes_needed(*d), h, 4 * p.floats, "hierarchy");
}

int mg_bnd_ok(const char* fn, int dim, int64_t Z, int64_t Y, int64_t X, int bnd) {
  DF_REQUIRE(bnd >= 1, DF_EINVAL, "%s: boundary width must be >= 1 (got %d)", fn, bnd);
  const int64_t need = 2 * static_cast<int64_t>(bnd) + 2;
  DF_REQUIRE(X >= need && Y >= need && (dim == 2 || Z >= need), DF_ESHAPE, "%s: every extent must be >= 2*bnd + 2 = %lld", fn, (long long)need);
  return DF_OK;
}

}  // namespace
