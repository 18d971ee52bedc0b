// The FLIP half of the reference's liquid scenes (scene/liquid_pos_size.py:254-295, scene/liquid3_d_r.py main(): mapPartsToMAC,
// extrapolateMACFromWeight / extrapolateMACSimple, markFluidCells, addGravity + setWallBcs, flipVelocityUpdate), written for gfx950 from
// the step definition in include/deepfluids_hip.h.  Bit parity with mantaflow is NOT claimed (it cannot be run here);
// tests/liquid_ref.py restates the definition.  The trace, the cell ranges and the pressure solve are those of particles.hip and
// smoke.hip.
//
//   pos, pvel [B,N,D] fp32, sorted by (batch entry, cell); velocity, weight [B,(Z,)Y,X,D] fp32 MAC face values; marks [B,(Z,)Y,X,D] uint8;
//   flags [B,(Z,)Y,X] uint8 in the layout of df_obstacle_flags*; cell (i,j,k) = [..,k,j,i].
//
//   p2g          the transpose of u(p) written as a gather: one thread = one cell and its D face components.  It walks the particles of
//                the 3^D cells around it in ascending cell order -- the cells of one row are consecutive keys, so 3^(D-1) contiguous
//                ranges of the sorted arrays -- and forms, per particle, the D weights with which u(p) reads its D faces (0 where it
//                does not).  Neighbouring threads walk overlapping ranges and share their lines through L1/L2; no LDS, no atomics: the
//                order of every sum is fixed by the extents and the particles alone.  This is the one kernel with real work per thread.
//   extrapolate  one layer per launch, from one (velocity, marks) pair into another: a thread reads its own D components and marks and
//                those of its 2D axis neighbours.  Nothing is written that the launch reads.
//   flags        cell_start -> the flags byte (and, if asked for, the "face touches a liquid cell" marks of the second extrapolation).
//   forces       element-wise: wall faces 0, faces of a liquid cell += force.
//   flip_update  one thread = one particle: two MAC samples at the particle and the blend.
//
// Arithmetic is written in the order of the step definition and the library is built with -ffp-contract=off.  The indices read from
// device memory (cell_start) are clamped before use, and a flags byte is believed only where the cell is interior by its index.
#include <cmath>

#include "advect_common.hpp"
#include "df_common.hpp"
#include "particles_common.hpp"
#include "stencil_common.hpp"

namespace {

using df::ceil_div;
using dfadv::AdvDims;
using dfadv::apart;
using dfadv::Cell;
using dfadv::decode;
using dfadv::hi_bit;
using dfadv::kFluid;
using dfadv::lo_bit;
using dfpart::aligned4;
using dfpart::axis_weights;
using dfpart::mac_sample;
using dfpart::PartDims;
using dfpart::Rec;
using dfst::kThreads;
using dfst::xcd_block;

template <int D>
struct Marks { uint8_t m[D]; };

// ---- particles to grid -----------------------------------------------------------------------------------------------------------------------
struct P2gDims {
  int64_t ncell;   // B*Z*Y*X
  int64_t total;   // B*N
  int Z, Y, X;
};

// the weight with which an axis interpolation (n; s0, s1) reads index t
__device__ __forceinline__ float reach(int n, float s0, float s1, int t) { return n == t ? s0 : (n + 1 == t ? s1 : 0.0f); }

template <int D>
__global__ __launch_bounds__(kThreads) void p2g_kernel(const float* __restrict__ pos, const float* __restrict__ pvel,
                                                       const int32_t* __restrict__ cell_start, float* __restrict__ vel,
                                                       float* __restrict__ weight, uint8_t* __restrict__ known, P2gDims d) {
  const int64_t idx = xcd_block(blockIdx.x, gridDim.x, 0) * kThreads + threadIdx.x;
  if (idx >= d.ncell) return;
  float num[D], den[D];
#pragma unroll
  for (int a = 0; a < D; ++a) num[a] = den[a] = 0.0f;
  if (d.total > 0) {
    const int64_t row = idx / d.X;
    const int i = static_cast<int>(idx - row * d.X);
    const int64_t slab = row / d.Y;                       // b*Z + k
    const int j = static_cast<int>(row - slab * d.Y);
    const int k = D == 3 ? static_cast<int>(slab % d.Z) : 0;
    const int64_t base = idx - ((static_cast<int64_t>(k) * d.Y + j) * d.X + i);   // key of cell (0,0,0) of this batch entry
    const int own[3] = {i, j, k};
    const int ext[3] = {d.X, d.Y, d.Z};
    const int x0 = max(i - 1, 0), x1 = min(i + 1, d.X - 1);
    const int y0 = max(j - 1, 0), y1 = min(j + 1, d.Y - 1);
    const int z0 = D == 3 ? max(k - 1, 0) : 0, z1 = D == 3 ? min(k + 1, d.Z - 1) : 0;
    const int32_t cap = static_cast<int32_t>(d.total);
    for (int z = z0; z <= z1; ++z)
      for (int y = y0; y <= y1; ++y) {
        const int64_t key = base + (static_cast<int64_t>(z) * d.Y + y) * d.X;
        const int32_t s = min(max(cell_start[key + x0], 0), cap);
        const int32_t e = min(max(cell_start[key + x1 + 1], 0), cap);
        for (int32_t p = s; p < e; ++p) {
          const Rec<D> q = *reinterpret_cast<const Rec<D>*>(pos + static_cast<int64_t>(p) * D);
          const Rec<D> u = *reinterpret_cast<const Rec<D>*>(pvel + static_cast<int64_t>(p) * D);
          float wc[3], wf[3];                              // per axis: the weight in the cell-centred frame and in the face frame
#pragma unroll
          for (int b = 0; b < D; ++b) {
            int n;
            float s0, s1;
            axis_weights(q.v[b] - 0.5f, ext[b], n, s0, s1);
            wc[b] = reach(n, s0, s1, own[b]);
            axis_weights(q.v[b], ext[b], n, s0, s1);
            wf[b] = reach(n, s0, s1, own[b]);
          }
#pragma unroll
          for (int a = 0; a < D; ++a) {
            float w = (a == 0 ? wf[0] : wc[0]) * (a == 1 ? wf[1] : wc[1]);
            if (D == 3) w = w * (a == 2 ? wf[2] : wc[2]);
            num[a] = num[a] + w * u.v[a];
            den[a] = den[a] + w;
          }
        }
      }
  }
  Rec<D> v, w;
  Marks<D> m;
#pragma unroll
  for (int a = 0; a < D; ++a) {
    const bool hit = den[a] > 0.0f;
    v.v[a] = hit ? num[a] / den[a] : 0.0f;
    w.v[a] = den[a];
    m.m[a] = hit ? 1 : 0;
  }
  *reinterpret_cast<Rec<D>*>(vel + idx * D) = v;
  *reinterpret_cast<Rec<D>*>(weight + idx * D) = w;
  if (known) *reinterpret_cast<Marks<D>*>(known + idx * D) = m;
}

// ---- extrapolation, one layer ---------------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(kThreads) void extrapolate_kernel(const float* __restrict__ vel, const uint8_t* __restrict__ mark,
                                                               float* __restrict__ vel_out, uint8_t* __restrict__ mark_out, AdvDims d,
                                                               int layer) {
  const int64_t idx = xcd_block(blockIdx.x, gridDim.x, 0) * kThreads + threadIdx.x;
  if (idx >= d.ncell) return;
  const Cell<D> c = decode<D>(idx, d);
  const int64_t st[3] = {1, d.X, static_cast<int64_t>(d.X) * d.Y};
  Rec<D> v = *reinterpret_cast<const Rec<D>*>(vel + idx * D);
  Marks<D> m = *reinterpret_cast<const Marks<D>*>(mark + idx * D);
#pragma unroll
  for (int a = 0; a < D; ++a) {
    // an unknown face between two interior cells; its axis neighbours are inside the grid because c is interior and bnd >= 1
    if (m.m[a] == 0 && c.interior && c.p[a] > d.bnd) {
      float sum = 0.0f;
      int cnt = 0;
#pragma unroll
      for (int b = 0; b < D; ++b) {
#pragma unroll
        for (int sgn = -1; sgn <= 1; sgn += 2) {
          const int64_t nb = (idx + sgn * st[b]) * D + a;
          const int mk = mark[nb];
          if (mk >= 1 && mk <= layer) { sum = sum + vel[nb]; ++cnt; }
        }
      }
      if (cnt > 0) {
        v.v[a] = sum / static_cast<float>(cnt);
        m.m[a] = static_cast<uint8_t>(layer + 1);
      }
    }
  }
  *reinterpret_cast<Rec<D>*>(vel_out + idx * D) = v;
  *reinterpret_cast<Marks<D>*>(mark_out + idx * D) = m;
}

// ---- liquid flags ------------------------------------------------------------------------------------------------------------------------------
// the byte of obstacle_flags_kernel with "no obstacle" read as "the cell's particle range is not empty"
template <int D>
__global__ __launch_bounds__(kThreads) void liquid_flags_kernel(const int32_t* __restrict__ cell_start, uint8_t* __restrict__ flags,
                                                                uint8_t* __restrict__ touch, AdvDims d, int has_particles) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (idx >= d.ncell) return;
  const Cell<D> c = decode<D>(idx, d);
  const int64_t st[3] = {1, d.X, static_cast<int64_t>(d.X) * d.Y};
  const int ext[3] = {d.X, d.Y, d.Z};
  bool in[3] = {true, true, true};
#pragma unroll
  for (int a = 0; a < D; ++a) in[a] = c.p[a] >= d.bnd && c.p[a] < ext[a] - d.bnd;
  unsigned f = 0u;
  if (has_particles) {
    if (c.interior && cell_start[idx + 1] > cell_start[idx]) f = kFluid;
#pragma unroll
    for (int a = 0; a < D; ++a) {
      bool rest = true;                                   // the neighbours along a share the cell's other coordinates
#pragma unroll
      for (int b = 0; b < D; ++b) if (b != a) rest = rest && in[b];
      // bnd >= 1: a neighbour whose index passes the interior test is inside the grid
      if (rest && c.p[a] - 1 >= d.bnd && c.p[a] - 1 < ext[a] - d.bnd && cell_start[idx - st[a] + 1] > cell_start[idx - st[a]]) f |= lo_bit(a);
      if (rest && c.p[a] + 1 >= d.bnd && c.p[a] + 1 < ext[a] - d.bnd && cell_start[idx + st[a] + 1] > cell_start[idx + st[a]]) f |= hi_bit(a);
    }
  }
  flags[idx] = static_cast<uint8_t>(f);
  if (touch) {
    Marks<D> m;
#pragma unroll
    for (int a = 0; a < D; ++a) m.m[a] = ((f & kFluid) || (f & lo_bit(a))) ? 1 : 0;
    *reinterpret_cast<Marks<D>*>(touch + idx * D) = m;
  }
}

// ---- gravity and walls -----------------------------------------------------------------------------------------------------------------------
struct Force { float f[3]; };

template <int D>
__global__ __launch_bounds__(kThreads) void liquid_forces_kernel(const float* vel, const uint8_t* __restrict__ flags, float* out, Force force,
                                                                 AdvDims d) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (idx >= d.ncell) return;
  const Cell<D> c = decode<D>(idx, d);
  const unsigned fl = c.interior ? flags[idx] : 0u;
  const Rec<D> v = *reinterpret_cast<const Rec<D>*>(vel + idx * D);
  Rec<D> r;
#pragma unroll
  for (int a = 0; a < D; ++a) {
    r.v[a] = 0.0f;
    if (c.interior && c.p[a] > d.bnd) r.v[a] = ((fl & kFluid) || (fl & lo_bit(a))) ? v.v[a] + force.f[a] : v.v[a];
  }
  *reinterpret_cast<Rec<D>*>(out + idx * D) = r;
}

// ---- FLIP update -------------------------------------------------------------------------------------------------------------------------------
// RAGGED: the entry of a row is found in entry_start [nb + 1] instead of idx / N; an unused row is neither read nor written
template <int D, bool RAGGED>
__global__ __launch_bounds__(kThreads) void flip_update_kernel(const float* __restrict__ pos, const float* pvel_in, float* pvel_out,
                                                               const float* __restrict__ vel, const float* __restrict__ vel_old, PartDims d,
                                                               float flip, float pic, const int32_t* __restrict__ entry_start, int nb) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (idx >= d.total) return;
  int64_t entry = 0;
  if (RAGGED) {
    entry = dfpart::ragged_entry(entry_start, nb, idx);
    if (entry < 0) return;
  } else {
    entry = idx / d.N;
  }
  const int64_t eo = entry * d.ncell * D;
  const Rec<D> p = *reinterpret_cast<const Rec<D>*>(pos + idx * D);
  const Rec<D> own = *reinterpret_cast<const Rec<D>*>(pvel_in + idx * D);
  float un[D], uo[D];
  mac_sample<D>(vel + eo, p.v, d, un);
  mac_sample<D>(vel_old + eo, p.v, d, uo);
  Rec<D> out;
#pragma unroll
  for (int a = 0; a < D; ++a) {
    const float diff = un[a] - uo[a];
    out.v[a] = flip * (own.v[a] + diff) + pic * un[a];
  }
  *reinterpret_cast<Rec<D>*>(pvel_out + idx * D) = out;
}

// ---- extrapolateLsSimple, the header's level-set extrapolation ---------------------------------------------------------------------------------
// marks: a cell off the outermost layer of the grid gets 1 where phi > 0 (inside) or phi < 0, else 2 where a face neighbour off the
// outermost layer would get 1, else 0; the outermost layer gets 0.  Mark 1 is a function of phi alone, so both come from one launch.
struct LsDims {
  int64_t n;       // B*Z*Y*X
  int Z, Y, X;
  int inside, layer;
  float direction;
};

template <int D>
__device__ __forceinline__ bool ls_inner(int64_t idx, const LsDims& d, int* p) {
  const int64_t row = idx / d.X;
  p[0] = static_cast<int>(idx - row * d.X);
  const int64_t slab = row / d.Y;
  p[1] = static_cast<int>(row - slab * d.Y);
  p[2] = D == 3 ? static_cast<int>(slab % d.Z) : 0;
  const int ext[3] = {d.X, d.Y, d.Z};
  bool inner = true;
#pragma unroll
  for (int a = 0; a < D; ++a) inner = inner && p[a] >= 1 && p[a] + 1 < ext[a];
  return inner;
}

__device__ __forceinline__ bool ls_source(float v, int inside) { return inside ? v > 0.0f : v < 0.0f; }

template <int D>
__global__ __launch_bounds__(kThreads) void levelset_marks_kernel(const float* __restrict__ phi, uint8_t* __restrict__ mark, LsDims d) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (idx >= d.n) return;
  int p[3];
  const int ext[3] = {d.X, d.Y, d.Z};
  const int64_t st[3] = {1, d.X, static_cast<int64_t>(d.X) * d.Y};
  unsigned m = 0u;
  if (ls_inner<D>(idx, d, p)) {                             // all 2D neighbours are inside the entry
    if (ls_source(phi[idx], d.inside)) {
      m = 1u;
    } else {
#pragma unroll
      for (int a = 0; a < D; ++a) {
        if (p[a] - 1 >= 1 && ls_source(phi[idx - st[a]], d.inside)) m = 2u;
        if (p[a] + 2 < ext[a] && ls_source(phi[idx + st[a]], d.inside)) m = 2u;
      }
    }
  }
  mark[idx] = static_cast<uint8_t>(m);
}

// One layer, IN PLACE: a cell with mark 0 off the outermost layer reads the phi of its neighbours marked `layer` and writes its own phi
// and the mark layer + 1.  A launch writes cells marked 0 only and reads the phi of cells marked `layer` >= 2 only; a mark read while
// its owner writes it is 0 or layer + 1, never `layer`: no value read depends on the order of the threads.  (No __restrict__ here.)
template <int D>
__global__ __launch_bounds__(kThreads) void levelset_layer_kernel(float* phi, uint8_t* mark, LsDims d) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (idx >= d.n) return;
  int p[3];
  if (!ls_inner<D>(idx, d, p) || mark[idx] != 0) return;
  const int64_t st[3] = {1, d.X, static_cast<int64_t>(d.X) * d.Y};
  float sum = 0.0f;
  int cnt = 0;
#pragma unroll
  for (int a = 0; a < D; ++a) {
#pragma unroll
    for (int sgn = -1; sgn <= 1; sgn += 2) {
      const int64_t nb = idx + sgn * st[a];
      if (mark[nb] == d.layer) { sum = sum + phi[nb]; ++cnt; }
    }
  }
  if (cnt > 0) {
    phi[idx] = sum / static_cast<float>(cnt) + d.direction;
    mark[idx] = static_cast<uint8_t>(d.layer + 1);
  }
}

// ---- adjustNumber, the header's resampling -----------------------------------------------------------------------------------------------------
struct ResDims {
  int64_t ncell;   // B*Z*Y*X
  int64_t total;   // the capacity P = B*N rows
  int64_t cells;   // Z*Y*X
  int Z, Y, X;
  int bnd;
  int minp, maxp;
  float surface;   // -2R
  uint32_t seed, step;
};

// the D-linear interpolation of the cell-centred phi of one entry at p: the weights of q = p - 0.5 per axis, along x, then y, then z
template <int D>
__device__ __forceinline__ float phi_sample(const float* __restrict__ phi, const float* p, const ResDims& d) {
  const int ext[3] = {d.X, d.Y, d.Z};
  int n[3] = {0, 0, 0};
  float s0[3], s1[3];
#pragma unroll
  for (int a = 0; a < D; ++a) axis_weights(p[a] - 0.5f, ext[a], n[a], s0[a], s1[a]);
  const int64_t sy = d.X, sz = static_cast<int64_t>(d.X) * d.Y;
  const float* q = phi + (static_cast<int64_t>(n[2]) * d.Y + n[1]) * d.X + n[0];
  const float r00 = s0[0] * q[0] + s1[0] * q[1];
  const float r01 = s0[0] * q[sy] + s1[0] * q[sy + 1];
  float r = s0[1] * r00 + s1[1] * r01;
  if (D == 3) {
    const float r10 = s0[0] * q[sz] + s1[0] * q[sz + 1];
    const float r11 = s0[0] * q[sz + sy] + s1[0] * q[sz + sy + 1];
    const float r1 = s0[1] * r10 + s1[1] * r11;
    r = s0[2] * r + s1[2] * r1;
  }
  return r;
}

// count: one thread = one (entry, cell); it walks the cell's range in sorted order and decides every particle of it
template <int D>
__global__ __launch_bounds__(kThreads) void resample_count_kernel(const float* __restrict__ pos, const int32_t* __restrict__ cell_start,
                                                                  const float* __restrict__ phi, const uint8_t* __restrict__ flags,
                                                                  uint8_t* __restrict__ keep, int32_t* __restrict__ kept,
                                                                  int32_t* __restrict__ seeds, ResDims d) {
  const int64_t idx = xcd_block(blockIdx.x, gridDim.x, 0) * kThreads + threadIdx.x;
  if (idx >= d.ncell) return;
  const int64_t entry = idx / d.cells;
  const float* pe = phi + entry * d.cells;
  const int32_t cap = static_cast<int32_t>(d.total);
  const int32_t s = min(max(cell_start[idx], 0), cap);
  const int32_t e = min(max(cell_start[idx + 1], 0), cap);
  int32_t k = 0;
  for (int32_t p = s; p < e; ++p) {
    const Rec<D> q = *reinterpret_cast<const Rec<D>*>(pos + static_cast<int64_t>(p) * D);
    const float phiv = phi_sample<D>(pe, q.v, d);
    const bool drop = phiv > 0.0f || (k > d.maxp && phiv <= d.surface);
    keep[p] = drop ? 0 : 1;
    k += drop ? 0 : 1;
  }
  // the cell's own indices, for "interior": a flags byte is believed only there
  const int64_t row = idx / d.X;
  const int i = static_cast<int>(idx - row * d.X);
  const int64_t slab = row / d.Y;
  const int j = static_cast<int>(row - slab * d.Y);
  const int kz = D == 3 ? static_cast<int>(slab % d.Z) : 0;
  const bool interior = i >= d.bnd && i < d.X - d.bnd && j >= d.bnd && j < d.Y - d.bnd && (D == 2 || (kz >= d.bnd && kz < d.Z - d.bnd));
  const bool deep = interior && (flags[idx] & kFluid) && phi[idx] <= d.surface;
  kept[idx] = k;
  seeds[idx] = (deep && k < d.minp) ? d.minp - k : 0;
}

// scatter: one thread = one (entry, cell); the kept particles of its range, in order, then its seeds.  No row >= total is written.
template <int D>
__global__ __launch_bounds__(kThreads) void resample_scatter_kernel(const float* __restrict__ pos, const float* __restrict__ pvel,
                                                                    const int32_t* __restrict__ cell_start, const uint8_t* __restrict__ keep,
                                                                    const int32_t* __restrict__ seeds, const int32_t* __restrict__ new_start,
                                                                    const float* __restrict__ vel, float* __restrict__ pos_out,
                                                                    float* __restrict__ pvel_out, ResDims d, PartDims pd) {
  const int64_t idx = xcd_block(blockIdx.x, gridDim.x, 0) * kThreads + threadIdx.x;
  if (idx >= d.ncell) return;
  const int32_t cap = static_cast<int32_t>(d.total);
  const int32_t s = min(max(cell_start[idx], 0), cap);
  const int32_t e = min(max(cell_start[idx + 1], 0), cap);
  int64_t dst = min(max(new_start[idx], 0), cap);
  for (int32_t p = s; p < e; ++p) {
    if (keep[p] && dst < d.total) {
      *reinterpret_cast<Rec<D>*>(pos_out + dst * D) = *reinterpret_cast<const Rec<D>*>(pos + static_cast<int64_t>(p) * D);
      *reinterpret_cast<Rec<D>*>(pvel_out + dst * D) = *reinterpret_cast<const Rec<D>*>(pvel + static_cast<int64_t>(p) * D);
      ++dst;
    }
  }
  const int32_t ns = min(max(seeds[idx], 0), d.minp);
  if (ns == 0) return;
  const int64_t entry = idx / d.cells;
  const int64_t row = idx / d.X;
  const int64_t slab = row / d.Y;
  const int c[3] = {static_cast<int>(idx - row * d.X), static_cast<int>(row - slab * d.Y), D == 3 ? static_cast<int>(slab % d.Z) : 0};
  const float* ve = vel + entry * d.cells * D;
  for (int32_t m = 0; m < ns && dst < d.total; ++m, ++dst) {
    Rec<D> q, u;
#pragma unroll
    for (int a = 0; a < D; ++a) {
      const uint32_t h = dfpart::mix4(d.seed, d.step, static_cast<uint32_t>(idx), static_cast<uint32_t>(m * D + a));
      const float lo = static_cast<float>(c[a]), up = static_cast<float>(c[a] + 1);
      const float v = lo + static_cast<float>(h >> 8) * 5.9604644775390625e-08f;       // 2^-24: a 24-bit uniform in [0, 1)
      // lo + u can round up to lo + 1: the largest float below it instead (c[a] + 1 >= 1 is a positive normal number)
      q.v[a] = v < up ? v : __uint_as_float(__float_as_uint(up) - 1u);
    }
    mac_sample<D>(ve, q.v, pd, u.v);
    *reinterpret_cast<Rec<D>*>(pos_out + dst * D) = q;
    *reinterpret_cast<Rec<D>*>(pvel_out + dst * D) = u;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------
// the cell-per-thread grid over all B*Z*Y*X cells of a solver grid (bnd >= 1)
int plan(const char* fn, int dim, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd, AdvDims* d, unsigned* nblk) {
  DF_REQUIRE(B > 0 && Z > 0 && Y > 0 && X > 0, DF_EINVAL, "%s: non-positive extent", fn);
  DF_REQUIRE(bnd >= 1, DF_EINVAL, "%s: boundary width must be >= 1 (got %d)", fn, bnd);
  DF_REQUIRE(B < (1 << 24) && Z < (1 << 24) && Y < (1 << 24) && X < (1 << 24), DF_ESHAPE, "%s: extent too large", fn);
  const int64_t need = 2 * static_cast<int64_t>(bnd) + 2;
  DF_REQUIRE(X >= need && Y >= need && (dim == 2 || Z >= need), DF_ESHAPE, "%s: every extent must be >= 2*bnd + 2 = %lld", fn,
             (long long)need);
  DF_REQUIRE(Z * Y * X < (1ll << 40) / B, DF_ESHAPE, "%s: extent too large", fn);
  const int64_t n = B * Z * Y * X;
  DF_REQUIRE(ceil_div(n, kThreads) < (1ll << 31), DF_ESHAPE, "%s: extent too large", fn);
  *d = AdvDims{n, (int)Z, (int)Y, (int)X, bnd, 0.0f, 1.0f};
  *nblk = static_cast<unsigned>(ceil_div(n, kThreads));
  return DF_OK;
}

template <int D>
int p2g(const char* fn, const float* pos, const float* pvel, const int32_t* cell_start, float* vel, float* weight, uint8_t* known, int64_t B,
        int64_t N, int64_t Z, int64_t Y, int64_t X, df_stream_t stream) {
  if (int e = dfpart::check_dims(fn, D, B, N, Z, Y, X, true)) return e;
  DF_REQUIRE(vel && weight && (N == 0 || (pos && pvel && cell_start)), DF_EINVAL, "%s: null %s", fn,
             !vel ? "velocity" : !weight ? "weight" : !pos ? "positions" : !pvel ? "particle velocities" : "cell ranges");
  DF_REQUIRE(aligned4(pos) && aligned4(pvel) && aligned4(cell_start) && aligned4(vel) && aligned4(weight), DF_EALIGN,
             "%s: pointers must be 4-byte aligned", fn);
  const int64_t n = B * Z * Y * X;
  DF_REQUIRE(vel != weight, DF_EINVAL, "%s: the weight must not be the velocity", fn);
  DF_REQUIRE(!known || (apart(known, n * D, vel, 4 * n * D) && apart(known, n * D, weight, 4 * n * D)), DF_EINVAL,
             "%s: the marks overlap an output", fn);
  const P2gDims d{n, B * N, (int)Z, (int)Y, (int)X};
  hipLaunchKernelGGL((p2g_kernel<D>), dim3((unsigned)ceil_div(n, kThreads)), dim3(kThreads), 0, df::as_stream(stream), pos, pvel, cell_start, vel,
                     weight, known, d);
  return df::launched(fn);
}

template <int D>
int extrapolate(const char* fn, const float* vel, const uint8_t* mark, float* vel_out, uint8_t* mark_out, int64_t B, int64_t Z, int64_t Y,
                int64_t X, int bnd, int layer, df_stream_t stream) {
  DF_REQUIRE(vel && mark && vel_out && mark_out, DF_EINVAL, "%s: null %s", fn, !vel ? "velocity" : !mark ? "marks" : "output");
  DF_REQUIRE(layer >= 1 && layer <= 254, DF_EINVAL, "%s: layer must be in 1..254 (got %d)", fn, layer);
  AdvDims d;
  unsigned nblk;
  if (int e = plan(fn, D, B, Z, Y, X, bnd, &d, &nblk)) return e;
  const int64_t n = d.ncell * D;
  DF_REQUIRE(vel_out != vel && mark_out != mark, DF_EINVAL, "%s: the output must not be the input (the step gathers)", fn);
  DF_REQUIRE(apart(mark_out, n, vel, 4 * n) && apart(mark_out, n, vel_out, 4 * n) && apart(mark, n, vel_out, 4 * n) &&
             apart(mark, n, mark_out, n) && apart(vel, 4 * n, vel_out, 4 * n), DF_EINVAL, "%s: the outputs overlap an input or each other", fn);
  DF_REQUIRE(aligned4(vel) && aligned4(vel_out), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  hipLaunchKernelGGL((extrapolate_kernel<D>), dim3(nblk), dim3(kThreads), 0, df::as_stream(stream), vel, mark, vel_out, mark_out, d, layer);
  return df::launched(fn);
}

template <int D>
int liquid_flags(const char* fn, const int32_t* cell_start, uint8_t* flags, uint8_t* touch, int64_t B, int64_t N, int64_t Z, int64_t Y,
                 int64_t X, int bnd, df_stream_t stream) {
  if (int e = dfpart::check_dims(fn, D, B, N, Z, Y, X, true)) return e;
  DF_REQUIRE(flags && (N == 0 || cell_start), DF_EINVAL, "%s: null %s", fn, !flags ? "flags" : "cell ranges");
  AdvDims d;
  unsigned nblk;
  if (int e = plan(fn, D, B, Z, Y, X, bnd, &d, &nblk)) return e;
  DF_REQUIRE(aligned4(cell_start), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  DF_REQUIRE(!cell_start || (apart(cell_start, 4 * (d.ncell + 1), flags, d.ncell) && (!touch || apart(cell_start, 4 * (d.ncell + 1), touch, d.ncell * D))),
             DF_EINVAL, "%s: an output overlaps the cell ranges (they are read at a neighbour)", fn);
  DF_REQUIRE(!touch || apart(touch, d.ncell * D, flags, d.ncell), DF_EINVAL, "%s: the marks overlap the flags", fn);
  hipLaunchKernelGGL((liquid_flags_kernel<D>), dim3(nblk), dim3(kThreads), 0, df::as_stream(stream), cell_start, flags, touch, d, N > 0 ? 1 : 0);
  return df::launched(fn);
}

template <int D>
int liquid_forces(const char* fn, const float* vel, const uint8_t* flags, float* out, int64_t B, int64_t Z, int64_t Y, int64_t X, Force f,
                  int bnd, df_stream_t stream) {
  DF_REQUIRE(vel && flags && out, DF_EINVAL, "%s: null %s", fn, !vel ? "velocity" : !flags ? "flags" : "output");
  AdvDims d;
  unsigned nblk;
  if (int e = plan(fn, D, B, Z, Y, X, bnd, &d, &nblk)) return e;
  DF_REQUIRE(apart(flags, d.ncell, out, 4 * d.ncell * D), DF_EINVAL, "%s: the flags overlap the output", fn);
  DF_REQUIRE(aligned4(vel) && aligned4(out), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  hipLaunchKernelGGL((liquid_forces_kernel<D>), dim3(nblk), dim3(kThreads), 0, df::as_stream(stream), vel, flags, out, f, d);
  return df::launched(fn);
}

template <int D>
int flip_update(const char* fn, const float* pos, const float* pvel_in, float* pvel_out, const float* vel, const float* vel_old,
                const int32_t* entry_start, bool ragged, int64_t B, int64_t N, int64_t Z, int64_t Y, int64_t X, float flip_ratio,
                df_stream_t stream) {
  if (int e = dfpart::check_dims(fn, D, B, N, Z, Y, X, ragged)) return e;
  if (int e = dfpart::check_ragged(fn, entry_start, ragged, N)) return e;
  DF_REQUIRE(vel && vel_old && (N == 0 || (pos && pvel_in && pvel_out)), DF_EINVAL, "%s: null %s", fn,
             !vel || !vel_old ? "velocity" : !pos ? "positions" : !pvel_in ? "input" : "output");
  DF_REQUIRE(flip_ratio >= 0.0f && flip_ratio <= 1.0f, DF_EINVAL, "%s: flip_ratio must lie in [0, 1] (got %g)", fn, (double)flip_ratio);
  DF_REQUIRE(aligned4(pos) && aligned4(pvel_in) && aligned4(pvel_out) && aligned4(vel) && aligned4(vel_old), DF_EALIGN,
             "%s: pointers must be 4-byte aligned", fn);
  if (N == 0) return DF_OK;
  DF_REQUIRE(static_cast<const void*>(pvel_out) != static_cast<const void*>(pos), DF_EINVAL, "%s: the output must not be the positions", fn);
  PartDims d = {};
  d.total = B * N; d.N = N; d.ncell = Z * Y * X;
  d.Z = (int)Z; d.Y = (int)Y; d.X = (int)X;
  d.vs = 1.0f;
  const unsigned nblk = static_cast<unsigned>(ceil_div(d.total, kThreads));
  hipStream_t s = df::as_stream(stream);
  const float pic = 1.0f - flip_ratio;
  if (ragged) hipLaunchKernelGGL((flip_update_kernel<D, true>), dim3(nblk), dim3(kThreads), 0, s, pos, pvel_in, pvel_out, vel, vel_old, d, flip_ratio, pic,
                                 entry_start, (int)B);
  else hipLaunchKernelGGL((flip_update_kernel<D, false>), dim3(nblk), dim3(kThreads), 0, s, pos, pvel_in, pvel_out, vel, vel_old, d, flip_ratio, pic,
                          entry_start, 0);
  return df::launched(fn);
}

template <int D>
int ls_dims(const char* fn, int64_t B, int64_t Z, int64_t Y, int64_t X, LsDims* d, unsigned* nblk) {
  if (int e = dfpart::check_dims(fn, D, B, 0, Z, Y, X, false)) return e;
  d->n = B * Z * Y * X;
  d->Z = (int)Z; d->Y = (int)Y; d->X = (int)X;
  *nblk = static_cast<unsigned>(ceil_div(d->n, kThreads));
  return DF_OK;
}

template <int D>
int levelset_marks(const char* fn, const float* phi, uint8_t* mark, int64_t B, int64_t Z, int64_t Y, int64_t X, int inside, df_stream_t stream) {
  DF_REQUIRE(phi && mark, DF_EINVAL, "%s: null %s", fn, !phi ? "phi" : "marks");
  DF_REQUIRE(inside == 0 || inside == 1, DF_EINVAL, "%s: inside must be 0 or 1 (got %d)", fn, inside);
  LsDims d = {};
  unsigned nblk;
  if (int e = ls_dims<D>(fn, B, Z, Y, X, &d, &nblk)) return e;
  DF_REQUIRE(aligned4(phi), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  DF_REQUIRE(apart(mark, d.n, phi, 4 * d.n), DF_EINVAL, "%s: the marks overlap phi", fn);
  d.inside = inside;
  hipLaunchKernelGGL((levelset_marks_kernel<D>), dim3(nblk), dim3(kThreads), 0, df::as_stream(stream), phi, mark, d);
  return df::launched(fn);
}

template <int D>
int levelset_layer(const char* fn, float* phi, uint8_t* mark, int64_t B, int64_t Z, int64_t Y, int64_t X, int inside, int layer,
                   df_stream_t stream) {
  DF_REQUIRE(phi && mark, DF_EINVAL, "%s: null %s", fn, !phi ? "phi" : "marks");
  DF_REQUIRE(inside == 0 || inside == 1, DF_EINVAL, "%s: inside must be 0 or 1 (got %d)", fn, inside);
  DF_REQUIRE(layer >= 2 && layer <= 254, DF_EINVAL, "%s: layer must be in 2..254 (got %d)", fn, layer);
  LsDims d = {};
  unsigned nblk;
  if (int e = ls_dims<D>(fn, B, Z, Y, X, &d, &nblk)) return e;
  DF_REQUIRE(aligned4(phi), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  DF_REQUIRE(apart(mark, d.n, phi, 4 * d.n), DF_EINVAL, "%s: the marks overlap phi", fn);
  d.inside = inside; d.layer = layer;
  d.direction = inside ? -1.0f : 1.0f;
  hipLaunchKernelGGL((levelset_layer_kernel<D>), dim3(nblk), dim3(kThreads), 0, df::as_stream(stream), phi, mark, d);
  return df::launched(fn);
}

template <int D>
int res_dims(const char* fn, int64_t B, int64_t N, int64_t Z, int64_t Y, int64_t X, int bnd, int min_particles, int max_particles, ResDims* d,
             unsigned* nblk) {
  if (int e = dfpart::check_dims(fn, D, B, N, Z, Y, X, true)) return e;
  AdvDims ad;
  if (int e = plan(fn, D, B, Z, Y, X, bnd, &ad, nblk)) return e;
  DF_REQUIRE(min_particles >= 1 && min_particles <= 4096, DF_EINVAL, "%s: min_particles must be in 1..4096 (got %d)", fn, min_particles);
  DF_REQUIRE(max_particles >= min_particles && max_particles <= 8192, DF_EINVAL, "%s: max_particles must be in min_particles..8192 (got %d)", fn,
             max_particles);
  d->ncell = ad.ncell; d->total = B * N; d->cells = Z * Y * X;
  DF_REQUIRE(d->ncell * min_particles <= dfpart::kInt32Max - d->total, DF_ESHAPE, "%s: the resampled total may not fit an int32", fn);
  d->Z = (int)Z; d->Y = (int)Y; d->X = (int)X;
  d->bnd = bnd; d->minp = min_particles; d->maxp = max_particles;
  return DF_OK;
}

template <int D>
int resample_count(const char* fn, const float* pos, const int32_t* cell_start, const float* phi, const uint8_t* flags, uint8_t* keep,
                   int32_t* kept, int32_t* seeds, int64_t B, int64_t N, int64_t Z, int64_t Y, int64_t X, int bnd, int min_particles,
                   int max_particles, float radius_factor, df_stream_t stream) {
  DF_REQUIRE(cell_start && phi && flags && kept && seeds && (N == 0 || (pos && keep)), DF_EINVAL, "%s: null %s", fn,
             !cell_start ? "cell ranges" : !phi ? "phi" : !flags ? "flags" : !kept || !seeds ? "counts" : !pos ? "positions" : "keep bytes");
  DF_REQUIRE(radius_factor >= 0.0f && radius_factor <= 1024.0f, DF_EINVAL, "%s: radius_factor must lie in [0, 1024] (got %g)", fn,
             (double)radius_factor);
  ResDims d = {};
  unsigned nblk;
  if (int e = res_dims<D>(fn, B, N, Z, Y, X, bnd, min_particles, max_particles, &d, &nblk)) return e;
  DF_REQUIRE(aligned4(pos) && aligned4(cell_start) && aligned4(phi) && aligned4(kept) && aligned4(seeds), DF_EALIGN,
             "%s: pointers must be 4-byte aligned", fn);
  DF_REQUIRE(kept != seeds, DF_EINVAL, "%s: the two count arrays are the same", fn);
  const float R = (0.5f * sqrtf(static_cast<float>(D))) * (radius_factor + 0.01f);
  d.surface = -2.0f * R;
  hipLaunchKernelGGL((resample_count_kernel<D>), dim3(nblk), dim3(kThreads), 0, df::as_stream(stream), pos, cell_start, phi, flags, keep, kept, seeds,
                     d);
  return df::launched(fn);
}

template <int D>
int resample_scatter(const char* fn, const float* pos, const float* pvel, const int32_t* cell_start, const uint8_t* keep, const int32_t* seeds,
                     const int32_t* new_start, const float* vel, float* pos_out, float* pvel_out, int64_t B, int64_t N, int64_t Z, int64_t Y,
                     int64_t X, int min_particles, uint32_t seed, uint32_t step, df_stream_t stream) {
  DF_REQUIRE(cell_start && seeds && new_start && vel && (N == 0 || (pos && pvel && keep && pos_out && pvel_out)), DF_EINVAL, "%s: null %s", fn,
             !cell_start || !new_start ? "cell ranges" : !seeds ? "counts" : !vel ? "velocity" : !pos || !pvel ? "input" : !keep ? "keep bytes"
                                                                                                                                 : "output");
  ResDims d = {};
  unsigned nblk;
  if (int e = res_dims<D>(fn, B, N, Z, Y, X, 1, min_particles, min_particles, &d, &nblk)) return e;
  DF_REQUIRE(aligned4(pos) && aligned4(pvel) && aligned4(cell_start) && aligned4(seeds) && aligned4(new_start) && aligned4(vel) &&
             aligned4(pos_out) && aligned4(pvel_out), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  if (N == 0) return DF_OK;
  const int64_t nb = 4 * d.total * D;
  DF_REQUIRE(apart(pos_out, nb, pos, nb) && apart(pos_out, nb, pvel, nb) && apart(pvel_out, nb, pos, nb) && apart(pvel_out, nb, pvel, nb) &&
             apart(pos_out, nb, pvel_out, nb), DF_EINVAL, "%s: the outputs overlap an input or each other (the pass gathers)", fn);
  d.seed = seed; d.step = step;
  PartDims pd = {};
  pd.total = d.total; pd.N = N; pd.ncell = d.cells;
  pd.Z = (int)Z; pd.Y = (int)Y; pd.X = (int)X;
  pd.vs = 1.0f;
  hipLaunchKernelGGL((resample_scatter_kernel<D>), dim3(nblk), dim3(kThreads), 0, df::as_stream(stream), pos, pvel, cell_start, keep, seeds, new_start,
                     vel, pos_out, pvel_out, d, pd);
  return df::launched(fn);
}

}  // namespace

extern "C" {

int df_liquid_p2g2d(const float* pos_sorted, const float* pvel_sorted, const int32_t* cell_start, float* vel, float* weight, uint8_t* known,
                    int64_t B, int64_t N, int64_t Y, int64_t X, df_stream_t stream) {
  return p2g<2>("df_liquid_p2g2d", pos_sorted, pvel_sorted, cell_start, vel, weight, known, B, N, 1, Y, X, stream);
}
int df_liquid_p2g3d(const float* pos_sorted, const float* pvel_sorted, const int32_t* cell_start, float* vel, float* weight, uint8_t* known,
                    int64_t B, int64_t N, int64_t Z, int64_t Y, int64_t X, df_stream_t stream) {
  return p2g<3>("df_liquid_p2g3d", pos_sorted, pvel_sorted, cell_start, vel, weight, known, B, N, Z, Y, X, stream);
}
int df_mac_extrapolate2d(const float* vel, const uint8_t* mark, float* vel_out, uint8_t* mark_out, int64_t B, int64_t Y, int64_t X, int bnd,
                         int layer, df_stream_t stream) {
  return extrapolate<2>("df_mac_extrapolate2d", vel, mark, vel_out, mark_out, B, 1, Y, X, bnd, layer, stream);
}
int df_mac_extrapolate3d(const float* vel, const uint8_t* mark, float* vel_out, uint8_t* mark_out, int64_t B, int64_t Z, int64_t Y, int64_t X,
                         int bnd, int layer, df_stream_t stream) {
  return extrapolate<3>("df_mac_extrapolate3d", vel, mark, vel_out, mark_out, B, Z, Y, X, bnd, layer, stream);
}
int df_liquid_flags2d(const int32_t* cell_start, uint8_t* flags, uint8_t* touch, int64_t B, int64_t N, int64_t Y, int64_t X, int bnd,
                      df_stream_t stream) {
  return liquid_flags<2>("df_liquid_flags2d", cell_start, flags, touch, B, N, 1, Y, X, bnd, stream);
}
int df_liquid_flags3d(const int32_t* cell_start, uint8_t* flags, uint8_t* touch, int64_t B, int64_t N, int64_t Z, int64_t Y, int64_t X,
                      int bnd, df_stream_t stream) {
  return liquid_flags<3>("df_liquid_flags3d", cell_start, flags, touch, B, N, Z, Y, X, bnd, stream);
}
int df_liquid_forces2d(const float* vel, const uint8_t* flags, float* out, int64_t B, int64_t Y, int64_t X, float fx, float fy, int bnd,
                       df_stream_t stream) {
  return liquid_forces<2>("df_liquid_forces2d", vel, flags, out, B, 1, Y, X, Force{{fx, fy, 0.0f}}, bnd, stream);
}
int df_liquid_forces3d(const float* vel, const uint8_t* flags, float* out, int64_t B, int64_t Z, int64_t Y, int64_t X, float fx, float fy,
                       float fz, int bnd, df_stream_t stream) {
  return liquid_forces<3>("df_liquid_forces3d", vel, flags, out, B, Z, Y, X, Force{{fx, fy, fz}}, bnd, stream);
}
int df_flip_update2d(const float* pos, const float* pvel_in, float* pvel_out, const float* vel, const float* vel_old, int64_t B, int64_t N,
                     int64_t Y, int64_t X, float flip_ratio, df_stream_t stream) {
  return flip_update<2>("df_flip_update2d", pos, pvel_in, pvel_out, vel, vel_old, nullptr, false, B, N, 1, Y, X, flip_ratio, stream);
}
int df_flip_update3d(const float* pos, const float* pvel_in, float* pvel_out, const float* vel, const float* vel_old, int64_t B, int64_t N,
                     int64_t Z, int64_t Y, int64_t X, float flip_ratio, df_stream_t stream) {
  return flip_update<3>("df_flip_update3d", pos, pvel_in, pvel_out, vel, vel_old, nullptr, false, B, N, Z, Y, X, flip_ratio, stream);
}

int df_flip_update2d_ragged(const float* pos, const float* pvel_in, float* pvel_out, const float* vel, const float* vel_old,
                            const int32_t* entry_start, int64_t B, int64_t N, int64_t Y, int64_t X, float flip_ratio, df_stream_t stream) {
  return flip_update<2>("df_flip_update2d_ragged", pos, pvel_in, pvel_out, vel, vel_old, entry_start, true, B, N, 1, Y, X, flip_ratio, stream);
}
int df_flip_update3d_ragged(const float* pos, const float* pvel_in, float* pvel_out, const float* vel, const float* vel_old,
                            const int32_t* entry_start, int64_t B, int64_t N, int64_t Z, int64_t Y, int64_t X, float flip_ratio,
                            df_stream_t stream) {
  return flip_update<3>("df_flip_update3d_ragged", pos, pvel_in, pvel_out, vel, vel_old, entry_start, true, B, N, Z, Y, X, flip_ratio, stream);
}
int df_levelset_extrapolate_marks2d(const float* phi, uint8_t* mark, int64_t B, int64_t Y, int64_t X, int inside, df_stream_t stream) {
  return levelset_marks<2>("df_levelset_extrapolate_marks2d", phi, mark, B, 1, Y, X, inside, stream);
}
int df_levelset_extrapolate_marks3d(const float* phi, uint8_t* mark, int64_t B, int64_t Z, int64_t Y, int64_t X, int inside, df_stream_t stream) {
  return levelset_marks<3>("df_levelset_extrapolate_marks3d", phi, mark, B, Z, Y, X, inside, stream);
}
int df_levelset_extrapolate_layer2d(float* phi, uint8_t* mark, int64_t B, int64_t Y, int64_t X, int inside, int layer, df_stream_t stream) {
  return levelset_layer<2>("df_levelset_extrapolate_layer2d", phi, mark, B, 1, Y, X, inside, layer, stream);
}
int df_levelset_extrapolate_layer3d(float* phi, uint8_t* mark, int64_t B, int64_t Z, int64_t Y, int64_t X, int inside, int layer,
                                    df_stream_t stream) {
  return levelset_layer<3>("df_levelset_extrapolate_layer3d", phi, mark, B, Z, Y, X, inside, layer, stream);
}
int df_resample_count2d(const float* pos_sorted, const int32_t* cell_start, const float* phi, const uint8_t* flags, uint8_t* keep, int32_t* kept,
                        int32_t* seeds, int64_t B, int64_t N, int64_t Y, int64_t X, int bnd, int min_particles, int max_particles,
                        float radius_factor, df_stream_t stream) {
  return resample_count<2>("df_resample_count2d", pos_sorted, cell_start, phi, flags, keep, kept, seeds, B, N, 1, Y, X, bnd, min_particles,
                           max_particles, radius_factor, stream);
}
int df_resample_count3d(const float* pos_sorted, const int32_t* cell_start, const float* phi, const uint8_t* flags, uint8_t* keep, int32_t* kept,
                        int32_t* seeds, int64_t B, int64_t N, int64_t Z, int64_t Y, int64_t X, int bnd, int min_particles, int max_particles,
                        float radius_factor, df_stream_t stream) {
  return resample_count<3>("df_resample_count3d", pos_sorted, cell_start, phi, flags, keep, kept, seeds, B, N, Z, Y, X, bnd, min_particles,
                           max_particles, radius_factor, stream);
}
int df_resample_scatter2d(const float* pos_sorted, const float* pvel_sorted, const int32_t* cell_start, const uint8_t* keep, const int32_t* seeds,
                          const int32_t* new_start, const float* vel, float* pos_out, float* pvel_out, int64_t B, int64_t N, int64_t Y,
                          int64_t X, int min_particles, uint32_t seed, uint32_t step, df_stream_t stream) {
  return resample_scatter<2>("df_resample_scatter2d", pos_sorted, pvel_sorted, cell_start, keep, seeds, new_start, vel, pos_out, pvel_out, B, N, 1,
                             Y, X, min_particles, seed, step, stream);
}
int df_resample_scatter3d(const float* pos_sorted, const float* pvel_sorted, const int32_t* cell_start, const uint8_t* keep, const int32_t* seeds,
                          const int32_t* new_start, const float* vel, float* pos_out, float* pvel_out, int64_t B, int64_t N, int64_t Z,
                          int64_t Y, int64_t X, int min_particles, uint32_t seed, uint32_t step, df_stream_t stream) {
  return resample_scatter<3>("df_resample_scatter3d", pos_sorted, pvel_sorted, cell_start, keep, seeds, new_start, vel, pos_out, pvel_out, B, N, Z,
                             Y, X, min_particles, seed, step, stream);
}

}  // extern "C"
