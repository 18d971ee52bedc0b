// A liquid carried through a generated velocity field: the `advect()` mode of the reference's liquid scene scripts
// (scene/liquid3_vis.py:47-148, scene/liquid_pos_size.py:47-132), which hand the work to mantaflow: marker particles traced with
// pp.advectInGrid(IntRK4), then gridParticleIndex + unionParticleLevelset.  Written for gfx950 from the step definition in
// include/deepfluids_hip.h; bit parity with mantaflow is NOT claimed (it cannot be run here).
//
//   pos [B,N,D] fp32 in cell units (x, y[, z]); velocity [B,(Z,)Y,X,D] fp32 MAC face values; phi [B,(Z,)Y,X] fp32; cell (i,j,k) =
//   [..,k,j,i].
//
//   trace:    one thread = one particle.  Four MAC samples (RK4), each D multilinear interpolations in the frame of its component;
//             the own record is one 8- or 12-byte load (records are 4-byte aligned), the 2^D corners of every sample are data
//             dependent gathers served by L1/L2 -- neighbouring particles of a seeded body share their lines; no LDS.  pos_out may be
//             pos_in: a thread reads and writes its own record only.
//   keys:     one thread = one particle, key = b*ncell + cell.  The stable sort by key and the per-cell ranges are the caller's.
//   gather:   pos_sorted[r] = pos[order[r]], the permutation the sort returned.
//   levelset: one thread = one cell, threads along x.  Cells of one window row are consecutive keys, so their particles are ONE
//             contiguous range of the sorted array: (2w+1)^(D-1) ranges per cell, and neighbouring threads walk overlapping ranges
//             and share their lines.  A min over particles needs no atomics: the output is deterministic.
//   averaged: the averaged level set of the liquid loops (averagedParticleLevelset, restated from memory; the definition is the header's,
//             parity is with tests/liquid_gf_ref.py, NOT with mantaflow): the same walk with a weight sum and a weighted position sum per
//             cell in ascending order; its smoothing passes and the closing band are one element-wise kernel between two buffers.
//
// Arithmetic is written in the order of the step definition and the library is built with -ffp-contract=off: a NumPy fp32 restatement
// in that order reproduces it.  Float -> int conversions are taken only of values already known to be inside the grid, and the indices
// read from device memory (order, cell_start) are clamped before use: a NaN, a huge velocity or a wrong index selects an edge cell or
// an edge particle, never an address outside the arrays.
#include <cmath>

#include "advect_common.hpp"
#include "df_common.hpp"
#include "particles_common.hpp"
#include "stencil_common.hpp"

namespace {

using df::ceil_div;
using dfpart::aligned4;
using dfpart::check_dims;
using dfpart::kInt32Max;
using dfpart::mac_sample;
using dfpart::PartDims;
using dfpart::ragged_entry;
using dfpart::Rec;
using dfst::kThreads;
using dfst::xcd_block;

// RAGGED: the entry of a row is found in entry_start [nb + 1] instead of idx / N; an unused row is neither read nor written
template <int D, bool RAGGED>
__global__ __launch_bounds__(kThreads) void particles_advect_kernel(const float* pos_in, float* pos_out, const float* __restrict__ vel,
                                                                    PartDims d, const int32_t* __restrict__ entry_start, int nb) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (idx >= d.total) return;
  int64_t entry = 0;
  if (RAGGED) {
    entry = ragged_entry(entry_start, nb, idx);
    if (entry < 0) return;
  } else {
    entry = idx / d.N;
  }
  const float* vb = vel + entry * d.ncell * D;
  const Rec<D> own = *reinterpret_cast<const Rec<D>*>(pos_in + idx * D);
  float k1[D], k2[D], k3[D], k4[D], q[D];
  mac_sample<D>(vb, own.v, d, k1);
#pragma unroll
  for (int a = 0; a < D; ++a) q[a] = own.v[a] + d.half_dt * k1[a];
  mac_sample<D>(vb, q, d, k2);
#pragma unroll
  for (int a = 0; a < D; ++a) q[a] = own.v[a] + d.half_dt * k2[a];
  mac_sample<D>(vb, q, d, k3);
#pragma unroll
  for (int a = 0; a < D; ++a) q[a] = own.v[a] + d.dt * k3[a];
  mac_sample<D>(vb, q, d, k4);
  Rec<D> out;
#pragma unroll
  for (int a = 0; a < D; ++a) {
    const float sum = ((k1[a] + 2.0f * k2[a]) + 2.0f * k3[a]) + k4[a];
    const float moved = own.v[a] + (d.dt * sum) / 6.0f;
    out.v[a] = fminf(fmaxf(moved, d.lo), d.hi[a]);            // a NaN comes out as lo
  }
  *reinterpret_cast<Rec<D>*>(pos_out + idx * D) = out;
}

// cell index along one axis of a position that need not be clamped: < 0 or NaN -> 0, >= ext -> ext - 1
__device__ __forceinline__ int cell_of(float p, int ext) {
  if (!(p >= 0.0f)) return 0;
  if (p >= static_cast<float>(ext)) return ext - 1;
  const int i = static_cast<int>(p);
  return i < ext - 1 ? i : ext - 1;
}

// RAGGED: as above; an unused row gets the key nb * ncell, behind every cell, and its position is not read
template <int D, bool RAGGED>
__global__ __launch_bounds__(kThreads) void particles_keys_kernel(const float* __restrict__ pos, int32_t* __restrict__ keys, PartDims d,
                                                                  const int32_t* __restrict__ entry_start, int nb) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (idx >= d.total) return;
  int64_t entry = 0;
  if (RAGGED) {
    entry = ragged_entry(entry_start, nb, idx);
    if (entry < 0) {
      keys[idx] = static_cast<int32_t>(nb * d.ncell);
      return;
    }
  } else {
    entry = idx / d.N;
  }
  const Rec<D> p = *reinterpret_cast<const Rec<D>*>(pos + idx * D);
  const int i = cell_of(p.v[0], d.X), j = cell_of(p.v[1], d.Y), k = D == 3 ? cell_of(p.v[D - 1], d.Z) : 0;
  keys[idx] = static_cast<int32_t>(entry * d.ncell + ((static_cast<int64_t>(k) * d.Y + j) * d.X + i));
}

template <int D>
__global__ __launch_bounds__(kThreads) void particles_gather_kernel(const float* __restrict__ pos, const int64_t* __restrict__ order,
                                                                    float* __restrict__ out, int64_t n) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (idx >= n) return;
  int64_t src = order[idx];
  src = src < 0 ? 0 : (src >= n ? n - 1 : src);
  *reinterpret_cast<Rec<D>*>(out + idx * D) = *reinterpret_cast<const Rec<D>*>(pos + src * D);
}

struct PhiDims {
  int64_t nphi;    // B*Z*Y*X
  int64_t total;   // B*N
  int Z, Y, X;
  int w;
  float radius;
};

template <int D>
__global__ __launch_bounds__(kThreads) void levelset_union_kernel(const float* __restrict__ pos, const int32_t* __restrict__ cell_start,
                                                                  float* __restrict__ phi, PhiDims d) {
  const int64_t idx = xcd_block(blockIdx.x, gridDim.x, 0) * kThreads + threadIdx.x;
  if (idx >= d.nphi) return;
  float r = d.radius;
  if (d.total > 0) {
    const int64_t row = idx / d.X;
    const int i = static_cast<int>(idx - row * d.X);
    const int64_t slab = row / d.Y;                       // b*Z + k
    const int j = static_cast<int>(row - slab * d.Y);
    const int k = D == 3 ? static_cast<int>(slab % d.Z) : 0;
    const int64_t base = idx - ((static_cast<int64_t>(k) * d.Y + j) * d.X + i);   // key of cell (0,0,0) of this batch entry
    const float cx = static_cast<float>(i) + 0.5f, cy = static_cast<float>(j) + 0.5f, cz = static_cast<float>(k) + 0.5f;
    const int x0 = max(i - d.w, 0), x1 = min(i + d.w, d.X - 1);
    const int y0 = max(j - d.w, 0), y1 = min(j + d.w, d.Y - 1);
    const int z0 = D == 3 ? max(k - d.w, 0) : 0, z1 = D == 3 ? min(k + d.w, d.Z - 1) : 0;
    const int32_t cap = static_cast<int32_t>(d.total);
    for (int z = z0; z <= z1; ++z)
      for (int y = y0; y <= y1; ++y) {
        const int64_t key = base + (static_cast<int64_t>(z) * d.Y + y) * d.X;
        const int32_t s = min(max(cell_start[key + x0], 0), cap);
        const int32_t e = min(max(cell_start[key + x1 + 1], 0), cap);
        for (int32_t p = s; p < e; ++p) {
          const Rec<D> q = *reinterpret_cast<const Rec<D>*>(pos + static_cast<int64_t>(p) * D);
          const float dx = cx - q.v[0], dy = cy - q.v[1];
          float s2 = dx * dx + dy * dy;
          if (D == 3) {
            const float dz = cz - q.v[D - 1];
            s2 = s2 + dz * dz;
          }
          r = fminf(r, sqrtf(s2) - d.radius);
        }
      }
  }
  phi[idx] = r;
}

// The averaged level set (the header's averagedParticleLevelset row): one thread = one cell, the runs of the union kernel above -- the
// particles of cells x-r .. x+r of one (z, y) row are ONE contiguous range -- walked in ascending (z, y) order, so the sums run in
// ascending cell order and, inside a cell, in sorted order.  Three (D = 2) or four accumulators per thread, no LDS, no atomics.
struct AvgDims {
  int64_t nphi;    // B*Z*Y*X
  int64_t total;   // B*N
  int Z, Y, X;
  int r;           // (int)radius + 1
  float radius, r4;   // r4 = 4 * (radius * radius)
};

template <int D>
__global__ __launch_bounds__(kThreads) void levelset_averaged_kernel(const float* __restrict__ pos, const int32_t* __restrict__ cell_start,
                                                                     float* __restrict__ phi, AvgDims d) {
  const int64_t idx = xcd_block(blockIdx.x, gridDim.x, 0) * kThreads + threadIdx.x;
  if (idx >= d.nphi) return;
  float out = d.radius;
  if (d.total > 0) {
    const int64_t row = idx / d.X;
    const int i = static_cast<int>(idx - row * d.X);
    const int64_t slab = row / d.Y;                       // b*Z + k
    const int j = static_cast<int>(row - slab * d.Y);
    const int k = D == 3 ? static_cast<int>(slab % d.Z) : 0;
    const int64_t base = idx - ((static_cast<int64_t>(k) * d.Y + j) * d.X + i);   // key of cell (0,0,0) of this batch entry
    const float c[3] = {static_cast<float>(i) + 0.5f, static_cast<float>(j) + 0.5f, static_cast<float>(k) + 0.5f};
    const int x0 = max(i - d.r, 0), x1 = min(i + d.r, d.X - 1);
    const int y0 = max(j - d.r, 0), y1 = min(j + d.r, d.Y - 1);
    const int z0 = D == 3 ? max(k - d.r, 0) : 0, z1 = D == 3 ? min(k + d.r, d.Z - 1) : 0;
    const int32_t cap = static_cast<int32_t>(d.total);
    float wacc = 0.0f, pacc[D];
#pragma unroll
    for (int a = 0; a < D; ++a) pacc[a] = 0.0f;
    for (int z = z0; z <= z1; ++z)
      for (int y = y0; y <= y1; ++y) {
        const int64_t key = base + (static_cast<int64_t>(z) * d.Y + y) * d.X;
        const int32_t s = min(max(cell_start[key + x0], 0), cap);
        const int32_t e = min(max(cell_start[key + x1 + 1], 0), cap);
        for (int32_t p = s; p < e; ++p) {
          const Rec<D> q = *reinterpret_cast<const Rec<D>*>(pos + static_cast<int64_t>(p) * D);
          const float dx = c[0] - q.v[0], dy = c[1] - q.v[1];
          float s2 = dx * dx + dy * dy;
          if (D == 3) {
            const float dz = c[D - 1] - q.v[D - 1];
            s2 = s2 + dz * dz;
          }
          const float w = fmaxf(0.0f, 1.0f - s2 / d.r4);    // a NaN comes out as 0
          wacc = wacc + w;
#pragma unroll
          for (int a = 0; a < D; ++a) pacc[a] = pacc[a] + w * q.v[a];
        }
      }
    if (wacc > 1e-6f) {
      const float ex = c[0] - pacc[0] / wacc, ey = c[1] - pacc[1] / wacc;
      float s2 = ex * ex + ey * ey;
      if (D == 3) {
        const float ez = c[D - 1] - pacc[D - 1] / wacc;
        s2 = s2 + ez * ez;
      }
      out = sqrtf(s2) - d.radius;
    }
  }
  phi[idx] = out;
}

// One smoothing pass of the averaged level set, or its closing band.  mode 1: t = (self + x-, x+, y-, y+[, z-, z+], from self, in that
// order) * (1 / (2D + 1)) on every cell off the outermost layer of the grid; mode 2: the same t kept only where t < self; mode 0: a copy.
// band > 0: the cells within `band` of a side are set to bound_value instead (the script's phi.setBound).  Element-wise but for the
// 2D neighbour reads, which are coalesced along x; in != out for modes 1 and 2.
struct SmoothDims {
  int64_t n;       // B*Z*Y*X
  int Z, Y, X;
  int mode, band;
  float inv, bound_value;
};

template <int D>
__global__ __launch_bounds__(kThreads) void levelset_smooth_kernel(const float* in, float* out, SmoothDims d) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (idx >= d.n) return;
  const int64_t row = idx / d.X;
  const int i = static_cast<int>(idx - row * d.X);
  const int64_t slab = row / d.Y;
  const int j = static_cast<int>(row - slab * d.Y);
  const int k = D == 3 ? static_cast<int>(slab % d.Z) : 0;
  const int p[3] = {i, j, k};
  const int ext[3] = {d.X, d.Y, d.Z};
  const int64_t st[3] = {1, d.X, static_cast<int64_t>(d.X) * d.Y};
  bool inner = true, banded = false;
#pragma unroll
  for (int a = 0; a < D; ++a) {
    inner = inner && p[a] >= 1 && p[a] + 1 < ext[a];
    banded = banded || p[a] < d.band || p[a] >= ext[a] - d.band;
  }
  float v = in[idx];
  if (d.mode != 0 && inner) {                             // inner: all 2D neighbours are inside the entry
    float t = v;
#pragma unroll
    for (int a = 0; a < D; ++a) {
      t = t + in[idx - st[a]];
      t = t + in[idx + st[a]];
    }
    t = t * d.inv;
    v = d.mode == 1 ? t : (t < v ? t : v);
  }
  out[idx] = banded ? d.bound_value : v;
}

template <int D>
int particles_advect(const char* fn, const float* pos_in, float* pos_out, const float* vel, const int32_t* entry_start, bool ragged, int64_t B,
                     int64_t N, int64_t Z, int64_t Y, int64_t X, float dt, float vel_scale, int bnd, df_stream_t stream) {
  if (int e = check_dims(fn, D, B, N, Z, Y, X, ragged)) return e;
  if (int e = dfpart::check_ragged(fn, entry_start, ragged, N)) return e;
  DF_REQUIRE(bnd >= 0, DF_EINVAL, "%s: boundary width must be >= 0 (got %d)", fn, bnd);
  const int64_t need = 2 * static_cast<int64_t>(bnd) + 2;
  DF_REQUIRE(X >= need && Y >= need && (D == 2 || Z >= need), DF_ESHAPE, "%s: every extent must be >= 2*bnd + 2 = %lld", fn, (long long)need);
  DF_REQUIRE(vel && (N == 0 || (pos_in && pos_out)), DF_EINVAL, "%s: null %s", fn, !vel ? "velocity" : !pos_in ? "input" : "output");
  DF_REQUIRE(aligned4(pos_in) && aligned4(pos_out) && aligned4(vel), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  if (N == 0) return DF_OK;
  PartDims d;
  d.total = B * N; d.N = N; d.ncell = Z * Y * X;
  d.Z = (int)Z; d.Y = (int)Y; d.X = (int)X;
  d.lo = static_cast<float>(bnd);
  const int64_t ext[3] = {X, Y, Z};
  for (int a = 0; a < 3; ++a) d.hi[a] = static_cast<float>(ext[a] - bnd) - 0.0009765625f;
  d.dt = dt; d.half_dt = 0.5f * dt; d.vs = vel_scale;
  const unsigned nblk = static_cast<unsigned>(ceil_div(d.total, kThreads));
  hipStream_t s = df::as_stream(stream);
  if (ragged) hipLaunchKernelGGL((particles_advect_kernel<D, true>), dim3(nblk), dim3(kThreads), 0, s, pos_in, pos_out, vel, d, entry_start, (int)B);
  else hipLaunchKernelGGL((particles_advect_kernel<D, false>), dim3(nblk), dim3(kThreads), 0, s, pos_in, pos_out, vel, d, entry_start, 0);
  return df::launched(fn);
}

template <int D>
int particles_keys(const char* fn, const float* pos, int32_t* keys, const int32_t* entry_start, bool ragged, int64_t B, int64_t N, int64_t Z,
                   int64_t Y, int64_t X, df_stream_t stream) {
  if (int e = check_dims(fn, D, B, N, Z, Y, X, true)) return e;
  if (int e = dfpart::check_ragged(fn, entry_start, ragged, N)) return e;
  DF_REQUIRE(N == 0 || (pos && keys), DF_EINVAL, "%s: null %s", fn, !pos ? "input" : "output");
  DF_REQUIRE(aligned4(pos) && aligned4(keys), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  if (N == 0) return DF_OK;
  PartDims d = {};
  d.total = B * N; d.N = N; d.ncell = Z * Y * X;
  d.Z = (int)Z; d.Y = (int)Y; d.X = (int)X;
  const unsigned nblk = static_cast<unsigned>(ceil_div(d.total, kThreads));
  hipStream_t s = df::as_stream(stream);
  if (ragged) hipLaunchKernelGGL((particles_keys_kernel<D, true>), dim3(nblk), dim3(kThreads), 0, s, pos, keys, d, entry_start, (int)B);
  else hipLaunchKernelGGL((particles_keys_kernel<D, false>), dim3(nblk), dim3(kThreads), 0, s, pos, keys, d, entry_start, 0);
  return df::launched(fn);
}

template <int D>
int levelset_union(const char* fn, const float* pos, const int32_t* cell_start, float* phi, int64_t B, int64_t N, int64_t Z, int64_t Y,
                   int64_t X, float radius_factor, df_stream_t stream) {
  if (int e = check_dims(fn, D, B, N, Z, Y, X, true)) return e;
  DF_REQUIRE(radius_factor >= 0.0f && radius_factor <= 1024.0f, DF_EINVAL, "%s: radius_factor must lie in [0, 1024] (got %g)", fn,
             (double)radius_factor);
  DF_REQUIRE(phi && (N == 0 || (pos && cell_start)), DF_EINVAL, "%s: null %s", fn, !phi ? "output" : !pos ? "input" : "cell ranges");
  DF_REQUIRE(aligned4(pos) && aligned4(cell_start) && aligned4(phi), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  PhiDims d;
  d.nphi = B * Z * Y * X; d.total = B * N;
  d.Z = (int)Z; d.Y = (int)Y; d.X = (int)X;
  d.w = static_cast<int>(radius_factor) + 1;
  d.radius = (0.5f * sqrtf(static_cast<float>(D))) * (radius_factor + 0.01f);
  const unsigned nblk = static_cast<unsigned>(ceil_div(d.nphi, kThreads));
  hipLaunchKernelGGL((levelset_union_kernel<D>), dim3(nblk), dim3(kThreads), 0, df::as_stream(stream), pos, cell_start, phi, d);
  return df::launched(fn);
}

template <int D>
int levelset_averaged(const char* fn, const float* pos, const int32_t* cell_start, float* phi, int64_t B, int64_t N, int64_t Z, int64_t Y,
                      int64_t X, float radius_factor, df_stream_t stream) {
  if (int e = check_dims(fn, D, B, N, Z, Y, X, true)) return e;
  DF_REQUIRE(radius_factor >= 0.0f && radius_factor <= 1024.0f, DF_EINVAL, "%s: radius_factor must lie in [0, 1024] (got %g)", fn,
             (double)radius_factor);
  DF_REQUIRE(phi && (N == 0 || (pos && cell_start)), DF_EINVAL, "%s: null %s", fn, !phi ? "output" : !pos ? "input" : "cell ranges");
  DF_REQUIRE(aligned4(pos) && aligned4(cell_start) && aligned4(phi), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  AvgDims d;
  d.nphi = B * Z * Y * X; d.total = B * N;
  d.Z = (int)Z; d.Y = (int)Y; d.X = (int)X;
  d.radius = (0.5f * sqrtf(static_cast<float>(D))) * (radius_factor + 0.01f);
  d.r = static_cast<int>(d.radius) + 1;
  d.r4 = 4.0f * (d.radius * d.radius);
  const unsigned nblk = static_cast<unsigned>(ceil_div(d.nphi, kThreads));
  hipLaunchKernelGGL((levelset_averaged_kernel<D>), dim3(nblk), dim3(kThreads), 0, df::as_stream(stream), pos, cell_start, phi, d);
  return df::launched(fn);
}

template <int D>
int levelset_smooth(const char* fn, const float* in, float* out, int64_t B, int64_t Z, int64_t Y, int64_t X, int mode, int band,
                    float bound_value, df_stream_t stream) {
  if (int e = check_dims(fn, D, B, 0, Z, Y, X, true)) return e;
  DF_REQUIRE(in && out, DF_EINVAL, "%s: null %s", fn, !in ? "input" : "output");
  DF_REQUIRE(mode >= 0 && mode <= 2, DF_EINVAL, "%s: mode must be 0, 1 or 2 (got %d)", fn, mode);
  DF_REQUIRE(band >= 0, DF_EINVAL, "%s: the band must be >= 0 (got %d)", fn, band);
  DF_REQUIRE(aligned4(in) && aligned4(out), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  SmoothDims d;
  d.n = B * Z * Y * X;
  DF_REQUIRE(mode == 0 || dfadv::apart(in, 4 * d.n, out, 4 * d.n), DF_EINVAL, "%s: the output overlaps the input (the pass reads neighbours)", fn);
  d.Z = (int)Z; d.Y = (int)Y; d.X = (int)X;
  d.mode = mode; d.band = band;
  d.inv = 1.0f / static_cast<float>(2 * D + 1);
  d.bound_value = bound_value;
  const unsigned nblk = static_cast<unsigned>(ceil_div(d.n, kThreads));
  hipLaunchKernelGGL((levelset_smooth_kernel<D>), dim3(nblk), dim3(kThreads), 0, df::as_stream(stream), in, out, d);
  return df::launched(fn);
}

}  // namespace

extern "C" {

int df_particles_advect2d(const float* pos_in, float* pos_out, const float* vel, int64_t B, int64_t N, int64_t Y, int64_t X, float dt,
                          float vel_scale, int bnd, df_stream_t stream) {
  return particles_advect<2>("df_particles_advect2d", pos_in, pos_out, vel, nullptr, false, B, N, 1, Y, X, dt, vel_scale, bnd, stream);
}

int df_particles_advect3d(const float* pos_in, float* pos_out, const float* vel, int64_t B, int64_t N, int64_t Z, int64_t Y, int64_t X,
                          float dt, float vel_scale, int bnd, df_stream_t stream) {
  return particles_advect<3>("df_particles_advect3d", pos_in, pos_out, vel, nullptr, false, B, N, Z, Y, X, dt, vel_scale, bnd, stream);
}

int df_particles_cell_keys2d(const float* pos, int32_t* keys, int64_t B, int64_t N, int64_t Y, int64_t X, df_stream_t stream) {
  return particles_keys<2>("df_particles_cell_keys2d", pos, keys, nullptr, false, B, N, 1, Y, X, stream);
}

int df_particles_cell_keys3d(const float* pos, int32_t* keys, int64_t B, int64_t N, int64_t Z, int64_t Y, int64_t X, df_stream_t stream) {
  return particles_keys<3>("df_particles_cell_keys3d", pos, keys, nullptr, false, B, N, Z, Y, X, stream);
}

int df_particles_advect2d_ragged(const float* pos_in, float* pos_out, const float* vel, const int32_t* entry_start, int64_t B, int64_t N,
                                 int64_t Y, int64_t X, float dt, float vel_scale, int bnd, df_stream_t stream) {
  return particles_advect<2>("df_particles_advect2d_ragged", pos_in, pos_out, vel, entry_start, true, B, N, 1, Y, X, dt, vel_scale, bnd, stream);
}

int df_particles_advect3d_ragged(const float* pos_in, float* pos_out, const float* vel, const int32_t* entry_start, int64_t B, int64_t N,
                                 int64_t Z, int64_t Y, int64_t X, float dt, float vel_scale, int bnd, df_stream_t stream) {
  return particles_advect<3>("df_particles_advect3d_ragged", pos_in, pos_out, vel, entry_start, true, B, N, Z, Y, X, dt, vel_scale, bnd, stream);
}

int df_particles_cell_keys2d_ragged(const float* pos, int32_t* keys, const int32_t* entry_start, int64_t B, int64_t N, int64_t Y, int64_t X,
                                    df_stream_t stream) {
  return particles_keys<2>("df_particles_cell_keys2d_ragged", pos, keys, entry_start, true, B, N, 1, Y, X, stream);
}

int df_particles_cell_keys3d_ragged(const float* pos, int32_t* keys, const int32_t* entry_start, int64_t B, int64_t N, int64_t Z, int64_t Y,
                                    int64_t X, df_stream_t stream) {
  return particles_keys<3>("df_particles_cell_keys3d_ragged", pos, keys, entry_start, true, B, N, Z, Y, X, stream);
}

int df_particles_gather(const float* pos, const int64_t* order, float* pos_sorted, int64_t n, int dim, df_stream_t stream) {
  const char* fn = "df_particles_gather";
  DF_REQUIRE(dim == 2 || dim == 3, DF_EINVAL, "%s: dim must be 2 or 3 (got %d)", fn, dim);
  DF_REQUIRE(n >= 0, DF_EINVAL, "%s: negative count", fn);
  DF_REQUIRE(n <= kInt32Max, DF_ESHAPE, "%s: the particle count does not fit an int32", fn);
  DF_REQUIRE(n == 0 || (pos && order && pos_sorted), DF_EINVAL, "%s: null %s", fn, !pos ? "input" : !order ? "order" : "output");
  DF_REQUIRE(pos_sorted != pos || n == 0, DF_EINVAL, "%s: the output must not be the input (the step gathers)", fn);
  DF_REQUIRE(aligned4(pos) && aligned4(pos_sorted) && (reinterpret_cast<uintptr_t>(order) & 7u) == 0, DF_EALIGN,
             "%s: positions must be 4-byte, the order 8-byte aligned", fn);
  if (n == 0) return DF_OK;
  const unsigned nblk = static_cast<unsigned>(ceil_div(n, kThreads));
  hipStream_t s = df::as_stream(stream);
  if (dim == 2) hipLaunchKernelGGL((particles_gather_kernel<2>), dim3(nblk), dim3(kThreads), 0, s, pos, order, pos_sorted, n);
  else hipLaunchKernelGGL((particles_gather_kernel<3>), dim3(nblk), dim3(kThreads), 0, s, pos, order, pos_sorted, n);
  return df::launched(fn);
}

int df_particle_levelset_union2d(const float* pos_sorted, const int32_t* cell_start, float* phi, int64_t B, int64_t N, int64_t Y, int64_t X,
                                 float radius_factor, df_stream_t stream) {
  return levelset_union<2>("df_particle_levelset_union2d", pos_sorted, cell_start, phi, B, N, 1, Y, X, radius_factor, stream);
}

int df_particle_levelset_union3d(const float* pos_sorted, const int32_t* cell_start, float* phi, int64_t B, int64_t N, int64_t Z, int64_t Y,
                                 int64_t X, float radius_factor, df_stream_t stream) {
  return levelset_union<3>("df_particle_levelset_union3d", pos_sorted, cell_start, phi, B, N, Z, Y, X, radius_factor, stream);
}

int df_particle_levelset_averaged2d(const float* pos_sorted, const int32_t* cell_start, float* phi, int64_t B, int64_t N, int64_t Y,
                                    int64_t X, float radius_factor, df_stream_t stream) {
  return levelset_averaged<2>("df_particle_levelset_averaged2d", pos_sorted, cell_start, phi, B, N, 1, Y, X, radius_factor, stream);
}

int df_particle_levelset_averaged3d(const float* pos_sorted, const int32_t* cell_start, float* phi, int64_t B, int64_t N, int64_t Z,
                                    int64_t Y, int64_t X, float radius_factor, df_stream_t stream) {
  return levelset_averaged<3>("df_particle_levelset_averaged3d", pos_sorted, cell_start, phi, B, N, Z, Y, X, radius_factor, stream);
}

int df_levelset_smooth2d(const float* phi_in, float* phi_out, int64_t B, int64_t Y, int64_t X, int mode, int band, float bound_value,
                         df_stream_t stream) {
  return levelset_smooth<2>("df_levelset_smooth2d", phi_in, phi_out, B, 1, Y, X, mode, band, bound_value, stream);
}

int df_levelset_smooth3d(const float* phi_in, float* phi_out, int64_t B, int64_t Z, int64_t Y, int64_t X, int mode, int band,
                         float bound_value, df_stream_t stream) {
  return levelset_smooth<3>("df_levelset_smooth3d", phi_in, phi_out, B, Z, Y, X, mode, band, bound_value, stream);
}

}  // extern "C"
