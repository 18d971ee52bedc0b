// The solver half of the reference's smoke scene (scene/smoke_pos_size.py:186-195 main(): advectSemiLagrange(vel, vel), setWallBcs,
// addBuoyancy, solvePressure, setWallBcs for a closed box), written for gfx950 from the step definition in include/deepfluids_hip.h.
// Bit parity with mantaflow is NOT claimed (it cannot be run here); tests/smoke_ref.py restates the definition.
//
//   velocity [B,(Z,)Y,X,D] fp32 MAC face values (component a of cell c on c's low-a face), density / pressure [B,(Z,)Y,X] fp32, cell
//   (i,j,k) = [..,k,j,i]; interior: bnd <= index < extent - bnd on every axis, else a wall cell.
//
//   mac_sl / mac_mc   the velocity carried through itself, one thread = one cell and its D components, the helpers of advect.hip read
//                     with stride D.  As there: the gathers are data dependent and served by L1/L2, no LDS.
//   wall_buoyancy     element-wise: wall faces 0, kept faces += (0.5*force[a]) * (rho(c) + rho(c - e_a)).  The `_dev` entry points read
//                     force from device memory, one per batch entry, and run the same cell function: equal forces, equal bits.
//   pressure          plain conjugate gradients on the 5- / 7-point Neumann Laplacian of the interior cells, two launches per iteration:
//     direction(k)    every workgroup first combines its entry's r.r and max|r| partials (fixed order) and takes the entry's decision
//                     (converged / max_iter / go on, beta = rr / rr_old); then p = r + beta*p_old is recomputed at the cell and at its
//                     neighbours, p and q = A p are written and the p.q partial of the workgroup is stored.
//     update(k)       every workgroup combines the p.q partials, alpha = rr / p.q; x += alpha p, r -= alpha q, r.r and max|r| partials.
//   All per-entry scalars live in the workspace (two copies: a launch reads one and writes the other, so no workgroup reads a word that
//   another workgroup of the same launch writes).  A workgroup belongs to ONE batch entry and the partials are combined in an order that
//   depends on the grid extents alone: an entry's result does not depend on the rest of the batch.  No floating-point atomics.
//   The grids of one entry at the sizes this is used for (96x128: 48 KiB per array) live in L2; the XCD remap hands each XCD a contiguous
//   run of workgroups, so an entry's neighbours in y and z are on the same L2.
//
//   obstacles         the `_flags` entry points are the same kernels with MASKED set: "interior" reads "fluid" (interior and no obstacle),
//                     taken from ONE byte per cell that obstacle_flags packs once per sequence (the cell is fluid, each of its six
//                     neighbours is fluid): n_c is a popcount, the stencil's neighbour loads are predicated on the bits.  A flags byte is
//                     only believed where the cell is interior by its index, so no flags array can send a load outside the arrays.
//                     With an all-zero obstacle every branch is taken as without flags: the same bits.
//
//   open sides        the `_open` entry points are the same kernels again with OPEN set and `open_sides` (bits 0..5: x-, x+, y-, y+, z-,
//                     z+) as a trailing scalar: a band cell is OPEN when every side it lies beyond is open, a face is LIVE when one of
//                     its two cells is fluid and the other fluid or open.  All of it is integer compares on the cell's own index; the one
//                     thing read that was not read before is the low-neighbour bit of the flags byte of a high-side boundary cell (the
//                     byte itself is loaded by every thread already), and the loads that bit guards are valid by the index alone.
//                     open_sides = 0 is dispatched to the closed instantiations on the host: the same bits by construction.
//   open_extrapolate  zero-gradient fill of the open cells, in place: every open cell copies, per component, from the fixed point of a
//                     clamp of its index; a fixed point only ever copies onto itself, so there is no race.
//   sphere_source     the source stamp with one sphere per batch entry, the centres read from device memory.
//   diffusion         cgSolveDiffusion of the viscous liquid scene (scene/liquid3_vis.py:281), restated from memory as the header says: the
//                     same CG over the B*D components of a velocity, each its own system (I + alpha * Laplacian on the interior cells,
//                     the band Dirichlet data).  diffuse_init de-interleaves into planar x, r, p; the kRowDiffuse instantiation of the
//                     direction kernel reads the entry's alpha from device memory; the update kernel is the pressure solve's;
//                     diffuse_finish interleaves x back.  The component reads of init (stride D) and the component gathers of finish
//                     (D planes) are each coalesced along x within a plane; every other pass is planar.
//
//   ghost fluid       the `_gf` entry points: the liquid rows with the surface where phi = 0 between a liquid cell and an air neighbour
//                     (mantaflow's solvePressure(phi=), restated from memory as the header says; parity is with tests/liquid_gf_ref.py).
//                     Init and correction are kernels of their own: init also writes diag (1 per liquid neighbour, 1/theta per air
//                     neighbour) and z = r / diag behind the plain workspace, the correction puts the ghost value on the air side of a
//                     surface face.  Direction and update are the kRowDiag / kLeaveJacobi instantiations of the kernels above: the
//                     Jacobi-preconditioned iteration with r.z in the place of r.r.  The loop, the partials, the state words and
//                     df_pressure_status are the plain solve's.
//   The two kernels of the iteration and the checks of the solve entry points live in smoke_common.hpp; multigrid.hip launches them too.
//
// Float -> int conversions are taken only of values already known to be inside the grid (advect_common.hpp).
#include "advect_common.hpp"
#include "df_common.hpp"
#include "smoke_common.hpp"
#include "stencil_common.hpp"

namespace {

using df::ceil_div;
using dfadv::AdvDims;
using dfadv::apart;
using dfadv::Cell;
using dfadv::check_flags;
using dfadv::corner_range;
using dfadv::decode;
using dfadv::hi_bit;
using dfadv::interp;
using dfadv::kFluid;
using dfadv::lo_bit;
using dfadv::open_hi;
using dfadv::open_lo;
using dfst::kThreads;
using dfst::xcd_block;

template <int D>
struct VelRec { float v[D]; };

// ---- open sides (open_lo / open_hi: advect_common.hpp) ---------------------------------------------------------------------------------------
// a band cell is open when, on every axis where its index lies outside [bnd, extent - bnd), the side it lies on is open (an edge or a
// corner shared with a closed side stays wall)
template <int D>
__device__ __forceinline__ bool open_cell(const int* p, const int* ext, int bnd, int os) {
  bool band = false, ok = true;
#pragma unroll
  for (int a = 0; a < D; ++a) {
    const bool lo = p[a] < bnd, hi = p[a] >= ext[a] - bnd;
    band = band || lo || hi;
    ok = ok && (!lo || open_lo(os, a)) && (!hi || open_hi(os, a));
  }
  return band && ok;
}

// component a of a band cell sits on the high-side boundary face of axis a: c - e_a is interior by its index
template <int D>
__device__ __forceinline__ bool high_face(const int* p, const int* ext, int bnd, int a) {
  bool r = p[a] == ext[a] - bnd;
#pragma unroll
  for (int b = 0; b < D; ++b) if (b != a) r = r && p[b] >= bnd && p[b] < ext[b] - bnd;
  return r;
}

// component a of cell c is live although c and c - e_a are not both fluid: a fluid cell whose a- neighbour is open, or an open cell on
// the high-side boundary face whose a- neighbour is fluid (MASKED: the low-neighbour bit of the cell's own flags byte)
template <int D, bool MASKED>
__device__ __forceinline__ bool open_live_face(const int* p, const int* ext, bool interior, unsigned fl, int bnd, int a, int os) {
  if (interior) return (!MASKED || (fl & kFluid)) && p[a] == bnd && open_lo(os, a);
  return high_face<D>(p, ext, bnd, a) && open_hi(os, a) && (!MASKED || (fl & lo_bit(a)));
}

// ---- MAC self-advection ------------------------------------------------------------------------------------------------------------------
// dt * uface_a of an interior cell: the own component as it is, every other component b the mean of the four faces around the a-face
template <int D>
__device__ __forceinline__ void face_displacement(const float* __restrict__ vel, const Cell<D>& c, const AdvDims& d, int a, float* du) {
  const int64_t st[3] = {D, static_cast<int64_t>(d.X) * D, static_cast<int64_t>(d.X) * d.Y * D};
  const float* v = vel + c.idx * D;
#pragma unroll
  for (int b = 0; b < D; ++b) {
    if (b == a) du[b] = d.dt * v[a];
    else du[b] = d.dt * (0.25f * (((v[b] + v[b - st[a]]) + v[b + st[b]]) + v[b - st[a] + st[b]]));
  }
}

// OPEN: also component a of an open cell on the high-side boundary face of axis a (every cell face_displacement and interp read for it
// is inside the grid: c - e_a is interior, c + e_b stays within the extent because c is inside on every axis b != a)
template <int D, bool OPEN>
__global__ __launch_bounds__(kThreads) void mac_sl_kernel(const float* __restrict__ vel, float* __restrict__ fwd, AdvDims d, int os) {
  const int64_t idx = xcd_block(blockIdx.x, gridDim.x, 0) * kThreads + threadIdx.x;
  if (idx >= d.ncell) return;
  const Cell<D> c = decode<D>(idx, d);
  const int ext[3] = {d.X, d.Y, d.Z};
  VelRec<D> r;
#pragma unroll
  for (int a = 0; a < D; ++a) {
    r.v[a] = 0.0f;
    if (c.interior || (OPEN && high_face<D>(c.p, ext, d.bnd, a) && open_hi(os, a))) {
      float du[3], pos[3];
      face_displacement<D>(vel, c, d, a, du);
#pragma unroll
      for (int b = 0; b < D; ++b) pos[b] = (static_cast<float>(c.p[b]) + 0.5f) - du[b];
      r.v[a] = interp<D, D>(vel + c.base * D + a, pos, d);
    }
  }
  *reinterpret_cast<VelRec<D>*>(fwd + idx * D) = r;
}

// component a of cell c is a kept face: c and c - e_a are both interior (MASKED: fluid, read from the cell's flags byte)
template <bool MASKED>
__device__ __forceinline__ bool kept_face(bool interior, int pa, int bnd, unsigned fl, int a) {
  if (MASKED) return interior && (fl & kFluid) && (fl & lo_bit(a));
  return interior && pa > bnd;
}

template <int D, int MODE, bool MASKED, bool OPEN>
__global__ __launch_bounds__(kThreads) void mac_mc_kernel(const float* __restrict__ orig, const float* __restrict__ fwd,
                                                          float* __restrict__ out, const uint8_t* __restrict__ flags, AdvDims d, int os) {
  const int64_t idx = xcd_block(blockIdx.x, gridDim.x, 0) * kThreads + threadIdx.x;
  if (idx >= d.ncell) return;
  const Cell<D> c = decode<D>(idx, d);
  const unsigned fl = MASKED ? flags[idx] : 0u;
  const uint8_t* efl = MASKED ? flags + c.base : nullptr;
  const int ext[3] = {d.X, d.Y, d.Z};
  VelRec<D> r;
#pragma unroll
  for (int a = 0; a < D; ++a) {
    r.v[a] = 0.0f;
    if (c.interior || (OPEN && high_face<D>(c.p, ext, d.bnd, a) && open_hi(os, a))) {   // where mac_sl_kernel has written fwd
      const float f = fwd[idx * D + a];
      r.v[a] = f;
      // c - e_a is interior (MASKED: fluid) too; OPEN: or the face is live
      if (kept_face<MASKED>(c.interior, c.p[a], d.bnd, fl, a) || (OPEN && open_live_face<D, MASKED>(c.p, ext, c.interior, fl, d.bnd, a, os))) {
        float du[3], pos[3], t[3];
        face_displacement<D>(orig, c, d, a, du);
#pragma unroll
        for (int b = 0; b < D; ++b) pos[b] = (static_cast<float>(c.p[b]) + 0.5f) + du[b];
        const float bwd = interp<D, D>(fwd + c.base * D + a, pos, d);
        const float cor = f + 0.5f * (orig[idx * D + a] - bwd);
        float mn = 0.0f, mx = 0.0f;
        bool found = false;
#pragma unroll
        for (int b = 0; b < D; ++b) t[b] = static_cast<float>(c.p[b]) - du[b];
        corner_range<D, D, MASKED>(orig + c.base * D + a, t, d, mn, mx, found, efl);
        if (MODE == 1) {
#pragma unroll
          for (int b = 0; b < D; ++b) t[b] = static_cast<float>(c.p[b]) + du[b];
          corner_range<D, D, MASKED>(orig + c.base * D + a, t, d, mn, mx, found, efl);
        }
        if (!found) r.v[a] = f;
        else if (MODE == 2) r.v[a] = (cor < mn || cor > mx) ? f : cor;
        else r.v[a] = fminf(fmaxf(cor, mn), mx);
      }
    }
  }
  *reinterpret_cast<VelRec<D>*>(out + idx * D) = r;
}

// ---- obstacle flags --------------------------------------------------------------------------------------------------------------------------
// one byte per cell: bit 0 = the cell is fluid, bits 1-6 = its x-, x+, y-, y+, z-, z+ neighbour is (a neighbour outside the grid is not)
template <int D>
__global__ __launch_bounds__(kThreads) void obstacle_flags_kernel(const uint8_t* __restrict__ obs, uint8_t* __restrict__ flags, AdvDims d) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (idx >= d.ncell) return;
  const Cell<D> c = decode<D>(idx, d);
  const int64_t st[3] = {1, d.X, static_cast<int64_t>(d.X) * d.Y};
  const int ext[3] = {d.X, d.Y, d.Z};
  bool in[3] = {true, true, true};
#pragma unroll
  for (int a = 0; a < D; ++a) in[a] = c.p[a] >= d.bnd && c.p[a] < ext[a] - d.bnd;
  unsigned f = (c.interior && !obs[idx]) ? kFluid : 0u;
#pragma unroll
  for (int a = 0; a < D; ++a) {
    bool rest = true;                                   // the neighbours along a share the cell's other coordinates
#pragma unroll
    for (int b = 0; b < D; ++b) if (b != a) rest = rest && in[b];
    // bnd >= 1: a neighbour whose index passes the interior test is inside the grid
    if (rest && c.p[a] - 1 >= d.bnd && c.p[a] - 1 < ext[a] - d.bnd && !obs[idx - st[a]]) f |= lo_bit(a);
    if (rest && c.p[a] + 1 >= d.bnd && c.p[a] + 1 < ext[a] - d.bnd && !obs[idx + st[a]]) f |= hi_bit(a);
  }
  flags[idx] = static_cast<uint8_t>(f);
}

// ---- walls and buoyancy --------------------------------------------------------------------------------------------------------------------
struct Force { float f[3]; };

// OPEN: a live face that is not between two fluid cells is kept without the buoyancy term, and every other component of an open cell is
// copied through (it holds filled values) -- so an open cell keeps all of its components
template <int D, bool MASKED, bool OPEN>
__device__ __forceinline__ void wall_buoyancy_cell(const float* vel, const float* __restrict__ rho, float* out, const uint8_t* __restrict__ flags,
                                                   const float* force, const Cell<D>& c, const AdvDims& d, int os) {
  const int64_t idx = c.idx;
  const unsigned fl = MASKED ? flags[idx] : 0u;
  const int64_t st[3] = {1, d.X, static_cast<int64_t>(d.X) * d.Y};
  const VelRec<D> v = *reinterpret_cast<const VelRec<D>*>(vel + idx * D);
  const int ext[3] = {d.X, d.Y, d.Z};
  const bool opn = OPEN && !c.interior && open_cell<D>(c.p, ext, d.bnd, os);
  VelRec<D> r;
#pragma unroll
  for (int a = 0; a < D; ++a) {
    r.v[a] = opn ? v.v[a] : 0.0f;
    if (kept_face<MASKED>(c.interior, c.p[a], d.bnd, fl, a)) r.v[a] = v.v[a] + (0.5f * force[a]) * (rho[idx] + rho[idx - st[a]]);
    else if (OPEN && open_live_face<D, MASKED>(c.p, ext, c.interior, fl, d.bnd, a, os)) r.v[a] = v.v[a];
  }
  *reinterpret_cast<VelRec<D>*>(out + idx * D) = r;
}

template <int D, bool MASKED, bool OPEN>
__global__ __launch_bounds__(kThreads) void wall_buoyancy_kernel(const float* vel, const float* __restrict__ rho, float* out,
                                                                 const uint8_t* __restrict__ flags, Force force, AdvDims d, int os) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (idx >= d.ncell) return;
  wall_buoyancy_cell<D, MASKED, OPEN>(vel, rho, out, flags, force.f, decode<D>(idx, d), d, os);
}

// the same cell with the force of the cell's batch entry read from device memory, forces [B,D]: the same expression, so equal forces
// give the bits of the kernel above
template <int D, bool MASKED, bool OPEN>
__global__ __launch_bounds__(kThreads) void wall_buoyancy_dev_kernel(const float* vel, const float* __restrict__ rho, float* out,
                                                                     const uint8_t* __restrict__ flags, const float* __restrict__ forces,
                                                                     AdvDims d, int os) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (idx >= d.ncell) return;
  const Cell<D> c = decode<D>(idx, d);
  const float* f = forces + c.base / (static_cast<int64_t>(d.X) * d.Y * d.Z) * D;
  float force[D];
#pragma unroll
  for (int a = 0; a < D; ++a) force[a] = f[a];
  wall_buoyancy_cell<D, MASKED, OPEN>(vel, rho, out, flags, force, c, d, os);
}

// ---- pressure projection ---------------------------------------------------------------------------------------------------------------------
// PDims, CgState, pdecode, the reductions, PWs and the iteration itself (cg_direction_kernel, cg_update_kernel) live in smoke_common.hpp
// (multigrid.hip shares them)

// the right-hand side b = -div u of fluid cell g (its high faces are the low faces of cells inside the grid)
template <int D>
__device__ __forceinline__ float neg_divergence(const float* __restrict__ vel, int64_t g, const PDims& d) {
  const int64_t st[3] = {D, static_cast<int64_t>(d.X) * D, static_cast<int64_t>(d.X) * d.Y * D};
  const float* v = vel + g * D;
  float div = v[st[0]] - v[0];
  div = div + (v[st[1] + 1] - v[1]);
  if (D == 3) div = div + (v[st[2] + 2] - v[2]);
  return -div;
}

template <int D, bool MASKED>
__global__ __launch_bounds__(kThreads) void pressure_init_kernel(const float* __restrict__ vel, float* __restrict__ x,
                                                                 const uint8_t* __restrict__ flags, PWs w, PDims d) {
  __shared__ float lds[4];
  const PCell c = pdecode<D, MASKED>(d, flags);
  const int64_t g = static_cast<int64_t>(c.e) * d.n + c.cell;
  float b = 0.0f;
  if (c.interior) b = neg_divergence<D>(vel, g, d);
  if (c.cell < d.n) {
    x[g] = 0.0f; w.r[g] = b; w.p[0][g] = b; w.p[1][g] = 0.0f; w.q[g] = 0.0f;
  }
  const float rr = block_reduce<false>(b * b, lds);
  const float mx = block_reduce<true>(fabsf(b), lds);
  if (threadIdx.x == 0) {
    w.rr_part[static_cast<int64_t>(c.e) * d.nblk + c.j] = rr;
    w.mx_part[static_cast<int64_t>(c.e) * d.nblk + c.j] = mx;
  }
}

// one workgroup: the number of active entries (an integer sum: order-free) and, if asked for, every entry's iteration count
__global__ __launch_bounds__(kThreads) void cg_status_kernel(const CgState* __restrict__ s, int B, int32_t* __restrict__ count,
                                                            int32_t* __restrict__ iters) {
  __shared__ int lds[4];
  int n = 0;
  for (int e = threadIdx.x; e < B; e += kThreads) {
    n += s[e].active ? 1 : 0;
    if (iters) iters[e] = s[e].iters;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) n += __shfl_xor(n, m);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0 && count) count[0] = lds[0] + lds[1] + lds[2] + lds[3];
}

// ---- implicit velocity diffusion: the CG above over the B*D (entry, component) pairs of a velocity ----------------------------------------
// planar x, r, p from the interleaved velocity: x = u everywhere (the band is Dirichlet data and stays), r = b - A u =
// alpha * (sum of all 2D neighbours - 2D * u) on I and 0 off it.  d.B = B*D pairs; pair e is component e % D of entry e / D.
template <int D>
__global__ __launch_bounds__(kThreads) void diffuse_init_kernel(const float* __restrict__ vel, const float* __restrict__ dalpha,
                                                                float* __restrict__ x, PWs w, PDims d) {
  __shared__ float lds[4];
  const PCell c = pdecode<D>(d);
  const int be = c.e / D, a = c.e - be * D;
  const int64_t g = static_cast<int64_t>(c.e) * d.n + c.cell;
  float r = 0.0f;
  if (c.cell < d.n) {
    const float* v = vel + (static_cast<int64_t>(be) * d.n + c.cell) * D + a;
    const float u = v[0];
    if (c.interior) {                                   // bnd >= 1: all 2D neighbours are inside the entry
      const int64_t st[3] = {D, static_cast<int64_t>(d.X) * D, static_cast<int64_t>(d.X) * d.Y * D};
      float sum = 0.0f;
#pragma unroll
      for (int b = 0; b < D; ++b) { sum += v[-st[b]]; sum += v[st[b]]; }
      r = dalpha[be] * (sum - static_cast<float>(2 * D) * u);
    }
    x[g] = u; w.r[g] = r; w.p[0][g] = r; w.p[1][g] = 0.0f; w.q[g] = 0.0f;
  }
  const float rr = block_reduce<false>(r * r, lds);
  const float mx = block_reduce<true>(fabsf(r), lds);
  if (threadIdx.x == 0) {
    w.rr_part[static_cast<int64_t>(c.e) * d.nblk + c.j] = rr;
    w.mx_part[static_cast<int64_t>(c.e) * d.nblk + c.j] = mx;
  }
}

// the planar x back into the interleaved velocity, one thread = one cell and its D components; x holds the input's bits off I
template <int D>
__global__ __launch_bounds__(kThreads) void diffuse_finish_kernel(const float* __restrict__ x, float* __restrict__ out, int64_t n, int64_t ncell) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (idx >= ncell) return;
  const int64_t e = idx / n, cell = idx - e * n;
  VelRec<D> r;
#pragma unroll
  for (int a = 0; a < D; ++a) r.v[a] = x[(e * D + a) * n + cell];
  *reinterpret_cast<VelRec<D>*>(out + idx * D) = r;
}

// OPEN: live faces are corrected with p as the array holds it (0 outside the fluid), open cells keep their other components
// LIQUID (with MASKED): a face between two interior cells is corrected when at least one of them is liquid, with p as the array holds it
// (0 in air), and copied through otherwise; wall faces are 0
template <int D, bool MASKED, bool OPEN, bool LIQUID = false>
__global__ __launch_bounds__(kThreads) void pressure_correct_kernel(const float* vel, const float* __restrict__ pr, float* out,
                                                                    const uint8_t* __restrict__ flags, AdvDims d, int os) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (idx >= d.ncell) return;
  const Cell<D> c = decode<D>(idx, d);
  const unsigned fl = MASKED ? flags[idx] : 0u;
  const int64_t st[3] = {1, d.X, static_cast<int64_t>(d.X) * d.Y};
  const VelRec<D> v = *reinterpret_cast<const VelRec<D>*>(vel + idx * D);
  const int ext[3] = {d.X, d.Y, d.Z};
  const bool opn = OPEN && !c.interior && open_cell<D>(c.p, ext, d.bnd, os);
  VelRec<D> r;
#pragma unroll
  for (int a = 0; a < D; ++a) {
    r.v[a] = opn ? v.v[a] : 0.0f;
    if (LIQUID) {                                       // fl is read of an interior cell only
      if (kept_face<false>(c.interior, c.p[a], d.bnd, 0u, a))
        r.v[a] = ((fl & kFluid) || (fl & lo_bit(a))) ? v.v[a] - (pr[idx] - pr[idx - st[a]]) : v.v[a];
    } else if (kept_face<MASKED>(c.interior, c.p[a], d.bnd, fl, a) || (OPEN && open_live_face<D, MASKED>(c.p, ext, c.interior, fl, d.bnd, a, os)))
      r.v[a] = v.v[a] - (pr[idx] - pr[idx - st[a]]);    // a live face has p[a] >= bnd >= 1: c - e_a is inside the grid
  }
  *reinterpret_cast<VelRec<D>*>(out + idx * D) = r;
}

// ---- ghost-fluid free surface: the liquid rows with the surface where phi = 0 between a liquid cell and an air neighbour ------------------
// (gf_inv_theta, the 1/theta of a liquid cell towards an interior air neighbour, and gf_clamp_ok: smoke_common.hpp)

// the two arrays of the ghost-fluid path lie behind the workspace of the plain solve (df_pressure_status finds its words unchanged)
GfWs carve_gf(void* ws, int64_t B, int64_t n, int64_t nblk) {
  float* f = static_cast<float*>(ws) + ws_floats(B, n, nblk);
  return GfWs{f, f + B * n};
}

// b = -div on the liquid cells; diag = (1 per liquid neighbour, 1/theta per interior air neighbour, summed from 0 in the order x-, x+, y-,
// y+[, z-, z+]); z = b / diag; x = 0, r = b, p = z; the first r.z and max|r| partials.  Off the liquid: diag = 1, everything else 0.
template <int D>
__global__ __launch_bounds__(kThreads) void pressure_init_gf(const float* __restrict__ vel, float* __restrict__ x,
                                                             const uint8_t* __restrict__ flags, const float* __restrict__ phi, PWs w, GfWs gw,
                                                             PDims d, float gf_clamp) {
  __shared__ float lds[4];
  const PCell c = pdecode<D, true>(d, flags);
  const int64_t g = static_cast<int64_t>(c.e) * d.n + c.cell;
  float b = 0.0f, dg = 1.0f, z = 0.0f;
  if (c.interior) {
    b = neg_divergence<D>(vel, g, d);
    const int64_t sc[3] = {1, d.X, static_cast<int64_t>(d.X) * d.Y};
    const int ext[3] = {d.X, d.Y, d.Z};
    const float pi = phi[g];
    dg = 0.0f;
#pragma unroll
    for (int a = 0; a < D; ++a) {                         // a liquid cell is interior by its index: both neighbours are inside the entry
      if (c.fl & lo_bit(a)) dg = dg + 1.0f;
      else if (c.p[a] > d.bnd) dg = dg + gf_inv_theta(pi, phi[g - sc[a]], gf_clamp);
      if (c.fl & hi_bit(a)) dg = dg + 1.0f;
      else if (c.p[a] + 1 < ext[a] - d.bnd) dg = dg + gf_inv_theta(pi, phi[g + sc[a]], gf_clamp);
    }
    if (!(dg > 0.0f)) dg = 1.0f;                          // a liquid cell between walls alone: its row is 0 = b, never divided by
    z = b / dg;
  }
  if (c.cell < d.n) {
    x[g] = 0.0f; w.r[g] = b; w.p[0][g] = z; w.p[1][g] = 0.0f; w.q[g] = 0.0f; gw.diag[g] = dg; gw.z[g] = z;
  }
  const float rz = block_reduce<false>(b * z, lds);
  const float mx = block_reduce<true>(fabsf(b), lds);
  if (threadIdx.x == 0) {
    w.rr_part[static_cast<int64_t>(c.e) * d.nblk + c.j] = rz;
    w.mx_part[static_cast<int64_t>(c.e) * d.nblk + c.j] = mx;
  }
}

// the correction with the ghost value on the air side of a surface face: between interior cells c and c - e_a, both liquid:
// out = vel - (p[c] - p[c - e_a]); c liquid alone: out = vel - p[c] * (1/theta); c - e_a liquid alone: out = vel + p[c - e_a] * (1/theta),
// theta of the liquid cell towards the air one; no liquid: copied; wall faces 0
template <int D>
__global__ __launch_bounds__(kThreads) void pressure_correct_gf(const float* vel, const float* __restrict__ pr, float* out,
                                                                const uint8_t* __restrict__ flags, const float* __restrict__ phi, AdvDims d,
                                                                float gf_clamp) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (idx >= d.ncell) return;
  const Cell<D> c = decode<D>(idx, d);
  const unsigned fl = c.interior ? flags[idx] : 0u;     // a flags byte is believed of an interior cell only
  const int64_t st[3] = {1, d.X, static_cast<int64_t>(d.X) * d.Y};
  const VelRec<D> v = *reinterpret_cast<const VelRec<D>*>(vel + idx * D);
  VelRec<D> r;
#pragma unroll
  for (int a = 0; a < D; ++a) {
    r.v[a] = 0.0f;
    if (kept_face<false>(c.interior, c.p[a], d.bnd, 0u, a)) {   // c and c - e_a are interior: both inside the grid
      const bool here = (fl & kFluid) != 0u, there = (fl & lo_bit(a)) != 0u;
      const int64_t nb = idx - st[a];
      if (here && there) r.v[a] = v.v[a] - (pr[idx] - pr[nb]);
      else if (here) r.v[a] = v.v[a] - pr[idx] * gf_inv_theta(phi[idx], phi[nb], gf_clamp);
      else if (there) r.v[a] = v.v[a] + pr[nb] * gf_inv_theta(phi[nb], phi[idx], gf_clamp);
      else r.v[a] = v.v[a];
    }
  }
  *reinterpret_cast<VelRec<D>*>(out + idx * D) = r;
}

// ---- the fill of the open cells, the sphere stamp ------------------------------------------------------------------------------------------
// in place: vel[c][a] = vel[c'][a], c' = c clamped to [bnd, extent - bnd] along a and to [bnd, extent - bnd - 1] along every other axis
template <int D>
__global__ __launch_bounds__(kThreads) void open_extrapolate_kernel(float* vel, AdvDims d, int os) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (idx >= d.ncell) return;
  const Cell<D> c = decode<D>(idx, d);
  const int ext[3] = {d.X, d.Y, d.Z};
  if (c.interior || !open_cell<D>(c.p, ext, d.bnd, os)) return;
  VelRec<D> r;
#pragma unroll
  for (int a = 0; a < D; ++a) {
    int q[3] = {0, 0, 0};
#pragma unroll
    for (int b = 0; b < D; ++b) q[b] = min(max(c.p[b], d.bnd), ext[b] - d.bnd - (b == a ? 0 : 1));
    r.v[a] = vel[(c.base + (static_cast<int64_t>(q[2]) * d.Y + q[1]) * d.X + q[0]) * D + a];
  }
  *reinterpret_cast<VelRec<D>*>(vel + idx * D) = r;
}

// out = value where the cell centre lies within radius of the entry's centre, else density; out may be density
template <int D>
__global__ __launch_bounds__(kThreads) void sphere_source_kernel(const float* density, const float* __restrict__ centers, float radius,
                                                                 float value, float* out, AdvDims d) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (idx >= d.ncell) return;
  const Cell<D> c = decode<D>(idx, d);
  const float* ctr = centers + c.base / (static_cast<int64_t>(d.X) * d.Y * d.Z) * D;
  const float dx = (static_cast<float>(c.p[0]) + 0.5f) - ctr[0], dy = (static_cast<float>(c.p[1]) + 0.5f) - ctr[1];
  float s = dx * dx + dy * dy;
  if (D == 3) {
    const float dz = (static_cast<float>(c.p[2]) + 0.5f) - ctr[2];
    s = s + dz * dz;
  }
  out[idx] = s <= radius * radius ? value : density[idx];   // a NaN centre compares false: nothing is stamped
}

// ---- host side (aligned4, check_ws, check_apart, check_open, check_iter, DF_OPEN_CALL: smoke_common.hpp) --------------------------------------
int check_dims(const char* fn, int dim, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd) {
  DF_REQUIRE(B > 0 && Z > 0 && Y > 0 && X > 0, DF_EINVAL, "%s: non-positive extent", fn);
  DF_REQUIRE(bnd >= 1, DF_EINVAL, "%s: boundary width must be >= 1 (got %d)", fn, bnd);
  DF_REQUIRE(B < (1 << 24) && Z < (1 << 24) && Y < (1 << 24) && X < (1 << 24), DF_ESHAPE, "%s: extent too large", fn);
  const int64_t need = 2 * static_cast<int64_t>(bnd) + 2;
  DF_REQUIRE(X >= need && Y >= need && (dim == 2 || Z >= need), DF_ESHAPE, "%s: every extent must be >= 2*bnd + 2 = %lld", fn,
             (long long)need);
  DF_REQUIRE(Z * Y * X < (1ll << 40) / B, DF_ESHAPE, "%s: extent too large", fn);
  return DF_OK;
}

// the cell-per-thread grid over all B*Z*Y*X cells
int plan(const char* fn, int dim, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd, float dt, AdvDims* d, unsigned* nblk) {
  if (int e = check_dims(fn, dim, B, Z, Y, X, bnd)) return e;
  const int64_t n = B * Z * Y * X;
  DF_REQUIRE(ceil_div(n, kThreads) < (1ll << 31), DF_ESHAPE, "%s: extent too large", fn);
  *d = AdvDims{n, (int)Z, (int)Y, (int)X, bnd, dt, 1.0f};
  *nblk = static_cast<unsigned>(ceil_div(n, kThreads));
  return DF_OK;
}

// the grid of the solver: workgroups that never straddle batch entries
int pplan(const char* fn, int dim, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd, PDims* d, unsigned* grid) {
  if (int e = check_dims(fn, dim, B, Z, Y, X, bnd)) return e;
  const int64_t n = Z * Y * X, nblk = ceil_div(n, kThreads);
  DF_REQUIRE(nblk * B < (1ll << 31), DF_ESHAPE, "%s: extent too large", fn);
  *d = PDims{n, (int)nblk, (int)B, (int)Z, (int)Y, (int)X, bnd};
  *grid = static_cast<unsigned>(nblk * B);
  return DF_OK;
}

template <int D>
int obstacle_flags(const char* fn, const uint8_t* obstacle, uint8_t* flags, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd,
                   df_stream_t stream) {
  DF_REQUIRE(obstacle && flags, DF_EINVAL, "%s: null %s", fn, !obstacle ? "obstacle" : "flags");
  AdvDims d;
  unsigned nblk;
  if (int e = plan(fn, D, B, Z, Y, X, bnd, 0.0f, &d, &nblk)) return e;
  DF_REQUIRE(apart(obstacle, d.ncell, flags, d.ncell), DF_EINVAL, "%s: the flags overlap the obstacle (it is read at a neighbour)", fn);
  hipLaunchKernelGGL((obstacle_flags_kernel<D>), dim3(nblk), dim3(kThreads), 0, df::as_stream(stream), obstacle, flags, d);
  return df::launched(fn);
}

template <int D, bool OPEN = false>
int mac_sl(const char* fn, const float* vel, float* fwd, int64_t B, int64_t Z, int64_t Y, int64_t X, float dt, int bnd, df_stream_t stream,
           int os = 0) {
  DF_REQUIRE(vel && fwd, DF_EINVAL, "%s: null %s", fn, !vel ? "velocity" : "output");
  AdvDims d;
  unsigned nblk;
  if (int e = plan(fn, D, B, Z, Y, X, bnd, dt, &d, &nblk)) return e;
  DF_REQUIRE(fwd != vel, DF_EINVAL, "%s: the output must not be the input (the step gathers)", fn);
  DF_REQUIRE(aligned4(vel) && aligned4(fwd), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  hipLaunchKernelGGL((mac_sl_kernel<D, OPEN>), dim3(nblk), dim3(kThreads), 0, df::as_stream(stream), vel, fwd, d, os);
  return df::launched(fn);
}

template <int D, bool MASKED, bool OPEN = false>
int mac_mc(const char* fn, const float* vel, const float* fwd, float* out, const uint8_t* flags, int64_t B, int64_t Z, int64_t Y, int64_t X,
           float dt, int bnd, int clamp_mode, df_stream_t stream, int os = 0) {
  DF_REQUIRE(vel && fwd && out, DF_EINVAL, "%s: null %s", fn, !vel ? "velocity" : !fwd ? "input" : "output");
  DF_REQUIRE(clamp_mode == 1 || clamp_mode == 2, DF_EINVAL, "%s: clamp_mode must be 1 or 2 (got %d)", fn, clamp_mode);
  AdvDims d;
  unsigned nblk;
  if (int e = plan(fn, D, B, Z, Y, X, bnd, dt, &d, &nblk)) return e;
  DF_REQUIRE(out != vel && out != fwd, DF_EINVAL, "%s: the output must not be an input (the step gathers)", fn);
  if (int e = check_flags<MASKED>(fn, flags, d.ncell, out, 4 * d.ncell * D, "output")) return e;
  DF_REQUIRE(aligned4(vel) && aligned4(fwd) && aligned4(out), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  hipStream_t s = df::as_stream(stream);
  if (clamp_mode == 2) hipLaunchKernelGGL((mac_mc_kernel<D, 2, MASKED, OPEN>), dim3(nblk), dim3(kThreads), 0, s, vel, fwd, out, flags, d, os);
  else hipLaunchKernelGGL((mac_mc_kernel<D, 1, MASKED, OPEN>), dim3(nblk), dim3(kThreads), 0, s, vel, fwd, out, flags, d, os);
  return df::launched(fn);
}

template <int D, bool MASKED, bool OPEN = false>
int wall_buoyancy(const char* fn, const float* vel, const float* rho, float* out, const uint8_t* flags, int64_t B, int64_t Z, int64_t Y,
                  int64_t X, Force f, int bnd, df_stream_t stream, int os = 0) {
  DF_REQUIRE(vel && rho && out, DF_EINVAL, "%s: null %s", fn, !vel ? "velocity" : !rho ? "density" : "output");
  AdvDims d;
  unsigned nblk;
  if (int e = plan(fn, D, B, Z, Y, X, bnd, 0.0f, &d, &nblk)) return e;
  DF_REQUIRE(static_cast<const void*>(out) != static_cast<const void*>(rho), DF_EINVAL,
             "%s: the output must not be the density (it is read at a neighbour)", fn);
  if (int e = check_flags<MASKED>(fn, flags, d.ncell, out, 4 * d.ncell * D, "output")) return e;
  DF_REQUIRE(aligned4(vel) && aligned4(rho) && aligned4(out), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  hipLaunchKernelGGL((wall_buoyancy_kernel<D, MASKED, OPEN>), dim3(nblk), dim3(kThreads), 0, df::as_stream(stream), vel, rho, out, flags, f, d,
                     os);
  return df::launched(fn);
}

template <int D, bool MASKED, bool OPEN = false>
int wall_buoyancy_dev(const char* fn, const float* vel, const float* rho, float* out, const uint8_t* flags, const float* forces, int64_t B,
                      int64_t Z, int64_t Y, int64_t X, int bnd, df_stream_t stream, int os = 0) {
  DF_REQUIRE(vel && rho && out && forces, DF_EINVAL, "%s: null %s", fn, !vel ? "velocity" : !rho ? "density" : !out ? "output" : "forces");
  AdvDims d;
  unsigned nblk;
  if (int e = plan(fn, D, B, Z, Y, X, bnd, 0.0f, &d, &nblk)) return e;
  DF_REQUIRE(static_cast<const void*>(out) != static_cast<const void*>(rho), DF_EINVAL,
             "%s: the output must not be the density (it is read at a neighbour)", fn);
  DF_REQUIRE(apart(forces, 4 * B * D, out, 4 * d.ncell * D), DF_EINVAL, "%s: the forces overlap the output", fn);
  if (int e = check_flags<MASKED>(fn, flags, d.ncell, out, 4 * d.ncell * D, "output")) return e;
  DF_REQUIRE(aligned4(vel) && aligned4(rho) && aligned4(out) && aligned4(forces), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  hipLaunchKernelGGL((wall_buoyancy_dev_kernel<D, MASKED, OPEN>), dim3(nblk), dim3(kThreads), 0, df::as_stream(stream), vel, rho, out, flags,
                     forces, d, os);
  return df::launched(fn);
}

template <int D, bool MASKED>
int pressure_init(const char* fn, const float* vel, float* pressure, void* ws, int64_t ws_bytes, const uint8_t* flags, int64_t B, int64_t Z,
                  int64_t Y, int64_t X, int bnd, df_stream_t stream) {
  DF_REQUIRE(vel && pressure, DF_EINVAL, "%s: null %s", fn, !vel ? "velocity" : "pressure");
  PDims d;
  unsigned grid;
  if (int e = pplan(fn, D, B, Z, Y, X, bnd, &d, &grid)) return e;
  if (int e = check_ws(fn, ws, ws_bytes, d)) return e;
  const int64_t need = ws_bytes_needed(d);
  DF_REQUIRE(static_cast<const void*>(pressure) != static_cast<const void*>(vel), DF_EINVAL,
             "%s: the pressure must not be the velocity (it is read at a neighbour)", fn);
  if (int e = check_apart(fn, ws, need, vel, 4 * d.n * B * D, "velocity")) return e;
  if (int e = check_apart(fn, ws, need, pressure, 4 * d.n * B, "pressure")) return e;
  if (int e = check_flags<MASKED>(fn, flags, d.n * B, pressure, 4 * d.n * B, "pressure")) return e;
  if (MASKED) if (int e = check_apart(fn, ws, need, flags, d.n * B, "flags")) return e;
  DF_REQUIRE(aligned4(vel) && aligned4(pressure), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  hipLaunchKernelGGL((pressure_init_kernel<D, MASKED>), dim3(grid), dim3(kThreads), 0, df::as_stream(stream), vel, pressure, flags,
                     carve(ws, B, d.n, d.nblk), d);
  return df::launched(fn);
}

// the floats of the ghost-fluid solve behind the plain workspace: diag and z (carve_gf)
int64_t gf_floats(const PDims& d) { return 2 * static_cast<int64_t>(d.B) * d.n; }

// ROW = kRowDiag is the ghost-fluid solve (Jacobi: the direction from z, diag the row's coefficient); kRowDiffuse reads `dalpha`
template <int D, bool MASKED, bool OPEN = false, bool LIQUID = false, CgRow ROW = kRowCount>
int cg_direction(const char* fn, void* ws, int64_t ws_bytes, const uint8_t* flags, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd,
                 int64_t k, float accuracy, int64_t max_iter, df_stream_t stream, int os = 0, const float* dalpha = nullptr) {
  PDims d;
  unsigned grid;
  if (int e = pplan(fn, D, B, Z, Y, X, bnd, &d, &grid)) return e;
  const int64_t extra = ROW == kRowDiag ? gf_floats(d) : 0;
  if (int e = check_ws(fn, ws, ws_bytes, d, extra)) return e;
  if (int e = check_iter(fn, k, accuracy, max_iter)) return e;
  if (int e = check_flags<MASKED>(fn, flags, d.n * B, nullptr, 0, "")) return e;
  if (MASKED) if (int e = check_apart(fn, ws, ws_bytes_needed(d, extra), flags, d.n * B, "flags")) return e;
  const PWs w = carve(ws, B, d.n, d.nblk);
  const GfWs gw = carve_gf(ws, B, d.n, d.nblk);
  hipLaunchKernelGGL((cg_direction_kernel<D, MASKED, OPEN, LIQUID, ROW>), dim3(grid), dim3(kThreads), 0, df::as_stream(stream), w,
                     ROW == kRowDiag ? gw.z : w.r, ROW == kRowDiag ? gw.diag : dalpha, flags, d, (int)(k & 1), k == 0 ? 1 : 0, accuracy,
                     (int)max_iter, os);
  return df::launched(fn);
}

// LEAVE = kLeaveJacobi is the ghost-fluid solve
template <int D, bool MASKED, CgLeave LEAVE = kLeavePlain>
int cg_update(const char* fn, float* pressure, void* ws, int64_t ws_bytes, const uint8_t* flags, int64_t B, int64_t Z, int64_t Y, int64_t X,
              int bnd, int64_t k, df_stream_t stream) {
  DF_REQUIRE(pressure, DF_EINVAL, "%s: null pressure", fn);
  PDims d;
  unsigned grid;
  if (int e = pplan(fn, D, B, Z, Y, X, bnd, &d, &grid)) return e;
  const int64_t extra = LEAVE == kLeaveJacobi ? gf_floats(d) : 0, need = ws_bytes_needed(d, extra);
  if (int e = check_ws(fn, ws, ws_bytes, d, extra)) return e;
  DF_REQUIRE(k >= 0, DF_EINVAL, "%s: iteration %lld", fn, (long long)k);
  if (int e = check_apart(fn, ws, need, pressure, 4 * d.n * B, "pressure")) return e;
  if (int e = check_flags<MASKED>(fn, flags, d.n * B, pressure, 4 * d.n * B, "pressure")) return e;
  if (MASKED) if (int e = check_apart(fn, ws, need, flags, d.n * B, "flags")) return e;
  DF_REQUIRE(aligned4(pressure), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  hipLaunchKernelGGL((cg_update_kernel<D, MASKED, LEAVE>), dim3(grid), dim3(kThreads), 0, df::as_stream(stream), pressure,
                     carve(ws, B, d.n, d.nblk), LEAVE == kLeaveJacobi ? carve_gf(ws, B, d.n, d.nblk) : GfWs{nullptr, nullptr}, flags, d,
                     (int)(k & 1));
  return df::launched(fn);
}

template <int D, bool MASKED, bool OPEN = false, bool LIQUID = false>
int pressure_correct(const char* fn, const float* vel, const float* pressure, float* out, const uint8_t* flags, int64_t B, int64_t Z, int64_t Y,
                     int64_t X, int bnd, df_stream_t stream, int os = 0) {
  DF_REQUIRE(vel && pressure && out, DF_EINVAL, "%s: null %s", fn, !vel ? "velocity" : !pressure ? "pressure" : "output");
  AdvDims d;
  unsigned nblk;
  if (int e = plan(fn, D, B, Z, Y, X, bnd, 0.0f, &d, &nblk)) return e;
  DF_REQUIRE(static_cast<const void*>(out) != static_cast<const void*>(pressure), DF_EINVAL,
             "%s: the output must not be the pressure (it is read at a neighbour)", fn);
  if (int e = check_flags<MASKED>(fn, flags, d.ncell, out, 4 * d.ncell * D, "output")) return e;
  DF_REQUIRE(aligned4(vel) && aligned4(pressure) && aligned4(out), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  hipLaunchKernelGGL((pressure_correct_kernel<D, MASKED, OPEN, LIQUID>), dim3(nblk), dim3(kThreads), 0, df::as_stream(stream), vel, pressure, out, flags,
                     d, os);
  return df::launched(fn);
}

template <int D>
int open_extrapolate(const char* fn, float* vel, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd, int open_sides, df_stream_t stream) {
  DF_REQUIRE(vel, DF_EINVAL, "%s: null velocity", fn);
  if (int e = check_open(fn, D, open_sides)) return e;
  AdvDims d;
  unsigned nblk;
  if (int e = plan(fn, D, B, Z, Y, X, bnd, 0.0f, &d, &nblk)) return e;
  DF_REQUIRE(aligned4(vel), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  if (!open_sides) return DF_OK;                        // no open cell: nothing to write
  hipLaunchKernelGGL((open_extrapolate_kernel<D>), dim3(nblk), dim3(kThreads), 0, df::as_stream(stream), vel, d, open_sides);
  return df::launched(fn);
}

template <int D>
int sphere_source(const char* fn, const float* density, const float* centers, float radius, float value, float* out, int64_t B, int64_t Z,
                  int64_t Y, int64_t X, df_stream_t stream) {
  DF_REQUIRE(density && centers && out, DF_EINVAL, "%s: null %s", fn, !density ? "density" : !centers ? "centres" : "output");
  DF_REQUIRE(B > 0 && Z > 0 && Y > 0 && X > 0, DF_EINVAL, "%s: non-positive extent", fn);
  DF_REQUIRE(B < (1 << 24) && Z < (1 << 24) && Y < (1 << 24) && X < (1 << 24) && Z * Y * X < (1ll << 40) / B, DF_ESHAPE,
             "%s: extent too large", fn);
  const int64_t n = B * Z * Y * X;
  DF_REQUIRE(ceil_div(n, kThreads) < (1ll << 31), DF_ESHAPE, "%s: extent too large", fn);
  DF_REQUIRE(apart(centers, 4 * B * D, out, 4 * n), DF_EINVAL, "%s: the centres overlap the output", fn);
  DF_REQUIRE(aligned4(density) && aligned4(centers) && aligned4(out), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  const AdvDims d{n, (int)Z, (int)Y, (int)X, 0, 0.0f, 1.0f};
  hipLaunchKernelGGL((sphere_source_kernel<D>), dim3((unsigned)ceil_div(n, kThreads)), dim3(kThreads), 0, df::as_stream(stream), density,
                     centers, radius, value, out, d);
  return df::launched(fn);
}

// the solve over B*D pairs: its plan, and the workspace = the CG's for B*D entries, then the planar x
template <int D>
int dplan(const char* fn, void* ws, int64_t ws_bytes, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd, PDims* d, unsigned* grid, float** x) {
  DF_REQUIRE(B > 0 && B < (1 << 24) / D, B > 0 ? DF_ESHAPE : DF_EINVAL, "%s: %s", fn, B > 0 ? "extent too large" : "non-positive extent");
  if (int e = pplan(fn, D, B * D, Z, Y, X, bnd, d, grid)) return e;
  if (int e = check_ws(fn, ws, ws_bytes, *d, d->B * d->n)) return e;
  *x = static_cast<float*>(ws) + ws_floats(d->B, d->n, d->nblk);
  return DF_OK;
}

// the bytes of that workspace
int64_t dbytes(const PDims& d) { return ws_bytes_needed(d, d.B * d.n); }

template <int D>
int diffuse_init(const char* fn, const float* vel, const float* alpha, void* ws, int64_t ws_bytes, int64_t B, int64_t Z, int64_t Y, int64_t X,
                 int bnd, df_stream_t stream) {
  DF_REQUIRE(vel && alpha, DF_EINVAL, "%s: null %s", fn, !vel ? "velocity" : "alpha");
  PDims d;
  unsigned grid;
  float* x;
  if (int e = dplan<D>(fn, ws, ws_bytes, B, Z, Y, X, bnd, &d, &grid, &x)) return e;
  if (int e = check_apart(fn, ws, dbytes(d), vel, 4 * d.n * d.B, "velocity")) return e;
  if (int e = check_apart(fn, ws, dbytes(d), alpha, 4 * B, "alpha")) return e;
  DF_REQUIRE(aligned4(vel) && aligned4(alpha), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  hipLaunchKernelGGL((diffuse_init_kernel<D>), dim3(grid), dim3(kThreads), 0, df::as_stream(stream), vel, alpha, x, carve(ws, d.B, d.n, d.nblk), d);
  return df::launched(fn);
}

template <int D>
int diffuse_direction(const char* fn, const float* alpha, void* ws, int64_t ws_bytes, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd,
                      int64_t k, float accuracy, int64_t max_iter, df_stream_t stream) {
  DF_REQUIRE(alpha, DF_EINVAL, "%s: null alpha", fn);
  PDims d;
  unsigned grid;
  float* x;
  if (int e = dplan<D>(fn, ws, ws_bytes, B, Z, Y, X, bnd, &d, &grid, &x)) return e;
  if (int e = check_apart(fn, ws, dbytes(d), alpha, 4 * B, "alpha")) return e;
  DF_REQUIRE(aligned4(alpha), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  return cg_direction<D, false, false, false, kRowDiffuse>(fn, ws, ws_bytes, nullptr, d.B, Z, Y, X, bnd, k, accuracy, max_iter, stream, 0, alpha);
}

template <int D>
int diffuse_update(const char* fn, void* ws, int64_t ws_bytes, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd, int64_t k,
                   df_stream_t stream) {
  PDims d;
  unsigned grid;
  float* x;
  if (int e = dplan<D>(fn, ws, ws_bytes, B, Z, Y, X, bnd, &d, &grid, &x)) return e;
  return cg_update<D, false>(fn, x, ws, ws_bytes, nullptr, d.B, Z, Y, X, bnd, k, stream);
}

template <int D>
int diffuse_finish(const char* fn, void* ws, int64_t ws_bytes, float* out, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd,
                   df_stream_t stream) {
  DF_REQUIRE(out, DF_EINVAL, "%s: null output", fn);
  PDims d;
  unsigned grid;
  float* x;
  if (int e = dplan<D>(fn, ws, ws_bytes, B, Z, Y, X, bnd, &d, &grid, &x)) return e;
  if (int e = check_apart(fn, ws, dbytes(d), out, 4 * d.n * d.B, "output")) return e;
  DF_REQUIRE(aligned4(out), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  const int64_t ncell = B * d.n;                        // B * nblk < 2^31 (pplan): so is ceil(ncell / kThreads)
  hipLaunchKernelGGL((diffuse_finish_kernel<D>), dim3((unsigned)ceil_div(ncell, kThreads)), dim3(kThreads), 0, df::as_stream(stream), x, out,
                     d.n, ncell);
  return df::launched(fn);
}

// ---- the ghost-fluid solve: the workspace of the plain solve, then diag and z ----
template <int D>
int pressure_init_gf_(const char* fn, const float* vel, float* pressure, void* ws, int64_t ws_bytes, const uint8_t* flags, const float* phi,
                      int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd, float gf_clamp, df_stream_t stream) {
  DF_REQUIRE(vel && pressure && phi, DF_EINVAL, "%s: null %s", fn, !vel ? "velocity" : !pressure ? "pressure" : "level set");
  if (int e = gf_clamp_ok(fn, gf_clamp)) return e;
  PDims d;
  unsigned grid;
  if (int e = pplan(fn, D, B, Z, Y, X, bnd, &d, &grid)) return e;
  if (int e = check_ws(fn, ws, ws_bytes, d, gf_floats(d))) return e;
  const int64_t need = ws_bytes_needed(d, gf_floats(d));
  DF_REQUIRE(static_cast<const void*>(pressure) != static_cast<const void*>(vel) && static_cast<const void*>(pressure) != static_cast<const void*>(phi),
             DF_EINVAL, "%s: the pressure must not be the velocity or the level set (they are read at a neighbour)", fn);
  if (int e = check_apart(fn, ws, need, vel, 4 * d.n * B * D, "velocity")) return e;
  if (int e = check_apart(fn, ws, need, pressure, 4 * d.n * B, "pressure")) return e;
  if (int e = check_apart(fn, ws, need, phi, 4 * d.n * B, "level set")) return e;
  if (int e = check_flags<true>(fn, flags, d.n * B, pressure, 4 * d.n * B, "pressure")) return e;
  if (int e = check_apart(fn, ws, need, flags, d.n * B, "flags")) return e;
  DF_REQUIRE(aligned4(vel) && aligned4(pressure) && aligned4(phi), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  hipLaunchKernelGGL((pressure_init_gf<D>), dim3(grid), dim3(kThreads), 0, df::as_stream(stream), vel, pressure, flags, phi,
                     carve(ws, B, d.n, d.nblk), carve_gf(ws, B, d.n, d.nblk), d, gf_clamp);
  return df::launched(fn);
}

template <int D>
int pressure_correct_gf_(const char* fn, const float* vel, const float* pressure, float* out, const uint8_t* flags, const float* phi, int64_t B,
                         int64_t Z, int64_t Y, int64_t X, int bnd, float gf_clamp, df_stream_t stream) {
  DF_REQUIRE(vel && pressure && out && phi, DF_EINVAL, "%s: null %s", fn, !vel ? "velocity" : !pressure ? "pressure" : !out ? "output" : "level set");
  if (int e = gf_clamp_ok(fn, gf_clamp)) return e;
  AdvDims d;
  unsigned nblk;
  if (int e = plan(fn, D, B, Z, Y, X, bnd, 0.0f, &d, &nblk)) return e;
  DF_REQUIRE(apart(out, 4 * d.ncell * D, pressure, 4 * d.ncell) && apart(out, 4 * d.ncell * D, phi, 4 * d.ncell), DF_EINVAL,
             "%s: the output overlaps the pressure or the level set (they are read at a neighbour)", fn);
  if (int e = check_flags<true>(fn, flags, d.ncell, out, 4 * d.ncell * D, "output")) return e;
  DF_REQUIRE(aligned4(vel) && aligned4(pressure) && aligned4(out) && aligned4(phi), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  hipLaunchKernelGGL((pressure_correct_gf<D>), dim3(nblk), dim3(kThreads), 0, df::as_stream(stream), vel, pressure, out, flags, phi, d, gf_clamp);
  return df::launched(fn);
}

}  // namespace

extern "C" {

int df_mac_advect_sl2d(const float* vel, float* fwd, int64_t B, int64_t Y, int64_t X, float dt, int bnd, df_stream_t stream) {
  return mac_sl<2>("df_mac_advect_sl2d", vel, fwd, B, 1, Y, X, dt, bnd, stream);
}
int df_mac_advect_sl3d(const float* vel, float* fwd, int64_t B, int64_t Z, int64_t Y, int64_t X, float dt, int bnd, df_stream_t stream) {
  return mac_sl<3>("df_mac_advect_sl3d", vel, fwd, B, Z, Y, X, dt, bnd, stream);
}
int df_mac_advect_mc2d(const float* vel, const float* fwd, float* out, int64_t B, int64_t Y, int64_t X, float dt, int bnd, int clamp_mode,
                       df_stream_t stream) {
  return mac_mc<2, false>("df_mac_advect_mc2d", vel, fwd, out, nullptr, B, 1, Y, X, dt, bnd, clamp_mode, stream);
}
int df_mac_advect_mc3d(const float* vel, const float* fwd, float* out, int64_t B, int64_t Z, int64_t Y, int64_t X, float dt, int bnd,
                       int clamp_mode, df_stream_t stream) {
  return mac_mc<3, false>("df_mac_advect_mc3d", vel, fwd, out, nullptr, B, Z, Y, X, dt, bnd, clamp_mode, stream);
}

int df_wall_buoyancy2d(const float* vel, const float* density, float* out, int64_t B, int64_t Y, int64_t X, float fx, float fy, int bnd,
                       df_stream_t stream) {
  return wall_buoyancy<2, false>("df_wall_buoyancy2d", vel, density, out, nullptr, B, 1, Y, X, Force{{fx, fy, 0.0f}}, bnd, stream);
}
int df_wall_buoyancy3d(const float* vel, const float* density, float* out, int64_t B, int64_t Z, int64_t Y, int64_t X, float fx, float fy,
                       float fz, int bnd, df_stream_t stream) {
  return wall_buoyancy<3, false>("df_wall_buoyancy3d", vel, density, out, nullptr, B, Z, Y, X, Force{{fx, fy, fz}}, bnd, stream);
}

int64_t df_pressure_workspace_bytes(int64_t B, int64_t Z, int64_t Y, int64_t X) {
  if (B <= 0 || Z <= 0 || Y <= 0 || X <= 0 || B >= (1 << 24) || Z >= (1 << 24) || Y >= (1 << 24) || X >= (1 << 24)) return DF_EINVAL;
  if (Z * Y * X >= (1ll << 40) / B) return DF_ESHAPE;
  const int64_t n = Z * Y * X;
  return 4 * ws_floats(B, n, ceil_div(n, kThreads));
}

int df_pressure_init2d(const float* vel, float* pressure, void* ws, int64_t ws_bytes, int64_t B, int64_t Y, int64_t X, int bnd,
                       df_stream_t stream) {
  return pressure_init<2, false>("df_pressure_init2d", vel, pressure, ws, ws_bytes, nullptr, B, 1, Y, X, bnd, stream);
}
int df_pressure_init3d(const float* vel, float* pressure, void* ws, int64_t ws_bytes, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd,
                       df_stream_t stream) {
  return pressure_init<3, false>("df_pressure_init3d", vel, pressure, ws, ws_bytes, nullptr, B, Z, Y, X, bnd, stream);
}
int df_pressure_cg_direction2d(void* ws, int64_t ws_bytes, int64_t B, int64_t Y, int64_t X, int bnd, int64_t k, float accuracy,
                               int64_t max_iter, df_stream_t stream) {
  return cg_direction<2, false>("df_pressure_cg_direction2d", ws, ws_bytes, nullptr, B, 1, Y, X, bnd, k, accuracy, max_iter, stream);
}
int df_pressure_cg_direction3d(void* ws, int64_t ws_bytes, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd, int64_t k, float accuracy,
                               int64_t max_iter, df_stream_t stream) {
  return cg_direction<3, false>("df_pressure_cg_direction3d", ws, ws_bytes, nullptr, B, Z, Y, X, bnd, k, accuracy, max_iter, stream);
}
int df_pressure_cg_update2d(float* pressure, void* ws, int64_t ws_bytes, int64_t B, int64_t Y, int64_t X, int bnd, int64_t k,
                            df_stream_t stream) {
  return cg_update<2, false>("df_pressure_cg_update2d", pressure, ws, ws_bytes, nullptr, B, 1, Y, X, bnd, k, stream);
}
int df_pressure_cg_update3d(float* pressure, void* ws, int64_t ws_bytes, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd, int64_t k,
                            df_stream_t stream) {
  return cg_update<3, false>("df_pressure_cg_update3d", pressure, ws, ws_bytes, nullptr, B, Z, Y, X, bnd, k, stream);
}

int df_pressure_status(const void* ws, int64_t ws_bytes, int64_t B, int64_t Z, int64_t Y, int64_t X, int64_t k, int32_t* active_count,
                       int32_t* iterations, df_stream_t stream) {
  const char* fn = "df_pressure_status";
  DF_REQUIRE(B > 0 && Z > 0 && Y > 0 && X > 0, DF_EINVAL, "%s: non-positive extent", fn);
  DF_REQUIRE(B < (1 << 24) && Z < (1 << 24) && Y < (1 << 24) && X < (1 << 24) && Z * Y * X < (1ll << 40) / B, DF_ESHAPE,
             "%s: extent too large", fn);
  const PDims d{Z * Y * X, (int)ceil_div(Z * Y * X, kThreads), (int)B, (int)Z, (int)Y, (int)X, 1};
  if (int e = check_ws(fn, ws, ws_bytes, d)) return e;
  DF_REQUIRE(active_count || iterations, DF_EINVAL, "%s: null outputs", fn);
  if (int e = check_apart(fn, ws, ws_bytes_needed(d), active_count, 4, "active count")) return e;
  if (int e = check_apart(fn, ws, ws_bytes_needed(d), iterations, 4 * B, "iteration counts")) return e;
  DF_REQUIRE(k >= 0, DF_EINVAL, "%s: iteration %lld", fn, (long long)k);
  DF_REQUIRE(aligned4(active_count) && aligned4(iterations), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  const PWs w = carve(const_cast<void*>(ws), B, d.n, d.nblk);
  hipLaunchKernelGGL(cg_status_kernel, dim3(1), dim3(kThreads), 0, df::as_stream(stream), w.state[(k & 1) ^ 1], (int)B, active_count, iterations);
  return df::launched(fn);
}

int df_pressure_correct2d(const float* vel, const float* pressure, float* out, int64_t B, int64_t Y, int64_t X, int bnd, df_stream_t stream) {
  return pressure_correct<2, false>("df_pressure_correct2d", vel, pressure, out, nullptr, B, 1, Y, X, bnd, stream);
}
int df_pressure_correct3d(const float* vel, const float* pressure, float* out, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd,
                          df_stream_t stream) {
  return pressure_correct<3, false>("df_pressure_correct3d", vel, pressure, out, nullptr, B, Z, Y, X, bnd, stream);
}

// ---- the same steps around obstacles: "interior" reads "fluid", taken from the flags of df_obstacle_flags* ----
int df_obstacle_flags2d(const uint8_t* obstacle, uint8_t* flags, int64_t B, int64_t Y, int64_t X, int bnd, df_stream_t stream) {
  return obstacle_flags<2>("df_obstacle_flags2d", obstacle, flags, B, 1, Y, X, bnd, stream);
}
int df_obstacle_flags3d(const uint8_t* obstacle, uint8_t* flags, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd, df_stream_t stream) {
  return obstacle_flags<3>("df_obstacle_flags3d", obstacle, flags, B, Z, Y, X, bnd, stream);
}
int df_mac_advect_mc2d_flags(const float* vel, const float* fwd, float* out, const uint8_t* flags, int64_t B, int64_t Y, int64_t X, float dt,
                             int bnd, int clamp_mode, df_stream_t stream) {
  return mac_mc<2, true>("df_mac_advect_mc2d_flags", vel, fwd, out, flags, B, 1, Y, X, dt, bnd, clamp_mode, stream);
}
int df_mac_advect_mc3d_flags(const float* vel, const float* fwd, float* out, const uint8_t* flags, int64_t B, int64_t Z, int64_t Y, int64_t X,
                             float dt, int bnd, int clamp_mode, df_stream_t stream) {
  return mac_mc<3, true>("df_mac_advect_mc3d_flags", vel, fwd, out, flags, B, Z, Y, X, dt, bnd, clamp_mode, stream);
}
int df_wall_buoyancy2d_flags(const float* vel, const float* density, float* out, const uint8_t* flags, int64_t B, int64_t Y, int64_t X,
                             float fx, float fy, int bnd, df_stream_t stream) {
  return wall_buoyancy<2, true>("df_wall_buoyancy2d_flags", vel, density, out, flags, B, 1, Y, X, Force{{fx, fy, 0.0f}}, bnd, stream);
}
int df_wall_buoyancy3d_flags(const float* vel, const float* density, float* out, const uint8_t* flags, int64_t B, int64_t Z, int64_t Y,
                             int64_t X, float fx, float fy, float fz, int bnd, df_stream_t stream) {
  return wall_buoyancy<3, true>("df_wall_buoyancy3d_flags", vel, density, out, flags, B, Z, Y, X, Force{{fx, fy, fz}}, bnd, stream);
}
int df_pressure_init2d_flags(const float* vel, float* pressure, void* ws, int64_t ws_bytes, const uint8_t* flags, int64_t B, int64_t Y,
                             int64_t X, int bnd, df_stream_t stream) {
  return pressure_init<2, true>("df_pressure_init2d_flags", vel, pressure, ws, ws_bytes, flags, B, 1, Y, X, bnd, stream);
}
int df_pressure_init3d_flags(const float* vel, float* pressure, void* ws, int64_t ws_bytes, const uint8_t* flags, int64_t B, int64_t Z,
                             int64_t Y, int64_t X, int bnd, df_stream_t stream) {
  return pressure_init<3, true>("df_pressure_init3d_flags", vel, pressure, ws, ws_bytes, flags, B, Z, Y, X, bnd, stream);
}
int df_pressure_cg_direction2d_flags(void* ws, int64_t ws_bytes, const uint8_t* flags, int64_t B, int64_t Y, int64_t X, int bnd, int64_t k,
                                     float accuracy, int64_t max_iter, df_stream_t stream) {
  return cg_direction<2, true>("df_pressure_cg_direction2d_flags", ws, ws_bytes, flags, B, 1, Y, X, bnd, k, accuracy, max_iter, stream);
}
int df_pressure_cg_direction3d_flags(void* ws, int64_t ws_bytes, const uint8_t* flags, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd,
                                     int64_t k, float accuracy, int64_t max_iter, df_stream_t stream) {
  return cg_direction<3, true>("df_pressure_cg_direction3d_flags", ws, ws_bytes, flags, B, Z, Y, X, bnd, k, accuracy, max_iter, stream);
}
int df_pressure_cg_update2d_flags(float* pressure, void* ws, int64_t ws_bytes, const uint8_t* flags, int64_t B, int64_t Y, int64_t X, int bnd,
                                  int64_t k, df_stream_t stream) {
  return cg_update<2, true>("df_pressure_cg_update2d_flags", pressure, ws, ws_bytes, flags, B, 1, Y, X, bnd, k, stream);
}
int df_pressure_cg_update3d_flags(float* pressure, void* ws, int64_t ws_bytes, const uint8_t* flags, int64_t B, int64_t Z, int64_t Y, int64_t X,
                                  int bnd, int64_t k, df_stream_t stream) {
  return cg_update<3, true>("df_pressure_cg_update3d_flags", pressure, ws, ws_bytes, flags, B, Z, Y, X, bnd, k, stream);
}
int df_pressure_correct2d_flags(const float* vel, const float* pressure, float* out, const uint8_t* flags, int64_t B, int64_t Y, int64_t X,
                                int bnd, df_stream_t stream) {
  return pressure_correct<2, true>("df_pressure_correct2d_flags", vel, pressure, out, flags, B, 1, Y, X, bnd, stream);
}
int df_pressure_correct3d_flags(const float* vel, const float* pressure, float* out, const uint8_t* flags, int64_t B, int64_t Z, int64_t Y,
                                int64_t X, int bnd, df_stream_t stream) {
  return pressure_correct<3, true>("df_pressure_correct3d_flags", vel, pressure, out, flags, B, Z, Y, X, bnd, stream);
}

// ---- the same steps with open sides: flags may be null (no obstacles), open_sides follows bnd ----
int df_mac_advect_sl2d_open(const float* vel, float* fwd, int64_t B, int64_t Y, int64_t X, float dt, int bnd, int open_sides,
                            df_stream_t stream) {
  const char* fn = "df_mac_advect_sl2d_open";
  if (int e = check_open(fn, 2, open_sides)) return e;
  return open_sides ? mac_sl<2, true>(fn, vel, fwd, B, 1, Y, X, dt, bnd, stream, open_sides) : mac_sl<2>(fn, vel, fwd, B, 1, Y, X, dt, bnd, stream);
}
int df_mac_advect_sl3d_open(const float* vel, float* fwd, int64_t B, int64_t Z, int64_t Y, int64_t X, float dt, int bnd, int open_sides,
                            df_stream_t stream) {
  const char* fn = "df_mac_advect_sl3d_open";
  if (int e = check_open(fn, 3, open_sides)) return e;
  return open_sides ? mac_sl<3, true>(fn, vel, fwd, B, Z, Y, X, dt, bnd, stream, open_sides) : mac_sl<3>(fn, vel, fwd, B, Z, Y, X, dt, bnd, stream);
}
int df_mac_advect_mc2d_open(const float* vel, const float* fwd, float* out, const uint8_t* flags, int64_t B, int64_t Y, int64_t X, float dt,
                            int bnd, int open_sides, int clamp_mode, df_stream_t stream) {
  const char* fn = "df_mac_advect_mc2d_open";
  if (int e = check_open(fn, 2, open_sides)) return e;
  return DF_OPEN_CALL(mac_mc, 2, fn, vel, fwd, out, flags, B, 1, Y, X, dt, bnd, clamp_mode, stream);
}
int df_mac_advect_mc3d_open(const float* vel, const float* fwd, float* out, const uint8_t* flags, int64_t B, int64_t Z, int64_t Y, int64_t X,
                            float dt, int bnd, int open_sides, int clamp_mode, df_stream_t stream) {
  const char* fn = "df_mac_advect_mc3d_open";
  if (int e = check_open(fn, 3, open_sides)) return e;
  return DF_OPEN_CALL(mac_mc, 3, fn, vel, fwd, out, flags, B, Z, Y, X, dt, bnd, clamp_mode, stream);
}
int df_wall_buoyancy2d_open(const float* vel, const float* density, float* out, const uint8_t* flags, int64_t B, int64_t Y, int64_t X,
                            float fx, float fy, int bnd, int open_sides, df_stream_t stream) {
  const char* fn = "df_wall_buoyancy2d_open";
  if (int e = check_open(fn, 2, open_sides)) return e;
  return DF_OPEN_CALL(wall_buoyancy, 2, fn, vel, density, out, flags, B, 1, Y, X, Force{{fx, fy, 0.0f}}, bnd, stream);
}
int df_wall_buoyancy3d_open(const float* vel, const float* density, float* out, const uint8_t* flags, int64_t B, int64_t Z, int64_t Y,
                            int64_t X, float fx, float fy, float fz, int bnd, int open_sides, df_stream_t stream) {
  const char* fn = "df_wall_buoyancy3d_open";
  if (int e = check_open(fn, 3, open_sides)) return e;
  return DF_OPEN_CALL(wall_buoyancy, 3, fn, vel, density, out, flags, B, Z, Y, X, Force{{fx, fy, fz}}, bnd, stream);
}
int df_wall_buoyancy2d_open_dev(const float* vel, const float* density, float* out, const uint8_t* flags, const float* forces, int64_t B,
                                int64_t Y, int64_t X, int bnd, int open_sides, df_stream_t stream) {
  const char* fn = "df_wall_buoyancy2d_open_dev";
  if (int e = check_open(fn, 2, open_sides)) return e;
  return DF_OPEN_CALL(wall_buoyancy_dev, 2, fn, vel, density, out, flags, forces, B, 1, Y, X, bnd, stream);
}
int df_wall_buoyancy3d_open_dev(const float* vel, const float* density, float* out, const uint8_t* flags, const float* forces, int64_t B,
                                int64_t Z, int64_t Y, int64_t X, int bnd, int open_sides, df_stream_t stream) {
  const char* fn = "df_wall_buoyancy3d_open_dev";
  if (int e = check_open(fn, 3, open_sides)) return e;
  return DF_OPEN_CALL(wall_buoyancy_dev, 3, fn, vel, density, out, flags, forces, B, Z, Y, X, bnd, stream);
}
int df_pressure_cg_direction2d_open(void* ws, int64_t ws_bytes, const uint8_t* flags, int64_t B, int64_t Y, int64_t X, int bnd,
                                    int open_sides, int64_t k, float accuracy, int64_t max_iter, df_stream_t stream) {
  const char* fn = "df_pressure_cg_direction2d_open";
  if (int e = check_open(fn, 2, open_sides)) return e;
  return DF_OPEN_CALL(cg_direction, 2, fn, ws, ws_bytes, flags, B, 1, Y, X, bnd, k, accuracy, max_iter, stream);
}
int df_pressure_cg_direction3d_open(void* ws, int64_t ws_bytes, const uint8_t* flags, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd,
                                    int open_sides, int64_t k, float accuracy, int64_t max_iter, df_stream_t stream) {
  const char* fn = "df_pressure_cg_direction3d_open";
  if (int e = check_open(fn, 3, open_sides)) return e;
  return DF_OPEN_CALL(cg_direction, 3, fn, ws, ws_bytes, flags, B, Z, Y, X, bnd, k, accuracy, max_iter, stream);
}
int df_pressure_correct2d_open(const float* vel, const float* pressure, float* out, const uint8_t* flags, int64_t B, int64_t Y, int64_t X,
                               int bnd, int open_sides, df_stream_t stream) {
  const char* fn = "df_pressure_correct2d_open";
  if (int e = check_open(fn, 2, open_sides)) return e;
  return DF_OPEN_CALL(pressure_correct, 2, fn, vel, pressure, out, flags, B, 1, Y, X, bnd, stream);
}
int df_pressure_correct3d_open(const float* vel, const float* pressure, float* out, const uint8_t* flags, int64_t B, int64_t Z, int64_t Y,
                               int64_t X, int bnd, int open_sides, df_stream_t stream) {
  const char* fn = "df_pressure_correct3d_open";
  if (int e = check_open(fn, 3, open_sides)) return e;
  return DF_OPEN_CALL(pressure_correct, 3, fn, vel, pressure, out, flags, B, Z, Y, X, bnd, stream);
}
// ---- the free-surface projection of the liquid step (liquid.hip): the flags of df_liquid_flags*, p = 0 in air cells ----
int df_pressure_cg_direction2d_liquid(void* ws, int64_t ws_bytes, const uint8_t* flags, int64_t B, int64_t Y, int64_t X, int bnd, int64_t k,
                                      float accuracy, int64_t max_iter, df_stream_t stream) {
  return cg_direction<2, true, false, true>("df_pressure_cg_direction2d_liquid", ws, ws_bytes, flags, B, 1, Y, X, bnd, k, accuracy, max_iter, stream);
}
int df_pressure_cg_direction3d_liquid(void* ws, int64_t ws_bytes, const uint8_t* flags, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd,
                                      int64_t k, float accuracy, int64_t max_iter, df_stream_t stream) {
  return cg_direction<3, true, false, true>("df_pressure_cg_direction3d_liquid", ws, ws_bytes, flags, B, Z, Y, X, bnd, k, accuracy, max_iter, stream);
}
int df_pressure_correct2d_liquid(const float* vel, const float* pressure, float* out, const uint8_t* flags, int64_t B, int64_t Y, int64_t X,
                                 int bnd, df_stream_t stream) {
  return pressure_correct<2, true, false, true>("df_pressure_correct2d_liquid", vel, pressure, out, flags, B, 1, Y, X, bnd, stream);
}
int df_pressure_correct3d_liquid(const float* vel, const float* pressure, float* out, const uint8_t* flags, int64_t B, int64_t Z, int64_t Y,
                                 int64_t X, int bnd, df_stream_t stream) {
  return pressure_correct<3, true, false, true>("df_pressure_correct3d_liquid", vel, pressure, out, flags, B, Z, Y, X, bnd, stream);
}
// ---- the ghost-fluid free-surface projection: phi beside the flags, Jacobi-preconditioned CG, diag and z behind the plain workspace ----
int64_t df_pressure_workspace_bytes_gf(int64_t B, int64_t Z, int64_t Y, int64_t X) {
  const int64_t cg = df_pressure_workspace_bytes(B, Z, Y, X);
  return cg < 0 ? cg : cg + 8 * B * Z * Y * X;
}
int df_pressure_init2d_gf(const float* vel, float* pressure, void* ws, int64_t ws_bytes, const uint8_t* flags, const float* phi, int64_t B,
                          int64_t Y, int64_t X, int bnd, float gf_clamp, df_stream_t stream) {
  return pressure_init_gf_<2>("df_pressure_init2d_gf", vel, pressure, ws, ws_bytes, flags, phi, B, 1, Y, X, bnd, gf_clamp, stream);
}
int df_pressure_init3d_gf(const float* vel, float* pressure, void* ws, int64_t ws_bytes, const uint8_t* flags, const float* phi, int64_t B,
                          int64_t Z, int64_t Y, int64_t X, int bnd, float gf_clamp, df_stream_t stream) {
  return pressure_init_gf_<3>("df_pressure_init3d_gf", vel, pressure, ws, ws_bytes, flags, phi, B, Z, Y, X, bnd, gf_clamp, stream);
}
int df_pressure_cg_direction2d_gf(void* ws, int64_t ws_bytes, const uint8_t* flags, int64_t B, int64_t Y, int64_t X, int bnd, int64_t k,
                                  float accuracy, int64_t max_iter, df_stream_t stream) {
  return cg_direction<2, true, false, false, kRowDiag>("df_pressure_cg_direction2d_gf", ws, ws_bytes, flags, B, 1, Y, X, bnd, k, accuracy, max_iter, stream);
}
int df_pressure_cg_direction3d_gf(void* ws, int64_t ws_bytes, const uint8_t* flags, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd,
                                  int64_t k, float accuracy, int64_t max_iter, df_stream_t stream) {
  return cg_direction<3, true, false, false, kRowDiag>("df_pressure_cg_direction3d_gf", ws, ws_bytes, flags, B, Z, Y, X, bnd, k, accuracy, max_iter, stream);
}
int df_pressure_cg_update2d_gf(float* pressure, void* ws, int64_t ws_bytes, const uint8_t* flags, int64_t B, int64_t Y, int64_t X, int bnd,
                               int64_t k, df_stream_t stream) {
  return cg_update<2, true, kLeaveJacobi>("df_pressure_cg_update2d_gf", pressure, ws, ws_bytes, flags, B, 1, Y, X, bnd, k, stream);
}
int df_pressure_cg_update3d_gf(float* pressure, void* ws, int64_t ws_bytes, const uint8_t* flags, int64_t B, int64_t Z, int64_t Y, int64_t X,
                               int bnd, int64_t k, df_stream_t stream) {
  return cg_update<3, true, kLeaveJacobi>("df_pressure_cg_update3d_gf", pressure, ws, ws_bytes, flags, B, Z, Y, X, bnd, k, stream);
}
int df_pressure_correct2d_gf(const float* vel, const float* pressure, float* out, const uint8_t* flags, const float* phi, int64_t B, int64_t Y,
                             int64_t X, int bnd, float gf_clamp, df_stream_t stream) {
  return pressure_correct_gf_<2>("df_pressure_correct2d_gf", vel, pressure, out, flags, phi, B, 1, Y, X, bnd, gf_clamp, stream);
}
int df_pressure_correct3d_gf(const float* vel, const float* pressure, float* out, const uint8_t* flags, const float* phi, int64_t B, int64_t Z,
                             int64_t Y, int64_t X, int bnd, float gf_clamp, df_stream_t stream) {
  return pressure_correct_gf_<3>("df_pressure_correct3d_gf", vel, pressure, out, flags, phi, B, Z, Y, X, bnd, gf_clamp, stream);
}
// ---- implicit velocity diffusion (cgSolveDiffusion): the CG over the B*D components, alpha[B] in device memory ----
int64_t df_diffuse_workspace_bytes(int64_t B, int64_t Z, int64_t Y, int64_t X, int dim) {
  if (dim != 2 && dim != 3) return DF_EINVAL;
  if (B <= 0 || B >= (1 << 24) / dim) return B <= 0 ? DF_EINVAL : DF_ESHAPE;
  const int64_t cg = df_pressure_workspace_bytes(B * dim, Z, Y, X);
  return cg < 0 ? cg : cg + 4 * B * dim * Z * Y * X;
}
int df_diffuse_init2d(const float* vel, const float* alpha, void* ws, int64_t ws_bytes, int64_t B, int64_t Y, int64_t X, int bnd,
                      df_stream_t stream) {
  return diffuse_init<2>("df_diffuse_init2d", vel, alpha, ws, ws_bytes, B, 1, Y, X, bnd, stream);
}
int df_diffuse_init3d(const float* vel, const float* alpha, void* ws, int64_t ws_bytes, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd,
                      df_stream_t stream) {
  return diffuse_init<3>("df_diffuse_init3d", vel, alpha, ws, ws_bytes, B, Z, Y, X, bnd, stream);
}
int df_diffuse_cg_direction2d(const float* alpha, void* ws, int64_t ws_bytes, int64_t B, int64_t Y, int64_t X, int bnd, int64_t k,
                              float accuracy, int64_t max_iter, df_stream_t stream) {
  return diffuse_direction<2>("df_diffuse_cg_direction2d", alpha, ws, ws_bytes, B, 1, Y, X, bnd, k, accuracy, max_iter, stream);
}
int df_diffuse_cg_direction3d(const float* alpha, void* ws, int64_t ws_bytes, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd, int64_t k,
                              float accuracy, int64_t max_iter, df_stream_t stream) {
  return diffuse_direction<3>("df_diffuse_cg_direction3d", alpha, ws, ws_bytes, B, Z, Y, X, bnd, k, accuracy, max_iter, stream);
}
int df_diffuse_cg_update2d(void* ws, int64_t ws_bytes, int64_t B, int64_t Y, int64_t X, int bnd, int64_t k, df_stream_t stream) {
  return diffuse_update<2>("df_diffuse_cg_update2d", ws, ws_bytes, B, 1, Y, X, bnd, k, stream);
}
int df_diffuse_cg_update3d(void* ws, int64_t ws_bytes, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd, int64_t k, df_stream_t stream) {
  return diffuse_update<3>("df_diffuse_cg_update3d", ws, ws_bytes, B, Z, Y, X, bnd, k, stream);
}
int df_diffuse_finish2d(void* ws, int64_t ws_bytes, float* out, int64_t B, int64_t Y, int64_t X, int bnd, df_stream_t stream) {
  return diffuse_finish<2>("df_diffuse_finish2d", ws, ws_bytes, out, B, 1, Y, X, bnd, stream);
}
int df_diffuse_finish3d(void* ws, int64_t ws_bytes, float* out, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd, df_stream_t stream) {
  return diffuse_finish<3>("df_diffuse_finish3d", ws, ws_bytes, out, B, Z, Y, X, bnd, stream);
}
int df_open_extrapolate2d(float* vel, int64_t B, int64_t Y, int64_t X, int bnd, int open_sides, df_stream_t stream) {
  return open_extrapolate<2>("df_open_extrapolate2d", vel, B, 1, Y, X, bnd, open_sides, stream);
}
int df_open_extrapolate3d(float* vel, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd, int open_sides, df_stream_t stream) {
  return open_extrapolate<3>("df_open_extrapolate3d", vel, B, Z, Y, X, bnd, open_sides, stream);
}
int df_density_sphere_source2d(const float* density, const float* centers, float radius, float value, float* out, int64_t B, int64_t Y,
                               int64_t X, df_stream_t stream) {
  return sphere_source<2>("df_density_sphere_source2d", density, centers, radius, value, out, B, 1, Y, X, stream);
}
int df_density_sphere_source3d(const float* density, const float* centers, float radius, float value, float* out, int64_t B, int64_t Z,
                               int64_t Y, int64_t X, df_stream_t stream) {
  return sphere_source<3>("df_density_sphere_source3d", density, centers, radius, value, out, B, Z, Y, X, stream);
}

}  // extern "C"
