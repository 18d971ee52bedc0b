// Density advection through a generated velocity field: the `advect()` mode of the reference's scene scripts (scene/smoke_pos_size.py:45-109,
// scene/smoke3_vel_buo.py:49-125), which hands the step to mantaflow's advectSemiLagrange(order, boundaryWidth, clampMode).  Written for
// gfx950 from the step definition in include/deepfluids_hip.h; bit parity with mantaflow is NOT claimed (it cannot be run here).
//
//   density [B,(Z,)Y,X] fp32, velocity [B,(Z,)Y,X,C] fp32 with C = 2 | 3 MAC face values (component x of cell i on its low-x face), cell
//   (i,j,k) = [..,k,j,i].  A cell is interior when bnd <= index < extent - bnd on every axis, else it is on the band.
//
//   kernel A  sl:  fwd = SL(orig, dt)          interior: interp(orig, centre - dt*uc), band: 0
//   kernel B  mc:  bwd = SL(fwd, -dt) at the cell, cor = fwd + 0.5*(orig - bwd), min / max of orig around the traced-back cell, clamp --
//                  one pass, neither bwd nor cor is written.  An order-2 step is A then B; order 1 is A alone.
//   source:        out = mask ? value : d, its own element-wise kernel (in place when out == d): the gathers of A and B then read a
//                  plain array and need no mask traffic of their own.
//   image:         uint8(clip(255 * d, 0, 255)) (3-D: of the z mean, a sequential ascending fp32 sum divided by Z), rows flipped in y.
//
// One thread = one cell, threads along x.  The own velocity record (2 or 3 adjacent floats) is one 8- or 12-byte load; the +1 neighbours
// are the next cell's x, the next row's y and the next slice's z component, whose lines the neighbouring waves fetch anyway.  The
// trace-back offsets are data dependent, so the 2^d corners are plain gathers served by L1/L2 (the XCD-aware block remap keeps a z
// neighbourhood on one L2); no LDS.  Arithmetic is written in the order of the step definition, s0*a + s1*b per axis with x innermost,
// and the library is built with -ffp-contract=off: a NumPy fp32 restatement in that order reproduces it.
//
// Float -> int conversions are taken only of values already known to be inside the grid: a NaN or a huge velocity selects an edge
// cell, never an address outside the arrays.
#include <cmath>

#include "advect_common.hpp"
#include "df_common.hpp"
#include "stencil_common.hpp"

namespace {

using df::ceil_div;
using dfadv::AdvDims;
using dfadv::axis_weights;
using dfadv::Cell;
using dfadv::corner_range;
using dfadv::decode;
using dfadv::interp;
using dfst::f32x4;
using dfst::kThreads;
using dfst::xcd_block;

template <int D>
struct VelRec { float v[D]; };

// dt * uc of an interior cell: uc = (0.5 * (face(i) + face(i+1))) * vel_scale per axis
template <int D>
__device__ __forceinline__ void displacement(const float* __restrict__ vel, const Cell<D>& c, const AdvDims& d, float* du) {
  const float* v = vel + c.idx * D;
  const VelRec<D> own = *reinterpret_cast<const VelRec<D>*>(v);
  const int64_t sy = static_cast<int64_t>(d.X) * D;
  float nb[3];
  nb[0] = v[D];
  nb[1] = v[sy + 1];
  if (D == 3) nb[2] = v[sy * d.Y + 2];
#pragma unroll
  for (int a = 0; a < D; ++a) du[a] = d.dt * ((0.5f * (own.v[a] + nb[a])) * d.vs);
}

template <int D>
__global__ __launch_bounds__(kThreads) void advect_sl_kernel(const float* __restrict__ orig, const float* __restrict__ vel,
                                                             float* __restrict__ fwd, AdvDims d) {
  const int64_t idx = xcd_block(blockIdx.x, gridDim.x, 0) * kThreads + threadIdx.x;
  if (idx >= d.ncell) return;
  const Cell<D> c = decode<D>(idx, d);
  float r = 0.0f;
  if (c.interior) {
    float du[3], pos[3];
    displacement<D>(vel, c, d, du);
#pragma unroll
    for (int a = 0; a < D; ++a) pos[a] = (static_cast<float>(c.p[a]) + 0.5f) - du[a];
    r = interp<D>(orig + c.base, pos, d);
  }
  fwd[idx] = r;
}

// MASKED (df_advect_mc*_flags): the correction and the clamp where the cell is fluid, over fluid corners; other interior cells keep fwd
template <int D, int MODE, bool MASKED>
__global__ __launch_bounds__(kThreads) void advect_mc_kernel(const float* __restrict__ orig, const float* __restrict__ fwd,
                                                             const float* __restrict__ vel, float* __restrict__ out,
                                                             const uint8_t* __restrict__ flags, AdvDims d) {
  const int64_t idx = xcd_block(blockIdx.x, gridDim.x, 0) * kThreads + threadIdx.x;
  if (idx >= d.ncell) return;
  const Cell<D> c = decode<D>(idx, d);
  float r = 0.0f;
  if (MASKED && c.interior && !(flags[idx] & dfadv::kFluid)) {
    r = fwd[idx];
  } else if (c.interior) {
    float du[3], pos[3], t[3];
    displacement<D>(vel, c, d, du);
#pragma unroll
    for (int a = 0; a < D; ++a) pos[a] = (static_cast<float>(c.p[a]) + 0.5f) + du[a];
    const float f = fwd[idx];
    const float bwd = interp<D>(fwd + c.base, pos, d);
    const float cor = f + 0.5f * (orig[idx] - bwd);
    float mn = 0.0f, mx = 0.0f;
    bool found = false;
#pragma unroll
    for (int a = 0; a < D; ++a) t[a] = static_cast<float>(c.p[a]) - du[a];
    const uint8_t* fl = MASKED ? flags + c.base : nullptr;
    corner_range<D, 1, MASKED>(orig + c.base, t, d, mn, mx, found, fl);
    if (MODE == 1) {
#pragma unroll
      for (int a = 0; a < D; ++a) t[a] = static_cast<float>(c.p[a]) + du[a];
      corner_range<D, 1, MASKED>(orig + c.base, t, d, mn, mx, found, fl);
    }
    if (!found) r = f;
    else if (MODE == 2) r = (cor < mn || cor > mx) ? f : cor;
    else r = fminf(fmaxf(cor, mn), mx);
  }
  out[idx] = r;
}

__global__ __launch_bounds__(kThreads) void density_source_kernel(const float* d, const uint8_t* __restrict__ mask, float value, float* out,
                                                                  int64_t n) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i < n) out[i] = mask[i] ? value : d[i];
}

__device__ __forceinline__ uint32_t grey(float v) {
  const float s = v * 255.0f;
  return static_cast<uint32_t>(static_cast<int>(fminf(fmaxf(s, 0.0f), 255.0f)));
}

// one thread = four consecutive x of one output row (b, y): walks z in registers, stores one 32-bit word at row Y-1-y.
// VEC: X % 4 == 0 and 16-byte aligned input, 4-byte aligned output.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void density_image_kernel(const float* __restrict__ d, uint8_t* __restrict__ img, int64_t nquad, int Z,
                                                                 int Y, int X) {
  const int64_t q = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (q >= nquad) return;
  const int XQ = (X + 3) >> 2;
  const int64_t row = q / XQ;                       // b*Y + y
  const int x0 = 4 * static_cast<int>(q - row * XQ);
  const int64_t b = row / Y;
  const int y = static_cast<int>(row - b * Y);
  const int64_t sz = static_cast<int64_t>(Y) * X;
  const float* p = d + (b * Z * Y + y) * X + x0;
  uint8_t* o = img + (b * Y + (Y - 1 - y)) * X + x0;
  if (VEC) {
    f32x4 a = *reinterpret_cast<const f32x4*>(p);
    for (int z = 1; z < Z; ++z) a += *reinterpret_cast<const f32x4*>(p + z * sz);
    if (Z > 1) a = a / static_cast<float>(Z);
    *reinterpret_cast<uint32_t*>(o) = grey(a[0]) | (grey(a[1]) << 8) | (grey(a[2]) << 16) | (grey(a[3]) << 24);
  } else {
    for (int j = 0; j < 4 && x0 + j < X; ++j) {
      float a = p[j];
      for (int z = 1; z < Z; ++z) a += p[z * sz + j];
      if (Z > 1) a = a / static_cast<float>(Z);
      o[j] = static_cast<uint8_t>(grey(a));
    }
  }
}

int plan(const char* fn, int dim, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd, float dt, float vs, AdvDims* d, unsigned* nblk) {
  DF_REQUIRE(B > 0 && Z > 0 && Y > 0 && X > 0, DF_EINVAL, "%s: non-positive extent", fn);
  DF_REQUIRE(bnd >= 1, DF_EINVAL, "%s: boundary width must be >= 1 (got %d)", fn, bnd);
  DF_REQUIRE(Z < (1 << 24) && Y < (1 << 24) && X < (1 << 24), DF_ESHAPE, "%s: extent too large", fn);
  const int64_t need = 2 * static_cast<int64_t>(bnd) + 2;
  DF_REQUIRE(X >= need && Y >= need && (dim == 2 || Z >= need), DF_ESHAPE, "%s: every extent must be >= 2*bnd + 2 = %lld", fn,
             (long long)need);
  const int64_t n = B * Z * Y * X;
  DF_REQUIRE(ceil_div(n, kThreads) < (1ll << 31), DF_ESHAPE, "%s: extent too large", fn);
  *d = AdvDims{n, (int)Z, (int)Y, (int)X, bnd, dt, vs};
  *nblk = static_cast<unsigned>(ceil_div(n, kThreads));
  return DF_OK;
}

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

template <int D>
int advect_sl(const char* fn, const float* density, const float* vel, float* fwd, int64_t B, int64_t Z, int64_t Y, int64_t X, float dt,
              float vel_scale, int bnd, df_stream_t stream) {
  DF_REQUIRE(density && vel && fwd, DF_EINVAL, "%s: null %s", fn, !density ? "input" : !vel ? "velocity" : "output");
  AdvDims d;
  unsigned nblk;
  if (int e = plan(fn, D, B, Z, Y, X, bnd, dt, vel_scale, &d, &nblk)) return e;
  DF_REQUIRE(fwd != density, DF_EINVAL, "%s: the output must not be the input (the step gathers)", fn);
  DF_REQUIRE(aligned4(density) && aligned4(vel) && aligned4(fwd), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  hipLaunchKernelGGL((advect_sl_kernel<D>), dim3(nblk), dim3(kThreads), 0, df::as_stream(stream), density, vel, fwd, d);
  return df::launched(fn);
}

template <int D, bool MASKED>
int advect_mc(const char* fn, const float* orig, const float* fwd, const float* vel, float* out, const uint8_t* flags, int64_t B, int64_t Z,
              int64_t Y, int64_t X, float dt, float vel_scale, int bnd, int clamp_mode, df_stream_t stream) {
  DF_REQUIRE(orig && fwd && vel && out, DF_EINVAL, "%s: null %s", fn, !orig || !fwd ? "input" : !vel ? "velocity" : "output");
  DF_REQUIRE(clamp_mode == 1 || clamp_mode == 2, DF_EINVAL, "%s: clamp_mode must be 1 or 2 (got %d)", fn, clamp_mode);
  AdvDims d;
  unsigned nblk;
  if (int e = plan(fn, D, B, Z, Y, X, bnd, dt, vel_scale, &d, &nblk)) return e;
  DF_REQUIRE(out != orig && out != fwd, DF_EINVAL, "%s: the output must not be an input (the step gathers)", fn);
  if (int e = dfadv::check_flags<MASKED>(fn, flags, d.ncell, out, 4 * d.ncell, "output")) return e;
  DF_REQUIRE(aligned4(orig) && aligned4(fwd) && aligned4(vel) && aligned4(out), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  hipStream_t s = df::as_stream(stream);
  if (clamp_mode == 2) hipLaunchKernelGGL((advect_mc_kernel<D, 2, MASKED>), dim3(nblk), dim3(kThreads), 0, s, orig, fwd, vel, out, flags, d);
  else hipLaunchKernelGGL((advect_mc_kernel<D, 1, MASKED>), dim3(nblk), dim3(kThreads), 0, s, orig, fwd, vel, out, flags, d);
  return df::launched(fn);
}

int density_image(const char* fn, const float* d, uint8_t* img, int64_t B, int64_t Z, int64_t Y, int64_t X, df_stream_t stream) {
  DF_REQUIRE(d && img, DF_EINVAL, "%s: null %s", fn, d ? "output" : "input");
  DF_REQUIRE(B > 0 && Z > 0 && Y > 0 && X > 0, DF_EINVAL, "%s: non-positive extent", fn);
  DF_REQUIRE(Z < (1 << 24) && Y < (1 << 24) && X < (1 << 24), DF_ESHAPE, "%s: extent too large", fn);
  DF_REQUIRE(aligned4(d), DF_EALIGN, "%s: input must be 4-byte aligned", fn);
  const int64_t nquad = B * Y * ceil_div(X, 4);
  const int64_t nblk = ceil_div(nquad, kThreads);
  DF_REQUIRE(nblk < (1ll << 31), DF_ESHAPE, "%s: extent too large", fn);
  hipStream_t s = df::as_stream(stream);
  if (X % 4 == 0 && df::aligned16(d) && aligned4(img))
    hipLaunchKernelGGL((density_image_kernel<true>), dim3((unsigned)nblk), dim3(kThreads), 0, s, d, img, nquad, (int)Z, (int)Y, (int)X);
  else
    hipLaunchKernelGGL((density_image_kernel<false>), dim3((unsigned)nblk), dim3(kThreads), 0, s, d, img, nquad, (int)Z, (int)Y, (int)X);
  return df::launched(fn);
}

}  // namespace

extern "C" {

int df_advect_sl2d(const float* density, const float* vel, float* fwd, int64_t B, int64_t Y, int64_t X, float dt, float vel_scale, int bnd,
                   df_stream_t stream) {
  return advect_sl<2>("df_advect_sl2d", density, vel, fwd, B, 1, Y, X, dt, vel_scale, bnd, stream);
}

int df_advect_sl3d(const float* density, const float* vel, float* fwd, int64_t B, int64_t Z, int64_t Y, int64_t X, float dt,
                   float vel_scale, int bnd, df_stream_t stream) {
  return advect_sl<3>("df_advect_sl3d", density, vel, fwd, B, Z, Y, X, dt, vel_scale, bnd, stream);
}

int df_advect_mc2d(const float* orig, const float* fwd, const float* vel, float* out, int64_t B, int64_t Y, int64_t X, float dt,
                   float vel_scale, int bnd, int clamp_mode, df_stream_t stream) {
  return advect_mc<2, false>("df_advect_mc2d", orig, fwd, vel, out, nullptr, B, 1, Y, X, dt, vel_scale, bnd, clamp_mode, stream);
}

int df_advect_mc3d(const float* orig, const float* fwd, const float* vel, float* out, int64_t B, int64_t Z, int64_t Y, int64_t X, float dt,
                   float vel_scale, int bnd, int clamp_mode, df_stream_t stream) {
  return advect_mc<3, false>("df_advect_mc3d", orig, fwd, vel, out, nullptr, B, Z, Y, X, dt, vel_scale, bnd, clamp_mode, stream);
}

int df_advect_mc2d_flags(const float* orig, const float* fwd, const float* vel, float* out, const uint8_t* flags, int64_t B, int64_t Y,
                         int64_t X, float dt, float vel_scale, int bnd, int clamp_mode, df_stream_t stream) {
  return advect_mc<2, true>("df_advect_mc2d_flags", orig, fwd, vel, out, flags, B, 1, Y, X, dt, vel_scale, bnd, clamp_mode, stream);
}

int df_advect_mc3d_flags(const float* orig, const float* fwd, const float* vel, float* out, const uint8_t* flags, int64_t B, int64_t Z,
                         int64_t Y, int64_t X, float dt, float vel_scale, int bnd, int clamp_mode, df_stream_t stream) {
  return advect_mc<3, true>("df_advect_mc3d_flags", orig, fwd, vel, out, flags, B, Z, Y, X, dt, vel_scale, bnd, clamp_mode, stream);
}

int df_density_source(const float* density, const uint8_t* mask, float value, float* out, int64_t n, df_stream_t stream) {
  DF_REQUIRE(density && mask && out, DF_EINVAL, "df_density_source: null %s", !density ? "input" : !mask ? "mask" : "output");
  DF_REQUIRE(n > 0, DF_EINVAL, "df_density_source: non-positive extent");
  DF_REQUIRE(aligned4(density) && aligned4(out), DF_EALIGN, "df_density_source: pointers must be 4-byte aligned");
  const int64_t nblk = ceil_div(n, kThreads);
  DF_REQUIRE(nblk < (1ll << 31), DF_ESHAPE, "df_density_source: extent too large");
  hipLaunchKernelGGL(density_source_kernel, dim3((unsigned)nblk), dim3(kThreads), 0, df::as_stream(stream), density, mask, value, out, n);
  return df::launched("df_density_source");
}

int df_density_image2d(const float* density, uint8_t* img, int64_t B, int64_t Y, int64_t X, df_stream_t stream) {
  return density_image("df_density_image2d", density, img, B, 1, Y, X, stream);
}

int df_density_image3d(const float* density, uint8_t* img, int64_t B, int64_t Z, int64_t Y, int64_t X, df_stream_t stream) {
  return density_image("df_density_image3d", density, img, B, Z, Y, X, stream);
}

}  // extern "C"
