// The inflow of the reference's scene/smoke3_vel_buo.py:222-223 -- densityInflow(noise, Cylinder) and Cylinder.applyToGrid(vel) -- written
// for gfx950 from the definition in include/deepfluids_hip.h ("the noise inflow and the cylinder stamp").  Bit parity with mantaflow is
// NOT claimed: it cannot be run here, and its NoiseField is wavelet noise read from a tile file; the seeded lattice value noise below is
// this project's own stand-in.  tests/smoke_inflow_ref.py restates the definition.
//
//   noise_inflow    one thread = one cell, x fastest across the lanes.  The entry's cylinder (2D+1 floats) is read through the scalar cache
//                   where a wave lies inside one entry.  A thread first tests the cylinder's bounding box, grown by sigma and one cell of
//                   slack, and copies when it is outside: at the scene's size (112 x 64 x 32, radius 9, half height 2.6) that is 98 % of
//                   the cells.  The others evaluate the signed distance and 2^D lattice hashes: integer and fp32 VALU only, no table,
//                   no LDS, no memory traffic beyond the one load and the one store, so no noise parameter can select an address.
//   cylinder_stamp  one thread = one cell and its D faces, the record read and written as one D-float access like the kernels of
//                   smoke.hip.
// Float -> int conversions are taken only of values clamped to +-2^30.
#include "advect_common.hpp"
#include "df_common.hpp"
#include "stencil_common.hpp"

namespace {

using df::ceil_div;
using dfadv::AdvDims;
using dfadv::apart;
using dfadv::Cell;
using dfadv::decode;
using dfst::kThreads;

template <int D>
struct VelRec { float v[D]; };

// a cylinder record as the header lays it out: centre, half-axis vector, radius; `ok` as the header defines a valid entry
template <int D>
struct Cyl {
  float c[D], a[D], zl, radius;
  bool ok;
};

template <int D>
__device__ __forceinline__ Cyl<D> load_cyl(const float* __restrict__ rec) {
  Cyl<D> s;
  float z[D];
  bool fin = true;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    s.c[k] = rec[k];
    z[k] = rec[D + k];
    fin = fin && fabsf(s.c[k]) < INFINITY && fabsf(z[k]) < INFINITY;
  }
  s.radius = rec[2 * D];
  float zl2 = z[0] * z[0] + z[1] * z[1];
  if (D == 3) zl2 = zl2 + z[2] * z[2];
  s.zl = sqrtf(zl2);
  s.ok = fin && fabsf(s.radius) < INFINITY && zl2 > 0.0f && zl2 < INFINITY;
#pragma unroll
  for (int k = 0; k < D; ++k) s.a[k] = z[k] / s.zl;
  return s;
}

// h = dot(q - centre, a) and r2 = max(|q - centre|^2 - h^2, 0)
template <int D>
__device__ __forceinline__ void axial(const Cyl<D>& s, const float* q, float& h, float& r2) {
  float d[D];
#pragma unroll
  for (int k = 0; k < D; ++k) d[k] = q[k] - s.c[k];
  h = d[0] * s.a[0] + d[1] * s.a[1];
  float d2 = d[0] * d[0] + d[1] * d[1];
  if (D == 3) {
    h = h + d[2] * s.a[2];
    d2 = d2 + d[2] * d[2];
  }
  r2 = fmaxf(d2 - h * h, 0.0f);
}

struct Noise {
  float pos_scale[3], pos_offset[3];
  float tq;                  // time_anim * time
  float val_offset, val_scale, clamp_neg, clamp_pos, inv_extent;
  uint32_t seed;
  int clamp;
};

__device__ __forceinline__ float lattice(uint32_t seed, uint32_t ix, uint32_t iy, uint32_t iz) {
  uint32_t h = seed ^ (ix * 0x8DA6B343u) ^ (iy * 0xD8163841u) ^ (iz * 0xCB1AB31Fu);
  h ^= h >> 16; h *= 0x7FEB352Du;
  h ^= h >> 15; h *= 0x846CA68Bu;
  h ^= h >> 16;
  return static_cast<float>(h >> 8) * 1.1920928955078125e-07f - 1.0f;   // 2^-23: exact, in [-1, 1)
}

__device__ __forceinline__ float lerp(float a, float b, float w) { return a + w * (b - a); }

template <int D>
__device__ __forceinline__ float noise_value(const Noise& n, const int* p) {
  uint32_t i0[3] = {0u, 0u, 0u};
  float w[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int k = 0; k < D; ++k) {
    float q = ((static_cast<float>(p[k]) * n.pos_scale[k]) * n.inv_extent + n.pos_offset[k]) + n.tq;
    q = fminf(fmaxf(q, -1073741824.0f), 1073741824.0f);     // a NaN becomes -2^30
    const float f = floorf(q), t = q - f;
    i0[k] = static_cast<uint32_t>(static_cast<int32_t>(f));
    w[k] = (t * t) * (3.0f - 2.0f * t);
  }
  float plane[2];
#pragma unroll
  for (int dz = 0; dz < (D == 3 ? 2 : 1); ++dz) {
    const uint32_t iz = D == 3 ? i0[2] + dz : 0u;
    const float r0 = lerp(lattice(n.seed, i0[0], i0[1], iz), lattice(n.seed, i0[0] + 1u, i0[1], iz), w[0]);
    const float r1 = lerp(lattice(n.seed, i0[0], i0[1] + 1u, iz), lattice(n.seed, i0[0] + 1u, i0[1] + 1u, iz), w[0]);
    plane[dz] = lerp(r0, r1, w[1]);
  }
  float v = D == 3 ? lerp(plane[0], plane[1], w[2]) : plane[0];
  v = (v + n.val_offset) * n.val_scale;
  if (n.clamp) v = fminf(fmaxf(v, n.clamp_neg), n.clamp_pos);
  return v;
}

template <int D>
__global__ __launch_bounds__(kThreads) void noise_inflow_kernel(const float* density, float* out, const float* __restrict__ cyl, Noise n,
                                                                float scale, float sigma, AdvDims d) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (idx >= d.ncell) return;
  const Cell<D> c = decode<D>(idx, d);
  const float rho = density[idx];
  float res = rho;
  if (c.interior) {
    const Cyl<D> s = load_cyl<D>(cyl + c.base / (static_cast<int64_t>(d.X) * d.Y * d.Z) * (2 * D + 1));
    float q[D];
    // the region sdf <= sigma lies within sqrt(|z|^2 + radius^2) + sigma of the centre: beyond that plus one cell, copy
    const float reach = (s.zl + fabsf(s.radius)) + (sigma + 1.0f);
    bool near = s.ok;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      q[k] = static_cast<float>(c.p[k]);
      near = near && fabsf(q[k] - s.c[k]) <= reach;
    }
    if (near) {
      float h, r2;
      axial<D>(s, q, h, r2);
      const float dh = fabsf(h) - s.zl, dr = sqrtf(r2) - s.radius;
      const float oh = fmaxf(dh, 0.0f), orr = fmaxf(dr, 0.0f);
      const float sdf = fminf(fmaxf(dh, dr), 0.0f) + sqrtf(oh * oh + orr * orr);
      if (sdf <= sigma) {
        const float factor = fminf(fmaxf(1.0f - (0.5f / sigma) * (sdf + sigma), 0.0f), 1.0f);
        const float target = (noise_value<D>(n, c.p) * scale) * factor;
        res = target > rho ? target : rho;
      }
    }
  }
  out[idx] = res;
}

template <int D>
__global__ __launch_bounds__(kThreads) void cylinder_stamp_kernel(const float* vel, const float* __restrict__ cyl,
                                                                  const float* __restrict__ values, float* out, AdvDims d) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (idx >= d.ncell) return;
  const Cell<D> c = decode<D>(idx, d);
  const int64_t e = c.base / (static_cast<int64_t>(d.X) * d.Y * d.Z);
  const Cyl<D> s = load_cyl<D>(cyl + e * (2 * D + 1));
  VelRec<D> r = *reinterpret_cast<const VelRec<D>*>(vel + idx * D);
#pragma unroll
  for (int a = 0; a < D; ++a) {
    float q[D], h, r2;
#pragma unroll
    for (int k = 0; k < D; ++k) q[k] = k == a ? static_cast<float>(c.p[k]) : static_cast<float>(c.p[k]) + 0.5f;
    axial<D>(s, q, h, r2);
    if (s.ok && fabsf(h) <= s.zl && r2 < s.radius * s.radius) r.v[a] = values[e * D + a];
  }
  *reinterpret_cast<VelRec<D>*>(out + idx * D) = r;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

int plan(const char* fn, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd, AdvDims* d, unsigned* nblk) {
  DF_REQUIRE(B > 0 && Z > 0 && Y > 0 && X > 0, DF_EINVAL, "%s: non-positive extent", fn);
  DF_REQUIRE(B < (1 << 24) && Z < (1 << 24) && Y < (1 << 24) && X < (1 << 24) && Z * Y * X < (1ll << 40) / B, DF_ESHAPE,
             "%s: extent too large", fn);
  const int64_t n = B * Z * Y * X;
  DF_REQUIRE(ceil_div(n, kThreads) < (1ll << 31), DF_ESHAPE, "%s: extent too large", fn);
  *d = AdvDims{n, (int)Z, (int)Y, (int)X, bnd, 0.0f, 1.0f};
  *nblk = static_cast<unsigned>(ceil_div(n, kThreads));
  return DF_OK;
}

template <int D>
int noise_inflow(const char* fn, const float* density, float* out, const float* cyl, const df_noise_params* np, float time, float scale,
                 float sigma, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd, df_stream_t stream) {
  DF_REQUIRE(density && out && cyl && np, DF_EINVAL, "%s: null %s", fn, !density ? "density" : !out ? "output" : !cyl ? "cylinders" : "noise");
  DF_REQUIRE(sigma > 0.0f && sigma < INFINITY, DF_EINVAL, "%s: sigma must be a positive number", fn);
  DF_REQUIRE(bnd >= 0, DF_EINVAL, "%s: boundary width must be >= 0 (got %d)", fn, bnd);
  AdvDims d;
  unsigned nblk;
  if (int e = plan(fn, B, Z, Y, X, bnd, &d, &nblk)) return e;
  DF_REQUIRE(apart(cyl, 4 * B * (2 * D + 1), out, 4 * d.ncell), DF_EINVAL, "%s: the cylinders overlap the output", fn);
  DF_REQUIRE(aligned4(density) && aligned4(out) && aligned4(cyl), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  Noise n;
  for (int k = 0; k < 3; ++k) { n.pos_scale[k] = np->pos_scale[k]; n.pos_offset[k] = np->pos_offset[k]; }
  n.tq = np->time_anim * time;
  n.val_offset = np->val_offset; n.val_scale = np->val_scale;
  n.clamp_neg = np->clamp_neg; n.clamp_pos = np->clamp_pos;
  n.inv_extent = np->inv_extent; n.seed = np->seed; n.clamp = np->clamp ? 1 : 0;
  hipLaunchKernelGGL((noise_inflow_kernel<D>), dim3(nblk), dim3(kThreads), 0, df::as_stream(stream), density, out, cyl, n, scale, sigma, d);
  return df::launched(fn);
}

template <int D>
int cylinder_stamp(const char* fn, const float* vel, const float* cyl, const float* values, float* out, int64_t B, int64_t Z, int64_t Y,
                   int64_t X, df_stream_t stream) {
  DF_REQUIRE(vel && cyl && values && out, DF_EINVAL, "%s: null %s", fn, !vel ? "velocity" : !cyl ? "cylinders" : !values ? "values" : "output");
  AdvDims d;
  unsigned nblk;
  if (int e = plan(fn, B, Z, Y, X, 0, &d, &nblk)) return e;
  DF_REQUIRE(apart(cyl, 4 * B * (2 * D + 1), out, 4 * d.ncell * D), DF_EINVAL, "%s: the cylinders overlap the output", fn);
  DF_REQUIRE(apart(values, 4 * B * D, out, 4 * d.ncell * D), DF_EINVAL, "%s: the values overlap the output", fn);
  DF_REQUIRE(aligned4(vel) && aligned4(cyl) && aligned4(values) && aligned4(out), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  hipLaunchKernelGGL((cylinder_stamp_kernel<D>), dim3(nblk), dim3(kThreads), 0, df::as_stream(stream), vel, cyl, values, out, d);
  return df::launched(fn);
}

}  // namespace

extern "C" {

int df_density_noise_inflow2d(const float* density, float* out, const float* cyl, const df_noise_params* noise, float time, float scale,
                              float sigma, int64_t B, int64_t Y, int64_t X, int bnd, df_stream_t stream) {
  return noise_inflow<2>("df_density_noise_inflow2d", density, out, cyl, noise, time, scale, sigma, B, 1, Y, X, bnd, stream);
}
int df_density_noise_inflow3d(const float* density, float* out, const float* cyl, const df_noise_params* noise, float time, float scale,
                              float sigma, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd, df_stream_t stream) {
  return noise_inflow<3>("df_density_noise_inflow3d", density, out, cyl, noise, time, scale, sigma, B, Z, Y, X, bnd, stream);
}
int df_mac_cylinder_stamp2d(const float* vel, const float* cyl, const float* values, float* out, int64_t B, int64_t Y, int64_t X,
                            df_stream_t stream) {
  return cylinder_stamp<2>("df_mac_cylinder_stamp2d", vel, cyl, values, out, B, 1, Y, X, stream);
}
int df_mac_cylinder_stamp3d(const float* vel, const float* cyl, const float* values, float* out, int64_t B, int64_t Z, int64_t Y, int64_t X,
                            df_stream_t stream) {
  return cylinder_stamp<3>("df_mac_cylinder_stamp3d", vel, cyl, values, out, B, Z, Y, X, stream);
}

}  // extern "C"
