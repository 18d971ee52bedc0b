// Shared pieces of the advection kernels (advect.hip: a cell-centred density; smoke.hip: the MAC velocity itself): the cell decode and
// the interp() / corner rule of the step definition in include/deepfluids_hip.h.  S is the stride, in floats, between neighbouring
// cells of the grid that is read: 1 for a density [B,(Z,)Y,X], D for one component of a velocity [B,(Z,)Y,X,D].
#ifndef DF_ADVECT_COMMON_HPP
#define DF_ADVECT_COMMON_HPP
#include <cmath>
#include <cstdint>

#include "df_common.hpp"

namespace dfadv {

struct AdvDims {
  int64_t ncell;   // B*Z*Y*X
  int Z, Y, X;     // Z = 1 in 2-D
  int bnd;
  float dt, vs;
};

template <int D>
struct Cell {
  int64_t idx;     // flat cell index
  int64_t base;    // flat index of cell (0,0,0) of this batch entry
  int p[3];        // i, j, k
  bool interior;
};

template <int D>
__device__ __forceinline__ Cell<D> decode(int64_t idx, const AdvDims& d) {
  Cell<D> c;
  c.idx = idx;
  const int64_t row = idx / d.X;
  c.p[0] = static_cast<int>(idx - row * d.X);
  const int64_t slab = row / d.Y;
  c.p[1] = static_cast<int>(row - slab * d.Y);
  c.p[2] = D == 3 ? static_cast<int>(slab % d.Z) : 0;
  c.base = idx - ((static_cast<int64_t>(c.p[2]) * d.Y + c.p[1]) * d.X + c.p[0]);
  c.interior = c.p[0] >= d.bnd && c.p[0] < d.X - d.bnd && c.p[1] >= d.bnd && c.p[1] < d.Y - d.bnd &&
               (D == 2 || (c.p[2] >= d.bnd && c.p[2] < d.Z - d.bnd));
  return c;
}

// one axis of interp(): q = p - 0.5, n = (int)q, s1 = q - n, s0 = 1 - s1; q < 0 -> (0, 1, 0); n >= ext - 1 -> (ext - 2, 0, 1)
__device__ __forceinline__ void axis_weights(float p, int ext, int& n, float& s0, float& s1) {
  const float q = p - 0.5f;
  if (!(q >= 0.0f)) {
    n = 0; s0 = 1.0f; s1 = 0.0f;
  } else if (q >= static_cast<float>(ext - 1)) {        // trunc(q) >= ext - 1
    n = ext - 2; s0 = 0.0f; s1 = 1.0f;
  } else {
    n = static_cast<int>(q);
    s1 = q - static_cast<float>(n);
    s0 = 1.0f - s1;
  }
}

// interp(g, pos) of one batch entry's grid g: tensor product over the 2^D corners, x innermost
template <int D, int S = 1>
__device__ __forceinline__ float interp(const float* __restrict__ g, const float* pos, const AdvDims& d) {
  int n[3];
  float s0[3], s1[3];
  axis_weights(pos[0], d.X, n[0], s0[0], s1[0]);
  axis_weights(pos[1], d.Y, n[1], s0[1], s1[1]);
  if (D == 3) axis_weights(pos[2], d.Z, n[2], s0[2], s1[2]);
  else n[2] = 0;
  const int64_t sx = S, sy = static_cast<int64_t>(d.X) * S, sz = static_cast<int64_t>(d.X) * d.Y * S;
  const float* q = g + ((static_cast<int64_t>(n[2]) * d.Y + n[1]) * d.X + n[0]) * S;
  const float r00 = s0[0] * q[0] + s1[0] * q[sx];
  const float r01 = s0[0] * q[sy] + s1[0] * q[sy + sx];
  const float r0 = s0[1] * r00 + s1[1] * r01;
  if (D == 2) return r0;
  const float r10 = s0[0] * q[sz] + s1[0] * q[sz + sx];
  const float r11 = s0[0] * q[sz + sy] + s1[0] * q[sz + sy + sx];
  const float r1 = s0[1] * r10 + s1[1] * r11;
  return s0[2] * r0 + s1[2] * r1;
}

// The obstacle flags of df_obstacle_flags*: one byte per cell, bit 0 = the cell is fluid (interior and no obstacle), bits 1-6 = its x-, x+,
// y-, y+, z-, z+ neighbour is fluid.  Component a of cell c is a kept face when c and c - e_a are both fluid.
constexpr unsigned kFluid = 1u;
__device__ __forceinline__ unsigned lo_bit(int a) { return 2u << (2 * a); }
__device__ __forceinline__ unsigned hi_bit(int a) { return 4u << (2 * a); }

// open_sides `os` of the `_open` entry points: bit 2a = the low side of axis a is open, bit 2a + 1 = its high side (the order of the flags
// byte's neighbour bits)
__device__ __forceinline__ bool open_lo(int os, int a) { return ((os >> (2 * a)) & 1) != 0; }
__device__ __forceinline__ bool open_hi(int os, int a) { return ((os >> (2 * a + 1)) & 1) != 0; }

// min / max of orig over the interior corners c, c+1 of the integer cell c = clamp(trunc(t), 0, ext - 2) per axis; with MASKED only
// those of them that are fluid (fl: the flags of this batch entry)
template <int D, int S = 1, bool MASKED = false>
__device__ __forceinline__ void corner_range(const float* __restrict__ g, const float* t, const AdvDims& d, float& mn, float& mx, bool& found,
                                             const uint8_t* __restrict__ fl = nullptr) {
  const int ext[3] = {d.X, d.Y, d.Z};
  int c[3] = {0, 0, 0};
#pragma unroll
  for (int a = 0; a < D; ++a) c[a] = static_cast<int>(fminf(fmaxf(t[a], 0.0f), static_cast<float>(ext[a] - 2)));
#pragma unroll
  for (int dz = 0; dz < (D == 3 ? 2 : 1); ++dz)
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const int x = c[0] + dx, y = c[1] + dy, z = c[2] + dz;
        bool in = x >= d.bnd && x < d.X - d.bnd && y >= d.bnd && y < d.Y - d.bnd && (D == 2 || (z >= d.bnd && z < d.Z - d.bnd));
        const int64_t at = (static_cast<int64_t>(z) * d.Y + y) * d.X + x;
        if (MASKED) in = in && (fl[at] & kFluid);
        if (in) {
          const float v = g[at * S];
          mn = found ? fminf(mn, v) : v;
          mx = found ? fmaxf(mx, v) : v;
          found = true;
        }
      }
}

// host side of the `_flags` entry points: two byte ranges share no byte
inline bool apart(const void* p, int64_t np, const void* q, int64_t nq) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a + static_cast<uintptr_t>(np) <= b || b + static_cast<uintptr_t>(nq) <= a;
}

// the flags of a `_flags` entry point: present, and sharing no byte with an array the launch writes (`out` may be null: none)
template <bool MASKED>
int check_flags(const char* fn, const uint8_t* flags, int64_t ncell, const void* out, int64_t out_bytes, const char* what) {
  if (!MASKED) return DF_OK;
  DF_REQUIRE(flags, DF_EINVAL, "%s: null flags", fn);
  DF_REQUIRE(!out || apart(flags, ncell, out, out_bytes), DF_EINVAL, "%s: the flags overlap the %s", fn, what);
  return DF_OK;
}

}  // namespace dfadv
#endif
