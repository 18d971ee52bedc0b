// Shared pieces of the particle kernels (particles.hip: trace, keys, level set; liquid.hip: the FLIP transfers): the particle record, the
// per-axis weights and the MAC sample u(p) of the step definition in include/deepfluids_hip.h, and the host checks of the extents.
#ifndef DF_PARTICLES_COMMON_HPP
#define DF_PARTICLES_COMMON_HPP
#include <cmath>
#include <cstdint>

#include "df_common.hpp"
#include "stencil_common.hpp"

namespace dfpart {

struct PartDims {
  int64_t total;   // B*N particles
  int64_t N;
  int64_t ncell;   // Z*Y*X cells of one batch entry
  int Z, Y, X;     // Z = 1 in 2-D
  float lo, hi[3]; // clamp of the traced position per axis (x, y, z)
  float dt, half_dt, vs;
};

template <int D>
struct Rec { float v[D]; };

// q < 0 or NaN -> (0; 1, 0); trunc(q) >= ext - 1 -> (ext - 2; 0, 1); else n = (int)q, s1 = q - n, s0 = 1 - s1
__device__ __forceinline__ void axis_weights(float q, int ext, int& n, float& s0, float& s1) {
  if (!(q >= 0.0f)) {
    n = 0; s0 = 1.0f; s1 = 0.0f;
  } else if (q >= static_cast<float>(ext - 1)) {
    n = ext - 2; s0 = 0.0f; s1 = 1.0f;
  } else {
    n = static_cast<int>(q);
    s1 = q - static_cast<float>(n);
    s0 = 1.0f - s1;
  }
}

// u(p) of one batch entry's MAC grid: component a is interpolated in the frame q_a = p_a, q_b = p_b - 0.5 (b != a), x innermost
template <int D>
__device__ __forceinline__ void mac_sample(const float* __restrict__ vel, const float* p, const PartDims& d, float* u) {
  const int ext[3] = {d.X, d.Y, d.Z};
  int nc[3], nf[3];                 // index in the cell-centred frame (p - 0.5) and in the face frame (p)
  float c0[3], c1[3], f0[3], f1[3];
#pragma unroll
  for (int a = 0; a < D; ++a) {
    axis_weights(p[a] - 0.5f, ext[a], nc[a], c0[a], c1[a]);
    axis_weights(p[a], ext[a], nf[a], f0[a], f1[a]);
  }
  const int64_t sx = D, sy = static_cast<int64_t>(d.X) * D, sz = sy * d.Y;
#pragma unroll
  for (int a = 0; a < D; ++a) {
    int n[3] = {0, 0, 0};
    float s0[3], s1[3];
#pragma unroll
    for (int b = 0; b < D; ++b) {
      n[b] = b == a ? nf[b] : nc[b];
      s0[b] = b == a ? f0[b] : c0[b];
      s1[b] = b == a ? f1[b] : c1[b];
    }
    const float* q = vel + ((static_cast<int64_t>(n[2]) * d.Y + n[1]) * d.X + n[0]) * D + a;
    const float r00 = s0[0] * q[0] + s1[0] * q[sx];
    const float r01 = s0[0] * q[sy] + s1[0] * q[sy + sx];
    float r = s0[1] * r00 + s1[1] * r01;
    if (D == 3) {
      const float r10 = s0[0] * q[sz] + s1[0] * q[sz + sx];
      const float r11 = s0[0] * q[sz + sy] + s1[0] * q[sz + sy + sx];
      const float r1 = s0[1] * r10 + s1[1] * r11;
      r = s0[2] * r + s1[2] * r1;
    }
    u[a] = r * d.vs;
  }
}

// The entry of row idx of a ragged batch (the header's "ragged particle batches"): rows start[b] .. start[b+1] - 1 belong to entry b, so
// the entry is (the number of b in 0..B with start[b] <= idx) - 1, found by bisection over the B + 1 non-decreasing starts.  -1: the
// row is unused (idx >= start[B], or < start[0]).  Whatever the starts hold, the result lies in [-1, B - 1]: it selects a velocity
// grid, never memory outside the arrays.
__device__ __forceinline__ int ragged_entry(const int32_t* __restrict__ start, int B, int64_t idx) {
  int lo = 0, hi = B + 1;                                   // the count lies in [lo, hi]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;                         // < B + 1
    if (static_cast<int64_t>(start[mid]) <= idx) lo = mid + 1;
    else hi = mid;
  }
  return lo == B + 1 ? -1 : lo - 1;
}

// The integer mix of the lattice noise (the header's noise inflow block), keyed by four words; uint32 arithmetic mod 2^32.
__device__ __forceinline__ uint32_t mix4(uint32_t seed, uint32_t a, uint32_t b, uint32_t c) {
  uint32_t h = seed ^ (a * 0x8DA6B343u) ^ (b * 0xD8163841u) ^ (c * 0xCB1AB31Fu);
  h ^= h >> 16; h *= 0x7FEB352Du; h ^= h >> 15; h *= 0x846CA68Bu; h ^= h >> 16;
  return h;
}

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

constexpr int64_t kInt32Max = 2147483647ll;

// extents and particle counts shared by every entry point; `keyed`: the keys (and the ranges over them) must fit an int32
inline int check_dims(const char* fn, int dim, int64_t B, int64_t N, int64_t Z, int64_t Y, int64_t X, bool keyed) {
  DF_REQUIRE(B > 0 && Z > 0 && Y > 0 && X > 0 && N >= 0, DF_EINVAL, "%s: non-positive extent", fn);
  DF_REQUIRE(X >= 2 && Y >= 2 && (dim == 2 || Z >= 2), DF_ESHAPE, "%s: every extent must be >= 2", fn);
  DF_REQUIRE(Z < (1 << 24) && Y < (1 << 24) && X < (1 << 24), DF_ESHAPE, "%s: extent too large", fn);
  DF_REQUIRE(N <= kInt32Max / B, DF_ESHAPE, "%s: B*N does not fit an int32", fn);
  const int64_t ncell = Z * Y * X;
  if (keyed) DF_REQUIRE(ncell <= kInt32Max / B, DF_ESHAPE, "%s: B*Z*Y*X = %lld cells: the cell keys do not fit an int32", fn, (long long)(B * ncell));
  else DF_REQUIRE(df::ceil_div(B * ncell, dfst::kThreads) < (1ll << 31), DF_ESHAPE, "%s: extent too large", fn);
  return DF_OK;
}

// the entry_start argument of a ragged entry point ([B + 1] int32 in device memory; read by the kernels, never by the host)
inline int check_ragged(const char* fn, const int32_t* entry_start, bool ragged, int64_t N) {
  if (!ragged) return DF_OK;
  DF_REQUIRE(entry_start || N == 0, DF_EINVAL, "%s: null entry_start", fn);
  DF_REQUIRE(aligned4(entry_start), DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  return DF_OK;
}

}  // namespace dfpart
#endif
