// The surface of a 3-D level set as an indexed triangle mesh: marching tetrahedra on the Kuhn split of the cubes between cell centres,
// written for gfx950 from the definition in include/deepfluids_hip.h ("liquid surface meshes").  The definition is this library's own, not
// mantaflow's marching cubes; tests/liquid_mesh_ref.py restates it and the kernels give the bits of its fp32 twin.  The case logic is
// mesh_cases.hpp, shared with the host.
//
//   phi [B,Z,Y,X] fp32;  mask, nvert, ntri [B*Z*Y*X] uint8;  vertex_offset, face_offset [B*Z*Y*X + 1] int32 (the exclusive sums of
//   nvert and ntri over the whole batch);  vertices, normals [V,3] fp32;  faces [T,3] int32.
//
//   count   one thread = one sample v: the effective values of v and of its seven upper neighbours v + d (x-fastest, so a wave reads
//           eight runs of consecutive floats, seven of them lines its neighbours read too), the crossing mask with the sample's own
//           sign in bit 7, the vertices it owns, the triangles of its cube.
//   emit    one thread = one sample again.  Its vertices: one per mask bit, at rows vertex_offset[v] + 0, 1, ...  Its cube's triangles,
//           at rows face_offset[v] + 0, 1, ...: the corner signs come from the mask alone (bit 7 and the crossings), the index of a
//           vertex from the owner's offset and the rank of its direction in the owner's mask, so the triangle half reads no phi.  A
//           thread whose mask has no crossing has neither vertices nor triangles and leaves after one byte.
//
// No atomics, no LDS, plain vector stores; every row index formed from device memory is checked against the capacity before the store.
#include <cmath>

#include "df_common.hpp"
#include "mesh_cases.hpp"
#include "particles_common.hpp"
#include "stencil_common.hpp"

namespace {

using df::ceil_div;
using dfpart::aligned4;
using dfpart::kInt32Max;
using dfst::kThreads;

struct MeshDims {
  int64_t n;        // B*Z*Y*X
  int64_t ncell;    // Z*Y*X
  int Z, Y, X;
  int lo[3], hi[3]; // the meshed box per axis (x, y, z), both ends included
  int closed;
  float closed_value;
};

// (x, y, z) of sample idx.  The host refuses 12 * n >= 2^31, so the index fits 32 bits: three 32-bit divisions, not 64-bit ones.
__device__ __forceinline__ uint32_t mesh_decode(int64_t idx, const MeshDims& d, int* p) {
  const uint32_t c = static_cast<uint32_t>(idx) % static_cast<uint32_t>(d.ncell);
  const uint32_t r = c / static_cast<uint32_t>(d.X);
  p[0] = static_cast<int>(c - r * static_cast<uint32_t>(d.X));
  p[2] = static_cast<int>(r / static_cast<uint32_t>(d.Y));
  p[1] = static_cast<int>(r - static_cast<uint32_t>(p[2]) * static_cast<uint32_t>(d.Y));
  return c;                                                      // the sample's index inside its batch entry
}

// the effective sample: with `closed`, a sample on the outer layer of the meshed box or beyond it reads max(phi, closed_value)
__device__ __forceinline__ float mesh_sample(const float* __restrict__ phi, int64_t idx, int x, int y, int z, const MeshDims& d) {
  float v = phi[idx];
  if (d.closed && (x <= d.lo[0] || x >= d.hi[0] || y <= d.lo[1] || y >= d.hi[1] || z <= d.lo[2] || z >= d.hi[2])) v = fmaxf(v, d.closed_value);
  return v;
}

__global__ __launch_bounds__(kThreads) void mesh_count_kernel(const float* __restrict__ phi, uint8_t* __restrict__ mask,
                                                              uint8_t* __restrict__ nvert, uint8_t* __restrict__ ntri, MeshDims d) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (idx >= d.n) return;
  int p[3];
  mesh_decode(idx, d, p);
  unsigned m = 0u, tris = 0u;
  bool in_box = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) in_box = in_box && p[a] >= d.lo[a] && p[a] <= d.hi[a];
  if (in_box) {
    const int64_t st[3] = {1, d.X, static_cast<int64_t>(d.X) * d.Y};
    const bool up[3] = {p[0] < d.hi[0], p[1] < d.hi[1], p[2] < d.hi[2]};      // the neighbour along +a is in the box
    const bool in0 = mesh_sample(phi, idx, p[0], p[1], p[2], d) < 0.0f;
    unsigned cube8 = in0 ? 1u : 0u;
#pragma unroll
    for (int o = 1; o < 8; ++o) {
      const bool ok = (!(o & 1) || up[0]) && (!(o & 2) || up[1]) && (!(o & 4) || up[2]);
      if (ok) {
        const int64_t j = idx + (o & 1) * st[0] + ((o >> 1) & 1) * st[1] + ((o >> 2) & 1) * st[2];
        const bool in = mesh_sample(phi, j, p[0] + (o & 1), p[1] + ((o >> 1) & 1), p[2] + ((o >> 2) & 1), d) < 0.0f;
        if (in != in0) m |= 1u << (o - 1);
        if (in) cube8 |= 1u << o;
      }
    }
    if (up[0] && up[1] && up[2]) tris = static_cast<unsigned>(dfmesh::cube_triangle_count(cube8));
    if (in0) m |= 128u;
  }
  mask[idx] = static_cast<uint8_t>(m);
  nvert[idx] = static_cast<uint8_t>(__popc(m & 127u));
  ntri[idx] = static_cast<uint8_t>(tris);
}

// central difference of the effective samples along axis a at sample (p, idx), one-sided on the grid's border
__device__ __forceinline__ float mesh_diff(const float* __restrict__ phi, int64_t idx, const int* p, int a, int64_t stride, int ext,
                                           const MeshDims& d) {
  int q[3] = {p[0], p[1], p[2]};
  const bool has_lo = p[a] > 0, has_hi = p[a] + 1 < ext;
  q[a] = p[a] + (has_hi ? 1 : 0);
  const float hi = mesh_sample(phi, idx + (has_hi ? stride : 0), q[0], q[1], q[2], d);
  q[a] = p[a] - (has_lo ? 1 : 0);
  const float lo = mesh_sample(phi, idx - (has_lo ? stride : 0), q[0], q[1], q[2], d);
  const float diff = hi - lo;
  return has_lo && has_hi ? 0.5f * diff : diff;
}

template <bool NORMALS>
__global__ __launch_bounds__(kThreads) void mesh_emit_kernel(const float* __restrict__ phi, const uint8_t* __restrict__ mask,
                                                             const int32_t* __restrict__ voff, const int32_t* __restrict__ foff,
                                                             float* __restrict__ vertices, float* __restrict__ normals,
                                                             int32_t* __restrict__ faces, int64_t vcap, int64_t fcap, MeshDims d) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (idx >= d.n) return;
  unsigned m0 = mask[idx];
  if ((m0 & 127u) == 0u) return;                               // no crossing edge: no vertex, and a cube of one sign
  int p[3];
  const uint32_t cell = mesh_decode(idx, d, p);
  const int ext[3] = {d.X, d.Y, d.Z};
  const int64_t st[3] = {1, d.X, static_cast<int64_t>(d.X) * d.Y};
  // a mask bit is believed only where the edge exists by the sample's index: whatever the byte holds, no sample outside the box is read
  bool in_box = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) in_box = in_box && p[a] >= d.lo[a] && p[a] <= d.hi[a];
  const bool up[3] = {p[0] < d.hi[0], p[1] < d.hi[1], p[2] < d.hi[2]};
  unsigned allowed = 128u;
#pragma unroll
  for (int o = 1; o < 8; ++o)
    if ((!(o & 1) || up[0]) && (!(o & 2) || up[1]) && (!(o & 4) || up[2])) allowed |= 1u << (o - 1);
  m0 &= in_box ? allowed : 0u;
  if ((m0 & 127u) == 0u) return;

  // ---- the vertices this sample owns ----
  const int64_t vrow0 = voff[idx];
  const float s0 = mesh_sample(phi, idx, p[0], p[1], p[2], d);
  float g0[3] = {0.0f, 0.0f, 0.0f};
  if (NORMALS) {
#pragma unroll
    for (int a = 0; a < 3; ++a) g0[a] = mesh_diff(phi, idx, p, a, st[a], ext[a], d);
  }
  int k = 0;
#pragma unroll
  for (int o = 1; o < 8; ++o) {
    if (m0 & (1u << (o - 1))) {
      const int q[3] = {p[0] + (o & 1), p[1] + ((o >> 1) & 1), p[2] + ((o >> 2) & 1)};
      const int64_t j = idx + (o & 1) * st[0] + ((o >> 1) & 1) * st[1] + ((o >> 2) & 1) * st[2];
      const float s1 = mesh_sample(phi, j, q[0], q[1], q[2], d);
      const float t = s0 / (s0 - s1);
      const int64_t row = vrow0 + k;
      ++k;
      if (row >= 0 && row < vcap) {
        float* v = vertices + 3 * row;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const float base = static_cast<float>(p[a]) + 0.5f;
          v[a] = ((o >> a) & 1) ? base + t : base;
        }
        if (NORMALS) {
          float nrm[3];
#pragma unroll
          for (int a = 0; a < 3; ++a) {
            const float g1 = mesh_diff(phi, j, q, a, st[a], ext[a], d);
            nrm[a] = g0[a] + t * (g1 - g0[a]);
          }
          const float len = sqrtf((nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2]);
          const bool ok = len > 0.0f;
          float* w = normals + 3 * row;
#pragma unroll
          for (int a = 0; a < 3; ++a) w[a] = ok ? nrm[a] / len : 0.0f;
        }
      }
    }
  }

  // ---- the triangles of the cube this sample is corner of ----
  if (!(up[0] && up[1] && up[2])) return;
  const int32_t base = voff[idx - cell];                         // faces are local to their batch entry
  unsigned cube8 = 0u;
  const unsigned in0 = m0 >> 7;
#pragma unroll
  for (int o = 0; o < 8; ++o) cube8 |= (o == 0 ? in0 : in0 ^ ((m0 >> (o - 1)) & 1u)) << o;
  unsigned cm[7];                                                // mask and local vertex offset of the seven owning corners
  int32_t cv[7];
  cm[0] = m0;
  cv[0] = static_cast<int32_t>(vrow0) - base;
#pragma unroll
  for (int o = 1; o < 7; ++o) {
    const int64_t j = idx + (o & 1) * st[0] + ((o >> 1) & 1) * st[1] + ((o >> 2) & 1) * st[2];
    cm[o] = mask[j];
    cv[o] = voff[j] - base;
  }
  int64_t frow = foff[idx];
#pragma unroll
  for (int t = 0; t < dfmesh::kTets; ++t) {
    const unsigned tri = dfmesh::tet_triangles(dfmesh::tet_inside(cube8, t), dfmesh::tet_odd(t));
    const int nt = dfmesh::triangles_count(tri);
    if (nt == 0) continue;
    int32_t ve[dfmesh::kTetEdges];
#pragma unroll
    for (int e = 0; e < dfmesh::kTetEdges; ++e) {
      const int own = dfmesh::edge_owner(t, e), dir = dfmesh::edge_dir(t, e);      // compile-time after unrolling
      ve[e] = cv[own] + dfmesh::edge_rank(cm[own], dir);
    }
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      if (f < nt) {
        int32_t out[3];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          const int e = dfmesh::triangles_edge(tri, 3 * f + s);
          int32_t r = ve[0];
#pragma unroll
          for (int c = 1; c < dfmesh::kTetEdges; ++c) r = e == c ? ve[c] : r;
          out[s] = r;
        }
        if (frow >= 0 && frow < fcap) {
          int32_t* w = faces + 3 * frow;
          w[0] = out[0]; w[1] = out[1]; w[2] = out[2];
        }
        ++frow;
      }
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
int mesh_dims(const char* fn, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd, int closed, float closed_value, MeshDims* d) {
  DF_REQUIRE(B > 0 && Z > 0 && Y > 0 && X > 0, DF_EINVAL, "%s: non-positive extent", fn);
  DF_REQUIRE(X >= 2 && Y >= 2 && Z >= 2, DF_ESHAPE, "%s: every extent must be >= 2", fn);
  DF_REQUIRE(Z < (1 << 24) && Y < (1 << 24) && X < (1 << 24), DF_ESHAPE, "%s: extent too large", fn);
  DF_REQUIRE(bnd >= 0, DF_EINVAL, "%s: bnd must be >= 0 (got %d)", fn, bnd);
  DF_REQUIRE(closed == 0 || closed == 1, DF_EINVAL, "%s: closed must be 0 or 1 (got %d)", fn, closed);
  DF_REQUIRE(!closed || bnd >= 1, DF_EINVAL, "%s: closed needs bnd >= 1 (the capped layer is the box's own outer layer)", fn);
  DF_REQUIRE(!closed || (closed_value > 0.0f && std::isfinite(closed_value)), DF_EINVAL,
             "%s: closed_value must be finite and > 0 (an outside value), got %g", fn, (double)closed_value);
  const int64_t w = closed ? bnd - 1 : bnd;                      // bnd'
  const int64_t least = Z < Y ? (Z < X ? Z : X) : (Y < X ? Y : X);
  DF_REQUIRE(least - 1 - 2 * w >= 1, DF_ESHAPE, "%s: bnd = %d is too wide for a grid %lldx%lldx%lld: the meshed box has no cube", fn, bnd,
             (long long)Z, (long long)Y, (long long)X);
  const int64_t ncell = Z * Y * X;
  DF_REQUIRE(ncell <= kInt32Max / 12 / B, DF_ESHAPE, "%s: B*Z*Y*X = %lld samples: 12 triangles per sample do not fit an int32 offset", fn,
             (long long)(B * ncell));
  d->n = B * ncell;
  d->ncell = ncell;
  d->Z = (int)Z; d->Y = (int)Y; d->X = (int)X;
  const int ext[3] = {(int)X, (int)Y, (int)Z};
  for (int a = 0; a < 3; ++a) {
    d->lo[a] = (int)w;
    d->hi[a] = ext[a] - 1 - (int)w;
  }
  d->closed = closed;
  d->closed_value = closed ? closed_value : 0.0f;
  return DF_OK;
}

}  // namespace

extern "C" {

int64_t df_mesh_capacity_bound(int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd, int closed, int what) {
  const char* fn = "df_mesh_capacity_bound";
  MeshDims d = {};
  if (int e = mesh_dims(fn, B, Z, Y, X, bnd, closed, 1.0f, &d)) return e;
  DF_REQUIRE(what == 0 || what == 1, DF_EINVAL, "%s: what must be 0 (vertices) or 1 (triangles), got %d", fn, what);
  const int64_t m[3] = {d.hi[0] - d.lo[0] + 1, d.hi[1] - d.lo[1] + 1, d.hi[2] - d.lo[2] + 1};   // samples of the box per axis
  if (what == 1) return B * dfmesh::kMaxCubeTriangles * (m[0] - 1) * (m[1] - 1) * (m[2] - 1);
  int64_t edges = 0;
  for (int o = 1; o < 8; ++o) edges += (m[0] - (o & 1)) * (m[1] - ((o >> 1) & 1)) * (m[2] - ((o >> 2) & 1));
  return B * edges;
}

int df_mesh_count(const float* phi, uint8_t* mask, uint8_t* nvert, uint8_t* ntri, int64_t B, int64_t Z, int64_t Y, int64_t X, int bnd,
                  int closed, float closed_value, df_stream_t stream) {
  const char* fn = "df_mesh_count";
  DF_REQUIRE(phi && mask && nvert && ntri, DF_EINVAL, "%s: null %s", fn, !phi ? "phi" : (!mask ? "mask" : "counts"));
  MeshDims d = {};
  if (int e = mesh_dims(fn, B, Z, Y, X, bnd, closed, closed_value, &d)) return e;
  DF_REQUIRE(aligned4(phi), DF_EALIGN, "%s: phi must be 4-byte aligned", fn);
  const unsigned nblk = static_cast<unsigned>(ceil_div(d.n, kThreads));
  hipLaunchKernelGGL(mesh_count_kernel, dim3(nblk), dim3(kThreads), 0, df::as_stream(stream), phi, mask, nvert, ntri, d);
  return df::launched(fn);
}

int df_mesh_emit(const float* phi, const uint8_t* mask, const int32_t* vertex_offset, const int32_t* face_offset, float* vertices,
                 float* normals, int32_t* faces, int64_t vertex_capacity, int64_t face_capacity, int64_t B, int64_t Z, int64_t Y, int64_t X,
                 int bnd, int closed, float closed_value, df_stream_t stream) {
  const char* fn = "df_mesh_emit";
  DF_REQUIRE(phi && mask && vertex_offset && face_offset, DF_EINVAL, "%s: null %s", fn,
             !phi ? "phi" : (!mask ? "mask" : "offsets"));
  DF_REQUIRE(vertex_capacity >= 0 && face_capacity >= 0, DF_EINVAL, "%s: negative capacity", fn);
  DF_REQUIRE((vertices || vertex_capacity == 0) && (faces || face_capacity == 0), DF_EINVAL, "%s: null %s", fn, !vertices ? "vertices" : "faces");
  MeshDims d = {};
  if (int e = mesh_dims(fn, B, Z, Y, X, bnd, closed, closed_value, &d)) return e;
  DF_REQUIRE(vertex_capacity <= kInt32Max / 3 && face_capacity <= kInt32Max / 3, DF_ESHAPE, "%s: capacity too large", fn);
  DF_REQUIRE(aligned4(phi) && aligned4(vertex_offset) && aligned4(face_offset) && aligned4(vertices) && aligned4(normals) && aligned4(faces),
             DF_EALIGN, "%s: pointers must be 4-byte aligned", fn);
  const unsigned nblk = static_cast<unsigned>(ceil_div(d.n, kThreads));
  hipStream_t s = df::as_stream(stream);
  if (normals) hipLaunchKernelGGL((mesh_emit_kernel<true>), dim3(nblk), dim3(kThreads), 0, s, phi, mask, vertex_offset, face_offset, vertices,
                                  normals, faces, vertex_capacity, face_capacity, d);
  else hipLaunchKernelGGL((mesh_emit_kernel<false>), dim3(nblk), dim3(kThreads), 0, s, phi, mask, vertex_offset, face_offset, vertices,
                          normals, faces, vertex_capacity, face_capacity, d);
  return df::launched(fn);
}

}  // extern "C"
