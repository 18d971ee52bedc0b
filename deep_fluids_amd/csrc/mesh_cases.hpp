// The case logic of the surface mesher (mesh.hip): marching tetrahedra on the Kuhn split of a cube, as include/deepfluids_hip.h
// defines it.  Everything here is integer arithmetic on a few bits, written once for the device and the host: the kernels call these
// functions, and tools/mesh_cases_check.cpp runs all 256 sign patterns of a cube through them on the CPU.  No tables: every case is
// derived from the two rules below, and tests/test_liquid_mesh_host.py checks the result geometrically for every pattern.
//
//   cube offsets   a corner of the cube at c is c + o, o in 0..7 with bit 0 = x, bit 1 = y, bit 2 = z
//   tets           tet t = 0..5 is the permutation (a, b, g) of the axes in lexicographic order, x < y < z:
//                  xyz, xzy, yxz, yzx, zxy, zyx.  Its corners are p0 = c, p1 = c + e_a, p2 = c + e_a + e_b, p3 = c + (1,1,1);
//                  det(p1 - p0, p2 - p0, p3 - p0) is the permutation's sign, so t = 1, 2, 5 are the mirrored (odd) tets
//   tet edges      e = 0..5 for the corner pairs (i, j), i < j: 01, 02, 03, 12, 13, 23.  The offset of p_i is a subset of the offset of
//                  p_j, so the edge is the grid edge (owner, d) = (c + o_i, o_j ^ o_i)
//   triangles      with n inside corners (bit i of `in4` = p_i inside):
//                  n = 1, corner k inside, the others q1 < q2 < q3:  (k q1, k q2, k q3)
//                  n = 3, corner k outside:                          the same triangle
//                  n = 2, i < j inside, k < l outside:               (i k, i l, j l) and (i k, j l, j k), the quad split at i k -- j l
//                  each written with its last two vertices swapped when `flip`:
//                  flip = sigma ^ (n == 3) ^ (the tet is odd), sigma = the parity of the permutation (k, q1, q2, q3) resp. (i, j, k, l)
//                  of (0, 1, 2, 3).  In an even tet with p0 alone inside, (01, 02, 03) has its normal pointing away from p0; every
//                  other case is that one relabelled (sigma), mirrored (odd tet) or with inside and outside exchanged (n == 3).
#ifndef DF_MESH_CASES_HPP
#define DF_MESH_CASES_HPP

#if defined(__HIPCC__)
#define DF_MESH_HD __host__ __device__ inline
#else
#define DF_MESH_HD inline
#endif

namespace dfmesh {

constexpr int kTets = 6;
constexpr int kTetEdges = 6;
constexpr int kMaxCubeTriangles = 12;

// axis a and b of tet t (g is the remaining one), and whether the permutation is odd
DF_MESH_HD constexpr int tet_axis_a(int t) { return t >> 1; }
DF_MESH_HD constexpr int tet_axis_b(int t) { return ((1 | 2 << 2 | 0 << 4 | 2 << 6 | 0 << 8 | 1 << 10) >> (2 * t)) & 3; }
DF_MESH_HD constexpr bool tet_odd(int t) { return ((0 | 1 << 1 | 1 << 2 | 0 << 3 | 0 << 4 | 1 << 5) >> t) & 1; }

// cube offset of corner i = 0..3 of tet t
DF_MESH_HD constexpr int tet_corner(int t, int i) {
  return i == 0 ? 0 : (i == 1 ? 1 << tet_axis_a(t) : (i == 2 ? (1 << tet_axis_a(t)) | (1 << tet_axis_b(t)) : 7));
}

// the two corners (i < j) of tet edge e
DF_MESH_HD constexpr int edge_lo(int e) { return e < 3 ? 0 : (e < 5 ? 1 : 2); }
DF_MESH_HD constexpr int edge_hi(int e) { return e < 3 ? e + 1 : (e < 5 ? e - 1 : 3); }
// ... and the edge of a corner pair, in either order
DF_MESH_HD constexpr int edge_of(int p, int q) { return (p < q ? p : q) == 0 ? (p < q ? q : p) - 1 : p + q; }

// the grid edge of tet edge e: its owner's cube offset and its direction d = 1..7
DF_MESH_HD constexpr int edge_owner(int t, int e) { return tet_corner(t, edge_lo(e)); }
DF_MESH_HD constexpr int edge_dir(int t, int e) { return tet_corner(t, edge_hi(e)) ^ tet_corner(t, edge_lo(e)); }

// the inside bits of tet t's corners from those of the cube's (bit o of cube8 = corner c + o inside)
DF_MESH_HD constexpr unsigned tet_inside(unsigned cube8, int t) {
  return ((cube8 >> tet_corner(t, 0)) & 1u) | ((cube8 >> tet_corner(t, 1)) & 1u) << 1 | ((cube8 >> tet_corner(t, 2)) & 1u) << 2 |
         ((cube8 >> tet_corner(t, 3)) & 1u) << 3;
}

DF_MESH_HD constexpr int popcount4(unsigned v) { return (int)((v & 1u) + ((v >> 1) & 1u) + ((v >> 2) & 1u) + ((v >> 3) & 1u)); }
DF_MESH_HD constexpr int lowest4(unsigned v) { return (v & 1u) ? 0 : ((v & 2u) ? 1 : ((v & 4u) ? 2 : 3)); }
DF_MESH_HD constexpr int highest4(unsigned v) { return (v & 8u) ? 3 : ((v & 4u) ? 2 : ((v & 2u) ? 1 : 0)); }

// triangles of a tet with inside bits in4: 0, 1 or 2
DF_MESH_HD constexpr int tet_triangle_count(unsigned in4) {
  return (popcount4(in4) & 1) ? 1 : (popcount4(in4) == 2 ? 2 : 0);
}

// triangles of the cube with corner bits cube8: at most kMaxCubeTriangles
DF_MESH_HD constexpr int cube_triangle_count(unsigned cube8) {
  int n = 0;
  for (int t = 0; t < kTets; ++t) n += tet_triangle_count(tet_inside(cube8, t));
  return n;
}

// The triangles of a tet, packed: bits 3s .. 3s + 2 hold the tet edge of vertex slot s (slots 0..2 the first triangle, 3..5 the
// second), bits 18..19 the number of triangles.
DF_MESH_HD unsigned tet_triangles(unsigned in4, bool odd) {
  const int n = popcount4(in4);
  unsigned e0, e1, e2, e3 = 0u, e4 = 0u, e5 = 0u;
  bool flip = odd;
  if (n == 1 || n == 3) {
    const int k = lowest4(n == 1 ? in4 : ~in4 & 15u);
    const int q1 = k <= 0 ? 1 : 0, q2 = k <= 1 ? 2 : 1, q3 = k <= 2 ? 3 : 2;
    e0 = (unsigned)edge_of(k, q1); e1 = (unsigned)edge_of(k, q2); e2 = (unsigned)edge_of(k, q3);
    flip ^= (k & 1) != 0;
    flip ^= n == 3;
  } else if (n == 2) {
    const unsigned out = ~in4 & 15u;
    const int i = lowest4(in4), j = highest4(in4), k = lowest4(out), l = highest4(out);
    e0 = (unsigned)edge_of(i, k); e1 = (unsigned)edge_of(i, l); e2 = (unsigned)edge_of(j, l);
    e3 = e0; e4 = e2; e5 = (unsigned)edge_of(j, k);
    flip ^= (((i > k) + (i > l) + (j > k) + (j > l)) & 1) != 0;
  } else {
    return 0u;
  }
  if (flip) {
    unsigned s = e1; e1 = e2; e2 = s;
    s = e4; e4 = e5; e5 = s;
  }
  return e0 | e1 << 3 | e2 << 6 | e3 << 9 | e4 << 12 | e5 << 15 | (unsigned)tet_triangle_count(in4) << 18;
}

DF_MESH_HD constexpr int triangles_count(unsigned packed) { return (int)(packed >> 18) & 3; }
DF_MESH_HD constexpr int triangles_edge(unsigned packed, int slot) { return (int)(packed >> (3 * slot)) & 7; }

// vertices owned below direction d in a sample's crossing mask: the edge (v, d) is vertex number rank(mask, d) of v
DF_MESH_HD int edge_rank(unsigned mask, int d) { return __builtin_popcount(mask & ((1u << (d - 1)) - 1u)); }

}  // namespace dfmesh
#endif
