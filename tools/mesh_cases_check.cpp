// Runs all 256 sign patterns of one cube through deep_fluids_amd/csrc/mesh_cases.hpp -- the very functions mesh.hip's kernels call -- on
// the CPU, and compares every triangle with the table tests/liquid_mesh_ref.py prints.  Host only, no GPU, not part of pytest:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o mesh_cases_check tools/mesh_cases_check.cpp
//   python tests/liquid_mesh_ref.py --cases | ./mesh_cases_check
//
// Exit status 0 and "256 patterns, N triangles: ok" when every pattern agrees.
#include <cstdio>
#include <cstdlib>

#include "../deep_fluids_amd/csrc/mesh_cases.hpp"

static int fail(int pattern, const char* what) {
  std::fprintf(stderr, "pattern %d: %s\n", pattern, what);
  return 1;
}

int main() {
  using namespace dfmesh;
  long total = 0;
  for (int want = 0; want < 256; ++want) {
    int pattern, ntri;
    if (std::scanf("%d %d", &pattern, &ntri) != 2 || pattern != want) return fail(want, "table line missing or out of order");
    const unsigned cube8 = (unsigned)pattern;
    if (cube_triangle_count(cube8) != ntri || ntri > kMaxCubeTriangles) return fail(pattern, "cube triangle count differs");
    int seen = 0;
    for (int t = 0; t < kTets; ++t) {
      const unsigned in4 = tet_inside(cube8, t);
      const unsigned tri = tet_triangles(in4, tet_odd(t));
      const int n = popcount4(in4);
      const int expect = (n == 1 || n == 3) ? 1 : (n == 2 ? 2 : 0);
      if (triangles_count(tri) != expect || tet_triangle_count(in4) != expect) return fail(pattern, "tet triangle count is not 0/1/2 by inside corners");
      for (int f = 0; f < triangles_count(tri); ++f, ++seen) {
        int tet;
        if (std::scanf("%d", &tet) != 1 || tet != t) return fail(pattern, "triangle of another tet in the table");
        for (int s = 0; s < 3; ++s) {
          int owner, d;
          if (std::scanf("%d %d", &owner, &d) != 2) return fail(pattern, "short table line");
          const int e = triangles_edge(tri, 3 * f + s);
          if (e < 0 || e >= kTetEdges) return fail(pattern, "edge number out of range");
          const int own = edge_owner(t, e), dir = edge_dir(t, e);
          if (own < 0 || own > 6 || dir < 1 || dir > 7 || (own & dir) != 0) return fail(pattern, "edge is no grid edge of the cube");
          if (((cube8 >> own) & 1u) == ((cube8 >> (own | dir)) & 1u)) return fail(pattern, "triangle vertex on an edge that does not cross");
          if (own != owner || dir != d) return fail(pattern, "triangle vertex differs from the reference's");
        }
      }
    }
    if (seen != ntri) return fail(pattern, "triangle total differs");
    total += ntri;
  }
  // the rank of a direction in a crossing mask, against a plain count
  for (unsigned mask = 0; mask < 256; ++mask)
    for (int d = 1; d <= 7; ++d) {
      int n = 0;
      for (int b = 1; b < d; ++b) n += (mask >> (b - 1)) & 1u;
      if (edge_rank(mask, d) != n) return fail((int)mask, "edge_rank differs");
    }
  std::printf("256 patterns, %ld triangles: ok\n", total);
  return 0;
}
