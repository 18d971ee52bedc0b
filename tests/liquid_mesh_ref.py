"""NumPy restatement of the surface mesher defined in include/deepfluids_hip.h ("liquid surface meshes"): marching tetrahedra on the Kuhn
split of the cubes between cell centres.  ``extract(phi, ..., dtype=np.float64)`` is the reference; ``dtype=np.float32`` is the
op-for-op twin whose bits the kernels give (every operation on float32 scalars, in the order the header writes them).  The ordering
rules are the definition's: vertices by owner sample index, then direction; triangles by cube, tet, case order.

Plain loops: the tests use grids of a few thousand samples at the most.

``python tests/liquid_mesh_ref.py --cases`` prints, for the 256 sign patterns of one cube, the table tools/mesh_cases_check.cpp compares
the shared case header with: ``pattern ntri`` followed by ``tet owner d owner d owner d`` per triangle."""
import sys

import numpy as np

PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))     # (a, b, g), lexicographic, x < y < z


def parity(seq):
    """1 for an odd permutation, by counting inversions"""
    seq = list(seq)
    return sum(1 for i in range(len(seq)) for j in range(i + 1, len(seq)) if seq[i] > seq[j]) & 1


def tet_corners(t):
    """cube offsets (bit 0 = x, 1 = y, 2 = z) of p0..p3 of tet t"""
    a, b, _ = PERMS[t]
    return (0, 1 << a, (1 << a) | (1 << b), 7)


def tet_triangles(inside, odd):
    """the triangles of a tet whose corners p0..p3 are ``inside`` (4 bools): a list of triangles, each three corner pairs (i, j), i < j"""
    ins = [i for i in range(4) if inside[i]]
    out = [i for i in range(4) if not inside[i]]
    if len(ins) in (0, 4):
        return []
    if len(ins) in (1, 3):
        k = ins[0] if len(ins) == 1 else out[0]
        q = [i for i in range(4) if i != k]
        tris = [[(k, q[0]), (k, q[1]), (k, q[2])]]
        flip = parity([k] + q) ^ (1 if len(ins) == 3 else 0) ^ odd
    else:
        (i, j), (k, l) = ins, out
        tris = [[(i, k), (i, l), (j, l)], [(i, k), (j, l), (j, k)]]
        flip = parity([i, j, k, l]) ^ odd
    if flip:
        tris = [[tr[0], tr[2], tr[1]] for tr in tris]
    return [[(min(p), max(p)) for p in tr] for tr in tris]


def cube_triangles(pattern):
    """triangles of the cube whose corner o is inside iff bit o of ``pattern``: a list of (tet, [(owner offset, d)] * 3)"""
    res = []
    for t in range(6):
        c = tet_corners(t)
        for tr in tet_triangles([(pattern >> c[i]) & 1 for i in range(4)], parity(PERMS[t])):
            res.append((t, [(c[i], c[j] ^ c[i]) for i, j in tr]))
    return res


def _box(shape, bnd, closed):
    if closed and bnd < 1:
        raise ValueError("closed needs bnd >= 1")
    w = bnd - 1 if closed else bnd
    lo = [w] * 3
    hi = [shape[2 - a] - 1 - w for a in range(3)]                  # per axis x, y, z of a shape [Z,Y,X]
    if min(h - l for h, l in zip(hi, lo)) < 1:
        raise ValueError("bnd too wide")
    return lo, hi


def extract(phi, bnd=0, closed=False, closed_value=0.5, normals=False, dtype=np.float64, capacity=None):
    """phi [B,Z,Y,X] -> dict(vertices [V,3] dtype, faces [T,3] int32 local to their entry, normals [V,3] | None,
    vertex_start, face_start [B+1] int32)"""
    phi = np.asarray(phi)
    if phi.ndim != 4 or min(phi.shape[1:]) < 2:
        raise ValueError("phi must be [B,Z,Y,X] with every extent >= 2")
    F = dtype
    B, Z, Y, X = phi.shape
    ext = (X, Y, Z)
    lo, hi = _box((Z, Y, X), bnd, closed)
    s = phi.astype(F)
    if closed:
        outer = np.zeros((Z, Y, X), bool)
        for a in range(3):
            idx = np.arange(ext[a])
            sh = [1, 1, 1]
            sh[2 - a] = ext[a]
            outer |= ((idx <= lo[a]) | (idx >= hi[a])).reshape(sh)
        s = np.where(outer[None], np.fmax(s, F(closed_value)), s)
    inside = s < 0

    def grad(b, p):
        g = []
        for a in range(3):
            q0, q1 = list(p), list(p)
            has_lo, has_hi = p[a] > 0, p[a] + 1 < ext[a]
            q1[a] += 1 if has_hi else 0
            q0[a] -= 1 if has_lo else 0
            diff = s[b, q1[2], q1[1], q1[0]] - s[b, q0[2], q0[1], q0[0]]
            g.append(F(0.5) * diff if has_lo and has_hi else diff)
        return g

    verts, norms, faces, vstart, fstart = [], [], [], [0], [0]
    for b in range(B):
        index = {}                                                   # (x, y, z, d) -> local vertex row
        for z in range(lo[2], hi[2] + 1):
            for y in range(lo[1], hi[1] + 1):
                for x in range(lo[0], hi[0] + 1):
                    p = (x, y, z)
                    for d in range(1, 8):
                        q = tuple(p[a] + ((d >> a) & 1) for a in range(3))
                        if any(q[a] > hi[a] for a in range(3)) or inside[b, z, y, x] == inside[b, q[2], q[1], q[0]]:
                            continue
                        s0, s1 = s[b, z, y, x], s[b, q[2], q[1], q[0]]
                        t = s0 / (s0 - s1)
                        index[(x, y, z, d)] = len(verts) - vstart[b]
                        verts.append([(F(p[a]) + F(0.5)) + t if (d >> a) & 1 else F(p[a]) + F(0.5) for a in range(3)])
                        if normals:
                            g0, g1 = grad(b, p), grad(b, q)
                            n = [g0[a] + t * (g1[a] - g0[a]) for a in range(3)]
                            ln = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
                            norms.append([n[a] / ln for a in range(3)] if ln > 0 else [F(0)] * 3)
        for z in range(lo[2], hi[2]):
            for y in range(lo[1], hi[1]):
                for x in range(lo[0], hi[0]):
                    pattern = 0
                    for o in range(8):
                        if inside[b, z + ((o >> 2) & 1), y + ((o >> 1) & 1), x + (o & 1)]:
                            pattern |= 1 << o
                    if pattern in (0, 255):
                        continue
                    for _, tri in cube_triangles(pattern):
                        faces.append([index[(x + (o & 1), y + ((o >> 1) & 1), z + ((o >> 2) & 1), d)] for o, d in tri])
        vstart.append(len(verts))
        fstart.append(len(faces))
    if capacity is not None and (len(verts) > capacity[0] or len(faces) > capacity[1]):
        raise ValueError("needs capacity=(%d, %d)" % (len(verts), len(faces)))
    with np.errstate(all="ignore"):
        return {"vertices": np.asarray(verts, F).reshape(-1, 3), "faces": np.asarray(faces, np.int32).reshape(-1, 3),
                "normals": np.asarray(norms, F).reshape(-1, 3) if normals else None,
                "vertex_start": np.asarray(vstart, np.int32), "face_start": np.asarray(fstart, np.int32)}


def entry(mesh, b):
    v = slice(mesh["vertex_start"][b], mesh["vertex_start"][b + 1])
    return mesh["vertices"][v], mesh["faces"][mesh["face_start"][b]:mesh["face_start"][b + 1]]


# ---- what the tests ask of a mesh ------------------------------------------------------------------------------------------------------
def directed_edges(faces):
    """{(a, b): how often the directed edge a -> b occurs in the faces}"""
    count = {}
    for f in np.asarray(faces):
        for k in range(3):
            e = (int(f[k]), int(f[(k + 1) % 3]))
            count[e] = count.get(e, 0) + 1
    return count


def is_watertight(faces):
    """every undirected edge occurs exactly twice, once in each direction"""
    count = directed_edges(faces)
    return bool(count) and all(n == 1 and count.get((b, a), 0) == 1 for (a, b), n in count.items())


def components(n_vertices, faces):
    """connected surfaces: a list of (vertex count, edge count, face count)"""
    parent = list(range(n_vertices))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    for f in np.asarray(faces):
        for k in (1, 2):
            a, b = find(int(f[0])), find(int(f[k]))
            if a != b:
                parent[a] = b
    stats = {}
    for i in range(n_vertices):
        stats.setdefault(find(i), [0, set(), 0])[0] += 1
    for f in np.asarray(faces):
        r = stats[find(int(f[0]))]
        r[2] += 1
        for k in range(3):
            a, b = int(f[k]), int(f[(k + 1) % 3])
            r[1].add((min(a, b), max(a, b)))
    return [(v, len(e), t) for v, e, t in stats.values()]


def volume(vertices, faces):
    """divergence-theorem volume of a closed mesh wound with outward normals, in float64"""
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


# ---- the fields the tests share ---------------------------------------------------------------------------------------------------------
def sphere_phi(shape, centre, radius):
    """|x - centre| - radius at the cell centres of a grid [Z,Y,X] (centre xyz in grid units), float32"""
    z, y, x = np.meshgrid(*(np.arange(n) + 0.5 for n in shape), indexing="ij")
    return (np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius).astype(np.float32)


def random_phi(shape, seed):
    """a seeded smooth random field: a few low-frequency cosines, float32, both signs"""
    rng = np.random.RandomState(seed)
    z, y, x = np.meshgrid(*(np.arange(n) + 0.5 for n in shape), indexing="ij")
    f = np.zeros(shape)
    for _ in range(6):
        k = rng.uniform(0.3, 1.3, 3)
        f += rng.uniform(0.5, 1.0) * np.cos(k[0] * x + k[1] * y + k[2] * z + rng.uniform(0, 2 * np.pi))
    return (f / 2.0).astype(np.float32)


def all_cube_patterns():
    """phi [256,2,2,2]: entry p has -1 at corner o (x = bit 0, y = bit 1, z = bit 2) iff bit o of p, else +1"""
    phi = np.ones((256, 2, 2, 2), np.float32)
    for p in range(256):
        for o in range(8):
            if (p >> o) & 1:
                phi[p, (o >> 2) & 1, (o >> 1) & 1, o & 1] = -1.0
    return phi


if __name__ == "__main__":
    if sys.argv[1:] == ["--cases"]:
        for pattern in range(256):
            tris = cube_triangles(pattern)
            print(" ".join([str(pattern), str(len(tris))] + ["%d %s" % (t, " ".join("%d %d" % od for od in tri)) for t, tri in tris]))
    else:
        sys.exit("usage: liquid_mesh_ref.py --cases")
