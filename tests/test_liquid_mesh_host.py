"""The surface mesher's definition (include/deepfluids_hip.h, "liquid surface meshes") checked on the CPU through its NumPy restatement
tests/liquid_mesh_ref.py -- case logic, watertightness, volume -- and the parts of the public interface that need no device: the
refusals of ``ops.extract_surface``, the OBJ files of ``util``, the C ABI's size query and argument errors.  No GPU needed."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import liquid_mesh_ref as ref  # noqa: E402

from deep_fluids_amd import _lib, ops, util  # noqa: E402


def test_all_256_sign_patterns_of_one_cube():
    """256 grids of 2x2x2 with +-1 at the corners: per tet 0, 1 or 2 triangles by its inside corners; every triangle vertex on a
    crossing edge; every triangle's normal has a positive dot product with the phi difference across it (the gradient of the tet's
    linear interpolant, which is constant over the tet)."""
    phi = ref.all_cube_patterns()
    m = ref.extract(phi)
    total = 0
    for p in range(256):
        corner_in = [(p >> o) & 1 for o in range(8)]
        tris = ref.cube_triangles(p)
        per_tet = [sum(1 for t, _ in tris if t == k) for k in range(6)]
        for k in range(6):
            n = sum(corner_in[c] for c in ref.tet_corners(k))
            assert per_tet[k] == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[n], (p, k)
        assert len(tris) <= 12
        v, f = ref.entry(m, p)
        assert len(f) == len(tris)
        assert len(v) == sum(1 for o in range(8) for d in range(1, 8) if not (o & d) and corner_in[o] != corner_in[o | d])
        for (t, tri), face in zip(tris, f):
            for (own, d), row in zip(tri, face):
                assert 0 <= own <= 6 and 1 <= d <= 7 and not (own & d)
                assert corner_in[own] != corner_in[own | d], (p, t, own, d)           # the vertex lies on a crossing edge ...
                mid = np.array([(own >> a) & 1 for a in range(3)]) + 0.5 + 0.5 * np.array([(d >> a) & 1 for a in range(3)])
                np.testing.assert_array_equal(v[row], mid)                            # ... at its middle, for values +-1
            c = ref.tet_corners(t)
            pts = np.array([[(o >> a) & 1 for a in range(3)] for o in c], np.float64)
            val = np.array([-1.0 if corner_in[o] else 1.0 for o in c])
            grad = np.linalg.solve(pts[1:] - pts[0], val[1:] - val[0])               # of the linear interpolant on the tet
            normal = np.cross(v[face[1]] - v[face[0]], v[face[2]] - v[face[0]])
            assert np.dot(normal, grad) > 0, (p, t)
        total += len(f)
    assert total == 1920 and m["face_start"][-1] == 1920
    assert m["vertex_start"][0] == 0 and m["vertex_start"][1] == 0 and m["face_start"][256] == m["face_start"][255]   # all out, all in


FIELDS = {
    "sphere": lambda: ref.sphere_phi((5, 6, 7), (3.4, 3.1, 2.6), 1.7),
    "two_spheres": lambda: np.minimum(ref.sphere_phi((5, 6, 7), (2.3, 3.0, 2.5), 1.4), ref.sphere_phi((5, 6, 7), (4.4, 3.2, 2.6), 1.5)),
    "random": lambda: ref.random_phi((5, 6, 7), 7),
}


@pytest.mark.parametrize("name", sorted(FIELDS))
def test_watertight_by_construction(name):
    phi = FIELDS[name]()[None]
    m = ref.extract(phi, bnd=1, closed=True)
    assert len(m["faces"]) > 0
    assert ref.is_watertight(m["faces"])
    comps = ref.components(len(m["vertices"]), m["faces"])
    if name == "sphere":
        assert len(comps) == 1
        v, e, f = comps[0]
        assert v - e + f == 2
    # the twin has the same faces: the signs do not depend on the precision
    np.testing.assert_array_equal(ref.extract(phi, bnd=1, closed=True, dtype=np.float32)["faces"], m["faces"])


def test_fp64_volume_of_a_sphere():
    r = 5.0
    m = ref.extract(ref.sphere_phi((16, 16, 16), (8.0, 8.0, 8.0), r)[None])
    assert ref.is_watertight(m["faces"])
    vol = ref.volume(m["vertices"], m["faces"])
    want = 4.0 / 3.0 * np.pi * r ** 3
    assert vol > 0
    rel = abs(vol - want) / want
    print("sphere volume: mesh %.6f, exact %.6f, relative error %.3e" % (vol, want, rel))
    # measured on the CPU: relative error 1.993e-02 (mesh 513.17 for 523.60).  The distance function is convex, so its linear
    # interpolant along the diagonal edges has its zero inside the sphere: discretisation error, not rounding.  Asserted with a
    # margin of x2 over the measured value.
    assert rel <= 2 * 1.993e-2


def test_refusals_without_a_device():
    ok = torch.zeros((1, 4, 4, 4))
    with pytest.raises(ValueError, match="3-D level set"):
        ops.extract_surface(torch.zeros((1, 4, 4)))
    with pytest.raises(ValueError, match=">= 2"):
        ops.extract_surface(torch.zeros((1, 4, 1, 4)))
    with pytest.raises(ValueError, match="bnd >= 1"):
        ops.extract_surface(ok, bnd=0, closed=True)
    with pytest.raises(ValueError, match="too wide"):
        ops.extract_surface(ok, bnd=2)
    with pytest.raises(ValueError, match="too wide"):
        ops.extract_surface(ok, bnd=3, closed=True)
    with pytest.raises(TypeError, match="float32"):
        ops.extract_surface(ok.double())
    with pytest.raises(ValueError, match="contiguous"):
        ops.extract_surface(torch.zeros((1, 4, 4, 8))[..., ::2])
    with pytest.raises(ValueError, match="bnd must be"):
        ops.extract_surface(ok, bnd=-1)
    with pytest.raises(ValueError, match="closed_value"):
        ops.extract_surface(ok, bnd=1, closed=True, closed_value=0.0)
    with pytest.raises(ValueError, match="capacity"):
        ops.extract_surface(ok, capacity=-1)
    with pytest.raises(ValueError, match="int32"):
        ops.extract_surface(torch.empty((1, 1024, 1024, 1024), device="meta"))
    # a capacity that is too small: the check the GPU path makes once the totals are known names the capacity needed
    with pytest.raises(_lib.DeepFluidsHipError, match=r"needs capacity=\(26, 48\)"):
        ops._mesh_fit(26, 48, (25, 48))
    with pytest.raises(_lib.DeepFluidsHipError, match=r"needs capacity=\(26, 48\)"):
        ops._mesh_fit(26, 48, (26, 47))
    ops._mesh_fit(26, 48, (26, 48))
    ops._mesh_fit(26, 48, None)
    if not torch.cuda.is_available():                                   # everything above was refused before anything asked for a device
        with pytest.raises(_lib.DeepFluidsHipError, match="no CPU path"):
            ops.extract_surface(ok)


def test_obj_round_trip(tmp_path):
    m = ref.extract(ref.sphere_phi((5, 6, 7), (3.4, 3.1, 2.6), 1.7)[None], normals=True, dtype=np.float32)
    v, f, n = m["vertices"], m["faces"], m["normals"]
    path = util.save_obj(str(tmp_path / "a.obj"), v, f)
    text = open(path).read().splitlines()
    assert text[0].startswith("v ") and sum(1 for ln in text if ln.startswith("f ")) == len(f)
    assert min(int(w) for ln in text if ln.startswith("f ") for w in ln.split()[1:]) == 1            # 1-based
    v2, f2, n2 = util.load_obj(path)
    np.testing.assert_array_equal(f2, f)
    assert f2.dtype == np.int32 and n2 is None
    np.testing.assert_allclose(v2, v, rtol=5e-9, atol=0)               # 9 significant digits are printed
    np.testing.assert_array_equal(v2, v)                               # ... which is enough for a float32 to survive
    path = util.save_obj(str(tmp_path / "b.obj"), torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(n))
    text = open(path).read()
    assert "vn " in text and "//" in text
    a, b = [ln for ln in text.splitlines() if ln.startswith("f ")][0].split()[1].split("//")
    assert a == b
    v3, f3, n3 = util.load_obj(path)
    np.testing.assert_array_equal(f3, f)
    np.testing.assert_array_equal(v3, v)
    np.testing.assert_array_equal(n3, n)
    with pytest.raises(ValueError, match="faces refer"):
        util.save_obj(str(tmp_path / "c.obj"), v[:3], f)


def test_cabi_size_query_and_argument_errors():
    h = _lib.lib()
    # the size query is host arithmetic: the edges of the box and 12 triangles per cube
    assert h.df_mesh_capacity_bound(1, 2, 2, 2, 0, 0, 0) == 19                  # 12 axis edges, 6 face diagonals, 1 cube diagonal
    assert h.df_mesh_capacity_bound(1, 2, 2, 2, 0, 0, 1) == 12
    assert h.df_mesh_capacity_bound(3, 5, 6, 7, 1, 0, 1) == 3 * 12 * 2 * 3 * 4
    assert h.df_mesh_capacity_bound(3, 5, 6, 7, 1, 1, 1) == 3 * 12 * 4 * 5 * 6  # closed: one layer wider
    m = (7, 6, 5)
    edges = sum((m[0] - (d & 1)) * (m[1] - ((d >> 1) & 1)) * (m[2] - ((d >> 2) & 1)) for d in range(1, 8))
    assert h.df_mesh_capacity_bound(2, 5, 6, 7, 0, 0, 0) == 2 * edges
    # ... and an upper bound of what the reference finds
    r = ref.extract(ref.random_phi((5, 6, 7), 7)[None])
    assert len(r["vertices"]) <= edges and len(r["faces"]) <= 12 * 4 * 5 * 6
    assert h.df_mesh_capacity_bound(1, 1, 4, 4, 0, 0, 0) == -2 and b">= 2" in h.df_last_error()
    assert h.df_mesh_capacity_bound(1, 4, 4, 4, 2, 0, 0) == -2 and b"too wide" in h.df_last_error()
    assert h.df_mesh_capacity_bound(1, 4, 4, 4, 0, 1, 0) == -1 and b"closed needs bnd >= 1" in h.df_last_error()
    assert h.df_mesh_capacity_bound(1, 4, 4, 4, 0, 0, 2) == -1 and b"what" in h.df_last_error()
    assert h.df_mesh_capacity_bound(1, 1024, 1024, 1024, 0, 0, 0) == -2 and b"int32" in h.df_last_error()
    buf = ctypes.create_string_buffer(4096)
    a = (ctypes.addressof(buf) + 15) & ~15
    assert h.df_mesh_count(None, a, a, a, 1, 2, 2, 2, 0, 0, 0.5, None) == -1 and b"null phi" in h.df_last_error()
    assert h.df_mesh_count(a, None, a, a, 1, 2, 2, 2, 0, 0, 0.5, None) == -1 and b"null mask" in h.df_last_error()
    assert h.df_mesh_count(a, a, a, None, 1, 2, 2, 2, 0, 0, 0.5, None) == -1 and b"null counts" in h.df_last_error()
    assert h.df_mesh_count(a, a, a, a, 1, 2, 1, 2, 0, 0, 0.5, None) == -2 and b">= 2" in h.df_last_error()
    assert h.df_mesh_count(a, a, a, a, 1, 4, 4, 4, 2, 0, 0.5, None) == -2 and b"too wide" in h.df_last_error()
    assert h.df_mesh_count(a, a, a, a, 1, 4, 4, 4, 0, 1, 0.5, None) == -1 and b"closed needs bnd >= 1" in h.df_last_error()
    assert h.df_mesh_count(a, a, a, a, 1, 4, 4, 4, 1, 1, -1.0, None) == -1 and b"closed_value" in h.df_last_error()
    assert h.df_mesh_count(a, a, a, a, 1, 4, 4, 4, -1, 0, 0.5, None) == -1 and b"bnd must be" in h.df_last_error()
    assert h.df_mesh_count(a + 2, a, a, a, 1, 4, 4, 4, 0, 0, 0.5, None) == -3
    assert h.df_mesh_emit(a, a, a, None, a, None, a, 1, 1, 1, 4, 4, 4, 0, 0, 0.5, None) == -1 and b"null offsets" in h.df_last_error()
    assert h.df_mesh_emit(a, a, a, a, None, None, a, 1, 1, 1, 4, 4, 4, 0, 0, 0.5, None) == -1 and b"null vertices" in h.df_last_error()
    assert h.df_mesh_emit(a, a, a, a, a, None, None, 1, 1, 1, 4, 4, 4, 0, 0, 0.5, None) == -1 and b"null faces" in h.df_last_error()
    assert h.df_mesh_emit(a, a, a, a, a, None, a, -1, 1, 1, 4, 4, 4, 0, 0, 0.5, None) == -1 and b"negative capacity" in h.df_last_error()
    assert h.df_mesh_emit(a, a, a, a, a, None, a, 1, 1, 1, 4, 4, 1, 0, 0, 0.5, None) == -2
    assert h.df_mesh_emit(a, a, a, a, a, None, a, 1, 1, 1, 4, 4, 4, 0, 1, 0.5, None) == -1 and b"closed needs bnd >= 1" in h.df_last_error()
    assert h.df_mesh_emit(a, a, a + 2, a, a, None, a, 1, 1, 1, 4, 4, 4, 0, 0, 0.5, None) == -3
