"""GPU side of the surface mesher (csrc/mesh.hip, ``ops.extract_surface``, ``Trainer.advect_liquid_(mesh=True)``) against
tests/liquid_mesh_ref.py: vertex positions bitwise the fp32 twin, faces and the ragged starts exact, normals against the fp64 reference
with a tolerance of 4 x the twin's own deviation from it, measured in the same test (the factor covers the normalise's rounding).

The twin's side of those figures (it needs no GPU): max |twin - fp64| over the normals' components 9.0e-08 .. 1.8e-07 on the six
5x6x7 cases below (sphere 9.7e-08 for all three boxes; random 9.5e-08, 9.0e-08, 1.8e-07 closed), so the tolerances are 3.6e-07 ..
7.4e-07; the positions' 2.3e-07 .. 2.9e-07 grid units play no part, they are compared bit for bit."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import liquid_mesh_ref as ref
from gpu_util import dev

pytestmark = pytest.mark.gpu


def _same_mesh(got, want):
    """positions bit for bit, faces and starts exact"""
    assert got.vertices.dtype == torch.float32 and got.faces.dtype == torch.int32
    assert got.vertex_start.dtype == torch.int32 and got.face_start.dtype == torch.int32
    np.testing.assert_array_equal(got.vertex_start.cpu().numpy(), want["vertex_start"])
    np.testing.assert_array_equal(got.face_start.cpu().numpy(), want["face_start"])
    assert tuple(got.vertices.shape) == want["vertices"].shape and tuple(got.faces.shape) == want["faces"].shape
    assert want["vertices"].dtype == np.float32
    assert got.vertices.cpu().numpy().tobytes() == want["vertices"].tobytes()
    np.testing.assert_array_equal(got.faces.cpu().numpy(), want["faces"])


@functools.lru_cache(maxsize=None)
def _field(name):
    phi = {"sphere": lambda: ref.sphere_phi((5, 6, 7), (3.4, 3.1, 2.6), 1.7), "random": lambda: ref.random_phi((5, 6, 7), 7)}[name]()[None]
    phi.setflags(write=False)
    return phi


@functools.lru_cache(maxsize=None)
def _reference(name, bnd, closed):
    phi = _field(name)
    return (ref.extract(phi, bnd=bnd, closed=closed, normals=True, dtype=np.float32),
            ref.extract(phi, bnd=bnd, closed=closed, normals=True, dtype=np.float64))


def test_all_256_cube_patterns_in_one_call():
    """B = 256 of 2x2x2: every case of the tets and the ragged offsets at once, the entries without a triangle (0 and 255) included"""
    from deep_fluids_amd import ops
    phi = ref.all_cube_patterns()
    want = ref.extract(phi, dtype=np.float32)
    got = ops.extract_surface(dev(phi))
    _same_mesh(got, want)
    assert got.normals is None and got.batch == 256 and got.faces.shape[0] == 1920
    for b in (0, 1, 37, 254, 255):
        v, f, n = got.entry(b)
        rv, rf = ref.entry(want, b)
        assert n is None and v.cpu().numpy().tobytes() == rv.tobytes()
        np.testing.assert_array_equal(f.cpu().numpy(), rf)
    assert got.entry(0)[1].shape[0] == 0 and got.entry(255)[0].shape[0] == 0
    with pytest.raises(IndexError):
        got.entry(256)


def test_smallest_closed_surface():
    """3x3x3 with only the centre sample negative: 14 edges leave it, 24 triangles close around it"""
    from deep_fluids_amd import ops
    phi = np.ones((1, 3, 3, 3), np.float32)
    phi[0, 1, 1, 1] = -0.25
    want = ref.extract(phi, dtype=np.float32)
    got = ops.extract_surface(dev(phi))
    _same_mesh(got, want)
    f = got.faces.cpu().numpy()
    assert got.vertices.shape[0] == 14 and f.shape[0] == 24
    assert ref.is_watertight(f)
    assert ref.volume(got.vertices.cpu().numpy(), f) > 0


@pytest.mark.parametrize("name", ["sphere", "random"])
@pytest.mark.parametrize("bnd,closed", [(0, False), (1, False), (1, True)])
def test_unequal_extents(name, bnd, closed):
    """5x6x7: positions bitwise the twin; normals within 4 x the twin's own deviation from fp64 (measured here: see the module's
    docstring for the figures)"""
    from deep_fluids_amd import ops
    r32, r64 = _reference(name, bnd, closed)
    phi = dev(_field(name))
    got = ops.extract_surface(phi, bnd=bnd, closed=closed, normals=True)
    _same_mesh(got, r32)
    assert got.faces.shape[0] > 0
    if closed:
        assert ref.is_watertight(got.faces.cpu().numpy())
    e32 = float(np.abs(r32["normals"].astype(np.float64) - r64["normals"]).max())
    n = got.normals.cpu().numpy().astype(np.float64)
    err = float(np.abs(n - r64["normals"]).max())
    print("%s bnd=%d closed=%d: V %d, T %d, normals e32 %.3e, gpu %.3e" % (name, bnd, closed, n.shape[0], got.faces.shape[0], e32, err))
    assert e32 > 0
    assert err <= 4 * e32
    # without normals: the same positions and faces
    plain = ops.extract_surface(phi, bnd=bnd, closed=closed)
    assert plain.normals is None and torch.equal(plain.vertices, got.vertices) and torch.equal(plain.faces, got.faces)
    # a roomy capacity changes nothing
    roomy = ops.extract_surface(phi, bnd=bnd, closed=closed, capacity=(n.shape[0] + 5, got.faces.shape[0] + 7))
    assert torch.equal(roomy.vertices, got.vertices) and torch.equal(roomy.faces, got.faces)


def test_exact_zeros_and_a_negative_zero():
    """an exact zero, of either sign, is outside: the reference's mesh, and no NaN"""
    from deep_fluids_amd import ops
    phi = ref.random_phi((4, 5, 6), 11)[None].copy()
    inside = np.argwhere(phi[0] < 0)
    assert len(inside) > 6
    for k, (z, y, x) in enumerate(inside[::3][:6]):
        phi[0, z, y, x] = 0.0 if k % 2 else -0.0
    assert np.signbit(phi[phi == 0]).any() and not np.signbit(phi[phi == 0]).all()
    for closed in (False, True):
        want = ref.extract(phi, bnd=1 if closed else 0, closed=closed, dtype=np.float32)
        got = ops.extract_surface(dev(phi), bnd=1 if closed else 0, closed=closed, normals=True)
        _same_mesh(got, want)
        assert torch.isfinite(got.vertices).all() and torch.isfinite(got.normals).all()


def test_batch_of_three():
    """4x5x6: all positive, all negative, a sphere -- the offsets, and the all-negative entry as a closed box with ``closed`` and as
    nothing without it"""
    from deep_fluids_amd import ops
    phi = np.stack([np.ones((4, 5, 6), np.float32), -np.ones((4, 5, 6), np.float32), ref.sphere_phi((4, 5, 6), (3.1, 2.4, 2.2), 1.3)])
    got = ops.extract_surface(dev(phi), bnd=1, closed=True)
    want = ref.extract(phi, bnd=1, closed=True, dtype=np.float32)
    _same_mesh(got, want)
    vs, fs = got.vertex_start.cpu().numpy(), got.face_start.cpu().numpy()
    assert vs[0] == vs[1] == 0 and fs[0] == fs[1] == 0 and vs[2] > vs[1] and vs[3] > vs[2]
    for b in (1, 2):
        v, f, _ = got.entry(b)
        f = f.cpu().numpy()
        assert f.min() == 0 and f.max() == v.shape[0] - 1                       # faces are local to their entry
        assert ref.is_watertight(f)
        comps = ref.components(v.shape[0], f)
        assert len(comps) == 1 and comps[0][0] - comps[0][1] + comps[0][2] == 2
    # the box: between the box of the inner samples (-1) and the one whose faces cut the axis edges to the outer layer (0.5) at 2/3
    # (the diagonal edges chamfer its edges and corners; the reference gives 29.85)
    vol = ref.volume(got.entry(1)[0].cpu().numpy(), got.entry(1)[1].cpu().numpy())
    assert 3 * 2 * 1 < vol < (3 + 4 / 3) * (2 + 4 / 3) * (1 + 4 / 3)
    open_ = ops.extract_surface(dev(phi), bnd=0, closed=False)
    _same_mesh(open_, ref.extract(phi, dtype=np.float32))
    assert open_.entry(0)[0].shape[0] == 0 and open_.entry(1)[0].shape[0] == 0 and open_.entry(1)[1].shape[0] == 0
    assert open_.entry(2)[1].shape[0] > 0


def test_capacity_one_short():
    """``ops`` refuses before anything is emitted and names the need; the entry point itself, handed a capacity one short, leaves the
    rows from the capacity on -- and a sentinel pattern beyond the buffers -- untouched"""
    from deep_fluids_amd import _lib, ops
    from deep_fluids_amd.ops import _ptr, _stream
    phi = dev(_field("random"))
    full = ops.extract_surface(phi, normals=True)
    V, T = full.vertices.shape[0], full.faces.shape[0]
    for cap in ((V - 1, T), (V, T - 1), V - 1 if V < T else T - 1):
        with pytest.raises(_lib.DeepFluidsHipError, match=r"needs capacity=\(%d, %d\)" % (V, T)):
            ops.extract_surface(phi, capacity=cap)
    dims = [1, 5, 6, 7]
    n = 5 * 6 * 7
    mask = torch.empty((n,), dtype=torch.uint8, device=phi.device)
    counts = torch.empty((2, n), dtype=torch.uint8, device=phi.device)
    _lib.call("df_mesh_count", _ptr(phi), _ptr(mask), _ptr(counts[0]), _ptr(counts[1]), *(dims + [0, 0, 0.5, _stream()]))
    off = torch.zeros((2, n + 1), dtype=torch.int32, device=phi.device)
    off[:, 1:] = torch.cumsum(counts.to(torch.int32), 1)
    assert int(off[0, -1]) == V and int(off[1, -1]) == T
    assert int(counts[0].max()) <= 7 and int(counts[1].max()) <= 12
    pad = 64
    sv, sf = 12345.0, -777
    vbuf = torch.full((V + pad, 3), sv, dtype=torch.float32, device=phi.device)
    nbuf = torch.full((V + pad, 3), sv, dtype=torch.float32, device=phi.device)
    fbuf = torch.full((T + pad, 3), sf, dtype=torch.int32, device=phi.device)
    _lib.call("df_mesh_emit", _ptr(phi), _ptr(mask), _ptr(off[0]), _ptr(off[1]), _ptr(vbuf), _ptr(nbuf), _ptr(fbuf), V - 1, T - 1,
              *(dims + [0, 0, 0.5, _stream()]))
    assert torch.equal(vbuf[:V - 1], full.vertices[:V - 1]) and torch.equal(fbuf[:T - 1], full.faces[:T - 1])
    assert torch.equal(nbuf[:V - 1], full.normals[:V - 1])
    assert bool((vbuf[V - 1:] == sv).all()) and bool((nbuf[V - 1:] == sv).all()) and bool((fbuf[T - 1:] == sf).all())


def test_trainer_writes_obj_frames(tmp_path):
    """a tiny 3-D trainer, two frames: obj/0000.obj and obj/0001.obj are closed surfaces; the PNGs and the returned tensors are those
    of mesh=False bit for bit"""
    from PIL import Image
    from deep_fluids_amd import ops, util
    from deep_fluids_amd.data import BatchManager, write_synthetic_dataset
    from deep_fluids_amd.trainer import Trainer3, default_config, liquid3_vis_body
    spatial, y3 = (8, 12, 8), 2
    root = str(tmp_path / "data")
    n = write_synthetic_dataset(root, spatial, num_p=(3, 2), num_frames=y3)
    cfg = default_config(is_3d=True, res_x=8, res_y=12, res_z=8, filters=16, batch_size=2, num_samples=n, model_dir=str(tmp_path / "run"),
                         test_batch_size=2, use_curl=False)
    dcfg = SimpleNamespace(random_seed=123, data_path=root, is_3d=True, arch="de", data_type="velocity", batch_size=2,
                           res_x=8, res_y=12, res_z=8, num_worker=1)
    ops.reset_variables()
    tr = Trainer3(cfg)
    bm = BatchManager(dcfg, device=None)
    body = liquid3_vis_body(bm)
    plain_dir, pos0, phi0 = tr.advect_liquid_(bm, model_dir=str(tmp_path / "plain"), p1=1, p2=1, body=body, seed=7)
    assert not os.path.exists(os.path.join(str(tmp_path / "plain"), "1_1", "obj"))
    out_dir, pos, phi = tr.advect_liquid_(bm, model_dir=str(tmp_path / "mesh"), p1=1, p2=1, body=body, seed=7, mesh=True)
    assert torch.equal(pos, pos0) and torch.equal(phi, phi0)
    obj_dir = os.path.join(str(tmp_path / "mesh"), "1_1", "obj")
    assert sorted(os.listdir(obj_dir)) == ["0000.obj", "0001.obj"]
    for t in range(y3):
        a, b = (np.asarray(Image.open(os.path.join(d, "%04d.png" % t))) for d in (plain_dir, out_dir))
        np.testing.assert_array_equal(a, b)
        v, f, nrm = util.load_obj(os.path.join(obj_dir, "%04d.obj" % t))
        assert nrm is None and len(f) > 0 and f.max() == len(v) - 1
        assert ref.is_watertight(f)
        assert ref.volume(v, f) > 0
        assert v.min() >= 0.5 and (v.max(axis=0) <= np.array(spatial[::-1]) - 0.5).all()
    # the last frame's file is the mesh of the returned level set
    m = ops.extract_surface(phi, bnd=1, closed=True)
    v, f, _ = util.load_obj(os.path.join(obj_dir, "0001.obj"))
    assert v.tobytes() == m.vertices.cpu().numpy().tobytes()
    np.testing.assert_array_equal(f, m.faces.cpu().numpy())
    ops.reset_variables()
