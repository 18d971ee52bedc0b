"""GPU side of the liquid step (particles.hip): the RK4 trace, the cell keys and ranges, the union level set, the sequence driver and
``Trainer.advect_liquid_`` against the restatement of tests/particles_ref.py -- fp64 as the reference, with a tolerance of
3 * e32 + 1e-7 where e32 is the distance of its fp32 twin from fp64, measured in the same test; bitwise where the arithmetic is exact.

The twin's side of those figures (it needs no GPU; tests/test_particles_host.py prints it): single trace steps e32 0 (one particle
resting on the clamp) .. 3.6e-06 cell units over the nine cases, 8-frame sequences e32 4.2e-06 (2-D) and 5.6e-06 (3-D) on the
positions and 2.2e-06 / 4.3e-06 on the last level set, level sets on given positions e32 2.6e-08 .. 3.8e-07.
Loose alignments, guarded buffers, the block remap's remainder and the documented hostile inputs: tests/test_gpu_particle_edges.py."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import particles_ref as ref
from gpu_util import dev

pytestmark = pytest.mark.gpu

GRIDS = [((12, 9), 1), ((12, 9), 2), ((7, 8, 6), 1), ((7, 8, 6), 2), ((16, 24, 16), 1)]


@pytest.mark.parametrize("shape,bnd", GRIDS)
def test_trace_bitwise(shape, bnd):
    """Zero velocity and the exact half-cell shift equal the twin bit for bit (tests/test_particles_host.py checks the twin itself)."""
    from deep_fluids_amd import ops
    D = len(shape)
    lo, hi = ref.clamp_bounds(shape, bnd, np.float32)
    for B, N in ((1, 1), (3, 255), (3, 257), (1, 1000)):
        pos = ref.make_positions(shape, B, N, bnd, 5)
        pos = np.fmin(np.fmax((np.round(pos * 1024) / 1024).astype(np.float32), lo), hi)
        zero = np.zeros((B,) + shape + (D,), np.float32)
        got = ops.advect_particles(dev(pos), dev(zero), 1.0, bnd=bnd)
        assert got.cpu().numpy().tobytes() == pos.tobytes()
        half = np.full_like(zero, 0.5)
        want = ref.trace(pos, half, 1.0, bnd, 1.0, np.float32)
        assert want.tobytes() == np.fmin(pos + np.float32(0.5), hi).astype(np.float32).tobytes()
        got = ops.advect_particles(dev(pos), dev(half), 1.0, bnd=bnd)
        assert got.dtype == torch.float32 and tuple(got.shape) == pos.shape
        assert got.cpu().numpy().tobytes() == want.tobytes()
        # the same displacement through vel_scale, and in place
        p = dev(pos)
        got = ops.advect_particles(p, dev(half / 4), 1.0, bnd=bnd, vel_scale=4.0, out=p)
        assert got is p and p.cpu().numpy().tobytes() == want.tobytes()


def test_trace_parity_with_the_fp64_restatement():
    from deep_fluids_amd import ops
    n = 0
    for name, pos, vel, kw in ref.trace_cases():
        r64 = ref.trace(pos, vel, dtype=np.float64, **kw)
        r32 = ref.trace(pos, vel, dtype=np.float32, **kw)
        e32 = ref.max_err(r32, r64)
        p = dev(pos)
        keep = p.clone()
        got = ops.advect_particles(p, dev(vel), kw["dt"], bnd=kw["bnd"], vel_scale=kw["vel_scale"])
        assert torch.equal(p, keep)
        inplace = ops.advect_particles(p, dev(vel), kw["dt"], bnd=kw["bnd"], vel_scale=kw["vel_scale"], out=p)
        assert torch.equal(inplace, got)                                                     # pos_out == pos_in
        got = got.cpu().numpy()
        assert got.dtype == np.float32 and got.shape == pos.shape
        err = ref.max_err(got, r64)
        print("trace %-14s e32 %.3e  gpu %.3e (bound %.3e)  gpu == twin bitwise: %s" %
              (name, e32, err, 3 * e32 + 1e-7, got.tobytes() == r32.tobytes()))
        assert err <= 3 * e32 + 1e-7, name                                                   # every particle
        n += 1
    assert n == 9


def test_keys_and_ranges():
    from deep_fluids_amd import ops
    cases = [(name, shape, pos) for name, shape, pos in ref.levelset_cases()]
    cases += [(name, vel.shape[1:-1], pos) for name, pos, vel, kw in ref.trace_cases()]       # exact clamp values, first and last cells
    cases.append(("2d-empty", (12, 9), np.zeros((3, 0, 2), np.float32)))
    cases.append(("3d-empty", (7, 8, 6), np.zeros((1, 0, 3), np.float32)))
    for name, shape, pos in cases:
        B, N, D = pos.shape
        nkeys = B * int(np.prod(shape))
        keys = ref.cell_keys(pos, shape)
        order, cell_start = ref.cell_ranges(keys, nkeys)
        p = dev(pos)
        k = torch.empty((B * N,), dtype=torch.int32, device="cuda")
        ops.call("df_particles_cell_keys%dd" % D, ops._ptr(p), ops._ptr(k), B, N, *(list(shape) + [ops._stream()]))
        np.testing.assert_array_equal(k.cpu().numpy(), keys, err_msg=name)
        spos, cs, od = ops.particle_cells(p, shape)
        assert spos.dtype == torch.float32 and tuple(spos.shape) == pos.shape
        assert cs.dtype == torch.int32 and tuple(cs.shape) == (nkeys + 1,) and od.dtype == torch.int64 and tuple(od.shape) == (B * N,)
        np.testing.assert_array_equal(od.cpu().numpy(), order, err_msg=name)                  # NumPy's stable argsort
        assert spos.cpu().numpy().tobytes() == pos.reshape(-1, D)[order].tobytes(), name      # sorted_pos == pos[order]
        np.testing.assert_array_equal(cs.cpu().numpy(), cell_start, err_msg=name)
        if name in ("2d-n1000", "3d-n1000"):
            assert np.diff(cell_start).max() >= 300                                           # one cell holds 300
        if N == 0:
            assert not cell_start.any()


def test_levelset_parity_with_the_fp64_brute_force():
    from deep_fluids_amd import ops
    n = 0
    for name, shape, pos in ref.levelset_cases():
        p = dev(pos)
        for rf in ref.RADIUS_FACTORS:
            f64 = ref.levelset_brute(pos, shape, rf, np.float64)                             # the same fp32 positions
            f32 = ref.levelset_brute(pos, shape, rf, np.float32)
            e32 = ref.max_err(f32, f64)
            got = ops.particle_levelset(p, shape, rf)
            assert got.dtype == torch.float32 and tuple(got.shape) == (pos.shape[0],) + shape
            again = ops.particle_levelset(p, shape, rf, out=torch.empty_like(got))
            assert torch.equal(got, again)                                                   # two runs, bitwise
            got = got.cpu().numpy()
            err = ref.max_err(got, f64)
            print("levelset %-12s rf %.1f  e32 %.3e  gpu %.3e (bound %.3e)  gpu == twin bitwise: %s" %
                  (name, rf, e32, err, 3 * e32 + 1e-7, got.tobytes() == f32.tobytes()))
            assert err <= 3 * e32 + 1e-7, (name, rf)                                          # every cell
            n += 1
    assert n == 15
    # (7, 8, 6) with radius_factor 2: w = 3 clips the window on both sides of the 6-wide axis
    assert ref.window_of(2.0) == 3


def test_levelset_window_is_the_definition():
    """radius_factor 0.99 in 3-D (w = 1, 2*radius > w + 0.5): the kernel follows the window form of the header, not the brute force."""
    from deep_fluids_amd import ops
    shape = (7, 8, 6)
    pos = ref.levelset_positions(shape, 2, 255, 21)
    w64 = ref.levelset_window(pos, shape, 0.99, np.float64)
    w32 = ref.levelset_window(pos, shape, 0.99, np.float32)
    e32 = ref.max_err(w32, w64)
    got = ops.particle_levelset(dev(pos), shape, 0.99).cpu().numpy()
    print("levelset window form rf 0.99  e32 %.3e  gpu %.3e" % (e32, ref.max_err(got, w64)))
    assert ref.max_err(got, w64) <= 3 * e32 + 1e-7


@pytest.mark.parametrize("shape", [(12, 9), (7, 8, 6)])
def test_levelset_without_particles(shape):
    from deep_fluids_amd import ops
    D = len(shape)
    for rf in ref.RADIUS_FACTORS:
        got = ops.particle_levelset(torch.zeros((3, 0, D), device="cuda"), shape, rf).cpu().numpy()
        want = np.full((3,) + shape, ref.radius_of(D, rf, np.float32), np.float32)
        assert got.tobytes() == want.tobytes()
    # no particles: the trace is a no-op
    v = torch.zeros((3,) + shape + (D,), device="cuda")
    assert tuple(ops.advect_particles(torch.zeros((3, 0, D), device="cuda"), v, 1.0).shape) == (3, 0, D)


def test_sequence_against_the_fp64_restatement():
    from deep_fluids_amd import ops
    for name, pos, vels, kw in ref.sequence_cases():
        T, B = vels.shape[:2]
        shape = vels.shape[2:-1]
        assert T == 8
        p64, phi64 = ref.sequence(pos, vels, dtype=np.float64, **kw)
        p32, phi32 = ref.sequence(pos, vels, dtype=np.float32, **kw)
        e_pos, e_phi = ref.max_err(p32, p64), ref.max_err(phi32[-1], phi64[-1])
        p0 = dev(pos)
        keep = p0.clone()
        final, phi, imgs = ops.liquid_sequence(p0, dev(vels), kw["dt"], bnd=kw["bnd"], vel_scale=kw["vel_scale"],
                                               radius_factor=kw["radius_factor"], images=True)
        assert torch.equal(p0, keep)
        assert final.dtype == torch.float32 and tuple(final.shape) == pos.shape
        assert phi.dtype == torch.float32 and tuple(phi.shape) == (B,) + shape
        assert imgs.dtype == np.uint8 and imgs.shape == (T, B) + shape[-2:]
        got_p, got_phi = final.cpu().numpy(), phi.cpu().numpy()
        print("sequence %-6s positions e32 %.3e gpu %.3e (bound %.3e)  last phi e32 %.3e gpu %.3e (bound %.3e)  gpu == twin bitwise: %s" %
              (name, e_pos, ref.max_err(got_p, p64), 3 * e_pos + 1e-7, e_phi, ref.max_err(got_phi, phi64[-1]), 3 * e_phi + 1e-7,
               got_p.tobytes() == p32.tobytes() and got_phi.tobytes() == phi32[-1].tobytes()))
        assert ref.max_err(got_p, p64) <= 3 * e_pos + 1e-7
        assert ref.max_err(got_phi, phi64[-1]) <= 3 * e_phi + 1e-7
        # the same loop by hand: bitwise, and every image is the restated l_adv frame of the GPU's own phi
        cur = p0
        for t in range(T):
            ph = ops.particle_levelset(cur, shape, kw["radius_factor"])
            np.testing.assert_array_equal(imgs[t], ref.density_image(ph.cpu().numpy()))
            np.testing.assert_array_equal(imgs[t], ops.density_image(ph).cpu().numpy())
            cur = ops.advect_particles(cur, dev(vels[t]), kw["dt"], bnd=kw["bnd"], vel_scale=kw["vel_scale"])
        assert torch.equal(cur, final) and torch.equal(ph, phi)
        assert imgs.max() > imgs.min()                                                       # liquid and air in the frames
        two = ops.liquid_sequence(p0, list(dev(vels)), kw["dt"], bnd=kw["bnd"], vel_scale=kw["vel_scale"], radius_factor=kw["radius_factor"])
        assert len(two) == 2 and torch.equal(two[0], final) and torch.equal(two[1], phi)


def test_python_surface_rejects_bad_arguments():
    from deep_fluids_amd import ops, _lib
    p = torch.zeros((2, 5, 3), device="cuda") + 2.0
    v = torch.zeros((2, 7, 8, 6, 3), device="cuda")
    with pytest.raises(_lib.DeepFluidsHipError):
        ops.advect_particles(p.cpu(), v, 1.0)
    with pytest.raises(TypeError):
        ops.advect_particles(p.double(), v, 1.0)
    with pytest.raises(ValueError):
        ops.advect_particles(p, v[..., :2].contiguous(), 1.0)
    with pytest.raises(ValueError):
        ops.advect_particles(p[..., :2].contiguous(), v, 1.0)
    with pytest.raises(ValueError):
        ops.advect_particles(p, v, 1.0, out=torch.empty((2, 4, 3), device="cuda"))
    with pytest.raises(_lib.DeepFluidsHipError):
        ops.advect_particles(p, v, 1.0, bnd=3)                                               # 2*3 + 2 > 6
    with pytest.raises(ValueError):
        ops.particle_levelset(p, (8, 6))
    with pytest.raises(_lib.DeepFluidsHipError):
        ops.particle_levelset(p, (7, 8, 6), radius_factor=-1.0)
    with pytest.raises(_lib.DeepFluidsHipError):
        ops.particle_levelset(p.cpu(), (7, 8, 6))


def test_cabi_error_paths():
    """Argument errors are answered on the host with the documented codes; nothing is launched (the pointers are not device memory)."""
    from deep_fluids_amd import _lib
    h = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    a = (ctypes.addressof(buf) + 15) & ~15
    big = 1 << 11
    # null pointers: DF_EINVAL
    assert h.df_particles_advect2d(None, a, a, 1, 4, 8, 8, 1.0, 1.0, 1, None) == -1 and b"null input" in h.df_last_error()
    assert h.df_particles_advect3d(a, None, a, 1, 4, 8, 8, 8, 1.0, 1.0, 1, None) == -1 and b"null output" in h.df_last_error()
    assert h.df_particles_advect3d(a, a, None, 1, 4, 8, 8, 8, 1.0, 1.0, 1, None) == -1 and b"null velocity" in h.df_last_error()
    assert h.df_particles_cell_keys2d(None, a, 1, 4, 8, 8, None) == -1
    assert h.df_particles_cell_keys3d(a, None, 1, 4, 8, 8, 8, None) == -1
    assert h.df_particles_gather(a, None, a + 64, 4, 3, None) == -1
    assert h.df_particles_gather(a, a + 128, a, 4, 3, None) == -1                             # in place
    assert h.df_particles_gather(a, a + 128, a + 64, 4, 4, None) == -1                        # dim
    assert h.df_particle_levelset_union2d(a, a, None, 1, 4, 8, 8, 1.0, None) == -1
    assert h.df_particle_levelset_union3d(None, a, a, 1, 4, 8, 8, 8, 1.0, None) == -1
    assert h.df_particle_levelset_union3d(a, None, a, 1, 4, 8, 8, 8, 1.0, None) == -1
    assert h.df_particle_levelset_union3d(a, a, a, 1, 4, 8, 8, 8, -0.5, None) == -1 and b"radius_factor" in h.df_last_error()
    assert h.df_particles_advect2d(a, a, a, 1, -1, 8, 8, 1.0, 1.0, 1, None) == -1
    assert h.df_particles_advect2d(a, a, a, 1, 4, 8, 8, 1.0, 1.0, -1, None) == -1
    # an extent of 1: DF_ESHAPE
    assert h.df_particles_advect2d(a, a, a, 1, 4, 1, 8, 1.0, 1.0, 0, None) == -2 and b">= 2" in h.df_last_error()
    assert h.df_particles_advect3d(a, a, a, 1, 4, 1, 8, 8, 1.0, 1.0, 0, None) == -2
    assert h.df_particles_cell_keys2d(a, a, 1, 4, 8, 1, None) == -2
    assert h.df_particles_cell_keys3d(a, a, 1, 4, 8, 1, 8, None) == -2
    assert h.df_particle_levelset_union2d(a, a, a, 1, 4, 1, 8, 1.0, None) == -2
    assert h.df_particle_levelset_union3d(a, a, a, 1, 4, 8, 8, 1, 1.0, None) == -2
    # bnd too large for the grid: DF_ESHAPE
    assert h.df_particles_advect2d(a, a, a, 1, 4, 8, 7, 1.0, 1.0, 3, None) == -2 and b"2*bnd + 2" in h.df_last_error()
    assert h.df_particles_advect3d(a, a, a, 1, 4, 5, 8, 8, 1.0, 1.0, 2, None) == -2
    # the keys do not fit an int32: DF_ESHAPE
    assert h.df_particles_cell_keys3d(a, a, 1, 4, big, big, big, None) == -2 and b"int32" in h.df_last_error()
    assert h.df_particles_cell_keys2d(a, a, 3, 4, 1 << 15, 1 << 15, None) == -2
    assert h.df_particle_levelset_union3d(a, a, a, 2, 4, 1 << 10, 1 << 10, 1 << 10, 1.0, None) == -2 and b"int32" in h.df_last_error()
    assert h.df_particles_cell_keys2d(a, a, 1 << 20, 1 << 20, 8, 8, None) == -2               # B*N
    # misaligned: DF_EALIGN
    assert h.df_particles_advect2d(a + 2, a, a, 1, 4, 8, 8, 1.0, 1.0, 1, None) == -3
    assert h.df_particles_gather(a, a + 132, a + 64, 4, 2, None) == -3
    torch.cuda.synchronize()                                                                  # nothing was enqueued, nothing faults


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_trainer_advect_liquid(tmp_path):
    from deep_fluids_amd import ops
    from deep_fluids_amd.data import BatchManager, write_synthetic_dataset
    from deep_fluids_amd.trainer import Trainer3, default_config, liquid3_vis_body, body_levelset
    spatial, y3 = (8, 16, 8), 4
    root = str(tmp_path / "data")
    n = write_synthetic_dataset(root, spatial, num_p=(3, 2), num_frames=y3)
    cfg = default_config(is_3d=True, res_x=8, res_y=16, res_z=8, filters=16, batch_size=2, num_samples=n, model_dir=str(tmp_path / "run"),
                         test_batch_size=2, use_curl=False)
    dcfg = SimpleNamespace(random_seed=123, data_path=root, is_3d=True, arch="de", data_type="velocity", batch_size=2,
                           res_x=8, res_y=16, res_z=8, num_worker=1)
    ops.reset_variables()
    tr = Trainer3(cfg)
    bm = BatchManager(dcfg, device=None)
    p1, p2 = 1, 1
    body = liquid3_vis_body(bm)
    out_dir, pos, phi = tr.advect_liquid_(bm, p1=p1, p2=p2, body=body, radius_factor=1.0, seed=7)
    assert out_dir == os.path.join(str(tmp_path / "run"), "%d_%d" % (p1, p2), "l_adv")
    assert sorted(os.listdir(out_dir)) == ["%04d.png" % t for t in range(y3)]
    # the same loop by hand
    z_c, niter, b = tr._sweep_codes(bm, p1, p2, None, "test")
    frames = torch.cat([tr.generate(torch.from_numpy(z_c[b * i:b * (i + 1)]).cuda()) for i in range(niter)], dim=0)
    assert tuple(frames.shape) == (y3,) + spatial + (3,)
    pos0 = ops.seed_particles(body_levelset(spatial, body), seed=7)
    assert pos0.shape == (8 * int((body_levelset(spatial, body)[1:-1, 1:-1, 1:-1] < 0).sum()), 3) and pos0.shape[0] > 0
    cur = torch.from_numpy(pos0).cuda().unsqueeze(0)
    for t in range(y3):
        ph = ops.particle_levelset(cur, spatial, 1.0)
        png = _png(os.path.join(out_dir, "%04d.png" % t))
        assert png.dtype == np.uint8 and png.shape == spatial[-2:]                          # grey, [Y,X]
        np.testing.assert_array_equal(png, ops.density_image(ph).cpu().numpy()[0])
        cur = ops.advect_particles(cur, frames[t:t + 1], 1.0, bnd=1, vel_scale=float(bm.x_range))
    assert pos.is_cuda and phi.is_cuda and tuple(pos.shape) == (1,) + pos0.shape and tuple(phi.shape) == (1,) + spatial
    assert torch.equal(pos, cur)                                                             # dt defaults to 1.0
    assert torch.equal(phi, ph)                                                              # the level set before the last trace
    assert float(phi.min()) < 0 < float(phi.max())
    # again, elsewhere: bitwise reproducible; dt="dataset" needs args.txt's time_step
    out2, pos2, phi2 = tr.advect_liquid_(bm, model_dir=str(tmp_path / "again"), p1=p1, p2=p2, body=body_levelset(spatial, body), seed=7)
    assert torch.equal(pos2, pos) and torch.equal(phi2, phi)
    for t in range(y3):
        np.testing.assert_array_equal(_png(os.path.join(out2, "%04d.png" % t)), _png(os.path.join(out_dir, "%04d.png" % t)))
    if "time_step" not in bm.args:
        with pytest.raises(KeyError):
            tr.advect_liquid_(bm, model_dir=str(tmp_path / "again"), p1=p1, p2=p2, body=body, dt="dataset")
    with pytest.raises(ValueError):
        tr.advect_liquid_(bm, model_dir=str(tmp_path / "again"), p1=p1, p2=p2, body=body, dt="frame")
    ops.reset_variables()
