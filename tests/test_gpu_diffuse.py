"""GPU side of the implicit velocity diffusion (the df_diffuse_* entry points of smoke.hip), of the viscous liquid step and of the
liquid3_vis set, against tests/diffuse_ref.py.

The solve cannot be bitwise with the fp32 twin: its dot products are summed in workgroup order on the GPU and by NumPy's pairwise sum in
the twin.  It is bounded as tests/test_gpu_liquid.py bounds the projection: the fp64 residual of the GPU's x by `accuracy` plus the
recurrence's drift measured on the twin, the distance from the dense fp64 solution by 3 x the twin's.  Every parity test prints its
figures before it asserts.

Shapes: (9,30) = 270 and (6,7,9) = 378 cells are two workgroups per (entry, component) pair with a ragged tail, extents that are no
multiple of anything; B = 2 with alpha = (0.23, 23.04), the second and the largest alpha of the liquid3_vis script.  At accuracy 1e-4
the twin needs 7 to 38 iterations on (9,30) and 8 to 22 on (6,7,9) (tests/test_diffuse_host.py), so the convergence tests pass
max_iter = 200 and the cap test relies on the 3-D default cap (9) lying below the counts at alpha = 23.04."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import diffuse_ref as ref
import liquid_ref as lref
from gpu_util import assert_bits, dev
from smoke_ref import interior_mask

pytestmark = pytest.mark.gpu

CASES = [(9, 30), (6, 7, 9)]
ALPHA = (0.23, 23.04)
ACC = 1e-4
_CACHE = {}


def _np(t):
    return t.cpu().numpy()


def _vel(shape, B=2, seed=7):
    return np.random.RandomState(seed).standard_normal((B,) + shape + (len(shape),)).astype(np.float32)


def _case(shape):
    """the input, the twin, the dense solution and the GPU's result at max_iter = 200: computed once, never written to"""
    if shape not in _CACHE:
        from deep_fluids_amd import ops
        v = _vel(shape)
        x32, it32, r32, _ = ref.cg(v, ALPHA, 1, ACC, 200, np.float32)
        excess = float(np.abs(ref.residual(x32, v, ALPHA, 1) - r32).max())
        got, iters = ops.diffuse_velocity(dev(v), ALPHA, accuracy=ACC, max_iter=200)
        _CACHE[shape] = SimpleNamespace(v=v, x32=x32, it32=it32, excess=excess, exact=ref.dense(v, ALPHA, 1), got=got, iters=iters)
    return _CACHE[shape]


# ---- 1, 2: the solve against the dense solution, the maximum principle -----------------------------------------------------------------------
@pytest.mark.parametrize("shape", CASES)
def test_diffusion_against_the_dense_solve(shape):
    c = _case(shape)
    D = len(shape)
    x = _np(c.got)
    res = float(np.abs(ref.residual(x, c.v, ALPHA, 1)).max())
    print("%s: iterations gpu %s twin %s  fp64 residual of the gpu's x %.4e (bound %.1e + twin's excess %.3e)" %
          (shape, _np(c.iters).tolist(), c.it32.tolist(), res, ACC, c.excess))
    assert c.iters.dtype == torch.int32 and tuple(c.iters.shape) == (2, D)
    assert (_np(c.iters) > 0).all() and (_np(c.iters) < 200).all()
    assert res <= ACC + c.excess
    d32 = float(np.abs(c.x32 - c.exact).max())
    dg = float(np.abs(x - c.exact).max())
    print("%s: distance from the dense fp64 solution: twin %.3e  gpu %.3e" % (shape, d32, dg))
    assert dg <= 3 * d32
    band = ~interior_mask(shape, 1)
    assert_bits(x[:, band], c.v[:, band], "band cells are copied")
    assert float(np.abs(x - c.v).max()) > 0.1                                # it diffuses


@pytest.mark.parametrize("shape", CASES)
def test_maximum_principle(shape):
    """(I - alpha * Laplacian) with Dirichlet data is an M-matrix whose rows, the Dirichlet terms included, sum to 1: the exact solution
    is a convex combination of the input's values, and |x - exact| = |A^-1 (b - A x)| <= max|b - A x| because ||A^-1||_inf <= 1"""
    c = _case(shape)
    B, D = 2, len(shape)
    x, u = ref.planar(_np(c.got)), ref.planar(c.v)
    for pair in range(B * D):
        mx, mu = float(np.abs(x[pair]).max()), float(np.abs(u[pair]).max())
        print("%s pair %d: max|x| %.6f  max|u| %.6f" % (shape, pair, mx, mu))
        assert mx <= mu + ACC + c.excess


# ---- 3: identity ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", CASES)
def test_identity(shape):
    from deep_fluids_amd import ops
    c = _case(shape)
    x, iters = ops.diffuse_velocity(dev(c.v), 0.0, accuracy=ACC, max_iter=200)
    assert_bits(_np(x), c.v, "alpha = 0")
    assert not _np(iters).any()
    x, iters = ops.diffuse_velocity(dev(c.v), (0.0, 2.3), accuracy=ACC, max_iter=200)
    assert_bits(_np(x)[0], c.v[0], "entry 0 at alpha = 0 beside an entry that iterates")
    assert not _np(iters)[0].any() and (_np(iters)[1] > 0).all()
    assert float(np.abs(_np(x)[1] - c.v[1]).max()) > 0.1
    x, iters = ops.diffuse_velocity(dev(c.v), ALPHA, accuracy=ACC, max_iter=0)
    assert_bits(_np(x), c.v, "max_iter = 0")
    assert not _np(iters).any()


# ---- 4: the iteration cap ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", CASES)
def test_iteration_cap(shape):
    from deep_fluids_amd import ops
    c = _case(shape)
    _, iters = ops.diffuse_velocity(dev(c.v), 23.04, accuracy=ACC, max_iter=4)
    assert (_np(iters) == 4).all()
    cap = ops.default_diffusion_max_iter(shape)
    assert cap == (9 if len(shape) == 3 else 120)
    _, iters = ops.diffuse_velocity(dev(c.v), 23.04, accuracy=ACC)
    print("%s: iterations at the default cap %d: %s" % (shape, cap, _np(iters).tolist()))
    assert (_np(iters) <= cap).all()
    if len(shape) == 3:
        assert (_np(iters) == cap).all()


# ---- 5: the bit rules ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", CASES)
def test_bit_rules(shape):
    from deep_fluids_amd import ops
    c = _case(shape)
    D = len(shape)
    kw = dict(accuracy=ACC, max_iter=200)
    x2, i2 = ops.diffuse_velocity(dev(c.v), ALPHA, **kw)
    assert torch.equal(x2, c.got) and torch.equal(i2, c.iters)
    ws = ops.diffusion_workspace(dev(c.v))
    ws.fill_(float("nan"))
    x3, i3 = ops.diffuse_velocity(dev(c.v), ALPHA, workspace=ws, **kw)
    assert torch.equal(x3, c.got) and torch.equal(i3, c.iters)
    x4, i4 = ops.diffuse_velocity(dev(c.v), ALPHA, check_every=3, **kw)
    assert torch.equal(x4, c.got) and torch.equal(i4, c.iters)
    for e in range(2):
        xe, ie = ops.diffuse_velocity(dev(c.v[e:e + 1]), ALPHA[e], **kw)
        assert_bits(_np(xe)[0], _np(c.got)[e], "entry %d alone" % e)
        assert torch.equal(ie[0], c.iters[e])
    vi = dev(c.v)
    xi, ii = ops.diffuse_velocity(vi, ALPHA, out=vi, **kw)
    assert xi is vi and torch.equal(vi, c.got) and torch.equal(ii, c.iters)
    # the components are independent systems: permuting them permutes the result and the counts (interleave and stride mistakes)
    perm = [1, 0] if D == 2 else [2, 0, 1]
    xp, ip = ops.diffuse_velocity(dev(c.v[..., perm]), ALPHA, **kw)
    assert_bits(_np(xp), _np(c.got)[..., perm], "permuted components")
    assert torch.equal(ip, c.iters[:, perm])


# ---- 6: the viscous step -------------------------------------------------------------------------------------------------------------------------
# seeds of the jitter, chosen on the CPU so that on all 3 steps the fp32 twin and the fp64 run sort every particle into the same cell
STEP_SEEDS = {(16, 16): (123, 124), (8, 12, 8): (123, 124)}
STEP_ALPHA = (0.23, 2.3)


def _parent_step(ops, p, u, v, dt, force, accuracy):
    """the step without viscosity, composed of the public ops in the order liquid_step ran them before it knew ``viscosity_alpha``"""
    shape = tuple(v.shape[1:-1])
    B, N, nd = p.shape
    moved = ops.advect_particles(p, v, dt, bnd=1)
    spos, cell_start, order = ops.particle_cells(moved, shape)
    su = u.reshape(-1, nd)[order.long()].reshape(u.shape).contiguous()
    vel, weight, known = ops.particles_to_grid(spos, su, cell_start, shape)
    vel_old = vel
    vel, _ = ops.extrapolate_mac(vel, known, 2, bnd=1)
    flags, touch = ops.liquid_flags(cell_start, shape, B, N, bnd=1)
    ops.liquid_forces(vel, flags, force, bnd=1, out=vel)
    _, _, iters = ops.solve_pressure_liquid(vel, flags, bnd=1, accuracy=accuracy, out=vel)
    vel, _ = ops.extrapolate_mac(vel, touch, 4, bnd=1)
    ops.flip_update(spos, su, vel, vel_old, out=su)
    return spos, su, vel, iters


@pytest.mark.parametrize("shape", [(16, 16), (8, 12, 8)])
def test_three_viscous_steps_of_a_drop_falling_into_a_basin(shape):
    from deep_fluids_amd import ops
    from test_gpu_liquid import drop_scene
    D = len(shape)
    pos0, vel0 = drop_scene(shape, STEP_SEEDS[shape])
    dt, tight, T = 0.5, 1e-6, 3
    pvel0 = lref.sample(vel0, pos0, np.float32)
    s64 = dict(pos=pos0.astype(np.float64), pvel=pvel0.astype(np.float64), vel=vel0.astype(np.float64))
    s32 = dict(pos=pos0, pvel=pvel0, vel=vel0)
    p, u, v = dev(pos0), dev(pvel0), dev(vel0)
    for t in range(T):
        # as in test_four_steps_of_a_drop_falling_into_a_basin: fp64 at an accuracy three decades below the one fp32 and the GPU stop at
        s64 = ref.step(s64["pos"], s64["pvel"], s64["vel"], dt, STEP_ALPHA, accuracy=tight * 1e-3, dtype=np.float64)
        s32 = ref.step(s32["pos"], s32["pvel"], s32["vel"], dt, STEP_ALPHA, accuracy=tight, dtype=np.float32)
        out = ops.liquid_step(p, u, v, dt, accuracy=tight, viscosity_alpha=STEP_ALPHA)
        assert len(out) == 5
        p, u, v, iters, diters = out
        assert diters.dtype == torch.int32 and tuple(diters.shape) == (2, D) and tuple(iters.shape) == (2,)
        assert (_np(diters) <= ops.default_diffusion_max_iter(shape)).all()
        np.testing.assert_array_equal(s32["cell_start"], s64["cell_start"])
        _, gcs, _ = ops.particle_cells(p, shape)
        np.testing.assert_array_equal(_np(gcs), s64["cell_start"])
        assert (s32["liquid"] == s64["liquid"]).all()
        e32 = [lref.max_err(s32[k], s64[k]) for k in ("vel", "pos", "pvel")]
        eg = [lref.max_err(_np(x), s64[k]) for x, k in ((v, "vel"), (p, "pos"), (u, "pvel"))]
        et = [lref.max_err(_np(x), s32[k]) for x, k in ((v, "vel"), (p, "pos"), (u, "pvel"))]
        print("%s step %d: iterations %s diffusion gpu %s twin %s  vel/pos/pvel twin-vs-fp64 %.3e %.3e %.3e  gpu-vs-fp64 %.3e %.3e %.3e  gpu-vs-twin %.3e %.3e %.3e"
              % ((shape, t + 1, _np(iters).tolist(), _np(diters).tolist(), s32["diters"].tolist()) + tuple(e32) + tuple(eg) + tuple(et)))
        for k in range(3):
            # the bound of test_four_steps_of_a_drop_falling_into_a_basin: margin 3 over the twin's own error plus the solves' accuracy
            assert eg[k] <= 3 * e32[k] + 2 * tight * max(shape), (k, eg[k], e32[k])
            assert et[k] <= 3 * e32[k] + 2 * tight * max(shape), (k, et[k], e32[k])
    assert _np(diters).any()                                                # the diffusion iterates once the liquid moves
    # the two entries differ in alpha and the viscosity matters at the bound's scale
    plain = dev(pos0), dev(pvel0), dev(vel0)
    for t in range(T):
        plain = ops.liquid_step(plain[0], plain[1], plain[2], dt, accuracy=tight)[:3]
    assert float((plain[2] - v).abs().max()) > 1e-3


@pytest.mark.parametrize("shape", [(16, 16), (8, 12, 8)])
def test_without_viscosity_the_step_keeps_its_bits(shape):
    from deep_fluids_amd import ops
    from test_gpu_liquid import drop_scene
    pos0, vel0 = drop_scene(shape, STEP_SEEDS[shape])
    dt, acc = 0.5, 1e-4
    force = ops.default_gravity_force(shape, dt)
    a = b = z = (dev(pos0), ops.sample_velocity(dev(vel0), dev(pos0)), dev(vel0))
    for t in range(2):
        a = ops.liquid_step(a[0], a[1], a[2], dt, accuracy=acc, viscosity_alpha=None)
        assert len(a) == 4
        b = _parent_step(ops, b[0], b[1], b[2], dt, force, acc)
        z = ops.liquid_step(z[0], z[1], z[2], dt, accuracy=acc, viscosity_alpha=(0.0, 0.0))
        assert len(z) == 5 and not _np(z[4]).any()
        for k, name in enumerate(("pos", "pvel", "vel")):
            assert_bits(_np(a[k]), _np(b[k]), "step %d %s: None vs the step before viscosity" % (t, name))
            assert torch.equal(z[k], a[k]), (t, name)
        assert torch.equal(a[3], b[3]) and torch.equal(z[3], a[3])
    # keep_every: the same chain, every second step kept
    p, u, v = dev(pos0), dev(lref.sample(vel0, pos0, np.float32)), dev(vel0)
    s1, s2 = [], []
    _, _, all5 = ops.simulate_liquid(p, u, v, 5, dt=dt, viscosity_alpha=STEP_ALPHA, stats=s1)
    pk, uk, kept = ops.simulate_liquid(p, u, v, 5, dt=dt, viscosity_alpha=STEP_ALPHA, keep_every=2, stats=s2)
    assert tuple(all5.shape)[0] == 5 and tuple(kept.shape)[0] == 3 and len(s1) == 5 and len(s2) == 5
    assert torch.equal(kept, all5[[0, 2, 4]])
    assert all(torch.equal(x, y) for x, y in zip(s1, s2))
    frames = list(ops.simulate_liquid(p, u, v, 5, dt=dt, viscosity_alpha=STEP_ALPHA, keep_every=2, stack=False))
    assert len(frames) == 3 and all(torch.equal(f[2], kept[n]) for n, f in enumerate(frames))
    with pytest.raises(ValueError):
        ops.simulate_liquid(p, u, v, 2, keep_every=0)
    with pytest.raises(ValueError):
        ops.liquid_step(p, u, v, dt, viscosity_alpha=(0.1, -0.1))


# ---- 7: the dataset ------------------------------------------------------------------------------------------------------------------------------
def test_generate_liquid3_vis_dataset(tmp_path):
    from deep_fluids_amd import ops
    from deep_fluids_amd.data import BatchManager, generate_liquid3_vis_dataset
    from deep_fluids_amd.trainer import body_levelset, liquid3_vis_body
    root = str(tmp_path / "vis")
    X, Y, Z, T = 16, 12, 8, 2
    n = generate_liquid3_vis_dataset(root, resolution_x=X, resolution_y=Y, resolution_z=Z, num_viscosity=2, max_viscosity=1, num_frames=T,
                                     time_step=0.5)
    assert n == 4
    assert sorted(os.listdir(os.path.join(root, "v"))) == ["0_0.npz", "0_1.npz", "1_0.npz", "1_1.npz"]
    lo, hi = np.inf, -np.inf
    stored = {}
    for i in range(2):
        for f in range(T):
            with np.load(os.path.join(root, "v", "%d_%d.npz" % (i, f))) as d:
                assert sorted(d.files) == ["x", "y"]
                x, y = d["x"], d["y"]
            assert x.dtype == np.float32 and x.shape == (Z, Y, X, 3)
            np.testing.assert_array_equal(y, [float(i), f])
            lo, hi = min(lo, float(x.min())), max(hi, float(x.max()))
            stored[i, f] = x
    assert open(os.path.join(root, "v_range.txt")).read() == "%.3f\n%.3f" % (lo, hi)
    assert lo < 0                                                            # the box collapses
    args = dict(line.rstrip("\n").split(": ") for line in open(os.path.join(root, "args.txt")))
    assert list(args) == ["log_dir", "num_param", "path_format", "p0", "p1", "viscosity_base", "vmin", "vmax", "min_viscosity", "max_viscosity",
                          "num_viscosity", "src_x_pos", "src_y_pos", "src_z_pos", "min_frames", "max_frames", "num_frames", "num_simulations",
                          "resolution_x", "resolution_y", "resolution_z", "gravity", "radius_factor", "min_particles", "bWidth", "open_bound",
                          "time_step"]
    assert args["num_viscosity"] == "2" and args["max_frames"] == "1" and args["time_step"] == "0.5" and args["p0"] == "viscosity"
    cfg = SimpleNamespace(random_seed=1, data_path=root, is_3d=True, data_type="velocity", arch="de", batch_size=3, res_x=X, res_y=Y, res_z=Z,
                          num_worker=1)
    bm = BatchManager(cfg, device=None)
    xb, yb = bm.batch()
    bm.stop_thread()
    assert tuple(xb.shape) == (3, Z, Y, X, 3) and tuple(yb.shape) == (3, 2)
    # the same state and alphas through simulate_liquid: frame 1 is step 2 (time_step 0.5: two steps per frame), frame 0 is step 0
    shape = (Z, Y, X)
    phi = body_levelset(shape, liquid3_vis_body(bm))
    p, u, v = ops.liquid_initial_state(shape, phi)
    assert not v.any() and not u.any()
    vis_list = 2 * np.logspace(-5, -2, 2)
    alphas = [ops.diffusion_alpha(float(vis_list[i]), 0.5, X) for i in range(2)]
    two = [torch.cat([t, t]) for t in (p, u, v)]
    _, _, vels = ops.simulate_liquid(two[0], two[1], two[2], 3, dt=0.5, force=ops.default_gravity_force(shape, 0.5), viscosity_alpha=alphas)
    for i in range(2):
        assert_bits(_np(vels[0, i]), stored[i, 0], "frame 0 of scene %d" % i)
        assert_bits(_np(vels[2, i]), stored[i, 1], "frame 1 of scene %d" % i)
    assert not np.array_equal(stored[0, 1], stored[1, 1])                   # the viscosities differ
    with pytest.raises(NotImplementedError):
        generate_liquid3_vis_dataset(str(tmp_path / "open"), open_bound=True)
    with pytest.raises(ValueError):
        generate_liquid3_vis_dataset(str(tmp_path / "p0"), p0="src_x_pos")
    with pytest.raises(ValueError):
        generate_liquid3_vis_dataset(str(tmp_path / "dt"), time_step=0.3)


# ---- 8: the C-ABI's error rules, the wrapper's argument checks ----------------------------------------------------------------------------------
def test_cabi_error_paths():
    """One case per rule of the header; every one is answered on the host (the pointers are not device memory, so a launch would fault)."""
    from deep_fluids_amd import _lib
    h = _lib.lib()
    need2, need3 = h.df_diffuse_workspace_bytes(1, 1, 8, 8, 2), h.df_diffuse_workspace_bytes(1, 8, 8, 8, 3)
    assert need2 == h.df_pressure_workspace_bytes(2, 1, 8, 8) + 4 * 2 * 64 and need3 == h.df_pressure_workspace_bytes(3, 8, 8, 8) + 4 * 3 * 512
    assert h.df_diffuse_workspace_bytes(1, 1, 8, 8, 4) == -1 and h.df_diffuse_workspace_bytes(0, 1, 8, 8, 2) == -1
    buf = ctypes.create_string_buffer(need3 + (1 << 16))
    a = (ctypes.addressof(buf) + 15) & ~15
    vel, al, ws = a, a + 8192, a + 16384
    # null
    assert h.df_diffuse_init2d(None, al, ws, need2, 1, 8, 8, 1, None) == -1 and b"null velocity" in h.df_last_error()
    assert h.df_diffuse_init3d(vel, None, ws, need3, 1, 8, 8, 8, 1, None) == -1 and b"null alpha" in h.df_last_error()
    assert h.df_diffuse_init2d(vel, al, None, need2, 1, 8, 8, 1, None) == -1 and b"null workspace" in h.df_last_error()
    assert h.df_diffuse_cg_direction2d(None, ws, need2, 1, 8, 8, 1, 0, 1e-4, 10, None) == -1 and b"null alpha" in h.df_last_error()
    assert h.df_diffuse_cg_direction3d(al, None, need3, 1, 8, 8, 8, 1, 0, 1e-4, 10, None) == -1
    assert h.df_diffuse_cg_update2d(None, need2, 1, 8, 8, 1, 0, None) == -1 and h.df_diffuse_cg_update3d(None, need3, 1, 8, 8, 8, 1, 0, None) == -1
    assert h.df_diffuse_finish2d(ws, need2, None, 1, 8, 8, 1, None) == -1 and b"null output" in h.df_last_error()
    assert h.df_diffuse_finish3d(None, need3, vel, 1, 8, 8, 8, 1, None) == -1
    # bnd = 0
    assert h.df_diffuse_init2d(vel, al, ws, need2, 1, 8, 8, 0, None) == -1 and b"boundary width" in h.df_last_error()
    assert h.df_diffuse_cg_direction3d(al, ws, need3, 1, 8, 8, 8, 0, 0, 1e-4, 10, None) == -1
    assert h.df_diffuse_cg_update2d(ws, need2, 1, 8, 8, 0, 0, None) == -1
    assert h.df_diffuse_finish3d(ws, need3, vel, 1, 8, 8, 8, 0, None) == -1
    # extents <= 2 * bnd
    assert h.df_diffuse_init2d(vel, al, ws, need2, 1, 8, 2, 1, None) == -2 and b"2*bnd + 2" in h.df_last_error()
    assert h.df_diffuse_init3d(vel, al, ws, need3, 1, 4, 8, 8, 2, None) == -2
    assert h.df_diffuse_cg_direction2d(al, ws, need2, 1, 2, 8, 1, 0, 1e-4, 10, None) == -2
    assert h.df_diffuse_cg_update3d(ws, need3, 1, 8, 1, 8, 1, 0, None) == -2
    assert h.df_diffuse_finish2d(ws, need2, vel, 1, 8, 4, 2, None) == -2
    # a workspace short by 4 bytes
    assert h.df_diffuse_init2d(vel, al, ws, need2 - 4, 1, 8, 8, 1, None) == -4
    assert h.df_diffuse_init3d(vel, al, ws, need3 - 4, 1, 8, 8, 8, 1, None) == -4
    assert h.df_diffuse_cg_direction2d(al, ws, need2 - 4, 1, 8, 8, 1, 0, 1e-4, 10, None) == -4
    assert h.df_diffuse_cg_update3d(ws, need3 - 4, 1, 8, 8, 8, 1, 0, None) == -4
    assert h.df_diffuse_finish2d(ws, need2 - 4, vel, 1, 8, 8, 1, None) == -4
    # a negative max_iter, a negative k
    assert h.df_diffuse_cg_direction2d(al, ws, need2, 1, 8, 8, 1, 0, 1e-4, -1, None) == -1 and b"iteration" in h.df_last_error()
    assert h.df_diffuse_cg_direction3d(al, ws, need3, 1, 8, 8, 8, 1, 0, 1e-4, -1, None) == -1
    assert h.df_diffuse_cg_update2d(ws, need2, 1, 8, 8, 1, -1, None) == -1
    # alignment, overlap with the workspace
    assert h.df_diffuse_init2d(vel + 2, al, ws, need2, 1, 8, 8, 1, None) == -3
    assert h.df_diffuse_init2d(ws + 16, al, ws, need2, 1, 8, 8, 1, None) == -1 and b"overlaps" in h.df_last_error()
    assert h.df_diffuse_finish2d(ws, need2, ws + need2 - 4, 1, 8, 8, 1, None) == -1 and b"overlaps" in h.df_last_error()
    torch.cuda.synchronize()                                                 # nothing was enqueued, nothing faults


def test_wrapper_argument_checks():
    from deep_fluids_amd import ops
    v = dev(_vel((6, 7)))
    for bad in (-0.1, float("nan"), float("inf"), (0.1, -1.0), (0.1, float("nan"))):
        with pytest.raises(ValueError):
            ops.diffuse_velocity(v, bad)
    for bad in ((0.1,), (0.1, 0.2, 0.3), np.zeros((2, 1))):
        with pytest.raises(ValueError):
            ops.diffuse_velocity(v, bad)
    with pytest.raises(ValueError):
        ops.diffuse_velocity(v.double(), 0.1)
    with pytest.raises(ValueError):
        ops.diffuse_velocity(v.transpose(1, 2), 0.1)
    with pytest.raises(ValueError):
        ops.diffuse_velocity(v, 0.1, out=torch.empty((2, 6, 8, 2), device="cuda"))
    with pytest.raises(ValueError):
        ops.diffuse_velocity(v, 0.1, out=torch.empty_like(v, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.diffuse_velocity(v, 0.1, workspace=torch.empty((16,), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):                                         # one float short
        ops.diffuse_velocity(v, 0.1, workspace=ops.diffusion_workspace(v)[1:].clone())
    for kw in (dict(bnd=0), dict(accuracy=-1.0), dict(max_iter=-1), dict(check_every=0)):
        with pytest.raises(ValueError):
            ops.diffuse_velocity(v, 0.1, **kw)
    x, iters = ops.diffuse_velocity(v, np.array([0.1, 0.2], np.float32))     # an ndarray of B floats is fine
    assert tuple(x.shape) == tuple(v.shape) and tuple(iters.shape) == (2, 2)
