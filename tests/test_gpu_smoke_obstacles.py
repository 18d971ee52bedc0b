"""GPU side of the smoke solver around obstacles (the `_flags` entry points of smoke.hip / advect.hip, ops' ``obstacle=`` keyword, the
3-D obstacle data set): against the fp64 restatement of tests/smoke_obs_ref.py with tolerances measured from its fp32 twin in the same
test.  Every parity test prints its figures before it asserts.

Shapes are smoke_ref.MAC_SHAPES; the obstacles (smoke_obs_ref.obstacle_cases) sit at the edges of the rule: one solid cell in
mid-fluid, a block on the wall, a solid run across a 256-cell workgroup boundary, a sphere, a wall that splits the box into two fluid
regions, an enclosed fluid cell (n_c = 0), an entry that is solid everywhere, different obstacles per batch entry."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import advect_ref as aref
import smoke_obs_ref as oref
import smoke_ref as ref
from gpu_util import assert_bits, dev

pytestmark = pytest.mark.gpu

SHAPES = [(s, b) for s, bnds in ref.MAC_SHAPES for b in bnds]
SOLVE_SHAPES = [((6, 6), 1), ((9, 7), 1), ((12, 10), 2), ((17, 130), 1), ((6, 6, 6), 1), ((7, 8, 6), 1), ((19, 10, 7), 2)]


def _np(t):
    return t.cpu().numpy()


def _obs(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _all_obstacles(shape, bnd):
    c = oref.obstacle_cases(shape, bnd)
    names = sorted(c)
    return names, np.stack([c[n] for n in names])


# ---- 1. zero obstacle: the bits of the unmasked path ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,bnd", SHAPES)
@pytest.mark.parametrize("B", [1, 3])
def test_zero_obstacle_is_bitwise_the_unmasked_path(shape, bnd, B):
    from deep_fluids_amd import ops
    D = len(shape)
    vel = dev(ref.make_velocity(shape, B=B, seed=1, vmax=min(3.0, 0.4 * min(shape))))
    rho = dev(ref.make_density(shape, B=B, seed=1))
    zero = torch.zeros((B,) + shape, dtype=torch.uint8, device="cuda")
    flags = ops.obstacle_flags(zero, bnd)
    for obstacle in (zero, flags, zero[0]):
        for mode in (1, 2):
            assert torch.equal(ops.advect(rho, vel, 1.0, clamp_mode=mode, bnd=bnd, obstacle=obstacle), ops.advect(rho, vel, 1.0, clamp_mode=mode, bnd=bnd))
            assert torch.equal(ops.advect_velocity(vel, 1.0, clamp_mode=mode, bnd=bnd, obstacle=obstacle),
                               ops.advect_velocity(vel, 1.0, clamp_mode=mode, bnd=bnd))
        force = (0.013, 0.256, -0.07)[:D]
        w = ops.wall_buoyancy(vel, rho, force, bnd=bnd)
        assert torch.equal(ops.wall_buoyancy(vel, rho, force, bnd=bnd, obstacle=obstacle), w)
        for kw in (dict(), dict(accuracy=0.0, max_iter=3)):
            got, want = ops.solve_pressure(w, bnd=bnd, obstacle=obstacle, **kw), ops.solve_pressure(w, bnd=bnd, **kw)
            for g, t in zip(got, want):
                assert torch.equal(g, t)
    assert torch.equal(ops.advect(rho, vel, 1.0, order=1, bnd=bnd, obstacle=zero), ops.advect(rho, vel, 1.0, order=1, bnd=bnd))
    src = _obs(aref.sphere_mask_loop(shape, [0.5 * n for n in shape[::-1]], 1.5))
    d0, v0 = torch.zeros_like(rho), torch.zeros_like(vel)
    s1, s2 = [], []
    dm, vm = ops.simulate_smoke(d0, v0, 8, source=src, bnd=bnd, obstacle=flags, stats=s1)
    du, vu = ops.simulate_smoke(d0, v0, 8, source=src, bnd=bnd, stats=s2)
    assert torch.equal(dm, du) and torch.equal(vm, vu) and all(torch.equal(a, b) for a, b in zip(s1, s2))
    assert float(vu.abs().max()) > 0


# ---- 2. flags and wall_buoyancy: bitwise against the restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape,bnd", SHAPES)
def test_flags_and_wall_buoyancy_bitwise(shape, bnd):
    from deep_fluids_amd import ops
    D = len(shape)
    names, obs = _all_obstacles(shape, bnd)
    B = len(names)
    flags = ops.obstacle_flags(_obs(obs), bnd)
    assert isinstance(flags, ops.ObstacleFlags) and flags.bnd == bnd and flags.dtype == torch.uint8 and tuple(flags.shape) == obs.shape
    np.testing.assert_array_equal(_np(flags), oref.flags(obs, bnd))
    np.testing.assert_array_equal(_np(ops.obstacle_flags(_obs(obs[1]), bnd, dim=D))[0], oref.flags(obs[1:2], bnd)[0])     # [(Z,)Y,X]
    np.testing.assert_array_equal(_np(ops.obstacle_flags(_obs(obs != 0), bnd)), oref.flags(obs, bnd))                    # a bool mask
    rng = np.random.RandomState(11)
    vel = ref.make_velocity(shape, B=B, seed=2)
    rho = rng.uniform(0, 1, (B,) + shape).astype(np.float32)
    force = (0.013, 0.256, -0.07)[:D]
    want = oref.wall_buoyancy(vel, rho, force, obs, bnd, np.float32)
    fluid = oref.fluid_mask(obs, bnd)
    v = dev(vel)
    for obstacle in (_obs(obs), flags):
        got = ops.wall_buoyancy(v, dev(rho), force, bnd=bnd, obstacle=obstacle)
        assert_bits(_np(got), want, "wall_buoyancy")
    for a in range(D):
        assert not _np(got)[..., a][~oref.face_mask(fluid, a)].any()                    # solid faces are exactly 0
    assert not _np(got)[names.index("solid")].any()
    assert_bits(_np(v), vel, "input untouched")
    assert ops.wall_buoyancy(v, dev(rho), force, bnd=bnd, out=v, obstacle=flags) is v    # in place
    assert torch.equal(v, got)
    with pytest.raises(ValueError):
        ops.wall_buoyancy(v, dev(rho), force, bnd=bnd + 1, obstacle=flags)               # flags of another boundary width
    with pytest.raises(ValueError):
        ops.wall_buoyancy(v, dev(rho), force, bnd=bnd, obstacle=torch.zeros((B + 1,) + shape, dtype=torch.uint8))


# ---- 3. advection parity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mac", "density"])
def test_masked_advection_parity_with_the_fp64_restatement(kind):
    from deep_fluids_amd import ops
    n = 0
    for name, vel, rho, obs, kw in oref.advect_cases(kind):
        o = _obs(obs)
        if kind == "mac":
            r64 = oref.mac_advect(vel, oref.OBS_DT, obs, dtype=np.float64, **kw)
            r32 = oref.mac_advect(vel, oref.OBS_DT, obs, dtype=np.float32, **kw)
            alt = oref.mac_alternatives(r64, vel, oref.OBS_DT, kw["clamp_mode"], kw["bnd"], obs)
            run = lambda sl: ops.advect_velocity(dev(vel[sl]), oref.OBS_DT, obstacle=o[sl], **kw)
            got = _np(run(slice(None)))
            gs = ref.vel_to_stacked(got)
        else:
            r64 = oref.advect_density(rho, vel, oref.OBS_DT, obs, dtype=np.float64, **kw)
            r32 = oref.advect_density(rho, vel, oref.OBS_DT, obs, dtype=np.float32, **kw)
            alt = oref.alternatives(r64, vel, oref.OBS_DT, kw["clamp_mode"], kw["bnd"], obs)
            run = lambda sl: ops.advect(dev(rho[sl]), dev(vel[sl]), oref.OBS_DT, obstacle=o[sl], **kw)
            got = _np(run(slice(None)))
            gs = got
        e32, twin_out = aref.twin_error(r64, r32, kw["bnd"])
        assert got.dtype == np.float32
        print("%-28s e32 %.3e  gpu max %.3e  twin left out %.5f %%  gpu == twin bitwise: %s" %
              (name, e32, float(np.abs(gs - r64["out"]).max()), 100 * twin_out, bool(np.array_equal(gs, r32["out"]))))
        err, share = aref.compare(gs, r64, e32, kw["bnd"], alt)
        print("%-28s gpu %.3e (bound %.3e)  left out %.5f %%" % ("", err, 3 * e32 + 1e-7, 100 * share))
        for e in range(obs.shape[0]):                       # an entry alone is that entry of the batch, bit for bit
            assert_bits(_np(run(slice(e, e + 1))), got[e:e + 1], name + " entry %d alone" % e)
        n += 1
    assert n == 20


# ---- 4. conjugate gradients ------------------------------------------------------------------------------------------------------------------------
def _check_contract(names, obs, bnd, v, p, iters, w):
    shape = obs.shape[1:]
    fluid = oref.fluid_mask(obs, bnd)
    assert np.isfinite(p).all() and np.isfinite(v).all()
    assert not p[~fluid].any()                                          # p is 0 outside the fluid
    for a in range(len(shape)):
        assert not v[..., a][~oref.face_mask(fluid, a)].any()           # no velocity on a solid face
    s = names.index("solid")
    assert iters[s] == 0 and not p[s].any() and not v[s].any()
    e = names.index("enclosed")
    mid = tuple(n // 2 for n in shape)
    assert fluid[e][mid] and p[e][mid] == 0 and not v[e][mid].any()


@pytest.mark.parametrize("shape,bnd", SOLVE_SHAPES)
def test_k_iterations_against_the_fp64_recurrence(shape, bnd):
    from deep_fluids_amd import ops
    names, obs = _all_obstacles(shape, bnd)
    w = oref.solve_input(shape, bnd, obs)
    live = np.array([n != "solid" for n in names])
    flags = ops.obstacle_flags(_obs(obs), bnd)
    for k in (1, 2, 3, 4):
        x64, it64, _ = oref.cg(w, obs, bnd, 0.0, k, np.float64)
        x32, _, _ = oref.cg(w, obs, bnd, 0.0, k, np.float32)
        e32 = float(np.abs(x32 - x64).max())
        v, p, iters = ops.solve_pressure(dev(w), bnd=bnd, accuracy=0.0, max_iter=k, obstacle=flags)
        err = float(np.abs(_np(p) - x64).max())
        print("%s bnd %d k %d: e32 %.3e  gpu %.3e (bound %.3e)  |x| %.3e" % (shape, bnd, k, e32, err, 3 * e32 + 1e-7, float(np.abs(x64).max())))
        assert (_np(iters)[live] == k).all() and (it64[live] == k).all()
        assert err <= 3 * e32 + 1e-7
        _check_contract(names, obs, bnd, _np(v), _np(p), _np(iters), w)


@pytest.mark.parametrize("shape,bnd", SOLVE_SHAPES)
def test_solve_residual_and_projection(shape, bnd):
    from deep_fluids_amd import ops
    names, obs = _all_obstacles(shape, bnd)
    w = oref.solve_input(shape, bnd, obs)
    live = np.array([n != "solid" for n in names])
    acc = 1e-4
    max_iter = ops.default_max_iter(shape)
    b64 = oref.rhs(w, obs, bnd, np.float64)
    v, p, iters = ops.solve_pressure(dev(w), bnd=bnd, accuracy=acc, obstacle=_obs(obs))
    x32, it32, r32 = oref.cg(w, obs, bnd, acc, max_iter, np.float32)
    # the twin's own excess (see test_gpu_smoke.py): |b - A p| <= |r| + drift, the drift measured on the twin in fp64
    excess = float(np.abs((b64 - oref.apply_A(x32.astype(np.float64), obs, bnd)) - r32).max())
    res = float(np.abs(b64 - oref.apply_A(_np(p).astype(np.float64), obs, bnd)).max())
    print("%s bnd %d: iterations gpu %s twin %s  fp64 residual of the gpu's p %.4e (bound %.1e + twin's excess %.3e)" %
          (shape, bnd, _np(iters).tolist(), it32.tolist(), res, acc, excess))
    assert (_np(iters)[live] > 0).all() and (_np(iters) < max_iter).all()
    assert res <= acc + excess
    if int(oref.fluid_mask(obs, bnd).sum(axis=tuple(range(1, obs.ndim))).max()) <= 1200:
        vex, _ = oref.exact_projection(w, obs, bnd)
        v32 = oref.correct(w, x32, obs, bnd, np.float32)
        d32 = float(np.abs(v32 - vex).max())
        dg = float(np.abs(_np(v) - vex).max())
        print("%s bnd %d: distance from the exact fp64 projection: twin %.3e  gpu %.3e" % (shape, bnd, d32, dg))
        assert dg <= 3 * d32
    _check_contract(names, obs, bnd, _np(v), _np(p), _np(iters), w)


# ---- 5. batch invariance, determinism, check_every ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,bnd", [((12, 10), 1), ((17, 130), 1), ((19, 10, 7), 1)])
def test_batch_invariance_determinism_and_check_every(shape, bnd):
    from deep_fluids_amd import ops
    names, obs = _all_obstacles(shape, bnd)
    w = oref.solve_input(shape, bnd, obs)
    o = _obs(obs)
    flags = ops.obstacle_flags(o, bnd)
    v, p, iters = ops.solve_pressure(dev(w), bnd=bnd, obstacle=flags)
    it = _np(iters).tolist()
    print("%s: obstacles %s iterations %s" % (shape, names, it))
    _check_contract(names, obs, bnd, _np(v), _np(p), it, w)
    for e in range(len(names)):
        ve, pe, ie = ops.solve_pressure(dev(w[e:e + 1]), bnd=bnd, obstacle=o[e:e + 1])
        vf, pf, jf = ops.solve_pressure(dev(w[e:e + 1]), bnd=bnd, obstacle=flags[e:e + 1])      # a slice of flags is still flags
        assert torch.equal(vf, ve) and torch.equal(pf, pe) and torch.equal(jf, ie)
        assert_bits(_np(pe)[0], _np(p)[e], "pressure of entry %d alone" % e)
        assert_bits(_np(ve)[0], _np(v)[e], "velocity of entry %d alone" % e)
        assert int(ie[0]) == it[e]
    ws = ops.pressure_workspace(dev(w))
    ws.fill_(float("nan"))                                 # nothing is read before it is written
    for ce in (None, 1, 16, 64):
        v2, p2, i2 = ops.solve_pressure(dev(w), bnd=bnd, check_every=ce, workspace=ws, obstacle=flags)
        assert_bits(_np(p2), _np(p), "check_every %s" % ce)
        assert_bits(_np(v2), _np(v), "check_every %s" % ce)
        assert torch.equal(i2, iters)
    vi = dev(w)
    assert ops.solve_pressure(vi, bnd=bnd, out=vi, obstacle=flags)[0] is vi and torch.equal(vi, v)            # in place


# ---- 6. the step ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(32, 24), (12, 16, 12)])
def test_step_equals_its_parts_and_eight_steps_from_rest(shape):
    from deep_fluids_amd import ops
    D = len(shape)
    ext = shape[::-1]
    B = 2
    src, obs = [], []
    for e in range(B):                                       # a sphere obstacle above the source, at another x per entry
        c = [0.5 * n for n in ext]
        c[1] = 0.15 * ext[1]
        src.append(aref.sphere_mask_loop(shape, c, 0.12 * ext[0]))
        c[0] = (0.4 + 0.2 * e) * ext[0]
        c[1] = 0.5 * ext[1]
        obs.append(aref.sphere_mask_loop(shape, c, 0.15 * ext[0]))
    src, obs = np.stack(src), np.stack(obs)
    assert obs.any() and not (src & obs).any()
    fluid = oref.fluid_mask(obs, 1)
    m, o = _obs(src), _obs(obs)
    flags = ops.obstacle_flags(o, 1)
    dt, acc, T = 0.5, 1e-4, 8
    force = ops.default_buoyancy_force(shape, dt)
    stats = []
    d0, v0 = torch.zeros((B,) + shape, device="cuda"), torch.zeros((B,) + shape + (D,), device="cuda")
    dT, vels = ops.simulate_smoke(d0, v0, T, dt=dt, source=m, stats=stats, obstacle=o)
    d, v = d0, v0
    for t in range(T):
        dn = ops.advect(d, v, dt, source=m, obstacle=flags)
        vn = ops.advect_velocity(v, dt, obstacle=flags)
        vn = ops.wall_buoyancy(vn, dn, force, obstacle=flags)
        vn, _, it = ops.solve_pressure(vn, obstacle=flags)
        ds, vs = ops.smoke_step(d, v, dt, source=m, obstacle=o)
        assert torch.equal(ds, dn) and torch.equal(vs, vn)                       # bitwise
        assert torch.equal(vels[t], vn) and torch.equal(stats[t], it)
        d, v = dn, vn
        vh, dh = _np(v), _np(d)
        div = float(np.abs(oref.divergence(vh, obs, 1)).max())
        print("%s step %d: iterations %s  max|div| in fluid %.3e  density in fluid [%.4f, %.4f]  max|v| %.4f" %
              (shape, t + 1, _np(it).tolist(), div, float(dh[fluid].min()), float(dh[fluid].max()), float(np.abs(vh).max())))
        assert div <= acc * (2 * D + 1)                  # |div| = |b - A p| up to rounding: the residual bound times the stencil's width
        assert dh[fluid].min() >= 0.0 and dh[fluid].max() <= 1.0                 # clamp mode 2 over fluid corners adds no extremum
        for a in range(D):
            assert not vh[..., a][~oref.face_mask(fluid, a)].any()               # no velocity on any solid face
    assert torch.equal(dT, d)
    assert float(vels[-1].abs().max()) > 0.01
    assert not torch.equal(vels[-1][0], vels[-1][1])                             # the obstacle's position matters


# ---- 7. the data set ---------------------------------------------------------------------------------------------------------------------------------
def test_generate_smoke3_obs_dataset(tmp_path):
    from deep_fluids_amd import ops
    from deep_fluids_amd.data import BatchManager, generate_smoke3_obs_dataset
    from deep_fluids_amd.trainer import smoke3_obs_buo_scene
    root = str(tmp_path / "smoke3_obs")
    X, Y, Z, T = 12, 16, 12, 4
    n = generate_smoke3_obs_dataset(root, num_obs_x_pos=3, num_buoyancy=2, num_frames=T, resolution_x=X, resolution_y=Y, resolution_z=Z,
                                    scenes_per_batch=2)
    assert n == 3 * 2 * T
    assert sorted(os.listdir(os.path.join(root, "v"))) == sorted("%d_%d_%d.npz" % (i, j, t) for i in range(3) for j in range(2) for t in range(T))
    args = dict(line.rstrip("\n").split(": ") for line in open(os.path.join(root, "args.txt")))
    want_keys = ["log_dir", "num_param", "path_format", "p0", "p1", "p2", "min_obs_x_pos", "max_obs_x_pos", "num_obs_x_pos", "obs_radius",
                 "obs_y_pos", "obs_z_pos", "min_buoyancy", "max_buoyancy", "num_buoyancy", "src_x_pos", "src_y_pos", "src_z_pos", "src_radius",
                 "min_frames", "max_frames", "num_frames", "num_simulations", "resolution_x", "resolution_y", "resolution_z", "bWidth",
                 "open_bound", "time_step", "adv_order", "clamp_mode"]
    assert list(args) == want_keys
    assert args["num_obs_x_pos"] == "3" and args["max_frames"] == "3" and args["p0"] == "obs_x_pos" and args["open_bound"] == "False"
    xs, bs = np.linspace(0.2, 0.8, 3), np.linspace(-8e-3, -16e-3, 2)
    lo, hi = np.inf, -np.inf
    for i in range(3):
        for j in range(2):
            for t in range(T):
                with np.load(os.path.join(root, "v", "%d_%d_%d.npz" % (i, j, t))) as f:
                    assert sorted(f.files) == ["x", "y"]
                    x, y = f["x"], f["y"]
                assert x.dtype == np.float32 and x.shape == (Z, Y, X, 3)
                np.testing.assert_array_equal(y, [xs[i], bs[j], t])
                lo, hi = min(lo, float(x.min())), max(hi, float(x.max()))
    assert open(os.path.join(root, "v_range.txt")).read() == "%.3f\n%.3f" % (lo, hi)
    assert hi > 0.01
    cfg = SimpleNamespace(random_seed=1, data_path=root, is_3d=True, data_type="velocity", arch="de", batch_size=5, res_x=X, res_y=Y, res_z=Z,
                          num_worker=1)
    bm = BatchManager(cfg, device=None)
    xb, yb = bm.batch()
    bm.stop_thread()
    assert tuple(xb.shape) == (5, Z, Y, X, 3) and tuple(yb.shape) == (5, 3)
    assert float(xb.abs().max()) <= 1 + 0.0005 / bm.x_range and float(yb.abs().max()) <= 1
    source, obstacle = smoke3_obs_buo_scene(bm, 1, 1)
    assert source == {"center": (X * 0.5, Y * 0.13, Z * 0.5), "radius": X * 0.12}
    assert obstacle == {"center": (X * xs[1], Y * 0.5, Z * 0.5), "radius": X * 0.15}
    smask = ops.sphere_mask((Z, Y, X), source["center"], source["radius"], "cuda")
    omask = ops.sphere_mask((Z, Y, X), obstacle["center"], obstacle["radius"], "cuda")
    assert int(smask.sum()) > 0 and int(omask.sum()) > 0
    # scene (1, 1) alone, re-simulated with the sphere the helper returns: the stored frames bit for bit
    d0 = torch.zeros((1, Z, Y, X), device="cuda")
    v0 = torch.zeros((1, Z, Y, X, 3), device="cuda")
    _, vels = ops.simulate_smoke(d0, v0, T, dt=0.5, source=smask, force=ops.default_buoyancy_force((Z, Y, X), 0.5, gravity=bs[1]),
                                 obstacle=omask)
    for t in range(T):
        with np.load(os.path.join(root, "v", "1_1_%d.npz" % t)) as f:
            assert_bits(_np(vels[t, 0]), f["x"], "frame %d of scene (1, 1)" % t)
            assert not f["x"][omask.cpu().numpy() != 0].any()
    # Trainer3.advect_ on it, around the obstacle (an untrained generator: the plumbing is what is checked)
    from deep_fluids_amd.trainer import Trainer3, default_config
    tcfg = default_config(is_3d=True, res_x=X, res_y=Y, res_z=Z, filters=16, batch_size=2, num_samples=n, model_dir=str(tmp_path / "run"),
                          test_batch_size=2)
    ops.reset_variables()
    tr = Trainer3(tcfg)
    out_dir, final = tr.advect_(bm, p1=1, p2=1, source=source, obstacle=obstacle)
    assert sorted(os.listdir(out_dir)) == ["%04d.png" % t for t in range(T)] and out_dir.endswith(os.path.join("1_1", "d_adv"))
    y1, y2 = int(bm.y_num[0]), int(bm.y_num[1])
    z_c = np.zeros((T, tr.c_num), np.float32)
    z_c[:, 0] = 1 / float(y1 - 1) * 2 - 1
    z_c[:, 1] = 1 / float(y2 - 1) * 2 - 1
    z_c[:, -1] = np.linspace(-1, 1, num=T)
    frames = torch.cat([tr.generate(torch.from_numpy(z_c[2 * i:2 * (i + 1)]).cuda()) for i in range(T // 2)], dim=0)
    want = ops.advect_sequence(d0, frames.unsqueeze(1), 0.5, vel_scale=float(bm.x_range), source=smask, obstacle=omask)
    assert final.is_cuda and torch.equal(final, want) and float(final.max()) > 0             # bitwise: dt is the set's time_step
    with pytest.raises(NotImplementedError):
        generate_smoke3_obs_dataset(str(tmp_path / "open"), open_bound=True)
