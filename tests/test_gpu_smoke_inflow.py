"""GPU side of the noise inflow, the cylinder stamp and the per-entry force (df_density_noise_inflow*, df_mac_cylinder_stamp*,
df_wall_buoyancy*_open_dev; ops' ``NoiseInflow``, ``stamp_velocity``, ``inflow_velocity=`` and tensor ``force``; the smoke3_vel_buo data
set): against the restatement of tests/smoke_inflow_ref.py -- a restatement of this project's own definition and its own lattice noise,
not of mantaflow -- with tolerances measured from its fp32 twin in the same test.  Every parity test prints its figures before it asserts.

Shapes are smoke_ref.MAC_SHAPES with their bnds: odd extents, (17, 130) with an x extent above a wavefront that is no multiple of 64,
(19, 10, 7), bnd = 2."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import advect_ref as aref
import smoke_inflow_ref as iref
import smoke_obs_ref as oref
import smoke_open_ref as pref
import smoke_ref as ref
from gpu_util import Guarded, assert_bits, dev

pytestmark = pytest.mark.gpu

SHAPES = [(s, b) for s, bnds in ref.MAC_SHAPES for b in bnds]
assert ((17, 130), 2) in SHAPES and ((19, 10, 7), 2) in SHAPES


def _np(t):
    return t.cpu().numpy()


def _obs(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _eighths(x):
    return np.floor(np.asarray(x, np.float64) * 8.0) / 8.0


def _stamp_cylinders(shape):
    """[D + 2, 2D+1], every number a multiple of 1/8: one cylinder along each axis, one partly outside the grid, one NaN entry"""
    D = len(shape)
    ext = np.array(shape[::-1], np.float64)
    rows = []
    for a in range(D):
        z = np.zeros(D); z[a] = 1.5
        rows.append(np.concatenate([_eighths(0.5 * ext) + 0.125 * (a + 1), z, [min(2.125, 0.25 * ext.min() + 0.625)]]))
    z = np.zeros(D); z[0] = 2.25
    c = _eighths(0.5 * ext); c[0] = -0.5
    rows.append(np.concatenate([c, z, [1.875]]))
    rows.append(np.concatenate([_eighths(0.5 * ext), z, [np.nan]]))
    return np.array(rows, np.float32)


def _noise_field(noise):
    from deep_fluids_amd import ops
    return ops.NoiseField(**noise)


# ---- 1. the stamp: bitwise ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,bnd", SHAPES)
def test_cylinder_stamp_bitwise(shape, bnd):
    from deep_fluids_amd import _lib, ops
    D = len(shape)
    cyl = _stamp_cylinders(shape)
    B = cyl.shape[0]
    dims = [B] + list(shape)
    stream = torch.cuda.current_stream().cuda_stream
    vel = ref.make_velocity(shape, B=B, seed=3)
    values = np.array([[b + 1 + 0.25 * a for a in range(D)] for b in range(B)], np.float32)
    want = iref.cylinder_stamp(vel, cyl, values, np.float32)
    assert_bits(want, iref.cylinder_stamp(vel, cyl, values, np.float64).astype(np.float32), "the restatement is exact here")
    for b in range(B - 1):
        for a in range(D):
            assert (want[b, ..., a] == values[b, a]).sum() > 0, (b, a)          # every cylinder stamps every component somewhere
    assert_bits(want[B - 1], vel[B - 1], "NaN entry")
    hit = [want[..., a] != vel[..., a] for a in range(D)]
    assert any(not np.array_equal(hit[0], h) for h in hit[1:])                  # the faces are tested one by one
    vin, cin, uin, out = Guarded(vel.shape, vel), Guarded(cyl.shape, cyl), Guarded(values.shape, values), Guarded(vel.shape)
    _lib.call("df_mac_cylinder_stamp%dd" % D, vin.ptr, cin.ptr, uin.ptr, out.ptr, *(dims + [stream]))
    assert_bits(out.get("stamp"), want, "stamp")
    _lib.call("df_mac_cylinder_stamp%dd" % D, vin.ptr, cin.ptr, uin.ptr, vin.ptr, *(dims + [stream]))           # out == vel
    assert_bits(vin.get("stamp in place"), want, "stamp in place")
    cin.check_guards(); uin.check_guards()
    shp = ops.CylinderShape(torch.from_numpy(cyl[:, :D]).cuda(), torch.from_numpy(cyl[:, D:2 * D]).cuda(), torch.from_numpy(cyl[:, 2 * D]).cuda())
    v = dev(vel)
    assert_bits(_np(ops.stamp_velocity(v, shp, values)), want, "ops.stamp_velocity")
    assert_bits(_np(v), vel, "the input is left alone")
    assert ops.stamp_velocity(v, shp, torch.from_numpy(values), out=v) is v
    assert_bits(_np(v), want, "ops.stamp_velocity in place")
    one = ops.stamp_velocity(dev(vel[:1]), shp.entry(0), values[0])            # [D] values, one entry
    assert_bits(_np(one), want[:1], "one entry, [D] values")


# ---- 2. the inflow against the fp64 restatement ----------------------------------------------------------------------------------------------------
def _inflow_cylinders(shape):
    """along y; tilted (not exact in fp32); wholly outside the grid; partly outside"""
    D = len(shape)
    ext = np.array(shape[::-1], np.float64)
    mid = 0.5 * ext
    r = max(1.5, 0.2 * ext.min())
    tilt = np.array([0.9, 1.3, 0.7][:D])
    y = np.zeros(D); y[1] = max(1.0, 0.12 * ext[1])
    far = mid.copy(); far[0] = ext[0] + 3 * r + 8
    edge = mid.copy(); edge[0] = 0.3
    return np.array([np.concatenate([mid - 0.3, y, [r]]), np.concatenate([mid + 0.2, tilt, [0.8 * r]]), np.concatenate([far, y, [r]]),
                     np.concatenate([edge, tilt[::-1], [r]])], np.float32)


@pytest.mark.parametrize("shape,bnd", SHAPES)
def test_noise_inflow_against_the_fp64_restatement(shape, bnd):
    from deep_fluids_amd import _lib, ops
    D = len(shape)
    cyl = _inflow_cylinders(shape)
    B = cyl.shape[0]
    dims = [B] + list(shape)
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.RandomState(5)
    rho = rng.uniform(0, 0.3, (B,) + shape).astype(np.float32)
    shp = ops.CylinderShape(cyl[:, :D], cyl[:, D:2 * D], cyl[:, 2 * D])
    for sigma, time, scale, noise in ((0.5, 0.0, 1.0, iref.noise_params()), (2.0, 1.5, 1.25, iref.noise_params(clamp=False, pos_offset=-0.375, seed=77)),
                                      (0.5, 7.0, 1.0, iref.noise_params(pos_scale=[45.0, 30.0, 17.0][:D], val_offset=0.5, val_scale=1.5))):
        o64, region, target = iref.density_inflow(rho, cyl, noise, time, scale, sigma, bnd, np.float64, parts=True)
        o32 = iref.density_inflow(rho, cyl, noise, time, scale, sigma, bnd, np.float32)
        e32 = float(np.abs(o32.astype(np.float64) - o64).max())
        q = _noise_field(noise).params(D, shape[-1])
        rin, cin, out = Guarded(rho.shape, rho), Guarded(cyl.shape, cyl), Guarded(rho.shape)
        _lib.call("df_density_noise_inflow%dd" % D, rin.ptr, out.ptr, cin.ptr, ctypes.addressof(q), time, scale, sigma, *(dims + [bnd, stream]))
        got = out.get("inflow")
        err = float(np.abs(got.astype(np.float64) - o64).max())
        name = "%s bnd %d sigma %.1f time %.1f clamp %s" % ("x".join(map(str, shape)), bnd, sigma, time, noise["clamp"])
        print("%-44s region %5d cells  target std %.3f  e32 %.3e  gpu %.3e (bound %.3e)  gpu == twin bitwise: %s" %
              (name, int(region.sum()), float(target[region].std()), e32, err, 3 * e32 + 1e-7, bool(np.array_equal(got, o32))))
        # the stamped region is not empty, the target varies inside it, and the inflow changes the density there: no constant passes
        assert region[0].sum() >= 8 and region[1].sum() >= 8 and float(target[region].std()) > 0.01 and (o64[region] > rho[region]).sum() >= 8
        assert err <= 3 * e32 + 1e-7
        assert_bits(got, o32, name + ": the fp32 restatement, bit for bit")
        assert_bits(got[2], rho[2], "a cylinder wholly outside the grid")
        assert_bits(got[:, ~ref.interior_mask(shape, bnd)], rho[:, ~ref.interior_mask(shape, bnd)], "the band is copied through")
        _lib.call("df_density_noise_inflow%dd" % D, rin.ptr, rin.ptr, cin.ptr, ctypes.addressof(q), time, scale, sigma, *(dims + [bnd, stream]))
        assert_bits(rin.get("inflow in place"), got, "inflow in place")
        cin.check_guards()
        inflow = ops.NoiseInflow(shp, _noise_field(noise), scale=scale, sigma=sigma)
        assert_bits(_np(ops.density_inflow(dev(rho), inflow, time=time, bnd=bnd)), got, "ops.density_inflow")
        # a density already above the target comes back bit for bit
        high = (rho + np.float32(4.0)).astype(np.float32)
        assert_bits(_np(ops.density_inflow(dev(high), inflow, time=time, bnd=bnd)), high, "a density above the target")
        # source= of advect: the inflow, then the advection
        vel = ref.make_velocity(shape, B=B, seed=2, vmax=1.0)
        assert torch.equal(ops.advect(dev(rho), dev(vel), 0.5, bnd=bnd, source=inflow, time=time), ops.advect(dev(got), dev(vel), 0.5, bnd=bnd))
    bad = np.array(cyl); bad[0, D:2 * D] = 0.0; bad[1, 0] = np.nan                 # a zero-length axis, a NaN: nothing is stamped
    cin, rin, out = Guarded(bad.shape, bad), Guarded(rho.shape, rho), Guarded(rho.shape)
    _lib.call("df_density_noise_inflow%dd" % D, rin.ptr, out.ptr, cin.ptr, ctypes.addressof(q), 0.0, 1.0, 0.5, *(dims + [bnd, stream]))
    assert_bits(out.get("invalid entries")[:3], rho[:3], "invalid entries stamp nothing")


# ---- 3. the per-entry force ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,bnd", SHAPES)
def test_per_entry_force_bitwise(shape, bnd):
    from deep_fluids_amd import _lib, ops
    D = len(shape)
    names, obs = pref.all_obstacles(shape, bnd)
    B = len(names)
    dims = [B] + list(shape)
    stream = torch.cuda.current_stream().cuda_stream
    flags = ops.obstacle_flags(_obs(obs), bnd)
    rng = np.random.RandomState(11)
    vel = ref.make_velocity(shape, B=B, seed=2)
    rho = rng.uniform(0, 1, (B,) + shape).astype(np.float32)
    force = (0.013, 0.256, -0.07)[:D]
    same = np.tile(np.array(force, np.float32), (B, 1))
    rows = (rng.uniform(-0.3, 0.3, (B, D))).astype(np.float32)
    zero = np.zeros_like(obs)
    assert [s for s, _ in pref.specs(D)][0] == ""                                # open_sides = 0 is among the cases
    for spec, bits in pref.specs(D):
        for o, fl in ((obs, flags.data_ptr()), (zero, None)):
            vin, rin, out = Guarded(vel.shape, vel), Guarded(rho.shape, rho), Guarded(vel.shape)
            _lib.call("df_wall_buoyancy%dd_open" % D, vin.ptr, rin.ptr, out.ptr, fl, *(dims + list(force) + [bnd, bits, stream]))
            scalar = out.get("scalar %r" % spec)
            for f, want, what in ((same, scalar, "equal rows"), (rows, iref.wall_buoyancy_dev(vel, rho, rows, o, bits, bnd, np.float32), "distinct rows")):
                fin, out = Guarded(f.shape, f), Guarded(vel.shape)
                _lib.call("df_wall_buoyancy%dd_open_dev" % D, vin.ptr, rin.ptr, out.ptr, fl, fin.ptr, *(dims + [bnd, bits, stream]))
                assert_bits(out.get("%s %r" % (what, spec)), want, "%s %r flags %s" % (what, spec, fl is not None))
                fin.check_guards()
            vin.check_guards(); rin.check_guards()
            got = ops.wall_buoyancy(dev(vel), dev(rho), torch.from_numpy(rows), bnd=bnd, open_bound=spec, obstacle=None if fl is None else flags)
            assert_bits(_np(got), want, "ops.wall_buoyancy with a force tensor %r" % spec)
    assert not np.array_equal(want, scalar)


# ---- 4. untouched paths, and an entry alone ---------------------------------------------------------------------------------------------------------
def _scene(shape, B=3):
    """B entries of the smoke3_vel_buo kind on a grid ``shape``: a cylinder along y near the low-x side, a different inflow velocity and
    buoyancy per entry"""
    from deep_fluids_amd import ops
    D = len(shape)
    ext = shape[::-1]
    centre = [0.2 * ext[0], 0.3 * ext[1]] + [0.5 * n for n in ext[2:]]
    cyl = np.tile(np.array(centre + [0.0, 0.1 * ext[1]] + [0.0] * (D - 2) + [0.2 * ext[1]], np.float32), (B, 1))
    values = np.zeros((B, D), np.float32)
    values[:, 0] = np.linspace(1.0, 3.0, B)
    gravities = np.linspace(-2e-3, -10e-3, B)
    noise = iref.noise_params(seed=123)
    shp = ops.CylinderShape(cyl[:, :D], cyl[:, D:2 * D], cyl[:, 2 * D])
    inflow = ops.NoiseInflow(shp, _noise_field(noise), scale=1.0, sigma=0.5)
    return cyl, values, gravities, noise, shp, inflow


@pytest.mark.parametrize("shape,bnd,spec", [((12, 10), 1, "xXyY"), ((17, 130), 2, ""), ((7, 8, 6), 1, "XyY")])
def test_untouched_paths_are_bitwise_their_pieces(shape, bnd, spec):
    from deep_fluids_amd import ops
    D = len(shape)
    B, T, dt = 3, 3, 0.5
    force = (0.0, 0.256, 0.0)[:D]
    src = _obs(aref.sphere_mask_loop(shape, [0.5 * n for n in shape[::-1]], 1.5))
    d0 = dev(ref.make_density(shape, B=B, seed=1))
    v0 = dev(pref.solve_input(shape, bnd, np.zeros((B,) + shape, np.uint8), pref.sides(spec, D)))
    stats = []
    dT, vels = ops.simulate_smoke(d0, v0, T, dt=dt, source=src, force=force, bnd=bnd, stats=stats, open_bound=spec)
    d, v = d0, v0
    for t in range(T):
        dn = ops.advect(d, v, dt, bnd=bnd, source=src)
        vn = ops.advect_velocity(v, dt, bnd=bnd, open_bound=spec)
        vn = ops.wall_buoyancy(vn, dn, force, bnd=bnd, open_bound=spec)
        vn, _, it = ops.solve_pressure(vn, bnd=bnd, open_bound=spec)
        ds, vs = ops.smoke_step(d, v, dt, source=src, force=force, bnd=bnd, open_bound=spec)
        assert torch.equal(ds, dn) and torch.equal(vs, vn) and torch.equal(vels[t], vn) and torch.equal(stats[t], it)
        # the same force as a tensor: the `_dev` entry point, the same bits
        dq, vq = ops.smoke_step(d, v, dt, source=src, force=torch.tensor([force] * B), bnd=bnd, open_bound=spec)
        assert torch.equal(dq, dn) and torch.equal(vq, vn)
        d, v = dn, vn
    assert torch.equal(dT, d) and float(vels[-1].abs().max()) > 0


@pytest.mark.parametrize("shape,bnd,spec", [((17, 130), 1, "xXyY"), ((19, 10, 7), 1, "XyY")])
def test_an_entry_alone_is_that_entry_of_the_batch(shape, bnd, spec):
    from deep_fluids_amd import ops
    D = len(shape)
    B, T, dt = 3, 3, 0.5
    cyl, values, gravities, noise, shp, inflow = _scene(shape, B)
    forces = ops.buoyancy_forces(shape, dt, gravities)
    d0, v0 = torch.zeros((B,) + shape, device="cuda"), torch.zeros((B,) + shape + (D,), device="cuda")
    kw = dict(dt=dt, bnd=bnd, open_bound=spec)
    dT, vels = ops.simulate_smoke(d0, v0, T, source=inflow, force=forces, inflow_velocity=(shp, values), **kw)
    assert not v0.any() and not d0.any()                                       # the caller's fields are never written
    assert float(dT.max()) > 0.3 and float(vels[-1].abs().max()) > 0.05
    for e in range(B):
        d1, v1 = ops.simulate_smoke(d0[e:e + 1], v0[e:e + 1], T, source=inflow.entry(e), force=forces[e:e + 1],
                                    inflow_velocity=(shp.entry(e), values[e]), **kw)
        assert torch.equal(d1[0], dT[e]) and torch.equal(v1[:, 0], vels[:, e]), e
    # with D floats as the force of a single entry: the scalar entry point, the same bits
    f0 = ops.default_buoyancy_force(shape, dt, float(gravities[0]))
    d1, v1 = ops.simulate_smoke(d0[:1], v0[:1], T, source=inflow.entry(0), force=f0, inflow_velocity=(shp.entry(0), values[0]), **kw)
    assert torch.equal(d1[0], dT[0]) and torch.equal(v1[:, 0], vels[:, 0])
    assert not torch.equal(vels[-1, 0], vels[-1, 1]) and not torch.equal(vels[-1, 1], vels[-1, 2])


# ---- 5. a short scene ---------------------------------------------------------------------------------------------------------------------------------
def test_short_scene_against_the_fp64_restatement():
    """Six frames of three entries with different inflow and buoyancy on (12, 16, 20), sides 'XyY' open.  Every frame is checked from the
    GPU's own previous state, so the solver's tolerance does not accumulate into the comparison:
      - the fields before the projection (inflow, stamp, both advections and the fill, walls and buoyancy) by the twin rule,
        |gpu - fp64| <= 3 * e32 + 1e-7 with e32 the fp32 restatement's own error on that field (advect_ref.compare for the advections);
      - the projected field to the solve's accuracy: its distance from the fp64 restatement solved to 1e-10 from the same input is at
        most 3 times the distance of the fp32 restatement, which stops at the same criterion (the rule of
        test_solve_residual_and_projection), plus the fp32 rounding of the field, 1e-7;
      - every fluid cell's divergence is within accuracy * (2D + 1), the residual bound times the stencil's width."""
    from deep_fluids_amd import ops
    shape, spec, bnd, dt, acc, T, B = (12, 16, 20), "XyY", 1, 0.5, 1e-4, 6, 3
    D = 3
    bits = pref.sides(spec, D)
    cyl, values, gravities, noise, shp, inflow = _scene(shape, B)
    forces = ops.buoyancy_forces(shape, dt, gravities)
    fnp = forces.numpy()
    obs = np.zeros((B,) + shape, np.uint8)
    d0, v0 = torch.zeros((B,) + shape, device="cuda"), torch.zeros((B,) + shape + (D,), device="cuda")
    frames = [(d.clone(), v.clone()) for d, v in ops.simulate_smoke(d0, v0, T, dt=dt, source=inflow, force=forces, open_bound=spec,
                                                                   inflow_velocity=(shp, values), accuracy=acc, stack=False)]
    assert len(frames) == T and not v0.any() and not d0.any()                  # the caller's vel0 is unchanged
    tol = lambda e: 3 * e + 1e-7
    d, v = d0, v0
    for t in range(T):
        time = t * dt
        # the pieces on the GPU, in the script's order
        g_din = ops.density_inflow(d, inflow, time=time)
        g_vin = ops.stamp_velocity(v, shp, values)
        g_d = ops.advect(g_din, g_vin, dt)
        g_va = ops.advect_velocity(g_vin, dt, open_bound=spec)
        g_vw = ops.wall_buoyancy(g_va, g_d, forces, open_bound=spec)
        g_v, _, it = ops.solve_pressure(g_vw, accuracy=acc, open_bound=spec)
        ds, vs = ops.smoke_step(d, v, dt, source=inflow, force=forces, open_bound=spec, inflow_velocity=(shp, values), time=time, accuracy=acc)
        assert torch.equal(ds, g_d) and torch.equal(vs, g_v) and torch.equal(frames[t][0], g_d) and torch.equal(frames[t][1], g_v)
        dh, vh = _np(d), _np(v)
        p64, p32 = (iref.step(dh, vh, dt, cyl, noise, time, values, fnp, bits, accuracy=acc, dtype=dt_, parts=True)[2] for dt_ in (np.float64, np.float32))
        for key, got in (("d_in", g_din), ("v_in", g_vin), ("v_wall", g_vw)):
            e32 = float(np.abs(p32[key].astype(np.float64) - p64[key]).max())
            err = float(np.abs(_np(got) - p64[key]).max())
            print("frame %d %-7s e32 %.3e  gpu %.3e (bound %.3e)" % (t, key, e32, err, tol(e32)))
            if key != "v_wall":
                assert err <= tol(e32), (t, key)
        vin = p64["v_in"]
        e32d, out_d = aref.twin_error(p64["rd"], p32["rd"], bnd)
        err_d, share_d = aref.compare(_np(g_d), p64["rd"], e32d, bnd, oref.alternatives(p64["rd"], vin, dt, 2, bnd, obs))
        e32v, out_v = aref.twin_error(p64["rv"], p32["rv"], bnd)
        ga = _np(g_va)
        assert_bits(ga, pref.extrapolate(ga, bits, bnd), "the advected velocity is filled")
        hf = np.stack([pref.high_face_mask(shape, bnd, bits, a) for a in range(D)], axis=-1)
        raw = np.where(pref.open_mask(shape, bnd, bits)[None, ..., None] & ~hf[None], np.float32(0), ga)
        err_v, share_v = aref.compare(ref.vel_to_stacked(raw), p64["rv"], e32v, bnd, pref.mac_alternatives(p64["rv"], vin, dt, 2, bnd, obs))
        print("frame %d density e32 %.3e gpu %.3e left out %.5f %%;  velocity e32 %.3e gpu %.3e left out %.5f %%" %
              (t, e32d, err_d, 100 * share_d, e32v, err_v, 100 * share_v))
        # walls and buoyancy and the projection from the GPU's own advected fields (a flipped advection branch must not enter them)
        gah, gdh = _np(g_va), _np(g_d)
        w64, w32 = (iref.wall_buoyancy_dev(gah, gdh, fnp, obs, bits, bnd, dt_) for dt_ in (np.float64, np.float32))
        e32w = float(np.abs(w32.astype(np.float64) - w64).max())
        err_w = float(np.abs(_np(g_vw) - w64).max())
        gwh = _np(g_vw)
        vex, _, _ = pref.solve_pressure(gwh, obs, bits, bnd, 1e-10, 4000, np.float64)
        v32, _, it32 = pref.solve_pressure(gwh, obs, bits, bnd, acc, ops.default_max_iter(shape), np.float32)
        d32, dg = float(np.abs(v32 - vex).max()), float(np.abs(_np(g_v) - vex).max())
        div = float(np.abs(pref.divergence(_np(g_v), obs, bnd)).max())
        print("frame %d walls e32 %.3e gpu %.3e;  projection: iterations gpu %s twin %s  distance from the fp64 solve: twin %.3e gpu %.3e  max|div| %.3e" %
              (t, e32w, err_w, _np(it).tolist(), it32.tolist(), d32, dg, div))
        assert err_w <= tol(e32w)
        assert dg <= 3 * d32 + 1e-7
        assert div <= acc * (2 * D + 1)
        dn = _np(g_d)
        assert np.isfinite(dn).all() and dn.min() >= 0.0 and not dn[:, ~ref.interior_mask(shape, bnd)].any()      # resetOutflow
        d, v = g_d, g_v
    vT = _np(v)
    assert float(_np(d).max()) > 0.5 and np.abs(vT).max() > 0.05
    assert not np.array_equal(vT[0], vT[1]) and not np.array_equal(vT[1], vT[2]) and not np.array_equal(vT[0], vT[2])      # the entries end different


# ---- 6. the generator -----------------------------------------------------------------------------------------------------------------------------------
KEYS = ["log_dir", "num_param", "path_format", "p0", "p1", "p2", "min_inflow", "max_inflow", "num_inflow", "min_buoyancy", "max_buoyancy",
        "num_buoyancy", "src_x_pos", "src_y_pos", "src_z_pos", "src_radius", "src_height", "min_frames", "max_frames", "num_frames",
        "num_simulations", "resolution_x", "resolution_y", "resolution_z", "bWidth", "open_bound", "time_step", "adv_order", "clamp_mode"]


def test_generate_smoke3_vel_buo_dataset(tmp_path):
    from deep_fluids_amd import ops
    from deep_fluids_amd.data import BatchManager, generate_smoke3_vel_buo_dataset, smoke3_vel_buo_inflow
    from deep_fluids_amd.trainer import smoke3_vel_buo_source
    X, Y, Z, T = 16, 12, 8, 3
    root = str(tmp_path / "vel_buo")
    # src_height 0.08: at Y = 12 the script's 0.04 is a half height of 0.48 cells, which no x face (at j + .5) lies within -- the inflow
    # velocity would stamp nothing and the first parameter would not matter
    kw = dict(num_inflow=2, num_buoyancy=2, num_frames=T, resolution_x=X, resolution_y=Y, resolution_z=Z, min_buoyancy=-2e-3, max_buoyancy=-10e-3,
              src_height=0.08)
    assert generate_smoke3_vel_buo_dataset(root, **kw) == 2 * 2 * T
    assert sorted(os.listdir(root)) == ["args.txt", "v", "v_range.txt"]
    assert sorted(os.listdir(os.path.join(root, "v"))) == sorted("%d_%d_%d.npz" % (i, j, t) for i in range(2) for j in range(2) for t in range(T))
    args = dict(line.rstrip("\n").split(": ") for line in open(os.path.join(root, "args.txt")))
    assert list(args) == KEYS and args["open_bound"] == "XyY" and args["num_frames"] == str(T) and args["max_frames"] == str(T - 1)
    assert args["num_simulations"] == str(4 * T) and args["p0"] == "inflow" and args["src_height"] == "0.08"
    p1s, p2s = np.linspace(1, 5, 2), np.linspace(-2e-3, -10e-3, 2)
    lo, hi = np.inf, -np.inf
    last = {}
    for i in range(2):
        for j in range(2):
            for t in range(T):
                with np.load(os.path.join(root, "v", "%d_%d_%d.npz" % (i, j, t))) as f:
                    assert sorted(f.files) == ["x", "y"]
                    x, y = f["x"], f["y"]
                assert x.dtype == np.float32 and x.shape == (Z, Y, X, 3)
                np.testing.assert_array_equal(y, [p1s[i], p2s[j], t])
                lo, hi = min(lo, float(x.min())), max(hi, float(x.max()))
                last[i, j] = x
    assert open(os.path.join(root, "v_range.txt")).read() == "%.3f\n%.3f" % (lo, hi) and hi > 0.05
    assert not np.array_equal(last[0, 0], last[1, 0]) and not np.array_equal(last[0, 0], last[0, 1])           # both parameters matter
    # scene (1, 0) alone, through simulate_smoke: the stored frames bit for bit
    inflow = smoke3_vel_buo_inflow((X, Y, Z), src_height=0.08)
    d0, v0 = torch.zeros((1, Z, Y, X), device="cuda"), torch.zeros((1, Z, Y, X, 3), device="cuda")
    dT, vels = ops.simulate_smoke(d0, v0, T, dt=0.5, source=inflow, force=ops.buoyancy_forces((Z, Y, X), 0.5, [p2s[0]]), open_bound="XyY",
                                  inflow_velocity=(inflow.shape, [p1s[1], 0.0, 0.0]))
    for t in range(T):
        with np.load(os.path.join(root, "v", "1_0_%d.npz" % t)) as f:
            assert_bits(_np(vels[t, 0]), f["x"], "frame %d of scene (1, 0)" % t)
    # one scene per batch: the same files
    split = str(tmp_path / "split")
    generate_smoke3_vel_buo_dataset(split, scenes_per_batch=1, **kw)
    for name in ("0_1_2.npz", "1_1_1.npz"):
        with np.load(os.path.join(root, "v", name)) as f, np.load(os.path.join(split, "v", name)) as g:
            assert_bits(f["x"], g["x"], name)
    cfg = SimpleNamespace(random_seed=1, data_path=root, is_3d=True, data_type="velocity", arch="de", batch_size=3, res_x=X, res_y=Y, res_z=Z,
                          num_worker=1)
    bm = BatchManager(cfg, device=None)
    xb, yb = bm.batch()
    bm.stop_thread()
    assert tuple(xb.shape) == (3, Z, Y, X, 3) and tuple(yb.shape) == (3, 3) and bm.num_samples == 4 * T
    # the helper rebuilds the generator's inflow: the density carried through the stored frames is the simulation's, bit for bit
    src = smoke3_vel_buo_source(bm)
    assert isinstance(src, ops.NoiseInflow) and torch.equal(src.shape.packed, inflow.shape.packed) and src.time_step == 0.5
    seq = torch.cat([v0[None], vels[:-1]])
    stamped = torch.stack([ops.stamp_velocity(seq[t], inflow.shape, [p1s[1], 0.0, 0.0]) for t in range(T)])     # the density moves through the stamped field
    got = ops.advect_sequence(d0, stamped, 0.5, source=src)
    assert torch.equal(got, ops.advect_sequence(d0, stamped, 0.5, source=inflow)) and torch.equal(got, dT) and float(dT.max()) > 0.3


# ---- 7. error codes, with real buffers --------------------------------------------------------------------------------------------------------------
def test_error_codes_of_the_new_entry_points():
    from deep_fluids_amd import _lib, ops
    h = _lib.lib()
    v, r, o = torch.zeros((1, 8, 8, 2), device="cuda"), torch.zeros((1, 8, 8), device="cuda"), torch.full((1, 8, 8, 2), 7.0, device="cuda")
    o1 = torch.full((1, 8, 8), 7.0, device="cuda")
    c, u = torch.tensor([[4.0, 4.0, 0.0, 1.0, 2.0]], device="cuda"), torch.ones((1, 2), device="cuda")
    q = ops.NoiseField().params(2, 8)
    qa = ctypes.addressof(q)
    assert h.df_density_noise_inflow2d(r.data_ptr(), o1.data_ptr(), c.data_ptr(), None, 0.0, 1.0, 0.5, 1, 8, 8, 1, None) == -1 and b"null noise" in h.df_last_error()
    for sigma in (0.0, -1.0, float("nan")):
        assert h.df_density_noise_inflow2d(r.data_ptr(), o1.data_ptr(), c.data_ptr(), qa, 0.0, 1.0, sigma, 1, 8, 8, 1, None) == -1 and b"sigma" in h.df_last_error()
    assert h.df_density_noise_inflow2d(r.data_ptr(), o1.data_ptr(), c.data_ptr(), qa, 0.0, 1.0, 0.5, 1, 8, 0, 1, None) == -1
    assert h.df_density_noise_inflow2d(r.data_ptr(), o1.data_ptr(), o1.data_ptr() + 16, qa, 0.0, 1.0, 0.5, 1, 8, 8, 1, None) == -1 and b"overlap" in h.df_last_error()
    assert h.df_density_noise_inflow2d(r.data_ptr(), o1.data_ptr() + 2, c.data_ptr(), qa, 0.0, 1.0, 0.5, 1, 8, 8, 1, None) == -3
    assert h.df_mac_cylinder_stamp2d(v.data_ptr(), c.data_ptr(), None, o.data_ptr(), 1, 8, 8, None) == -1 and b"null values" in h.df_last_error()
    assert h.df_mac_cylinder_stamp2d(v.data_ptr(), c.data_ptr(), o.data_ptr() + 8, o.data_ptr(), 1, 8, 8, None) == -1 and b"values overlap" in h.df_last_error()
    assert h.df_mac_cylinder_stamp2d(v.data_ptr(), c.data_ptr(), u.data_ptr(), o.data_ptr(), 1 << 24, 8, 8, None) == -2
    assert h.df_wall_buoyancy2d_open_dev(v.data_ptr(), r.data_ptr(), o.data_ptr(), None, None, 1, 8, 8, 1, 0, None) == -1 and b"null forces" in h.df_last_error()
    assert h.df_wall_buoyancy2d_open_dev(v.data_ptr(), r.data_ptr(), o.data_ptr(), None, u.data_ptr(), 1, 8, 8, 1, 16, None) == -1 and b"z side" in h.df_last_error()
    assert h.df_wall_buoyancy2d_open_dev(v.data_ptr(), r.data_ptr(), o.data_ptr(), None, u.data_ptr(), 1, 8, 8, 0, 0, None) == -1
    assert h.df_wall_buoyancy2d_open_dev(v.data_ptr(), r.data_ptr(), o.data_ptr(), None, u.data_ptr(), 1, 8, 3, 1, 0, None) == -2
    torch.cuda.synchronize()
    assert bool((o == 7.0).all()) and bool((o1 == 7.0).all())                  # a refused call writes nothing
    with pytest.raises(ValueError):
        ops.density_inflow(r, ops.NoiseInflow(ops.CylinderShape([4.0, 4.0, 4.0], [0.0, 1.0, 0.0], 2.0), ops.NoiseField()))       # a 3-D cylinder, a 2-D grid
    with pytest.raises(ValueError):
        ops.stamp_velocity(v, ops.CylinderShape([[4.0, 4.0]] * 2, [0.0, 1.0], 2.0), [1.0, 0.0])                                 # two cylinders, one entry
    with pytest.raises(ValueError):
        ops.wall_buoyancy(v, r, torch.zeros((2, 2)))                                                                               # two forces, one entry
