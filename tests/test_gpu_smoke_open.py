"""GPU side of the smoke solver with open sides (the `_open` entry points of smoke.hip, df_open_extrapolate*, df_density_sphere_source*,
ops' ``open_bound=`` keyword and ``SphereSource``, the moving-source data sets): against the restatement of tests/smoke_open_ref.py --
a restatement of this project's own definition, not of mantaflow -- with tolerances measured from its fp32 twin in the same test.
Every parity test prints its figures before it asserts.

Shapes are smoke_ref.MAC_SHAPES, the open specs smoke_open_ref.SPECS ('', 'Y', 'xX', 'XyY', 'xXyY', 'xXyYzZ'; a 2-D grid drops the z
letters), the obstacles those of smoke_obs_ref plus a block against an open side and a closed chamber that reaches none."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import advect_ref as aref
import smoke_obs_ref as oref
import smoke_open_ref as pref
import smoke_ref as ref
from gpu_util import Guarded, assert_bits, dev

pytestmark = pytest.mark.gpu

SHAPES = [(s, b) for s, bnds in ref.MAC_SHAPES for b in bnds]
SOLVE_SHAPES = [((6, 6), 1), ((9, 7), 1), ((12, 10), 2), ((17, 130), 1), ((6, 6, 6), 1), ((7, 8, 6), 1), ((19, 10, 7), 2)]


def _np(t):
    return t.cpu().numpy()


def _obs(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _open_specs(dim):
    return [(s, b) for s, b in pref.specs(dim) if b]


# ---- 1. no open side: the bits of the closed calls -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,bnd", SHAPES)
def test_no_open_side_is_bitwise_the_closed_path(shape, bnd):
    from deep_fluids_amd import ops
    D = len(shape)
    B = 3
    vel = dev(ref.make_velocity(shape, B=B, seed=1, vmax=min(3.0, 0.4 * min(shape))))
    rho = dev(ref.make_density(shape, B=B, seed=1))
    force = (0.013, 0.256, -0.07)[:D]
    src = _obs(aref.sphere_mask_loop(shape, [0.5 * n for n in shape[::-1]], 1.5))
    d0, v0 = torch.zeros_like(rho), torch.zeros_like(vel)
    for obstacle in (None, ops.obstacle_flags(_obs(oref.mixed_batch(shape, bnd)), bnd)):
        kw = {} if obstacle is None else dict(obstacle=obstacle)
        for ob in ("", 0):
            for mode in (1, 2):
                assert torch.equal(ops.advect_velocity(vel, 1.0, clamp_mode=mode, bnd=bnd, open_bound=ob, **kw),
                                   ops.advect_velocity(vel, 1.0, clamp_mode=mode, bnd=bnd, **kw))
            assert torch.equal(ops.advect_velocity(vel, 1.0, order=1, bnd=bnd, open_bound=ob, **kw), ops.advect_velocity(vel, 1.0, order=1, bnd=bnd, **kw))
            w = ops.wall_buoyancy(vel, rho, force, bnd=bnd, **kw)
            assert torch.equal(ops.wall_buoyancy(vel, rho, force, bnd=bnd, open_bound=ob, **kw), w)
            for skw in (dict(), dict(accuracy=0.0, max_iter=3)):
                got, want = ops.solve_pressure(w, bnd=bnd, open_bound=ob, **skw, **kw), ops.solve_pressure(w, bnd=bnd, **skw, **kw)
                for g, t in zip(got, want):
                    assert torch.equal(g, t)
            s1, s2 = [], []
            dm, vm = ops.simulate_smoke(d0, v0, 8, source=src, bnd=bnd, stats=s1, open_bound=ob, **kw)
            du, vu = ops.simulate_smoke(d0, v0, 8, source=src, bnd=bnd, stats=s2, **kw)
            assert torch.equal(dm, du) and torch.equal(vm, vu) and all(torch.equal(a, b) for a, b in zip(s1, s2))
            assert float(vu.abs().max()) > 0


def _abi_open(name, D, arrays, flags, dims, mid, osd, tail=()):
    """call an `_open` entry point: arrays, flags (may be None), dims, the scalars before open_sides, open_sides, the rest, the stream"""
    from deep_fluids_amd import _lib
    stream = torch.cuda.current_stream().cuda_stream
    _lib.call("%s%dd_open" % (name, D), *(list(arrays) + [flags] + list(dims) + list(mid) + [osd] + list(tail) + [stream]))


# ---- 2. wall_buoyancy, the fill and the stamp: bitwise against the fp32 restatement, through the C ABI into guarded buffers ---------------------
@pytest.mark.parametrize("shape,bnd", SHAPES)
def test_wall_buoyancy_fill_and_stamp_bitwise(shape, bnd):
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
    zero = np.zeros_like(obs)
    for spec, bits in pref.specs(D):
        for o, fl in ((obs, flags.data_ptr()), (zero, None)):
            want = pref.wall_buoyancy(vel, rho, force, o, bits, bnd, np.float32)
            vin, rin, out = Guarded(vel.shape, vel), Guarded(rho.shape, rho), Guarded(vel.shape)
            _abi_open("df_wall_buoyancy", D, [vin.ptr, rin.ptr, out.ptr], fl, dims, list(force) + [bnd], bits)
            assert_bits(out.get("wall_buoyancy %r" % spec), want, "wall_buoyancy %r" % spec)
            vin.check_guards(); rin.check_guards()
            assert_bits(_np(ops.wall_buoyancy(dev(vel), dev(rho), force, bnd=bnd, open_bound=spec, obstacle=None if fl is None else flags)), want,
                        "ops.wall_buoyancy %r" % spec)
        v = dev(vel)
        assert ops.wall_buoyancy(v, dev(rho), force, bnd=bnd, out=v, obstacle=flags, open_bound=spec) is v            # in place stays legal
        assert_bits(_np(v), pref.wall_buoyancy(vel, rho, force, obs, bits, bnd, np.float32), "in place %r" % spec)
        # the fill, in place
        buf = Guarded(vel.shape, vel)
        _lib.call("df_open_extrapolate%dd" % D, buf.ptr, *(dims + [bnd, bits, stream]))
        assert_bits(buf.get("fill %r" % spec), pref.extrapolate(vel, bits, bnd), "fill %r" % spec)
    # the stamp: centres and radii are multiples of 1/8, so fp32 is exact and the result is also sphere_mask + df_density_source
    ext = shape[::-1]
    centers = np.array([[(0.25 + 0.125 * e) * ext[a] // 0.125 * 0.125 for a in range(D)] for e in range(B)], np.float32)
    centers[B - 1] = np.nan                                         # a NaN centre stamps nothing
    centers[B - 2, 0] = -3.0                                        # a sphere that is partly outside the grid
    radius = 2.375
    want = pref.sphere_source(rho, centers, radius, 0.75, np.float32)
    assert_bits(want, pref.sphere_source(rho, centers, radius, 0.75, np.float64).astype(np.float32), "the restatement is exact here")
    cin, rin, out = Guarded(centers.shape, centers), Guarded(rho.shape, rho), Guarded(rho.shape)
    _lib.call("df_density_sphere_source%dd" % D, rin.ptr, cin.ptr, radius, 0.75, out.ptr, *(dims + [stream]))
    assert_bits(out.get("stamp"), want, "stamp")
    assert_bits(want[B - 1], rho[B - 1], "NaN centre")
    assert (want[0] == 0.75).sum() > 0
    _lib.call("df_density_sphere_source%dd" % D, rin.ptr, cin.ptr, radius, 0.75, rin.ptr, *(dims + [stream]))                # out == density
    assert_bits(rin.get("stamp in place"), want, "stamp in place")
    cin.check_guards()
    for e in range(B - 1):
        m = ops.sphere_mask(shape, [float(c) for c in centers[e]], radius, "cuda")
        o1 = torch.empty((1,) + shape, device="cuda")
        r1 = dev(rho[e:e + 1])
        _lib.call("df_density_source", r1.data_ptr(), m.data_ptr(), 0.75, o1.data_ptr(), m.numel(), stream)
        assert_bits(_np(o1)[0], want[e], "sphere_mask + df_density_source, entry %d" % e)


# ---- 3. MAC advection parity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,bnd", SHAPES)
def test_mac_advection_parity_with_the_fp64_restatement(shape, bnd):
    from deep_fluids_amd import ops
    D = len(shape)
    obs = pref.mixed_batch(shape, bnd)
    o = _obs(obs)
    vel = ref.make_velocity(shape, seed=0, vmax=min(3.0, 0.4 * min(shape)))
    n = 0
    for spec, bits in _open_specs(D):
        for order, mode in ((1, 2), (2, 1), (2, 2)):
            kw = dict(order=order, clamp_mode=mode, bnd=bnd)
            r64 = pref.mac_advect(vel, 1.0, obs, bits, dtype=np.float64, **kw)
            r32 = pref.mac_advect(vel, 1.0, obs, bits, dtype=np.float32, **kw)
            alt = pref.mac_alternatives(r64, vel, 1.0, mode, bnd, obs)
            run = lambda sl: ops.advect_velocity(dev(vel[sl]), 1.0, obstacle=o[sl], open_bound=spec, **kw)
            got = _np(run(slice(None)))
            opn = pref.open_mask(shape, bnd, bits)
            # what the op returns is filled; the record is not: compare the record where it is defined, the fill on its own
            assert_bits(got, pref.extrapolate(got, bits, bnd), "%r: the result is filled" % spec)
            hf = np.stack([pref.high_face_mask(shape, bnd, bits, a) for a in range(D)], axis=-1)
            raw = np.where(opn[None, ..., None] & ~hf[None], np.float32(0), got)       # open cells: only the high-face component is advected
            gs = ref.vel_to_stacked(raw)
            e32, twin_out = aref.twin_error(r64, r32, bnd)
            name = "%s-%r-o%d-m%d-b%d" % ("x".join(map(str, shape)), spec, order, mode, bnd)
            print("%-30s e32 %.3e  gpu max %.3e  twin left out %.5f %%  gpu == twin bitwise: %s" %
                  (name, e32, float(np.abs(gs - r64["out"]).max()), 100 * twin_out, bool(np.array_equal(gs, r32["out"]))))
            err, share = aref.compare(gs, r64, e32, bnd, alt)
            print("%-30s gpu %.3e (bound %.3e)  left out %.5f %%" % ("", err, 3 * e32 + 1e-7, 100 * share))
            if (order, mode) == (2, 2):
                for e in range(obs.shape[0]):                   # an entry alone is that entry of the batch, bit for bit
                    assert_bits(_np(run(slice(e, e + 1))), got[e:e + 1], name + " entry %d alone" % e)
            n += 1
    assert n == 3 * (4 if D == 2 else 5)


# ---- 4. conjugate gradients ------------------------------------------------------------------------------------------------------------------------
def _check_contract(obs, bnd, bits, v, p):
    fluid = oref.fluid_mask(obs, bnd)
    opn = pref._opn(obs, bnd, bits)
    assert np.isfinite(p).all() and np.isfinite(v).all()
    assert not p[~fluid].any()                                          # p is 0 outside the fluid
    for a in range(obs.ndim - 1):
        assert not v[..., a][~pref.live_mask(fluid, opn, a) & ~opn].any()   # non-live faces of fluid, solid and wall cells are exactly 0
    assert_bits(v, pref.extrapolate(v, bits, bnd), "the result is filled")


@pytest.mark.parametrize("shape,bnd", SOLVE_SHAPES)
def test_k_iterations_against_the_fp64_recurrence(shape, bnd):
    from deep_fluids_amd import ops
    names, obs = pref.all_obstacles(shape, bnd)
    live = np.array([n != "solid" for n in names])
    flags = ops.obstacle_flags(_obs(obs), bnd)
    for spec, bits in _open_specs(len(shape)):
        w = pref.solve_input(shape, bnd, obs, bits)
        for k in (1, 2, 3, 4):
            x64, it64, _ = pref.cg(w, obs, bits, bnd, 0.0, k, np.float64)
            x32, _, _ = pref.cg(w, obs, bits, bnd, 0.0, k, np.float32)
            e32 = float(np.abs(x32 - x64).max())
            v, p, iters = ops.solve_pressure(dev(w), bnd=bnd, accuracy=0.0, max_iter=k, obstacle=flags, open_bound=spec)
            err = float(np.abs(_np(p) - x64).max())
            print("%s bnd %d %r k %d: e32 %.3e  gpu %.3e (bound %.3e)  |x| %.3e" % (shape, bnd, spec, k, e32, err, 3 * e32 + 1e-7, float(np.abs(x64).max())))
            assert (_np(iters)[live] == k).all() and (it64[live] == k).all()
            assert err <= 3 * e32 + 1e-7
            _check_contract(obs, bnd, bits, _np(v), _np(p))


@pytest.mark.parametrize("shape,bnd", SOLVE_SHAPES)
def test_solve_residual_and_projection(shape, bnd):
    from deep_fluids_amd import ops
    names, obs = pref.all_obstacles(shape, bnd)
    live = np.array([n != "solid" for n in names])
    acc = 1e-4
    max_iter = ops.default_max_iter(shape)
    for spec, bits in _open_specs(len(shape)):
        for inflow in (0.0, 0.5):                              # 0.5: a net inflow through the open sides, b does not sum to zero
            w = pref.solve_input(shape, bnd, obs, bits, inflow=inflow)
            b64 = pref.rhs(w, obs, bnd, np.float64)
            v, p, iters = ops.solve_pressure(dev(w), bnd=bnd, accuracy=acc, obstacle=_obs(obs), open_bound=spec)
            x32, it32, r32 = pref.cg(w, obs, bits, bnd, acc, max_iter, np.float32)
            # the twin's own excess (see test_gpu_smoke.py): |b - A p| <= |r| + drift, the drift measured on the twin in fp64
            excess = float(np.abs((b64 - pref.apply_A(x32.astype(np.float64), obs, bits, bnd)) - r32).max())
            res = float(np.abs(b64 - pref.apply_A(_np(p).astype(np.float64), obs, bits, bnd)).max())
            print("%s bnd %d %r inflow %.1f: sum b %.3f  iterations gpu %s twin %s  fp64 residual of the gpu's p %.4e (bound %.1e + twin's excess %.3e)" %
                  (shape, bnd, spec, inflow, float(b64[0].sum()), _np(iters).tolist(), it32.tolist(), res, acc, excess))
            assert (_np(iters)[live] > 0).all() and (_np(iters) < max_iter).all()        # converged, the net-inflow case too
            assert res <= acc + excess
            if inflow == 0.0 and int(oref.fluid_mask(obs, bnd).sum(axis=tuple(range(1, obs.ndim))).max()) <= 1200:
                vex, _ = pref.exact_projection(w, obs, bits, bnd)
                v32 = pref.extrapolate(pref.correct(w, x32, obs, bits, bnd, np.float32), bits, bnd)
                d32 = float(np.abs(v32 - vex).max())
                dg = float(np.abs(_np(v) - vex).max())
                print("%s bnd %d %r: distance from the exact fp64 projection: twin %.3e  gpu %.3e" % (shape, bnd, spec, d32, dg))
                assert dg <= 3 * d32
            _check_contract(obs, bnd, bits, _np(v), _np(p))


# ---- 5. batch invariance, determinism, check_every ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,bnd,spec", [((12, 10), 1, "XyY"), ((17, 130), 1, "xXyY"), ((19, 10, 7), 1, "xXyYzZ")])
def test_batch_invariance_determinism_and_check_every(shape, bnd, spec):
    from deep_fluids_amd import ops
    names, obs = pref.all_obstacles(shape, bnd)
    bits = pref.sides(spec, len(shape))
    w = pref.solve_input(shape, bnd, obs, bits)
    o = _obs(obs)
    flags = ops.obstacle_flags(o, bnd)
    v, p, iters = ops.solve_pressure(dev(w), bnd=bnd, obstacle=flags, open_bound=spec)
    it = _np(iters).tolist()
    print("%s %r: obstacles %s iterations %s" % (shape, spec, names, it))
    _check_contract(obs, bnd, bits, _np(v), _np(p))
    for e in range(len(names)):
        ve, pe, ie = ops.solve_pressure(dev(w[e:e + 1]), bnd=bnd, obstacle=o[e:e + 1], open_bound=bits)
        assert_bits(_np(pe)[0], _np(p)[e], "pressure of entry %d alone" % e)
        assert_bits(_np(ve)[0], _np(v)[e], "velocity of entry %d alone" % e)
        assert int(ie[0]) == it[e]
    ws = ops.pressure_workspace(dev(w))
    ws.fill_(float("nan"))                                 # nothing is read before it is written
    for ce in (None, 1, 16, 64):
        v2, p2, i2 = ops.solve_pressure(dev(w), bnd=bnd, check_every=ce, workspace=ws, obstacle=flags, open_bound=spec)
        assert_bits(_np(p2), _np(p), "check_every %s" % ce)
        assert_bits(_np(v2), _np(v), "check_every %s" % ce)
        assert torch.equal(i2, iters)
    vi = dev(w)
    assert ops.solve_pressure(vi, bnd=bnd, out=vi, obstacle=flags, open_bound=spec)[0] is vi and torch.equal(vi, v)            # in place
    a1 = ops.advect_velocity(dev(w), 1.0, bnd=bnd, obstacle=flags, open_bound=spec)
    assert torch.equal(a1, ops.advect_velocity(dev(w), 1.0, bnd=bnd, obstacle=flags, open_bound=spec))                       # run to run


# ---- 6. the step ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,spec", [((32, 24), "xXyY"), ((12, 16, 12), "xXyYzZ")])
def test_step_equals_its_parts_and_eight_steps_from_rest(shape, spec):
    from deep_fluids_amd import ops
    D = len(shape)
    ext = shape[::-1]
    B, T = 2, 8
    bits = pref.sides(spec, D)
    # a moving source near the open x- side (entry 0) and near the open y- side (entry 1)
    centers = np.zeros((T, B, D), np.float32)
    for t in range(T):
        centers[t, 0] = [2.5 + 0.25 * t] + [0.5 * n for n in ext[1:]]
        centers[t, 1] = [0.5 * ext[0] + 0.5 * t, 2.0] + [0.5 * n for n in ext[2:]]
    src = ops.SphereSource(centers, 0.12 * ext[0])
    obs = np.zeros((B,) + shape, np.uint8)
    dt, acc = 0.5, 1e-4
    force = ops.default_buoyancy_force(shape, dt)
    stats = []
    d0, v0 = torch.zeros((B,) + shape, device="cuda"), torch.zeros((B,) + shape + (D,), device="cuda")
    dT, vels = ops.simulate_smoke(d0, v0, T, dt=dt, source=src, stats=stats, open_bound=spec)
    d, v = d0, v0
    fluid = oref.fluid_mask(obs, 1)
    for t in range(T):
        st = ops.SphereSource(torch.from_numpy(centers[t]).cuda(), src.radius)
        dn = ops.advect(d, v, dt, source=st)
        vn = ops.advect_velocity(v, dt, open_bound=spec)
        vn = ops.wall_buoyancy(vn, dn, force, open_bound=spec)
        vn, _, it = ops.solve_pressure(vn, open_bound=spec)
        ds, vs = ops.smoke_step(d, v, dt, source=st, open_bound=bits)
        assert torch.equal(ds, dn) and torch.equal(vs, vn)                       # bitwise
        assert torch.equal(vels[t], vn) and torch.equal(stats[t], it)
        d, v = dn, vn
        vh, dh = _np(v), _np(d)
        div = float(np.abs(pref.divergence(vh, obs, 1)).max())
        print("%s %r step %d: iterations %s  max|div| in fluid %.3e  density [%.4f, %.4f]  max|v| %.4f" %
              (shape, spec, t + 1, _np(it).tolist(), div, float(dh.min()), float(dh.max()), float(np.abs(vh).max())))
        assert div <= acc * (2 * D + 1)                  # |div| = |b - A p| up to rounding: the residual bound times the stencil's width
        assert np.isfinite(dh).all() and dh.min() >= 0.0 and dh.max() <= 1.0
        assert not dh[:, ~ref.interior_mask(shape, 1)].any()                     # the band of the density is 0: resetOutflow
    assert torch.equal(dT, d)
    assert float(vels[-1].abs().max()) > 0.01
    # the same eight frames through advect_sequence with the [T,B,D] source: the density of the simulation, bit for bit
    assert torch.equal(ops.advect_sequence(d0, torch.cat([v0[None], vels[:-1]]), dt, source=src), dT)
    # one step of the restatement from rest: the density is exact (nothing moves yet); the velocity is printed, the solve's accuracy and
    # not rounding sets its distance
    d64, v64 = pref.step(np.zeros((B,) + shape), np.zeros((B,) + shape + (D,)), dt, obs, bits, source=(centers[0], src.radius), accuracy=1e-9)
    assert_bits(_np(ops.smoke_step(d0, v0, dt, source=src.frame(0), open_bound=spec)[0]), d64, "density after one step from rest")
    print("%s %r: step 1 against the fp64 restatement solved to 1e-9: %.3e" % (shape, spec, float(np.abs(_np(vels[0]) - v64).max())))


# ---- 7. the data sets --------------------------------------------------------------------------------------------------------------------------------
ROT_KEYS = ["log_dir", "num_param", "path_format", "p0", "min_src_pos", "max_src_pos", "src_y_pos", "src_radius", "circle_radius", "circle_period",
            "min_frames", "max_frames", "num_frames", "num_simulations", "num_dof", "resolution_x", "resolution_y", "resolution_z", "buoyancy",
            "bWidth", "open_bound", "time_step", "adv_order", "clamp_mode"]
MOV_KEYS = ["log_dir", "num_param", "path_format", "p0", "p1", "min_src_pos", "max_src_pos", "src_y_pos", "src_radius", "min_scenes", "max_scenes",
            "num_scenes", "min_frames", "max_frames", "num_frames", "num_simulations", "num_dof", "resolution_x", "resolution_y", "resolution_z",
            "buoyancy", "bWidth", "open_bound", "time_step", "adv_order", "clamp_mode", "nscale", "nrepeat", "nseed"]


def _check_moving_set(root, S, T, shape, keys, name, positions):
    from deep_fluids_amd.data import BatchManager
    Z, Y, X = shape
    assert sorted(os.listdir(root)) == ["args.txt", "n.npz", "v", "v_range.txt"]
    assert sorted(os.listdir(os.path.join(root, "v"))) == sorted(name(i, t) for i in range(S) for t in range(T))
    args = dict(line.rstrip("\n").split(": ") for line in open(os.path.join(root, "args.txt")))
    assert list(args) == keys and args["open_bound"] == "xXyYzZ" and args["num_frames"] == str(T) and args["max_frames"] == str(T - 1)
    assert args["num_dof"] == "2" and args["num_simulations"] == str(S * T)
    lo, hi = np.inf, -np.inf
    for i in range(S):
        for t in range(T):
            with np.load(os.path.join(root, "v", name(i, t))) as f:
                assert sorted(f.files) == ["x", "y"]
                x, y = f["x"], f["y"]
            assert x.dtype == np.float32 and x.shape == (Z, Y, X, 3) and y.shape == (2, T)
            want = np.full((2, T), -1.0)
            want[:, T - 1 - t:] = positions[i, :t + 1].T                # the window of the last T positions, padded in front with -1
            np.testing.assert_array_equal(y, want)
            lo, hi = min(lo, float(x.min())), max(hi, float(x.max()))
    assert open(os.path.join(root, "v_range.txt")).read() == "%.3f\n%.3f" % (lo, hi) and hi > 0.001
    with np.load(os.path.join(root, "n.npz")) as f:
        np.testing.assert_array_equal(f["nx"], positions[..., 0]); np.testing.assert_array_equal(f["nz"], positions[..., 1])
    cfg = SimpleNamespace(random_seed=1, data_path=root, is_3d=True, data_type="velocity", arch="ae", batch_size=3, res_x=X, res_y=Y, res_z=Z,
                          num_worker=1)
    bm = BatchManager(cfg, device=None)
    xb, yb = bm.batch()
    bm.stop_thread()
    assert tuple(xb.shape) == (3, Z, Y, X, 3) and tuple(yb.shape) == (3, 2, T) and bm.num_samples == S * T
    return bm


def test_generate_moving_source_datasets(tmp_path):
    from deep_fluids_amd import ops
    from deep_fluids_amd.data import generate_smoke3_mov_dataset, generate_smoke3_rot_dataset, smooth_source_paths
    from deep_fluids_amd.trainer import moving_source
    X, Y, Z, T, S = 12, 16, 12, 3, 2
    res = dict(resolution_x=X, resolution_y=Y, resolution_z=Z)
    root = str(tmp_path / "rot")
    assert generate_smoke3_rot_dataset(root, num_frames=T, circle_period=8, **res) == T
    t = np.arange(T)
    pos = np.stack([0.5 + 0.25 * np.cos(t * 2 * np.pi / 8), 0.5 + 0.25 * np.sin(t * 2 * np.pi / 8)], axis=-1)[None]
    bm = _check_moving_set(root, 1, T, (Z, Y, X), ROT_KEYS, lambda i, t: "%d.npz" % t, pos)
    src = moving_source(bm)
    assert isinstance(src, ops.SphereSource) and tuple(src.centers.shape) == (T, 1, 3) and src.radius == X * 0.08
    np.testing.assert_allclose(_np(src.centers)[:, 0], np.stack([X * pos[0, :, 0], np.full(T, Y * 0.1), Z * pos[0, :, 1]], axis=-1), rtol=1e-6)
    # re-simulated with the source the helper returns: the stored frames bit for bit; and advect_sequence takes it
    d0, v0 = torch.zeros((1, Z, Y, X), device="cuda"), torch.zeros((1, Z, Y, X, 3), device="cuda")
    dT, vels = ops.simulate_smoke(d0, v0, T, dt=0.5, source=src, force=ops.default_buoyancy_force((Z, Y, X), 0.5), open_bound="xXyYzZ")
    for k in range(T):
        with np.load(os.path.join(root, "v", "%d.npz" % k)) as f:
            assert_bits(_np(vels[k, 0]), f["x"], "frame %d" % k)
    assert torch.equal(ops.advect_sequence(d0, torch.cat([v0[None], vels[:-1]]), 0.5, source=src), dT) and float(dT.max()) > 0.5

    root = str(tmp_path / "mov")
    assert generate_smoke3_mov_dataset(root, num_scenes=S, num_frames=T, scenes_per_batch=1, **res) == S * T
    pos = smooth_source_paths(S, T, 0.1, 0.9, seed=123)
    assert pos.min() >= 0.1 and pos.max() <= 0.9 and not np.array_equal(pos[0], pos[1])
    bm = _check_moving_set(root, S, T, (Z, Y, X), MOV_KEYS, lambda i, t: "%d_%d.npz" % (i, t), pos)
    src = moving_source(bm, scene=1)
    np.testing.assert_allclose(_np(src.centers)[:, 0, 0], X * pos[1, :, 0], rtol=1e-6)
    both = str(tmp_path / "mov2")                              # the two scenes in one batch: the same files (an entry does not depend on its batch)
    given = np.stack([pos[0], np.full((T, 2), 0.5)])           # explicit paths
    generate_smoke3_mov_dataset(both, num_scenes=S, num_frames=T, positions=given, **res)
    for k in range(T):
        with np.load(os.path.join(root, "v", "0_%d.npz" % k)) as f, np.load(os.path.join(both, "v", "0_%d.npz" % k)) as g:
            assert_bits(f["x"], g["x"], "scene 0 frame %d" % k)
            np.testing.assert_array_equal(f["y"], g["y"])
    with pytest.raises(ValueError):
        generate_smoke3_mov_dataset(str(tmp_path / "bad"), num_scenes=S, num_frames=T, positions=given[:1], **res)


def test_existing_generators_honour_open_bound(tmp_path):
    from deep_fluids_amd import ops
    from deep_fluids_amd.data import BatchManager, generate_smoke3_obs_dataset, generate_smoke_dataset
    X, Y, T = 24, 32, 4
    root, closed = str(tmp_path / "open2d"), str(tmp_path / "closed2d")
    kw = dict(num_src_x_pos=2, num_src_radius=2, num_frames=T, resolution_x=X, resolution_y=Y)
    assert generate_smoke_dataset(root, open_bound="xXyY", **kw) == 2 * 2 * T          # the sides the script's open_bound opens
    generate_smoke_dataset(closed, **kw)
    args = dict(line.rstrip("\n").split(": ") for line in open(os.path.join(root, "args.txt")))
    assert args["open_bound"] == "xXyY" and sorted(os.listdir(os.path.join(root, "v"))) == sorted(os.listdir(os.path.join(closed, "v")))
    # scene (1, 1) re-simulated with those sides
    mask = ops.sphere_mask((Y, X), (X * 0.8, Y * 0.1), X * 0.12).cuda()
    d0, v0 = torch.zeros((1, Y, X), device="cuda"), torch.zeros((1, Y, X, 2), device="cuda")
    _, vels = ops.simulate_smoke(d0, v0, T, dt=0.5, source=mask, force=ops.default_buoyancy_force((Y, X), 0.5), open_bound="xXyY")
    differs = False
    for k in range(T):
        with np.load(os.path.join(root, "v", "1_1_%d.npz" % k)) as f, np.load(os.path.join(closed, "v", "1_1_%d.npz" % k)) as g:
            assert_bits(_np(vels[k, 0]), f["x"], "frame %d of scene (1, 1)" % k)
            differs = differs or not np.array_equal(f["x"], g["x"])
            np.testing.assert_array_equal(f["y"], g["y"])
    assert differs                                             # the open sides change the flow
    cfg = SimpleNamespace(random_seed=1, data_path=root, is_3d=False, data_type="velocity", arch="de", batch_size=3, res_x=X, res_y=Y, res_z=1,
                          num_worker=1)
    bm = BatchManager(cfg, device=None)
    xb, _ = bm.batch()
    bm.stop_thread()
    assert tuple(xb.shape) == (3, Y, X, 2)
    root3 = str(tmp_path / "open3d")
    assert generate_smoke3_obs_dataset(root3, open_bound="xXyYzZ", num_obs_x_pos=2, num_buoyancy=1, num_frames=2, resolution_x=12, resolution_y=16,
                                       resolution_z=12) == 2 * 1 * 2
    with np.load(os.path.join(root3, "v", "1_0_1.npz")) as f:
        assert np.isfinite(f["x"]).all() and np.abs(f["x"]).max() > 0


# ---- 8. error codes, with real buffers -----------------------------------------------------------------------------------------------------------
def test_error_codes_of_the_new_entry_points():
    from deep_fluids_amd import _lib, ops
    h = _lib.lib()
    shape = (8, 8)
    v, r, o = torch.zeros((1,) + shape + (2,), device="cuda"), torch.zeros((1,) + shape, device="cuda"), torch.full((1,) + shape + (2,), 7.0, device="cuda")
    c = torch.zeros((1, 2), device="cuda")
    ws = ops.pressure_workspace(v)
    for bad, word in ((64, b"open_sides"), (-1, b"open_sides"), (16, b"z side")):
        assert h.df_mac_advect_sl2d_open(v.data_ptr(), o.data_ptr(), 1, 8, 8, 1.0, 1, bad, None) == -1 and word in h.df_last_error()
        assert h.df_mac_advect_mc2d_open(v.data_ptr(), v.data_ptr(), o.data_ptr(), None, 1, 8, 8, 1.0, 1, bad, 2, None) == -1 and word in h.df_last_error()
        assert h.df_wall_buoyancy2d_open(v.data_ptr(), r.data_ptr(), o.data_ptr(), None, 1, 8, 8, 0.0, 0.1, 1, bad, None) == -1 and word in h.df_last_error()
        assert h.df_pressure_cg_direction2d_open(ws.data_ptr(), ws.numel() * 4, None, 1, 8, 8, 1, bad, 0, 1e-4, 10, None) == -1 and word in h.df_last_error()
        assert h.df_pressure_correct2d_open(v.data_ptr(), r.data_ptr(), o.data_ptr(), None, 1, 8, 8, 1, bad, None) == -1 and word in h.df_last_error()
        assert h.df_open_extrapolate2d(o.data_ptr(), 1, 8, 8, 1, bad, None) == -1 and word in h.df_last_error()
    assert h.df_density_sphere_source2d(r.data_ptr(), r.data_ptr() + 8, 2.0, 1.0, r.data_ptr(), 1, 8, 8, None) == -1 and b"centres overlap" in h.df_last_error()
    assert h.df_density_sphere_source2d(r.data_ptr(), c.data_ptr(), 2.0, 1.0, None, 1, 8, 8, None) == -1
    assert h.df_open_extrapolate2d(o.data_ptr(), 1, 8, 8, 1, 0, None) == 0
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())                              # a refused call, and the fill with no open side, write nothing
    with pytest.raises(ValueError):
        ops.advect_velocity(v, 1.0, open_bound="xXyYzZ")
    with pytest.raises(ValueError):
        ops.simulate_smoke(r, v, 3, source=ops.SphereSource(torch.zeros((2, 1, 2)), 1.0))      # two frames of centres for three steps
    with pytest.raises(ValueError):
        ops.advect(r, v, 0.5, source=ops.SphereSource(torch.zeros((2, 2)), 1.0))                # centres of another batch size
