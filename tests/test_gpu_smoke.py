"""GPU side of the smoke solver step (smoke.hip): MAC self-advection, walls and buoyancy, the conjugate-gradient pressure projection,
the chained step and the dataset generator, against the fp64 restatement of tests/smoke_ref.py with tolerances measured from its fp32
twin in the same test.  Every parity test prints its figures before it asserts.

Shapes are the smallest that can go wrong: (6,6) is 2*bnd + 4, (17,130) has X % 4 != 0 and nine workgroups per entry of which the last
is ragged, (19,10,7) is odd on every axis; B = 3 puts several entries into one launch."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import advect_ref as aref
import smoke_ref as ref
from gpu_util import assert_bits, dev

pytestmark = pytest.mark.gpu

SHAPES = [(s, b) for s, bnds in ref.MAC_SHAPES for b in bnds]
SOLVE_SHAPES = [((6, 6), 1), ((9, 7), 1), ((12, 10), 2), ((17, 130), 1), ((6, 6, 6), 1), ((7, 8, 6), 1), ((19, 10, 7), 2)]


def _np(t):
    return t.cpu().numpy()


# ---- MAC advection ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,bnd", SHAPES)
@pytest.mark.parametrize("B", [1, 3])
def test_mac_zero_velocity_and_integer_shift_bitwise(shape, bnd, B):
    from deep_fluids_amd import ops
    D = len(shape)
    inter = ref.interior_mask(shape, bnd)
    # a velocity that is zero carries nothing: dt * 0 = 0, every interior value comes back, the wall band is 0.  Advecting a field
    # through ITSELF leaves no freedom for "zero velocity, non-zero payload", so the payload is scaled by dt = 0.
    v = ref.make_velocity(shape, B=B, seed=7)
    want = np.where(inter[None, ..., None], v, 0).astype(np.float32)
    for order, mode in ((1, 2), (2, 1), (2, 2)):
        assert_bits(_np(ops.advect_velocity(dev(v), 0.0, order=order, clamp_mode=mode, bnd=bnd)), want, "dt = 0")
    z = np.zeros_like(v)
    assert_bits(_np(ops.advect_velocity(dev(z), 0.5, bnd=bnd)), z, "zero field")
    # a uniform integer shift: u = (2, -2[, 2]) everywhere, dt = 0.5 -> every face value is read one cell up-wind, where it is the
    # same number: the interior keeps it exactly, and MacCormack has nothing to correct
    u = np.zeros_like(v)
    for a, s in enumerate((2.0, -2.0, 2.0)[:D]):
        u[..., a] = s
    want = np.where(inter[None, ..., None], u, 0).astype(np.float32)
    for order, mode in ((1, 2), (2, 1), (2, 2)):
        assert_bits(_np(ops.advect_velocity(dev(u), 0.5, order=order, clamp_mode=mode, bnd=bnd)), want, "uniform shift")
    # a shift that moves a pattern: u_x = 2, u_y in {-2, 0, 2} per cell (u_z = 0), dt = 0.5.  The y component is gathered from whole cells
    # away; the x component is interpolated with dyadic weights between equal numbers.  Nothing rounds, in fp32 or fp64.
    rng = np.random.RandomState(3)
    w = np.zeros_like(v)
    w[..., 0] = 2.0
    w[..., 1] = 2.0 * rng.randint(-1, 2, size=w.shape[:-1])
    r64 = ref.mac_advect(w, 0.5, order=1, bnd=bnd, dtype=np.float64)
    assert_bits(_np(ops.advect_velocity(dev(w), 0.5, order=1, bnd=bnd)), r64["vel"].astype(np.float32), "pattern shift")
    np.testing.assert_array_equal(r64["vel"].astype(np.float32).astype(np.float64), r64["vel"])


def test_mac_parity_with_the_fp64_restatement():
    from deep_fluids_amd import ops
    n = 0
    for name, vel, kw in ref.mac_cases():
        r64 = ref.mac_advect(vel, ref.MAC_DT, dtype=np.float64, **kw)
        r32 = ref.mac_advect(vel, ref.MAC_DT, dtype=np.float32, **kw)
        e32, twin_out = aref.twin_error(r64, r32, kw["bnd"])
        got = _np(ops.advect_velocity(dev(vel), ref.MAC_DT, **kw))
        assert got.dtype == np.float32 and got.shape == vel.shape
        gs = ref.vel_to_stacked(got)
        print("%-24s e32 %.3e  gpu max %.3e  twin left out %.5f %%  gpu == twin bitwise: %s" %
              (name, e32, float(np.abs(gs - r64["out"]).max()), 100 * twin_out, bool(np.array_equal(gs, r32["out"]))))
        err, share = aref.compare(gs, r64, e32, kw["bnd"], ref.mac_alternatives(r64, vel, ref.MAC_DT, kw["clamp_mode"], kw["bnd"]))
        print("%-24s gpu %.3e (bound %.3e)  left out %.5f %%" % ("", err, 3 * e32 + 1e-7, 100 * share))
        # B = 1: the first entry alone is the first entry of the batch, bit for bit
        one = _np(ops.advect_velocity(dev(vel[:1]), ref.MAC_DT, **kw))
        assert_bits(one, got[:1], name + " B=1")
        n += 1
    assert n == 30
    v = dev(vel)
    with pytest.raises(ValueError):
        ops.advect_velocity(v, 0.5, out=v)
    with pytest.raises(ValueError):
        ops.advect_velocity(v, 0.5, workspace=torch.empty(8, device="cuda"))
    ws, out = torch.empty(v.numel(), device="cuda"), torch.empty_like(v)
    assert ops.advect_velocity(v, ref.MAC_DT, out=out, workspace=ws, **kw) is out
    assert_bits(_np(out), got, "out / workspace")


# ---- walls and buoyancy --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,bnd", SHAPES)
def test_wall_buoyancy_bitwise(shape, bnd):
    from deep_fluids_amd import ops
    D = len(shape)
    rng = np.random.RandomState(11)
    for B in (1, 3):
        vel = ref.make_velocity(shape, B=B, seed=2)
        rho = rng.uniform(0, 1, (B,) + shape).astype(np.float32)
        force = (0.013, 0.256, -0.07)[:D]
        want = ref.wall_buoyancy(vel, rho, force, bnd, np.float32)
        v = dev(vel)
        got = ops.wall_buoyancy(v, dev(rho), force, bnd=bnd)
        assert_bits(_np(got), want, "wall_buoyancy")
        for a in range(D):
            assert not _np(got)[..., a][:, ~ref.face_mask(shape, bnd, a)].any()
        assert_bits(_np(v), vel, "input untouched")
        assert ops.wall_buoyancy(v, dev(rho), force, bnd=bnd, out=v) is v                    # in place
        assert torch.equal(v, got)


# ---- pressure -------------------------------------------------------------------------------------------------------------------------------------
def _solve_input(shape, bnd, B=3, seed=4):
    rng = np.random.RandomState(seed)
    vel = ref.make_velocity(shape, B=B, seed=seed, vmax=1.0)
    rho = rng.uniform(0, 1, (B,) + shape).astype(np.float32)
    return ref.wall_buoyancy(vel, rho, (0.0, 0.25, 0.0)[:len(shape)], bnd, np.float32)


@pytest.mark.parametrize("shape,bnd", SOLVE_SHAPES)
def test_k_iterations_against_the_fp64_recurrence(shape, bnd):
    from deep_fluids_amd import ops
    w = _solve_input(shape, bnd)
    for k in (1, 2, 3, 4):
        x64, it64, _ = ref.cg(w, bnd, 0.0, k, np.float64)
        x32, _, _ = ref.cg(w, bnd, 0.0, k, np.float32)
        e32 = float(np.abs(x32 - x64).max())
        _, p, iters = ops.solve_pressure(dev(w), bnd=bnd, accuracy=0.0, max_iter=k)
        err = float(np.abs(_np(p) - x64).max())
        print("%s bnd %d k %d: e32 %.3e  gpu %.3e (bound %.3e)  |x| %.3e" % (shape, bnd, k, e32, err, 3 * e32 + 1e-7, float(np.abs(x64).max())))
        assert (_np(iters) == k).all() and (it64 == k).all()
        assert err <= 3 * e32 + 1e-7
        assert not _np(p)[:, ~ref.interior_mask(shape, bnd)].any()


@pytest.mark.parametrize("shape,bnd", SOLVE_SHAPES)
def test_solve_residual_and_projection(shape, bnd):
    from deep_fluids_amd import ops
    w = _solve_input(shape, bnd)
    acc = 1e-4
    max_iter = ops.default_max_iter(shape)
    b64 = ref.rhs(w, bnd, np.float64)
    v, p, iters = ops.solve_pressure(dev(w), bnd=bnd, accuracy=acc)
    x32, it32, r32 = ref.cg(w, bnd, acc, max_iter, np.float32)
    # the twin's own excess: the recurrence's r drifts from the true residual b - A p by rounding, and the solver stops on r.  By the
    # triangle inequality |b - A p| <= |r| + |(b - A p) - r| <= accuracy + drift; the drift is measured on the twin, in fp64.
    excess = float(np.abs((b64 - ref.apply_A(x32.astype(np.float64), bnd)) - r32).max())
    res = float(np.abs(b64 - ref.apply_A(_np(p).astype(np.float64), bnd)).max())
    print("%s bnd %d: iterations gpu %s twin %s  fp64 residual of the gpu's p %.4e (bound %.1e + twin's excess %.3e)" %
          (shape, bnd, _np(iters).tolist(), it32.tolist(), res, acc, excess))
    assert (_np(iters) > 0).all() and (_np(iters) < max_iter).all()
    assert res <= acc + excess
    if int(ref.interior_mask(shape, bnd).sum()) <= 1200:
        vex, _ = ref.exact_projection(w, bnd)
        v32 = ref.correct(w, x32, bnd, np.float32)
        d32 = float(np.abs(v32 - vex).max())
        dg = float(np.abs(_np(v) - vex).max())
        print("%s bnd %d: distance from the exact fp64 projection: twin %.3e  gpu %.3e" % (shape, bnd, d32, dg))
        assert dg <= 3 * d32
    for a in range(len(shape)):
        assert not _np(v)[..., a][:, ~ref.face_mask(shape, bnd, a)].any()


@pytest.mark.parametrize("shape,bnd", [((12, 10), 1), ((17, 130), 1), ((19, 10, 7), 1)])
def test_batch_invariance_determinism_and_check_every(shape, bnd):
    from deep_fluids_amd import ops
    w = _solve_input(shape, bnd)
    w[0] = 0                      # nothing to do
    w[1] *= 1e-3                  # easy: close to the accuracy already
    v, p, iters = ops.solve_pressure(dev(w), bnd=bnd)
    it = _np(iters).tolist()
    print("%s: iterations %s" % (shape, it))
    assert it[0] == 0 and not _np(p)[0].any() and 0 < it[1] < it[2]
    assert torch.isfinite(v).all() and torch.isfinite(p).all()
    for e in range(3):
        ve, pe, ie = ops.solve_pressure(dev(w[e:e + 1]), bnd=bnd)
        assert_bits(_np(pe)[0], _np(p)[e], "pressure of entry %d alone" % e)
        assert_bits(_np(ve)[0], _np(v)[e], "velocity of entry %d alone" % e)
        assert int(ie[0]) == it[e]
    ws = ops.pressure_workspace(dev(w))
    ws.fill_(float("nan"))                                 # nothing is read before it is written
    v2, p2, i2 = ops.solve_pressure(dev(w), bnd=bnd, workspace=ws)
    assert_bits(_np(p2), _np(p), "second run")
    assert_bits(_np(v2), _np(v), "second run")
    assert torch.equal(i2, iters)
    for ce in (1, 7):
        v3, p3, i3 = ops.solve_pressure(dev(w), bnd=bnd, check_every=ce, workspace=ws)
        assert_bits(_np(p3), _np(p), "check_every %d" % ce)
        assert_bits(_np(v3), _np(v), "check_every %d" % ce)
        assert torch.equal(i3, iters)
    vi = dev(w)
    assert ops.solve_pressure(vi, bnd=bnd, out=vi)[0] is vi and torch.equal(vi, v)            # in place


# ---- the step and the sequence ----------------------------------------------------------------------------------------------------------------
def _scene(shape, B=2):
    D = len(shape)
    ext = shape[::-1]
    masks = []
    for e in range(B):
        c = [0.5 * n for n in ext]
        c[0] = (0.4 + 0.2 * e) * ext[0]
        c[1] = 0.2 * ext[1]
        masks.append(aref.sphere_mask_loop(shape, c, 0.12 * ext[0] + e))
    return np.stack(masks), np.zeros((B,) + shape, np.float32), np.zeros((B,) + shape + (D,), np.float32)


@pytest.mark.parametrize("shape", [(32, 24), (12, 16, 12)])
def test_step_equals_its_parts_and_eight_steps_from_rest(shape):
    from deep_fluids_amd import ops
    D = len(shape)
    mask, d0, v0 = _scene(shape)
    m = torch.from_numpy(mask).cuda()
    dt, acc, T = 0.5, 1e-4, 8
    force = ops.default_buoyancy_force(shape, dt)
    assert force[1] > 0
    stats = []
    dT, vels = ops.simulate_smoke(dev(d0), dev(v0), T, dt=dt, source=m, stats=stats)
    assert tuple(vels.shape) == (T,) + v0.shape and len(stats) == T
    d, v = dev(d0), dev(v0)
    ycoord = np.arange(shape[-2]).reshape((1,) * (D - 1) + (shape[-2], 1)) + 0.5
    height = []
    for t in range(T):
        # the seven statements, one by one
        dn = ops.advect(d, v, dt, source=m)
        vn = ops.advect_velocity(v, dt)
        vn = ops.wall_buoyancy(vn, dn, force)
        vn, _, it = ops.solve_pressure(vn)
        ds, vs = ops.smoke_step(d, v, dt, source=m)
        assert torch.equal(ds, dn) and torch.equal(vs, vn)                       # bitwise
        assert torch.equal(vels[t], vn) and torch.equal(stats[t], it)
        d, v = dn, vn
        vh = _np(v)
        div = float(np.abs(ref.divergence(vh, 1)).max())
        rho = _np(d).astype(np.float64)
        height.append(float((rho * ycoord).sum() / rho.sum()))
        print("%s step %d: iterations %s  max|div| %.3e  mean height %.4f  max|v| %.4f" % (shape, t + 1, _np(it).tolist(), div, height[-1], float(np.abs(vh).max())))
        assert div <= acc * (2 * D + 1)                  # |div| = |b - A p| up to rounding: the residual bound times the stencil's width
        for a in range(D):
            assert not vh[..., a][:, ~ref.face_mask(shape, 1, a)].any()
    assert torch.equal(dT, d)
    assert height[-1] > height[0]                        # the smoke has risen
    frames = list(ops.simulate_smoke(dev(d0), dev(v0), 2, dt=dt, source=m, stack=False))
    assert len(frames) == 2 and torch.equal(frames[-1][1], vels[1])
    # against the fp64 sequence.  The solve is only accurate to `acc`, so fp64 and fp32 fields differ by the solver's tolerance, not by
    # rounding: the comparison is made at an accuracy both reach, 1e-6 of velocities of order 0.1, and bounded by the twin's distance.
    tight = 1e-6
    d64, v64, d32, v32 = d0, v0, d0, v0
    dg, vg = dev(d0), dev(v0)
    for t in range(T):
        d64, v64, rd64, _ = ref.step(d64, v64, dt, source=mask, accuracy=tight * 1e-3, dtype=np.float64)
        d32, v32, rd32, _ = ref.step(d32, v32, dt, source=mask, accuracy=tight, dtype=np.float32)
        dg, vg = ops.smoke_step(dg, vg, dt, source=m, accuracy=tight)
    e32v = float(np.abs(v32 - v64).max())
    e32d, twin_out = aref.twin_error(rd64, rd32, 1)
    gv = float(np.abs(_np(vg) - v64).max())
    print("%s T=8: velocity components outside 3*e32 + 1e-7: %.5f %%" % (shape, 100.0 * float((np.abs(_np(vg) - v64) > 3 * e32v + 1e-7).mean())))
    print("%s T=8: velocity e32 %.3e  gpu %.3e (bound %.3e);  density e32 %.3e  twin left out %.5f %%" % (shape, e32v, gv, 3 * e32v + 1e-7, e32d, 100 * twin_out))
    vbad = np.abs(_np(vg) - v64) > 3 * e32v + 1e-7
    assert float(vbad.sum()) / vbad.size <= 1e-3
    bad = np.abs(_np(dg) - d64) > 3 * e32d + 1e-7
    share = float(bad.sum()) / (int(ref.interior_mask(shape, 1).sum()) * d0.shape[0])
    print("%s T=8: density cells outside 3*e32 + 1e-7: %.5f %%" % (shape, 100 * share))
    assert share <= 1e-3


# ---- the dataset ----------------------------------------------------------------------------------------------------------------------------------
def test_generate_smoke_dataset(tmp_path):
    from deep_fluids_amd import ops
    from deep_fluids_amd.data import BatchManager, generate_smoke_dataset
    from deep_fluids_amd.trainer import smoke_pos_size_source
    root = str(tmp_path / "smoke")
    X, Y, T = 24, 32, 4
    n = generate_smoke_dataset(root, num_src_x_pos=3, num_src_radius=2, num_frames=T, resolution_x=X, resolution_y=Y, scenes_per_batch=4)
    assert n == 3 * 2 * T
    assert sorted(os.listdir(os.path.join(root, "v"))) == sorted("%d_%d_%d.npz" % (i, j, t) for i in range(3) for j in range(2) for t in range(T))
    args = dict(line.rstrip("\n").split(": ") for line in open(os.path.join(root, "args.txt")))
    want_keys = ["log_dir", "num_param", "path_format", "p0", "p1", "p2", "num_src_x_pos", "min_src_x_pos", "max_src_x_pos", "src_y_pos",
                 "num_src_radius", "min_src_radius", "max_src_radius", "num_frames", "min_frames", "max_frames", "num_simulations",
                 "resolution_x", "resolution_y", "buoyancy", "bWidth", "open_bound", "time_step", "adv_order", "clamp_mode"]
    assert list(args) == want_keys
    assert args["num_src_x_pos"] == "3" and args["max_frames"] == "3" and args["time_step"] == "0.5" and args["open_bound"] == "False"
    lo, hi = np.inf, -np.inf
    for i in range(3):
        for j in range(2):
            for t in range(T):
                with np.load(os.path.join(root, "v", "%d_%d_%d.npz" % (i, j, t))) as f:
                    assert sorted(f.files) == ["x", "y"]
                    x, y = f["x"], f["y"]
                assert x.dtype == np.float32 and x.shape == (Y, X, 2)
                np.testing.assert_array_equal(y, [i / 2.0 * (0.8 - 0.2) + 0.2, j / 1.0 * (0.12 - 0.04) + 0.04, t])
                lo, hi = min(lo, float(x.min())), max(hi, float(x.max()))
    assert open(os.path.join(root, "v_range.txt")).read() == "%.3f\n%.3f" % (lo, hi)
    assert hi > 0.01
    cfg = SimpleNamespace(random_seed=1, data_path=root, is_3d=False, data_type="velocity", arch="de", batch_size=5, res_x=X, res_y=Y, res_z=1,
                          num_worker=1)
    bm = BatchManager(cfg, device=None)
    xb, yb = bm.batch()
    bm.stop_thread()
    assert tuple(xb.shape) == (5, Y, X, 2) and tuple(yb.shape) == (5, 3)
    # v_range.txt carries three decimals: the normalised field may pass 1 by the rounding of the range, 0.0005 / x_range
    assert float(xb.abs().max()) <= 1 + 0.0005 / bm.x_range and float(yb.abs().max()) <= 1
    back = xb.numpy().astype(np.float64) * bm.x_range                   # ... and, scaled back, lies within the stored extremes
    assert lo - 1e-6 * bm.x_range <= back.min() and back.max() <= hi + 1e-6 * bm.x_range      # fp32 rounding of x / x_range
    src = smoke_pos_size_source(bm, 1, 1)
    assert src["center"] == (X * 0.5, Y * 0.1) and src["radius"] == X * 0.12
    mask = ops.sphere_mask((Y, X), src["center"], src["radius"], "cuda")
    assert int(mask.sum()) > 0
    # scene (1, 1) alone, re-simulated: the stored frames bit for bit
    d0 = torch.zeros((1, Y, X), device="cuda")
    v0 = torch.zeros((1, Y, X, 2), device="cuda")
    _, vels = ops.simulate_smoke(d0, v0, T, dt=0.5, source=mask[None], force=ops.default_buoyancy_force((Y, X), 0.5))
    for t in range(T):
        with np.load(os.path.join(root, "v", "1_1_%d.npz" % t)) as f:
            assert_bits(_np(vels[t, 0]), f["x"], "frame %d of scene (1, 1)" % t)
    with pytest.raises(NotImplementedError):
        generate_smoke_dataset(str(tmp_path / "open"), open_bound=True)
