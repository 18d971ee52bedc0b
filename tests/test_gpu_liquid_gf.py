"""GPU side of the liquid solver's surface (the averaged level set of particles.hip, the `_gf` pressure entry points of smoke.hip, the
step with `ghost_fluid`) against tests/liquid_gf_ref.py.

The level set is compared BITWISE with the fp32 twin, which performs the same operations in the same order (the library is built
without contraction, as for particles_to_grid).  The solve cannot be bitwise -- its dot products are summed in workgroup order -- and
is bounded through `accuracy` in the form of test_gpu_liquid.test_projection_against_the_dense_solve; the chained step by the margin
of test_four_steps_of_a_drop_falling_into_a_basin.  Every parity test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

import liquid_gf_ref as gref
import liquid_ref as ref
from gpu_util import assert_bits, dev

pytestmark = pytest.mark.gpu


def _np(t):
    return t.cpu().numpy()


def _u8(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


# ---- the averaged level set -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,B,bnd", gref.LEVELSET_CASES)
@pytest.mark.parametrize("radius_factor", [1.0, 2.5])
def test_levelset_bitwise(shape, B, bnd, radius_factor):
    from deep_fluids_amd import ops
    pos = gref.levelset_positions(shape, B, bnd, 11)
    kw = dict(radius_factor=radius_factor, bnd=bnd)
    got = ops.particle_levelset_averaged(dev(pos), shape, **kw)
    t32 = gref.levelset_averaged(pos, shape, dtype=np.float32, **kw)
    t64 = gref.levelset_averaged(pos, shape, dtype=np.float64, **kw)
    print("%s rf %.1f: twin-vs-fp64 %.3e  gpu-vs-fp64 %.3e" % (shape, radius_factor, ref.max_err(t32, t64), ref.max_err(_np(got), t64)))
    assert_bits(_np(got), t32, "averaged level set, smooth 1, smooth_neg 1, band")
    for smooth, neg in ((0, 0), (0, 1), (2, 0), (1, 2), (2, 2)):
        g = ops.particle_levelset_averaged(dev(pos), shape, smooth=smooth, smooth_neg=neg, bound_value=0.75, **kw)
        assert_bits(_np(g), gref.levelset_averaged(pos, shape, smooth=smooth, smooth_neg=neg, bound_value=0.75, dtype=np.float32, **kw),
                    "smooth %d, smooth_neg %d" % (smooth, neg))
    raw = ops.particle_levelset_averaged(dev(pos), shape, radius_factor=radius_factor, smooth=0, smooth_neg=0, bnd=0)
    assert_bits(_np(raw), gref.levelset_averaged(pos, shape, radius_factor, 0, 0, 1.0, 0, np.float32), "no pass, no band")
    # every entry alone, the caller's sort, a second run, out=
    for e in range(B):
        assert_bits(_np(ops.particle_levelset_averaged(dev(pos[e:e + 1]), shape, **kw))[0], _np(got)[e], "entry %d alone" % e)
    spos, cell_start, _ = ops.particle_cells(dev(pos), shape)
    out = torch.full_like(got, float("nan"))
    assert ops.particle_levelset_averaged(dev(pos), shape, out=out, cells=(spos, cell_start), **kw) is out and torch.equal(out, got)
    # no particles: the radius, and the band
    none = ops.particle_levelset_averaged(dev(pos[:, :0]), shape, **kw)
    assert_bits(_np(none), gref.levelset_averaged(pos[:, :0], shape, dtype=np.float32, **kw), "N = 0")


# ---- the ghost-fluid solve against the dense fp64 solve ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(gref.solve_cases()), ids=lambda c: c[0])
def test_ghost_fluid_projection_against_the_dense_solve(case):
    from deep_fluids_amd import ops
    name, liquid, w, phi, clamp = case
    shape = liquid.shape[1:]
    D = len(shape)
    assert all(n > 0 for n in gref.theta_branches(phi, liquid, clamp)), gref.theta_branches(phi, liquid, clamp)
    flags = _u8(ref.flags_of(liquid)[0])
    acc = 1e-4
    max_iter = ops.default_max_iter(shape)
    v, p, iters = ops.solve_pressure_liquid(dev(w), flags, accuracy=acc, phi=dev(phi), gf_clamp=clamp)
    x32, it32, r32 = gref.pcg(w, liquid, phi, 1, acc, max_iter, clamp, np.float32)
    # |b - A p| <= |r| + |(b - A p) - r| <= accuracy + the recurrence's drift, measured on the twin in fp64
    excess = float(np.abs(gref.residual(w, x32, liquid, phi, 1, clamp) - r32).max())
    res = float(np.abs(gref.residual(w, _np(p), liquid, phi, 1, clamp)).max())
    print("%s: iterations gpu %s twin %s  fp64 residual of the gpu's p %.4e (bound %.1e + twin's excess %.3e)" %
          (name, _np(iters).tolist(), it32.tolist(), res, acc, excess))
    assert (_np(iters) > 0).all() and (_np(iters) < max_iter).all()
    assert res <= acc + excess
    assert not _np(p)[~liquid].any()
    vex, _ = gref.exact_projection(w, liquid, phi, 1, clamp)
    v32 = gref.correct(w, x32, liquid, phi, 1, clamp, np.float32)
    d32 = float(np.abs(v32 - vex).max())
    dg = float(np.abs(_np(v) - vex).max())
    print("%s: distance from the exact fp64 projection: twin %.3e  gpu %.3e" % (name, d32, dg))
    assert dg <= 3 * d32
    # the liquid cells' divergence after the correction is b - A p up to the rounding of the correction (the surface faces carry p / theta)
    div = float(np.abs(ref.divergence(_np(v), liquid)).max())
    it64, _ = gref.inv_theta(phi, liquid, 1, clamp, np.float64)
    big = float(np.abs(it64 * _np(p).astype(np.float64)[None]).max())
    print("%s: max |div| over liquid cells %.3e" % (name, div))
    assert div <= acc + excess + (2 * D) * 2.0 ** -22 * float(np.abs(w).max() + 2 * max(np.abs(_np(p)).max(), big))
    for a in range(D):
        live, kept = ref.live_face(liquid, 1, a), ref.both_interior(shape, 1, a)[None]
        assert_bits(_np(v)[..., a][kept & ~live], w[..., a][kept & ~live], "faces without a liquid cell are copied")
        assert not _np(v)[..., a][np.broadcast_to(~kept, live.shape)].any()
    # determinism, batch invariance, check_every, the workspace is written before it is read, in place
    ws = ops.pressure_workspace(dev(w), ghost_fluid=True)
    assert ws.numel() == ops.pressure_workspace(dev(w)).numel() + 2 * liquid.size
    ws.fill_(float("nan"))
    v2, p2, i2 = ops.solve_pressure_liquid(dev(w), flags, accuracy=acc, workspace=ws, check_every=3, phi=dev(phi), gf_clamp=clamp)
    assert torch.equal(v2, v) and torch.equal(p2, p) and torch.equal(i2, iters)
    for e in range(2):
        ve, pe, ie = ops.solve_pressure_liquid(dev(w[e:e + 1]), flags[e:e + 1].contiguous(), accuracy=acc, phi=dev(phi[e:e + 1]), gf_clamp=clamp)
        assert_bits(_np(pe)[0], _np(p)[e], "pressure of entry %d alone" % e)
        assert_bits(_np(ve)[0], _np(v)[e], "velocity of entry %d alone" % e)
    vi = dev(w)
    assert ops.solve_pressure_liquid(vi, flags, accuracy=acc, out=vi, phi=dev(phi), gf_clamp=clamp)[0] is vi and torch.equal(vi, v)
    with pytest.raises(Exception, match="workspace"):                      # the plain workspace is too small: refused on the C side
        ops.solve_pressure_liquid(dev(w), flags, workspace=ops.pressure_workspace(dev(w)), phi=dev(phi))


@pytest.mark.parametrize("shape", [(8, 8), (6, 6, 6)])
def test_max_iter_zero_a_frozen_entry_and_unit_theta(shape):
    from deep_fluids_amd import ops
    D = len(shape)
    liquid, w = gref.ragged(shape, 2, 3)
    phi = gref.branch_phi(liquid, 5)
    flags = _u8(ref.flags_of(liquid)[0])
    # max_iter = 0: p = 0, no iteration, the correction of a zero pressure
    v, p, iters = ops.solve_pressure_liquid(dev(w), flags, max_iter=0, phi=dev(phi))
    assert not _np(p).any() and not _np(iters).any()
    assert_bits(_np(v), gref.correct(w, np.zeros(liquid.shape, np.float32), liquid, phi, 1, 1e-4, np.float32), "max_iter = 0")
    # an all-air entry beside a live one: b = 0, it stops at iteration 0 and is not touched; the live one has the bits of its own call
    liq2 = liquid.copy(); liq2[0] = False
    w2 = w.copy(); w2[0] = ref.forces(w[:1], liq2[:1], (0.0,) * D, 1, np.float32)[0]
    f2 = _u8(ref.flags_of(liq2)[0])
    v2, p2, i2 = ops.solve_pressure_liquid(dev(w2), f2, phi=dev(phi))
    assert int(i2[0]) == 0 and int(i2[1]) > 0 and not _np(p2)[0].any()
    assert_bits(_np(v2)[0], w2[0], "the all-air entry's velocity is copied")
    v1, p1, _ = ops.solve_pressure_liquid(dev(w2[1:]), f2[1:].contiguous(), phi=dev(phi[1:]))
    assert_bits(_np(p2)[1], _np(p1)[0], "the live entry beside a frozen one")
    assert_bits(_np(v2)[1], _np(v1)[0], "the live entry beside a frozen one")
    # every theta 1: the first-order system, solved by another iteration -- the pressures agree to the two solves' accuracy
    acc = 1e-5
    one = gref.unit_theta_phi(liquid)
    vg, pg, ig = ops.solve_pressure_liquid(dev(w), flags, accuracy=acc, phi=dev(one))
    vp, pp, ip = ops.solve_pressure_liquid(dev(w), flags, accuracy=acc)
    rg = float(np.abs(gref.residual(w, _np(pg), liquid, one)).max())
    rp = float(np.abs(gref.residual(w, _np(pp), liquid, one)).max())
    ninv = max(float(np.abs(np.linalg.inv(gref.dense_matrix(liquid[e], one[e].astype(np.float64))[0])).sum(axis=1).max()) for e in range(2))
    dp = float(np.abs(_np(pg).astype(np.float64) - _np(pp)).max())
    pmax = float(max(np.abs(_np(pg)).max(), np.abs(_np(pp)).max()))
    print("%s unit theta: iterations pcg %s cg %s  fp64 residuals %.3e %.3e  |A^-1|_inf %.2f  pressure difference %.3e (bound %.3e)" %
          (shape, _np(ig).tolist(), _np(ip).tolist(), rg, rp, ninv, dp, ninv * (rg + rp) + 2.0 ** -22 * pmax))
    assert (_np(ig) > 0).all() and (_np(ip) > 0).all()
    # every liquid region of these masks touches air (tests/test_liquid_gf_host.py): A is non-singular and
    # p_g - p_p = A^-1 ((b - A p_p) - (b - A p_g)), the residuals taken in fp64 of the fp32 pressures; 2^-22 |p| for their evaluation
    assert dp <= ninv * (rg + rp) + 2.0 ** -22 * pmax
    # the corrected velocities: a face carries a difference of two pressures (or one, at the surface with theta 1)
    assert float(np.abs(_np(vg) - _np(vp)).max()) <= 2 * dp + 2.0 ** -22 * float(np.abs(w).max() + 2 * pmax)


# ---- the hydrostatic column: what the feature is for ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", gref.HYDRO_SHAPES)
@pytest.mark.parametrize("s", gref.HYDRO_S)
def test_hydrostatic_column(shape, s):
    from deep_fluids_amd import ops
    D = len(shape)
    g, acc = gref.HYDRO_G, 1e-6
    liquid, vel, phi, depth = gref.hydrostatic_case(shape, s)
    flags = _u8(ref.flags_of(liquid)[0])
    w = ops.liquid_forces(torch.zeros((1,) + shape + (D,), device="cuda"), flags, (0.0, g, 0.0)[:D])
    assert_bits(_np(w), vel, "the column's velocity after the force")
    v, p, iters = ops.solve_pressure_liquid(w, flags, accuracy=acc, phi=dev(phi))
    want = abs(g) * depth
    # the bound the twin gives: p - p* = A^-1 (b - A p), |b - A p| <= accuracy + the twin's drift, |A^-1|_inf from the dense fp64 matrix;
    # p* itself is |g| * depth up to the fp32 rounding of phi (measured in fp64).  A corrected face is a difference of two such
    # pressures or one of them over theta >= s, plus the rounding of the correction.
    cap = ops.default_max_iter(shape)
    x32, it32, r32 = gref.pcg(vel, liquid, phi, 1, acc, cap, 1e-4, np.float32)
    excess = float(np.abs(gref.residual(vel, x32, liquid, phi) - r32).max())
    A, _ = gref.dense_matrix(liquid[0], phi[0].astype(np.float64))
    ninv = float(np.abs(np.linalg.inv(A)).sum(axis=1).max())
    vex, pex = gref.exact_projection(vel, liquid, phi)
    model = float(np.abs(pex - want).max())
    pb = ninv * (acc + excess) + model
    fb = max(2.0, 1.0 / s) * pb + float(np.abs(vex).max()) + 2.0 ** -22 * (abs(g) + 2 * float(want.max()) / s)
    ep, ev = float(np.abs(_np(p) - want).max()), float(np.abs(_np(v)).max())
    e32 = float(np.abs(x32 - want).max())
    print("%s s %.2f: iterations gpu %s twin %s  |p - |g| depth| gpu %.3e twin %.3e (bound %.3e)  max |corrected face| %.3e (bound %.3e)" %
          (shape, s, _np(iters).tolist(), it32.tolist(), ep, e32, pb, ev, fb))
    assert 0 < int(iters[0]) < cap
    assert ep <= pb and e32 <= pb
    assert ev <= fb
    # the first-order path puts |g| * 1 into the top cell where the ghost-fluid one puts |g| * s
    v1, p1, _ = ops.solve_pressure_liquid(w, flags, accuracy=acc)
    top = (slice(None),) * (D - 1) + (shape[-2] // 2 - 1,)
    t1, tg = _np(p1)[top][liquid[top]], _np(p)[top][liquid[top]]
    assert float(np.abs(t1 - abs(g)).max()) <= pb + 4 * acc * shape[-2] and float(np.abs(tg - abs(g) * s).max()) <= pb


# ---- the chained step ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", gref.STEP_SHAPES)
def test_four_steps_with_the_ghost_fluid_surface(shape):
    from deep_fluids_amd import ops
    from test_gpu_liquid import drop_scene
    pos0, vel0 = drop_scene(shape, gref.STEP_SEEDS[shape])
    dt, tight, T = 0.5, 1e-6, 4
    pvel0 = ref.sample(vel0, pos0, np.float32)
    s64 = dict(pos=pos0.astype(np.float64), pvel=pvel0.astype(np.float64), vel=vel0.astype(np.float64))
    s32 = dict(pos=pos0, pvel=pvel0, vel=vel0)
    p, u, v = dev(pos0), dev(pvel0), dev(vel0)
    stats = []
    _, _, vels = ops.simulate_liquid(p, u, v, T, dt=dt, accuracy=tight, stats=stats, ghost_fluid=True)
    for t in range(T):
        s64 = gref.step(s64["pos"], s64["pvel"], s64["vel"], dt, accuracy=tight * 1e-3, dtype=np.float64)
        s32 = gref.step(s32["pos"], s32["pvel"], s32["vel"], dt, accuracy=tight, dtype=np.float32)
        p, u, v, iters = ops.liquid_step(p, u, v, dt, accuracy=tight, ghost_fluid=True)
        assert torch.equal(v, vels[t]) and torch.equal(iters, stats[t])
        np.testing.assert_array_equal(s32["cell_start"], s64["cell_start"])
        spos, gcs, _ = ops.particle_cells(p, shape)
        np.testing.assert_array_equal(_np(gcs), s64["cell_start"])
        e32 = [ref.max_err(s32[k], s64[k]) for k in ("vel", "pos", "pvel")]
        eg = [ref.max_err(_np(x), s64[k]) for x, k in ((v, "vel"), (p, "pos"), (u, "pvel"))]
        et = [ref.max_err(_np(x), s32[k]) for x, k in ((v, "vel"), (p, "pos"), (u, "pvel"))]
        print("%s step %d: iterations %s  vel/pos/pvel twin-vs-fp64 %.3e %.3e %.3e  gpu-vs-fp64 %.3e %.3e %.3e  gpu-vs-twin %.3e %.3e %.3e"
              % ((shape, t + 1, _np(iters).tolist()) + tuple(e32) + tuple(eg) + tuple(et)))
        for k in range(3):
            # margin 3 over the twin's own error on these inputs plus the two solves' accuracy, as in test_gpu_liquid
            assert eg[k] <= 3 * e32[k] + 2 * tight * max(shape), (k, eg[k], e32[k])
            assert et[k] <= 3 * e32[k] + 2 * tight * max(shape), (k, et[k], e32[k])
    # the surface changes the frames, and with ghost_fluid=False the step is the one without the argument, bit for bit
    a = ops.liquid_step(dev(pos0), dev(pvel0), dev(vel0), dt, accuracy=tight, ghost_fluid=False)
    b = ops.liquid_step(dev(pos0), dev(pvel0), dev(vel0), dt, accuracy=tight)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[2], vels[0])
    _, _, plain = ops.simulate_liquid(dev(pos0), dev(pvel0), dev(vel0), 2, dt=dt, accuracy=tight, ghost_fluid=False)
    _, _, old = ops.simulate_liquid(dev(pos0), dev(pvel0), dev(vel0), 2, dt=dt, accuracy=tight)
    assert torch.equal(plain, old)
