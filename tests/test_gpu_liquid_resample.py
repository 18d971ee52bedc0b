"""GPU side of the liquid solver's resampling block (the ragged forms of the trace, the keys and the FLIP update, the level-set
extrapolation, the count and scatter passes of liquid.hip) against tests/liquid_resample_ref.py.

Nothing here passes through a solve, so every comparison is BITWISE with the fp32 twin, which performs the same operations in the same
order (the library is built without contraction).  The shapes are the smallest at which each thing can go wrong: 2-D 12x10 and 3-D
8x10x12, bnd 1, B = 3 (more than one block of cells in 3-D, odd particle counts, an empty entry).
The step with `resample=` does pass through the solve: every step is compared with the twin's step FROM THE SAME STATE (the GPU's own
previous result), so the traced positions, the ranges, the keep decisions and the seeds stay bitwise, and only `pvel` and `vel` carry the
solve's tolerance, taken as tests/test_gpu_liquid.py takes it."""
import numpy as np
import pytest
import torch

import liquid_ref as ref
import liquid_resample_ref as rr
from gpu_util import assert_bits, dev

pytestmark = pytest.mark.gpu

N = 67


def _np(t):
    return t.cpu().numpy()


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def _nan_equal(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), what


@pytest.mark.parametrize("shape", rr.SHAPES)
def test_ragged_with_even_starts_is_dense(shape):
    from deep_fluids_amd import ops
    D = len(shape)
    rng = np.random.RandomState(4)
    lo, hi = rr.pref.clamp_bounds(shape, rr.BND, np.float32)
    pos = (lo + rng.uniform(0, 1, size=(rr.B, N, D)) * (hi - lo)).astype(np.float32)
    pvel = rng.standard_normal(pos.shape).astype(np.float32)
    vel, vel2 = rr.velocity(shape, 2), rr.velocity(shape, 3)
    es = _i32(np.arange(rr.B + 1) * N)
    p, u, v, v2 = dev(pos), dev(pvel), dev(vel), dev(vel2)
    flat, uflat = p.view(-1, D), u.view(-1, D)
    dense = ops.advect_particles(p, v, 0.5, bnd=rr.BND)
    assert torch.equal(ops.advect_particles(flat, v, 0.5, bnd=rr.BND, entry_start=es).view(dense.shape), dense)
    sp, cs, order = ops.particle_cells(p, shape)
    rsp, rcs, rorder = ops.particle_cells(flat, shape, entry_start=es)
    assert torch.equal(rsp.view(sp.shape), sp) and torch.equal(rcs, cs) and torch.equal(rorder, order)
    dense = ops.flip_update(p, u, v, v2, 0.9)
    assert torch.equal(ops.flip_update(flat, uflat, v, v2, 0.9, entry_start=es).view(dense.shape), dense)
    assert torch.equal(ops.sample_velocity(v, flat, entry_start=es).view(dense.shape), ops.sample_velocity(v, p))
    assert torch.equal(ops.particle_levelset_averaged(flat, shape, entry_start=es), ops.particle_levelset_averaged(p, shape))


@pytest.mark.parametrize("shape", rr.SHAPES)
def test_ragged_is_every_entry_alone(shape):
    from deep_fluids_amd import ops
    D = len(shape)
    pos, pvel, es, parts, vels = rr.ragged_case(shape, N, 1)
    vel, vel2 = rr.velocity(shape, 2), rr.velocity(shape, 3)
    p, u, v, v2, e = dev(pos), dev(pvel), dev(vel), dev(vel2), _i32(es)
    ncell = int(np.prod(shape))
    live = int(es[-1])
    moved = _np(ops.advect_particles(p, v, 0.5, bnd=rr.BND, entry_start=e))
    flipped = _np(ops.flip_update(p, u, v, v2, 0.9, entry_start=e))
    sp, cs, order = ops.particle_cells(p, shape, entry_start=e)
    keys = torch.empty((len(pos),), dtype=torch.int32, device="cuda")
    ops.call("df_particles_cell_keys%dd_ragged" % D, p.data_ptr(), keys.data_ptr(), e.data_ptr(), rr.B, N,
             *(list(shape) + [torch.cuda.current_stream().cuda_stream]))
    keys = _np(keys)
    assert (keys[live:] == rr.B * ncell).all()
    np.testing.assert_array_equal(keys, rr.keys(pos, es, shape))
    for b in range(rr.B):
        rows = slice(int(es[b]), int(es[b + 1]))
        if not len(parts[b]):
            continue
        one = dev(parts[b][None])
        assert_bits(moved[rows], _np(ops.advect_particles(one, v[b:b + 1], 0.5, bnd=rr.BND))[0], "trace, entry %d" % b)
        assert_bits(flipped[rows], _np(ops.flip_update(one, dev(vels[b][None]), v[b:b + 1], v2[b:b + 1], 0.9))[0], "FLIP, entry %d" % b)
        _, cs1, _ = ops.particle_cells(one, shape)
        np.testing.assert_array_equal(_np(cs)[b * ncell:(b + 1) * ncell + 1] - int(es[b]), _np(cs1))
    # the twin, bitwise; unused rows come back untouched (NaN payloads and all); the sort keeps entry_start
    assert_bits(moved[:live], rr.trace(pos, vel, es, 0.5, rr.BND, 1.0, np.float32)[:live], "ragged trace vs twin")
    assert_bits(flipped[:live], rr.flip_update(pos, pvel, vel, vel2, es, 0.9, np.float32)[:live], "ragged FLIP vs twin")
    out = torch.full_like(p, 7.0)
    ops.advect_particles(p, v, 0.5, bnd=rr.BND, entry_start=e, out=out)
    assert (out[live:] == 7.0).all()
    out = torch.full_like(p, 7.0)
    ops.flip_update(p, u, v, v2, 0.9, entry_start=e, out=out)
    assert (out[live:] == 7.0).all()
    tsp, _, tcs, torder = rr.sort(pos, None, es, shape)
    np.testing.assert_array_equal(_np(cs), tcs)
    np.testing.assert_array_equal(_np(order), torder)
    _nan_equal(_np(sp), tsp, "sorted positions")
    assert int(_np(cs)[-1]) == live and list(_np(cs)[::ncell]) == list(es)
    # everything driven by cell_start takes the ragged batch as it is
    phi = ops.particle_levelset_averaged(p, shape, entry_start=e, cells=(sp, cs))
    for b in (0, 2):
        assert_bits(_np(phi)[b], _np(ops.particle_levelset_averaged(dev(parts[b][None]), shape))[0], "level set, entry %d" % b)
    assert_bits(_np(phi)[1], _np(ops.particle_levelset_averaged(dev(parts[1][None]), shape))[0], "level set, the empty entry")
    su = torch.empty_like(u)
    ops.call("df_particles_gather", u.data_ptr(), order.data_ptr(), su.data_ptr(), len(pos), D, torch.cuda.current_stream().cuda_stream)
    gv, gw, gk = ops.particles_to_grid(sp.view(rr.B, N, D), su.view(rr.B, N, D), cs, shape)
    fl, touch = ops.liquid_flags(cs, shape, rr.B, N, bnd=rr.BND)
    for b in (0, 2):
        sp1, cs1, o1 = ops.particle_cells(dev(parts[b][None]), shape)
        su1 = dev(vels[b][None]).view(-1, D)[o1].view(1, -1, D).contiguous()
        v1, w1, k1 = ops.particles_to_grid(sp1, su1, cs1, shape)
        assert torch.equal(gv[b], v1[0]) and torch.equal(gw[b], w1[0]) and torch.equal(gk[b], k1[0])
        f1, t1 = ops.liquid_flags(cs1, shape, 1, len(parts[b]), bnd=rr.BND)
        assert torch.equal(fl[b], f1[0]) and torch.equal(touch[b], t1[0])
    assert not fl[1].any() and not gk[1].any()


@pytest.mark.parametrize("shape", rr.SHAPES)
def test_extrapolate_levelset_bitwise(shape):
    from deep_fluids_amd import ops
    phi = rr.pocket_phi(shape, 3)
    g = dev(phi)
    for inside in (True, False):
        for distance in (0, 1, 2, 4):
            got = ops.extrapolate_levelset(g, distance, inside)
            t32 = rr.extrapolate_levelset(phi, distance, inside, np.float32)
            t64 = rr.extrapolate_levelset(phi, distance, inside, np.float64)
            print("%s distance %d inside %s: twin-vs-fp64 %.3e  gpu-vs-fp64 %.3e  cells changed %d" %
                  (shape, distance, inside, ref.max_err(t32, t64), ref.max_err(_np(got), t64), int((t32 != phi).sum())))
            assert_bits(_np(got), t32, "extrapolated level set, distance %d, inside %s" % (distance, inside))
            assert got.data_ptr() != g.data_ptr() and torch.equal(g, dev(phi))          # the input is left untouched
    assert (rr.extrapolate_levelset(phi, 4, True, np.float32)[0] != phi[0]).any()         # the pocket and the surface did something
    # all negative: nothing marked, the input's bits (entry 1 within the batch, and alone)
    assert_bits(_np(ops.extrapolate_levelset(g, 4, True))[1], phi[1], "all-negative entry")
    assert_bits(_np(ops.extrapolate_levelset(g[1:2].contiguous(), 4, True)), phi[1:2], "all-negative phi alone")
    # out=, in place, and a second run
    out = torch.full_like(g, float("nan"))
    assert ops.extrapolate_levelset(g, 4, True, out=out) is out and torch.equal(out, ops.extrapolate_levelset(g, 4, True))
    work = g.clone()
    assert ops.extrapolate_levelset(work, 4, True, out=work) is work and torch.equal(work, out)


def _resample(st, **kw):
    from deep_fluids_amd import ops
    liquid = st["liquid"]
    flags, _ = ref.flags_of(liquid)
    args = (dev(st["pos"]), dev(st["pvel"]), _i32(st["cell_start"]), _i32(st["entry_start"]), dev(st["phi"]),
            torch.from_numpy(flags).cuda(), dev(st["vel"]), rr.MIN_P)
    return ops.resample_particles(*args, bnd=rr.BND, details=True, **kw)


@pytest.mark.parametrize("shape", rr.SHAPES)
def test_resample_particles_bitwise(shape):
    st = rr.resample_state(shape)
    pos, pvel, es, cs, (keep, kept, seeds) = _resample(st)
    t = rr.resample(st["pos"], st["pvel"], st["cell_start"], st["phi"], st["liquid"], st["vel"], rr.MIN_P, dtype=np.float32)
    t["old_cell_start"] = st["cell_start"]
    rr.check_invariants(t, st["phi"], st["liquid"], rr.MIN_P, 2 * rr.MIN_P)
    total = t["total"]
    print("%s: %d rows, %d live -> %d (%d seeds, %d dropped)" % (shape, len(st["pos"]), int(st["cell_start"][-1]), total, int(t["seeds"].sum()),
                                                                 int(st["cell_start"][-1]) - int(t["kept"].sum())))
    live = int(st["cell_start"][-1])
    np.testing.assert_array_equal(_np(keep)[:live], t["keep"][:live])
    np.testing.assert_array_equal(_np(kept), t["kept"])
    np.testing.assert_array_equal(_np(seeds), t["seeds"])
    np.testing.assert_array_equal(_np(cs), t["cell_start"])
    np.testing.assert_array_equal(_np(es), t["entry_start"])
    assert total <= len(st["pos"]) and t["seeded"].sum() > 0 and (t["keep"][:live] == 0).any()
    assert_bits(_np(pos)[:total][~t["seeded"]], t["pos"][~t["seeded"]], "kept positions")
    assert_bits(_np(pvel)[:total][~t["seeded"]], t["pvel"][~t["seeded"]], "kept velocities")
    assert_bits(_np(pos)[:total][t["seeded"]], t["pos"][t["seeded"]], "seeded positions")
    assert_bits(_np(pvel)[:total][t["seeded"]], t["pvel"][t["seeded"]], "seeded velocities")
    # the cases of the state (the host test checks that the twin holds them), and the invariants on the GPU's own result.  phiv and
    # seeded are the TWIN's: sound only because keep and the ranges were asserted equal to the twin's above, not an independent sample
    g = dict(pos=_np(pos)[:total], pvel=_np(pvel)[:total], entry_start=_np(es), cell_start=_np(cs), keep=_np(keep), kept=_np(kept),
             seeds=_np(seeds), phiv=t["phiv"], seeded=t["seeded"], total=total, old_cell_start=st["cell_start"])
    rr.check_invariants(g, st["phi"], st["liquid"], rr.MIN_P, 2 * rr.MIN_P)
    c = st["cells"]
    assert g["kept"][c["deep_crowded"]] == 2 * rr.MIN_P + 1 and g["kept"][c["surface_crowded"]] == 2 * rr.MIN_P + 3
    assert g["seeds"][c["last_column"]] == rr.MIN_P - 1 and g["seeds"][c["emptied"]] == rr.MIN_P
    sd = g["pos"][t["seeded"]]
    X = shape[-1]
    assert (np.floor(sd[:, 0]) == X - 2).any() and (sd[:, 0] < X - 1).all()
    # the same (seed, step) twice; another step moves the seeds and nothing else
    again = _resample(st)
    assert torch.equal(again[0][:total], pos[:total]) and torch.equal(again[1][:total], pvel[:total])
    other = _resample(st, step=1)
    t1 = rr.resample(st["pos"], st["pvel"], st["cell_start"], st["phi"], st["liquid"], st["vel"], rr.MIN_P, step=1, dtype=np.float32)
    assert_bits(_np(other[0])[:total], t1["pos"], "step 1 positions")
    assert_bits(_np(other[1])[:total], t1["pvel"], "step 1 velocities")
    assert (_np(other[0])[:total][t["seeded"]] != g["pos"][t["seeded"]]).any()
    # the output is a sorted ragged batch: the keys kernel and the sort agree with new_start
    from deep_fluids_amd import ops
    _, cs2, _ = ops.particle_cells(pos, shape, entry_start=es)
    assert torch.equal(cs2, cs)


@pytest.mark.parametrize("shape", rr.SHAPES)
def test_resample_refuses_a_state_that_does_not_fit(shape):
    """a guard check on valid memory: the storage is a view of a larger tensor whose tail holds a canary"""
    from deep_fluids_amd import _lib, ops
    st = rr.resample_state(shape)
    D = len(shape)
    live = int(st["cell_start"][-1])
    P = -(-live // rr.B) * rr.B                                           # room for the live particles, none for the seeds
    t = rr.resample(st["pos"], st["pvel"], st["cell_start"], st["phi"], st["liquid"], st["vel"], rr.MIN_P, dtype=np.float32)
    assert t["total"] > P
    flags, _ = ref.flags_of(st["liquid"])
    pad = 4096
    # the op allocates its outputs; call the passes on storage of ours, as the op does, to watch the rows behind P
    big_pos = torch.full((P + pad, D), -77.0, device="cuda")
    big_vel = torch.full((P + pad, D), -77.0, device="cuda")
    pos_in, pvel_in = dev(st["pos"][:P]), dev(st["pvel"][:P])
    with pytest.raises(_lib.DeepFluidsHipError, match=r"capacity of at least %d" % (-(-t["total"] // rr.B) * rr.B)):
        ops.resample_particles(pos_in, pvel_in, _i32(st["cell_start"]), _i32(st["entry_start"]), dev(st["phi"]),
                               torch.from_numpy(flags).cuda(), dev(st["vel"]), rr.MIN_P, bnd=rr.BND)
    ncell = int(np.prod(shape))
    keep = torch.zeros((P,), dtype=torch.uint8, device="cuda")
    kept = torch.empty((rr.B * ncell,), dtype=torch.int32, device="cuda")
    seeds = torch.empty_like(kept)
    s = torch.cuda.current_stream().cuda_stream
    cs, ph, fl, v = _i32(st["cell_start"]), dev(st["phi"]), torch.from_numpy(flags).cuda(), dev(st["vel"])
    ops.call("df_resample_count%dd" % D, pos_in.data_ptr(), cs.data_ptr(), ph.data_ptr(), fl.data_ptr(), keep.data_ptr(), kept.data_ptr(),
             seeds.data_ptr(), rr.B, P // rr.B, *(list(shape) + [rr.BND, rr.MIN_P, 2 * rr.MIN_P, 1.0, s]))
    new_start = _i32(np.concatenate([[0], np.cumsum(_np(kept).astype(np.int64) + _np(seeds))]))
    assert int(_np(new_start)[-1]) == t["total"]
    ops.call("df_resample_scatter%dd" % D, pos_in.data_ptr(), pvel_in.data_ptr(), cs.data_ptr(), keep.data_ptr(), seeds.data_ptr(),
             new_start.data_ptr(), v.data_ptr(), big_pos.data_ptr(), big_vel.data_ptr(), rr.B, P // rr.B, *(list(shape) + [rr.MIN_P, 123, 0, s]))
    torch.cuda.synchronize()
    assert (big_pos[P:] == -77.0).all() and (big_vel[P:] == -77.0).all()               # the canary is intact
    assert_bits(_np(big_pos)[:P], t["pos"][:P], "the rows that fit")


# ---- the step ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rr.STEP_CASES, ids=lambda c: c[0])
def test_three_chained_steps_with_resample(case):
    from deep_fluids_amd import ops
    from test_liquid_resample_host import initial_step_state
    name, shape, gf, alpha = case
    D = len(shape)
    minp = rr.STEP_MIN_P[D]
    pos0, pvel0, es0, vel0 = initial_step_state(shape)
    P = len(pos0)
    parts = [pos0[es0[b]:es0[b + 1]] for b in range(rr.B)]
    # a ragged start through pack_particles; the default capacity of a ragged state is its own storage
    gp, ges = ops.pack_particles([dev(q) for q in parts], capacity=P)
    assert_bits(_np(gp), pos0, "packed positions")
    gu = ops.sample_velocity(dev(vel0), gp, entry_start=ges)
    assert_bits(_np(gu), pvel0, "initial particle velocities")
    gv = dev(vel0)
    rs = ops.Resample(minp)
    kw = dict(accuracy=rr.STEP_ACC, ghost_fluid=gf)
    if alpha is not None:
        kw["viscosity_alpha"] = list(alpha)
    tight = rr.STEP_ACC
    counts0 = np.diff(es0).tolist()
    for t in range(rr.STEP_T):
        state = (_np(gp), _np(gu), _np(ges), _np(gv))
        rk = dict(ghost_fluid=gf, alpha=None if alpha is None else np.asarray(alpha), step_no=t)
        s32 = rr.step(*state, rr.STEP_DT, minp, accuracy=tight, dtype=np.float32, **rk)
        s64 = rr.step(*state, rr.STEP_DT, minp, accuracy=tight * 1e-3, dtype=np.float64, **rk)
        out = ops.liquid_step(gp, gu, gv, rr.STEP_DT, resample=rs, entry_start=ges, **kw)
        assert len(out) == (6 if alpha is not None else 5) and rs.step == t + 1
        gp, gu, gv, iters, ges = out[0], out[1], out[2], out[3], out[-1]
        total = s32["total"]
        # bitwise: counts, entry_start, the ranges of the result, kept and seeded positions
        np.testing.assert_array_equal(_np(ges), s32["entry_start"])
        np.testing.assert_array_equal(s32["cell_start"], s64["cell_start"])
        _, gcs, _ = ops.particle_cells(gp, shape, entry_start=ges)
        np.testing.assert_array_equal(_np(gcs), s32["cell_start"])
        assert_bits(_np(gp)[:total], s32["pos"], "positions after step %d" % (t + 1))
        e32 = [ref.max_err(s32[k], s64[k]) for k in ("vel", "pvel")]
        eg = [ref.max_err(_np(gv), s64["vel"]), ref.max_err(_np(gu)[:total], s64["pvel"])]
        et = [ref.max_err(_np(gv), s32["vel"]), ref.max_err(_np(gu)[:total], s32["pvel"])]
        r = s32["resampled"]
        print("%s step %d: iterations %s  live %d -> %d (%d seeds, %d dropped)  vel/pvel twin-vs-fp64 %.3e %.3e  gpu-vs-fp64 %.3e %.3e  gpu-vs-twin %.3e %.3e"
              % ((name, t + 1, _np(iters).tolist(), int(r["old_cell_start"][-1]), total, int(r["seeds"].sum()),
                  int((r["keep"][:r["old_cell_start"][-1]] == 0).sum())) + tuple(e32) + tuple(eg) + tuple(et)))
        for k in range(2):
            # the margin of test_gpu_liquid.test_four_steps_of_a_drop_falling_into_a_basin: 3 over the twin's own error on these inputs
            # plus the two solves' accuracy (2e-6 * 12 = 2.4e-05 here).  Measured on the MI355X, worst over the five cases and three
            # steps: twin-vs-fp64 5.02e-07 (vel), 6.06e-07 (pvel); gpu-vs-fp64 5.02e-07, 6.06e-07; gpu-vs-twin 1.19e-07, 1.79e-07
            assert eg[k] <= 3 * e32[k] + 2 * tight * max(shape), (k, eg[k], e32[k])
            assert et[k] <= 3 * e32[k] + 2 * tight * max(shape), (k, et[k], e32[k])
        # the invariants, on the GPU's own positions and ranges (the keep bytes are internal to the step: the twin's, equal by the above)
        g = dict(r, pos=_np(gp)[:total], pvel=_np(gu)[:total], entry_start=_np(ges), cell_start=_np(gcs))
        rr.check_invariants(g, s32["phi"], s32["liquid"], minp, 2 * minp)
    assert np.diff(_np(ges)).tolist() != counts0                          # the counts moved: the state is ragged for real
    # a dense [B,N,D] start is packed internally, and simulate_liquid chains the same steps with the counter advancing
    if D == 2 and alpha is None:
        n = min(len(q) for q in parts)
        dense = np.stack([q[:n] for q in parts])
        dp, dv = dev(dense), dev(vel0)
        du = ops.sample_velocity(dv, dp)
        a = ops.liquid_step(dp, du, dv, rr.STEP_DT, resample=ops.Resample(minp), **kw)
        fp, fes = ops.pack_particles([dp[b] for b in range(rr.B)], capacity=2 * rr.B * n)
        fu, _ = ops.pack_particles([du[b] for b in range(rr.B)], capacity=2 * rr.B * n)
        b = ops.liquid_step(fp, fu, dv, rr.STEP_DT, resample=ops.Resample(minp), entry_start=fes, **kw)
        live = int(_np(a[-1])[-1])
        assert tuple(a[0].shape) == (2 * rr.B * n, D) and torch.equal(a[-1], b[-1]) and torch.equal(a[0][:live], b[0][:live])
        assert torch.equal(a[1][:live], b[1][:live]) and torch.equal(a[2], b[2])
        sp, su, vels, ses = ops.simulate_liquid(dp, du, dv, 2, dt=rr.STEP_DT, resample=ops.Resample(minp), **kw)
        rs2 = ops.Resample(minp)
        c = ops.liquid_step(dp, du, dv, rr.STEP_DT, resample=rs2, **kw)
        c2 = ops.liquid_step(c[0], c[1], c[2], rr.STEP_DT, resample=rs2, entry_start=c[-1], **kw)
        assert torch.equal(vels[0], c[2]) and torch.equal(vels[1], c2[2]) and torch.equal(ses, c2[-1])
        # a capacity that does not hold the result: refused before the step returns
        from deep_fluids_amd import _lib
        with pytest.raises(_lib.DeepFluidsHipError, match="capacity of at least"):
            ops.liquid_step(dp, du, dv, rr.STEP_DT, resample=ops.Resample(minp, capacity=rr.B * n), **kw)


def _composed_dense_step(ops, p, u, v, shape, ghost_fluid=False, viscosity_alpha=None):
    """the dense step put together from the public functions, in the order the ``liquid_step`` docstring gives"""
    B, n, D = p.shape
    moved = ops.advect_particles(p, v, rr.STEP_DT, bnd=rr.BND)
    spos, cell_start, order = ops.particle_cells(moved, shape)
    su = torch.empty_like(u)
    ops.call("df_particles_gather", ops._ptr(u), ops._ptr(order), ops._ptr(su), B * n, D, ops._stream())
    vel_old, _, known = ops.particles_to_grid(spos, su, cell_start, shape)
    vel, _ = ops.extrapolate_mac(vel_old, known, 2, bnd=rr.BND)
    flags, touch = ops.liquid_flags(cell_start, shape, B, n, bnd=rr.BND)
    solve = dict()
    if ghost_fluid:
        solve = dict(phi=ops.particle_levelset_averaged(spos, shape, 1.0, 1, 1, 1.0, rr.BND, cells=(spos, cell_start)), gf_clamp=1e-4)
    diters = ()
    if viscosity_alpha is not None:
        vel = ops.liquid_forces(vel, flags, (0.0,) * D, bnd=rr.BND)
        vel, it = ops.diffuse_velocity(vel, viscosity_alpha, bnd=rr.BND, accuracy=1e-4, max_iter=ops.default_diffusion_max_iter(shape))
        diters = (it,)
    vel = ops.liquid_forces(vel, flags, ops.default_gravity_force(shape, rr.STEP_DT), bnd=rr.BND)
    vel, _, iters = ops.solve_pressure_liquid(vel, flags, bnd=rr.BND, **solve)
    vel, _ = ops.extrapolate_mac(vel, touch, 4, bnd=rr.BND)
    return (spos, ops.flip_update(spos, su, vel, vel_old), vel, iters) + diters


@pytest.mark.parametrize("shape", rr.SHAPES)
def test_resample_none_keeps_the_dense_step(shape):
    """the off switch: with resample=None the step and the simulation return the bits of the dense step as its docstring composes it
    from the public functions, taken in the same run"""
    from deep_fluids_amd import ops
    parts, vel0 = rr.step_scene(shape)
    n = min(len(q) for q in parts)
    p, v = dev(np.stack([q[:n] for q in parts])), dev(vel0)
    u = ops.sample_velocity(v, p)
    names = []
    real = ops.call
    try:
        ops.call = lambda name, *a: (names.append(name), real(name, *a))[1]
        for kw in (dict(), dict(ghost_fluid=True), dict(viscosity_alpha=0.3)):
            want = _composed_dense_step(ops, p, u, v, shape, **kw)
            got = ops.liquid_step(p, u, v, rr.STEP_DT, resample=None, **kw)
            assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
            sim = ops.simulate_liquid(p, u, v, 2, dt=rr.STEP_DT, resample=None, **kw)
            nxt = ops.liquid_step(got[0], got[1], got[2], rr.STEP_DT, **kw)
            assert len(sim) == 3 and torch.equal(sim[2][0], got[2]) and torch.equal(sim[2][1], nxt[2]) and torch.equal(sim[0], nxt[0])
    finally:
        ops.call = real
    assert names and not [x for x in names if "ragged" in x or "resample" in x or "levelset_extrapolate" in x], sorted(set(names))
