"""GPU side of the liquid solver step (liquid.hip and the `_liquid` pressure entry points of smoke.hip) against tests/liquid_ref.py.

Particles to grid, extrapolation, flags, forces and the FLIP update are compared BITWISE with the fp32 twin, which performs the same
operations in the same order.  The pressure solve cannot be bitwise: its dot products are summed in workgroup order on the GPU and by
NumPy's pairwise sum in the twin, so it is bounded through `accuracy` as tests/test_gpu_smoke.py does, and the chained step by a stated
margin over the twin's own distance from fp64.  Every parity test prints its figures before it asserts.

Shapes: (7,9) and (5,7,6) are odd on every axis, (16,12) with bnd 2 has a two-cell band, B = 2 puts two entries into one launch whose
particles differ.
Loose alignments, guarded buffers, the block remap's remainder and the documented hostile inputs: tests/test_gpu_particle_edges.py."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import liquid_ref as ref
import particles_ref as pref
from gpu_util import assert_bits, dev
from smoke_ref import interior_mask
import smoke_ref as sref

pytestmark = pytest.mark.gpu

#        shape        B  bnd
CASES = [((7, 9), 2, 1), ((16, 12), 1, 2), ((5, 7, 6), 2, 1)]


def _np(t):
    return t.cpu().numpy()


def _u8(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def particle_set(shape, B, N, bnd, seed):
    """[B,N,D] positions and velocities: the rows of particles_ref.special_positions (both clamp limits on every axis, band cells), a crowd of 70 in
    one cell, the rest in the lower-index 60 % of the grid, so that the upper cells are empty.  The LAST entry's bulk is shifted."""
    rng = np.random.RandomState(seed)
    D = len(shape)
    ext = np.array(shape[::-1], np.float64)
    lo, hi = pref.clamp_bounds(shape, bnd, np.float32)
    p = (lo + rng.uniform(0, 1, size=(B, N, D)) * (0.6 * (hi - lo))).astype(np.float32)
    sp = pref.special_positions(shape, bnd)              # with positions inside the band: the edge rules of the weights
    p[:, :len(sp)] = sp
    cell = np.floor(0.5 * ext)
    p[:, len(sp):len(sp) + 70] = (cell + rng.uniform(0.01, 0.99, size=(B, 70, D))).astype(np.float32)
    if B > 1:
        p[-1, len(sp) + 70:] += np.float32(0.3)
    u = rng.uniform(-1.5, 1.5, size=p.shape).astype(np.float32)
    return p, u


def _sorted_on_gpu(pos, pvel, shape):
    from deep_fluids_amd import ops
    p, u = dev(pos), dev(pvel)
    spos, cell_start, order = ops.particle_cells(p, shape)
    su = u.reshape(-1, u.shape[-1])[order].reshape(u.shape).contiguous()
    return spos, su, cell_start


# ---- the kernels against the op-for-op twin, bitwise --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,B,bnd", CASES)
def test_p2g_flags_forces_bitwise(shape, B, bnd):
    from deep_fluids_amd import ops
    D = len(shape)
    pos, pvel = particle_set(shape, B, 400, bnd, 21)
    rp, ru, rcs, _ = ref.sort_particles(pos, pvel, shape)
    spos, su, cs = _sorted_on_gpu(pos, pvel, shape)
    assert_bits(_np(spos), rp, "sorted positions")
    assert_bits(_np(su), ru, "sorted velocities")
    np.testing.assert_array_equal(_np(cs), rcs)
    counts = np.diff(rcs)
    assert counts.max() > 64 and (counts == 0).any()
    want_v, want_w, want_k = ref.p2g(rp, ru, rcs, shape, np.float32)
    vel, weight, known = ops.particles_to_grid(spos, su, cs, shape)
    assert_bits(_np(weight), want_w, "weight")
    assert_bits(_np(vel), want_v, "velocity")
    np.testing.assert_array_equal(_np(known), want_k)
    v64, w64, _ = ref.p2g(rp, ru, rcs, shape, np.float64)
    print("%s: p2g twin-vs-fp64 %.3e (velocity), %.3e (weight); max particles per cell %d" %
          (shape, ref.max_err(want_v, v64), ref.max_err(want_w, w64), int(counts.max())))
    # flags: liquid where a range is not empty and the cell is interior
    liquid = ref.liquid_mask(rcs, B, shape, bnd)
    wf, wt = ref.flags_of(liquid)
    flags, touch = ops.liquid_flags(cs, shape, B, 400, bnd=bnd)
    np.testing.assert_array_equal(_np(flags), wf)
    np.testing.assert_array_equal(_np(touch), wt)
    assert liquid.any() and (~liquid & interior_mask(shape, bnd)[None]).any()
    # forces
    force = (0.013, -0.256, 0.07)[:D]
    rng = np.random.RandomState(1)
    v0 = rng.standard_normal((B,) + shape + (D,)).astype(np.float32)
    got = ops.liquid_forces(dev(v0), flags, force, bnd=bnd)
    assert_bits(_np(got), ref.forces(v0, liquid, force, bnd, np.float32), "forces")
    for a in range(D):
        assert not _np(got)[..., a][:, ~ref.both_interior(shape, bnd, a)].any()
    vi = dev(v0)
    assert ops.liquid_forces(vi, flags, force, bnd=bnd, out=vi) is vi and torch.equal(vi, got)
    # two runs, and entry b alone: bit for bit
    vel2, weight2, _ = ops.particles_to_grid(spos, su, cs, shape)
    assert torch.equal(vel2, vel) and torch.equal(weight2, weight)
    for e in range(B):
        s1, u1, c1 = _sorted_on_gpu(pos[e:e + 1], pvel[e:e + 1], shape)
        v1, w1, _ = ops.particles_to_grid(s1, u1, c1, shape)
        assert_bits(_np(v1)[0], _np(vel)[e], "entry %d alone" % e)
        assert_bits(_np(w1)[0], _np(weight)[e], "entry %d alone" % e)
        f1, _ = ops.liquid_flags(c1, shape, 1, 400, bnd=bnd)
        np.testing.assert_array_equal(_np(f1)[0], wf[e])


@pytest.mark.parametrize("shape", [(7, 9), (5, 7, 6)])
def test_no_particles_all_air_and_all_liquid_entries(shape):
    from deep_fluids_amd import ops
    D = len(shape)
    # N = 0: zeros, all air
    p0 = torch.empty((2, 0, D), device="cuda")
    spos, cs, order = ops.particle_cells(p0, shape)
    vel, weight, known = ops.particles_to_grid(spos, torch.empty_like(spos), cs, shape)
    flags, touch = ops.liquid_flags(cs, shape, 2, 0)
    assert not vel.any() and not weight.any() and not known.any() and not flags.any() and not touch.any()
    assert tuple(ops.flip_update(p0, p0, vel, vel).shape) == (2, 0, D)
    # entry 0: one particle in every interior cell (liquid touching no air); entry 1: all its particles in ONE band cell (all air)
    inter = interior_mask(shape, 1)
    cells = np.argwhere(inter)[:, ::-1].astype(np.float32) + np.float32(0.5)
    pos = np.stack([cells, np.full_like(cells, 0.5)])
    pvel = np.random.RandomState(2).uniform(-1, 1, pos.shape).astype(np.float32)
    rp, ru, rcs, _ = ref.sort_particles(pos, pvel, shape)
    spos, su, cs = _sorted_on_gpu(pos, pvel, shape)
    flags, _ = ops.liquid_flags(cs, shape, 2, pos.shape[1])
    liquid = ref.liquid_mask(rcs, 2, shape, 1)
    assert (liquid[0] == inter).all() and not liquid[1].any()
    np.testing.assert_array_equal(_np(flags), ref.flags_of(liquid)[0])
    vel, weight, _ = ops.particles_to_grid(spos, su, cs, shape)
    wv, ww, _ = ref.p2g(rp, ru, rcs, shape, np.float32)
    assert_bits(_np(vel), wv, "velocity")
    assert_bits(_np(weight), ww, "weight")
    # the projection: the all-air entry is left alone but for its wall faces, the all-liquid one is the closed box's, bit for bit
    w = sref.walled(sref.make_velocity(shape, B=2, seed=4, vmax=1.0), 1)
    v, p, iters = ops.solve_pressure_liquid(dev(w), flags)
    vc, pc, ic = ops.solve_pressure(dev(w[:1]))
    assert_bits(_np(p)[0], _np(pc)[0], "all-liquid pressure == closed box")
    assert_bits(_np(v)[0], _np(vc)[0], "all-liquid velocity == closed box")
    assert int(iters[0]) == int(ic[0]) > 0 and int(iters[1]) == 0
    assert_bits(_np(v)[1], w[1], "all-air entry")
    assert not _np(p)[1].any()


@pytest.mark.parametrize("shape,B,bnd", CASES)
@pytest.mark.parametrize("distance", [0, 1, 2, 4])
def test_extrapolate_bitwise(shape, B, bnd, distance):
    from deep_fluids_amd import ops
    D = len(shape)
    rng = np.random.RandomState(distance)
    v = rng.standard_normal((B,) + shape + (D,)).astype(np.float32)
    m = (rng.uniform(size=v.shape) < 0.12).astype(np.uint8)
    # entry 0: a single known face; component 1 of it has none at all
    m[0] = 0
    m[0][tuple(n // 2 for n in shape) + (0,)] = 1
    want_v, want_m = ref.extrapolate(v, m, distance, bnd, np.float32)
    tv, tm = dev(v), _u8(m)
    got_v, got_m = ops.extrapolate_mac(tv, tm, distance, bnd=bnd)
    assert_bits(_np(got_v), want_v, "values")
    np.testing.assert_array_equal(_np(got_m), want_m)
    assert_bits(_np(tv), v, "input untouched")
    assert got_v.data_ptr() != tv.data_ptr()
    assert int(got_m.max()) <= distance + 1 and not _np(got_m)[0, ..., 1].any()
    for a in range(D):
        wall = ~ref.both_interior(shape, bnd, a)
        assert_bits(_np(got_v)[..., a][:, wall], v[..., a][:, wall], "wall faces are never filled")
        np.testing.assert_array_equal(_np(got_m)[..., a][:, wall], m[..., a][:, wall])
    # zero velocities with known wall faces: wall faces stay 0
    z, zm = ops.extrapolate_mac(dev(np.zeros_like(v)), tm, distance, bnd=bnd)
    assert not z.any()
    e = 1 if B > 1 else 0
    one_v, one_m = ops.extrapolate_mac(dev(v[e:e + 1]), _u8(m[e:e + 1]), distance, bnd=bnd)
    assert_bits(_np(one_v)[0], _np(got_v)[e], "entry alone")


@pytest.mark.parametrize("shape,B,bnd", CASES)
def test_flip_update_bitwise(shape, B, bnd):
    from deep_fluids_amd import ops
    D = len(shape)
    pos, pvel = particle_set(shape, B, 300, bnd, 5)
    vel = sref.make_velocity(shape, B=B, seed=8, vmax=2.0)
    old = sref.make_velocity(shape, B=B, seed=9, vmax=2.0)
    for flip in (0.97, 0.0, 1.0):
        want = ref.flip_update(pos, pvel, vel, old, flip, np.float32)
        got = ops.flip_update(dev(pos), dev(pvel), dev(vel), dev(old), flip_ratio=flip)
        assert_bits(_np(got), want, "flip %.2f" % flip)
    w64 = ref.flip_update(pos, pvel, vel, old, 0.97, np.float64)
    print("%s: flip update twin-vs-fp64 %.3e" % (shape, ref.max_err(ref.flip_update(pos, pvel, vel, old, 0.97, np.float32), w64)))
    assert_bits(_np(ops.sample_velocity(dev(vel), dev(pos))), ref.sample(vel, pos, np.float32), "sample")
    u = dev(pvel)
    assert ops.flip_update(dev(pos), u, dev(vel), dev(old), out=u) is u
    assert_bits(_np(u), ref.flip_update(pos, pvel, vel, old, 0.97, np.float32), "in place")
    one = ops.flip_update(dev(pos[-1:]), dev(pvel[-1:]), dev(vel[-1:]), dev(old[-1:]))
    assert_bits(_np(one)[0], ref.flip_update(pos, pvel, vel, old, 0.97, np.float32)[-1], "entry alone")


# ---- the free-surface projection ------------------------------------------------------------------------------------------------------------
def _ragged(shape, B, seed):
    rng = np.random.RandomState(seed)
    liquid = (rng.uniform(size=(B,) + shape) < 0.7) & interior_mask(shape, 1)[None]
    D = len(shape)
    vel = ref.forces(rng.standard_normal((B,) + shape + (D,)), liquid, (0.0, -0.25, 0.0)[:D], 1, np.float32)
    return liquid, vel.astype(np.float32)


@pytest.mark.parametrize("shape", [(8, 8), (6, 6, 6)])
def test_projection_against_the_dense_solve(shape):
    from deep_fluids_amd import ops
    D = len(shape)
    liquid, w = _ragged(shape, 2, 3)
    flags = _u8(ref.flags_of(liquid)[0])
    acc = 1e-4
    max_iter = ops.default_max_iter(shape)
    b64 = ref.rhs(w, liquid, np.float64)
    v, p, iters = ops.solve_pressure_liquid(dev(w), flags, accuracy=acc)
    x32, it32, r32 = ref.cg(w, liquid, 1, acc, max_iter, np.float32)
    # as in tests/test_gpu_smoke.py: |b - A p| <= |r| + |(b - A p) - r| <= accuracy + the recurrence's drift, measured on the twin in fp64
    excess = float(np.abs((b64 - ref.apply_A(x32.astype(np.float64), liquid, 1)) - r32).max())
    res = float(np.abs(b64 - ref.apply_A(_np(p).astype(np.float64), liquid, 1)).max())
    print("%s: iterations gpu %s twin %s  fp64 residual of the gpu's p %.4e (bound %.1e + twin's excess %.3e)" %
          (shape, _np(iters).tolist(), it32.tolist(), res, acc, excess))
    assert (_np(iters) > 0).all() and (_np(iters) < max_iter).all()
    assert res <= acc + excess
    assert not _np(p)[~liquid].any()
    vex, _ = ref.exact_projection(w, liquid, 1)
    v32 = ref.correct(w, x32, liquid, 1, np.float32)
    d32 = float(np.abs(v32 - vex).max())
    dg = float(np.abs(_np(v) - vex).max())
    print("%s: distance from the exact fp64 projection: twin %.3e  gpu %.3e" % (shape, d32, dg))
    assert dg <= 3 * d32
    # liquid-cell divergence after the correction: |div| = |b - A p| up to the rounding of the correction, the same rule
    div = float(np.abs(ref.divergence(_np(v), liquid)).max())
    print("%s: max |div| over liquid cells %.3e" % (shape, div))
    assert div <= acc + excess + (2 * D) * 2.0 ** -22 * float(np.abs(w).max() + 2 * np.abs(_np(p)).max())
    for a in range(D):
        live, kept = ref.live_face(liquid, 1, a), ref.both_interior(shape, 1, a)[None]
        assert_bits(_np(v)[..., a][kept & ~live], w[..., a][kept & ~live], "faces without a liquid cell are copied")
        assert not _np(v)[..., a][np.broadcast_to(~kept, live.shape)].any()
    # determinism, batch invariance, check_every, the workspace is written before it is read, in place
    ws = ops.pressure_workspace(dev(w))
    ws.fill_(float("nan"))
    v2, p2, i2 = ops.solve_pressure_liquid(dev(w), flags, accuracy=acc, workspace=ws, check_every=3)
    assert torch.equal(v2, v) and torch.equal(p2, p) and torch.equal(i2, iters)
    for e in range(2):
        ve, pe, ie = ops.solve_pressure_liquid(dev(w[e:e + 1]), flags[e:e + 1].contiguous(), accuracy=acc)
        assert_bits(_np(pe)[0], _np(p)[e], "pressure of entry %d alone" % e)
        assert_bits(_np(ve)[0], _np(v)[e], "velocity of entry %d alone" % e)
    vi = dev(w)
    assert ops.solve_pressure_liquid(vi, flags, accuracy=acc, out=vi)[0] is vi and torch.equal(vi, v)


# ---- the chained step -----------------------------------------------------------------------------------------------------------------------------
def drop_scene(shape, seeds, drop_x=(0.35, 0.6)):
    """a drop above a basin, one batch entry per drop position: (pos [B,N,D], vel0 [B,..,D]) float32, equal N by construction of the
    drop radius; None if the seeded counts differ"""
    from deep_fluids_amd import ops
    D = len(shape)
    ext = np.array(shape[::-1], np.float64)
    pos, vel = [], []
    for n, fx in enumerate(drop_x):
        hi = ext.copy()
        hi[1] = 0.3 * ext[1]
        c = 0.5 * ext
        c[0] = np.floor(fx * ext[0]) + 0.5
        c[1] = np.floor(0.65 * ext[1]) + 0.5
        phi = np.minimum(ops.box_levelset(shape, np.zeros(D), hi), ops.sphere_levelset(shape, c, 0.13 * ext[0]))
        pos.append(ops.seed_particles(phi, seed=seeds[n]))
        vel.append(ref.initial_velocity(shape, [(c, 0.13 * ext[0] + 1.0)]))
    assert len(set(len(p) for p in pos)) == 1, [len(p) for p in pos]
    return np.stack(pos), np.stack(vel)


# seeds of the jitter, chosen on the CPU so that on all 4 steps the fp32 twin and the fp64 run sort every particle into the same cell
STEP_SEEDS = {(12, 16): (123, 124), (8, 10, 8): (123, 124)}


@pytest.mark.parametrize("shape", [(12, 16), (8, 10, 8)])
def test_four_steps_of_a_drop_falling_into_a_basin(shape):
    from deep_fluids_amd import ops
    pos0, vel0 = drop_scene(shape, STEP_SEEDS[shape])
    dt, tight, T = 0.5, 1e-6, 4
    pvel0 = ref.sample(vel0, pos0, np.float32)
    s64 = dict(pos=pos0.astype(np.float64), pvel=pvel0.astype(np.float64), vel=vel0.astype(np.float64))
    s32 = dict(pos=pos0, pvel=pvel0, vel=vel0)
    p, u, v = dev(pos0), ops.sample_velocity(dev(vel0), dev(pos0)), dev(vel0)
    assert_bits(_np(u), pvel0, "initial particle velocities")
    stats = []
    _, _, vels = ops.simulate_liquid(p, u, v, T, dt=dt, accuracy=tight, stats=stats)
    for t in range(T):
        # the solve is only accurate to its `accuracy`: fp64 and fp32 are compared at an accuracy both reach, as the smoke step is
        s64 = ref.step(s64["pos"], s64["pvel"], s64["vel"], dt, accuracy=tight * 1e-3, dtype=np.float64)
        s32 = ref.step(s32["pos"], s32["pvel"], s32["vel"], dt, accuracy=tight, dtype=np.float32)
        p, u, v, iters = ops.liquid_step(p, u, v, dt, accuracy=tight)
        assert torch.equal(v, vels[t]) and torch.equal(iters, stats[t])
        # the identity the comparison rests on: the same particles in the same cells, in all three runs
        np.testing.assert_array_equal(s32["cell_start"], s64["cell_start"])
        _, gcs, _ = ops.particle_cells(p, shape)
        np.testing.assert_array_equal(_np(gcs), s64["cell_start"])
        assert (s32["liquid"] == s64["liquid"]).all()
        e32 = [ref.max_err(s32[k], s64[k]) for k in ("vel", "pos", "pvel")]
        eg = [ref.max_err(_np(x), s64[k]) for x, k in ((v, "vel"), (p, "pos"), (u, "pvel"))]
        et = [ref.max_err(_np(x), s32[k]) for x, k in ((v, "vel"), (p, "pos"), (u, "pvel"))]
        print("%s step %d: iterations %s  liquid cells %s  vel/pos/pvel twin-vs-fp64 %.3e %.3e %.3e  gpu-vs-fp64 %.3e %.3e %.3e  gpu-vs-twin %.3e %.3e %.3e"
              % ((shape, t + 1, _np(iters).tolist(), s64["liquid"].reshape(2, -1).sum(1).tolist()) + tuple(e32) + tuple(eg) + tuple(et)))
        div = float(np.abs(ref.divergence(_np(v), s64["liquid"])).max())
        for k in range(3):
            # margin 3 over the twin's own error on these inputs plus the two solves' accuracy (both stop at max|r| <= 1e-6, anywhere below)
            assert eg[k] <= 3 * e32[k] + 2 * tight * max(shape), (k, eg[k], e32[k])
            assert et[k] <= 3 * e32[k] + 2 * tight * max(shape), (k, et[k], e32[k])
    assert float(np.abs(_np(v)).max()) > 0.1 and float(_np(p)[..., 1].mean()) < float(pos0[..., 1].mean())      # it falls
    # entry 1 alone, and a second run: bit for bit
    p1, u1, v1 = dev(pos0[1:]), dev(pvel0[1:]), dev(vel0[1:])
    _, _, one = ops.simulate_liquid(p1, u1, v1, T, dt=dt, accuracy=tight)
    assert_bits(_np(one)[:, 0], _np(vels)[:, 1], "entry 1 alone")
    frames = list(ops.simulate_liquid(dev(pos0), dev(pvel0), dev(vel0), 2, dt=dt, accuracy=tight, stack=False))
    assert len(frames) == 2 and torch.equal(frames[-1][2], vels[1])


@pytest.mark.parametrize("shape", [(12, 16), (8, 10, 8)])
def test_hydrostatic_rest_over_ten_steps(shape):
    from deep_fluids_amd import ops
    D = len(shape)
    ext = np.array(shape[::-1], np.float64)
    hi = ext.copy()
    hi[1] = float(shape[-2] // 2)
    phi = ops.box_levelset(shape, np.zeros(D), hi)
    p, u, v = ops.liquid_initial_state(shape, phi, randomness=0.0)
    assert not u.any() and not v.any() and p.shape[1] == int((phi < 0)[interior_mask(shape, 1)].sum()) * 2 ** D
    acc, dt = 1e-6, 0.5
    force = ops.default_gravity_force(shape, dt)
    # what the fp64 restatement leaves after ONE force + projection at this accuracy: the pressure error across a face
    liquid = ((phi < 0) & interior_mask(shape, 1))[None]
    out64, _, _ = ref.solve_pressure(ref.forces(np.zeros((1,) + shape + (D,)), liquid, force, 1), liquid, 1, acc, None, np.float64)
    rest64 = float(np.abs(out64).max())
    worst = 0.0
    for t in range(10):
        p, u, v, iters = ops.liquid_step(p, u, v, dt, force=force, accuracy=acc)
        worst = max(worst, float(v.abs().max()))
    print("%s: max |vel| over 10 steps %.3e (fp64 restatement, one step: %.3e; |force| %.3e)" % (shape, worst, rest64, abs(force[1])))
    # margin: each step adds at most what one projection leaves (2 * acc across a face bounds it: two cell pressures, each within the
    # residual bound times the column depth), FLIP carries 0.97 of it on: a geometric sum below 1 / 0.03 of a step's share
    assert worst <= max(rest64, 2 * acc * shape[-2]) / 0.03


# ---- the C-ABI's error rules ------------------------------------------------------------------------------------------------------------------
def test_cabi_error_paths():
    """One case per rule of the header; every one is answered on the host (the pointers are not device memory, so a launch would fault)."""
    from deep_fluids_amd import _lib
    h = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    a = (ctypes.addressof(buf) + 15) & ~15
    b, c, d, e, f = a + 4096, a + 8192, a + 12288, a + 16384, a + 20480
    # null
    assert h.df_liquid_p2g2d(None, b, c, d, e, None, 1, 4, 8, 8, None) == -1 and b"null positions" in h.df_last_error()
    assert h.df_liquid_p2g3d(a, b, c, None, e, None, 1, 4, 8, 8, 8, None) == -1 and b"null velocity" in h.df_last_error()
    assert h.df_mac_extrapolate2d(a, None, c, d, 1, 8, 8, 1, 1, None) == -1 and b"null marks" in h.df_last_error()
    assert h.df_liquid_flags3d(a, None, None, 1, 4, 8, 8, 8, 1, None) == -1 and b"null flags" in h.df_last_error()
    assert h.df_liquid_forces2d(a, None, c, 1, 8, 8, 0.0, 0.0, 1, None) == -1
    assert h.df_flip_update2d(None, b, c, d, e, 1, 4, 8, 8, 0.97, None) == -1
    assert h.df_pressure_cg_direction2d_liquid(a, 1 << 20, None, 1, 8, 8, 1, 0, 1e-4, 10, None) == -1 and b"null flags" in h.df_last_error()
    assert h.df_pressure_correct3d_liquid(a, b, c, None, 1, 8, 8, 8, 1, None) == -1
    # values
    assert h.df_mac_extrapolate2d(a, b, c, d, 1, 8, 8, 1, 0, None) == -1 and b"layer" in h.df_last_error()
    assert h.df_mac_extrapolate3d(a, b, c, d, 1, 8, 8, 8, 0, 1, None) == -1 and b"boundary width" in h.df_last_error()
    assert h.df_flip_update3d(a, b, c, d, e, 1, 4, 8, 8, 8, 1.5, None) == -1 and b"flip_ratio" in h.df_last_error()
    assert h.df_liquid_p2g2d(a, b, c, d, e, None, 1, -1, 8, 8, None) == -1
    # extents
    assert h.df_liquid_forces2d(a, b, c, 1, 8, 5, 0.0, 0.0, 2, None) == -2 and b"2*bnd + 2" in h.df_last_error()
    assert h.df_liquid_flags2d(a, b, None, 1, 4, 8, 3, 1, None) == -2
    assert h.df_liquid_p2g3d(a, b, c, d, e, None, 2, 4, 1 << 10, 1 << 10, 1 << 10, None) == -2 and b"int32" in h.df_last_error()
    assert h.df_flip_update2d(a, b, c, d, e, 1 << 20, 1 << 20, 8, 8, 0.97, None) == -2 and b"int32" in h.df_last_error()
    # alignment
    assert h.df_liquid_p2g2d(a + 2, b, c, d, e, None, 1, 4, 8, 8, None) == -3
    assert h.df_mac_extrapolate2d(a, b, c + 2, d, 1, 8, 8, 1, 1, None) == -3
    assert h.df_liquid_flags2d(a + 2, b, None, 1, 4, 8, 8, 1, None) == -3
    assert h.df_liquid_forces3d(a, b, c + 1, 1, 8, 8, 8, 0.0, 0.0, 0.0, 1, None) == -3
    assert h.df_flip_update2d(a, b + 2, c, d, e, 1, 4, 8, 8, 0.97, None) == -3
    # aliasing of what a launch gathers from
    assert h.df_mac_extrapolate2d(a, b, a, d, 1, 8, 8, 1, 1, None) == -1 and b"must not be the input" in h.df_last_error()
    assert h.df_mac_extrapolate2d(a, b, c, b, 1, 8, 8, 1, 1, None) == -1
    assert h.df_mac_extrapolate2d(a, b, c, a + 16, 1, 8, 8, 1, 1, None) == -1 and b"overlap" in h.df_last_error()
    assert h.df_liquid_p2g2d(a, b, c, d, d, None, 1, 4, 8, 8, None) == -1
    assert h.df_liquid_p2g2d(a, b, c, d, e, d + 8, 1, 4, 8, 8, None) == -1 and b"overlap" in h.df_last_error()
    assert h.df_liquid_flags2d(a, a + 8, None, 1, 4, 8, 8, 1, None) == -1 and b"overlap" in h.df_last_error()
    assert h.df_liquid_forces2d(a, c + 8, c, 1, 8, 8, 0.0, 0.0, 1, None) == -1 and b"overlap" in h.df_last_error()
    assert h.df_flip_update2d(a, b, a, d, e, 1, 4, 8, 8, 0.97, None) == -1
    assert h.df_pressure_correct2d_liquid(a, b, b, f, 1, 8, 8, 1, None) == -1
    # workspace size
    need = h.df_pressure_workspace_bytes(1, 1, 8, 8)
    assert h.df_pressure_cg_direction2d_liquid(a, need - 4, f + 8192, 1, 8, 8, 1, 0, 1e-4, 10, None) == -4
    assert h.df_pressure_cg_direction3d_liquid(a, 16, f, 1, 8, 8, 8, 1, 0, 1e-4, 10, None) == -4
    # N = 0 launches nothing: null particle arrays are fine for the particle-indexed kernel
    assert h.df_flip_update2d(None, None, None, d, e, 1, 0, 8, 8, 0.97, None) == 0
    torch.cuda.synchronize()                                                                  # nothing was enqueued, nothing faults


# ---- the datasets -----------------------------------------------------------------------------------------------------------------------------
def _check_dataset(root, n0, n1, T, xshape, params):
    assert sorted(os.listdir(os.path.join(root, "v"))) == sorted("%d_%d_%d.npz" % (i, j, t) for i in range(n0) for j in range(n1) for t in range(T))
    lo, hi = np.inf, -np.inf
    for i in range(n0):
        for j in range(n1):
            for t in range(T):
                with np.load(os.path.join(root, "v", "%d_%d_%d.npz" % (i, j, t))) as f:
                    assert sorted(f.files) == ["x", "y"]
                    x, y = f["x"], f["y"]
                assert x.dtype == np.float32 and x.shape == xshape
                np.testing.assert_array_equal(y, list(params(i, j)) + [t])
                lo, hi = min(lo, float(x.min())), max(hi, float(x.max()))
    assert open(os.path.join(root, "v_range.txt")).read() == "%.3f\n%.3f" % (lo, hi)
    assert lo < -0.5                                                         # the drop falls
    return dict(line.rstrip("\n").split(": ") for line in open(os.path.join(root, "args.txt")))


def test_generate_liquid_dataset(tmp_path):
    from deep_fluids_amd import ops
    from deep_fluids_amd.data import BatchManager, generate_liquid_dataset
    from deep_fluids_amd.trainer import body_levelset, liquid_pos_size_body
    root = str(tmp_path / "liquid")
    X, Y, T = 16, 12, 3
    n = generate_liquid_dataset(root, num_src_x_pos=2, num_src_radius=2, min_src_x_pos=0.35, max_src_x_pos=0.65, min_src_radius=0.08,
                                max_src_radius=0.12, num_frames=T, resolution_x=X, resolution_y=Y)
    assert n == 2 * 2 * T
    args = _check_dataset(root, 2, 2, T, (Y, X, 2), lambda i, j: (i / 1.0 * (0.65 - 0.35) + 0.35, j / 1.0 * (0.12 - 0.08) + 0.08))
    assert list(args) == ["log_dir", "num_param", "path_format", "p0", "p1", "p2", "num_src_x_pos", "min_src_x_pos", "max_src_x_pos", "src_y_pos",
                          "num_src_radius", "min_src_radius", "max_src_radius", "basin_y_pos", "num_frames", "min_frames", "max_frames",
                          "num_simulations", "resolution_x", "resolution_y", "gravity", "radius_factor", "min_particles", "bWidth",
                          "open_bound", "time_step"]
    assert args["num_src_x_pos"] == "2" and args["max_frames"] == "2" and args["time_step"] == "0.5" and args["open_bound"] == "False"
    cfg = SimpleNamespace(random_seed=1, data_path=root, is_3d=False, data_type="velocity", arch="de", batch_size=5, res_x=X, res_y=Y, res_z=1,
                          num_worker=1)
    bm = BatchManager(cfg, device=None)
    xb, yb = bm.batch()
    bm.stop_thread()
    assert tuple(xb.shape) == (5, Y, X, 2) and tuple(yb.shape) == (5, 3)
    # scene (1, 1) alone, re-simulated from the body the trainer's helper names: the stored frames bit for bit
    body = liquid_pos_size_body(bm, 1, 1)
    px, pr = 1 / 1.0 * (0.65 - 0.35) + 0.35, 1 / 1.0 * (0.12 - 0.08) + 0.08
    assert body["spheres"] == [((px, 0.6), pr)] and body["boxes"] == [((0.0, 0.0), (1.0, 0.2))]
    phi = body_levelset((Y, X), body)
    p, u, v = ops.liquid_initial_state((Y, X), phi, [((X * px, Y * 0.6), X * (pr + 0.05))])
    _, _, vels = ops.simulate_liquid(p, u, v, T, dt=0.5, force=ops.default_gravity_force((Y, X), 0.5))
    for t in range(T):
        with np.load(os.path.join(root, "v", "1_1_%d.npz" % t)) as f:
            assert_bits(_np(vels[t, 0]), f["x"], "frame %d of scene (1, 1)" % t)
    with pytest.raises(NotImplementedError):
        generate_liquid_dataset(str(tmp_path / "open"), open_bound=True)


def test_generate_liquid3_d_r_dataset(tmp_path):
    from deep_fluids_amd import ops
    from deep_fluids_amd.data import BatchManager, generate_liquid3_d_r_dataset
    root = str(tmp_path / "liquid3")
    X, Y, Z, T = 8, 10, 8, 2
    n = generate_liquid3_d_r_dataset(root, num_dist=2, num_rot=1, num_frames=T, resolution_x=X, resolution_y=Y, resolution_z=Z, src_radius=0.15)
    assert n == 2 * 1 * T
    args = _check_dataset(root, 2, 1, T, (Z, Y, X, 3), lambda i, j: (np.linspace(0.15, 0.25, 2)[i], 0.0))
    assert list(args) == ["log_dir", "num_param", "path_format", "p0", "p1", "p2", "min_dist", "max_dist", "num_dist", "min_rot", "max_rot",
                          "num_rot", "src_y_pos", "src_radius", "basin_y_pos", "min_frames", "max_frames", "num_frames", "num_simulations",
                          "resolution_x", "resolution_y", "resolution_z", "gravity", "radius_factor", "min_particles", "bWidth", "open_bound",
                          "time_step"]
    assert args["time_step"] == "0.8" and args["max_frames"] == "1" and args["resolution_z"] == "8"
    cfg = SimpleNamespace(random_seed=1, data_path=root, is_3d=True, data_type="velocity", arch="de", batch_size=3, res_x=X, res_y=Y, res_z=Z,
                          num_worker=1)
    bm = BatchManager(cfg, device=None)
    xb, yb = bm.batch()
    bm.stop_thread()
    assert tuple(xb.shape) == (3, Z, Y, X, 3) and tuple(yb.shape) == (3, 3)
    # scene (1, 0) alone: the stored frames bit for bit
    shape = (Z, Y, X)
    cs = [(X * 0.5 + X * 0.25, Y * 0.6, Z * 0.5), (X * 0.5 + X * 0.25 * np.cos(np.pi), Y * 0.6, Z * 0.5 + X * 0.25 * np.sin(np.pi))]
    phi = ops.box_levelset(shape, (0.0, 0.0, 0.0), (X * 1.0, Y * 0.2, Z * 1.0))
    for c in cs:
        phi = np.minimum(phi, ops.sphere_levelset(shape, c, X * 0.15))
    p, u, v = ops.liquid_initial_state(shape, phi, [(c, X * (0.15 + 0.05)) for c in cs])
    _, _, vels = ops.simulate_liquid(p, u, v, T, dt=0.8, force=ops.default_gravity_force(shape, 0.8))
    for t in range(T):
        with np.load(os.path.join(root, "v", "1_0_%d.npz" % t)) as f:
            assert_bits(_np(vels[t, 0]), f["x"], "frame %d of scene (1, 0)" % t)
    with pytest.raises(NotImplementedError):
        generate_liquid3_d_r_dataset(str(tmp_path / "open"), open_bound=True)
