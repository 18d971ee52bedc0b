"""CPU tests of the restatement of the liquid solver's resampling block (tests/liquid_resample_ref.py): the fp32 twin against fp64, the
invariants of a resampled state, the ragged helpers, and the argument checks of the Python surface and of the C entry points that need
no GPU."""
import ctypes

import numpy as np
import pytest

import liquid_ref as ref
import liquid_resample_ref as rr
import particles_ref as pref


def _resampled(st, dtype, **kw):
    r = rr.resample(st["pos"], st["pvel"], st["cell_start"], st["phi"], st["liquid"], st["vel"], rr.MIN_P, dtype=dtype, **kw)
    r["old_cell_start"] = st["cell_start"]
    return r


@pytest.mark.parametrize("shape", rr.SHAPES)
def test_twin_against_fp64_and_the_invariants(shape):
    st = rr.resample_state(shape)
    r32, r64 = _resampled(st, np.float32), _resampled(st, np.float64)
    for r in (r32, r64):
        rr.check_invariants(r, st["phi"], st["liquid"], rr.MIN_P, 2 * rr.MIN_P)
    assert r32["pos"].dtype == np.float32
    for k in ("keep", "kept", "seeds", "entry_start", "cell_start"):
        np.testing.assert_array_equal(r32[k], r64[k])
    # kept rows are copies; a seed is cell + a 24-bit fraction (half an ulp of the largest extent), its velocity a multilinear sample
    ulp = float(np.spacing(np.float32(max(shape))))
    assert ref.max_err(r32["pos"], r64["pos"]) <= ulp
    assert ref.max_err(r32["pvel"], r64["pvel"]) <= 64 * ulp * float(np.abs(st["vel"]).max())
    # the state holds every case the GPU test relies on
    c, maxp = st["cells"], 2 * rr.MIN_P
    kept, seeds = r32["kept"], r32["seeds"]
    cs = st["cell_start"]
    assert cs[c["deep_crowded"] + 1] - cs[c["deep_crowded"]] == maxp + 3 and kept[c["deep_crowded"]] == maxp + 1
    assert kept[c["surface_crowded"]] == maxp + 3
    assert cs[c["outside"] + 1] - cs[c["outside"]] == 3 and kept[c["outside"]] == 0 and seeds[c["outside"]] == 0
    assert kept[c["deep_single"]] == 1 and seeds[c["deep_single"]] == rr.MIN_P - 1
    assert kept[c["last_column"]] == 1 and seeds[c["last_column"]] == rr.MIN_P - 1
    assert cs[c["emptied"] + 1] - cs[c["emptied"]] == 2 and kept[c["emptied"]] == 0 and seeds[c["emptied"]] == rr.MIN_P
    es = st["entry_start"]
    assert es[2] == es[1] and r32["entry_start"][2] > r32["entry_start"][1]          # the empty entry is filled from nothing
    # seeds lie inside their cell, per axis
    D = len(shape)
    k = rr.keys(r32["pos"], np.concatenate([r32["entry_start"][:-1], [r32["total"]]]), shape)
    np.testing.assert_array_equal(np.searchsorted(k, np.arange(rr.B * int(np.prod(shape)) + 1)), r32["cell_start"])
    # the same (seed, step) twice, another step
    again, other = _resampled(st, np.float32), _resampled(st, np.float32, step=1)
    np.testing.assert_array_equal(again["pos"], r32["pos"])
    sd = r32["seeded"]
    np.testing.assert_array_equal(other["seeded"], sd)
    assert (other["pos"][sd] != r32["pos"][sd]).any() and np.array_equal(other["pos"][~sd], r32["pos"][~sd])


def test_a_seed_that_rounds_up_stays_inside_its_cell():
    """float32(i) + u rounds to i + 1 for the largest 24-bit fraction once i >= 1: the rule puts it on the largest float below i + 1"""
    u = np.float32((2 ** 24 - 1) * 2.0 ** -24)
    for i in (0, 1, 2, 8, 11, 127):
        lo, up = np.float32(i), np.float32(i + 1)
        val = lo + u
        got = val if val < up else np.nextafter(up, np.float32(0))
        assert lo <= got < up and int(got) == i
        assert (val >= up) == (i >= 1)
    assert rr.mix4(123, 0, 5, 1) == rr.mix4(123, 0, 5, 1) != rr.mix4(123, 1, 5, 1)
    hs = np.array([rr.mix4(7, 3, c, m) >> 8 for c in range(64) for m in range(16)])
    assert hs.max() < 2 ** 24 and abs(hs.mean() / 2 ** 24 - 0.5) < 0.05


@pytest.mark.parametrize("shape", rr.SHAPES)
def test_extrapolation_properties(shape):
    phi = rr.pocket_phi(shape, 3)
    inner = np.broadcast_to(ref.interior_mask(shape, 1)[None], phi.shape)
    for inside in (True, False):
        for d in (0, 1):
            np.testing.assert_array_equal(rr.extrapolate_levelset(phi, d, inside, np.float32), phi)
        out, m = rr.extrapolate_levelset(phi, 4, inside, np.float32, marks=True)
        o64 = rr.extrapolate_levelset(phi, 4, inside, np.float64)
        assert ref.max_err(out, o64) <= 8 * float(np.spacing(np.float32(np.abs(o64).max())))
        changed = out != phi
        assert changed.any() and not changed[~inner].any() and not m[~inner].any()
        assert (m[changed] >= 3).all() and not changed[m <= 2].any()
        assert m.max() == 5
    # inside: phi decreases by at most 1 per layer away from the cells that kept their value, and is <= the layer before it
    out, m = rr.extrapolate_levelset(phi, 4, True, np.float64, marks=True)
    for d in (3, 4, 5):
        assert out[m == d].max() < out[m == d - 1].max()
    # all negative: nothing is marked, nothing changes (entry 1)
    np.testing.assert_array_equal(rr.extrapolate_levelset(phi[1:2], 4, True, np.float32), phi[1:2])
    assert not rr.extrapolate_marks(phi[1:2], True).any()


@pytest.mark.parametrize("shape", rr.SHAPES)
def test_ragged_helpers(shape):
    D = len(shape)
    pos, pvel, es, parts, vels = rr.ragged_case(shape, 30, 1)
    assert list(es) == [0, 30, 30, 40] and np.isnan(pos[40:]).all()
    e = rr.entries(es, len(pos))
    assert (e[:30] == 0).all() and (e[30:40] == 2).all() and (e[40:] == -1).all()
    vel = rr.velocity(shape, 2)
    moved = rr.trace(pos, vel, es, 0.5, rr.BND, 1.0, np.float32)
    np.testing.assert_array_equal(moved[:30], pref.trace(parts[0][None], vel[0:1], 0.5, rr.BND, 1.0, np.float32)[0])
    np.testing.assert_array_equal(moved[30:40], pref.trace(parts[2][None], vel[2:3], 0.5, rr.BND, 1.0, np.float32)[0])
    assert np.isnan(moved[40:]).all()
    k = rr.keys(pos, es, shape)
    ncell = int(np.prod(shape))
    assert (k[40:] == rr.B * ncell).all() and (k[:30] < ncell).all() and (k[30:40] >= 2 * ncell).all()
    sp, su, cs, order = rr.sort(pos, pvel, es, shape)
    assert cs[-1] == 40 and list(cs[::ncell]) == list(es)                # entry_start survives the sort; the last range is the live total
    np.testing.assert_array_equal(np.sort(order[:30]), np.arange(30))


def test_pack_unpack_round_trip_and_argument_errors():
    import torch
    from deep_fluids_amd import ops
    rng = np.random.RandomState(0)
    parts = [torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32)) for n in (5, 0, 2)]
    pos, es = ops.pack_particles(parts)
    assert tuple(pos.shape) == (9, 3) and es.dtype == torch.int32 and es.tolist() == [0, 5, 5, 7]
    back = ops.unpack_particles(pos, es)
    assert len(back) == 3 and all(torch.equal(a, b) for a, b in zip(back, parts))
    pos, es = ops.pack_particles(parts, capacity=12)
    assert tuple(pos.shape) == (12, 3) and all(torch.equal(a, b) for a, b in zip(ops.unpack_particles(pos, es), parts))
    ref_pos, ref_es = rr.pack([p.numpy() for p in parts], 12)
    np.testing.assert_array_equal(pos.numpy(), ref_pos)
    np.testing.assert_array_equal(es.numpy(), ref_es)
    for cap in (6, 10):                                                   # too small; not a multiple of B
        with pytest.raises(ValueError, match="capacity"):
            ops.pack_particles(parts, capacity=cap)
    with pytest.raises(ValueError):
        ops.pack_particles([])
    with pytest.raises(ValueError):
        ops.unpack_particles(pos, es.to(torch.int64))
    with pytest.raises(ValueError):
        ops.unpack_particles(pos, torch.tensor([0, 5, 4, 7], dtype=torch.int32))

    vel = torch.zeros((3, 6, 7, 8, 3))
    shape = (6, 7, 8)
    calls = (lambda p, e: ops.advect_particles(p, vel, 0.5, entry_start=e), lambda p, e: ops.particle_cells(p, shape, entry_start=e),
             lambda p, e: ops.flip_update(p, p, vel, vel, entry_start=e), lambda p, e: ops.sample_velocity(vel, p, entry_start=e),
             lambda p, e: ops.particle_levelset_averaged(p, shape, entry_start=e),
             lambda p, e: ops.resample_particles(p, p, None, e, None, None, vel, 2))
    es3 = torch.tensor([0, 3, 3, 5], dtype=torch.int32)
    for fn in calls:
        with pytest.raises(ValueError, match="multiple of B"):
            fn(torch.zeros((10, 3)), es3)                                   # P not a multiple of B
        with pytest.raises(ValueError, match="entry_start"):
            fn(torch.zeros((12, 3)), es3.to(torch.int64))                   # dtype
        with pytest.raises(ValueError, match="entry_start"):
            fn(torch.zeros((12, 3)), es3.view(1, 4))                        # shape
        with pytest.raises(ValueError, match="entry_start"):
            fn(torch.zeros((12, 3)), torch.zeros((1,), dtype=torch.int32))  # no entry at all
        with pytest.raises(ValueError):
            fn(torch.zeros((3, 4, 3)), es3)                                 # a dense [B,N,D] with entry_start
    # a wrong length is a wrong B: refused where P is no multiple of it (otherwise the velocity's batch size disagrees, on the GPU)
    with pytest.raises(ValueError, match="multiple of B"):
        ops.advect_particles(torch.zeros((12, 3)), vel, 0.5, entry_start=torch.tensor([0, 1, 2, 3, 4, 5], dtype=torch.int32))
    for kw in (dict(min_particles=2, max_particles=1), dict(min_particles=0), dict(min_particles=2, radius_factor=-1.0)):
        with pytest.raises(ValueError):
            ops.resample_particles(torch.zeros((12, 3)), torch.zeros((12, 3)), None, es3, None, None, vel, **kw)
    with pytest.raises(ValueError, match="max < min"):
        ops.resample_particles(torch.zeros((12, 3)), torch.zeros((12, 3)), None, es3, None, None, vel, 4, 3)
    for d in (-1, 255):
        with pytest.raises(ValueError, match="distance"):
            ops.extrapolate_levelset(torch.zeros((1, 6, 7)), distance=d)
    with pytest.raises(ValueError):
        ops.extrapolate_levelset(torch.zeros((6, 7)))
    for name in ("pack_particles", "unpack_particles", "extrapolate_levelset", "resample_particles"):
        assert name in ops.__all__


def initial_step_state(shape):
    """(pos, pvel [P,D], entry_start, vel0) of rr.step_scene, packed into twice the live total as ops.Resample's default capacity is"""
    parts, vel0 = rr.step_scene(shape)
    total = sum(len(q) for q in parts)
    P = -(-2 * total // rr.B) * rr.B
    pos, es = rr.pack(parts, P)
    pvel = np.zeros_like(pos)
    for b in range(rr.B):
        pvel[es[b]:es[b + 1]] = ref.sample(vel0[b:b + 1], parts[b][None], np.float32)[0]
    return pos, pvel, es, vel0


@pytest.mark.parametrize("case", [c for c in rr.STEP_CASES if c[0] in ("dam2d", "dam2d-gf-visc", "drop3d-gf")], ids=lambda c: c[0])
def test_the_step_twin_against_fp64_and_its_invariants(case):
    """what the GPU's step test rests on: from the same fp32 state the twin and the fp64 step sort, keep and seed alike, and every solve
    stops below the iteration cap; the step seeds and drops particles, so the counts change"""
    name, shape, gf, alpha = case
    D = len(shape)
    pos, pvel, es, vel = initial_step_state(shape)
    P = len(pos)
    cap = ref.default_max_iter(shape)
    changed = False
    for t in range(rr.STEP_T):
        kw = dict(ghost_fluid=gf, alpha=None if alpha is None else np.asarray(alpha), step_no=t)
        s32 = rr.step(pos, pvel, es, vel, rr.STEP_DT, rr.STEP_MIN_P[D], accuracy=rr.STEP_ACC, dtype=np.float32, **kw)
        s64 = rr.step(pos, pvel, es, vel, rr.STEP_DT, rr.STEP_MIN_P[D], accuracy=rr.STEP_ACC * 1e-3, dtype=np.float64, **kw)
        for k in ("cell_start", "entry_start"):
            np.testing.assert_array_equal(s32[k], s64[k])
        for k in ("keep", "kept", "seeds"):
            np.testing.assert_array_equal(s32["resampled"][k], s64["resampled"][k])
        assert (s32["iters"] < cap).all() and (s64["iters"] < cap).all()
        for s in (s32, s64):
            rr.check_invariants(s["resampled"], s["phi"], s["liquid"], rr.STEP_MIN_P[D], 2 * rr.STEP_MIN_P[D])
        e = [ref.max_err(s32[k], s64[k]) for k in ("vel", "pos", "pvel")]
        print("%s step %d: live %d -> %d  vel/pos/pvel twin-vs-fp64 %.3e %.3e %.3e" % ((name, t + 1, int(s32["resampled"]["old_cell_start"][-1]),
                                                                                      s32["total"]) + tuple(e)))
        assert max(e) <= 1e-5
        changed = changed or s32["resampled"]["seeds"].sum() > 0
        assert s32["total"] <= P
        pos, pvel, es, vel = rr.padded(s32["pos"], rr.B, P), rr.padded(s32["pvel"], rr.B, P), s32["entry_start"], s32["vel"]
    assert changed and list(np.diff(es)) != list(np.diff(initial_step_state(shape)[2]))


def test_step_arguments_without_a_gpu():
    import inspect
    import torch
    from deep_fluids_amd import data, ops
    for fn in (ops.liquid_step, ops.simulate_liquid):
        assert inspect.signature(fn).parameters["resample"].default is None
        with pytest.raises(ValueError, match="resample"):
            fn(None, None, None, 0.5, resample=dict(min_particles=2))
        with pytest.raises(ValueError, match="entry_start"):
            fn(None, None, None, 0.5, entry_start=torch.zeros((3,), dtype=torch.int32))
    for fn in (data.generate_liquid_dataset, data.generate_liquid3_d_r_dataset, data.generate_liquid3_vis_dataset):
        assert inspect.signature(fn).parameters["resample"].default is False
    rs = ops.Resample(3)
    assert (rs.min_particles, rs.max_particles, rs.seed, rs.capacity, rs.step) == (3, 6, 123, None, 0)
    for bad in (dict(min_particles=0), dict(min_particles=3, max_particles=2), dict(min_particles=2, capacity=0), dict(min_particles=2, capacity=2.5)):
        with pytest.raises(ValueError):
            ops.Resample(**bad)
    assert "Resample" in ops.__all__


def _lib_or_skip():
    from deep_fluids_amd import _lib
    return _lib, _lib.lib()


def test_cabi_rejections_before_the_device_is_touched():
    _lib, h = _lib_or_skip()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    q = p + 8192
    EINVAL = h.df_particles_advect2d(None, None, None, 1, 1, 8, 8, 0.5, 1.0, 1, None)     # a null velocity: the code for EINVAL
    assert EINVAL != 0
    ESHAPE = h.df_particles_advect2d(p, p, p, 1, 1, 2, 2, 0.5, 1.0, 1, None)              # an extent < 2*bnd + 2
    assert ESHAPE not in (0, EINVAL)

    def err():
        return h.df_last_error().decode()

    # ragged: null entry_start, null velocity, misaligned entry_start
    assert h.df_particles_advect2d_ragged(p, p, p, None, 2, 4, 8, 8, 0.5, 1.0, 1, None) == EINVAL and "entry_start" in err()
    assert h.df_particles_advect3d_ragged(p, p, None, p, 2, 4, 8, 8, 8, 0.5, 1.0, 1, None) == EINVAL
    assert h.df_particles_cell_keys2d_ragged(p, p, None, 2, 4, 8, 8, None) == EINVAL and "entry_start" in err()
    assert h.df_particles_cell_keys3d_ragged(p, p, p + 2, 2, 4, 8, 8, 8, None) not in (0, EINVAL, ESHAPE)       # alignment
    assert h.df_particles_cell_keys2d_ragged(p, p, p, 2, 4, 1, 8, None) == ESHAPE
    assert h.df_flip_update2d_ragged(p, p, p, p, p, None, 2, 4, 8, 8, 0.5, None) == EINVAL and "entry_start" in err()
    assert h.df_flip_update3d_ragged(p, p, p, p, p, p, 2, 4, 8, 8, 8, 1.5, None) == EINVAL and "flip_ratio" in err()
    assert h.df_flip_update2d_ragged(p, p, p, p, p, p, 0, 4, 8, 8, 0.5, None) == EINVAL
    # extrapolation
    assert h.df_levelset_extrapolate_marks2d(None, p, 1, 8, 8, 1, None) == EINVAL
    assert h.df_levelset_extrapolate_marks3d(p, None, 1, 8, 8, 8, 1, None) == EINVAL
    assert h.df_levelset_extrapolate_marks2d(p, q, 1, 8, 8, 2, None) == EINVAL and "inside" in err()
    assert h.df_levelset_extrapolate_marks2d(p, p, 1, 8, 8, 1, None) == EINVAL and "overlap" in err()
    assert h.df_levelset_extrapolate_marks2d(p, q, 1, 8, 1, 1, None) == ESHAPE
    for layer in (0, 1, 255):
        assert h.df_levelset_extrapolate_layer2d(p, q, 1, 8, 8, 1, layer, None) == EINVAL and "layer" in err()
    assert h.df_levelset_extrapolate_layer3d(None, q, 1, 8, 8, 8, 1, 2, None) == EINVAL
    assert h.df_levelset_extrapolate_layer3d(p, q, 1, 8, 8, 0, 1, 2, None) == EINVAL
    # resampling: nulls, counts, bnd, extents
    for k in range(7):                                                    # every pointer of the count pass is required
        a = [p, p, p, p, p, p, q]
        a[k] = None
        assert h.df_resample_count2d(*(a + [2, 4, 8, 8, 1, 2, 4, 1.0, None])) == EINVAL, k
    a = [p, p, p, p, p, p, q]
    assert h.df_resample_count2d(*(a + [2, 4, 8, 8, 1, 0, 4, 1.0, None])) == EINVAL and "min_particles" in err()
    assert h.df_resample_count2d(*(a + [2, 4, 8, 8, 1, 4, 3, 1.0, None])) == EINVAL and "max_particles" in err()
    assert h.df_resample_count3d(*(a + [2, 4, 8, 8, 8, 0, 2, 4, 1.0, None])) == EINVAL                         # bnd < 1
    assert h.df_resample_count3d(*(a + [2, 4, 8, 8, 3, 1, 2, 4, 1.0, None])) == ESHAPE
    assert h.df_resample_count2d(*(a + [2, 4, 8, 8, 1, 2, 4, -1.0, None])) == EINVAL and "radius_factor" in err()
    assert h.df_resample_count2d(*([p, p, p, p, p, p, p] + [2, 4, 8, 8, 1, 2, 4, 1.0, None])) == EINVAL         # kept is seeds
    assert h.df_resample_count2d(*(a + [1, 4, 46000, 46000, 1, 4096, 4096, 1.0, None])) == ESHAPE                # the total may overflow
    for k in range(9):
        b = [p, q, p, p, p, p, p, p + 16384 * 2, p + 16384 * 3]
        b[k] = None
        assert h.df_resample_scatter2d(*(b + [2, 4, 8, 8, 2, 1, 0, None])) == EINVAL, k
    b = [p, q, p, p, p, p, p, p, p + 16384 * 3]
    assert h.df_resample_scatter2d(*(b + [2, 4, 8, 8, 2, 1, 0, None])) == EINVAL and "overlap" in err()         # pos_out is pos
    b = [p, q, p, p, p, p, p, p + 16384 * 2, p + 16384 * 2]
    assert h.df_resample_scatter3d(*(b + [2, 4, 8, 8, 8, 2, 1, 0, None])) == EINVAL and "overlap" in err()      # the outputs coincide
    b = [p, q, p, p, p, p, p, p + 16384 * 2, p + 16384 * 3]
    assert h.df_resample_scatter3d(*(b + [2, 4, 8, 8, 8, 0, 1, 0, None])) == EINVAL
    assert h.df_resample_scatter2d(*(b + [2, -1, 8, 8, 2, 1, 0, None])) == EINVAL
