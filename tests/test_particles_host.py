"""Host side of the liquid step (no GPU): the fp32 twin of tests/particles_ref.py against its fp64 form on the cases the GPU tests run
(the printed e32 figures are quoted in tests/test_gpu_particles.py), the window form of the level set against the brute-force
minimum, the twin's exact cases, and the host helpers of deep_fluids_amd.ops (seeding, box and sphere level sets)."""
import numpy as np
import pytest

import particles_ref as ref


def test_twin_against_fp64_single_step():
    lo_hit, hi_hit = {2: set(), 3: set()}, {2: set(), 3: set()}
    for name, pos, vel, kw in ref.trace_cases():
        r64 = ref.trace(pos, vel, dtype=np.float64, **kw)
        r32 = ref.trace(pos, vel, dtype=np.float32, **kw)
        assert r32.dtype == np.float32 and r64.dtype == np.float64 and r32.shape == pos.shape
        e32 = ref.max_err(r32, r64)
        print("trace %-14s e32 %.3e" % (name, e32))
        assert e32 < 1e-4                                    # the twin is a restatement of the same step, not another one
        shape = vel.shape[1:-1]
        lo, hi = ref.clamp_bounds(shape, kw["bnd"], np.float32)
        assert (r32 >= lo).all() and (r32 <= hi).all()
        D = pos.shape[-1]
        for a in range(D):
            if (r32[..., a] == lo).any():
                lo_hit[D].add(a)
            if (r32[..., a] == hi[a]).any():
                hi_hit[D].add(a)
    # the fixtures carry particles out of every face
    for D in (2, 3):
        assert lo_hit[D] == set(range(D)) and hi_hit[D] == set(range(D)), (D, lo_hit[D], hi_hit[D])


def test_twin_against_fp64_sequence():
    for name, pos, vels, kw in ref.sequence_cases():
        assert vels.shape[0] == 8
        p64, phi64 = ref.sequence(pos, vels, dtype=np.float64, **kw)
        p32, phi32 = ref.sequence(pos, vels, dtype=np.float32, **kw)
        print("sequence %-8s e32 positions %.3e  last phi %.3e" % (name, ref.max_err(p32, p64), ref.max_err(phi32[-1], phi64[-1])))
        assert ref.max_err(p32, p64) < 1e-3 and ref.max_err(phi32[-1], phi64[-1]) < 1e-3
        assert float(phi64[-1].min()) < 0 < float(phi64[-1].max())


def test_levelset_twin_against_fp64():
    for name, shape, pos in ref.levelset_cases():
        for rf in ref.RADIUS_FACTORS:
            f64 = ref.levelset_brute(pos, shape, rf, np.float64)
            f32 = ref.levelset_brute(pos, shape, rf, np.float32)
            assert f32.dtype == np.float32 and f32.shape == (pos.shape[0],) + shape
            print("levelset %-12s rf %.1f  e32 %.3e" % (name, rf, ref.max_err(f32, f64)))
            assert ref.max_err(f32, f64) < 1e-5
            assert float(f64.max()) == float(ref.radius_of(len(shape), rf, np.float64))       # the grids keep empty regions


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_window_form_equals_brute_force(dtype):
    """2*radius <= w + 0.5 for the radius factors in use, so the +-w window over the cell index loses no particle that matters."""
    for name, shape, B, N, crowd in (("2d", (12, 9), 2, 400, 300), ("3d", (7, 8, 6), 2, 400, 300)):
        pos = ref.levelset_positions(shape, B, N, 7, crowd)
        keys = ref.cell_keys(pos, shape)
        counts = np.bincount(keys, minlength=B * int(np.prod(shape)))
        assert counts.max() >= 300 and (counts == 0).sum() > 0.3 * counts.size               # one crowded cell, many empty ones
        for rf in ref.RADIUS_FACTORS:
            D = len(shape)
            assert 2 * float(ref.radius_of(D, rf, np.float64)) <= ref.window_of(rf) + 0.5
            np.testing.assert_array_equal(ref.levelset_window(pos, shape, rf, dtype), ref.levelset_brute(pos, shape, rf, dtype))
    # no particles at all: phi = radius
    empty = np.zeros((2, 0, 2), np.float32)
    np.testing.assert_array_equal(ref.levelset_window(empty, (5, 4), 1.0, dtype), np.full((2, 5, 4), ref.radius_of(2, 1.0, dtype), dtype))


def test_window_form_is_the_definition_where_the_two_differ():
    """radius_factor 0.99 in 3-D: w = 1 but 2*radius = 1.73 > 1.5 -- a particle two cells away still lowers the brute-force minimum."""
    pos = np.array([[[3.05, 3.5, 3.5]]], np.float32)
    win = ref.levelset_window(pos, (7, 7, 7), 0.99, np.float64)
    bru = ref.levelset_brute(pos, (7, 7, 7), 0.99, np.float64)
    assert win[0, 3, 3, 1] == ref.radius_of(3, 0.99, np.float64) and bru[0, 3, 3, 1] < win[0, 3, 3, 1]
    assert (bru <= win).all()


def test_keys_and_ranges_restatement():
    pos = np.array([[[0.0, 0.0], [11.999, 8.999], [3.5, 2.25], [3.25, 2.75], [-1.0, 20.0], [np.nan, 1.0]]], np.float32)
    keys = ref.cell_keys(pos, (9, 12))
    np.testing.assert_array_equal(keys, [0, 8 * 12 + 11, 2 * 12 + 3, 2 * 12 + 3, 8 * 12 + 0, 12])
    order, start = ref.cell_ranges(keys, 9 * 12)
    np.testing.assert_array_equal(order, [0, 5, 2, 3, 4, 1])                               # stable: 2 stays ahead of 3
    assert start[0] == 0 and start[1] == 1 and start[27] == 2 and start[28] == 4 and start[-1] == 6 and start.size == 109


def test_twin_exact_cases():
    for shape in ((12, 9), (7, 8, 6)):
        D = len(shape)
        for bnd in (1, 2):
            pos = ref.make_positions(shape, 3, 257, bnd, 5)
            lo, hi = ref.clamp_bounds(shape, bnd, np.float32)
            inside = np.fmin(np.fmax(pos, lo), hi)
            zero = np.zeros((3,) + shape + (D,), np.float32)
            # zero velocity: positions inside the clamp stay bitwise
            got = ref.trace(inside, zero, 1.0, bnd, 1.0, np.float32)
            assert got.tobytes() == inside.tobytes()
            # a uniform field of 0.5 with dt = 1 moves every particle that stays inside the clamp by exactly 0.5 per axis (positions
            # on a 2^-10 lattice, so that p + 0.5 is exact)
            p = (np.round(inside * 1024) / 1024).astype(np.float32)
            p = np.fmin(np.fmax(p, lo), hi)
            half = np.full_like(zero, 0.5)
            for v, vs in ((half, 1.0), (half / 4, 4.0)):
                got = ref.trace(p, v, 1.0, bnd, vs, np.float32)
                want = np.fmin(p + np.float32(0.5), hi)
                assert got.tobytes() == want.astype(np.float32).tobytes()
                assert ((p + np.float32(0.5) <= hi) & (got - p == np.float32(0.5))).sum() > 0.5 * p.size
            np.testing.assert_array_equal(ref.trace(p, half, 1.0, bnd, 1.0, np.float64), np.fmin(p.astype(np.float64) + 0.5, hi))


def test_density_image_restatement():
    phi = np.array([[[-0.5, 0.0, 0.25], [0.5, 1.0, 2.0]]], np.float32)
    np.testing.assert_array_equal(ref.density_image(phi), [[[127, 255, 255], [0, 0, 63]]])
    phi3 = np.stack([phi, phi + np.float32(0.5)], axis=1)
    np.testing.assert_array_equal(ref.density_image(phi3), [[[191, 255, 255], [0, 63, 127]]])


# ---- host helpers of the package --------------------------------------------------------------------------------------------------
def test_box_and_sphere_levelsets():
    from deep_fluids_amd import ops
    box = ops.box_levelset((8, 10, 6), (1.8, 0.0, 1.8), (4.2, 8.0, 4.2))                    # grid [Z,Y,X] = 8, 10, 6; corners in xyz
    assert box.dtype == np.float32 and box.shape == (8, 10, 6)
    assert box[3, 4, 2] < 0 and box[3, 4, 3] < 0 and box[0, 4, 2] > 0 and box[3, 9, 2] > 0 and box[3, 4, 5] > 0
    assert box[3, 0, 2] < 0                                                                   # the box starts at y = 0
    assert abs(box[3, 4, 2] - (-0.7)) < 1e-6 and abs(box[3, 4, 5] - 1.3) < 1e-6              # centre 2.5: 0.7 inside; 5.5: 1.3 outside
    assert abs(box[3, 9, 5] - np.hypot(1.3, 1.5)) < 1e-6                                     # outside an edge: Euclidean
    sph = ops.sphere_levelset((9, 12), (6.0, 4.5), 3.0)
    assert sph.dtype == np.float32 and sph.shape == (9, 12)
    assert abs(sph[4, 5] - (0.5 - 3.0)) < 1e-6 and abs(sph[4, 11] - (5.5 - 3.0)) < 1e-6
    joined = np.minimum(ops.box_levelset((9, 12), (0, 0), (12, 2.0)), sph)
    assert (joined < 0).sum() > (sph < 0).sum()
    with pytest.raises(ValueError):
        ops.box_levelset((9, 12), (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError):
        ops.sphere_levelset((9, 12), (0, 0, 0), 1)


@pytest.mark.parametrize("shape", [(9, 12), (8, 10, 6)])
def test_seed_particles(shape):
    from deep_fluids_amd import ops
    D = len(shape)
    ext = shape[::-1]
    phi0 = ops.box_levelset(shape, [0.0] * D, [0.7 * e for e in ext])                        # reaches into the band at the low faces
    for disc, bnd in ((2, 1), (3, 2), (1, 1)):
        eligible = phi0 < 0
        for ax, n in enumerate(shape):
            idx = np.arange(n)
            sh = [1] * D
            sh[ax] = n
            eligible = eligible & ((idx >= bnd) & (idx < n - bnd)).reshape(sh)
        assert 0 < eligible.sum() < (phi0 < 0).sum()
        p = ops.seed_particles(phi0, discretization=disc, randomness=0.05, seed=9, bnd=bnd)
        assert p.dtype == np.float32 and p.shape == (disc ** D * int(eligible.sum()), D)
        cells = np.floor(p).astype(np.int64)
        assert eligible[tuple(cells[:, a] for a in reversed(range(D)))].all()                # every particle inside an eligible cell
        counts = np.zeros(shape, np.int64)
        np.add.at(counts, tuple(cells[:, a] for a in reversed(range(D))), 1)
        assert (counts[eligible] == disc ** D).all() and counts.sum() == p.shape[0]
        # ... inside its sub-cell, within the jitter of the sub-cell centre, and not all on it
        sub = np.floor((p - cells) * disc)
        off = np.abs((p - cells) - (sub + 0.5) / disc)
        assert off.max() <= 0.05 / disc + 1e-6 and off.max() > 0.01 / disc
        np.testing.assert_array_equal(p, ops.seed_particles(phi0, discretization=disc, randomness=0.05, seed=9, bnd=bnd))
        assert not np.array_equal(p, ops.seed_particles(phi0, discretization=disc, randomness=0.05, seed=10, bnd=bnd))
    assert ops.seed_particles(np.ones(shape, np.float32)).shape == (0, D)


def test_body_levelset_and_the_liquid3_vis_box():
    from types import SimpleNamespace
    from deep_fluids_amd import ops
    from deep_fluids_amd.trainer import body_levelset, liquid3_vis_body
    body = liquid3_vis_body(SimpleNamespace(is_3d=True))
    spatial = (10, 20, 10)
    phi = body_levelset(spatial, body)
    np.testing.assert_array_equal(phi, ops.box_levelset(spatial, (3.0, 0.0, 3.0), (7.0, 16.0, 7.0)))
    assert int((phi < 0).sum()) == 4 * 16 * 4
    both = body_levelset((9, 12), {"boxes": [((0, 0), (1.0, 0.25))], "spheres": [((0.5, 0.6), 0.1)]})
    np.testing.assert_array_equal(both, np.minimum(ops.box_levelset((9, 12), (0, 0), (12.0, 2.25)), ops.sphere_levelset((9, 12), (6.0, 5.4), 1.2)))
    np.testing.assert_array_equal(body_levelset((9, 12), both), both)
    with pytest.raises(ValueError):
        body_levelset((9, 12), {"cubes": []})
    with pytest.raises(ValueError):
        body_levelset((9, 13), both)
    with pytest.raises(ValueError):
        liquid3_vis_body(SimpleNamespace(is_3d=False))
