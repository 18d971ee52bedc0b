"""Host side of the smoke solver with open sides (no GPU): properties of the NumPy restatement the GPU tests compare against
(tests/smoke_open_ref.py) -- it guards the REFERENCE: that its projection really leaves every fluid cell divergence free, that a net
inflow is solvable once a side is open, that it reduces to smoke_ref / smoke_obs_ref bit for bit with no side open, the corner rule --
then ``ops.open_sides``, and the C-ABI surface of the new entry points with their argument checks (these need the built library and
fail on a tree without the feature)."""
import ctypes
import subprocess

import numpy as np
import pytest

import smoke_obs_ref as oref
import smoke_open_ref as pref
import smoke_ref as ref
from deep_fluids_amd import _lib, ops

OPENED = ["df_mac_advect_sl", "df_mac_advect_mc", "df_wall_buoyancy", "df_pressure_cg_direction", "df_pressure_correct"]
NEW = ["%s%dd_open" % (n, d) for n in OPENED for d in (2, 3)] + ["%s%dd" % (n, d) for n in ("df_open_extrapolate", "df_density_sphere_source")
                                                                 for d in (2, 3)]
SMALL = [((6, 6), 1), ((9, 7), 1), ((12, 10), 2), ((6, 6, 6), 1), ((7, 8, 6), 1), ((19, 10, 7), 2)]


# ---- the restatement against itself ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,bnd", SMALL)
def test_exact_projection_leaves_every_fluid_cell_divergence_free(shape, bnd):
    names, obs = pref.all_obstacles(shape, bnd)
    for spec, bits in pref.specs(len(shape)):
        w = pref.solve_input(shape, bnd, obs, bits)
        v, p = pref.exact_projection(w, obs, bits, bnd)
        fluid = oref.fluid_mask(obs, bnd)
        div = np.abs(pref.divergence(v, obs, bnd))[fluid]
        assert div.size and div.max() <= 1e-10, (spec, float(div.max()))
        assert not p[~fluid].any()
        opn = pref._opn(obs, bnd, bits)
        for a in range(len(shape)):                                   # non-live faces of fluid, solid and wall cells are exactly 0
            assert not v[..., a][~pref.live_mask(fluid, opn, a) & ~opn].any(), (spec, a)


@pytest.mark.parametrize("shape,bnd", [((9, 7), 1), ((7, 8, 6), 1)])
def test_a_net_inflow_is_solvable_with_an_open_side(shape, bnd):
    obs = np.zeros((1,) + shape, np.uint8)
    bits = pref.sides("Y", len(shape))
    w = pref.solve_input(shape, bnd, obs, bits, inflow=0.5)
    b = pref.rhs(w, obs, bnd)
    assert abs(float(b.sum())) > 1.0                                  # the flux through the open side: b does not sum to zero
    v, _ = pref.exact_projection(w, obs, bits, bnd)
    assert np.abs(pref.divergence(v, obs, bnd)).max() <= 1e-10
    A, _ = pref.dense_A(shape, bnd, obs[0], bits)
    assert np.linalg.eigvalsh(A).min() > 1e-6                         # non-singular SPD, where the closed box has the constant null vector
    A0, _ = pref.dense_A(shape, bnd, obs[0], 0)
    assert abs(np.linalg.eigvalsh(A0).min()) < 1e-10
    x, iters, r = pref.cg(w, obs, bits, bnd, 1e-4, ops.default_max_iter(shape), np.float32)
    assert iters[0] < ops.default_max_iter(shape) and np.abs(r).max() <= 1e-4


@pytest.mark.parametrize("shape,bnd", SMALL + [((17, 130), 1)])
def test_no_open_side_reproduces_the_closed_restatements_bit_for_bit(shape, bnd):
    D = len(shape)
    vel = ref.make_velocity(shape, seed=1, vmax=min(3.0, 0.4 * min(shape)))
    rho = ref.make_density(shape, seed=1)
    force = (0.013, 0.256, -0.07)[:D]
    zero = np.zeros((3,) + shape, np.uint8)
    for obs, closed in ((zero, None), (oref.mixed_batch(shape, bnd), "obs")):
        for dtype in (np.float32, np.float64):
            for mode in (1, 2):
                got = pref.mac_advect(vel, 1.0, obs, 0, clamp_mode=mode, bnd=bnd, dtype=dtype)
                want = (ref.mac_advect(vel, 1.0, clamp_mode=mode, bnd=bnd, dtype=dtype) if closed is None else
                        oref.mac_advect(vel, 1.0, obs, clamp_mode=mode, bnd=bnd, dtype=dtype))
                for k in ("out", "branch", "cell", "fwd"):
                    assert np.array_equal(got[k], want[k]), (k, mode)
            w = pref.wall_buoyancy(vel, rho, force, obs, 0, bnd, dtype)
            assert np.array_equal(w, ref.wall_buoyancy(vel, rho, force, bnd, dtype) if closed is None else oref.wall_buoyancy(vel, rho, force, obs, bnd, dtype))
            x, it, r = pref.cg(w, obs, 0, bnd, 0.0, 3, dtype)
            x0, it0, r0 = ref.cg(w, bnd, 0.0, 3, dtype) if closed is None else oref.cg(w, obs, bnd, 0.0, 3, dtype)
            assert np.array_equal(x, x0) and np.array_equal(it, it0) and np.array_equal(r, r0)
            c = pref.correct(w, x, obs, 0, bnd, dtype)
            assert np.array_equal(c, ref.correct(w, x, bnd, dtype) if closed is None else oref.correct(w, x, obs, bnd, dtype))
            assert np.array_equal(pref.extrapolate(c, 0, bnd), c)


def test_corner_rule_and_fill_sources():
    shape, bnd = (8, 9), 2
    o = pref.open_mask(shape, bnd, pref.sides("xX", 2))
    assert o[4, 0] and o[4, 1] and o[4, 8] and not o[4, 2]           # the x bands beside interior rows
    assert not o[0, 0] and not o[1, 8] and not o[0, 4]               # corners shared with the closed y sides, and the y bands: wall
    o = pref.open_mask(shape, bnd, pref.sides("xXyY", 2))
    assert o[0, 0] and o[7, 8] and (o | ref.interior_mask(shape, bnd)).all()
    o = pref.open_mask(shape, bnd, pref.sides("XyY", 2))
    assert not o[0, 0] and not o[4, 1] and o[0, 8] and o[0, 4]       # a corner with the closed x- side stays wall
    assert not pref.open_mask(shape, bnd, 0).any() and pref.wall_mask(shape, bnd, 0).sum() == 8 * 9 - 4 * 5
    assert pref.sides("xXyYzZ", 2) == 15 and pref.sides("xXyYzZ", 3) == 63 and pref.sides("XyY", 3) == 0b001110
    # the fill: a field that is its own index shows where every open cell reads from
    Y, X = shape
    v = np.zeros((1, Y, X, 2))
    v[0, ..., 0] = np.arange(Y)[:, None] * 100 + np.arange(X)[None]
    v[0, ..., 1] = v[0, ..., 0]
    f = pref.extrapolate(v, 15, bnd)
    assert f[0, 0, 0, 0] == 2 * 100 + 2 and f[0, 7, 8, 0] == 5 * 100 + 7 and f[0, 7, 8, 1] == 6 * 100 + 6
    assert f[0, 4, 7, 0] == 4 * 100 + 7 and f[0, 4, 8, 0] == 4 * 100 + 7 and f[0, 4, 7, 1] == 4 * 100 + 6
    assert np.array_equal(pref.extrapolate(f, 15, bnd), f)            # sources are fixed points: the fill is idempotent


def test_sphere_source_restatement_equals_the_mask():
    import advect_ref as aref
    for shape, c, r in (((9, 7), (3.125, 4.5), 2.25), ((6, 8, 7), (3.5, 4.25, 2.875), 2.5)):
        d = ref.make_density(shape, B=2, seed=3)
        centers = np.array([c, [float("nan")] * len(shape)], np.float32)
        for dtype in (np.float32, np.float64):
            got = pref.sphere_source(d, centers, r, 0.75, dtype)
            want = np.where(aref.sphere_mask_loop(shape, c, r), 0.75, d[0])
            assert np.array_equal(got[0], want.astype(dtype)) and np.array_equal(got[1], d[1].astype(dtype))


# ---- ops.open_sides ----------------------------------------------------------------------------------------------------------------------------
def test_open_sides_parsing():
    for dim in (2, 3):
        for closed in (None, False, "", 0):
            assert ops.open_sides(closed, dim) == 0
        assert ops.open_sides(True, dim) == (15 if dim == 2 else 63)
        for spec in ("Y", "xX", "XyY", "xXyY", "Xx"):
            assert ops.open_sides(spec, dim) == pref.sides(spec, dim)
    assert ops.open_sides("xXyYzZ", 3) == 63 and ops.open_sides("z", 3) == 16 and ops.open_sides(37, 3) == 37
    for bad, dim in (("xXyYzZ", 2), ("Z", 2), (16, 2), ("w", 3), (64, 3), (-1, 2), (1.5, 2), ("x", 4)):
        with pytest.raises(ValueError):
            ops.open_sides(bad, dim)
    import inspect
    for fn in ("advect_velocity", "wall_buoyancy", "solve_pressure", "smoke_step", "simulate_smoke"):
        assert inspect.signature(getattr(ops, fn)).parameters["open_bound"].default is None, fn
    assert "open_bound" not in inspect.signature(ops.advect).parameters            # the density needs nothing
    assert "open_sides" in ops.__all__ and "SphereSource" in ops.__all__
    s = ops.SphereSource([[[1.0, 2.0]], [[3.0, 4.0]]], 2.5)
    assert tuple(s.centers.shape) == (2, 1, 2) and s.frame(1).centers.tolist() == [[3.0, 4.0]] and s.frame(1).frame(7).centers.tolist() == [[3.0, 4.0]]
    with pytest.raises(ValueError):
        ops.SphereSource([1.0, 2.0], 1.0)
    with pytest.raises(ValueError):
        s.frame(2)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_open_entry_points():
    declared = _lib.declared_symbols()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NEW:
        assert name in declared and name in exported and name in _lib.SIGNATURES, name
    assert _lib.query("df_version") == 207
    from deep_fluids_amd import data, trainer
    assert callable(data.generate_smoke3_rot_dataset) and callable(data.generate_smoke3_mov_dataset) and callable(trainer.moving_source)


def test_argument_checks_of_the_open_entry_points():
    """every check runs before anything is launched, so fake (aligned, disjoint) addresses do"""
    h = _lib.lib()
    err = lambda: h.df_last_error()
    a, b, o, fl, ws = 0x10000, 0x20000, 0x30000, 0x40000, 0x100000
    need = h.df_pressure_workspace_bytes(1, 1, 8, 8)
    for bad in (-1, 64):                                              # open_sides outside 0..63
        assert h.df_mac_advect_sl2d_open(a, o, 1, 8, 8, 1.0, 1, bad, None) == -1 and b"open_sides" in err()
        assert h.df_mac_advect_mc3d_open(a, b, o, None, 1, 8, 8, 8, 1.0, 1, bad, 2, None) == -1 and b"open_sides" in err()
        assert h.df_wall_buoyancy2d_open(a, b, o, fl, 1, 8, 8, 0.0, 0.1, 1, bad, None) == -1 and b"open_sides" in err()
        assert h.df_pressure_cg_direction3d_open(ws, need * 8, None, 1, 8, 8, 8, 1, bad, 0, 1e-4, 10, None) == -1 and b"open_sides" in err()
        assert h.df_pressure_correct2d_open(a, b, o, None, 1, 8, 8, 1, bad, None) == -1 and b"open_sides" in err()
        assert h.df_open_extrapolate3d(a, 1, 8, 8, 8, 1, bad, None) == -1 and b"open_sides" in err()
    for zbits in (16, 32, 63):                                        # z bits in 2-D
        assert h.df_mac_advect_sl2d_open(a, o, 1, 8, 8, 1.0, 1, zbits, None) == -1 and b"z side" in err()
        assert h.df_mac_advect_mc2d_open(a, b, o, None, 1, 8, 8, 1.0, 1, zbits, 2, None) == -1 and b"z side" in err()
        assert h.df_wall_buoyancy2d_open(a, b, o, None, 1, 8, 8, 0.0, 0.1, 1, zbits, None) == -1 and b"z side" in err()
        assert h.df_pressure_cg_direction2d_open(ws, need, None, 1, 8, 8, 1, zbits, 0, 1e-4, 10, None) == -1 and b"z side" in err()
        assert h.df_pressure_correct2d_open(a, b, o, None, 1, 8, 8, 1, zbits, None) == -1 and b"z side" in err()
        assert h.df_open_extrapolate2d(a, 1, 8, 8, 1, zbits, None) == -1 and b"z side" in err()
    # those of the counterparts, with and without flags, open or not
    for osd in (0, 5):
        for f in (None, fl):
            assert h.df_mac_advect_mc2d_open(a, b, a, f, 1, 8, 8, 1.0, 1, osd, 2, None) == -1 and b"gathers" in err()
            assert h.df_mac_advect_mc2d_open(a, b, o, f, 1, 8, 8, 1.0, 1, osd, 3, None) == -1 and b"clamp_mode" in err()
            assert h.df_mac_advect_mc2d_open(None, b, o, f, 1, 8, 8, 1.0, 1, osd, 2, None) == -1
            assert h.df_mac_advect_mc3d_open(a, b, o, f, 1, 8, 8, 3, 1.0, 1, osd, 2, None) == -2
            assert h.df_mac_advect_mc2d_open(a, b, o + 2, f, 1, 8, 8, 1.0, 1, osd, 2, None) == -3
            assert h.df_wall_buoyancy2d_open(a, b, b, f, 1, 8, 8, 0.0, 0.1, 1, osd, None) == -1 and b"neighbour" in err()
            assert h.df_wall_buoyancy3d_open(a, b, o, f, 1, 8, 8, 8, 0.0, 0.1, 0.0, 0, osd, None) == -1 and b"boundary width" in err()
            assert h.df_pressure_cg_direction2d_open(ws, 16, f, 1, 8, 8, 1, osd, 0, 1e-4, 10, None) == -4
            assert h.df_pressure_cg_direction2d_open(None, need, f, 1, 8, 8, 1, osd, 0, 1e-4, 10, None) == -1
            assert h.df_pressure_cg_direction2d_open(ws, need, f, 1, 8, 8, 1, osd, -1, 1e-4, 10, None) == -1
            assert h.df_pressure_correct2d_open(a, b, b, f, 1, 8, 8, 1, osd, None) == -1 and b"neighbour" in err()
            assert h.df_pressure_correct3d_open(a, b, o, f, 1, 8, 8, 3, 1, osd, None) == -2
        assert h.df_mac_advect_mc2d_open(a, b, o, o + 100, 1, 8, 8, 1.0, 1, osd, 2, None) == -1 and b"flags overlap the output" in err()
        assert h.df_pressure_cg_direction2d_open(ws, need, ws + 16, 1, 8, 8, 1, osd, 0, 1e-4, 10, None) == -1 and b"workspace overlaps the flags" in err()
        assert h.df_mac_advect_sl2d_open(a, a, 1, 8, 8, 1.0, 1, osd, None) == -1 and b"gathers" in err()
        assert h.df_mac_advect_sl3d_open(a, o, 1, 8, 8, 3, 1.0, 1, osd, None) == -2
        assert h.df_open_extrapolate2d(None, 1, 8, 8, 1, osd, None) == -1
        assert h.df_open_extrapolate2d(a + 2, 1, 8, 8, 1, osd, None) == -3
        assert h.df_open_extrapolate3d(a, 1, 8, 8, 3, 1, osd, None) == -2
        assert h.df_open_extrapolate2d(a, 1, 8, 8, 0, osd, None) == -1
    assert h.df_open_extrapolate2d(a, 1, 8, 8, 1, 0, None) == 0      # no open side: nothing is launched, nothing written
    # df_density_sphere_source2d(density, centers, radius, value, out, B, Y, X, stream)
    assert h.df_density_sphere_source2d(a, b, 2.0, 1.0, None, 1, 8, 8, None) == -1
    assert h.df_density_sphere_source2d(a, None, 2.0, 1.0, o, 1, 8, 8, None) == -1 and b"centres" in err()
    assert h.df_density_sphere_source2d(a, o + 16, 2.0, 1.0, o, 1, 8, 8, None) == -1 and b"centres overlap the output" in err()
    assert h.df_density_sphere_source3d(a, o + 4 * 512 - 4, 2.0, 1.0, o, 1, 8, 8, 8, None) == -1 and b"centres overlap the output" in err()
    assert h.df_density_sphere_source2d(a, b, 2.0, 1.0, o, 0, 8, 8, None) == -1
    assert h.df_density_sphere_source2d(a, b + 2, 2.0, 1.0, o, 1, 8, 8, None) == -3
    assert h.df_density_sphere_source3d(a, b, 2.0, 1.0, o, 1, 1 << 24, 8, 8, None) == -2
