"""Host side of the smoke solver around obstacles (no GPU): the C-ABI surface of the `_flags` entry points and their argument checks,
properties of the NumPy restatement the GPU tests compare against (tests/smoke_obs_ref.py), and the gate that keeps the masked
advection fixtures away from decisions that flip by rounding.

The tests from "properties of the restatement" down touch NumPy only: they guard the REFERENCE (that it reduces to smoke_ref with no
obstacle, that its systems are consistent, that its fixtures are decidable), not the kernels, and pass without the library.  The
tests above them need the new symbols and keywords."""
import ctypes
import subprocess

import numpy as np
import pytest

import advect_ref as aref
import smoke_obs_ref as oref
import smoke_ref as ref
from deep_fluids_amd import _lib, ops

FLAGGED = ["df_advect_mc", "df_mac_advect_mc", "df_wall_buoyancy", "df_pressure_init", "df_pressure_cg_direction", "df_pressure_cg_update",
           "df_pressure_correct"]
NEW = ["df_obstacle_flags2d", "df_obstacle_flags3d"] + ["%s%dd_flags" % (n, d) for n in FLAGGED for d in (2, 3)]
SMALL = [((6, 6), 1), ((9, 7), 1), ((12, 10), 2), ((6, 6, 6), 1), ((7, 8, 6), 1)]


def test_header_declares_and_library_exports_the_obstacle_entry_points():
    declared = _lib.declared_symbols()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NEW:
        assert name in declared and name in exported and name in _lib.SIGNATURES, name
    assert callable(ops.obstacle_flags) and "obstacle_flags" in ops.__all__
    import inspect
    for fn in ("advect", "advect_sequence", "advect_velocity", "wall_buoyancy", "solve_pressure", "smoke_step", "simulate_smoke"):
        assert inspect.signature(getattr(ops, fn)).parameters["obstacle"].default is None, fn
    from deep_fluids_amd import data, trainer
    assert callable(data.generate_smoke3_obs_dataset) and callable(trainer.smoke3_obs_buo_scene)
    par = inspect.signature(trainer.Trainer.advect_).parameters["obstacle"]
    assert par.default is None and par.kind is par.KEYWORD_ONLY


def test_flags_entry_points_reject_bad_arguments_before_the_device():
    h = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    a = (ctypes.addressof(buf) + 15) & ~15
    b, c, o, ws, fl = a + 4096, a + 8192, a + 12288, a + 16384, a + 40960
    f = ctypes.c_float
    err = h.df_last_error
    # df_obstacle_flags2d(obstacle, flags, B, Y, X, bnd, stream)
    assert h.df_obstacle_flags2d(None, fl, 1, 8, 8, 1, None) == -1 and b"obstacle" in err()
    assert h.df_obstacle_flags2d(a, None, 1, 8, 8, 1, None) == -1 and b"flags" in err()
    assert h.df_obstacle_flags2d(a, a, 1, 8, 8, 1, None) == -1 and b"overlap" in err()
    assert h.df_obstacle_flags2d(a, a + 63, 1, 8, 8, 1, None) == -1 and b"overlap" in err()
    assert h.df_obstacle_flags2d(a, fl, 1, 8, 8, 0, None) == -1 and b"boundary width" in err()
    assert h.df_obstacle_flags2d(a, fl, 0, 8, 8, 1, None) == -1
    assert h.df_obstacle_flags2d(a, fl, 1, 3, 8, 1, None) == -2 and b"2*bnd + 2" in err()
    assert h.df_obstacle_flags3d(a, fl, 1, 8, 8, 5, 2, None) == -2
    assert h.df_obstacle_flags3d(None, fl, 1, 8, 8, 8, 1, None) == -1
    # df_advect_mc2d_flags(orig, fwd, vel, out, flags, B, Y, X, dt, vel_scale, bnd, clamp_mode, stream)
    assert h.df_advect_mc2d_flags(a, b, c, o, None, 1, 8, 8, f(.5), f(1), 1, 2, None) == -1 and b"null flags" in err()
    assert h.df_advect_mc2d_flags(None, b, c, o, fl, 1, 8, 8, f(.5), f(1), 1, 2, None) == -1
    assert h.df_advect_mc2d_flags(a, b, c, o, o + 255, 1, 8, 8, f(.5), f(1), 1, 2, None) == -1 and b"flags overlap the output" in err()
    assert h.df_advect_mc2d_flags(a, b, c, a, fl, 1, 8, 8, f(.5), f(1), 1, 2, None) == -1 and b"gathers" in err()
    assert h.df_advect_mc2d_flags(a, b, c, o, fl, 1, 8, 8, f(.5), f(1), 1, 3, None) == -1 and b"clamp_mode" in err()
    assert h.df_advect_mc2d_flags(a, b, c, o, fl, 1, 8, 3, f(.5), f(1), 1, 2, None) == -2
    assert h.df_advect_mc2d_flags(a, b, c, o + 2, fl, 1, 8, 8, f(.5), f(1), 1, 2, None) == -3
    assert h.df_advect_mc3d_flags(a, b, c, o, None, 1, 8, 8, 8, f(.5), f(1), 1, 2, None) == -1
    assert h.df_advect_mc3d_flags(a, b, c, o, fl, 1, 8, 8, 5, f(.5), f(1), 2, 2, None) == -2
    # df_mac_advect_mc2d_flags(vel, fwd, out, flags, B, Y, X, dt, bnd, clamp_mode, stream)
    assert h.df_mac_advect_mc2d_flags(a, b, o, None, 1, 8, 8, f(.5), 1, 2, None) == -1 and b"null flags" in err()
    assert h.df_mac_advect_mc2d_flags(a, b, o, o + 511, 1, 8, 8, f(.5), 1, 2, None) == -1 and b"flags overlap the output" in err()
    assert h.df_mac_advect_mc2d_flags(a, b, b, fl, 1, 8, 8, f(.5), 1, 2, None) == -1 and b"gathers" in err()
    assert h.df_mac_advect_mc2d_flags(a, b, o, fl, 1, 8, 8, f(.5), 1, 0, None) == -1
    assert h.df_mac_advect_mc2d_flags(a, b, o + 1, fl, 1, 8, 8, f(.5), 1, 2, None) == -3
    assert h.df_mac_advect_mc3d_flags(a, b, o, None, 1, 8, 8, 8, f(.5), 1, 2, None) == -1
    assert h.df_mac_advect_mc3d_flags(a, b, o, fl, 1, 8, 3, 8, f(.5), 1, 2, None) == -2
    # df_wall_buoyancy2d_flags(vel, density, out, flags, B, Y, X, fx, fy, bnd, stream)
    assert h.df_wall_buoyancy2d_flags(a, b, o, None, 1, 8, 8, f(0), f(1), 1, None) == -1 and b"null flags" in err()
    assert h.df_wall_buoyancy2d_flags(a, b, o, o, 1, 8, 8, f(0), f(1), 1, None) == -1 and b"flags overlap the output" in err()
    assert h.df_wall_buoyancy2d_flags(a, b, b, fl, 1, 8, 8, f(0), f(1), 1, None) == -1 and b"neighbour" in err()
    assert h.df_wall_buoyancy2d_flags(a, None, o, fl, 1, 8, 8, f(0), f(1), 1, None) == -1 and b"density" in err()
    assert h.df_wall_buoyancy2d_flags(a, b, o, fl, 1, 8, 8, f(0), f(1), 0, None) == -1
    assert h.df_wall_buoyancy3d_flags(a, b, o, None, 1, 8, 8, 8, f(0), f(1), f(0), 1, None) == -1
    assert h.df_wall_buoyancy3d_flags(a, b, o, fl, 1, 8, 8, 5, f(0), f(1), f(0), 2, None) == -2
    need = h.df_pressure_workspace_bytes(1, 1, 8, 8)
    # df_pressure_init2d_flags(vel, pressure, ws, ws_bytes, flags, B, Y, X, bnd, stream)
    assert h.df_pressure_init2d_flags(a, o, ws, need, None, 1, 8, 8, 1, None) == -1 and b"null flags" in err()
    assert h.df_pressure_init2d_flags(a, o, ws, need, o + 8, 1, 8, 8, 1, None) == -1 and b"flags overlap the pressure" in err()
    assert h.df_pressure_init2d_flags(a, o, ws, need, ws + need - 1, 1, 8, 8, 1, None) == -1 and b"workspace overlaps the flags" in err()
    assert h.df_pressure_init2d_flags(None, o, ws, need, fl, 1, 8, 8, 1, None) == -1 and b"velocity" in err()
    assert h.df_pressure_init2d_flags(a, o, ws, need - 4, fl, 1, 8, 8, 1, None) == -4
    assert h.df_pressure_init2d_flags(a, o, ws, need, fl, 1, 8, 3, 1, None) == -2
    assert h.df_pressure_init3d_flags(a, o, ws, 1 << 20, None, 1, 8, 8, 8, 1, None) == -1
    # df_pressure_cg_direction2d_flags(ws, ws_bytes, flags, B, Y, X, bnd, k, accuracy, max_iter, stream)
    assert h.df_pressure_cg_direction2d_flags(ws, need, None, 1, 8, 8, 1, 0, f(1e-4), 10, None) == -1 and b"null flags" in err()
    assert h.df_pressure_cg_direction2d_flags(ws, need, ws, 1, 8, 8, 1, 0, f(1e-4), 10, None) == -1 and b"workspace overlaps the flags" in err()
    assert h.df_pressure_cg_direction2d_flags(ws, need, fl, 1, 8, 8, 1, 0, f(-1), 10, None) == -1 and b"accuracy" in err()
    assert h.df_pressure_cg_direction2d_flags(ws, need - 1, fl, 1, 8, 8, 1, 0, f(1e-4), 10, None) == -4
    assert h.df_pressure_cg_direction3d_flags(ws, 1 << 20, None, 1, 8, 8, 8, 1, 0, f(1e-4), 10, None) == -1
    # df_pressure_cg_update2d_flags(pressure, ws, ws_bytes, flags, B, Y, X, bnd, k, stream)
    assert h.df_pressure_cg_update2d_flags(o, ws, need, None, 1, 8, 8, 1, 0, None) == -1 and b"null flags" in err()
    assert h.df_pressure_cg_update2d_flags(o, ws, need, o + 255, 1, 8, 8, 1, 0, None) == -1 and b"flags overlap the pressure" in err()
    assert h.df_pressure_cg_update2d_flags(o, ws, need, ws + 16, 1, 8, 8, 1, 0, None) == -1 and b"workspace overlaps the flags" in err()
    assert h.df_pressure_cg_update2d_flags(None, ws, need, fl, 1, 8, 8, 1, 0, None) == -1
    assert h.df_pressure_cg_update2d_flags(o, ws, need, fl, 1, 8, 8, 1, -3, None) == -1
    assert h.df_pressure_cg_update3d_flags(o, ws, 16, fl, 1, 8, 8, 8, 1, 0, None) == -4
    # df_pressure_correct2d_flags(vel, pressure, out, flags, B, Y, X, bnd, stream)
    assert h.df_pressure_correct2d_flags(a, b, o, None, 1, 8, 8, 1, None) == -1 and b"null flags" in err()
    assert h.df_pressure_correct2d_flags(a, b, o, o + 100, 1, 8, 8, 1, None) == -1 and b"flags overlap the output" in err()
    assert h.df_pressure_correct2d_flags(a, b, b, fl, 1, 8, 8, 1, None) == -1 and b"neighbour" in err()
    assert h.df_pressure_correct2d_flags(a, b, o + 2, fl, 1, 8, 8, 1, None) == -3
    assert h.df_pressure_correct3d_flags(a, b, o, None, 1, 8, 8, 8, 1, None) == -1
    assert h.df_pressure_correct3d_flags(a, b, o, fl, 1, 8, 8, 3, 1, None) == -2


def test_python_surface_validates_and_fails_loudly_without_gpu(tmp_path):
    import torch
    from deep_fluids_amd.data import generate_smoke3_obs_dataset
    with pytest.raises(NotImplementedError):
        generate_smoke3_obs_dataset(str(tmp_path / "open"), open_bound=True)
    with pytest.raises(ValueError):
        generate_smoke3_obs_dataset(str(tmp_path / "names"), p0="src_x_pos")
    with pytest.raises(ValueError):
        generate_smoke3_obs_dataset(str(tmp_path / "names"), p1="src_radius")
    with pytest.raises(ValueError):
        generate_smoke3_obs_dataset(str(tmp_path / "names"), num_param=2)
    assert not (tmp_path / "open").exists() and not (tmp_path / "names").exists()
    from types import SimpleNamespace
    from deep_fluids_amd.trainer import smoke3_obs_buo_scene
    with pytest.raises(KeyError, match="not a smoke3_obs_buo scene"):
        smoke3_obs_buo_scene(SimpleNamespace(args={"src_x_pos": "0.5"}, root="somewhere", res_x=8, res_y=8, res_z=8), 0, 0)
    if torch.cuda.is_available():
        return          # with a GPU these calls are exercised by tests/test_gpu_smoke_obstacles.py
    v, d, o = torch.zeros((1, 8, 8, 2)), torch.zeros((1, 8, 8)), torch.zeros((1, 8, 8), dtype=torch.uint8)
    for fn in (lambda: ops.wall_buoyancy(v, d, (0, 1), obstacle=o), lambda: ops.solve_pressure(v, obstacle=o),
               lambda: ops.smoke_step(d, v, 0.5, obstacle=o)):
        with pytest.raises((_lib.DeepFluidsHipError, RuntimeError, AssertionError)):
            fn()


def test_flags_stay_flags_through_views_and_copies_and_nothing_else():
    import torch
    t = torch.tensor([[[1, 3], [5, 0]], [[1, 1], [0, 0]]], dtype=torch.uint8).as_subclass(ops.ObstacleFlags)
    t.bnd = 2
    for x in (t[1:2], t[0][None], t.clone(), t.detach(), t.contiguous(), t.to("cpu", copy=True), t[:1].expand(3, 2, 2).contiguous()):
        assert isinstance(x, ops.ObstacleFlags) and x.bnd == 2 and x.dtype == torch.uint8
    for x in (t & 1, t != 0, t + t, t.float(), t.as_subclass(torch.Tensor), torch.from_numpy(t.numpy())):
        assert type(x) is torch.Tensor                               # computed from flags: a mask or a number again
    # a slice of flags is taken for flags (a mask of these bytes would turn every fluid cell solid), with its own checks
    assert ops._obstacle_arg(t[1:2], (1, 2, 2), 2, "test") .data_ptr() == t[1:2].data_ptr()
    with pytest.raises(ValueError, match="built for bnd=2"):
        ops._obstacle_arg(t, (2, 2, 2), 1, "test")
    with pytest.raises(ValueError, match="do not fit"):
        ops._obstacle_arg(t, (3, 2, 2), 2, "test")
    with pytest.raises(ValueError, match="packed already"):
        ops.obstacle_flags(t, 2)


# ---- properties of the restatement -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,bnd", SMALL + [((17, 130), 2), ((19, 10, 7), 2)])
def test_zero_obstacle_equals_the_unmasked_restatement_exactly(shape, bnd):
    D = len(shape)
    zero = np.zeros((3,) + shape, np.uint8)
    vel = ref.make_velocity(shape, seed=1, vmax=min(3.0, 0.4 * min(shape)))
    rho = ref.make_density(shape, seed=1)
    inter = ref.interior_mask(shape, bnd)
    np.testing.assert_array_equal(oref.fluid_mask(zero, bnd), np.broadcast_to(inter, zero.shape))
    fl = oref.flags(zero, bnd)
    assert ((fl & 1) == inter).all()
    for a in range(D):
        np.testing.assert_array_equal(oref.face_mask(oref.fluid_mask(zero, bnd), a)[0], ref.face_mask(shape, bnd, a))
        assert (((fl >> (1 + 2 * a)) & 1)[0][inter] == ref.face_mask(shape, bnd, a)[inter]).all()
    for dtype in (np.float64, np.float32):
        for order, mode in ((1, 2), (2, 1), (2, 2)):
            kw = dict(order=order, clamp_mode=mode, bnd=bnd, dtype=dtype)
            r, ro = ref.mac_advect(vel, 1.0, **kw), oref.mac_advect(vel, 1.0, zero, **kw)
            d, do = aref.step(rho, vel, 1.0, **kw), oref.advect_density(rho, vel, 1.0, zero, **kw)
            for k in ("out", "branch", "cell", "fwd", "cor", "orig"):
                np.testing.assert_array_equal(ro[k], r[k])
                np.testing.assert_array_equal(do[k], d[k])
        force = (0.013, 0.256, -0.07)[:D]
        w = ref.wall_buoyancy(vel, rho, force, bnd, dtype)
        np.testing.assert_array_equal(oref.wall_buoyancy(vel, rho, force, zero, bnd, dtype), w)
        np.testing.assert_array_equal(oref.rhs(w, zero, bnd, dtype), ref.rhs(w, bnd, dtype))
        x = ref.rhs(w, bnd, dtype)
        np.testing.assert_array_equal(oref.apply_A(x, zero, bnd), ref.apply_A(x, bnd))
        got, want = oref.cg(w, zero, bnd, 1e-4, 6, dtype), ref.cg(w, bnd, 1e-4, 6, dtype)
        for g, t in zip(got, want):
            np.testing.assert_array_equal(g, t)
        np.testing.assert_array_equal(oref.correct(w, want[0], zero, bnd, dtype), ref.correct(w, want[0], bnd, dtype))
    if int(inter.sum()) <= 200:
        np.testing.assert_array_equal(oref.dense_A(shape, bnd, zero[0])[0], ref.dense_A(shape, bnd)[0])


@pytest.mark.parametrize("shape,bnd", SMALL)
def test_rhs_sums_to_zero_per_region_and_the_exact_projection_is_divergence_free(shape, bnd):
    D = len(shape)
    cases = oref.obstacle_cases(shape, bnd)
    assert {"cell", "block", "split", "enclosed", "solid"} <= set(cases)
    names = sorted(cases)
    obs = oref.batch_obstacle(shape, bnd, names)
    B = len(names)
    rng = np.random.RandomState(2)
    vel = ref.make_velocity(shape, B=B, seed=3)
    rho = rng.uniform(0, 1, (B,) + shape).astype(np.float32)
    w = oref.wall_buoyancy(vel, rho, (0.1, 0.25, -0.05)[:D], obs, bnd, np.float64)
    fluid = oref.fluid_mask(obs, bnd)
    b = oref.rhs(w, obs, bnd, np.float64)
    nc = oref.neighbour_count(obs, bnd)
    for e, name in enumerate(names):
        lab, n = oref.regions(fluid[e])
        assert n == {"solid": 0, "split": 2, "enclosed": 2}.get(name, 1), (name, n)
        for r in range(n):
            assert abs(b[e][lab == r].sum()) <= 1e-12 * np.abs(b[e]).sum() + 1e-30       # faces telescope to zero solid faces
        A, cells = oref.dense_A(shape, bnd, obs[e])
        assert cells.size == int(fluid[e].sum())
        np.testing.assert_array_equal(A, A.T)
        np.testing.assert_array_equal(A.sum(axis=1), 0)
        np.testing.assert_array_equal(np.diag(A), nc[e].reshape(-1)[cells])
        if cells.size:
            assert np.linalg.matrix_rank(A) == cells.size - n                             # singular once per region
    e = names.index("enclosed")
    mid = tuple(n // 2 for n in shape)
    assert fluid[e][mid] and nc[e][mid] == 0 and b[e][mid] == 0 and not w[e][mid].any()
    for a in range(D):
        assert (w[..., a][~oref.face_mask(fluid, a)] == 0).all()
    vp, p = oref.exact_projection(w, obs, bnd)
    div = float(np.abs(oref.divergence(vp, obs, bnd)).max())
    print("%s bnd %d: max|div| in fluid cells after the exact projection %.3e" % (shape, bnd, div))
    assert div < 1e-12
    for a in range(D):
        assert (vp[..., a][~oref.face_mask(fluid, a)] == 0).all()
    # the enclosed cell's row of A is zero: the minimum-norm solution is 0 there, up to the rounding of the dense factorisation
    assert not p[~fluid].any() and abs(p[e][mid]) < 1e-12 and not p[names.index("solid")].any()
    # fp64 CG run to the end agrees with it; the all-solid entry stops at iteration 0, the enclosed cell keeps p = 0
    v64, x64, it = oref.solve_pressure(w, obs, bnd, 1e-13, 20 * int(np.prod(shape)), np.float64)
    assert np.abs(v64 - vp).max() < 1e-9, it
    assert it[names.index("solid")] == 0 and x64[e][mid] == 0 and np.isfinite(x64).all()


# ---- the fixture gate: the fp32 twin alone leaves out at most 0.05 % of the cells on every masked advection fixture --------------------------
@pytest.mark.parametrize("kind", ["mac", "density"])
def test_fixture_gate_masked_advection(kind):
    n = 0
    for name, vel, rho, obs, kw in oref.advect_cases(kind):
        if kind == "mac":
            r64 = oref.mac_advect(vel, oref.OBS_DT, obs, dtype=np.float64, **kw)
            r32 = oref.mac_advect(vel, oref.OBS_DT, obs, dtype=np.float32, **kw)
            alt = oref.mac_alternatives(r64, vel, oref.OBS_DT, kw["clamp_mode"], kw["bnd"], obs)
        else:
            r64 = oref.advect_density(rho, vel, oref.OBS_DT, obs, dtype=np.float64, **kw)
            r32 = oref.advect_density(rho, vel, oref.OBS_DT, obs, dtype=np.float32, **kw)
            alt = oref.alternatives(r64, vel, oref.OBS_DT, kw["clamp_mode"], kw["bnd"], obs)
        e32, share = aref.twin_error(r64, r32, kw["bnd"])
        print("%-28s e32 %.3e  left out %.5f %%  corrected %d  fwd %d  no fluid corner %d" %
              (name, e32, 100 * share, int((r64["branch"] == aref.COR).sum()), int((r64["branch"] == aref.FWD).sum()),
               int((r64["branch"] == aref.NOCORNER).sum())))
        assert share <= 5e-4, (name, share)
        assert 0 < e32 < 1e-4, (name, e32)
        aref.compare(r32["out"], r64, e32, kw["bnd"], alt)
        n += 1
    assert n == 10 * 2
