"""Host side of the smoke solver step (no GPU): the C-ABI surface of smoke.hip, its argument checks, properties of the NumPy restatement
the GPU tests compare against (tests/smoke_ref.py), and the gate that keeps the MAC-advection fixtures away from decisions that flip by
rounding."""
import ctypes
import subprocess

import numpy as np
import pytest

import advect_ref as aref
import smoke_ref as ref
from deep_fluids_amd import _lib, ops

NEW = ["df_mac_advect_sl2d", "df_mac_advect_sl3d", "df_mac_advect_mc2d", "df_mac_advect_mc3d", "df_wall_buoyancy2d", "df_wall_buoyancy3d",
       "df_pressure_workspace_bytes", "df_pressure_init2d", "df_pressure_init3d", "df_pressure_cg_direction2d", "df_pressure_cg_direction3d",
       "df_pressure_cg_update2d", "df_pressure_cg_update3d", "df_pressure_status", "df_pressure_correct2d", "df_pressure_correct3d"]


def test_header_declares_and_library_exports_the_smoke_entry_points():
    declared = _lib.declared_symbols()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NEW:
        assert name in declared, name
        assert name in exported, name
        assert name in _lib.SIGNATURES, name
    assert _lib.lib().df_version() == 207
    for fn in ("advect_velocity", "wall_buoyancy", "solve_pressure", "smoke_step", "simulate_smoke", "pressure_workspace", "default_buoyancy_force",
               "default_max_iter"):
        assert callable(getattr(ops, fn)) and fn in ops.__all__
    from deep_fluids_amd import data
    assert callable(data.generate_smoke_dataset)


def test_smoke_entry_points_reject_bad_arguments_before_the_device():
    h = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    a = (ctypes.addressof(buf) + 15) & ~15
    b, c, o, ws = a + 4096, a + 8192, a + 12288, a + 16384
    f = ctypes.c_float
    err = h.df_last_error
    # df_mac_advect_sl2d(vel, fwd, B, Y, X, dt, bnd, stream)
    assert h.df_mac_advect_sl2d(None, o, 1, 8, 8, f(.5), 1, None) == -1 and b"velocity" in err()
    assert h.df_mac_advect_sl2d(a, None, 1, 8, 8, f(.5), 1, None) == -1 and b"output" in err()
    assert h.df_mac_advect_sl2d(a, o, 1, 0, 8, f(.5), 1, None) == -1
    assert h.df_mac_advect_sl2d(a, o, 1, 8, 8, f(.5), 0, None) == -1 and b"boundary width" in err()
    assert h.df_mac_advect_sl2d(a, a, 1, 8, 8, f(.5), 1, None) == -1 and b"gathers" in err()
    assert h.df_mac_advect_sl2d(a, o, 1, 3, 8, f(.5), 1, None) == -2 and b"2*bnd + 2" in err()
    assert h.df_mac_advect_sl2d(a, o, 1, 8, 5, f(.5), 2, None) == -2
    assert h.df_mac_advect_sl2d(a + 2, o, 1, 8, 8, f(.5), 1, None) == -3 and b"aligned" in err()
    assert h.df_mac_advect_sl3d(None, o, 1, 8, 8, 8, f(.5), 1, None) == -1
    assert h.df_mac_advect_sl3d(a, o, 1, 3, 8, 8, f(.5), 1, None) == -2
    assert h.df_mac_advect_sl3d(a, o, 1, 8, 8, 8, f(.5), -1, None) == -1
    # df_mac_advect_mc2d(vel, fwd, out, B, Y, X, dt, bnd, clamp_mode, stream)
    assert h.df_mac_advect_mc2d(None, b, o, 1, 8, 8, f(.5), 1, 2, None) == -1
    assert h.df_mac_advect_mc2d(a, None, o, 1, 8, 8, f(.5), 1, 2, None) == -1
    assert h.df_mac_advect_mc2d(a, b, None, 1, 8, 8, f(.5), 1, 2, None) == -1
    for mode in (0, 3):
        assert h.df_mac_advect_mc2d(a, b, o, 1, 8, 8, f(.5), 1, mode, None) == -1 and b"clamp_mode" in err()
    assert h.df_mac_advect_mc2d(a, b, b, 1, 8, 8, f(.5), 1, 2, None) == -1 and b"gathers" in err()
    assert h.df_mac_advect_mc2d(a, b, a, 1, 8, 8, f(.5), 1, 2, None) == -1
    assert h.df_mac_advect_mc2d(a, b, o, 1, 8, 3, f(.5), 1, 2, None) == -2
    assert h.df_mac_advect_mc2d(a, b, o + 1, 1, 8, 8, f(.5), 1, 2, None) == -3
    assert h.df_mac_advect_mc3d(a, b, o, 1, 8, 8, 8, f(.5), 1, 5, None) == -1
    assert h.df_mac_advect_mc3d(a, b, o, 1, 8, 5, 8, f(.5), 2, 1, None) == -2
    # df_wall_buoyancy2d(vel, density, out, B, Y, X, fx, fy, bnd, stream)
    assert h.df_wall_buoyancy2d(None, b, o, 1, 8, 8, f(0), f(1), 1, None) == -1 and b"velocity" in err()
    assert h.df_wall_buoyancy2d(a, None, o, 1, 8, 8, f(0), f(1), 1, None) == -1 and b"density" in err()
    assert h.df_wall_buoyancy2d(a, b, None, 1, 8, 8, f(0), f(1), 1, None) == -1
    assert h.df_wall_buoyancy2d(a, b, b, 1, 8, 8, f(0), f(1), 1, None) == -1 and b"neighbour" in err()
    assert h.df_wall_buoyancy2d(a, b, o, 1, 8, 8, f(0), f(1), 0, None) == -1
    assert h.df_wall_buoyancy2d(a, b, o, 1, 8, 3, f(0), f(1), 1, None) == -2
    assert h.df_wall_buoyancy2d(a, b + 1, o, 1, 8, 8, f(0), f(1), 1, None) == -3
    assert h.df_wall_buoyancy3d(a, b, o, 1, 8, 8, 5, f(0), f(1), f(0), 2, None) == -2
    assert h.df_wall_buoyancy3d(a, b, o, 0, 8, 8, 8, f(0), f(1), f(0), 1, None) == -1
    # df_pressure_workspace_bytes(B, Z, Y, X): r, p, p, q + 3 partials per workgroup of 256 cells + 2 records of 32 bytes per entry
    assert h.df_pressure_workspace_bytes(3, 1, 17, 130) == 4 * (4 * 3 * 17 * 130 + 3 * 3 * 9 + 2 * 3 * 8)
    assert h.df_pressure_workspace_bytes(1, 6, 6, 6) == 4 * (4 * 216 + 3 + 16)
    assert h.df_pressure_workspace_bytes(0, 1, 8, 8) == -1
    need = h.df_pressure_workspace_bytes(1, 1, 8, 8)
    # df_pressure_init2d(vel, pressure, ws, ws_bytes, B, Y, X, bnd, stream)
    assert h.df_pressure_init2d(None, o, ws, need, 1, 8, 8, 1, None) == -1 and b"velocity" in err()
    assert h.df_pressure_init2d(a, None, ws, need, 1, 8, 8, 1, None) == -1 and b"pressure" in err()
    assert h.df_pressure_init2d(a, o, None, need, 1, 8, 8, 1, None) == -1 and b"workspace" in err()
    assert h.df_pressure_init2d(a, o, ws, need - 4, 1, 8, 8, 1, None) == -4
    assert h.df_pressure_init2d(a, a, ws, need, 1, 8, 8, 1, None) == -1 and b"neighbour" in err()
    assert h.df_pressure_init2d(a, o, ws, need, 1, 8, 3, 1, None) == -2
    assert h.df_pressure_init2d(a, o, ws, need, 1, 8, 8, 0, None) == -1
    assert h.df_pressure_init2d(a, o + 2, ws, need, 1, 8, 8, 1, None) == -3
    assert h.df_pressure_init2d(a, o, ws + 1, need, 1, 8, 8, 1, None) == -3
    assert h.df_pressure_init2d(a, o, a + 256, need, 1, 8, 8, 1, None) == -1 and b"overlaps the velocity" in err()
    assert h.df_pressure_init2d(a, o, o - need + 4, need, 1, 8, 8, 1, None) == -1 and b"overlaps the pressure" in err()
    assert h.df_pressure_init3d(a, o, ws, 64, 1, 8, 8, 8, 1, None) == -4
    assert h.df_pressure_init3d(a, o, ws, 1 << 20, 1, 8, 8, 5, 2, None) == -2
    # df_pressure_cg_direction2d(ws, ws_bytes, B, Y, X, bnd, k, accuracy, max_iter, stream)
    assert h.df_pressure_cg_direction2d(None, need, 1, 8, 8, 1, 0, f(1e-4), 10, None) == -1
    assert h.df_pressure_cg_direction2d(ws, need - 1, 1, 8, 8, 1, 0, f(1e-4), 10, None) == -4
    assert h.df_pressure_cg_direction2d(ws, need, 1, 8, 8, 1, -1, f(1e-4), 10, None) == -1
    assert h.df_pressure_cg_direction2d(ws, need, 1, 8, 8, 1, 0, f(-1), 10, None) == -1 and b"accuracy" in err()
    assert h.df_pressure_cg_direction2d(ws, need, 1, 8, 8, 1, 0, f(1e-4), -2, None) == -1
    assert h.df_pressure_cg_direction2d(ws, need, 1, 2, 8, 1, 0, f(1e-4), 10, None) == -2
    assert h.df_pressure_cg_direction3d(ws, 16, 1, 8, 8, 8, 1, 0, f(1e-4), 10, None) == -4
    # df_pressure_cg_update2d(pressure, ws, ws_bytes, B, Y, X, bnd, k, stream)
    assert h.df_pressure_cg_update2d(None, ws, need, 1, 8, 8, 1, 0, None) == -1
    assert h.df_pressure_cg_update2d(o, None, need, 1, 8, 8, 1, 0, None) == -1
    assert h.df_pressure_cg_update2d(o, ws, need - 4, 1, 8, 8, 1, 0, None) == -4
    assert h.df_pressure_cg_update2d(o, ws, need, 1, 8, 8, 1, -3, None) == -1
    assert h.df_pressure_cg_update2d(o + 1, ws, need, 1, 8, 8, 1, 0, None) == -3
    assert h.df_pressure_cg_update2d(ws + 64, ws, need, 1, 8, 8, 1, 0, None) == -1 and b"overlaps the pressure" in err()
    assert h.df_pressure_cg_update3d(o, ws, 16, 1, 8, 8, 8, 1, 0, None) == -4
    # df_pressure_status(ws, ws_bytes, B, Z, Y, X, k, active_count, iterations, stream)
    assert h.df_pressure_status(None, need, 1, 1, 8, 8, 0, o, None, None) == -1
    assert h.df_pressure_status(ws, need - 4, 1, 1, 8, 8, 0, o, None, None) == -4
    assert h.df_pressure_status(ws, need, 1, 1, 8, 8, 0, None, None, None) == -1 and b"null outputs" in err()
    assert h.df_pressure_status(ws, need, 1, 1, 8, 8, 0, o + 2, None, None) == -3
    assert h.df_pressure_status(ws, need, 1, 0, 8, 8, 0, o, None, None) == -1
    assert h.df_pressure_status(ws, need, 1, 1, 8, 8, 0, ws + need - 4, None, None) == -1 and b"overlaps the active count" in err()
    assert h.df_pressure_status(ws, need, 1, 1, 8, 8, 0, o, ws + 8, None) == -1 and b"overlaps the iteration counts" in err()
    # df_pressure_correct2d(vel, pressure, out, B, Y, X, bnd, stream)
    assert h.df_pressure_correct2d(None, b, o, 1, 8, 8, 1, None) == -1
    assert h.df_pressure_correct2d(a, None, o, 1, 8, 8, 1, None) == -1 and b"pressure" in err()
    assert h.df_pressure_correct2d(a, b, None, 1, 8, 8, 1, None) == -1
    assert h.df_pressure_correct2d(a, b, b, 1, 8, 8, 1, None) == -1 and b"neighbour" in err()
    assert h.df_pressure_correct2d(a, b, o, 1, 3, 8, 1, None) == -2
    assert h.df_pressure_correct2d(a, b, o, 1, 8, 8, 0, None) == -1
    assert h.df_pressure_correct2d(a, b, o + 2, 1, 8, 8, 1, None) == -3
    assert h.df_pressure_correct3d(a, b, o, 1, 8, 8, 3, 1, None) == -2


def test_python_surface_of_the_smoke_step_fails_loudly_without_gpu():
    import torch
    v, d = torch.zeros((1, 8, 8, 2)), torch.zeros((1, 8, 8))
    if torch.cuda.is_available():
        return          # with a GPU these calls are exercised by tests/test_gpu_smoke.py
    for fn in (lambda: ops.advect_velocity(v, 0.5), lambda: ops.wall_buoyancy(v, d, (0, 1)), lambda: ops.solve_pressure(v),
               lambda: ops.smoke_step(d, v, 0.5), lambda: ops.simulate_smoke(d, v, 2)):
        with pytest.raises(_lib.DeepFluidsHipError):
            fn()


def test_default_force_and_max_iter():
    assert ops.default_buoyancy_force((128, 96), 0.5) == (0.0, 4e-3 * 0.5 * 128)
    assert ops.default_buoyancy_force((12, 16, 12), 0.5) == (0.0, 4e-3 * 0.5 * 16, 0.0) == ref.default_force((12, 16, 12), 0.5)
    assert ops.default_max_iter((128, 96)) == 5120 and ops.default_max_iter((64, 96, 64)) == 960


# ---- properties of the restatement -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,bnd", [((6, 6), 1), ((9, 7), 1), ((12, 10), 2), ((6, 6, 6), 1), ((7, 8, 6), 1)])
def test_A_is_symmetric_with_zero_row_sums_and_the_exact_projection_is_divergence_free(shape, bnd):
    A, cells = ref.dense_A(shape, bnd)
    assert cells.size == int(ref.interior_mask(shape, bnd).sum())
    np.testing.assert_array_equal(A, A.T)
    np.testing.assert_array_equal(A.sum(axis=1), 0)
    assert (np.diag(A) >= 2).all()
    rng = np.random.RandomState(2)
    vel = ref.make_velocity(shape, B=2, seed=3)
    rho = rng.uniform(0, 1, (2,) + shape).astype(np.float32)
    for dtype in (np.float64, np.float32):
        w = ref.wall_buoyancy(vel, rho, (0.1, 0.25, -0.05)[:len(shape)], bnd, dtype)
        for a in range(len(shape)):
            assert (w[..., a][:, ~ref.face_mask(shape, bnd, a)] == 0).all()
        b = ref.rhs(w, bnd, np.float64)
        assert abs(b.sum()) <= 1e-12 * np.abs(b).sum() + 1e-30           # the face differences telescope to the (zero) wall faces
    w = ref.wall_buoyancy(vel, rho, (0.1, 0.25, -0.05)[:len(shape)], bnd, np.float64)
    vp, p = ref.exact_projection(w, bnd)
    div = float(np.abs(ref.divergence(vp, bnd)).max())
    print("%s bnd %d: %d unknowns, max|div| after the exact projection %.3e" % (shape, bnd, cells.size, div))
    assert div < 1e-12
    # fp64 CG run to the end agrees with it
    v64, _, it = ref.solve_pressure(w, bnd, 1e-13, 10 * cells.size, np.float64)
    assert np.abs(v64 - vp).max() < 1e-10, it


@pytest.mark.parametrize("shape", [(8, 6), (6, 7, 6)])
def test_rest_is_a_fixed_point(shape):
    d0 = np.zeros((2,) + shape, np.float32)
    v0 = np.zeros((2,) + shape + (len(shape),), np.float32)
    for dtype in (np.float64, np.float32):
        d, v, _, _ = ref.step(d0, v0, 0.5, dtype=dtype)
        assert not d.any() and not v.any() and not np.isnan(v).any()
    x, iters, r = ref.cg(v0, 1, 1e-4, 50, np.float32)
    assert not x.any() and not iters.any()


def test_cg_freezes_converged_entries():
    shape = (9, 7)
    v = ref.walled(ref.make_velocity(shape, B=3, seed=5), 1)
    v[0] = 0
    v[1] *= 1e-3
    x, iters, _ = ref.cg(v, 1, 1e-4, 500, np.float64)
    assert iters[0] == 0 and not x[0].any() and 0 < iters[1] < iters[2]
    for e in range(3):
        xe, ie, _ = ref.cg(v[e:e + 1], 1, 1e-4, 500, np.float64)
        np.testing.assert_array_equal(xe[0], x[e])
        assert ie[0] == iters[e]


# ---- the fixture gate: the fp32 twin alone leaves out at most 0.05 % of the components on every MAC-advection fixture ----------------------
def test_fixture_gate_mac_advection():
    n = 0
    for name, vel, kw in ref.mac_cases():
        r64 = ref.mac_advect(vel, ref.MAC_DT, dtype=np.float64, **kw)
        r32 = ref.mac_advect(vel, ref.MAC_DT, dtype=np.float32, **kw)
        e32, share = aref.twin_error(r64, r32, kw["bnd"])
        reach = float(np.abs(vel).max() * ref.MAC_DT)
        print("%-24s e32 %.3e  left out %.5f %%  reach %.2f cells  corrected %d  reverted or wall-side %d" %
              (name, e32, 100 * share, reach, int((r64["branch"] == aref.COR).sum()), int((r64["branch"] == aref.FWD).sum())))
        assert share <= 5e-4, (name, share)
        assert 0 < e32 < 1e-4, (name, e32)
        aref.compare(r32["out"], r64, e32, kw["bnd"], ref.mac_alternatives(r64, vel, ref.MAC_DT, kw["clamp_mode"], kw["bnd"]))
        assert reach > 1.5                                  # traces leave their cell and reach the wall band
        n += 1
    assert n == 10 * 3
