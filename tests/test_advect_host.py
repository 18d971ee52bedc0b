"""Host side of the density advection (no GPU): the C-ABI surface of advect.hip, its argument checks, properties of the NumPy
restatement the GPU tests compare against (tests/advect_ref.py), and the gate that keeps those tests' fixtures away from decisions that
flip by rounding."""
import ctypes
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import advect_ref as ref
from deep_fluids_amd import _lib, ops

NEW = ["df_advect_sl2d", "df_advect_sl3d", "df_advect_mc2d", "df_advect_mc3d", "df_density_source", "df_density_image2d",
       "df_density_image3d"]


# ---- (a) the header declares the entry points, the library exports them, the ctypes table binds them ---------------------------------
def test_header_declares_and_library_exports_the_advection_entry_points():
    declared = _lib.declared_symbols()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NEW:
        assert name in declared, name
        assert name in exported, name
        assert name in _lib.SIGNATURES, name
    assert _lib.lib().df_version() == 207
    for fn in ("advect", "advect_sequence", "density_image", "sphere_mask"):
        assert callable(getattr(ops, fn)) and fn in ops.__all__


# ---- (b) argument errors come back without a GPU ------------------------------------------------------------------------------------
def test_advection_entry_points_reject_bad_arguments_before_the_device():
    h = _lib.lib()
    buf = ctypes.create_string_buffer(8192)
    a = (ctypes.addressof(buf) + 15) & ~15
    b, c, o = a + 1024, a + 2048, a + 4096
    f = ctypes.c_float
    # df_advect_sl2d(density, vel, fwd, B, Y, X, dt, vel_scale, bnd, stream)
    assert h.df_advect_sl2d(None, b, o, 1, 8, 8, f(.5), f(1), 1, None) == -1
    assert b"null input" in h.df_last_error()
    assert h.df_advect_sl2d(a, None, o, 1, 8, 8, f(.5), f(1), 1, None) == -1
    assert b"velocity" in h.df_last_error()
    assert h.df_advect_sl2d(a, b, None, 1, 8, 8, f(.5), f(1), 1, None) == -1
    assert b"output" in h.df_last_error()
    assert h.df_advect_sl2d(a, b, o, 1, 0, 8, f(.5), f(1), 1, None) == -1
    assert h.df_advect_sl2d(a, b, o, 1, 8, 8, f(.5), f(1), 0, None) == -1
    assert b"boundary width" in h.df_last_error()
    assert h.df_advect_sl2d(a, b, a, 1, 8, 8, f(.5), f(1), 1, None) == -1           # in place: the step gathers
    assert b"gathers" in h.df_last_error()
    assert h.df_advect_sl2d(a, b, o, 1, 3, 8, f(.5), f(1), 1, None) == -2           # 2*bnd + 2 = 4 > 3
    assert b"2*bnd + 2" in h.df_last_error()
    assert h.df_advect_sl2d(a, b, o, 1, 8, 5, f(.5), f(1), 2, None) == -2
    assert h.df_advect_sl2d(a + 2, b, o, 1, 8, 8, f(.5), f(1), 1, None) == -3
    assert b"aligned" in h.df_last_error()
    # df_advect_sl3d(density, vel, fwd, B, Z, Y, X, dt, vel_scale, bnd, stream)
    assert h.df_advect_sl3d(None, b, o, 1, 8, 8, 8, f(.5), f(1), 1, None) == -1
    assert h.df_advect_sl3d(a, b, o, 1, 3, 8, 8, f(.5), f(1), 1, None) == -2
    assert h.df_advect_sl3d(a, b, o, 1, 8, 8, 8, f(.5), f(1), -1, None) == -1
    # df_advect_mc2d(orig, fwd, vel, out, B, Y, X, dt, vel_scale, bnd, clamp_mode, stream)
    assert h.df_advect_mc2d(None, b, c, o, 1, 8, 8, f(.5), f(1), 1, 2, None) == -1
    assert h.df_advect_mc2d(a, b, c, None, 1, 8, 8, f(.5), f(1), 1, 2, None) == -1
    for mode in (0, 3):
        assert h.df_advect_mc2d(a, b, c, o, 1, 8, 8, f(.5), f(1), 1, mode, None) == -1
        assert b"clamp_mode" in h.df_last_error()
    assert h.df_advect_mc2d(a, b, c, b, 1, 8, 8, f(.5), f(1), 1, 2, None) == -1      # out aliases fwd
    assert h.df_advect_mc2d(a, b, c, o, 1, 8, 3, f(.5), f(1), 1, 2, None) == -2
    assert h.df_advect_mc2d(a, b, c, o + 1, 1, 8, 8, f(.5), f(1), 1, 2, None) == -3
    # df_advect_mc3d(orig, fwd, vel, out, B, Z, Y, X, dt, vel_scale, bnd, clamp_mode, stream)
    assert h.df_advect_mc3d(a, None, c, o, 1, 8, 8, 8, f(.5), f(1), 1, 2, None) == -1
    assert h.df_advect_mc3d(a, b, c, o, 1, 8, 8, 8, f(.5), f(1), 1, 5, None) == -1
    assert h.df_advect_mc3d(a, b, c, o, 1, 8, 5, 8, f(.5), f(1), 2, 1, None) == -2
    # df_density_source(density, mask, value, out, n, stream)
    assert h.df_density_source(None, b, f(1), o, 16, None) == -1
    assert h.df_density_source(a, None, f(1), o, 16, None) == -1
    assert b"mask" in h.df_last_error()
    assert h.df_density_source(a, b, f(1), o, 0, None) == -1
    assert h.df_density_source(a, b, f(1), o + 2, 16, None) == -3
    # df_density_image2d(density, img, B, Y, X, stream) / df_density_image3d(density, img, B, Z, Y, X, stream)
    assert h.df_density_image2d(None, o, 1, 4, 4, None) == -1
    assert b"null input" in h.df_last_error()
    assert h.df_density_image2d(a, None, 1, 4, 4, None) == -1
    assert b"null output" in h.df_last_error()
    assert h.df_density_image2d(a, o, 1, 0, 4, None) == -1
    assert h.df_density_image3d(a, o, 1, 4, 4, 0, None) == -1
    assert h.df_density_image3d(a + 1, o, 1, 4, 4, 4, None) == -3


def test_python_surface_of_the_advection_fails_loudly_without_gpu():
    import torch
    with pytest.raises(ValueError):
        ops.advect(torch.zeros((1, 8, 8)), torch.zeros((1, 8, 8, 2)), 0.5, order=3)
    with pytest.raises(ValueError):
        ops.advect(torch.zeros((1, 8, 8)), torch.zeros((1, 8, 8, 2)), 0.5, clamp_mode=0)
    if torch.cuda.is_available():
        return          # with a GPU the calls below are exercised by tests/test_gpu_advect.py
    with pytest.raises(_lib.DeepFluidsHipError):
        ops.advect(torch.zeros((1, 8, 8)), torch.zeros((1, 8, 8, 2)), 0.5)
    with pytest.raises(_lib.DeepFluidsHipError):
        ops.advect_sequence(torch.zeros((1, 8, 8, 8)), torch.zeros((2, 1, 8, 8, 8, 3)), 0.5)
    with pytest.raises(_lib.DeepFluidsHipError):
        ops.density_image(torch.zeros((1, 8, 8)))


# ---- (c) properties of the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(12, 9), (7, 8, 6)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_zero_velocity_is_the_identity_on_interior_cells(shape, dtype):
    rng = np.random.RandomState(1)
    d = rng.uniform(0, 1, (2,) + shape).astype(np.float32)
    v = np.zeros((2,) + shape + (len(shape),), np.float32)
    for bnd in (1, 2):
        inter = ref.interior_mask(shape, bnd)[None]
        want = np.where(inter, d, 0)
        for order, mode in ((1, 2), (2, 1), (2, 2)):
            r = ref.step(d, v, 0.5, order=order, clamp_mode=mode, bnd=bnd, dtype=dtype)
            np.testing.assert_array_equal(r["out"], want.astype(dtype))
            assert r["out"].dtype == dtype
            assert set(np.unique(r["branch"][np.broadcast_to(inter, d.shape)])) <= {ref.FWD, ref.COR}
            assert (r["branch"][np.broadcast_to(~inter, d.shape)] == ref.BAND).all()


@pytest.mark.parametrize("shape", [(12, 10), (8, 9, 10)])
def test_uniform_integer_displacement_shifts_exactly(shape):
    d, v, shift = ref.exact_shift_inputs(shape)
    for dtype in (np.float64, np.float32):
        for bnd in (1, 2):
            r = ref.step(d, v, 0.5, order=1, bnd=bnd, dtype=dtype)
            np.testing.assert_array_equal(r["out"], ref.shifted(d, shift, bnd).astype(dtype))
    # the fp32 twin of the MacCormack step equals fp64 bit for bit on these inputs (nothing rounds)
    for mode in (1, 2):
        r64 = ref.step(d, v, 0.5, order=2, clamp_mode=mode, dtype=np.float64)
        r32 = ref.step(d, v, 0.5, order=2, clamp_mode=mode, dtype=np.float32)
        np.testing.assert_array_equal(r32["out"].astype(np.float64), r64["out"])
        np.testing.assert_array_equal(r32["branch"], r64["branch"])


def test_mode_2_keeps_the_density_inside_the_unit_interval():
    for name, fx, kw in ref.single_step_cases():
        if kw["order"] != 2 or kw["clamp_mode"] != 2:
            continue
        assert fx["density"].min() >= 0 and fx["density"].max() <= 1
        r = ref.step(fx["density"], fx["vels"][0], fx["dt"], vel_scale=fx["vel_scale"], source=fx["source"], dtype=np.float32, **kw)
        assert r["out"].min() >= 0 and r["out"].max() <= 1, name


def test_sphere_mask_against_a_brute_force_loop():
    for shape, center, radius in (((12, 9), (4.2, 6.0), 3.3), ((7, 8, 6), (3.0, 4.5, 3.5), 2.5), ((5, 5), (2.5, 2.5), 0.4),
                                  ((6, 7), (-3.0, 2.0), 2.0)):
        m = ops.sphere_mask(shape, center, radius)
        assert m.dtype.is_floating_point is False and tuple(m.shape) == shape
        np.testing.assert_array_equal(m.numpy(), ref.sphere_mask_loop(shape, center, radius))
    assert ops.sphere_mask((5, 5), (2.5, 2.5), 0.4).sum() == 1        # the one cell whose centre is the sphere's


def test_density_image_host_formula():
    d = np.array([[[0.0, 0.5, 1.0, 2.0], [-1.0, 0.999, 0.1, 0.25]]], np.float32)
    np.testing.assert_array_equal(ref.density_image(d), [[[0, 254, 25, 63], [0, 127, 255, 255]]])


def test_smoke_pos_size_source(tmp_path):
    from deep_fluids_amd.data import BatchManager, write_synthetic_dataset
    from deep_fluids_amd.trainer import smoke_pos_size_source
    root = str(tmp_path)
    write_synthetic_dataset(root, (16, 8), num_p=(3, 2), num_frames=4)
    cfg = SimpleNamespace(random_seed=1, data_path=root, is_3d=False, data_type="velocity", arch="de", batch_size=2, res_x=8, res_y=16, res_z=1)
    bm = BatchManager(cfg, device=None)
    with pytest.raises(KeyError, match="src_y_pos"):                    # the synthetic dataset's args.txt has no src_y_pos
        smoke_pos_size_source(bm, 1, 1)
    bm.args["src_y_pos"] = "0.1"
    s = smoke_pos_size_source(bm, 1, 1)
    assert s["center"] == (8 * (1 / 2.0 * (0.8 - 0.2) + 0.2), 16 * 0.1) and s["radius"] == 8 * (1 / 1.0 * (0.12 - 0.04) + 0.04)


# ---- (d) the fixture gate: the fp32 twin alone leaves out at most 0.05 % of the interior cells on every fixture -----------------------
def test_fixture_gate_single_steps():
    n = 0
    for name, fx, kw in ref.single_step_cases():
        args = dict(vel_scale=fx["vel_scale"], source=fx["source"], **kw)
        r64 = ref.step(fx["density"], fx["vels"][0], fx["dt"], dtype=np.float64, **args)
        r32 = ref.step(fx["density"], fx["vels"][0], fx["dt"], dtype=np.float32, **args)
        e32, share = ref.twin_error(r64, r32, kw["bnd"])
        reach = float(np.abs(fx["vels"][0]).max() * fx["vel_scale"] * fx["dt"])
        print("%-36s e32 %.3e  left out %.5f %%  reach %.2f cells  reverts %d" % (name, e32, 100 * share, reach, int((r64["branch"] == ref.FWD).sum())))
        assert share <= 5e-4, (name, share)
        assert 0 < e32 < 1e-4, (name, e32)
        # the rule of the GPU test, applied to the twin: what it asks of the kernel is within reach of fp32 arithmetic in this order
        ref.compare(r32["out"], r64, e32, kw["bnd"], ref.alternatives_of(r64, fx["vels"][0], fx["dt"], kw["clamp_mode"], kw["bnd"], fx["vel_scale"]))
        assert reach > 4                                   # traces reach the band
        n += 1
    assert n == 3 * 2 * 3 * 2


def test_fixture_gate_sequences():
    for name, fx, kw in ref.sequence_cases():
        args = dict(vel_scale=fx["vel_scale"], source=fx["source"], **kw)
        s64 = ref.sequence(fx["density"], fx["vels"], fx["dt"], dtype=np.float64, **args)
        s32 = ref.sequence(fx["density"], fx["vels"], fx["dt"], dtype=np.float32, **args)
        worst = max(ref.twin_error(a, b, kw["bnd"])[1] for a, b in zip(s64, s32))
        e32, share = ref.twin_error(s64[-1], s32[-1], kw["bnd"])
        print("%-36s e32 %.3e  left out %.5f %% (worst step %.5f %%)" % (name, e32, 100 * share, 100 * worst))
        assert share <= 5e-4 and worst <= 5e-4, (name, share, worst)
        assert 0 < e32 < 1e-4, (name, e32)
        ref.compare(s32[-1]["out"], s64[-1], e32, kw["bnd"], ref.alternatives_of(s64[-1], fx["vels"][-1], fx["dt"], kw["clamp_mode"], kw["bnd"], fx["vel_scale"]))
